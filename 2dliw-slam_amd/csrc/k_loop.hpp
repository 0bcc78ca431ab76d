// k_loop.hpp — interface between the loop detector's host code (liw_loop.cpp) and its kernels (k_loop.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace liw_loop_dev {

constexpr int kDraws = 5;        // max_match_times (keyframe_manager.cpp:1141)
constexpr int kMaxBins = 256;    // nAngle + 1 bins of the per-task LDS histogram
constexpr int kRowsPerBlock = 16;

struct Cand {                    // one launched candidate
    int slot;                    // key-frame index of the candidate feature
    int n2;                      // its points
    int rows[kDraws];            // drawn query rows, -1 for a repeated draw
    int pad;
};

struct Geom {                    // store strides and the matching constants
    int P, W, nb, orign, thr;
    double a_res;
};

constexpr double kPi = 3.14159265358979323846;

// ---- row routines shared by k_loop.hip and k_loop_batch.hip (both include this header under fp contract(off))
// match_des's bin of a pair: wrap the angle difference to [-pi, pi), truncate toward zero, shift by nAngle / 2.  Clamped to
// the histogram (finite inputs never leave it: |bin - orign| <= int(pi / a_res) < orign).
__device__ __forceinline__ int angle_bin(double a1, double a2, double a_res, int orign, int nb) {
    double d = a1 - a2;
    if (d >= kPi) d -= kPi * 2;
    else if (d < -kPi) d += kPi * 2;
    const double q = d / a_res;
    int b = (q == q) ? (int)q : 0;
    b += orign;
    return b < 0 ? 0 : (b >= nb ? nb - 1 : b);
}

// first index in keys[0, n) with keys[e] >= v (keys ascending)
__device__ __forceinline__ int lower_bound_u32(const uint32_t* keys, int n, uint32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one wave per point of slot `slot`: rows of (dij << 12 | j) keys, aij and quick_des; inv[slot] = 1 on a dij overflow
int launch_describe(const double* pts, int n, int slot, const Geom& g, double d_res, uint32_t* keys, double* aij, uint64_t* quick, int* inv,
                    hipStream_t s);
// one task per (candidate, draw, row); tres[(c * kDraws + d) * P + r] = {size, bin | quick_pass << 16}
int launch_match(const Cand* cands, int ncand, int max_n2, int qslot, int n1, const Geom& g, const uint32_t* keys, const double* aij,
                 const uint64_t* quick, int2* tres, hipStream_t s);
// one wave per candidate: the first task of maximal size; summary[c * 8 + .] = {size, draw, row, bin, quick_pass, list length};
// lists[(c * P + e) * 2 + .] = the correspondences (query point, candidate point) of winners with size > thr
int launch_select(const Cand* cands, int ncand, int qslot, int n1, const Geom& g, const uint32_t* keys, const double* aij, const int2* tres,
                  int* summary, int* lists, hipStream_t s);

}  // namespace liw_loop_dev
