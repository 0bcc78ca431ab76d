// k_loop.hpp — interface between the loop detector's host code (liw_loop.cpp) and its kernels (k_loop.hip); the device bodies that
// k_loop.hip shares with the fleet's k_loop_batch.hip are in k_loop_dev.hpp.
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

// The draws of the query rows (include/liw_loop.h): one function for the host's make_cand and the fleet's k_floop_gates.
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// draw d of query key frame q against candidate key frame c: a row of the query's n1
__host__ __device__ inline int draw_row(uint64_t seed, int q, int c, int d, int n1) {
    return (int)(splitmix64(seed ^ ((uint64_t)q << 40) ^ ((uint64_t)c << 8) ^ (uint64_t)d) % (uint64_t)n1);
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
