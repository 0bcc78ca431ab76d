// k_loop_dev.hpp — the loop detector's algorithm, once: the device bodies that k_loop.hip (one robot) and k_loop_batch.hip (the
// fleet) both call.  The kernels of the two files only compute addresses (Cand and a slot there, Pair, feature_slot and a robot
// region here), loop over their items and call these bodies with plain pointers and sizes.
//
//   describe_point  one wave, one point i of a sub-map: lanes over j build dij = int(|p_j - p_i| / d_res + 0.5) and aij
//                   (keyframe_manager.cpp:945-1032), the 32-bit keys dij << 12 | j are bitonic-sorted in LDS (= the (dij, j)
//                   order), aij is gathered by j, quick_des is or-ed together in LDS.
//   match_rows      one work-group of four waves, 16 rows of one candidate against one drawn query row, which is staged in LDS
//                   once; a wave per row.  Quick filter: lane-parallel AND + popcount over the W words, a wave reduction.  Then
//                   lanes run over the query entries m, find the run of equal dij in the candidate row by binary search and
//                   fill a per-wave LDS histogram of the angle bins.
//   select_best     one wave, one candidate: the first task of maximal size in (draw, row) order (the reference's strict >),
//                   and for a winner above the threshold its correspondence lists by a ballot and prefix sum over m.
//
// Why the histogram is the serial walk (match_des, :1034-1123).  Every d1[m].j is distinct and differs from d1.i, so in a
// bin the has-used check only rejects a second pair (m, k') of an m already in that bin: the bin's size is 1 + the number of
// distinct m with a pair in it, and its last append happens at (m_last, the first k of m_last that falls in it).  The tie
// list's first element is the bin that reached the final maximum first, i.e. the largest count and then the earliest such
// (m_last, k) — the packed reach time.  The lists are [d1.i] + [d1[m].j, ascending m] and [d2.i] + [d2[first k of m].j].
// tests/test_gpu_loop.py checks this against a literal serial walk (tests/loop_reference.py).
//
// LDS atomics only (the per-task histogram and the quick_des bitmap); no global atomics; results are reproducible.
#pragma once
#pragma clang fp contract(off)   // dij must be bit-identical to the host arithmetic (the x86-64 host build does not contract)

#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_loop.hpp"

namespace liw_loop_dev {

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

// Point i of the n points pts[. * STRIDE] (x, y first) -> its rows ko [n - 1] keys, ao [n - 1] aij, qo [W] quick_des.  One wave;
// smem holds n * 8 + W * 8 + N2 * 4 bytes (N2: n - 1 rounded up to a power of two).  Returns whether a dij overflowed its 20 bits
// (per lane: the caller raises the flag).  A caller that runs a second point in the same LDS puts a barrier in between.
template <int STRIDE>
__device__ __forceinline__ bool describe_point(const double* __restrict__ pts, int n, int i, Geom g, double d_res, char* smem,
                                               uint32_t* __restrict__ ko, double* __restrict__ ao, uint64_t* __restrict__ qo) {
    const int m = n - 1;
    int N2 = 1;
    while (N2 < m) N2 <<= 1;
    double* a_j = (double*)smem;                    // [n]  aij by j
    uint64_t* q = (uint64_t*)(a_j + n);             // [W]
    uint32_t* key = (uint32_t*)(q + g.W);           // [N2]
    const int lane = threadIdx.x;
    for (int w = lane; w < g.W; w += 64) q[w] = 0;
    __syncthreads();
    const double xi = pts[STRIDE * i], yi = pts[STRIDE * i + 1];
    bool bad = false;
    for (int j = lane; j < n; j += 64) {
        if (j == i) { a_j[j] = 0.0; continue; }
        const double vx = pts[STRIDE * j] - xi, vy = pts[STRIDE * j + 1] - yi;
        const double nrm = sqrt(vx * vx + vy * vy);
        const double c = acos(vx / nrm);
        a_j[j] = vy > 0 ? c : kPi * 2 - c;            // f(v_ij), :931-938
        const double r = nrm / d_res + 0.5;           // round(), :939-942
        uint32_t dij;
        if (!(r < 1048575.0)) { bad = true; dij = 0xFFFFFu; }   // dij <= 2^20 - 2: (dij + 1) << 12 stays in 32 bits
        else dij = (uint32_t)(int)r;
        key[j < i ? j : j - 1] = dij << 12 | (uint32_t)j;
        if ((int)(dij >> 6) < g.W) atomicOr((unsigned long long*)&q[dij >> 6], 1ull << (dij & 63));   // des_i::set_1, :28-35
    }
    for (int e = m + lane; e < N2; e += 64) key[e] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < N2; t += 64) {
                const int u = t ^ jj;
                if (u > t) {
                    const uint32_t a = key[t], b = key[u];
                    if ((a > b) == ((t & k) == 0)) { key[t] = b; key[u] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int e = lane; e < m; e += 64) {
        const uint32_t kv = key[e];
        ko[e] = kv;
        ao[e] = a_j[kv & 0xFFFu];
    }
    for (int w = lane; w < g.W; w += 64) qo[w] = q[w];
    return bad;
}

// Rows r0 .. r0 + 15 (below n2) of a candidate feature against one drawn query row: out[r] = {size, bin | quick_pass << 16}.
// qk / qa / q1: the query row's keys, aij and quick_des; ck0 / ca0 / cq0: row 0 of the candidate's slot (rows P, P and W apart).
// A work-group of 256; smem holds (n1 - 1) * 12 + 4 * (nb * 8 + MW * 256) bytes.  Every thread of the work-group calls it.
__device__ __forceinline__ void match_rows(int n1, int n2, int r0, const uint32_t* __restrict__ qk, const double* __restrict__ qa,
                                           const uint64_t* __restrict__ q1, const uint32_t* __restrict__ ck0, const double* __restrict__ ca0,
                                           const uint64_t* __restrict__ cq0, Geom g, char* smem, int2* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m1 = n1 - 1, m2 = n2 - 1;
    const int MW = (g.nb + 31) >> 5;
    double* sa = (double*)smem;                       // [m1] aij of the drawn query row
    uint32_t* sk = (uint32_t*)(sa + m1);              // [m1] its keys
    char* wbase = (char*)(sk + m1) + (size_t)wave * ((size_t)g.nb * 8 + (size_t)MW * 64 * 4);
    int* cnt = (int*)wbase;                           // [nb]  distinct m per bin
    uint32_t* reach = (uint32_t*)(cnt + g.nb);        // [nb]  max of m << 12 | (4095 - k)
    uint32_t* mask = reach + g.nb;                    // [MW][64] bins the current m of each lane has hit
    for (int e = tid; e < m1; e += blockDim.x) {
        sk[e] = qk[e];
        sa[e] = qa[e];
    }
    __syncthreads();
    for (int it = 0; it < kRowsPerBlock / 4; ++it) {
        const int r = r0 + it * 4 + wave;
        const bool active = r < n2;                   // wave-uniform
        for (int b = lane; b < g.nb; b += 64) { cnt[b] = 0; reach[b] = 0; }
        __syncthreads();
        bool pass = false;
        if (active) {
            const uint64_t* q2 = cq0 + (size_t)r * g.W;
            int pc = 0;
            for (int w = lane; w < g.W; w += 64) pc += __popcll(q1[w] & q2[w]);
            for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o, 64);
            pass = pc >= g.thr;
            if (pass) {
                const uint32_t* ck = ck0 + (size_t)r * g.P;
                const double* ca = ca0 + (size_t)r * g.P;
                for (int m = lane; m < m1; m += 64) {
                    const uint32_t dij = sk[m] >> 12;
                    const int lo = lower_bound_u32(ck, m2, dij << 12), hi = lower_bound_u32(ck, m2, (dij + 1) << 12);
                    if (lo >= hi) continue;
                    for (int w = 0; w < MW; ++w) mask[w * 64 + lane] = 0;
                    const double a1 = sa[m];
                    for (int k = lo; k < hi; ++k) {
                        const int b = angle_bin(a1, ca[k], g.a_res, g.orign, g.nb);
                        const uint32_t bit = 1u << (b & 31);
                        uint32_t* mw = &mask[(b >> 5) * 64 + lane];
                        if (*mw & bit) continue;   // this m is already in bin b: the has-used check
                        *mw |= bit;
                        atomicAdd(&cnt[b], 1);
                        atomicMax(&reach[b], (uint32_t)m << 12 | (uint32_t)(4095 - k));
                    }
                }
            }
        }
        __syncthreads();
        if (active) {
            // largest count, then the earliest reach time (m_last << 12 | k_first); bins are unique per reach time
            uint64_t best = 0;
            for (int b = lane; b < g.nb; b += 64) {
                const int nc = cnt[b];
                if (nc <= 0) continue;
                const uint32_t rv = reach[b];
                const uint32_t rt = (rv & ~0xFFFu) | (4095u - (rv & 0xFFFu));
                const uint64_t v = (uint64_t)nc << 40 | (uint64_t)(0xFFFFFFu - rt) << 16 | (uint64_t)b;
                best = v > best ? v : best;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t x = __shfl_xor(best, o, 64);
                best = x > best ? x : best;
            }
            if (lane == 0) {
                const int nc = (int)(best >> 40);
                out[r] = make_int2(nc ? nc + 1 : 0, (nc ? (int)(best & 0xFFFF) : 0) | (pass ? 1 << 16 : 0));
            }
        }
        __syncthreads();
    }
}

// One candidate (or pair): rows[kDraws] are its drawn query rows (read through the pointer: a dynamically indexed copy would live
// in scratch), tr its tres block [kDraws][P].  qk0 / qa0 and ck0 / ca0: row 0 of the query's and the candidate's feature slot.
// sm[0 .. 6) = {size, draw, row, bin, quick_pass, list length}; L[e * 2 + .] = the correspondences (query point, candidate point)
// of a winner with size > thr.  One wave.
__device__ __forceinline__ void select_best(const int* __restrict__ rows, int n1, int n2, const int2* __restrict__ tr,
                                            const uint32_t* __restrict__ qk0, const double* __restrict__ qa0, const uint32_t* __restrict__ ck0,
                                            const double* __restrict__ ca0, Geom g, int* __restrict__ sm, int* __restrict__ L) {
    const int lane = threadIdx.x;
    uint64_t best = 0;
    int npass = 0;
    const int ntask = kDraws * n2;
    for (int t = lane; t < ntask; t += 64) {
        const int d = t / n2, r = t - d * n2;
        if (rows[d] < 0) continue;
        const int2 v = tr[(size_t)d * g.P + r];
        npass += (v.y >> 16) & 1;
        if (v.x > 0) {
            const uint64_t key = (uint64_t)v.x << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)t);
            best = key > best ? key : best;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = __shfl_xor(best, o, 64);
        best = x > best ? x : best;
        npass += __shfl_xor(npass, o, 64);
    }
    const int size = (int)(best >> 32);
    if (size == 0) {
        if (lane == 0) { sm[0] = 0; sm[1] = -1; sm[2] = -1; sm[3] = -1; sm[4] = npass; sm[5] = 0; }
        return;
    }
    const int t = (int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFu));
    const int d = t / n2, r = t - d * n2;
    const int bin = tr[(size_t)d * g.P + r].y & 0xFFFF;
    int len = 0;
    if (size > g.thr) {
        const int row1 = rows[d];
        const uint32_t* qk = qk0 + (size_t)row1 * g.P;
        const double* qa = qa0 + (size_t)row1 * g.P;
        const uint32_t* ck = ck0 + (size_t)r * g.P;
        const double* ca = ca0 + (size_t)r * g.P;
        if (lane == 0) { L[0] = row1; L[1] = r; }
        len = 1;
        const int m1 = n1 - 1, m2 = n2 - 1;
        for (int m0 = 0; m0 < m1; m0 += 64) {
            const int m = m0 + lane;
            int kk = -1;
            if (m < m1) {
                const uint32_t dij = qk[m] >> 12;
                const int lo = lower_bound_u32(ck, m2, dij << 12), hi = lower_bound_u32(ck, m2, (dij + 1) << 12);
                for (int k = lo; k < hi; ++k)
                    if (angle_bin(qa[m], ca[k], g.a_res, g.orign, g.nb) == bin) { kk = k; break; }
            }
            const unsigned long long hit = __ballot(kk >= 0);
            const int pos = len + __popcll(hit & ((1ull << lane) - 1ull));
            if (kk >= 0 && pos < g.P) { L[pos * 2] = (int)(qk[m] & 0xFFFu); L[pos * 2 + 1] = (int)(ck[kk] & 0xFFFu); }
            len += __popcll(hit);
        }
    }
    if (lane == 0) { sm[0] = size; sm[1] = d; sm[2] = r; sm[3] = bin; sm[4] = npass; sm[5] = len; }
}

}  // namespace liw_loop_dev
