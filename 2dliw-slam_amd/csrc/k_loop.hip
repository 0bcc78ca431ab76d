// k_loop.hip — the loop detector's device work (C ABI include/liw_loop.h, host side liw_loop.cpp).
//
//   k_loop_describe  one wave per point i of a new sub-map: lanes over j build dij = int(|p_j - p_i| / d_res + 0.5) and
//                    aij (keyframe_manager.cpp:945-1032), the 32-bit keys dij << 12 | j are bitonic-sorted in LDS (= the
//                    (dij, j) order), aij is gathered by j, quick_des is or-ed together in LDS.
//   k_loop_match     one wave per (candidate, draw, row of the candidate) task; a work-group takes 16 rows of one
//                    (candidate, draw) and stages the drawn query row in LDS once.  Quick filter: lane-parallel AND +
//                    popcount over the W words, a wave reduction.  Then lanes run over the query entries m, find the run of
//                    equal dij in the candidate row by binary search and fill a per-task LDS histogram of the angle bins.
//   k_loop_select    one wave per candidate: the first task of maximal size in (draw, row) order (the reference's strict >),
//                    and for a winner above the threshold its correspondence lists by a ballot and prefix sum over m.
//
// Why the histogram is the serial walk (match_des, :1034-1123).  Every d1[m].j is distinct and differs from d1.i, so in a
// bin the has-used check only rejects a second pair (m, k') of an m already in that bin: the bin's size is 1 + the number of
// distinct m with a pair in it, and its last append happens at (m_last, the first k of m_last that falls in it).  The tie
// list's first element is the bin that reached the final maximum first, i.e. the largest count and then the earliest such
// (m_last, k) — the packed reach time.  The lists are [d1.i] + [d1[m].j, ascending m] and [d2.i] + [d2[first k of m].j].
// tests/test_gpu_loop.py checks this against a literal serial walk (tests/loop_reference.py).
//
// LDS atomics only (the per-task histogram and the quick_des bitmap); no global atomics; results are reproducible.
#pragma clang fp contract(off)   // dij must be bit-identical to the host arithmetic (the x86-64 host build does not contract)

#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_loop.hpp"

namespace liw_loop_dev {

__global__ __launch_bounds__(64) void k_loop_describe(const double* __restrict__ pts, int n, int slot, Geom g, double d_res,
                                                      uint32_t* __restrict__ keys, double* __restrict__ aij, uint64_t* __restrict__ quick,
                                                      int* __restrict__ inv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int m = n - 1;
    int N2 = 1;
    while (N2 < m) N2 <<= 1;
    double* a_j = (double*)smem;                    // [n]  aij by j
    uint64_t* q = (uint64_t*)(a_j + n);             // [W]
    uint32_t* key = (uint32_t*)(q + g.W);           // [N2]
    const int i = blockIdx.x, lane = threadIdx.x;
    for (int w = lane; w < g.W; w += 64) q[w] = 0;
    __syncthreads();
    const double xi = pts[2 * i], yi = pts[2 * i + 1];
    bool bad = false;
    for (int j = lane; j < n; j += 64) {
        if (j == i) { a_j[j] = 0.0; continue; }
        const double vx = pts[2 * j] - xi, vy = pts[2 * j + 1] - yi;
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
    const size_t row = (size_t)slot * g.P + i;
    uint32_t* ko = keys + row * g.P;
    double* ao = aij + row * g.P;
    for (int e = lane; e < m; e += 64) {
        const uint32_t kv = key[e];
        ko[e] = kv;
        ao[e] = a_j[kv & 0xFFFu];
    }
    uint64_t* qo = quick + row * g.W;
    for (int w = lane; w < g.W; w += 64) qo[w] = q[w];
    if (bad) inv[slot] = 1;   // every writer stores the same value
}

__global__ __launch_bounds__(256) void k_loop_match(const Cand* __restrict__ cands, int qslot, int n1, Geom g, const uint32_t* __restrict__ keys,
                                                    const double* __restrict__ aij, const uint64_t* __restrict__ quick, int2* __restrict__ tres) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Cand* c = cands + blockIdx.z;               // read through the pointer: a dynamically indexed copy would live in scratch
    const int d = blockIdx.y, n2 = c->n2, row1 = c->rows[d];
    const int r0 = blockIdx.x * kRowsPerBlock;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int2* out = tres + ((size_t)blockIdx.z * kDraws + d) * g.P;
    if (r0 >= n2) return;
    if (row1 < 0) {   // a repeated draw: no task
        for (int r = r0 + tid; r < n2 && r < r0 + kRowsPerBlock; r += blockDim.x) out[r] = make_int2(0, 0);
        return;
    }
    const int m1 = n1 - 1, m2 = n2 - 1;
    const int MW = (g.nb + 31) >> 5;
    double* qa = (double*)smem;                       // [m1] aij of the drawn query row
    uint32_t* qk = (uint32_t*)(qa + m1);              // [m1] its keys
    char* wbase = (char*)(qk + m1) + (size_t)wave * ((size_t)g.nb * 8 + (size_t)MW * 64 * 4);
    int* cnt = (int*)wbase;                           // [nb]  distinct m per bin
    uint32_t* reach = (uint32_t*)(cnt + g.nb);        // [nb]  max of m << 12 | (4095 - k)
    uint32_t* mask = reach + g.nb;                    // [MW][64] bins the current m of each lane has hit
    const size_t qrow = (size_t)qslot * g.P + row1;
    for (int e = tid; e < m1; e += blockDim.x) {
        qk[e] = keys[qrow * g.P + e];
        qa[e] = aij[qrow * g.P + e];
    }
    const uint64_t* q1 = quick + qrow * g.W;
    __syncthreads();
    for (int it = 0; it < kRowsPerBlock / 4; ++it) {
        const int r = r0 + it * 4 + wave;
        const bool active = r < n2;                   // wave-uniform
        for (int b = lane; b < g.nb; b += 64) { cnt[b] = 0; reach[b] = 0; }
        __syncthreads();
        bool pass = false;
        const size_t crow = (size_t)c->slot * g.P + (active ? r : 0);
        if (active) {
            const uint64_t* q2 = quick + crow * g.W;
            int pc = 0;
            for (int w = lane; w < g.W; w += 64) pc += __popcll(q1[w] & q2[w]);
            for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o, 64);
            pass = pc >= g.thr;
            if (pass) {
                const uint32_t* ck = keys + crow * g.P;
                const double* ca = aij + crow * g.P;
                for (int m = lane; m < m1; m += 64) {
                    const uint32_t dij = qk[m] >> 12;
                    const int lo = lower_bound_u32(ck, m2, dij << 12), hi = lower_bound_u32(ck, m2, (dij + 1) << 12);
                    if (lo >= hi) continue;
                    for (int w = 0; w < MW; ++w) mask[w * 64 + lane] = 0;
                    const double a1 = qa[m];
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

__global__ __launch_bounds__(64) void k_loop_select(const Cand* __restrict__ cands, int qslot, int n1, Geom g, const uint32_t* __restrict__ keys,
                                                    const double* __restrict__ aij, const int2* __restrict__ tres, int* __restrict__ summary,
                                                    int* __restrict__ lists) {
    const Cand* c = cands + blockIdx.x;
    const int lane = threadIdx.x, n2 = c->n2;
    const int2* tr = tres + (size_t)blockIdx.x * kDraws * g.P;
    uint64_t best = 0;
    int npass = 0;
    const int ntask = kDraws * n2;
    for (int t = lane; t < ntask; t += 64) {
        const int d = t / n2, r = t - d * n2;
        if (c->rows[d] < 0) continue;
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
    int* sm = summary + (size_t)blockIdx.x * 8;
    if (size == 0) {
        if (lane == 0) { sm[0] = 0; sm[1] = -1; sm[2] = -1; sm[3] = -1; sm[4] = npass; sm[5] = 0; }
        return;
    }
    const int t = (int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFu));
    const int d = t / n2, r = t - d * n2;
    const int bin = tr[(size_t)d * g.P + r].y & 0xFFFF;
    int len = 0;
    if (size > g.thr) {
        const int row1 = c->rows[d];
        const size_t qrow = (size_t)qslot * g.P + row1, crow = (size_t)c->slot * g.P + r;
        const uint32_t* qk = keys + qrow * g.P;
        const double* qa = aij + qrow * g.P;
        const uint32_t* ck = keys + crow * g.P;
        const double* ca = aij + crow * g.P;
        int* L = lists + (size_t)blockIdx.x * g.P * 2;
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

static size_t match_lds(int n1, const Geom& g) {
    const int MW = (g.nb + 31) >> 5;
    return (size_t)(n1 > 0 ? n1 - 1 : 0) * 12 + 4 * ((size_t)g.nb * 8 + (size_t)MW * 64 * 4);
}

int launch_describe(const double* pts, int n, int slot, const Geom& g, double d_res, uint32_t* keys, double* aij, uint64_t* quick, int* inv,
                    hipStream_t s) {
    if (n <= 0) return 0;
    int N2 = 1;
    while (N2 < n - 1) N2 <<= 1;
    const size_t lds = (size_t)n * 8 + (size_t)g.W * 8 + (size_t)N2 * 4;
    hipLaunchKernelGGL(k_loop_describe, dim3(n), dim3(64), lds, s, pts, n, slot, g, d_res, keys, aij, quick, inv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_match(const Cand* cands, int ncand, int max_n2, int qslot, int n1, const Geom& g, const uint32_t* keys, const double* aij,
                 const uint64_t* quick, int2* tres, hipStream_t s) {
    if (ncand <= 0 || max_n2 <= 0) return 0;
    const dim3 grid((max_n2 + kRowsPerBlock - 1) / kRowsPerBlock, kDraws, ncand);
    hipLaunchKernelGGL(k_loop_match, grid, dim3(256), match_lds(n1, g), s, cands, qslot, n1, g, keys, aij, quick, tres);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_select(const Cand* cands, int ncand, int qslot, int n1, const Geom& g, const uint32_t* keys, const double* aij, const int2* tres,
                  int* summary, int* lists, hipStream_t s) {
    if (ncand <= 0) return 0;
    hipLaunchKernelGGL(k_loop_select, dim3(ncand), dim3(64), 0, s, cands, qslot, n1, g, keys, aij, tres, summary, lists);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace liw_loop_dev
