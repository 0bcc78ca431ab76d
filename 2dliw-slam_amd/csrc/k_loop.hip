// k_loop.hip — the loop detector's kernels (C ABI include/liw_loop.h, host side liw_loop.cpp): the addressing of one robot's store
// (a Cand per launched candidate, a feature slot per key frame) around the bodies of k_loop_dev.hpp, which explains the algorithm
// and why it is the reference's serial walk.
//
//   k_loop_describe  one wave per point i of a new sub-map: describe_point.
//   k_loop_match     one work-group per (candidate, draw, 16 rows of the candidate): match_rows.
//   k_loop_select    one wave per candidate: select_best.
#pragma clang fp contract(off)   // dij must be bit-identical to the host arithmetic (the x86-64 host build does not contract)

#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_loop_dev.hpp"

namespace liw_loop_dev {

__global__ __launch_bounds__(64) void k_loop_describe(const double* __restrict__ pts, int n, int slot, Geom g, double d_res,
                                                      uint32_t* __restrict__ keys, double* __restrict__ aij, uint64_t* __restrict__ quick,
                                                      int* __restrict__ inv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t row = (size_t)slot * g.P + blockIdx.x;
    if (describe_point<2>(pts, n, blockIdx.x, g, d_res, smem, keys + row * g.P, aij + row * g.P, quick + row * g.W))
        inv[slot] = 1;   // every writer stores the same value
}

__global__ __launch_bounds__(256) void k_loop_match(const Cand* __restrict__ cands, int qslot, int n1, Geom g, const uint32_t* __restrict__ keys,
                                                    const double* __restrict__ aij, const uint64_t* __restrict__ quick, int2* __restrict__ tres) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Cand* c = cands + blockIdx.z;               // read through the pointer: a dynamically indexed copy would live in scratch
    const int d = blockIdx.y, n2 = c->n2, row1 = c->rows[d];
    const int r0 = blockIdx.x * kRowsPerBlock;
    int2* out = tres + ((size_t)blockIdx.z * kDraws + d) * g.P;
    if (r0 >= n2) return;
    if (row1 < 0) {   // a repeated draw: no task
        for (int r = r0 + threadIdx.x; r < n2 && r < r0 + kRowsPerBlock; r += blockDim.x) out[r] = make_int2(0, 0);
        return;
    }
    const size_t qrow = (size_t)qslot * g.P + row1, cslot = (size_t)c->slot * g.P;
    match_rows(n1, n2, r0, keys + qrow * g.P, aij + qrow * g.P, quick + qrow * g.W, keys + cslot * g.P, aij + cslot * g.P, quick + cslot * g.W, g,
               smem, out);
}

__global__ __launch_bounds__(64) void k_loop_select(const Cand* __restrict__ cands, int qslot, int n1, Geom g, const uint32_t* __restrict__ keys,
                                                    const double* __restrict__ aij, const int2* __restrict__ tres, int* __restrict__ summary,
                                                    int* __restrict__ lists) {
    const Cand* c = cands + blockIdx.x;
    const size_t qs = (size_t)qslot * g.P * g.P, cs = (size_t)c->slot * g.P * g.P;
    select_best(c->rows, n1, c->n2, tres + (size_t)blockIdx.x * kDraws * g.P, keys + qs, aij + qs, keys + cs, aij + cs, g,
                summary + (size_t)blockIdx.x * 8, lists + (size_t)blockIdx.x * g.P * 2);
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
