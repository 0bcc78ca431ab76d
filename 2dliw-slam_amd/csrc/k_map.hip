// k_map.hip — the occupancy-grid map's device work (C ABI include/liw_map.h, host side liw_map.cpp).
//
//   k_map_bounds   a lane per point: world point, then a wave / work-group reduction of min / max x, y, the largest ray length
//                  and the number of valid points; one partial per work-group.  k_map_fold (one work-group) folds the partials.
//                  min / max and an integer-valued sum are order-free, so no floating-point atomics are needed.
//   k_map_clear    zeroes the cell bits and the counters.
//   k_map_rays     16 lanes per ray (four rays per wave), lanes striding over the sample index k with tr = T[k] from the step
//                  table (its head staged in LDS): no lane walks a serial tr += step chain.  A lane drops a sample whose cell
//                  equals that of sample k - 1 (step = res / 2: about every second one), reads the cell's byte, and only if the
//                  SAMPLED bit is missing issues a 32-bit atomic OR on the containing word.  The bits are monotone, so a stale
//                  read costs a redundant atomic and never a wrong cell.  The target cell uses the returned old value:
//                  old = or(HIT1); if old had HIT1, or(HIT2) — skipped altogether once the byte shows HIT2.
//   k_map_finish   bits -> -1 / 0 / 50 / 100, 16 cells per lane, and the counts of 0 / 50 / 100 (one integer add per wave).
// The per-ray bodies (make_ray, cell_of, or_cell, the 16-lane walk) are in k_map_dev.hpp, shared with k_map_batch.hip.
//
// Integer OR / add atomics only: the grid and the counts do not depend on the arrival order.
#pragma clang fp contract(off)   // every product and sum rounds on its own, as in the x86-64 host build of the serial walk

#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_map.hpp"
#include "k_map_dev.hpp"

namespace liw_map_dev {

__global__ __launch_bounds__(kBlock) void k_map_bounds(const double* __restrict__ pts, const int* __restrict__ sub, const double* __restrict__ tf,
                                                       long long npts, double* __restrict__ partial) {
    __shared__ double sm[kBlock / 64][6];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    double v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    if (i < npts) {
        const Ray r = make_ray(pts, sub, tf, i);
        if (r.valid) { v[0] = v[1] = r.P[0]; v[2] = v[3] = r.P[1]; v[4] = r.len; v[5] = 1.0; }
    }
    block_fold6(v, sm);
    if (threadIdx.x < 6) partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v[0];
}

__global__ __launch_bounds__(kBlock) void k_map_fold(const double* __restrict__ partial, int nblocks, double* __restrict__ bounds) {
    __shared__ double sm[kBlock / 64][6];
    double v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += kBlock) {
        const double* p = partial + (size_t)b * 6;
        v[0] = fmin(v[0], p[0]); v[1] = fmax(v[1], p[1]); v[2] = fmin(v[2], p[2]); v[3] = fmax(v[3], p[3]); v[4] = fmax(v[4], p[4]); v[5] += p[5];
    }
    block_fold6(v, sm);
    if (threadIdx.x < 6) bounds[threadIdx.x] = v[0];
}

__global__ __launch_bounds__(kBlock) void k_map_clear(uint4* __restrict__ bits16, long long n16, unsigned long long* __restrict__ counters) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n16) bits16[i] = make_uint4(0u, 0u, 0u, 0u);
    if (i < kCounters) counters[i] = 0ull;
}

__global__ __launch_bounds__(kBlock) void k_map_rays(const double* __restrict__ pts, const int* __restrict__ sub, const double* __restrict__ tf,
                                                     long long npts, const double* __restrict__ T, int nT, Grid g, uint8_t* bits,
                                                     unsigned long long* __restrict__ counters) {
    __shared__ double sT[kLdsSteps];
    const int nl = nT < kLdsSteps ? nT : kLdsSteps;
    for (int e = threadIdx.x; e < nl; e += kBlock) sT[e] = T[e];
    __syncthreads();
    const int group = threadIdx.x / kRayLanes, s = threadIdx.x % kRayLanes;
    constexpr int kGroups = kBlock / kRayLanes;
    unsigned long long samples = 0;
    unsigned long long visits = 0, atomics = 0, hit_atomics = 0;   // cell visits after the repeat filter, SAMPLED / HIT atomics issued
    for (long long ray = (long long)blockIdx.x * kGroups + group; ray < npts; ray += (long long)gridDim.x * kGroups) {
        const Ray r = make_ray(pts, sub, tf, ray);
        if (!r.valid) continue;
        walk_ray(r, g, sT, T, nl, s, bits, samples, visits, atomics, hit_atomics);
    }
    samples = wave_sum(samples);
    if ((threadIdx.x & 63) == 0 && samples) atomicAdd(&counters[0], samples);
    visits = wave_sum(visits);
    atomics = wave_sum(atomics);
    hit_atomics = wave_sum(hit_atomics);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&counters[4], atomics); atomicAdd(&counters[5], visits); atomicAdd(&counters[6], hit_atomics); }
}

__global__ __launch_bounds__(kBlock) void k_map_finish(const uint4* __restrict__ bits16, long long n16, uint4* __restrict__ grid16,
                                                       unsigned long long* __restrict__ counters) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long c0 = 0, c50 = 0, c100 = 0;
    if (i < n16) {
        const uint4 b = bits16[i];
        const unsigned in[4] = {b.x, b.y, b.z, b.w};
        unsigned out[4];
        for (int w = 0; w < 4; ++w) {
            unsigned o = 0;
            for (int e = 0; e < 4; ++e) {
                const unsigned v = (in[w] >> (8 * e)) & 0xFFu;
                unsigned val;
                if (v & kHit2) { val = 100u; ++c100; }
                else if (v & kHit1) { val = 50u; ++c50; }
                else if (v & kSampled) { val = 0u; ++c0; }
                else val = 0xFFu;   // -1
                o |= val << (8 * e);
            }
            out[w] = o;
        }
        grid16[i] = make_uint4(out[0], out[1], out[2], out[3]);
    }
    c0 = wave_sum(c0);
    c50 = wave_sum(c50);
    c100 = wave_sum(c100);
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(&counters[1], c0);
        if (c50) atomicAdd(&counters[2], c50);
        if (c100) atomicAdd(&counters[3], c100);
    }
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

int launch_bounds(const double* pts, const int* sub, const double* tf, long long npts, double* partial, double* bounds, hipStream_t s) {
    const int nb = (int)((npts + kBlock - 1) / kBlock);
    if (nb > 0) hipLaunchKernelGGL(k_map_bounds, dim3(nb), dim3(kBlock), 0, s, pts, sub, tf, npts, partial);
    hipLaunchKernelGGL(k_map_fold, dim3(1), dim3(kBlock), 0, s, (const double*)partial, nb, bounds);
    return launched();
}

int launch_clear(uint8_t* bits, long long ncell, unsigned long long* counters, hipStream_t s) {
    const long long n16 = (ncell + 15) / 16;
    const long long nb = (n16 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_map_clear, dim3((unsigned)(nb > 0 ? nb : 1)), dim3(kBlock), 0, s, (uint4*)bits, n16, counters);
    return launched();
}

int launch_rays(const double* pts, const int* sub, const double* tf, long long npts, const double* T, int nT, const Grid& g, uint8_t* bits,
                unsigned long long* counters, hipStream_t s) {
    if (npts <= 0) return 0;
    constexpr int kGroups = kBlock / kRayLanes;
    long long nb = (npts + kGroups - 1) / kGroups;
    if (nb > 2048) nb = 2048;   // 8 work-groups per CU; each strides over the rays, so the LDS table is staged once per 2048th of them
    hipLaunchKernelGGL(k_map_rays, dim3((unsigned)nb), dim3(kBlock), 0, s, pts, sub, tf, npts, T, nT, g, bits, counters);
    return launched();
}

int launch_finish(const uint8_t* bits, long long ncell, signed char* grid, unsigned long long* counters, hipStream_t s) {
    const long long n16 = (ncell + 15) / 16;
    if (n16 <= 0) return 0;
    const long long nb = (n16 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_map_finish, dim3((unsigned)nb), dim3(kBlock), 0, s, (const uint4*)bits, n16, (uint4*)grid, counters);
    return launched();
}

}  // namespace liw_map_dev
