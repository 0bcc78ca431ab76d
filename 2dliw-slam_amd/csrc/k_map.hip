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
//
// Integer OR / add atomics only: the grid and the counts do not depend on the arrival order.
#pragma clang fp contract(off)   // every product and sum rounds on its own, as in the x86-64 host build of the serial walk

#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_map.hpp"

namespace liw_map_dev {

struct Ray {
    double O[3], P[3], d[3], len;
    bool valid;
};

// world point P = T_w_l * pt with the sum order ((R0 x + R1 y) + R2 z) + t, the ray O -> P and its length
__device__ __forceinline__ Ray make_ray(const double* __restrict__ pts, const int* __restrict__ sub, const double* __restrict__ tf, long long i) {
    Ray r;
    const double* T = tf + (size_t)sub[i] * 12;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    for (int c = 0; c < 3; ++c) {
        r.O[c] = T[9 + c];
        r.P[c] = ((T[3 * c] * x + T[3 * c + 1] * y) + T[3 * c + 2] * z) + r.O[c];
        r.d[c] = r.P[c] - r.O[c];
    }
    r.len = sqrt((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    r.valid = isfinite(r.P[0]) && isfinite(r.P[1]) && isfinite(r.P[2]) && isfinite(r.len);
    return r;
}

// v = {min x, max x, min y, max y, max len, count} over the work-group; thread c < 6 returns component c in v[0]
__device__ __forceinline__ void block_fold6(double* v, double (*sm)[6]) {
    for (int o = 32; o > 0; o >>= 1) {
        v[0] = fmin(v[0], __shfl_xor(v[0], o));
        v[1] = fmax(v[1], __shfl_xor(v[1], o));
        v[2] = fmin(v[2], __shfl_xor(v[2], o));
        v[3] = fmax(v[3], __shfl_xor(v[3], o));
        v[4] = fmax(v[4], __shfl_xor(v[4], o));
        v[5] = v[5] + __shfl_xor(v[5], o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 6; ++c) sm[wave][c] = v[c];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        double a = sm[0][c];
        for (int w = 1; w < kBlock / 64; ++w) {
            const double b = sm[w][c];
            a = (c == 0 || c == 2) ? fmin(a, b) : (c == 5 ? a + b : fmax(a, b));
        }
        v[0] = a;
    }
}

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

// cell index of a point, -1 outside the grid.  int(q) is in [0, n) exactly when -1 < q < n (the conversion truncates toward
// zero), which also keeps the conversion itself in range; a NaN fails both comparisons.
__device__ __forceinline__ int cell_of(double cx, double cy, const Grid& g) {
    const double qx = (cx - g.origin_x) / g.res, qy = (cy - g.origin_y) / g.res;
    if (!(qx > -1.0 && qx < (double)g.width && qy > -1.0 && qy < (double)g.height)) return -1;
    return (int)qy * g.width + (int)qx;
}

__device__ __forceinline__ unsigned or_cell(uint8_t* bits, int cell, unsigned bit) {
    const unsigned sh = 8u * ((unsigned)cell & 3u);
    const unsigned old = __hip_atomic_fetch_or((unsigned*)bits + (cell >> 2), bit << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (old >> sh) & 0xFFu;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
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
        if (s == 0) {   // the target cell: -1 / 0 -> 50, 50 / 100 -> 100.  A cell seen with HIT2 needs nothing more (walls are hit
                        // by thousands of rays: without this look every ray pays one or two atomics on the same few words)
            const int cell = cell_of(r.P[0], r.P[1], g);
            if (cell >= 0 && !(bits[cell] & kHit2)) {
                ++hit_atomics;
                if (or_cell(bits, cell, kHit1) & kHit1) { or_cell(bits, cell, kHit2); ++hit_atomics; }
            }
        }
        if (!(r.len > 0.0)) continue;   // a ray of length 0 has no direction: only its target cell
        const double ux = r.d[0] / r.len, uy = r.d[1] / r.len;
        // samples k = 0 .. n - 1 with T[k] <= len: int(len / step) is within one of the last index (the table drifts from
        // k * step by 1e-12 of a step); the host made the table two entries longer than the longest ray needs
        int last = (int)(r.len / g.step);
        const double tl = last < nl ? sT[last] : T[last];
        if (tl > r.len) --last;
        else {
            const double tn = last + 1 < nl ? sT[last + 1] : T[last + 1];
            if (tn <= r.len) ++last;
        }
        const int n = last + 1;
        if (s == 0) samples += (unsigned long long)n;
        int prev_last = -1;   // cell of sample base - 1
        for (int base = 0; base < n; base += kRayLanes) {
            const int k = base + s;
            int cell = -1;
            if (k < n) {
                const double tr = k < nl ? sT[k] : T[k];
                cell = cell_of(r.O[0] + ux * tr, r.O[1] + uy * tr, g);
            }
            int before = __shfl_up(cell, 1, kRayLanes);
            if (s == 0) before = prev_last;
            prev_last = __shfl(cell, kRayLanes - 1, kRayLanes);
            if (cell >= 0 && cell != before) {
                ++visits;
                if (!(bits[cell] & kSampled)) {
                    or_cell(bits, cell, kSampled);
                    ++atomics;
                }
            }
        }
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
