// k_map_dev.hpp — the per-ray device bodies of the occupancy-grid map, shared by the single-robot kernels (k_map.hip) and the
// fleet's (k_map_batch.hip): both run the same instructions per ray, so a fleet robot's grid equals the single map's cell for
// cell.  Include after `#pragma clang fp contract(off)`: every product and sum rounds on its own.
#pragma once
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

// What lane s of the kRayLanes lanes that share ray r does with it: the target cell, the sample count and the walk over the
// samples k = s, s + kRayLanes, ...  sT holds the first nl entries of the step table T (LDS), later ones come from T itself.
// samples is counted by lane 0 of the ray; visits / atomics / hit_atomics count per lane (cell visits after the repeat filter,
// SAMPLED / HIT atomics issued).  All kRayLanes lanes of a ray must call it together.
__device__ __forceinline__ void walk_ray(const Ray& r, const Grid& g, const double* sT, const double* __restrict__ T, int nl, int s, uint8_t* bits,
                                         unsigned long long& samples, unsigned long long& visits, unsigned long long& atomics,
                                         unsigned long long& hit_atomics) {
    if (s == 0) {   // the target cell: -1 / 0 -> 50, 50 / 100 -> 100.  A cell seen with HIT2 needs nothing more (walls are hit
                    // by thousands of rays: without this look every ray pays one or two atomics on the same few words)
        const int cell = cell_of(r.P[0], r.P[1], g);
        if (cell >= 0 && !(bits[cell] & kHit2)) {
            ++hit_atomics;
            if (or_cell(bits, cell, kHit1) & kHit1) { or_cell(bits, cell, kHit2); ++hit_atomics; }
        }
    }
    if (!(r.len > 0.0)) return;   // a ray of length 0 has no direction: only its target cell
    const double ux = r.d[0] / r.len, uy = r.d[1] / r.len;
    // samples k = 0 .. n - 1 with T[k] <= len: int(len / step) is within one of the last index (the table drifts from
    // k * step by 1e-12 of a step); the table is two entries longer than the longest ray needs
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

}  // namespace liw_map_dev
