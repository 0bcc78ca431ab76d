// k_map_batch_dev.hpp — the device bodies that the fleet map's kernels (k_map_batch.hip: a grid per robot) and the group map's
// (k_map_group.hip: a grid per group of robots) share.  A body is told where its target lives (the held liw_map_info, the cell
// bits, the grid, the info row) and which robot region its rays come from; for the fleet map both are the robot's own region.
// The ray kernels' body is k_map_rays_body.inc, included as text: as a function the per-robot kernel compiled to other code.
// Include after `#pragma clang fp contract(off)`: every product and sum rounds on its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/liw_map_batch.h"
#include "k_map_batch.hpp"
#include "k_map_dev.hpp"
#include "liw_crmath.hpp"
#include "liw_dual.hpp"

namespace liw_fmap_dev {

using liw_map_dev::Grid;
using liw_map_dev::kBlock;
using liw_map_dev::kLdsSteps;
using liw_map_dev::kRayLanes;
using liw_map_dev::Ray;

// A double whose sin / cos / atan2 are the correctly rounded ones of liw_crmath.hpp, as in k_loop_batch.hip
struct CR {
    double v;
    __host__ __device__ CR() : v(0.0) {}
    __host__ __device__ CR(double c) : v(c) {}  // NOLINT(implicit)
};
__host__ __device__ inline CR operator+(const CR& a, const CR& b) { return CR(a.v + b.v); }
__host__ __device__ inline CR operator-(const CR& a, const CR& b) { return CR(a.v - b.v); }
__host__ __device__ inline CR operator-(const CR& a) { return CR(-a.v); }
__host__ __device__ inline CR operator*(const CR& a, const CR& b) { return CR(a.v * b.v); }
__host__ __device__ inline CR operator/(const CR& a, const CR& b) { return CR(a.v / b.v); }
__host__ __device__ inline bool operator>(const CR& a, const CR& b) { return a.v > b.v; }
__host__ __device__ inline bool operator<(const CR& a, const CR& b) { return a.v < b.v; }
__host__ __device__ inline CR dsqrt(const CR& a) { return CR(sqrt(a.v)); }
__host__ __device__ inline CR dsin(const CR& a) { return CR(liw_cr::cr_sin(a.v)); }
__host__ __device__ inline CR dcos(const CR& a) { return CR(liw_cr::cr_cos(a.v)); }
__host__ __device__ inline CR datan2(const CR& y, const CR& x) { return CR(liw_cr::cr_atan2(y.v, x.v)); }
__host__ __device__ inline CR dfloor(const CR& a) { return CR(floor(a.v)); }

struct Til12 { double v[12]; };      // T_imu_to_laser by value

__device__ __forceinline__ char* robot_region(char* store, const Lay& L, int b) { return store + (size_t)b * L.robot_bytes; }
__device__ __forceinline__ liw_map_info* held_info(char* R) { return (liw_map_info*)(R + HB_INFO); }   // of a robot or a group region

__device__ __forceinline__ liw_map_info empty_info(double res) {
    liw_map_info mi;
    mi.width = mi.height = 0;
    mi.resolution = res;
    mi.origin_x = mi.origin_y = 0.0;
    mi.rays = mi.samples = mi.unknown = mi.free_cells = mi.hit_once = mi.hit_more = 0;
    return mi;
}

// T_w_l = make_tf(p, q) * T_imu_to_laser of one key frame (ps: p, rotation vector q) as 12 doubles
__device__ __forceinline__ void compose_twl(const double* __restrict__ ps, const Til12& til, double* tf) {
    const liw::Iso<CR> A = liw::make_tf(liw::V3<CR>(ps[0], ps[1], ps[2]), liw::V3<CR>(ps[3], ps[4], ps[5]));
    const liw::Iso<CR> T = liw::mul(A, liw::cast_iso<CR>(til.v, til.v + 9));
    for (int e = 0; e < 9; ++e) tf[e] = T.R.m[e].v;
    tf[9] = T.t.x.v; tf[10] = T.t.y.v; tf[11] = T.t.z.v;
}

// partial record c of nchunk over the points of robot region R: thread t < 6 returns component t in v[0]
__device__ __forceinline__ void bounds_body(char* R, const Lay& L, const double* __restrict__ tf, int c, double* v, double (*sm)[6]) {
    const int npts = ((const int*)R)[H_NPTS];
    const double* pts = (const double*)(R + L.r_pts);
    const int* sub = (const int*)(R + L.r_sub);
    v[0] = INFINITY; v[1] = -INFINITY; v[2] = INFINITY; v[3] = -INFINITY; v[4] = 0.0; v[5] = 0.0;
    for (int i = c * kBlock + threadIdx.x; i < npts; i += L.nchunk * kBlock) {
        const Ray r = liw_map_dev::make_ray(pts, sub, tf, i);
        if (r.valid) {
            v[0] = fmin(v[0], r.P[0]); v[1] = fmax(v[1], r.P[0]); v[2] = fmin(v[2], r.P[1]); v[3] = fmax(v[3], r.P[1]);
            v[4] = fmax(v[4], r.len); v[5] += 1.0;
        }
    }
    liw_map_dev::block_fold6(v, sm);
}

// one more partial record into the running fold v
__device__ __forceinline__ void fold_partial(double* v, const double* __restrict__ p) {
    v[0] = fmin(v[0], p[0]); v[1] = fmax(v[1], p[1]); v[2] = fmin(v[2], p[2]); v[3] = fmax(v[3], p[3]); v[4] = fmax(v[4], p[4]); v[5] += p[5];
}

// Width, height and origin from the folded bounds v with the arithmetic of liw_map_render_tf's host code
// (visualization.cpp:412-413), and the capacity checks against max_cells C and max_steps S.  Returns the status.
__device__ __forceinline__ int derive_box(const double* v, double res, int C, int S, liw_map_info* out) {
    const double step = res / 2;
    liw_map_info mi = empty_info(res);
    mi.rays = (long long)v[5];
    int st = LIW_FMAP_OK;
    if (mi.rays == 0) st = LIW_FMAP_EMPTY;   // no valid point: a 0 x 0 map
    else {
        const double wd = (v[1] - v[0]) / res + 1, hd = (v[3] - v[2]) / res + 1;
        mi.origin_x = v[0];
        mi.origin_y = v[2];
        if (!(wd < 2147483647.0) || !(hd < 2147483647.0)) {
            mi.width = mi.height = 2147483647;
            st = LIW_FMAP_OVER_CELLS;
        } else {
            mi.width = (int)wd;
            mi.height = (int)hd;
            const long long ncell = (long long)mi.width * mi.height;
            const double nsteps = v[4] / step;
            if (ncell > (long long)C) st = LIW_FMAP_OVER_CELLS;
            else if (!(nsteps < (double)(S - 2))) st = LIW_FMAP_RAY_TOO_LONG;   // the ray walk looks one entry past int(len / step)
            else mi.unknown = ncell;   // the finish takes the known cells off
        }
    }
    *out = mi;
    return st;
}

// zeroes the cell bits of the held grid (rounded up to 16): chunk c of nchunk
__device__ __forceinline__ void clear_body(const liw_map_info* hi, char* bits, int c, int nchunk) {
    const long long n16 = ((long long)hi->width * hi->height + 15) / 16;
    unsigned long long* bits8 = (unsigned long long*)bits;   // the stores are 8-byte aligned: two 8-byte words per item
    for (long long i = (long long)c * kBlock + threadIdx.x; i < n16; i += (long long)nchunk * kBlock) {
        bits8[2 * i] = 0ull;
        bits8[2 * i + 1] = 0ull;
    }
}

// the known cells of a wave go from `unknown` to their counts
__device__ __forceinline__ void add_counts(liw_map_info* mi, unsigned long long c0, unsigned long long c50, unsigned long long c100) {
    if (c0) atomicAdd((unsigned long long*)&mi->free_cells, c0);
    if (c50) atomicAdd((unsigned long long*)&mi->hit_once, c50);
    if (c100) atomicAdd((unsigned long long*)&mi->hit_more, c100);
    atomicAdd((unsigned long long*)&mi->unknown, 0ull - (c0 + c50 + c100));
}

// bits -> -1 / 0 / 50 / 100 for the cells of the held grid, chunk c of nchunk; the counts go into `hi` and `row`
__device__ __forceinline__ void finish_body(liw_map_info* hi, const char* bits, char* grid, liw_map_info* row, int c, int nchunk) {
    const long long n16 = ((long long)hi->width * hi->height + 15) / 16;
    const uint2* bits8 = (const uint2*)bits;
    uint2* grid8 = (uint2*)grid;
    unsigned long long c0 = 0, c50 = 0, c100 = 0;
    for (long long i = (long long)c * kBlock + threadIdx.x; i < n16; i += (long long)nchunk * kBlock) {
        const uint2 lo = bits8[2 * i], hi2 = bits8[2 * i + 1];
        const unsigned in[4] = {lo.x, lo.y, hi2.x, hi2.y};
        unsigned out[4];
        for (int w = 0; w < 4; ++w) {
            unsigned o = 0;
            for (int e = 0; e < 4; ++e) {
                const unsigned v = (in[w] >> (8 * e)) & 0xFFu;
                unsigned val;
                if (v & liw_map_dev::kHit2) { val = 100u; ++c100; }
                else if (v & liw_map_dev::kHit1) { val = 50u; ++c50; }
                else if (v & liw_map_dev::kSampled) { val = 0u; ++c0; }
                else val = 0xFFu;   // -1
                o |= val << (8 * e);
            }
            out[w] = o;
        }
        grid8[2 * i] = make_uint2(out[0], out[1]);
        grid8[2 * i + 1] = make_uint2(out[2], out[3]);
    }
    c0 = liw_map_dev::wave_sum(c0);
    c50 = liw_map_dev::wave_sum(c50);
    c100 = liw_map_dev::wave_sum(c100);
    if ((threadIdx.x & 63) == 0 && (c0 | c50 | c100)) {
        add_counts(hi, c0, c50, c100);
        add_counts(row, c0, c50, c100);
    }
}

}  // namespace liw_fmap_dev
