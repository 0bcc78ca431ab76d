// k_map_batch.hip — the fleet's occupancy-grid maps on the device (C ABI include/liw_map_batch.h, host side liw_map_batch.cpp):
// what k_map.hip does for one robot with two read-backs, for B robots per launch and with none.  Every grid is fixed by
// the dims; the work-groups of a robot that is not selected, or whose render failed its capacity check, exit at once.
//
//   kernel          mapping                                   work
//   k_fmap_reset    a lane per robot, plus one lane           header, sub-map offset 0, held info 0 x 0; the one lane writes the
//                                                             step table T[k + 1] = fl(T[k] + res / 2), a serial chain
//   k_fmap_add      a work-group per robot                    the `full` decision before any store, then the new sub-map's
//                                                             offset, its points (16-byte words where source and target agree
//                                                             modulo 16) and the sub-map index of each
//   k_fmap_tf       a lane per (robot, key frame)             T_w_l = make_tf(p, q) * T_imu_to_laser with the correctly rounded
//                                                             sin / cos of liw_crmath.hpp (liw_fmap_render only)
//   k_fmap_bounds   a work-group per (robot, chunk)           strides over the robot's points: six partials (min / max x, y,
//                                                             longest ray, valid points) per work-group
//   k_fmap_fold     a wave per robot                          folds the partials (min / max and an integer-valued count are
//                                                             order-free); lane 0 derives width, height and origin with the
//                                                             arithmetic of liw_map_render_tf, checks max_cells and max_steps,
//                                                             writes status, the info row and (OK / EMPTY) the held info
//   k_fmap_clear    a work-group per (robot, chunk)           zeroes width * height (rounded up to 16) cell bits of OK robots
//   k_fmap_rays     16 lanes per ray, a work-group per        strides over the robot's rays; the Grid comes from the robot's
//                   (robot, chunk)                            header, the head of the step table from LDS; the bodies are those
//                                                             of k_map_rays (k_map_dev.hpp): repeat filter, read-before-atomic
//   k_fmap_finish   16 cells per lane, a work-group per       bits -> -1 / 0 / 50 / 100; the counts go by wave sums and integer
//                   (robot, chunk)                            adds into the robot's held info and its info row
//
// Integer OR / add atomics only: a robot's region and rows do not depend on the arrival order, on B or on the robot's index.
#pragma clang fp contract(off)   // every product and sum rounds on its own, as in k_map.hip and the serial walk

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/liw_map_batch.h"
#include "k_map_batch.hpp"
#include "k_map_batch_dev.hpp"   // the bodies shared with k_map_group.hip

namespace liw_fmap_dev {

__device__ __forceinline__ bool robot_on(const unsigned char* a, int b) { return !a || a[b] != 0; }

__global__ __launch_bounds__(256) void k_fmap_reset(char* store, Lay L, const unsigned char* __restrict__ mask) {
    const int nrb = (L.B + 255) / 256;
    if ((int)blockIdx.x == nrb) {   // the step table: tr of `for (tr = 0; ...; tr += step)`, one lane
        if (threadIdx.x == 0) {
            double* T = (double*)(store + L.s_table);
            const double step = L.res / 2;
            double tr = 0.0;
            for (int k = 0; k < L.S; ++k, tr += step) T[k] = tr;
        }
        return;
    }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b)) return;
    char* R = robot_region(store, L, b);
    int* hdr = (int*)R;
    for (int k = 0; k < 8; ++k) hdr[k] = 0;
    *held_info(R) = empty_info(L.res);
    *(int*)(R + L.r_off) = 0;
}

__global__ __launch_bounds__(256) void k_fmap_add(char* store, Lay L, const unsigned char* __restrict__ key, const double* __restrict__ points,
                                                  int stride, const int* __restrict__ n_points, const unsigned char* __restrict__ mask,
                                                  unsigned char* __restrict__ added) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (!robot_on(mask, b)) return;
    if (!key[b]) {
        if (added && t == 0) added[b] = 0;
        return;
    }
    char* R = robot_region(store, L, b);
    int* hdr = (int*)R;
    int* off = (int*)(R + L.r_off);
    const int k = hdr[H_NSUB], was_full = hdr[H_FULL];
    int n = n_points[b];
    n = n < 0 ? 0 : (n > stride ? stride : n);
    const int base = k < L.K ? off[k] : L.P;
    const bool full = was_full || k >= L.K || (long long)base + n > (long long)L.P;
    __syncthreads();   // every lane has read the header before lane 0 changes it
    if (full) {        // sticky until reset: a later, smaller scan would otherwise be stored under the wrong index
        if (t == 0) {
            hdr[H_FULL] = 1;
            if (added) added[b] = 0;
        }
        return;
    }
    const double* src = points + (size_t)b * stride * 3;
    double* dst = (double*)(R + L.r_pts) + (size_t)base * 3;
    const int nd = 3 * n;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {   // 16-byte words between one leading and one trailing double
        const int head = ((uintptr_t)src & 15) && nd > 0 ? 1 : 0;
        const int n2 = (nd - head) / 2;
        if (t == 0 && head) dst[0] = src[0];
        const double2* s2 = (const double2*)(src + head);
        double2* d2 = (double2*)(dst + head);
        for (int e = t; e < n2; e += 256) d2[e] = s2[e];
        if (t == 0 && head + 2 * n2 < nd) dst[nd - 1] = src[nd - 1];
    } else {
        for (int e = t; e < nd; e += 256) dst[e] = src[e];
    }
    int* sub = (int*)(R + L.r_sub) + base;
    for (int e = t; e < n; e += 256) sub[e] = k;
    if (t == 0) {
        off[k + 1] = base + n;
        hdr[H_NSUB] = k + 1;
        hdr[H_NPTS] = base + n;
        if (added) added[b] = 1;
    }
}

__global__ __launch_bounds__(256) void k_fmap_tf(char* store, Lay L, const double* __restrict__ poses, long long robot_stride, Til12 til,
                                                 const unsigned char* __restrict__ sel) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)L.B * L.K) return;
    const int b = (int)(i / L.K), k = (int)(i % L.K);
    if (!robot_on(sel, b)) return;
    char* R = robot_region(store, L, b);
    int* hdr = (int*)R;
    const int nsub = hdr[H_NSUB];
    if (k == 0) hdr[H_NTF] = nsub;
    if (k >= nsub) return;
    compose_twl(poses + (size_t)b * robot_stride + (size_t)k * 6, til, (double*)(R + L.r_tf) + (size_t)k * 12);
}

__global__ __launch_bounds__(kBlock) void k_fmap_bounds(char* store, Lay L, const double* __restrict__ tfbase, long long tfstride,
                                                        const unsigned char* __restrict__ sel) {
    __shared__ double sm[kBlock / 64][6];
    const int b = blockIdx.x / L.nchunk, c = blockIdx.x % L.nchunk;
    if (!robot_on(sel, b)) return;
    char* R = robot_region(store, L, b);
    double v[6];
    bounds_body(R, L, tfbase + (size_t)b * tfstride, c, v, sm);
    if (threadIdx.x < 6) ((double*)(R + L.r_partial))[(size_t)c * 6 + threadIdx.x] = v[0];
}

__global__ __launch_bounds__(64) void k_fmap_fold(char* store, Lay L, const unsigned char* __restrict__ sel, int* __restrict__ status,
                                                  liw_map_info* __restrict__ info) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!robot_on(sel, b)) return;
    char* R = robot_region(store, L, b);
    const double* partial = (const double*)(R + L.r_partial);
    double v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    for (int c = lane; c < L.nchunk; c += 64) fold_partial(v, partial + (size_t)c * 6);
    for (int o = 32; o > 0; o >>= 1) {
        v[0] = fmin(v[0], __shfl_xor(v[0], o));
        v[1] = fmax(v[1], __shfl_xor(v[1], o));
        v[2] = fmin(v[2], __shfl_xor(v[2], o));
        v[3] = fmax(v[3], __shfl_xor(v[3], o));
        v[4] = fmax(v[4], __shfl_xor(v[4], o));
        v[5] = v[5] + __shfl_xor(v[5], o);
    }
    if (lane != 0) return;
    liw_map_info mi;
    const int st = derive_box(v, L.res, L.C, L.S, &mi);
    ((int*)R)[H_STATUS] = st;
    status[b] = st;
    info[b] = mi;
    if (st == LIW_FMAP_OK || st == LIW_FMAP_EMPTY) *held_info(R) = mi;
}

// the robot's cells in 16-cell items; false for a robot that is not rendered
__device__ __forceinline__ bool rendered(char* R, const unsigned char* sel, int b) { return robot_on(sel, b) && ((const int*)R)[H_STATUS] == LIW_FMAP_OK; }

__global__ __launch_bounds__(kBlock) void k_fmap_clear(char* store, Lay L, const unsigned char* __restrict__ sel) {
    const int b = blockIdx.x / L.cchunk, c = blockIdx.x % L.cchunk;
    char* R = robot_region(store, L, b);
    if (!rendered(R, sel, b)) return;
    clear_body(held_info(R), R + L.r_bits, c, L.cchunk);
}

__global__ __launch_bounds__(kBlock) void k_fmap_rays(char* store, Lay L, const double* __restrict__ tfbase, long long tfstride,
                                                      const unsigned char* __restrict__ sel, liw_map_info* __restrict__ info) {
    __shared__ double sT[kLdsSteps];
    const int b = blockIdx.x / L.rchunk, c = blockIdx.x % L.rchunk;
    char* R = robot_region(store, L, b);
    if (!rendered(R, sel, b)) return;
#define RAYS_INFO held_info(R)
#define RAYS_BITS R + L.r_bits
#define RAYS_TF tfbase + (size_t)b * tfstride
#define RAYS_ROW info[b]
#include "k_map_rays_body.inc"
#undef RAYS_INFO
#undef RAYS_BITS
#undef RAYS_TF
#undef RAYS_ROW
}

__global__ __launch_bounds__(kBlock) void k_fmap_finish(char* store, Lay L, const unsigned char* __restrict__ sel, liw_map_info* __restrict__ info) {
    const int b = blockIdx.x / L.cchunk, c = blockIdx.x % L.cchunk;
    char* R = robot_region(store, L, b);
    if (!rendered(R, sel, b)) return;
    finish_body(held_info(R), R + L.r_bits, R + L.r_grid, info + b, c, L.cchunk);
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fmap_reset, dim3((L.B + 255) / 256 + 1), dim3(256), 0, s, store, L, mask);
    return launched();
}

int launch_add(char* store, const Lay& L, const unsigned char* key, const double* points, int stride, const int* n_points, const unsigned char* mask,
               unsigned char* added, hipStream_t s) {
    hipLaunchKernelGGL(k_fmap_add, dim3(L.B), dim3(256), 0, s, store, L, key, points, stride, n_points, mask, added);
    return launched();
}

int launch_render(char* store, const Lay& L, const double* T_w_l, const double* poses, const double* Til, long long robot_stride,
                  const unsigned char* sel, int* status, void* info, hipStream_t s) {
    const double* tfbase = T_w_l;
    long long tfstride = robot_stride;
    if (poses) {
        Til12 til;
        for (int k = 0; k < 12; ++k) til.v[k] = Til[k];
        const long long n = (long long)L.B * L.K;
        hipLaunchKernelGGL(k_fmap_tf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, store, L, poses, robot_stride, til, sel);
        tfbase = (const double*)(store + L.r_tf);
        tfstride = (long long)(L.robot_bytes / 8);
    }
    liw_map_info* mi = (liw_map_info*)info;
    hipLaunchKernelGGL(k_fmap_bounds, dim3((unsigned)L.B * L.nchunk), dim3(kBlock), 0, s, store, L, tfbase, tfstride, sel);
    hipLaunchKernelGGL(k_fmap_fold, dim3(L.B), dim3(64), 0, s, store, L, sel, status, mi);
    hipLaunchKernelGGL(k_fmap_clear, dim3((unsigned)L.B * L.cchunk), dim3(kBlock), 0, s, store, L, sel);
    hipLaunchKernelGGL(k_fmap_rays, dim3((unsigned)L.B * L.rchunk), dim3(kBlock), 0, s, store, L, tfbase, tfstride, sel, mi);
    hipLaunchKernelGGL(k_fmap_finish, dim3((unsigned)L.B * L.cchunk), dim3(kBlock), 0, s, store, L, sel, mi);
    return launched();
}

}  // namespace liw_fmap_dev
