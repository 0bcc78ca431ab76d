// k_map_group.hip — one occupancy grid per GROUP of fleet robots (C ABI include/liw_map_group.h, host side liw_map_group.cpp): the
// grid of liw_map.h over the concatenation of the members' sub-maps, each moved into the group's frame by one rigid transform per
// robot.  The sub-maps stay where liw_fmap_add_keyframes put them (the robot regions of the fleet map's store); the grids live in
// a store of their own, a region per group.  The per-ray, per-cell and bounds bodies are those of the fleet map
// (k_map_batch_dev.hpp, k_map_rays_body.inc, k_map_dev.hpp): only where a body's target lives differs.
//
//   kernel          mapping                                   work
//   k_gmap_reset    a lane per group                          header (status EMPTY), held info 0 x 0
//   k_gmap_tf       a lane per (robot, key frame)             T_g_l = T_g_w[b] * T_w_l[b][k] into the robot's tf part (liw::mul's
//                                                             product and sum order); T_w_l is read, or composed from the pose as
//                                                             k_fmap_tf does; without T_g_w it is stored bit for bit
//   k_gmap_bounds   a work-group per (robot, chunk)           the six partials of k_fmap_bounds, into the robot's partials part
//   k_gmap_fold     a work-group per group                    folds the partials of the members (min / max and integer-valued
//                                                             counts are order-free); thread 0 derives the box, checks the
//                                                             group's max_cells and max_steps, writes status, members, sub-maps,
//                                                             the info row and (OK / EMPTY) the held info
//   k_gmap_clear    a work-group per (group, chunk)           zeroes the cell bits of OK groups
//   k_gmap_rays     16 lanes per ray, a work-group per        a member's rays into its group's cell bits; the samples go by wave
//                   (robot, chunk)                            sums and integer adds into the group's held info and row
//   k_gmap_finish   16 cells per lane, a work-group per       bits -> -1 / 0 / 50 / 100 and the counts
//                   (group, chunk)
//
// Integer OR / add atomics only: a group's region and rows depend neither on the arrival order nor on B, the members' robot
// indices or their order.  The work-groups of a robot in no selected group, and of a group that is not rendered, exit at once.
#pragma clang fp contract(off)   // every product and sum rounds on its own, as in k_map_batch.hip and the serial walk

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/liw_map_batch.h"
#include "k_map_batch_dev.hpp"
#include "k_map_group.hpp"

namespace liw_fmap_dev {

struct Members {                     // who renders: robot b is a member of group group_of[b] when that lies in 0 .. G-1
    const int* group_of;
    const unsigned char* gsel;
    int G;
    // the robot's group when it is one of a selected group, else -1
    __device__ __forceinline__ int group(int b) const {
        const int g = group_of[b];
        return (g >= 0 && g < G && (!gsel || gsel[g] != 0)) ? g : -1;
    }
    __device__ __forceinline__ bool selected(int g) const { return !gsel || gsel[g] != 0; }
};

__device__ __forceinline__ char* group_region(char* gstore, const GLay& GL, int g) { return gstore + (size_t)g * GL.group_bytes; }

__global__ __launch_bounds__(256) void k_gmap_reset(char* gstore, GLay GL, double res, const unsigned char* __restrict__ gmask) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= GL.G || (gmask && !gmask[g])) return;
    char* GR = group_region(gstore, GL, g);
    int* hdr = (int*)GR;
    for (int k = 0; k < 8; ++k) hdr[k] = 0;
    hdr[GH_STATUS] = LIW_FMAP_EMPTY;
    *held_info(GR) = empty_info(res);
}

template <bool kPoses>
__global__ __launch_bounds__(256) void k_gmap_tf(char* store, Lay L, const double* __restrict__ src, long long robot_stride, Til12 til, Members M,
                                                 const double* __restrict__ T_g_w) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)L.B * L.K) return;
    const int b = (int)(i / L.K), k = (int)(i % L.K);
    if (M.group(b) < 0) return;
    char* R = robot_region(store, L, b);
    int* hdr = (int*)R;
    const int nsub = hdr[H_NSUB];
    if (k == 0) hdr[H_NTF] = nsub;
    if (k >= nsub) return;
    double w[12];
    if (kPoses) compose_twl(src + (size_t)b * robot_stride + (size_t)k * 6, til, w);
    else {
        const double* t = src + (size_t)b * robot_stride + (size_t)k * 12;
        for (int e = 0; e < 12; ++e) w[e] = t[e];
    }
    double* tf = (double*)(R + L.r_tf) + (size_t)k * 12;
    if (T_g_w) {
        const double* a = T_g_w + (size_t)b * 12;
        const liw::Iso<double> T = liw::mul(liw::cast_iso<double>(a, a + 9), liw::cast_iso<double>(w, w + 9));
        for (int e = 0; e < 9; ++e) tf[e] = T.R.m[e];
        tf[9] = T.t.x; tf[10] = T.t.y; tf[11] = T.t.z;
    } else {
        for (int e = 0; e < 12; ++e) tf[e] = w[e];
    }
}

__global__ __launch_bounds__(kBlock) void k_gmap_bounds(char* store, Lay L, Members M) {
    __shared__ double sm[kBlock / 64][6];
    const int b = blockIdx.x / L.nchunk, c = blockIdx.x % L.nchunk;
    if (M.group(b) < 0) return;
    char* R = robot_region(store, L, b);
    double v[6];
    bounds_body(R, L, (const double*)(R + L.r_tf), c, v, sm);
    if (threadIdx.x < 6) ((double*)(R + L.r_partial))[(size_t)c * 6 + threadIdx.x] = v[0];
}

__global__ __launch_bounds__(kBlock) void k_gmap_fold(char* store, Lay L, char* gstore, GLay GL, Members M, int* __restrict__ gstatus,
                                                      liw_map_info* __restrict__ ginfo) {
    __shared__ double sm[kBlock / 64][6];
    __shared__ double box[6];
    __shared__ int count[2];
    const int g = blockIdx.x, t = threadIdx.x;
    if (!M.selected(g)) return;
    if (t == 0) count[0] = count[1] = 0;
    double v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    unsigned long long members = 0, submaps = 0;
    for (int b = t; b < L.B; b += kBlock) {
        if (M.group_of[b] != g) continue;
        char* R = robot_region(store, L, b);
        const double* partial = (const double*)(R + L.r_partial);
        for (int c = 0; c < L.nchunk; ++c) fold_partial(v, partial + (size_t)c * 6);
        members += 1;
        submaps += (unsigned long long)((const int*)R)[H_NSUB];
    }
    liw_map_dev::block_fold6(v, sm);   // synchronises: count[] is zero for everyone behind it
    if (t < 6) box[t] = v[0];
    members = liw_map_dev::wave_sum(members);
    submaps = liw_map_dev::wave_sum(submaps);
    if ((t & 63) == 0) {
        atomicAdd(&count[0], (int)members);
        atomicAdd(&count[1], (int)submaps);
    }
    __syncthreads();
    if (t != 0) return;
    char* GR = group_region(gstore, GL, g);
    liw_map_info mi;
    const int st = derive_box(box, L.res, GL.C, L.S, &mi);
    int* hdr = (int*)GR;
    hdr[GH_STATUS] = st;
    hdr[GH_MEMBERS] = count[0];
    hdr[GH_SUBMAPS] = count[1];
    gstatus[g] = st;
    ginfo[g] = mi;
    if (st == LIW_FMAP_OK || st == LIW_FMAP_EMPTY) *held_info(GR) = mi;
}

// false for a group that is not rendered
__device__ __forceinline__ bool rendered(const char* GR) { return ((const int*)GR)[GH_STATUS] == LIW_FMAP_OK; }

__global__ __launch_bounds__(kBlock) void k_gmap_clear(char* gstore, GLay GL, Members M) {
    const int g = blockIdx.x / GL.cchunk, c = blockIdx.x % GL.cchunk;
    char* GR = group_region(gstore, GL, g);
    if (!M.selected(g) || !rendered(GR)) return;
    clear_body(held_info(GR), GR + GL.g_bits, c, GL.cchunk);
}

__global__ __launch_bounds__(kBlock) void k_gmap_rays(char* store, Lay L, char* gstore, GLay GL, Members M, liw_map_info* __restrict__ ginfo) {
    __shared__ double sT[kLdsSteps];
    const int b = blockIdx.x / L.rchunk, c = blockIdx.x % L.rchunk;
    const int grp = M.group(b);
    if (grp < 0) return;
    char* GR = group_region(gstore, GL, grp);
    if (!rendered(GR)) return;
    char* R = robot_region(store, L, b);
#define RAYS_INFO held_info(GR)
#define RAYS_BITS GR + GL.g_bits
#define RAYS_TF (const double*)(R + L.r_tf)
#define RAYS_ROW ginfo[grp]
#include "k_map_rays_body.inc"
#undef RAYS_INFO
#undef RAYS_BITS
#undef RAYS_TF
#undef RAYS_ROW
}

__global__ __launch_bounds__(kBlock) void k_gmap_finish(char* gstore, GLay GL, Members M, liw_map_info* __restrict__ ginfo) {
    const int g = blockIdx.x / GL.cchunk, c = blockIdx.x % GL.cchunk;
    char* GR = group_region(gstore, GL, g);
    if (!M.selected(g) || !rendered(GR)) return;
    finish_body(held_info(GR), GR + GL.g_bits, GR + GL.g_grid, ginfo + g, c, GL.cchunk);
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

int launch_group_reset(char* gstore, const GLay& GL, double res, const unsigned char* gmask, hipStream_t s) {
    hipLaunchKernelGGL(k_gmap_reset, dim3((GL.G + 255) / 256), dim3(256), 0, s, gstore, GL, res, gmask);
    return launched();
}

int launch_group_render(char* store, const Lay& L, char* gstore, const GLay& GL, const double* T_w_l, const double* poses, const double* Til,
                        long long robot_stride, const int* group_of, const double* T_g_w, const unsigned char* gsel, int* gstatus, void* ginfo,
                        hipStream_t s) {
    const Members M{group_of, gsel, GL.G};
    Til12 til;
    for (int k = 0; k < 12; ++k) til.v[k] = Til[k];
    const long long n = (long long)L.B * L.K;
    const dim3 tfgrid((unsigned)((n + 255) / 256));
    if (poses) hipLaunchKernelGGL(k_gmap_tf<true>, tfgrid, dim3(256), 0, s, store, L, poses, robot_stride, til, M, T_g_w);
    else hipLaunchKernelGGL(k_gmap_tf<false>, tfgrid, dim3(256), 0, s, store, L, T_w_l, robot_stride, til, M, T_g_w);
    liw_map_info* mi = (liw_map_info*)ginfo;
    hipLaunchKernelGGL(k_gmap_bounds, dim3((unsigned)L.B * L.nchunk), dim3(kBlock), 0, s, store, L, M);
    hipLaunchKernelGGL(k_gmap_fold, dim3(GL.G), dim3(kBlock), 0, s, store, L, gstore, GL, M, gstatus, mi);
    hipLaunchKernelGGL(k_gmap_clear, dim3((unsigned)GL.G * GL.cchunk), dim3(kBlock), 0, s, gstore, GL, M);
    hipLaunchKernelGGL(k_gmap_rays, dim3((unsigned)L.B * L.rchunk), dim3(kBlock), 0, s, store, L, gstore, GL, M, mi);
    hipLaunchKernelGGL(k_gmap_finish, dim3((unsigned)GL.G * GL.cchunk), dim3(kBlock), 0, s, gstore, GL, M, mi);
    return launched();
}

}  // namespace liw_fmap_dev
