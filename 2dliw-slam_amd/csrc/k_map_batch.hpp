// k_map_batch.hpp — interface between the fleet map's host code (liw_map_batch.cpp) and its kernels (k_map_batch.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace liw_fmap_dev {

// header of a robot region: int32 words, then the held liw_map_info
constexpr int H_NSUB = 0, H_FULL = 1, H_STATUS = 2, H_NPTS = 3, H_NTF = 4;
constexpr size_t HB_INFO = 32;      // byte offset of the held liw_map_info (80 bytes)
constexpr int kMaxChunks = 64;      // bounds partials per robot at most

struct Lay {                         // byte offsets within a robot region (r_*) and within the store (s_*)
    int B, K, P, C, S;               // robots, max_submaps, max_points, max_cells, max_steps
    int nchunk;                      // work-groups per robot of k_fmap_bounds = partial records per robot
    int rchunk;                      // work-groups per robot of k_fmap_rays
    int cchunk;                      // work-groups per robot of k_fmap_clear and k_fmap_finish
    size_t Cn;                       // max_cells rounded up to 16
    size_t r_off, r_pts, r_sub, r_tf, r_partial, r_bits, r_grid, robot_bytes;
    size_t s_table, shared_bytes, bytes;
    double res;
};

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_add(char* store, const Lay& L, const unsigned char* key, const double* points, int stride, const int* n_points, const unsigned char* mask,
               unsigned char* added, hipStream_t s);
// poses != nullptr: k_fmap_tf composes make_tf(p, q) * Til into the regions first; else T_w_l is copied there
int launch_render(char* store, const Lay& L, const double* T_w_l, const double* poses, const double* Til, long long robot_stride,
                  const unsigned char* sel, int* status, void* info, hipStream_t s);

}  // namespace liw_fmap_dev
