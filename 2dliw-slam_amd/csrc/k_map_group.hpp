// k_map_group.hpp — interface between the group map's host code (liw_map_group.cpp) and its kernels (k_map_group.hip), and what the
// group map borrows from a fleet-map context (liw_map_batch.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "k_map_batch.hpp"

struct liw_fmap_ctx;

namespace liw_fmap_dev {

// header of a group region: int32 words, then the held liw_map_info at HB_INFO
constexpr int GH_STATUS = 0, GH_MEMBERS = 1, GH_SUBMAPS = 2;

struct GLay {                        // byte offsets within a group region (g_*)
    int G, C;                        // groups, max_cells of one group's grid
    int cchunk;                      // work-groups per group of k_gmap_clear and k_gmap_finish
    size_t Cn;                       // max_cells rounded up to 16
    size_t g_bits, g_grid, group_bytes, bytes;
};

struct FmapView {                    // what liw_gmap_create copies out of a liw_fmap_ctx
    Lay L;
    double Til[12];
    int device;
    bool have_device;
};
FmapView fmap_view(const liw_fmap_ctx* c);   // liw_map_batch.cpp

int launch_group_reset(char* gstore, const GLay& GL, double res, const unsigned char* gmask, hipStream_t s);
// poses != nullptr: T_w_l = make_tf(p, q) * Til is composed first; T_g_w == nullptr: T_g_l = T_w_l bit for bit
int launch_group_render(char* store, const Lay& L, char* gstore, const GLay& GL, const double* T_w_l, const double* poses, const double* Til,
                        long long robot_stride, const int* group_of, const double* T_g_w, const unsigned char* gsel, int* gstatus, void* ginfo,
                        hipStream_t s);

}  // namespace liw_fmap_dev
