// k_map_locate.hpp — interface between the localiser's host code (liw_map_locate.cpp) and its kernels (k_map_locate.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace liw_floc_dev {

// header of a map region: int32 words, then the liw_map_info copied from the source at HB_INFO (as in a fleet-map region)
constexpr int FH_STATUS = 0, FH_OCC = 1, FH_NEAR = 2;
constexpr size_t HB_INFO = 32;
constexpr int kRecInts = 8;          // int32 per partial record: score, ix, iy, ties, n_valid, 0, 0, 0
constexpr int REC_SCORE = 0, REC_IX = 1, REC_IY = 2, REC_TIES = 3, REC_NVALID = 4;

struct FLay {
    int Q, M, C, T;                  // query rows, map regions, max_cells, max_theta
    int cchunk;                      // work-groups per map of k_floc_field
    size_t Cn;                       // max_cells rounded up to 16
    size_t m_field, map_bytes;       // within a map region
    size_t s_partial, row_bytes, bytes;
};

struct MatchArgs {
    const int* map_of;
    const double* points;
    int point_stride;
    const int* n_points;
    const double* T0;
    const double* table;
    int n_theta, W, min_permille;
    const unsigned char* mask;
    unsigned char* found;
    int* best;
    int* stats;
    double* T_m_l;
};

int launch_build(char* lstore, const FLay& L, const char* src_store, size_t region_bytes, size_t grid_off, const int* src_of,
                 const unsigned char* msel, hipStream_t s);
int launch_match(char* lstore, const FLay& L, const MatchArgs& a, hipStream_t s);
int launch_link_tf(int Q, const double* T_m_l, const double* poses, long long robot_stride, const double* Til, const unsigned char* found,
                   const unsigned char* mask, double* T_w_l, double* T_g_w, hipStream_t s);

}  // namespace liw_floc_dev
