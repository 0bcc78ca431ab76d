// k_loop_batch.hpp — interface between the fleet loop detector's host code (liw_loop_batch.cpp) and its kernels (k_loop_batch.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "k_loop.hpp"

namespace liw_floop_dev {

using liw_loop_dev::Geom;
using liw_loop_dev::kDraws;

struct Lay {                     // the store: byte offsets inside a robot region (r_*) and inside the whole store (f_*)
    int B, K, P, C, S, step, NC, NS, W;
    size_t r_tf, r_state, r_npts, r_ringn, r_ring, r_pts, r_keys, r_aij, r_quick, robot_bytes, feature_bytes;
    size_t f_hdr, f_work, f_cnt, f_base, f_cmax, f_pre, f_pairs, f_tres, f_summary, f_lists, f_res, bytes;
};

// feature slot of key frame k: a candidate slot when k % s == 0, else the one query slot (which holds the newest such k only)
__host__ __device__ inline int feature_slot(const Lay& L, int k) { return k % L.step == 0 ? k / L.step : L.NC; }

struct Prm {
    Geom g;
    double d_res, max_dis, max_tf_p, max_tf_q;
    int min_interval;
    unsigned long long seed;
    double Tiw[12];
};

struct Pre {                     // gate result of (robot, candidate index), before compaction
    int rank;                    // position among the robot's launched candidates, -1: not launched
    int n2;
    int rows[kDraws];
    int pad;
};

struct Pair {                    // one launched (robot, candidate) pair of the compact list
    int robot, cand, query;      // key-frame indices
    int n1, n2;
    int rows[kDraws];            // drawn query rows, -1 for a repeated draw
    int pad[2];
};

struct Res {                     // ICP + tf gate of a pair
    double tf12[12];
    int checked, pass;
};

size_t gather_lds(const Lay& L);
size_t describe_lds(const Lay& L);
size_t match_lds(const Lay& L, const Geom& g);

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_add(char* store, const Lay& L, const Prm& p, const unsigned char* key, const double* pose, const double* corners, int stride,
               const int* n_corners, const unsigned char* mask, unsigned char* added, hipStream_t s);
int launch_detect(char* store, const Lay& L, const Prm& p, const unsigned char* key, const unsigned char* mask, unsigned char* found, int* edge,
                  double* tf12, long long* stats, hipStream_t s);
// k_floop_scan alone (f_cnt, f_cmax -> f_base, f_hdr), for the cross detection of k_loop_cross.hip
int launch_scan(char* store, const Lay& L, hipStream_t s);

}  // namespace liw_floop_dev
