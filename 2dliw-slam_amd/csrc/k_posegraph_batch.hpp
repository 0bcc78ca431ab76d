// k_posegraph_batch.hpp — what liw_posegraph_batch.cpp (host: layout, argument checks, getters) and k_posegraph_batch.hip (kernels and
// their launches) share: the store layout of include/liw_posegraph_batch.h and the launch entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/liw_posegraph_batch.h"
#include "liw_kernels.hpp"

namespace liw_fpg_dev {

// header of a robot region: int32 words, then doubles (byte offsets in include/liw_posegraph_batch.h)
constexpr int H_NKF = 0, H_NLOOP = 1, H_FULL = 2, H_LFULL = 3, H_BAD = 4, H_PEND = 5, H_SOLVES = 6;
constexpr size_t HB_TLAST = 32, HB_MOD = 40, HB_SUMMARY = 136;

struct Lay {
    int B, K, ML;     // robots, max_keyframes, max_loops
    int NE;           // edge slots per robot: K - 1 sequential, then ML loops (at least 1)
    int NS;           // most separators of a robot
    size_t robot_bytes, r_stamp, r_tf, r_pose, r_seq, r_lidx, r_ltf;   // offsets inside a robot region
    size_t work_off, work_robot_bytes;                                 // robot b's work block starts at work_off + b * work_robot_bytes
    size_t w_x, w_cand, w_y, w_scale, w_dgn, w_Ye, w_Yg, w_Dd, w_gd, w_Os, w_Lb, w_sep, w_sepidx, w_Sred, w_rec, w_Hr, w_rhs;   // inside a work block (0: LM state)
    size_t g_count;   // one int32 behind the work blocks: robots still iterating
    size_t bytes;
};

// pose-graph noise and ground switches (liw_pg_params) in the form the factors read
struct Noise { double J[36]; double ground_on_p, ground_on_q, loop_edge_k; };

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_add_keyframes(char* store, const Lay& L, const unsigned char* key, const double* pose, const double* stamp, const unsigned char* mask,
                         unsigned char* added, hipStream_t s);
int launch_add_loops(char* store, const Lay& L, const unsigned char* found, const int* edge, const double* tf12, const unsigned char* mask, hipStream_t s);
int launch_due(char* store, const Lay& L, double period, const unsigned char* key, const double* stamp, const unsigned char* mask, unsigned char* due,
               int* n_due, hipStream_t s);
int launch_correct(char* store, const Lay& L, const double* pose_in, double* pose_out, const unsigned char* mask, hipStream_t s);
constexpr int kLdsDoubles = 8192;   // 64 KB: the most LDS k_fpg_reduced asks for
// the whole lock-step solve; lds_cap_doubles (0 .. kLdsDoubles): a separator triangle of more doubles runs from the work area;
// check_every > 0 reads the count of robots still iterating back every check_every iterations
int launch_solve(char* store, const Lay& L, const Noise& noise, const liw::DevParams& P, const unsigned char* sel, const double* stamp, int max_iters,
                 int check_every, int lds_cap_doubles, liw_summary* summary, hipStream_t s);

}  // namespace liw_fpg_dev
