// k_group_joint.hpp — what liw_group_joint.cpp (host: layout, argument checks, getters) and k_group_joint.hip (kernels and their
// launches) share: the store layout of include/liw_group_joint.h, the parts of the two stores that are read in place, and the launch
// entry point.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/liw_group_joint.h"
#include "liw_kernels.hpp"

namespace liw_gjoint_dev {

// header of a group: int32 words, then the summary (include/liw_group_joint.h)
constexpr int H_RESERVED = 0, H_MFULL = 1, H_NFULL = 2, H_LFULL = 3, H_MEMBERS = 4, H_NODES = 5, H_SEQ = 6, H_OWN = 7, H_USED = 8, H_SKIPPED = 9,
              H_SEPS = 10, H_SOLVED = 11, H_CONST = 12;
constexpr size_t HB_SUMMARY = 64, kHeaderBytes = 256;

struct Lay {
    int B, G, K, RL, E, M, N, ML;   // robots, groups, back-end max_keyframes / max_loops, group-graph max_edges, max_members / nodes / loops
    int NE;                          // edge slots of a group: N sequential (slot n: the edge into node n), then ML loops
    int NS;                          // most separators of a group
    // the back-end store (include/liw_posegraph_batch.h): region of a robot and its parts
    size_t f_robot_bytes, f_pose, f_seq, f_lidx, f_ltf;
    // the group-graph store (include/liw_group_graph.h): region of a group; header 256 B, records of 128 B with tf12 at byte 32
    size_t gg_group_bytes;
    size_t pose_off, hdr_off, roff_off, work_off, work_group_bytes;
    size_t w_mem, w_moff, w_nmem, w_nrow, w_lidx, w_ltf, w_x, w_cand, w_y, w_scale, w_dgn, w_Ye, w_Yg, w_Dd, w_gd, w_Os, w_Lb, w_sep, w_sepidx,
        w_Sred, w_rec, w_Hr, w_rhs;   // inside a work area (0: LM state)
    size_t g_count;                   // one int32 behind the work areas: groups still iterating
    size_t bytes;
};

struct Noise { double J[36]; double ground_on_p, ground_on_q, loop_edge_k; };

struct In {   // the inputs of a solve, all device pointers
    const char* fpg; const char* gg; const int* group_of; const unsigned char* linked; const unsigned char* fixed; const double* T_g_w;
    const unsigned char* gsel;
};

constexpr int kLdsDoubles = 8192;   // 64 KiB: the most LDS k_gj_reduced asks for

int launch_solve(char* store, const Lay& L, const Noise& noise, const liw::DevParams& P, const In& in, int max_iters, int check_every,
                 int lds_cap_doubles, liw_summary* summary, hipStream_t s);

}  // namespace liw_gjoint_dev
