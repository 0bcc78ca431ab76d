// k_group_graph.hpp — what liw_group_graph.cpp (host: layout, argument checks, getters) and k_group_graph.hip (kernels and their
// launches) share: the store layout of include/liw_group_graph.h and the launch entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/liw_group_graph.h"

namespace liw_ggraph_dev {

// header of a group region: int32 words, then the summary (byte offsets in include/liw_group_graph.h)
constexpr int H_NE = 0, H_EFULL = 1, H_MFULL = 2, H_BAD = 3, H_SOLVES = 4, H_SKIPPED = 5, H_NODES = 6, H_USED = 7;
constexpr size_t HB_SUMMARY = 32, kHeaderBytes = 256, kEdgeBytes = 128, kEdgeTf = 32;
// what include/liw_group_gate.h adds: two header words behind the summary, and in an edge record the state word and chi2
constexpr int H_REJECTED = 16, H_GATED = 17, R_STATE = 5;
constexpr size_t kEdgeChi2 = 24;

struct Lay {
    int B, G, M, E;
    size_t group_bytes;                   // header + E edge records
    size_t work_off, work_group_bytes;    // group g's work area starts at work_off + g * work_group_bytes
    size_t w_nodes, w_const, w_enode, w_x, w_cand, w_y, w_scale, w_dgn, w_gd, w_Dd, w_Ye, w_Z, w_Hr, w_rhs;   // inside a work area (0: LM state)
    size_t bytes;
};

struct Noise { double J[36]; };   // edge_noise of the loop sigmas

constexpr int kLdsDoubles = 8192;   // 64 KiB: the most LDS k_ggraph_solve asks for

int launch_reset(char* store, const Lay& L, const unsigned char* gmask, hipStream_t s);
int launch_add_edges(char* store, const Lay& L, const int* group_of, const unsigned char* found, const int* edge, const double* tf12,
                     const unsigned char* mask, hipStream_t s);
int launch_partner(int B, const int* group_of, const unsigned char* linked, int round, int* partner, hipStream_t s);
int launch_solve(char* store, const Lay& L, const Noise& noise, const double* poses, long long robot_stride, const int* n_keyframes, const int* group_of,
                 const unsigned char* linked, const unsigned char* fixed, double* T_g_w, const unsigned char* gsel, int max_iters, int lds_cap_doubles,
                 liw_summary* summary, hipStream_t s);
int launch_gate(char* store, const Lay& L, const Noise& noise, const unsigned char* gsel, double chi2_max, int min_support, unsigned char* changed,
                hipStream_t s);

}  // namespace liw_ggraph_dev
