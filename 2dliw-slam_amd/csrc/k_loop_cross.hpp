// k_loop_cross.hpp — interface between the cross-robot loop detection's host code (liw_loop_cross.cpp) and its kernels
// (k_loop_cross.hip).  The store, its layout Lay and the parameters Prm are the fleet loop detector's (k_loop_batch.hpp).
#pragma once
#include "k_loop_batch.hpp"

namespace liw_xloop_dev {

using liw_floop_dev::Lay;
using liw_floop_dev::Prm;
using liw_loop_dev::kDraws;

struct XPair {                   // one launched (query robot, candidate of its partner) pair, in the bytes of liw_floop_dev::Pair
    int robot, partner;          // robot regions of the query and of the candidate
    int cand, query;             // key-frame indices: cand in the partner, query in the robot
    int n1, n2;
    int rows[kDraws];            // drawn query rows, -1 for a repeated draw
    int pad;
};
static_assert(sizeof(XPair) == sizeof(liw_floop_dev::Pair), "XPair lives in the f_pairs bytes");

struct XRes {                    // ICP of a pair, in the bytes of liw_floop_dev::Res
    double tf12[12];
    double rms;                  // -1: the size gate rejected the pair (no ICP); a residual is never negative
};
static_assert(sizeof(XRes) == sizeof(liw_floop_dev::Res), "XRes lives in the f_res bytes");

struct XPrm {
    int min_match;
    double max_rms;
};

int launch_cross_detect(char* store, const Lay& L, const Prm& p, const XPrm& x, const unsigned char* key, const int* partner,
                        const unsigned char* mask, unsigned char* found, int* edge, double* tf12, double* T_w1_w2, double* rms, long long* stats,
                        hipStream_t s);
int launch_partner(int B, const int* group_of, const unsigned char* linked, int round, int* partner, hipStream_t s);
int launch_link(int B, const int* group_of, const int* partner, const unsigned char* found, const int* edge, const double* T_w1_w2,
                unsigned char* linked, double* T_g_w, int* via, int* group_linked, hipStream_t s);

}  // namespace liw_xloop_dev
