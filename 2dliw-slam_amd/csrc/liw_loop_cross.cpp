// liw_loop_cross.cpp — host side of the cross-robot loop detection (C ABI include/liw_loop_cross.h; kernels in k_loop_cross.hip):
// argument checks, the launches and the synchronous test getter.  The handle and the store are the fleet loop detector's
// (liw_loop_batch.cpp).  Bad arguments are reported before the missing device, so that the checks run on any machine.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/liw_loop_cross.h"
#include "k_loop_cross.hpp"
#include "liw_host_common.hpp"
#include "liw_loop_batch_ctx.hpp"

using liw_floop_dev::Lay;
using liw_xloop_dev::XPair;

extern "C" {

int liw_xloop_detect(liw_floop_ctx* c, const void* store, const unsigned char* key, const int* partner, const liw_xloop_params* params,
                     const unsigned char* mask, unsigned char* found, int* edge, double* tf12, double* T_w1_w2, double* rms, long long* stats,
                     void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || !key || !partner || !params || !found || !edge || !tf12 || !T_w1_w2 || !rms || !stats)
        return fail(c, LIW_EINVAL, "liw_xloop_detect: bad argument");
    if (params->min_match < c->P.g.thr || !(params->max_rms >= 0.0))
        return fail(c, LIW_EINVAL, "liw_xloop_detect: min_match below min_match_threshold, or max_rms negative or NaN");
    LIW_FLEET_DEV(c);
    liw_xloop_dev::XPrm x;
    x.min_match = params->min_match;
    x.max_rms = params->max_rms;
    // the robot regions are only read; the scratch area behind them is written, as by liw_floop_detect
    if (liw_xloop_dev::launch_cross_detect((char*)const_cast<void*>(store), c->L, c->P, x, key, partner, mask, found, edge, tf12, T_w1_w2, rms, stats,
                                           (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_xloop_detect: kernel launch failed");
    return LIW_OK;
}

int liw_xloop_partner(liw_floop_ctx* c, const int* group_of, const unsigned char* linked, int round, int* partner, void* stream) {
    if (!c) return LIW_EINVAL;
    if (!group_of || !linked || !partner || round < 0) return fail(c, LIW_EINVAL, "liw_xloop_partner: bad argument");
    LIW_FLEET_DEV(c);
    if (liw_xloop_dev::launch_partner(c->L.B, group_of, linked, round, partner, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_xloop_partner: kernel launch failed");
    return LIW_OK;
}

int liw_xloop_link(liw_floop_ctx* c, const int* group_of, const int* partner, const unsigned char* found, const int* edge, const double* T_w1_w2,
                   unsigned char* linked, double* T_g_w, int* via, int* group_linked, void* stream) {
    if (!c) return LIW_EINVAL;
    if (!group_of || !partner || !found || !edge || !T_w1_w2 || !linked || !T_g_w || !via || !group_linked)
        return fail(c, LIW_EINVAL, "liw_xloop_link: bad argument");
    LIW_FLEET_DEV(c);
    if (liw_xloop_dev::launch_link(c->L.B, group_of, partner, found, edge, T_w1_w2, linked, T_g_w, via, group_linked, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_xloop_link: kernel launch failed");
    return LIW_OK;
}

int liw_xloop_get_pair(liw_floop_ctx* c, const void* store, int robot, int cand, int cap, int* info, int* p1, int* p2) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || !info || robot < 0 || robot >= c->L.B || cap < 0) return fail(c, LIW_EINVAL, "liw_xloop_get_pair: bad argument");
    LIW_FLEET_DEV(c);
    const Lay& L = c->L;
    int n = 0, base = 0;
    if (!pull(store, L.f_cnt + (size_t)robot * 4, &n, 1) || !pull(store, L.f_base + (size_t)robot * 4, &base, 1))
        return fail(c, LIW_EHIP, "liw_xloop_get_pair: hipMemcpy");
    if (n < 0 || n > L.NC || base < 0 || (long long)base + n > (long long)L.B * L.NC) return fail(c, LIW_EINVAL, "liw_xloop_get_pair: no pair list");
    std::vector<XPair> pairs((size_t)std::max(n, 1));
    if (!pull(store, L.f_pairs + (size_t)base * sizeof(XPair), pairs.data(), (size_t)n)) return fail(c, LIW_EHIP, "liw_xloop_get_pair: hipMemcpy");
    int at = -1;
    for (int k = 0; k < n; ++k)
        if (pairs[(size_t)k].robot == robot && pairs[(size_t)k].cand == cand) at = k;
    if (at < 0) return fail(c, LIW_EINVAL, "liw_xloop_get_pair: the pair was not launched");
    const size_t pi = (size_t)base + at;
    int sm[8];
    if (!pull(store, L.f_summary + pi * 32, sm, 8)) return fail(c, LIW_EHIP, "liw_xloop_get_pair: hipMemcpy");
    const XPair& x = pairs[(size_t)at];
    for (int k = 0; k < 6; ++k) info[k] = sm[k];
    info[6] = sm[1] >= 0 && sm[1] < liw_xloop_dev::kDraws ? x.rows[sm[1]] : -1;
    info[7] = x.n2;
    const int len = std::max(0, std::min(sm[5], L.P));
    const int m = std::min(len, cap);
    std::vector<int> ls((size_t)std::max(2 * m, 1));
    if (!pull(store, L.f_lists + pi * L.P * 8, ls.data(), (size_t)2 * m)) return fail(c, LIW_EHIP, "liw_xloop_get_pair: hipMemcpy");
    for (int k = 0; k < m; ++k) {
        if (p1) p1[k] = ls[(size_t)2 * k];
        if (p2) p2[k] = ls[(size_t)2 * k + 1];
    }
    return len;
}

}  // extern "C"
