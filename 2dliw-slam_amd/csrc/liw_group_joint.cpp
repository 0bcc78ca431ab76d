// liw_group_joint.cpp — host side of the joint pose graph of a group (C ABI include/liw_group_joint.h; kernels in k_group_joint.hip):
// the store layout, the parts of the back-end and group-graph stores that the kernels read in place, argument checks, the launch and
// the synchronous getters.  No per-group work happens here.  Bad arguments are reported before the missing device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/liw_group_graph.h"
#include "../../include/liw_group_joint.h"
#include "../../include/liw_posegraph_batch.h"
#include "k_group_joint.hpp"
#include "k_posegraph_dev.hpp"
#include "liw_host_common.hpp"

void liw_fill_devparams(const liw_params* prm, liw::DevParams* dp);   // liw_capi.hip

namespace {

using namespace liw_gjoint_dev;

bool make_lay(const liw_gjoint_dims* d, Lay* L) {
    if (!d || d->B < 1 || d->G < 1 || d->max_keyframes < 1 || d->max_robot_loops < 0 || d->max_edges < 1 || d->max_members < 1 || d->max_nodes < 1 ||
        d->max_loops < 1 || d->max_members > 1024)
        return false;
    // the grids are over (group, node), (group, edge slot) and (robot, key frame) slots, in 32-bit block indices
    if ((long long)d->G * ((long long)d->max_nodes + d->max_loops) > 0x7fffffffLL || (long long)d->B * d->max_keyframes > 0x7fffffffLL ||
        (long long)d->max_nodes + 2LL * d->max_loops > 0x00ffffffLL)
        return false;
    L->B = d->B; L->G = d->G; L->K = d->max_keyframes; L->RL = d->max_robot_loops; L->E = d->max_edges; L->M = d->max_members; L->N = d->max_nodes;
    L->ML = d->max_loops;
    L->NE = L->N + L->ML;
    L->NS = (int)std::min<long long>(L->N, (long long)L->N / liw::PG_STRIDE + 2LL * L->M + 2LL * L->ML);
    // the two stores that are read in place, from their own layout calls and the part sizes their headers state
    liw_fpg_dims fd{d->B, d->max_keyframes, d->max_robot_loops};
    liw_fpg_layout_info fi{};
    size_t fpose = 0;
    if (liw_fpg_layout(&fd, &fi) != LIW_OK || liw_fpg_pose_offset(&fd, &fpose) != LIW_OK) return false;
    const size_t K = (size_t)L->K, RL = (size_t)L->RL;
    L->f_robot_bytes = fi.robot_bytes;
    L->f_pose = fpose;
    L->f_seq = al256(fpose + K * 48);
    L->f_lidx = al256(L->f_seq + K * 96);
    L->f_ltf = al256(L->f_lidx + RL * 8);
    if (al256(L->f_ltf + RL * 96) != fi.robot_bytes) return false;   // the layout stated in liw_posegraph_batch.h
    liw_ggraph_dims gd{d->B, d->G, 1, d->max_edges};
    liw_ggraph_layout_info gi{};
    if (liw_ggraph_layout(&gd, &gi) != LIW_OK) return false;
    L->gg_group_bytes = gi.group_bytes;
    const size_t B = (size_t)L->B, G = (size_t)L->G, M = (size_t)L->M, N = (size_t)L->N, ML = (size_t)L->ML, NE = (size_t)L->NE, NS = (size_t)L->NS, nr = 6 * NS;
    L->pose_off = 0;
    L->hdr_off = al256(B * K * 48);
    L->roff_off = L->hdr_off + G * kHeaderBytes;
    L->work_off = al256(L->roff_off + B * 4);
    size_t o = 256;   // the LM state
    L->w_mem = o; o = al256(o + M * 4);
    L->w_moff = o; o = al256(o + (M + 1) * 4);
    L->w_nmem = o; o = al256(o + N * 4);
    L->w_nrow = o; o = al256(o + N * 4);
    L->w_lidx = o; o = al256(o + ML * 8);
    L->w_ltf = o; o = al256(o + ML * 96);
    L->w_x = o; o = al256(o + N * 48);
    L->w_cand = o; o = al256(o + N * 48);
    L->w_y = o; o = al256(o + N * 48);
    L->w_scale = o; o = al256(o + N * 48);
    L->w_dgn = o; o = al256(o + N * 48);
    L->w_Ye = o; o = al256(o + NE * 78 * 8);
    L->w_Yg = o; o = al256(o + N * 14 * 8);
    L->w_Dd = o; o = al256(o + N * 36 * 8);
    L->w_gd = o; o = al256(o + N * 48);
    L->w_Os = o; o = al256(o + N * 36 * 8);
    L->w_Lb = o; o = al256(o + ML * 36 * 8);
    L->w_sep = o; o = al256(o + NS * 4);
    L->w_sepidx = o; o = al256(o + N * 4);
    L->w_Sred = o; o = al256(o + NS * liw::PG_SEG * 8);
    L->w_rec = o; o = al256(o + N * 78 * 8);
    L->w_Hr = o; o = al256(o + nr * (nr + 1) / 2 * 8);
    L->w_rhs = o; o = al256(o + nr * 8);
    L->work_group_bytes = o;
    L->g_count = L->work_off + G * L->work_group_bytes;
    L->bytes = L->g_count + 256;
    return true;
}

}  // namespace

struct liw_gjoint_ctx : liw_fleet_ctx_base {
    Lay L{};
    Noise noise{};
    liw::DevParams P{};
    int lds_cap = kLdsDoubles;
};

namespace {

// the first 16 header words of a group; < 0 on error
int group_header(liw_gjoint_ctx* c, const void* store, int group, int* hdr) {
    if (bad_store(store) || group < 0 || group >= c->L.G) return fail(c, LIW_EINVAL, "liw_gjoint: store or group");
    LIW_FLEET_DEV(c);
    if (!pull(store, c->L.hdr_off + (size_t)group * kHeaderBytes, hdr, 16)) return fail(c, LIW_EHIP, "liw_gjoint: hipMemcpy");
    return 0;
}
size_t work_of(const Lay& L, int group) { return L.work_off + (size_t)group * L.work_group_bytes; }

}  // namespace

extern "C" {

int liw_gjoint_layout(const liw_gjoint_dims* dims, liw_gjoint_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->pose_off = L.pose_off;
    out->header_off = L.hdr_off;
    out->work_off = L.work_off;
    out->work_group_bytes = L.work_group_bytes;
    out->max_separators = L.NS;
    out->tri_doubles = 3 * L.NS * (6 * L.NS + 1);
    return LIW_OK;
}

int liw_gjoint_store_bytes(const liw_gjoint_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

int liw_gjoint_pose_offset(const liw_gjoint_dims* dims, size_t* off) {
    Lay L{};
    if (!off || !make_lay(dims, &L)) return LIW_EINVAL;
    *off = L.pose_off;
    return LIW_OK;
}

liw_gjoint_ctx* liw_gjoint_create(const liw_params* params, const liw_pg_params* pg, const liw_gjoint_dims* dims, int device) {
    Lay L{};
    if (!params || !pg || !make_lay(dims, &L)) return nullptr;
    liw_gjoint_ctx* c = new liw_gjoint_ctx();
    c->L = L;
    c->device = device;
    liw_fill_devparams(params, &c->P);
    Noise& n = c->noise;
    for (int k = 0; k < 36; ++k) n.J[k] = (k % 7 == 0) ? 1.0 : 0.0;   // edge_noise (edge_factor.h:15-25), J(1,2) as written there
    n.J[0] = 1.0 / pg->loop_sigma_p[0]; n.J[1 * 6 + 2] = 1.0 / pg->loop_sigma_p[1]; n.J[2 * 6 + 2] = 1.0 / pg->loop_sigma_p[2];
    n.J[3 * 6 + 3] = 1.0 / pg->loop_sigma_q[0]; n.J[4 * 6 + 4] = 1.0 / pg->loop_sigma_q[1]; n.J[5 * 6 + 5] = 1.0 / pg->loop_sigma_q[2];
    n.ground_on_p = pg->use_ground_p_factor ? 1.0 : 0.0;
    n.ground_on_q = pg->use_ground_q_factor ? 1.0 : 0.0;
    n.loop_edge_k = pg->loop_edge_k;
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_gjoint_destroy(liw_gjoint_ctx* c) { delete c; }
const char* liw_gjoint_last_error(liw_gjoint_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_gjoint_set_lds_doubles(liw_gjoint_ctx* c, int doubles) {
    if (!c) return LIW_EINVAL;
    if (doubles < 0 || doubles > kLdsDoubles) return fail(c, LIW_EINVAL, "liw_gjoint_set_lds_doubles: outside 0 .. 8192");
    c->lds_cap = doubles;
    return LIW_OK;
}

int liw_gjoint_solve(liw_gjoint_ctx* c, void* store, const void* fpg_store, const void* ggraph_store, const int* group_of, const unsigned char* linked,
                     const unsigned char* fixed, const double* T_g_w, const unsigned char* gsel, int max_iters, int check_every, liw_summary* summary,
                     void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || bad_store(fpg_store) || bad_store(ggraph_store) || !group_of || !linked || !fixed || !T_g_w || !gsel || !summary)
        return fail(c, LIW_EINVAL, "liw_gjoint_solve: bad argument");
    LIW_FLEET_DEV(c);
    In in{(const char*)fpg_store, (const char*)ggraph_store, group_of, linked, fixed, T_g_w, gsel};
    if (launch_solve((char*)store, c->L, c->noise, c->P, in, max_iters, check_every, c->lds_cap, summary, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_gjoint_solve: kernel launch or read-back failed");
    return LIW_OK;
}

int liw_gjoint_get_header(liw_gjoint_ctx* c, const void* store, int group, int* words16) {
    if (!c) return LIW_EINVAL;
    if (!words16) return fail(c, LIW_EINVAL, "liw_gjoint_get_header: null output");
    int hdr[16];
    if (int r = group_header(c, store, group, hdr)) return r;
    std::copy(hdr, hdr + 16, words16);
    return LIW_OK;
}

int liw_gjoint_get_summary(liw_gjoint_ctx* c, const void* store, int group, liw_summary* summary) {
    if (!c) return LIW_EINVAL;
    if (!summary) return fail(c, LIW_EINVAL, "liw_gjoint_get_summary: null output");
    int hdr[16];
    if (int r = group_header(c, store, group, hdr)) return r;
    if (!pull(store, c->L.hdr_off + (size_t)group * kHeaderBytes + HB_SUMMARY, summary, 1)) return fail(c, LIW_EHIP, "liw_gjoint_get_summary: hipMemcpy");
    return LIW_OK;
}

int liw_gjoint_get_members(liw_gjoint_ctx* c, const void* store, int group, int cap, int* robots, int* offsets) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_gjoint_get_members: cap");
    int hdr[16];
    if (int r = group_header(c, store, group, hdr)) return r;
    const Lay& L = c->L;
    const int n = hdr[H_MFULL] ? 0 : std::max(0, std::min(hdr[H_MEMBERS], L.M)), m = std::min(n, cap);
    if ((robots && !pull(store, work_of(L, group) + L.w_mem, robots, (size_t)m)) || (offsets && !pull(store, work_of(L, group) + L.w_moff, offsets, (size_t)m)))
        return fail(c, LIW_EHIP, "liw_gjoint_get_members: hipMemcpy");
    return n;
}

int liw_gjoint_get_nodes(liw_gjoint_ctx* c, const void* store, int group, int cap, int* row, int* sepidx) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_gjoint_get_nodes: cap");
    int hdr[16];
    if (int r = group_header(c, store, group, hdr)) return r;
    const Lay& L = c->L;
    const bool full = hdr[H_MFULL] || hdr[H_NFULL] || hdr[H_LFULL];
    const int n = full ? 0 : std::max(0, std::min(hdr[H_NODES], L.N)), m = std::min(n, cap);
    if ((row && !pull(store, work_of(L, group) + L.w_nrow, row, (size_t)m)) || (sepidx && !pull(store, work_of(L, group) + L.w_sepidx, sepidx, (size_t)m)))
        return fail(c, LIW_EHIP, "liw_gjoint_get_nodes: hipMemcpy");
    return n;
}

int liw_gjoint_get_separators(liw_gjoint_ctx* c, const void* store, int group, int cap, int* sep) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_gjoint_get_separators: cap");
    int hdr[16];
    if (int r = group_header(c, store, group, hdr)) return r;
    const Lay& L = c->L;
    const int n = std::max(0, std::min(hdr[H_SEPS], L.NS)), m = std::min(n, cap);
    if (sep && !pull(store, work_of(L, group) + L.w_sep, sep, (size_t)m)) return fail(c, LIW_EHIP, "liw_gjoint_get_separators: hipMemcpy");
    return n;
}

}  // extern "C"
