// liw_group_graph.cpp — host side of the group pose graph (C ABI include/liw_group_graph.h, and include/liw_group_gate.h on the same ctx
// and store; kernels in k_group_graph.hip): the store layout, argument checks, the launches and the synchronous getters.  No per-group
// work happens here.  Bad arguments are reported before the missing device, so that the checks run on any machine.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/liw_group_gate.h"
#include "../../include/liw_group_graph.h"
#include "k_group_graph.hpp"
#include "liw_host_common.hpp"

namespace {

using namespace liw_ggraph_dev;

bool make_lay(const liw_ggraph_dims* d, Lay* L) {
    if (!d || d->B < 1 || d->G < 1 || d->max_members < 1 || d->max_edges < 1 || d->max_members > 1024 || d->max_edges > 65536) return false;
    L->B = d->B; L->G = d->G; L->M = d->max_members; L->E = d->max_edges;
    const size_t M = (size_t)L->M, E = (size_t)L->E, G = (size_t)L->G, nr = 6 * M;
    L->group_bytes = al256(kHeaderBytes + E * kEdgeBytes);
    size_t o = 256;   // the LM state
    L->w_nodes = o; o = al256(o + M * 4);
    L->w_const = o; o = al256(o + M * 4);
    L->w_enode = o; o = al256(o + E * 12);
    L->w_x = o; o = al256(o + M * 48);
    L->w_cand = o; o = al256(o + M * 48);
    L->w_y = o; o = al256(o + M * 48);
    L->w_scale = o; o = al256(o + M * 48);
    L->w_dgn = o; o = al256(o + M * 48);
    L->w_gd = o; o = al256(o + M * 48);
    L->w_Dd = o; o = al256(o + M * 36 * 8);
    L->w_Ye = o; o = al256(o + E * 78 * 8);
    L->w_Z = o; o = al256(o + E * 36 * 8);
    L->w_Hr = o; o = al256(o + nr * (nr + 1) / 2 * 8);
    L->w_rhs = o; o = al256(o + nr * 8);
    L->work_group_bytes = o;
    L->work_off = G * L->group_bytes;
    L->bytes = L->work_off + G * L->work_group_bytes;
    return true;
}

}  // namespace

struct liw_ggraph_ctx : liw_fleet_ctx_base {
    Lay L{};
    Noise noise{};
    int lds_cap = kLdsDoubles;
};

namespace {

// the eight header words of a group; < 0 on error
int group_header(liw_ggraph_ctx* c, const void* store, int group, int* hdr) {
    if (bad_store(store) || group < 0 || group >= c->L.G) return fail(c, LIW_EINVAL, "liw_ggraph: store or group");
    LIW_FLEET_DEV(c);
    if (!pull(store, (size_t)group * c->L.group_bytes, hdr, 8)) return fail(c, LIW_EHIP, "liw_ggraph: hipMemcpy");
    return 0;
}

}  // namespace

extern "C" {

int liw_ggraph_layout(const liw_ggraph_dims* dims, liw_ggraph_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->group_bytes = L.group_bytes;
    out->work_off = L.work_off;
    out->work_bytes = L.bytes - L.work_off;
    out->work_group_bytes = L.work_group_bytes;
    out->tri_doubles = 3 * L.M * (6 * L.M + 1);
    return LIW_OK;
}

int liw_ggraph_store_bytes(const liw_ggraph_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_ggraph_ctx* liw_ggraph_create(const liw_pg_params* pg, const liw_ggraph_dims* dims, int device) {
    Lay L{};
    if (!pg || !make_lay(dims, &L)) return nullptr;
    liw_ggraph_ctx* c = new liw_ggraph_ctx();
    c->L = L;
    c->device = device;
    double* J = c->noise.J;
    for (int k = 0; k < 36; ++k) J[k] = (k % 7 == 0) ? 1.0 : 0.0;   // edge_noise (edge_factor.h:15-25), J(1,2) as written there
    J[0] = 1.0 / pg->loop_sigma_p[0]; J[1 * 6 + 2] = 1.0 / pg->loop_sigma_p[1]; J[2 * 6 + 2] = 1.0 / pg->loop_sigma_p[2];
    J[3 * 6 + 3] = 1.0 / pg->loop_sigma_q[0]; J[4 * 6 + 4] = 1.0 / pg->loop_sigma_q[1]; J[5 * 6 + 5] = 1.0 / pg->loop_sigma_q[2];
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_ggraph_destroy(liw_ggraph_ctx* c) { delete c; }
const char* liw_ggraph_last_error(liw_ggraph_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_ggraph_set_lds_doubles(liw_ggraph_ctx* c, int doubles) {
    if (!c) return LIW_EINVAL;
    if (doubles < 0 || doubles > kLdsDoubles) return fail(c, LIW_EINVAL, "liw_ggraph_set_lds_doubles: outside 0 .. 8192");
    c->lds_cap = doubles;
    return LIW_OK;
}

int liw_ggraph_reset(liw_ggraph_ctx* c, void* store, const unsigned char* gmask, void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store)) return fail(c, LIW_EINVAL, "liw_ggraph_reset: store");
    LIW_FLEET_DEV(c);
    if (launch_reset((char*)store, c->L, gmask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_ggraph_reset: kernel launch failed");
    return LIW_OK;
}

int liw_ggraph_add_edges(liw_ggraph_ctx* c, void* store, const int* group_of, const unsigned char* found, const int* edge, const double* tf12,
                         const unsigned char* mask, void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || !group_of || !found || !edge || !tf12) return fail(c, LIW_EINVAL, "liw_ggraph_add_edges: bad argument");
    LIW_FLEET_DEV(c);
    if (launch_add_edges((char*)store, c->L, group_of, found, edge, tf12, mask, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_ggraph_add_edges: kernel launch failed");
    return LIW_OK;
}

int liw_ggraph_partner(liw_ggraph_ctx* c, const int* group_of, const unsigned char* linked, int round, int* partner, void* stream) {
    if (!c) return LIW_EINVAL;
    if (!group_of || !linked || !partner || round < 0) return fail(c, LIW_EINVAL, "liw_ggraph_partner: bad argument");
    LIW_FLEET_DEV(c);
    if (launch_partner(c->L.B, group_of, linked, round, partner, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_ggraph_partner: kernel launch failed");
    return LIW_OK;
}

int liw_ggraph_solve(liw_ggraph_ctx* c, void* store, const double* poses, long long robot_stride, const int* n_keyframes, const int* group_of,
                     const unsigned char* linked, const unsigned char* fixed, double* T_g_w, const unsigned char* gsel, int max_iters,
                     liw_summary* summary, void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || !poses || robot_stride < 0 || !n_keyframes || !group_of || !linked || !fixed || !T_g_w || !gsel || !summary)
        return fail(c, LIW_EINVAL, "liw_ggraph_solve: bad argument");
    LIW_FLEET_DEV(c);
    if (launch_solve((char*)store, c->L, c->noise, poses, robot_stride, n_keyframes, group_of, linked, fixed, T_g_w, gsel, max_iters, c->lds_cap, summary,
                     (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_ggraph_solve: kernel launch failed");
    return LIW_OK;
}

int liw_ggraph_get_edges(liw_ggraph_ctx* c, const void* store, int group, int cap, int* idx, double* tf12) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_ggraph_get_edges: cap");
    int hdr[8];
    if (int r = group_header(c, store, group, hdr)) return r;
    const int n = std::max(0, std::min(hdr[H_NE], c->L.E)), m = std::min(n, cap);
    std::vector<char> rec((size_t)std::max(m, 1) * kEdgeBytes);
    if (!pull(store, (size_t)group * c->L.group_bytes + kHeaderBytes, rec.data(), (size_t)m * kEdgeBytes)) return fail(c, LIW_EHIP, "liw_ggraph_get_edges: hipMemcpy");
    for (int e = 0; e < m; ++e) {
        const char* r = rec.data() + (size_t)e * kEdgeBytes;
        if (idx) std::copy((const int*)r, (const int*)r + 5, idx + (size_t)e * 5);
        if (tf12) std::copy((const double*)(r + kEdgeTf), (const double*)(r + kEdgeTf) + 12, tf12 + (size_t)e * 12);
    }
    return n;
}

int liw_ggraph_get_flags(liw_ggraph_ctx* c, const void* store, int group, int* flags8) {
    if (!c) return LIW_EINVAL;
    if (!flags8) return fail(c, LIW_EINVAL, "liw_ggraph_get_flags: null flags");
    int hdr[8];
    if (int r = group_header(c, store, group, hdr)) return r;
    std::copy(hdr, hdr + 8, flags8);
    return LIW_OK;
}

int liw_ggraph_get_summary(liw_ggraph_ctx* c, const void* store, int group, liw_summary* summary) {
    if (!c) return LIW_EINVAL;
    if (!summary) return fail(c, LIW_EINVAL, "liw_ggraph_get_summary: null output");
    int hdr[8];
    if (int r = group_header(c, store, group, hdr)) return r;
    if (!pull(store, (size_t)group * c->L.group_bytes + HB_SUMMARY, summary, 1)) return fail(c, LIW_EHIP, "liw_ggraph_get_summary: hipMemcpy");
    return LIW_OK;
}

int liw_ggraph_get_Z(liw_ggraph_ctx* c, const void* store, int group, int cap, int* used, double* Z, double* Ta, double* Tb) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_ggraph_get_Z: cap");
    int hdr[8];
    if (int r = group_header(c, store, group, hdr)) return r;
    const Lay& L = c->L;
    const int n = std::max(0, std::min(hdr[H_NE], L.E)), m = std::min(n, cap);
    const size_t W = L.work_off + (size_t)group * L.work_group_bytes;
    std::vector<int> en((size_t)std::max(m, 1) * 3);
    std::vector<double> z((size_t)std::max(m, 1) * 36);
    if (!pull(store, W + L.w_enode, en.data(), (size_t)m * 3) || !pull(store, W + L.w_Z, z.data(), (size_t)m * 36)) return fail(c, LIW_EHIP, "liw_ggraph_get_Z: hipMemcpy");
    for (int e = 0; e < m; ++e) {
        const double* s = &z[(size_t)e * 36];
        if (used) used[e] = en[(size_t)e * 3 + 2];
        if (Z) std::copy(s, s + 12, Z + (size_t)e * 12);
        if (Ta) std::copy(s + 12, s + 24, Ta + (size_t)e * 12);
        if (Tb) std::copy(s + 24, s + 36, Tb + (size_t)e * 12);
    }
    return n;
}

// ---- include/liw_group_gate.h: the same ctx and store
int liw_ggate_gate(liw_ggraph_ctx* c, void* store, const unsigned char* gsel, double chi2_max, int min_support, unsigned char* changed, void* stream) {
    if (!c) return LIW_EINVAL;
    if (bad_store(store) || !gsel || !changed || !(chi2_max > 0.0) || !std::isfinite(chi2_max) || min_support < 1)
        return fail(c, LIW_EINVAL, "liw_ggate_gate: bad argument");
    LIW_FLEET_DEV(c);
    if (launch_gate((char*)store, c->L, c->noise, gsel, chi2_max, min_support, changed, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_ggate_gate: kernel launch failed");
    return LIW_OK;
}

int liw_ggate_get(liw_ggraph_ctx* c, const void* store, int group, int cap, int* state, double* chi2, int* counts2) {
    if (!c) return LIW_EINVAL;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_ggate_get: cap");
    int hdr[8];
    if (int r = group_header(c, store, group, hdr)) return r;
    const size_t G0 = (size_t)group * c->L.group_bytes;
    const int n = std::max(0, std::min(hdr[H_NE], c->L.E)), m = std::min(n, cap);
    std::vector<char> rec((size_t)std::max(m, 1) * kEdgeBytes);
    int counts[2];
    if (!pull(store, G0 + kHeaderBytes, rec.data(), (size_t)m * kEdgeBytes) || !pull(store, G0 + 4 * (size_t)H_REJECTED, counts, 2))
        return fail(c, LIW_EHIP, "liw_ggate_get: hipMemcpy");
    for (int e = 0; e < m; ++e) {
        const char* r = rec.data() + (size_t)e * kEdgeBytes;
        if (state) state[e] = ((const int*)r)[R_STATE];
        if (chi2) chi2[e] = *(const double*)(r + kEdgeChi2);
    }
    if (counts2) { counts2[0] = counts[0]; counts2[1] = counts[1]; }
    return n;
}

}  // extern "C"
