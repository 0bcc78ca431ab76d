// liw_posegraph_batch.cpp — host side of the fleet pose-graph back-end (C ABI include/liw_posegraph_batch.h; kernels in
// k_posegraph_batch.hip): the store layout, argument checks, the launches and the synchronous getters.  No per-robot work happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_lie.h"
#include "../../include/liw_posegraph_batch.h"
#include "k_posegraph_batch.hpp"
#include "k_posegraph_dev.hpp"
#include "liw_host_common.hpp"

void liw_fill_devparams(const liw_params* prm, liw::DevParams* dp);   // liw_capi.hip

namespace {

using liw_fpg_dev::Lay;
using namespace liw_fpg_dev;

bool make_lay(const liw_fpg_dims* d, Lay* L) {
    if (!d || d->B < 1 || d->max_keyframes < 1 || d->max_loops < 0) return false;
    // the grids are over (robot, key frame) and (robot, edge) slots, in 32-bit block indices
    if ((long long)d->B * ((long long)d->max_keyframes + d->max_loops) > 0x7fffffffLL || (long long)d->max_keyframes + 2LL * d->max_loops > 0x0fffffffLL) return false;
    L->B = d->B; L->K = d->max_keyframes; L->ML = d->max_loops;
    L->NE = std::max(1, L->K - 1 + L->ML);
    L->NS = std::min(L->K, (L->K + 47) / 48 + 1 + 2 * L->ML);
    const size_t K = (size_t)L->K, ML = (size_t)L->ML, NE = (size_t)L->NE, NS = (size_t)L->NS, B = (size_t)L->B, nr = 6 * NS;
    size_t o = 256;
    L->r_stamp = o; o = al256(o + K * 8);
    L->r_tf = o; o = al256(o + K * 96);
    L->r_pose = o; o = al256(o + K * 48);
    L->r_seq = o; o = al256(o + K * 96);
    L->r_lidx = o; o = al256(o + ML * 8);
    L->r_ltf = o; o = al256(o + ML * 96);
    L->robot_bytes = o;
    o = 256;   // the LM state
    L->w_x = o; o = al256(o + K * 48);
    L->w_cand = o; o = al256(o + K * 48);
    L->w_y = o; o = al256(o + K * 48);
    L->w_scale = o; o = al256(o + K * 48);
    L->w_dgn = o; o = al256(o + K * 48);
    L->w_Ye = o; o = al256(o + NE * 78 * 8);
    L->w_Yg = o; o = al256(o + K * 14 * 8);
    L->w_Dd = o; o = al256(o + K * 36 * 8);
    L->w_gd = o; o = al256(o + K * 48);
    L->w_Os = o; o = al256(o + K * 36 * 8);
    L->w_Lb = o; o = al256(o + ML * 36 * 8);
    L->w_sep = o; o = al256(o + NS * 4);
    L->w_sepidx = o; o = al256(o + K * 4);
    L->w_Sred = o; o = al256(o + NS * liw::PG_SEG * 8);
    L->w_rec = o; o = al256(o + K * 78 * 8);
    L->w_Hr = o; o = al256(o + nr * (nr + 1) / 2 * 8);
    L->w_rhs = o; o = al256(o + nr * 8);
    L->work_robot_bytes = o;
    L->work_off = B * L->robot_bytes;
    L->g_count = L->work_off + B * L->work_robot_bytes;
    L->bytes = L->g_count + 256;
    return true;
}

}  // namespace

struct liw_fpg_ctx : liw_fleet_ctx_base {
    Lay L{};
    Noise noise{};
    liw::DevParams P{};
    double period = 0.0;
    int lds_cap = kLdsDoubles;
};

namespace {

// the eight header words of a robot; < 0 on error
int robot_header(liw_fpg_ctx* c, const void* store, int robot, int* hdr) {
    if (bad_store(store) || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_fpg: store or robot");
    if (!pull(store, (size_t)robot * c->L.robot_bytes, hdr, 8)) return fail(c, LIW_EHIP, "liw_fpg: hipMemcpy");
    return 0;
}

}  // namespace

extern "C" {

int liw_fpg_layout(const liw_fpg_dims* dims, liw_fpg_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->robot_bytes = L.robot_bytes;
    out->work_off = L.work_off;
    out->work_bytes = L.bytes - L.work_off;
    out->work_robot_bytes = L.work_robot_bytes;
    out->max_separators = L.NS;
    out->edge_slots = L.K - 1 + L.ML;
    return LIW_OK;
}

int liw_fpg_pose_offset(const liw_fpg_dims* dims, size_t* off) {
    Lay L{};
    if (!off || !make_lay(dims, &L)) return LIW_EINVAL;
    *off = L.r_pose;
    return LIW_OK;
}

int liw_fpg_store_bytes(const liw_fpg_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_fpg_ctx* liw_fpg_create(const liw_params* params, const liw_pg_params* pg, const liw_fpg_dims* dims, double solve_period, int device) {
    Lay L{};
    if (!params || !pg || !std::isfinite(solve_period) || !make_lay(dims, &L)) return nullptr;
    liw_fpg_ctx* c = new liw_fpg_ctx();
    c->L = L;
    c->device = device;
    c->period = solve_period;
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

void liw_fpg_destroy(liw_fpg_ctx* c) { delete c; }
const char* liw_fpg_last_error(liw_fpg_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_fpg_set_lds_doubles(liw_fpg_ctx* c, int doubles) {
    if (!c) return LIW_EINVAL;
    if (doubles < 0 || doubles > kLdsDoubles) return fail(c, LIW_EINVAL, "liw_fpg_set_lds_doubles: outside 0 .. 8192");
    c->lds_cap = doubles;
    return LIW_OK;
}

int liw_fpg_reset(liw_fpg_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store)) return fail(c, LIW_EINVAL, "liw_fpg_reset: store");
    if (launch_reset((char*)store, c->L, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpg_reset: kernel launch failed");
    return LIW_OK;
}

int liw_fpg_add_keyframes(liw_fpg_ctx* c, void* store, const unsigned char* key, const double* pose, const double* stamp, const unsigned char* mask,
                          unsigned char* added, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !key || !pose || !stamp) return fail(c, LIW_EINVAL, "liw_fpg_add_keyframes: bad argument");
    if (launch_add_keyframes((char*)store, c->L, key, pose, stamp, mask, added, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fpg_add_keyframes: kernel launch failed");
    return LIW_OK;
}

int liw_fpg_add_loops(liw_fpg_ctx* c, void* store, const unsigned char* found, const int* edge, const double* tf12, const unsigned char* mask,
                      void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !found || !edge || !tf12) return fail(c, LIW_EINVAL, "liw_fpg_add_loops: bad argument");
    if (launch_add_loops((char*)store, c->L, found, edge, tf12, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpg_add_loops: kernel launch failed");
    return LIW_OK;
}

int liw_fpg_due(liw_fpg_ctx* c, void* store, const unsigned char* key, const double* stamp, const unsigned char* mask, unsigned char* due, int* n_due,
                void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !key || !stamp || !due) return fail(c, LIW_EINVAL, "liw_fpg_due: bad argument");
    if (launch_due((char*)store, c->L, c->period, key, stamp, mask, due, n_due, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpg_due: kernel launch failed");
    return LIW_OK;
}

int liw_fpg_solve(liw_fpg_ctx* c, void* store, const unsigned char* sel, const double* stamp, int max_iters, int check_every, liw_summary* summary,
                  void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !sel || !stamp || !summary) return fail(c, LIW_EINVAL, "liw_fpg_solve: bad argument");
    if (launch_solve((char*)store, c->L, c->noise, c->P, sel, stamp, max_iters, check_every, c->lds_cap, summary, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fpg_solve: kernel launch or read-back failed");
    return LIW_OK;
}

int liw_fpg_correct(liw_fpg_ctx* c, void* store, const double* pose_in, double* pose_out, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !pose_in || !pose_out) return fail(c, LIW_EINVAL, "liw_fpg_correct: bad argument");
    if (launch_correct((char*)store, c->L, pose_in, pose_out, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpg_correct: kernel launch failed");
    return LIW_OK;
}

int liw_fpg_num_keyframes(liw_fpg_ctx* c, const void* store, int robot) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    return hdr[H_NKF];
}

int liw_fpg_flags(liw_fpg_ctx* c, const void* store, int robot, int* flags6, double* last_solve_time) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (!flags6) return fail(c, LIW_EINVAL, "liw_fpg_flags: null flags");
    if (int r = robot_header(c, store, robot, hdr)) return r;
    for (int k = 0; k < 6; ++k) flags6[k] = hdr[1 + k];
    if (last_solve_time && !pull(store, (size_t)robot * c->L.robot_bytes + HB_TLAST, last_solve_time, 1)) return fail(c, LIW_EHIP, "liw_fpg_flags: hipMemcpy");
    return LIW_OK;
}

int liw_fpg_get_keyframes(liw_fpg_ctx* c, const void* store, int robot, int cap, double* poses, double* stamps, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_fpg_get_keyframes: cap");
    const size_t m = (size_t)std::min(hdr[H_NKF], cap), base = (size_t)robot * c->L.robot_bytes;
    if ((poses && !pull(store, base + c->L.r_pose, poses, m * 6)) || (stamps && !pull(store, base + c->L.r_stamp, stamps, m)) ||
        (tf12 && !pull(store, base + c->L.r_tf, tf12, m * 12)))
        return fail(c, LIW_EHIP, "liw_fpg_get_keyframes: hipMemcpy");
    return hdr[H_NKF];
}

int liw_fpg_get_seq_edges(liw_fpg_ctx* c, const void* store, int robot, int cap, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_fpg_get_seq_edges: cap");
    const int n = std::max(0, hdr[H_NKF] - 1);
    if (tf12 && !pull(store, (size_t)robot * c->L.robot_bytes + c->L.r_seq + 96, tf12, (size_t)std::min(n, cap) * 12))
        return fail(c, LIW_EHIP, "liw_fpg_get_seq_edges: hipMemcpy");
    return n;
}

int liw_fpg_get_loop_edges(liw_fpg_ctx* c, const void* store, int robot, int cap, int* idx, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (cap < 0) return fail(c, LIW_EINVAL, "liw_fpg_get_loop_edges: cap");
    const size_t m = (size_t)std::min(hdr[H_NLOOP], cap), base = (size_t)robot * c->L.robot_bytes;
    if ((idx && !pull(store, base + c->L.r_lidx, idx, m * 2)) || (tf12 && !pull(store, base + c->L.r_ltf, tf12, m * 12)))
        return fail(c, LIW_EHIP, "liw_fpg_get_loop_edges: hipMemcpy");
    return hdr[H_NLOOP];
}

int liw_fpg_get_modify_delta_tf(liw_fpg_ctx* c, const void* store, int robot, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (!tf12) return fail(c, LIW_EINVAL, "liw_fpg_get_modify_delta_tf: null output");
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (!pull(store, (size_t)robot * c->L.robot_bytes + HB_MOD, tf12, 12)) return fail(c, LIW_EHIP, "liw_fpg_get_modify_delta_tf: hipMemcpy");
    return LIW_OK;
}

int liw_fpg_get_summary(liw_fpg_ctx* c, const void* store, int robot, liw_summary* summary) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (!summary) return fail(c, LIW_EINVAL, "liw_fpg_get_summary: null output");
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (!pull(store, (size_t)robot * c->L.robot_bytes + HB_SUMMARY, summary, 1)) return fail(c, LIW_EHIP, "liw_fpg_get_summary: hipMemcpy");
    return LIW_OK;
}

int liw_fpg_load_graph(liw_fpg_ctx* c, void* store, int robot, int N, const double* poses, const double* stamps, const double* seq_tf12, int n_loop,
                       const int* loop_idx, const double* loop_tf12) {
    LIW_FLEET_DEV(c);
    const Lay& L = c->L;
    if (bad_store(store) || robot < 0 || robot >= L.B || N < 1 || N > L.K || !poses || (N > 1 && !seq_tf12) || n_loop < 0 || n_loop > L.ML ||
        (n_loop && (!loop_idx || !loop_tf12)))
        return fail(c, LIW_EINVAL, "liw_fpg_load_graph: bad argument");
    for (int e = 0; e < 2 * n_loop; ++e)
        if (loop_idx[e] < 0 || loop_idx[e] >= N || (e % 2 && loop_idx[e] == loop_idx[e - 1])) return fail(c, LIW_EINVAL, "liw_fpg_load_graph: loop index");
    std::vector<char> hdr(256, 0);
    int* h = (int*)hdr.data();
    h[H_NKF] = N; h[H_NLOOP] = n_loop; h[H_PEND] = n_loop > 0;
    *(double*)(hdr.data() + HB_TLAST) = -1e300;
    double* mod = (double*)(hdr.data() + HB_MOD);
    mod[0] = mod[4] = mod[8] = 1.0;
    std::vector<double> tf((size_t)N * 12), st((size_t)N);
    for (int k = 0; k < N; ++k) {
        liw_lie_make_tf(poses + (size_t)k * 6, poses + (size_t)k * 6 + 3, &tf[(size_t)k * 12]);
        st[k] = stamps ? stamps[k] : (double)k;
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(c, LIW_EHIP, "liw_fpg_load_graph: hipDeviceSynchronize");
    const size_t base = (size_t)robot * L.robot_bytes;
    if (!push(store, base, hdr.data(), 256) || !push(store, base + L.r_stamp, st.data(), (size_t)N) || !push(store, base + L.r_tf, tf.data(), (size_t)N * 12) ||
        !push(store, base + L.r_pose, poses, (size_t)N * 6) || !push(store, base + L.r_seq + 96, seq_tf12, (size_t)(N - 1) * 12) ||
        !push(store, base + L.r_lidx, loop_idx, (size_t)n_loop * 2) || !push(store, base + L.r_ltf, loop_tf12, (size_t)n_loop * 12))
        return fail(c, LIW_EHIP, "liw_fpg_load_graph: hipMemcpy");
    return LIW_OK;
}

}  // extern "C"
