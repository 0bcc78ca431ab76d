// liw_loop_batch.cpp — host side of the fleet loop detector (C ABI include/liw_loop_batch.h; kernels in k_loop_batch.hip): the store
// layout, argument checks, the launches and the synchronous getters.  No per-robot work happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_lie.h"
#include "../../include/liw_loop_batch.h"
#include "k_loop_batch.hpp"
#include "liw_host_common.hpp"
#include "liw_loop_batch_ctx.hpp"

namespace {

using liw_floop_dev::Lay;
using liw_floop_dev::Prm;

bool make_lay(const liw_loop_params* p, const liw_floop_dims* d, Lay* L, int* nAngle) {
    int W = 0, na = 0;
    if (liw_loop_sizes(p, &W, &na)) return false;
    if (!d || d->B < 1 || d->max_keyframes < 1 || d->max_points < 1 || d->max_points > 1024 || d->max_kf_corners < 1) return false;
    if (nAngle) *nAngle = na;
    L->B = d->B; L->K = d->max_keyframes; L->P = d->max_points; L->C = d->max_kf_corners; L->S = p->submap_count; L->W = W;
    L->step = p->submap_count / 3 + 1;
    L->NC = (L->K + L->step - 1) / L->step;
    L->NS = L->NC + 1;
    const size_t K = (size_t)L->K, P = (size_t)L->P, C = (size_t)L->C, S = (size_t)L->S, NS = (size_t)L->NS, NC = (size_t)L->NC, B = (size_t)L->B;
    size_t o = 256;
    L->r_tf = o; o = al256(o + K * 96);
    L->r_state = o; o = al256(o + K * 4);
    L->r_npts = o; o = al256(o + K * 4);
    L->r_ringn = o; o = al256(o + S * 4);
    L->r_ring = o; o = al256(o + S * C * 24);
    L->r_pts = o; o = al256(o + NS * P * 24);
    L->r_keys = o; o = al256(o + NS * P * P * 4);
    L->r_aij = o; o = al256(o + NS * P * P * 8);
    L->r_quick = o; o = al256(o + NS * P * (size_t)W * 8);
    L->robot_bytes = o;
    L->feature_bytes = P * 24 + P * P * 12 + P * (size_t)W * 8;
    o = B * L->robot_bytes;
    L->f_hdr = o; o += 256;
    L->f_work = o; o = al256(o + B * 4);
    L->f_cnt = o; o = al256(o + B * 4);
    L->f_base = o; o = al256(o + B * 4);
    L->f_cmax = o; o = al256(o + B * 4);
    L->f_pre = o; o = al256(o + B * NC * sizeof(liw_floop_dev::Pre));
    L->f_pairs = o; o = al256(o + B * NC * sizeof(liw_floop_dev::Pair));
    L->f_tres = o; o = al256(o + B * NC * liw_floop_dev::kDraws * P * 8);
    L->f_summary = o; o = al256(o + B * NC * 32);
    L->f_lists = o; o = al256(o + B * NC * P * 8);
    L->f_res = o; o = al256(o + B * NC * sizeof(liw_floop_dev::Res));
    L->bytes = o;
    return true;
}

}  // namespace

namespace {

// header {K, full} of a robot; < 0 on error
int robot_header(liw_floop_ctx* c, const void* store, int robot, int* hdr) {
    if (bad_store(store) || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_floop: store or robot");
    if (!pull(store, (size_t)robot * c->L.robot_bytes, hdr, 2)) return fail(c, LIW_EHIP, "liw_floop: hipMemcpy");
    return 0;
}

}  // namespace

extern "C" {

int liw_floop_layout(const liw_loop_params* params, const liw_floop_dims* dims, liw_floop_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(params, dims, &L, nullptr)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->robot_bytes = L.robot_bytes;
    out->scratch_off = L.f_hdr;
    out->scratch_bytes = L.bytes - L.f_hdr;
    out->feature_bytes = L.feature_bytes;
    out->feature_slots = L.NS;
    out->stride = L.step;
    out->quick_words = L.W;
    return LIW_OK;
}

int liw_floop_store_bytes(const liw_loop_params* params, const liw_floop_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(params, dims, &L, nullptr)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_floop_ctx* liw_floop_create(const liw_loop_params* params, const liw_floop_dims* dims, const double* T_imu_to_wheel16, int normalize_extrinsics,
                                int device) {
    Lay L{};
    int nAngle = 0;
    if (!T_imu_to_wheel16 || !make_lay(params, dims, &L, &nAngle)) return nullptr;
    liw_floop_ctx* c = new liw_floop_ctx();
    c->L = L;
    c->device = device;
    Prm& P = c->P;
    P.g.P = L.P; P.g.W = L.W; P.g.nb = nAngle + 1; P.g.orign = nAngle / 2; P.g.thr = params->min_match_threshold; P.g.a_res = params->a_res;
    P.d_res = params->d_res; P.max_dis = params->max_dis; P.max_tf_p = params->max_tf_p; P.max_tf_q = params->max_tf_q;
    P.min_interval = params->min_interval;
    P.seed = params->seed;
    liw_lie_from_matrix16(T_imu_to_wheel16, normalize_extrinsics, P.Tiw);
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_floop_destroy(liw_floop_ctx* c) { delete c; }
const char* liw_floop_last_error(liw_floop_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_floop_reset(liw_floop_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store)) return fail(c, LIW_EINVAL, "liw_floop_reset: store");
    if (liw_floop_dev::launch_reset((char*)store, c->L, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_floop_reset: kernel launch failed");
    return LIW_OK;
}

int liw_floop_add_keyframes(liw_floop_ctx* c, void* store, const unsigned char* key, const double* pose, const double* corners, int corner_stride,
                            const int* n_corners, const unsigned char* mask, unsigned char* added, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !key || !pose || !corners || !n_corners || corner_stride < 1)
        return fail(c, LIW_EINVAL, "liw_floop_add_keyframes: bad argument");
    if (liw_floop_dev::launch_add((char*)store, c->L, c->P, key, pose, corners, corner_stride, n_corners, mask, added, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_floop_add_keyframes: kernel launch failed");
    return LIW_OK;
}

int liw_floop_detect(liw_floop_ctx* c, void* store, const unsigned char* key, const unsigned char* mask, unsigned char* found, int* edge, double* tf12,
                     long long* stats, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !key || !found || !edge || !tf12 || !stats) return fail(c, LIW_EINVAL, "liw_floop_detect: bad argument");
    if (liw_floop_dev::launch_detect((char*)store, c->L, c->P, key, mask, found, edge, tf12, stats, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_floop_detect: kernel launch failed");
    return LIW_OK;
}

int liw_floop_num_keyframes(liw_floop_ctx* c, const void* store, int robot) {
    LIW_FLEET_DEV(c);
    int hdr[2];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    return hdr[0];
}

int liw_floop_full(liw_floop_ctx* c, const void* store, int robot) {
    LIW_FLEET_DEV(c);
    int hdr[2];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    return hdr[1] != 0;
}

int liw_floop_status(liw_floop_ctx* c, const void* store, int robot, int k, int* n_points, double* origin12, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[2];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (k < 0 || k >= hdr[0]) return fail(c, LIW_EINVAL, "liw_floop_status: no such key frame");
    const size_t base = (size_t)robot * c->L.robot_bytes;
    int state = 0, n = 0;
    double tf[12];
    if (!pull(store, base + c->L.r_state + (size_t)k * 4, &state, 1) || !pull(store, base + c->L.r_npts + (size_t)k * 4, &n, 1) ||
        !pull(store, base + c->L.r_tf + (size_t)k * 96, tf, 12))
        return fail(c, LIW_EHIP, "liw_floop_status: hipMemcpy");
    if (n_points) *n_points = n;
    if (tf12) std::memcpy(tf12, tf, sizeof tf);
    if (origin12) {   // the sub-map's origin is the key frame's own pose, identity when submap_count == 1
        if (c->L.S > 1) std::memcpy(origin12, tf, sizeof tf);
        else { std::memset(origin12, 0, 12 * sizeof(double)); origin12[0] = origin12[4] = origin12[8] = 1.0; }
    }
    return state;
}

// feature slot of key frame k of a robot with K key frames, -1 if its feature is not held
static int held_slot(const Lay& L, int k, int K) {
    if (k < 0 || k >= K) return -1;
    const int fs = liw_floop_dev::feature_slot(L, k);
    return fs < L.NC || k == K - 1 ? fs : -1;
}

int liw_floop_get_points(liw_floop_ctx* c, const void* store, int robot, int k, int cap, double* points) {
    LIW_FLEET_DEV(c);
    int hdr[2];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    const int fs = held_slot(c->L, k, hdr[0]);
    if (fs < 0 || cap < 0 || (cap > 0 && !points)) return fail(c, LIW_EINVAL, "liw_floop_get_points: feature not held or bad argument");
    int n = 0;
    const int st = liw_floop_status(c, store, robot, k, &n, nullptr, nullptr);
    if (st < 0) return st;
    if (st != LIW_LOOP_VALID && st != LIW_LOOP_DIJ_OVERFLOW) return fail(c, LIW_EINVAL, "liw_floop_get_points: no points");
    const int m = std::min(n, cap);
    if (!pull(store, (size_t)robot * c->L.robot_bytes + c->L.r_pts + (size_t)fs * c->L.P * 24, points, (size_t)m * 3))
        return fail(c, LIW_EHIP, "liw_floop_get_points: hipMemcpy");
    return n;
}

int liw_floop_get_row(liw_floop_ctx* c, const void* store, int robot, int k, int i, int cap, int* dij, int* j, double* aij, unsigned long long* quick_des) {
    LIW_FLEET_DEV(c);
    int hdr[2];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    const Lay& L = c->L;
    const int fs = held_slot(L, k, hdr[0]);
    if (fs < 0) return fail(c, LIW_EINVAL, "liw_floop_get_row: feature not held");
    int n = 0;
    const int st = liw_floop_status(c, store, robot, k, &n, nullptr, nullptr);
    if (st < 0) return st;
    if (st != LIW_LOOP_VALID || i < 0 || i >= n || cap < 0) return fail(c, LIW_EINVAL, "liw_floop_get_row: no descriptors or bad argument");
    const int m = std::min(n - 1, cap);
    const size_t base = (size_t)robot * L.robot_bytes, row = (size_t)fs * L.P + i;
    std::vector<uint32_t> kv((size_t)std::max(m, 1));
    std::vector<double> av((size_t)std::max(m, 1));
    std::vector<unsigned long long> qv((size_t)L.W);
    if (!pull(store, base + L.r_keys + row * L.P * 4, kv.data(), m) || !pull(store, base + L.r_aij + row * L.P * 8, av.data(), m))
        return fail(c, LIW_EHIP, "liw_floop_get_row: hipMemcpy");
    if (!pull(store, base + L.r_quick + row * L.W * 8, qv.data(), L.W)) return fail(c, LIW_EHIP, "liw_floop_get_row: hipMemcpy");
    for (int e = 0; e < m; ++e) {
        if (dij) dij[e] = (int)(kv[e] >> 12);
        if (j) j[e] = (int)(kv[e] & 0xFFFu);
        if (aij) aij[e] = av[e];
    }
    if (quick_des) std::memcpy(quick_des, qv.data(), sizeof(unsigned long long) * L.W);
    return n - 1;
}

}  // extern "C"
