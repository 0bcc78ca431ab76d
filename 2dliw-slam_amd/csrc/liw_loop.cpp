// liw_loop.cpp — host side of the laser loop detector (C ABI include/liw_loop.h; kernels in k_loop.hip).
//
// The host keeps the key frames (tracking pose, corners), builds each sub-map's point set in the reference's serial order
// (spawn_laser_map_feature + the de-duplication of the laser_map_feature constructor, keyframe_manager.cpp:898-980), gates the
// candidates on size and origin distance (match_map, :1125-1137), draws the query rows, and after the device match walks the
// candidates that passed in ascending order through the closed-form ICP and the tf gate (laser_loop_detect, :642-712).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_lie.h"
#include "../../include/liw_loop.h"
#include "k_loop.hpp"
#include "liw_host_common.hpp"

struct liw_ctx;
hipStream_t liw_ctx_stream(liw_ctx* c);
int liw_ctx_device(liw_ctx* c);
bool liw_ctx_has_device(liw_ctx* c);

namespace {

using liw_loop_dev::Cand;
using liw_loop_dev::Geom;
using liw_loop_dev::kDraws;

constexpr double kPi = 3.14159265358979323846;

struct Layout {
    size_t keys, aij, quick, inv, pts, cands, tres, summary, lists, bytes;
};

int check_params(const liw_loop_params* p, int* W, int* nAngle) {
    if (!p || !(p->a_res > 0) || !(p->d_res > 0) || !std::isfinite(p->a_res) || !std::isfinite(p->d_res)) return LIW_EINVAL;
    if (p->submap_count < 1 || p->min_interval < 1 || p->min_match_threshold < 0) return LIW_EINVAL;
    const double na = kPi * 2 / p->a_res + 2, w = (100.0 / p->d_res + 1) / 64 + 1;   // :1054, :23
    if (!(na + 1 <= liw_loop_dev::kMaxBins) || !(w < 513)) return LIW_EINVAL;
    if (nAngle) *nAngle = (int)na;
    if (W) *W = (int)w;
    return LIW_OK;
}

int layout(const liw_loop_params* p, const liw_loop_dims* d, Layout* L) {
    int W = 0;
    if (check_params(p, &W, nullptr)) return LIW_EINVAL;
    if (!d || d->max_keyframes < 1 || d->max_points < 1 || d->max_points > 4096) return LIW_EINVAL;
    const size_t K = (size_t)d->max_keyframes, P = (size_t)d->max_points;
    size_t o = 0;
    L->keys = o; o = al256(o + K * P * P * 4);
    L->aij = o; o = al256(o + K * P * P * 8);
    L->quick = o; o = al256(o + K * P * (size_t)W * 8);
    L->inv = o; o = al256(o + K * 4);
    L->pts = o; o = al256(o + P * 16);
    L->cands = o; o = al256(o + K * sizeof(Cand));
    L->tres = o; o = al256(o + K * kDraws * P * 8);
    L->summary = o; o = al256(o + K * 8 * 4);
    L->lists = o; o = al256(o + K * P * 8);
    L->bytes = o;
    return LIW_OK;
}

struct KF {
    bool laser = false;
    double tf[12];
    std::vector<double> corners;   // [k][3] world frame
    int state = LIW_LOOP_NULL;
    std::vector<double> points;    // [n][3] de-duplicated
    double origin[12];
};

void identity12(double* T) {
    std::memset(T, 0, 12 * sizeof(double));
    T[0] = T[4] = T[8] = 1.0;
}

}  // namespace

struct liw_loop {
    liw_ctx* ctx = nullptr;
    liw_loop_params p{};
    liw_loop_dims dims{};
    Layout L{};
    Geom g{};
    int nAngle = 0;
    bool have_device = false;
    bool store_failed = false;   // a device is there but hipMalloc of the store failed
    char* store = nullptr;
    double Tiw[12];
    std::vector<KF> kfs;
    liw_loop_stats stats{};
    std::string err;

    int fail(int code, const char* what) { err = what; return code; }
    template <class T> T* dev(size_t off) const { return (T*)(store + off); }
};

namespace {

// match_map's gates before any descriptor work (:1128-1135); invalid features are treated as null
int gate(const liw_loop* h, int q, int c) {
    const KF &a = h->kfs[q], &b = h->kfs[c];
    if (a.state != LIW_LOOP_VALID || b.state != LIW_LOOP_VALID) return LIW_LOOP_GATE_NULL;
    const int n1 = (int)a.points.size() / 3, n2 = (int)b.points.size() / 3, thr = h->p.min_match_threshold;
    if (n1 < thr || n2 < thr || n1 == 0 || n2 == 0) return LIW_LOOP_GATE_POINTS;
    double inv[12], rel[12];
    liw_lie_inverse(a.origin, inv);
    liw_lie_mul(inv, b.origin, rel);
    if (std::sqrt(rel[9] * rel[9] + rel[10] * rel[10] + rel[11] * rel[11]) > h->p.max_dis) return LIW_LOOP_GATE_DIS;
    return LIW_LOOP_ACCEPTED;
}

Cand make_cand(const liw_loop* h, int q, int c) {
    Cand x{};
    x.slot = c;
    x.n2 = (int)h->kfs[c].points.size() / 3;
    const int n1 = (int)h->kfs[q].points.size() / 3;
    for (int d = 0; d < kDraws; ++d) {
        const int row = liw_loop_dev::draw_row(h->p.seed, q, c, d, n1);
        bool rep = false;
        for (int e = 0; e < d; ++e) rep |= x.rows[e] == row;
        x.rows[d] = rep ? -1 : row;
    }
    return x;
}

// device match + select of query q against `cands`; summary [ncand][8] to the host
int run_match(liw_loop* h, int q, const std::vector<Cand>& cands, std::vector<int>& summary) {
    hipStream_t s = liw_ctx_stream(h->ctx);
    const int nc = (int)cands.size();
    summary.assign((size_t)nc * 8, 0);
    if (!nc) return 0;
    if (nc > h->dims.max_keyframes) return h->fail(LIW_EINVAL, "liw_loop: too many candidates");
    int max_n2 = 0;
    for (const Cand& c : cands) max_n2 = std::max(max_n2, c.n2);
    const int n1 = (int)h->kfs[q].points.size() / 3;
    (void)hipMemcpyAsync(h->dev<Cand>(h->L.cands), cands.data(), sizeof(Cand) * nc, hipMemcpyHostToDevice, s);
    if (liw_loop_dev::launch_match(h->dev<Cand>(h->L.cands), nc, max_n2, q, n1, h->g, h->dev<uint32_t>(h->L.keys), h->dev<double>(h->L.aij),
                                   h->dev<uint64_t>(h->L.quick), h->dev<int2>(h->L.tres), s) ||
        liw_loop_dev::launch_select(h->dev<Cand>(h->L.cands), nc, q, n1, h->g, h->dev<uint32_t>(h->L.keys), h->dev<double>(h->L.aij),
                                    h->dev<int2>(h->L.tres), h->dev<int>(h->L.summary), h->dev<int>(h->L.lists), s))
        return h->fail(LIW_EHIP, "liw_loop: kernel launch failed");
    (void)hipMemcpyAsync(summary.data(), h->dev<int>(h->L.summary), sizeof(int) * 8 * nc, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return h->fail(LIW_EHIP, "liw_loop: hipStreamSynchronize");
    return 0;
}

int read_lists(liw_loop* h, int ci, int len, std::vector<int>& lists) {
    lists.resize((size_t)len * 2);
    if (hipMemcpy(lists.data(), h->dev<int>(h->L.lists) + (size_t)ci * h->dims.max_points * 2, sizeof(int) * 2 * len, hipMemcpyDeviceToHost) !=
        hipSuccess)
        return h->fail(LIW_EHIP, "liw_loop: hipMemcpy");
    return 0;
}

#define LOOP_NEED_DEVICE(h)                                                                                  \
    do {                                                                                                     \
        if (!(h)) return LIW_EINVAL;                                                                         \
        if ((h)->store_failed) return LIW_ENOMEM;   /* err keeps the hipMalloc message */                  \
        if (!(h)->have_device) return (h)->fail(LIW_ENODEV, "no usable gfx950 device (no CPU fallback)"); \
        (void)hipSetDevice(liw_ctx_device((h)->ctx));                                                        \
    } while (0)

}  // namespace

extern "C" {

int liw_loop_sizes(const liw_loop_params* params, int* quick_words, int* n_angle) { return check_params(params, quick_words, n_angle); }

int liw_loop_store_bytes(const liw_loop_params* params, const liw_loop_dims* dims, size_t* bytes) {
    Layout L{};
    if (!bytes || layout(params, dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

int liw_loop_icp(int n, const double* p1, const double* p2, double* T12) {
    if (n < 1 || !p1 || !p2 || !T12) return LIW_EINVAL;
    double c1x = 0, c1y = 0, c2x = 0, c2y = 0;
    for (int i = 0; i < n; ++i) { c1x += p1[3 * i]; c1y += p1[3 * i + 1]; c2x += p2[3 * i]; c2y += p2[3 * i + 1]; }
    c1x /= n; c1y /= n; c2x /= n; c2y /= n;
    double sdot = 0, scross = 0;   // sum a . b and sum (b x a)_z, a = p1 - c1, b = p2 - c2
    for (int i = 0; i < n; ++i) {
        const double ax = p1[3 * i] - c1x, ay = p1[3 * i + 1] - c1y, bx = p2[3 * i] - c2x, by = p2[3 * i + 1] - c2y;
        sdot += ax * bx + ay * by;
        scross += bx * ay - by * ax;
    }
    const double yaw = std::atan2(scross, sdot), c = std::cos(yaw), s = std::sin(yaw);
    const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    std::memcpy(T12, R, sizeof R);
    T12[9] = c1x - (c * c2x - s * c2y);
    T12[10] = c1y - (s * c2x + c * c2y);
    T12[11] = 0.0;
    return LIW_OK;
}

liw_loop* liw_loop_create(liw_ctx* ctx, const liw_loop_params* params, const liw_loop_dims* dims) {
    Layout L{};
    int W = 0, nAngle = 0;
    if (!ctx || layout(params, dims, &L) || check_params(params, &W, &nAngle)) return nullptr;
    liw_loop* h = new liw_loop();
    h->ctx = ctx;
    h->p = *params;
    h->dims = *dims;
    h->L = L;
    h->nAngle = nAngle;
    h->g.P = dims->max_points;
    h->g.W = W;
    h->g.nb = nAngle + 1;
    h->g.orign = nAngle / 2;
    h->g.thr = params->min_match_threshold;
    h->g.a_res = params->a_res;
    double M[16];
    liw_get_extrinsics(ctx, M, nullptr);
    liw_lie_from_matrix16(M, 0, h->Tiw);
    if (liw_ctx_has_device(ctx)) {
        (void)hipSetDevice(liw_ctx_device(ctx));
        if (hipMalloc((void**)&h->store, L.bytes) == hipSuccess) h->have_device = true;
        else {
            h->store = nullptr;
            h->store_failed = true;
            h->err = "liw_loop_create: hipMalloc of the " + std::to_string(L.bytes) + "-byte store failed (max_keyframes x max_points too large)";
        }
    } else {
        h->err = "no usable gfx950 device (no CPU fallback)";
    }
    return h;
}

void liw_loop_destroy(liw_loop* h) {
    if (!h) return;
    if (h->store) (void)hipFree(h->store);
    delete h;
}

const char* liw_loop_last_error(liw_loop* h) { return h ? h->err.c_str() : "null handle"; }
int liw_loop_num_keyframes(liw_loop* h) { return h ? (int)h->kfs.size() : LIW_EINVAL; }

int liw_loop_add_keyframe(liw_loop* h, int is_laser, const double* tf12, int n_corners, const double* corners) {
    LOOP_NEED_DEVICE(h);
    if (!tf12 || n_corners < 0 || (n_corners > 0 && !corners)) return h->fail(LIW_EINVAL, "liw_loop_add_keyframe: bad argument");
    if ((int)h->kfs.size() >= h->dims.max_keyframes) return h->fail(LIW_ENOMEM, "liw_loop_add_keyframe: max_keyframes key frames held");
    const int slot = (int)h->kfs.size();
    h->kfs.emplace_back();
    KF& f = h->kfs.back();
    f.laser = is_laser != 0;
    std::memcpy(f.tf, tf12, sizeof f.tf);
    identity12(f.origin);
    if (!f.laser) return slot;
    f.corners.assign(corners, corners + (size_t)n_corners * 3);
    // spawn_laser_map_feature (:898-929): newest first, origin = the newest laser key frame's pose unless submap_count == 1
    std::vector<const std::vector<double>*> concers;
    int count = 0, index = -1;
    for (int i = slot; i > -1; --i) {
        if (!h->kfs[i].laser) continue;
        ++count;
        concers.push_back(&h->kfs[i].corners);
        if (count == h->p.submap_count) break;
        if (index == -1) { index = i; std::memcpy(f.origin, h->kfs[i].tf, sizeof f.origin); }
    }
    // de-duplication (:955-980), serial
    const double dr = h->p.d_res;
    std::vector<double>& pts = f.points;
    for (const std::vector<double>* cs : concers) {
        for (size_t j = 0; j + 2 < cs->size(); j += 3) {
            const double* c = cs->data() + j;
            bool dup = false;
            for (size_t k = 0; k < pts.size(); k += 3) {
                const double dx = c[0] - pts[k], dy = c[1] - pts[k + 1];
                const double nrm = std::sqrt(dx * dx + dy * dy);
                if (nrm < dr / 2)
                    for (int e = 0; e < 3; ++e) pts[k + e] = (pts[k + e] * 3 + c[e]) / 4;
                if (nrm < dr * 5) { dup = true; break; }
            }
            if (!dup) pts.insert(pts.end(), c, c + 3);
        }
    }
    const int n = (int)pts.size() / 3;
    if (n > h->dims.max_points) { f.state = LIW_LOOP_OVER_CAP; return slot; }
    std::vector<double> xy((size_t)n * 2);
    for (int i = 0; i < n; ++i) { xy[2 * i] = pts[3 * i]; xy[2 * i + 1] = pts[3 * i + 1]; }
    hipStream_t s = liw_ctx_stream(h->ctx);
    int bad = 0;
    (void)hipMemcpyAsync(h->dev<double>(h->L.pts), xy.data(), sizeof(double) * xy.size(), hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(h->dev<int>(h->L.inv) + slot, 0, sizeof(int), s);
    if (liw_loop_dev::launch_describe(h->dev<double>(h->L.pts), n, slot, h->g, dr, h->dev<uint32_t>(h->L.keys), h->dev<double>(h->L.aij),
                                      h->dev<uint64_t>(h->L.quick), h->dev<int>(h->L.inv), s))
        return h->fail(LIW_EHIP, "liw_loop_add_keyframe: kernel launch failed");
    (void)hipMemcpyAsync(&bad, h->dev<int>(h->L.inv) + slot, sizeof(int), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return h->fail(LIW_EHIP, "liw_loop_add_keyframe: hipStreamSynchronize");
    f.state = bad ? LIW_LOOP_DIJ_OVERFLOW : LIW_LOOP_VALID;
    return slot;
}

int liw_loop_detect(liw_loop* h, liw_loop_edge* out) {
    LOOP_NEED_DEVICE(h);
    h->stats = liw_loop_stats{};
    const int K = (int)h->kfs.size();
    if (K < h->p.min_interval) return 0;
    const int q = K - 1;
    if (h->kfs[q].state != LIW_LOOP_VALID) return 0;
    const int step = h->p.submap_count / 3 + 1;
    std::vector<Cand> cands;
    for (int i = 0; i < K - h->p.min_interval; i += step) {   // :651
        ++h->stats.candidates;
        if (gate(h, q, i) == LIW_LOOP_ACCEPTED) cands.push_back(make_cand(h, q, i));
    }
    h->stats.launched = (int)cands.size();
    for (const Cand& c : cands)
        for (int d = 0; d < kDraws; ++d) h->stats.tasks += c.rows[d] >= 0 ? c.n2 : 0;
    std::vector<int> sm, lists;
    if (int r = run_match(h, q, cands, sm)) return r;
    const KF& f1 = h->kfs[q];
    double A1[12], inv1[12], inv_iw[12];
    liw_lie_mul(f1.tf, h->Tiw, A1);
    liw_lie_inverse(A1, inv1);
    liw_lie_inverse(h->Tiw, inv_iw);
    for (size_t ci = 0; ci < cands.size(); ++ci) {
        h->stats.quick_pass += sm[ci * 8 + 4];
        if (sm[ci * 8] > h->p.min_match_threshold) ++h->stats.accepted;
    }
    for (size_t ci = 0; ci < cands.size(); ++ci) {
        const int size = sm[ci * 8], len = sm[ci * 8 + 5];
        if (size <= h->p.min_match_threshold) continue;
        if (len != size) return h->fail(LIW_ESTATE, "liw_loop_detect: correspondence list does not match the bin size");
        if (int r = read_lists(h, (int)ci, len, lists)) return r;
        ++h->stats.icp_checked;
        const KF& f2 = h->kfs[cands[ci].slot];
        double A2[12], inv2[12];
        liw_lie_mul(f2.tf, h->Tiw, A2);
        liw_lie_inverse(A2, inv2);
        std::vector<double> P1((size_t)len * 3), P2((size_t)len * 3);
        for (int k = 0; k < len; ++k) {
            liw_lie_apply(inv1, &f1.points[(size_t)lists[2 * k] * 3], &P1[(size_t)k * 3]);
            liw_lie_apply(inv2, &f2.points[(size_t)lists[2 * k + 1] * 3], &P2[(size_t)k * 3]);
            P1[(size_t)k * 3 + 2] = 0.0;
            P2[(size_t)k * 3 + 2] = 0.0;
        }
        double wT12[12], tmp[12], it12[12], inv_f1[12], track[12], inv_it[12], errT[12], dp[3], dq[3];
        liw_loop_icp(len, P1.data(), P2.data(), wT12);
        liw_lie_mul(h->Tiw, wT12, tmp);
        liw_lie_mul(tmp, inv_iw, it12);
        liw_lie_inverse(f1.tf, inv_f1);
        liw_lie_mul(inv_f1, f2.tf, track);
        liw_lie_inverse(it12, inv_it);
        liw_lie_mul(inv_it, track, errT);
        liw_lie_log_SE3(errT, dp, dq);
        if (std::sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]) > h->p.max_tf_p ||
            std::sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2]) > h->p.max_tf_q)
            continue;
        if (out) {
            out->index1 = q;
            out->index2 = cands[ci].slot;
            out->size = size;
            std::memcpy(out->tf12, it12, sizeof it12);
        }
        return 1;
    }
    return 0;
}

int liw_loop_last_stats(liw_loop* h, liw_loop_stats* out) {
    if (!h || !out) return LIW_EINVAL;
    *out = h->stats;
    return LIW_OK;
}

int liw_loop_match(liw_loop* h, int query, int candidate, int cap, int* p1_idx, int* p2_idx, liw_loop_match_info* info) {
    LOOP_NEED_DEVICE(h);
    const int K = (int)h->kfs.size();
    if (query < 0 || query >= K || candidate < 0 || candidate >= K || cap < 0 || (cap > 0 && (!p1_idx || !p2_idx)))
        return h->fail(LIW_EINVAL, "liw_loop_match: bad argument");
    liw_loop_match_info mi{0, -1, -1, -1, -1, 0, 0, 0};
    mi.gate = gate(h, query, candidate);
    int written = 0;
    if (mi.gate == LIW_LOOP_ACCEPTED) {
        std::vector<Cand> cands{make_cand(h, query, candidate)};
        std::vector<int> sm, lists;
        if (int r = run_match(h, query, cands, sm)) return r;
        for (int d = 0; d < kDraws; ++d) mi.tasks += cands[0].rows[d] >= 0 ? cands[0].n2 : 0;
        mi.size = sm[0];
        mi.draw = sm[1];
        mi.row = sm[2];
        mi.bin = sm[3];
        mi.quick_pass = sm[4];
        mi.query_row = mi.draw >= 0 ? cands[0].rows[mi.draw] : -1;
        if (mi.size <= h->p.min_match_threshold) mi.gate = LIW_LOOP_GATE_SIZE;
        else {
            const int len = sm[5];
            if (len != mi.size) return h->fail(LIW_ESTATE, "liw_loop_match: correspondence list does not match the bin size");
            if (int r = read_lists(h, 0, len, lists)) return r;
            written = std::min(len, cap);
            for (int k = 0; k < written; ++k) { p1_idx[k] = lists[2 * k]; p2_idx[k] = lists[2 * k + 1]; }
        }
    }
    if (info) *info = mi;
    return written;
}

int liw_loop_get_points(liw_loop* h, int k, int cap, double* points) {
    if (!h || k < 0 || k >= (int)h->kfs.size() || cap < 0 || (cap > 0 && !points)) return LIW_EINVAL;
    const std::vector<double>& p = h->kfs[k].points;
    const int n = (int)p.size() / 3;
    std::memcpy(points, p.data(), sizeof(double) * 3 * (size_t)std::min(n, cap));
    return n;
}

int liw_loop_get_row(liw_loop* h, int k, int i, int cap, int* dij, int* j, double* aij, unsigned long long* quick_des) {
    LOOP_NEED_DEVICE(h);
    if (k < 0 || k >= (int)h->kfs.size() || h->kfs[k].state != LIW_LOOP_VALID) return h->fail(LIW_EINVAL, "liw_loop_get_row: no descriptors");
    const int n = (int)h->kfs[k].points.size() / 3;
    if (i < 0 || i >= n || cap < 0) return h->fail(LIW_EINVAL, "liw_loop_get_row: bad argument");
    const int m = std::min(n - 1, cap);
    const size_t row = (size_t)k * h->g.P + i;
    std::vector<uint32_t> kv((size_t)std::max(m, 1));
    std::vector<double> av((size_t)std::max(m, 1));
    std::vector<unsigned long long> qv((size_t)h->g.W);
    if (m > 0) {
        (void)hipMemcpy(kv.data(), h->dev<uint32_t>(h->L.keys) + row * h->g.P, sizeof(uint32_t) * m, hipMemcpyDeviceToHost);
        (void)hipMemcpy(av.data(), h->dev<double>(h->L.aij) + row * h->g.P, sizeof(double) * m, hipMemcpyDeviceToHost);
    }
    if (hipMemcpy(qv.data(), h->dev<uint64_t>(h->L.quick) + row * h->g.W, sizeof(uint64_t) * h->g.W, hipMemcpyDeviceToHost) != hipSuccess)
        return h->fail(LIW_EHIP, "liw_loop_get_row: hipMemcpy");
    for (int e = 0; e < m; ++e) {
        if (dij) dij[e] = (int)(kv[e] >> 12);
        if (j) j[e] = (int)(kv[e] & 0xFFFu);
        if (aij) aij[e] = av[e];
    }
    if (quick_des) std::memcpy(quick_des, qv.data(), sizeof(uint64_t) * h->g.W);
    return n - 1;
}

int liw_loop_status(liw_loop* h, int k, int* n_points, double* origin12) {
    if (!h || k < 0 || k >= (int)h->kfs.size()) return LIW_EINVAL;
    const KF& f = h->kfs[k];
    if (n_points) *n_points = (int)f.points.size() / 3;
    if (origin12) std::memcpy(origin12, f.origin, sizeof f.origin);
    return f.state;
}

}  // extern "C"
