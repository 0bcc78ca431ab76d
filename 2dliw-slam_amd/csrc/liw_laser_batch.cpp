// liw_laser_batch.cpp — host side of the fleet laser front-end (C ABI include/liw_laser_batch.h; kernels in k_lfe_lines.hip,
// k_lfe_match.hip and k_lfe_state.hip): the store layout, argument checks, the lane / wave dispatch with its LDS limits, the launches
// and the synchronous getters.  No per-robot work happens here.
#pragma clang fp contract(off)   // liw_lfe_set_geometry reproduces the float arithmetic of the x86-64 host build of liw_laser.cpp

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_laser_batch.h"
#include "k_lfe.hpp"
#include "liw_host_common.hpp"

void liw_normalize_rotation_host(double* R9);   // liw_capi.hip (params.cpp:44-54 round trip)

using namespace lfe;

struct liw_lfe_ctx : liw_fleet_ctx_base {
    liw_laser_params prm;
    Lay L;
    DP P;
    float2* d_cs = nullptr;
    int* d_rows = nullptr;   // B ints between the two launches of liw_lfe_init_begin
    int n_rays = 0;
    float tinc = 0.0f;
    int add_path = -1;   // the kernel of the last add_scan / rebuild: 0 lane, 1 wave (liw_lfe_add_scan_path)
};

namespace {

bool make_lay(const liw_lfe_dims* d, Lay& L) {
    if (!d || d->B <= 0 || d->slots <= 0 || d->max_points <= 0 || d->max_lines <= 0 || d->max_cell_entries <= 0) return false;
    L.B = d->B; L.slots = d->slots; L.max_points = d->max_points; L.max_lines = d->max_lines; L.max_entries = d->max_cell_entries;
    L.slot_bytes = al256(kHdrBytes + 80 * (size_t)d->max_lines + 8 * (size_t)d->max_cell_entries);
    L.robot_bytes = kMgrBytes + (size_t)(d->slots + 2) * L.slot_bytes;
    return true;
}
// the three liw_lfe_*_layout entries: B records of per_robot bytes (0: the store's robot_bytes)
int layout(const liw_lfe_dims* dims, size_t per_robot, size_t* bytes) {
    Lay L;
    if (!bytes || !make_lay(dims, L)) return LIW_EINVAL;
    *bytes = (size_t)dims->B * (per_robot ? per_robot : L.robot_bytes);
    return LIW_OK;
}

// the result of a launch_*: the HIP error's text goes to the handle
int launched(liw_lfe_ctx* c, int r) { return r == LIW_OK ? LIW_OK : fail(c, r, hipGetErrorString(hipGetLastError())); }

// LIW_LFE_SPAWN / LIW_LFE_ADD_SCAN, read per call: "lane" asks for the lane kernel, "wave", nothing or an empty value for the
// default, anything else is an error
int lane_requested(liw_lfe_ctx* c, const char* name, bool* lane) {
    const char* env = std::getenv(name);
    *lane = false;
    if (env && *env) {
        if (!std::strcmp(env, "lane")) *lane = true;
        else if (std::strcmp(env, "wave")) return fail(c, LIW_EINVAL, (std::string(name) + " must be lane or wave").c_str());
    }
    return LIW_OK;
}
// liw_lfe_spawn / liw_lfe_spawn_corners: the wave-per-scan kernel unless LIW_LFE_SPAWN=lane asks for the lane-per-scan kernel, or
// the dimensions need more LDS than a work-group has (then the lane kernel; it knows no corners)
int spawn_launch(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, int max_corners, double* corners,
                 int* n_corners, void* stream) {
    bool lane;
    if (int r = lane_requested(c, "LIW_LFE_SPAWN", &lane)) return r;
    const WaveLds O = wave_lds(c->L);
    if (corners && lane) return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: the lane kernel (LIW_LFE_SPAWN=lane) does not compute corners");
    if (corners && O.total > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: max_points / max_lines need more than 64 KiB of LDS");
    if (lane || O.total > kWaveLdsMax) return launched(c, launch_spawn(store, c->L, c->P, slot, pts, n_pts, times, (hipStream_t)stream));
    return launched(c, launch_spawn_wave(store, c->L, c->P, O, slot, pts, n_pts, times, max_corners, corners, n_corners, (hipStream_t)stream));
}
// liw_lfe_add_scan(_flags) (F = 1, reset = false) and liw_lfe_rebuild: the wave-per-robot kernel in one launch unless
// LIW_LFE_ADD_SCAN=lane asks for the lane-per-robot kernel, or the dimensions need more LDS than a work-group has
int add_scan_launch(liw_lfe_ctx* c, void* store, int first_slot, int F, bool reset, const double* poses, long long robot_stride, long long frame_stride,
                    const unsigned char* mask, unsigned char* flags, void* stream) {
    bool lane;
    if (int r = lane_requested(c, "LIW_LFE_ADD_SCAN", &lane)) return r;
    const AddLds O = add_lds(c->L);
    hipStream_t s = (hipStream_t)stream;
    if (!lane && O.total <= kWaveLdsMax) {
        c->add_path = 1;
        return launched(c, launch_add_scan_wave(store, c->L, c->P, O, first_slot, F, reset ? 1 : 0, poses, robot_stride, frame_stride, mask, flags, s));
    }
    c->add_path = 0;
    int r = reset ? launch_reset_mgr(store, c->L, mask, s) : LIW_OK;
    for (int k = 0; k < F; ++k) {
        const int rk = launch_add_scan(store, c->L, c->P, first_slot + k, poses + (long long)k * frame_stride, robot_stride, mask, flags, s);
        if (r == LIW_OK) r = rk;
    }
    return launched(c, r);
}
// the first half of the three pack entries (`who` names the entry in the messages): laser_off [R + 1] = the offset scan of R windows
// of F counts (sel may be null), then Ltot = laser_off[R] read back on the stream.  -> Ltot, or < 0 (LIW_ENOMEM past L_cap)
int scan_offsets(liw_lfe_ctx* c, const char* who, int R, int F, int cap, const int* count, const int* sel, int L_cap, int* laser_off, hipStream_t s) {
    if (int r = launched(c, launch_scan_init(R, F, cap, count, sel, laser_off, s))) return r;
    int Ltot = 0;
    if (hipMemcpyAsync(&Ltot, laser_off + R, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(c, LIW_EHIP, (std::string(who) + ": read-back of Ltot").c_str());
    if (Ltot > L_cap) return fail(c, LIW_ENOMEM, (std::string(who) + ": Ltot exceeds L_cap").c_str());
    return Ltot;
}

// head of the synchronous store getters; a bad argument returns LIW_EINVAL and leaves the handle's message alone
int getter_head(liw_lfe_ctx* c, const void* store, int robot, bool slot_ok) {
    if (!c || !store || robot < 0 || robot >= c->L.B || !slot_ok) return LIW_EINVAL;
    LIW_FLEET_DEV(c);
    return LIW_OK;
}
// a robot's manager record on the host; sub = which of its two sub-maps LIW_LFE_REF / LIW_LFE_SPAWNING names, -1 when the robot has
// none such (or `slot` is neither selector)
int host_mgr(liw_lfe_ctx* c, const void* store, int robot, int slot, Mgr& m, int& sub) {
    if (!pull(store, (size_t)robot * c->L.robot_bytes, &m, 1)) return fail(c, LIW_EHIP, "hipMemcpy");
    const int rs = m.ref_sub & 1;
    sub = slot == LIW_LFE_REF ? (m.has_ref ? rs : -1) : (slot == LIW_LFE_SPAWNING && m.has_spawn ? 1 - rs : -1);
    return LIW_OK;
}
// host copy of a slot's header, and its physical slot, of robot / selector; 1 when a sub-map does not exist
int host_slot(liw_lfe_ctx* c, const void* store, int robot, int slot, SlotHdr& h, int& phys) {
    if (int r = getter_head(c, store, robot, slot >= LIW_LFE_SPAWNING && (!c || slot < c->L.slots))) return r;
    phys = slot;
    if (slot < 0) {
        Mgr m;
        int sub;
        if (int r = host_mgr(c, store, robot, slot, m, sub)) return r;
        if (sub < 0) return 1;
        phys = c->L.slots + sub;
    }
    if (!pull(store, (size_t)robot * c->L.robot_bytes + slot_off(c->L, phys), &h, 1)) return fail(c, LIW_EHIP, "hipMemcpy");
    return 0;
}

TP track_tp(const liw_lfe_track_params* tp) {   // the extrinsic as liw_lie_from_matrix16 loads it
    TP t;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) t.Tiw_R[i * 3 + j] = tp->T_imu_to_wheel[i * 4 + j]; t.Tiw_t[i] = tp->T_imu_to_wheel[i * 4 + 3]; }
    if (tp->normalize_extrinsics) liw_normalize_rotation_host(t.Tiw_R);
    t.min_dt = tp->min_delta_t; t.p_thr = tp->key_frame_p_motion_threshold; t.q_thr = tp->key_frame_q_motion_threshold;
    return t;
}
IP init_ip(const liw_lfe_track_params* tp, const liw_lfe_init_params* ip) {
    const TP t = track_tp(tp);
    IP p;
    for (int k = 0; k < 9; ++k) p.Tiw_R[k] = t.Tiw_R[k];
    for (int k = 0; k < 3; ++k) p.Tiw_t[k] = t.Tiw_t[k];
    p.N = ip ? ip->slide_window_size : 0;
    p.p_thr = ip ? ip->p_motion_threshold : 0.0;
    p.q_thr = ip ? ip->q_motion_threshold : 0.0;
    return p;
}

}  // namespace

extern "C" {

int liw_lfe_store_layout(const liw_lfe_dims* dims, size_t* bytes) { return layout(dims, 0, bytes); }
int liw_lfe_track_layout(const liw_lfe_dims* dims, size_t* bytes) { return layout(dims, kTrkBytes, bytes); }
int liw_lfe_init_layout(const liw_lfe_dims* dims, size_t* bytes) { return layout(dims, kIniBytes, bytes); }

liw_lfe_ctx* liw_lfe_create(const liw_laser_params* prm, const liw_lfe_dims* dims, int device) {
    Lay L;
    if (!prm || !make_lay(dims, L) || !(prm->laser_resolution > 0)) return nullptr;
    liw_lfe_ctx* c = new liw_lfe_ctx();
    c->prm = *prm;
    c->L = L;
    c->device = device;
    DP& P = c->P;
    P.res = prm->laser_resolution; P.cont_thr = prm->line_continuous_threshold; P.min_len = prm->line_min_len; P.max_dis = prm->line_max_dis;
    P.tol = prm->line_max_tolerance_angle / 180.0 * kPi;   // deg2rad as liw_laser.cpp
    P.mf_p = prm->ref_motion_filter_p; P.mf_q = prm->ref_motion_filter_q; P.n_acc = prm->ref_n_accumulation;
    P.w = (int)(prm->w_laser_each_scan / prm->laser_resolution + 1);   // laser_manager ctor (:229-241)
    P.h = (int)(prm->h_laser_each_scan / prm->laser_resolution + 1);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.Til_R[i * 3 + j] = prm->T_imu_to_laser[i * 4 + j]; P.Til_t[i] = prm->T_imu_to_laser[i * 4 + 3]; }
    if (prm->normalize_extrinsics) liw_normalize_rotation_host(P.Til_R);
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_lfe_destroy(liw_lfe_ctx* c) {
    if (!c) return;
    if (c->d_cs) { (void)hipSetDevice(c->device); (void)hipFree(c->d_cs); }
    if (c->d_rows) { (void)hipSetDevice(c->device); (void)hipFree(c->d_rows); }
    delete c;
}

const char* liw_lfe_last_error(liw_lfe_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_lfe_set_geometry(liw_lfe_ctx* c, int n_rays, float angle_min, float angle_increment, float time_increment) {
    LIW_FLEET_DEV(c);
    if (n_rays <= 0 || !(angle_increment > 0)) return fail(c, LIW_EINVAL, "liw_lfe_set_geometry: n_rays > 0 and angle_increment > 0");
    // exactly the float arithmetic of liw_laser_to_points (common.cpp:22-24): float angle, cosf / sinf of the host libm
    std::vector<float2> cs(n_rays);
    for (int i = 0; i < n_rays; ++i) {
        const volatile float prod = (float)(size_t)i * angle_increment;
        const float ang = angle_min + prod;
        cs[i].x = std::cos(ang);
        cs[i].y = std::sin(ang);
    }
    if (c->d_cs) { (void)hipFree(c->d_cs); c->d_cs = nullptr; }
    if (hipMalloc(&c->d_cs, sizeof(float2) * n_rays) != hipSuccess) return fail(c, LIW_ENOMEM, "hipMalloc");
    if (hipMemcpy(c->d_cs, cs.data(), sizeof(float2) * n_rays, hipMemcpyHostToDevice) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    c->n_rays = n_rays;
    c->tinc = time_increment;
    return LIW_OK;
}

int liw_lfe_store_reset(liw_lfe_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store) return fail(c, LIW_EINVAL, "liw_lfe_store_reset: store");
    return launched(c, launch_reset(store, c->L, mask, (hipStream_t)stream));
}

int liw_lfe_ranges_to_points(liw_lfe_ctx* c, void* store, const float* ranges, const double* stamps, double* pts, double* times, int* n_pts, void* stream) {
    LIW_FLEET_DEV(c);
    if (!c->d_cs) return fail(c, LIW_ESTATE, "liw_lfe_ranges_to_points: no geometry (liw_lfe_set_geometry)");
    if (!ranges || !stamps || !pts || !times || !n_pts) return fail(c, LIW_EINVAL, "liw_lfe_ranges_to_points: null array");
    return launched(c, launch_ranges(store, c->L, ranges, c->n_rays, c->d_cs, c->tinc, stamps, pts, times, n_pts, (hipStream_t)stream));
}

int liw_lfe_deskew(liw_lfe_ctx* c, double* pts, const double* times, const int* n_pts, const double* stamps, const double* linear, const double* angular,
                   void* stream) {
    LIW_FLEET_DEV(c);
    if (!pts || !times || !n_pts || !stamps || !linear || !angular) return fail(c, LIW_EINVAL, "liw_lfe_deskew: null array");
    return launched(c, launch_deskew(c->L, pts, times, n_pts, stamps, linear, angular, (hipStream_t)stream));
}

int liw_lfe_spawn(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pts || !n_pts || slot < 0 || slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_spawn: bad argument");
    return spawn_launch(c, store, slot, pts, n_pts, times, 0, nullptr, nullptr, stream);
}

int liw_lfe_spawn_corners(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, int max_corners,
                          double* corners, int* n_corners, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pts || !n_pts || slot < 0 || slot >= c->L.slots || max_corners < 1 || !corners || !n_corners)
        return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: bad argument");
    return spawn_launch(c, store, slot, pts, n_pts, times, max_corners, corners, n_corners, stream);
}

int liw_lfe_corners_to_world(liw_lfe_ctx* c, void* store, int max_corners, const double* corners, const int* n_corners, const double* pose,
                             const unsigned char* mask, const unsigned char* clear, int acc_cap, double* acc, int* n_acc, void* stream) {
    LIW_FLEET_DEV(c);
    if (max_corners < 1 || !corners || !n_corners || !pose || acc_cap < 1 || !acc || !n_acc) return fail(c, LIW_EINVAL, "liw_lfe_corners_to_world: bad argument");
    return launched(c, launch_corners_world(store, c->L, c->P, max_corners, corners, n_corners, pose, mask, clear, acc_cap, acc, n_acc, (hipStream_t)stream));
}

int liw_lfe_match(liw_lfe_ctx* c, void* store, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap, int* count, double* recs,
                  int* idx1, int* idx2, double* match_pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose2 || !count || !recs || !match_pose || cap < 1 || kk < 0 || slot2 < 0 || slot2 >= c->L.slots ||
        !(slot1 == LIW_LFE_REF || (slot1 >= 0 && slot1 < c->L.slots)) || (slot1 != LIW_LFE_REF && !pose1))
        return fail(c, LIW_EINVAL, "liw_lfe_match: bad argument");
    return launched(c, launch_match(store, c->L, c->P, slot1, slot2, pose1, pose2, kk, cap, count, recs, idx1, idx2, match_pose, (hipStream_t)stream));
}

int liw_lfe_add_scan(liw_lfe_ctx* c, void* store, int src_slot, const double* pose, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose || src_slot < 0 || src_slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_add_scan: bad argument");
    return add_scan_launch(c, store, src_slot, 1, false, pose, 6LL, 0LL, mask, nullptr, stream);
}

int liw_lfe_add_scan_flags(liw_lfe_ctx* c, void* store, int src_slot, const double* pose, const unsigned char* mask, unsigned char* flags, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose || !flags || src_slot < 0 || src_slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_add_scan_flags: bad argument");
    return add_scan_launch(c, store, src_slot, 1, false, pose, 6LL, 0LL, mask, flags, stream);
}

int liw_lfe_add_scan_path(liw_lfe_ctx* c) {
    if (!c) return LIW_EINVAL;
    if (!c->have_device) return fail(c, LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");
    return c->add_path < 0 ? fail(c, LIW_EINVAL, "liw_lfe_add_scan_path: no add_scan or rebuild yet") : c->add_path;
}

int liw_lfe_pack_track(liw_lfe_ctx* c, int n, int frame, int cap, const int* count, const double* recs, const double* match_pose, int L_cap,
                       int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match, void* stream) {
    LIW_FLEET_DEV(c);
    if (n < 1 || frame < 0 || frame >= n || cap < 1 || L_cap < 0 || !count || !recs || !match_pose || !laser_off || !laser_frame || !laser_pts ||
        !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_track: bad argument");
    if ((long long)c->L.B * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_track: B * cap must fit in int32");
    hipStream_t s = (hipStream_t)stream;
    const int Ltot = scan_offsets(c, "liw_lfe_pack_track", c->L.B, 1, cap, count, nullptr, L_cap, laser_off, s);
    if (Ltot < 0) return Ltot;
    if (int r = launched(c, launch_pack(c->L.B, n, frame, cap, Ltot, laser_off, recs, match_pose, laser_frame, laser_pts, match_pose_out, has_match, s))) return r;
    return Ltot;
}

int liw_lfe_match_front(liw_lfe_ctx* c, void* store, int front_slot, int first_slot, int F, const double* pose_front, const double* poses,
                        long long robot_stride, long long frame_stride, int kk, int cap, int* count, double* recs, int* idx1, int* idx2,
                        double* match_pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose_front || !poses || !count || !recs || !match_pose || cap < 1 || kk < 0 || F < 1 || first_slot < 0 ||
        (long long)first_slot + F > c->L.slots || front_slot < 0 || front_slot >= c->L.slots)
        return fail(c, LIW_EINVAL, "liw_lfe_match_front: bad argument");
    if ((long long)c->L.B * F >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_match_front: B * F must fit in int32");
    if (match_lds(c->L) > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_match_front: max_lines needs more than 64 KiB of LDS");
    return launched(c, launch_match_wave(store, c->L, c->P, front_slot, first_slot, F, pose_front, poses, robot_stride, frame_stride, kk, cap, count, recs,
                                         idx1, idx2, match_pose, (hipStream_t)stream));
}

int liw_lfe_pack_init(liw_lfe_ctx* c, int n, int cap, const int* count, const double* recs, const double* match_pose, const double* pose_front,
                      int L_cap, int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match,
                      unsigned char* init_ok, void* stream) {
    LIW_FLEET_DEV(c);
    if (n < 2 || cap < 1 || L_cap < 0 || !count || !recs || !match_pose || !pose_front || !laser_off || !laser_frame || !laser_pts ||
        !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_init: bad argument");
    if ((long long)c->L.B * (n - 1) * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_init: B * (n - 1) * cap must fit in int32");
    if (pack_init_lds(n) > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_pack_init: n needs more than 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    const int Ltot = scan_offsets(c, "liw_lfe_pack_init", c->L.B, n - 1, cap, count, nullptr, L_cap, laser_off, s);
    if (Ltot < 0) return Ltot;
    if (int r = launched(c, launch_pack_init(c->L.B, n, cap, Ltot, laser_off, count, recs, match_pose, pose_front, 6, nullptr, laser_frame, laser_pts,
                                             match_pose_out, has_match, init_ok, s)))
        return r;
    return Ltot;
}

int liw_lfe_rebuild(liw_lfe_ctx* c, void* store, int first_slot, int F, const double* poses, long long robot_stride, long long frame_stride,
                    const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !poses || F < 1 || first_slot < 0 || (long long)first_slot + F > c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_rebuild: bad argument");
    return add_scan_launch(c, store, first_slot, F, true, poses, robot_stride, frame_stride, mask, nullptr, stream);
}

int liw_lfe_track_init(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, const double* x, long long robot_stride, const double* angular_local,
                       const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !x || robot_stride < 1) return fail(c, LIW_EINVAL, "liw_lfe_track_init: bad argument");
    return launched(c, launch_track_init(c->L.B, track, x, robot_stride, angular_local, mask, (hipStream_t)stream));
}

int liw_lfe_track_begin(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, double* x, const double* imu_X, const double* imu_Dt,
                        const double* wheel_T, const double* stamps, const unsigned char* mask, double* linear, double* angular, double* pose_new,
                        unsigned char* skip, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !x || !imu_X || !imu_Dt || !wheel_T || !stamps || !linear || !angular || !pose_new || !skip)
        return fail(c, LIW_EINVAL, "liw_lfe_track_begin: null argument");
    return launched(c, launch_track_begin(c->L.B, c->P, track_tp(tp), track, x, imu_X, imu_Dt, wheel_T, stamps, mask, linear, angular, pose_new, skip,
                                          (hipStream_t)stream));
}

int liw_lfe_track_end(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, const void* store, int slot, const double* x, const int* count,
                      const unsigned char* mask, unsigned char* key, double* pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !store || !x || !count || !key || !pose || slot < 0 || slot >= c->L.slots)
        return fail(c, LIW_EINVAL, "liw_lfe_track_end: bad argument");
    return launched(c, launch_track_end(store, c->L, c->P, track_tp(tp), track, slot, x, count, mask, key, pose, (hipStream_t)stream));
}

int liw_lfe_track_get(liw_lfe_ctx* c, const void* track, int robot, double* tf12, double* angular3, double* stamp, int* counters) {
    LIW_FLEET_DEV(c);
    if (!track || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_lfe_track_get: bad argument");
    Trk t;
    if (!pull(track, (size_t)robot * kTrkBytes, &t, 1)) return fail(c, LIW_EHIP, "hipMemcpy");
    if (tf12) { for (int k = 0; k < 9; ++k) tf12[k] = t.kf_R[k]; for (int k = 0; k < 3; ++k) tf12[9 + k] = t.kf_t[k]; }
    if (angular3) for (int k = 0; k < 3; ++k) angular3[k] = t.ang[k];
    if (stamp) *stamp = t.stamp;
    if (counters) { counters[0] = t.tracked; counters[1] = t.keys; counters[2] = t.skipped; }
    return LIW_OK;
}

int liw_lfe_init_reset(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* init, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !init) return fail(c, LIW_EINVAL, "liw_lfe_init_reset: bad argument");
    return launched(c, launch_init_reset(c->L.B, init_ip(tp, nullptr), init, mask, (hipStream_t)stream));
}

int liw_lfe_init_get(liw_lfe_ctx* c, const void* init, int robot, int* status, int* n_frames, double* state15, double* angular3, int* counters) {
    LIW_FLEET_DEV(c);
    if (!init || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_lfe_init_get: bad argument");
    Ini r;
    if (!pull(init, (size_t)robot * kIniBytes, &r, 1)) return fail(c, LIW_EHIP, "hipMemcpy");
    if (status) *status = r.status;
    if (n_frames) *n_frames = r.n_frames;
    if (state15) {
        for (int k = 0; k < 3; ++k) { state15[k] = r.p[k]; state15[3 + k] = r.q[k]; state15[6 + k] = r.v[k]; }
        for (int k = 0; k < 6; ++k) state15[9 + k] = r.bs[k];
    }
    if (angular3) for (int k = 0; k < 3; ++k) angular3[k] = r.ang[k];
    if (counters) { counters[0] = r.inits; counters[1] = r.failed; counters[2] = r.dropped; }
    return LIW_OK;
}

// Two launches: k_lfe_init_begin decides a lane per robot and leaves in d_rows the interval row each robot's arrays go to, then
// k_lfe_init_rows copies them a wavefront per robot.
int liw_lfe_init_begin(liw_lfe_ctx* c, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, const double* imu_X,
                       const double* imu_J, const double* imu_sqrtP, const double* imu_Dt, const double* wheel_T, const double* wheel_sqrtP,
                       const unsigned char* mask, double* x_init, double* w_imu_X, double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt,
                       double* w_wheel_T, double* w_wheel_sqrtP, unsigned char* drop, int* slot_of, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !ip || !init || !imu_X || !imu_J || !imu_sqrtP || !imu_Dt || !wheel_T || !wheel_sqrtP || !x_init || !w_imu_X || !w_imu_J ||
        !w_imu_sqrtP || !w_imu_Dt || !w_wheel_T || !w_wheel_sqrtP || !drop || !slot_of)
        return fail(c, LIW_EINVAL, "liw_lfe_init_begin: null argument");
    if (ip->slide_window_size < 2 || ip->slide_window_size > c->L.slots - 1)
        return fail(c, LIW_EINVAL, "liw_lfe_init_begin: slide_window_size must be 2 .. slots - 1");
    if (!c->d_rows && hipMalloc(&c->d_rows, sizeof(int) * (size_t)c->L.B) != hipSuccess) { c->d_rows = nullptr; return fail(c, LIW_ENOMEM, "hipMalloc"); }
    hipStream_t s = (hipStream_t)stream;
    if (int r = launched(c, launch_init_begin(c->L.B, c->P, init_ip(tp, ip), init, imu_X, imu_Dt, wheel_T, mask, x_init, drop, slot_of, c->d_rows, s))) return r;
    return launched(c, launch_init_rows(c->L.B, ip->slide_window_size - 1, c->d_rows, imu_X, imu_J, imu_sqrtP, imu_Dt, wheel_T, wheel_sqrtP, w_imu_X, w_imu_J,
                                        w_imu_sqrtP, w_imu_Dt, w_wheel_T, w_wheel_sqrtP, s));
}

int liw_lfe_slot_copy(liw_lfe_ctx* c, void* store, const int* dst_slot, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !dst_slot) return fail(c, LIW_EINVAL, "liw_lfe_slot_copy: null argument");
    if (((size_t)store & 15) != 0) return fail(c, LIW_EINVAL, "liw_lfe_slot_copy: the store must be 16-byte aligned");
    return launched(c, launch_slot_copy(store, c->L, dst_slot, mask, (hipStream_t)stream));
}

int liw_lfe_init_select(liw_lfe_ctx* c, const liw_lfe_init_params* ip, const void* init, unsigned char* ready, int* sel, int* n_sel, int* R_host,
                        void* stream) {
    LIW_FLEET_DEV(c);
    if (!ip || !init || !ready || !sel || !n_sel || ip->slide_window_size < 2) return fail(c, LIW_EINVAL, "liw_lfe_init_select: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (int r = launched(c, launch_init_select(c->L.B, ip->slide_window_size, init, ready, sel, n_sel, s))) return r;
    if (R_host && hipMemcpyAsync(R_host, n_sel, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(c, LIW_EHIP, "liw_lfe_init_select: copy of R");
    return LIW_OK;
}

int liw_lfe_pack_init_sel(liw_lfe_ctx* c, int R, const int* sel, int n, int cap, const int* count, const double* recs, const double* match_pose,
                          const double* pose_front, long long front_stride, int L_cap, int* laser_off, int* laser_frame, double* laser_pts,
                          double* match_pose_out, unsigned char* has_match, unsigned char* init_ok, void* stream) {
    LIW_FLEET_DEV(c);
    if (R < 1 || R > c->L.B || !sel || n < 2 || cap < 1 || L_cap < 0 || front_stride < 6 || !count || !recs || !match_pose || !pose_front || !laser_off ||
        !laser_frame || !laser_pts || !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: bad argument");
    if ((long long)c->L.B * (n - 1) * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: B * (n - 1) * cap must fit in int32");
    if (pack_init_lds(n) > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: n needs more than 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    const int Ltot = scan_offsets(c, "liw_lfe_pack_init_sel", R, n - 1, cap, count, sel, L_cap, laser_off, s);
    if (Ltot < 0) return Ltot;
    if (int r = launched(c, launch_pack_init(R, n, cap, Ltot, laser_off, count, recs, match_pose, pose_front, front_stride, sel, laser_frame, laser_pts,
                                             match_pose_out, has_match, init_ok, s)))
        return r;
    return Ltot;
}

int liw_lfe_init_commit(liw_lfe_ctx* c, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, void* track, int R, const int* sel,
                        const unsigned char* init_ok, const double* x_sol, double* x_init, double* x_track, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !ip || !init || !track || R < 1 || R > c->L.B || !sel || !init_ok || !x_sol || !x_init || !x_track || ip->slide_window_size < 2)
        return fail(c, LIW_EINVAL, "liw_lfe_init_commit: bad argument");
    return launched(c, launch_init_commit(R, init_ip(tp, ip), init, track, sel, init_ok, x_sol, x_init, x_track, (hipStream_t)stream));
}

int liw_lfe_crmath_eval(liw_lfe_ctx* c, int op, int n, const double* a, const double* b, double* out, void* stream) {
    LIW_FLEET_DEV(c);
    if (op < 0 || op > 2 || n < 0 || !a || !out || (op == 2 && !b)) return fail(c, LIW_EINVAL, "liw_lfe_crmath_eval: bad argument");
    if (n == 0) return LIW_OK;
    return launched(c, launch_crmath(op, n, a, b, out, (hipStream_t)stream));
}

int liw_lfe_status(liw_lfe_ctx* c, const void* store, int robot, int slot) {
    if (slot == LIW_LFE_ROBOT) {
        if (int r = getter_head(c, store, robot, true)) return r;
        Mgr m;
        int sub;
        if (int r = host_mgr(c, store, robot, slot, m, sub)) return r;
        return m.status;
    }
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    return r < 0 ? r : (r == 1 ? LIW_LFE_NONE : h.status);
}

int liw_lfe_num_lines(liw_lfe_ctx* c, const void* store, int robot, int slot) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    return r < 0 ? r : (r == 1 ? LIW_LFE_NONE : h.n_lines);
}

int liw_lfe_get_lines(liw_lfe_ctx* c, const void* store, int robot, int slot, double* out, int cap) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    if (r) return r < 0 ? r : 0;
    const int nl = h.n_lines < c->L.max_lines ? h.n_lines : c->L.max_lines;
    const int n = nl < cap ? nl : cap;
    if (n > 0 && out && !pull(store, (size_t)robot * c->L.robot_bytes + slot_off(c->L, phys) + kHdrBytes, out, 10 * (size_t)n))
        return fail(c, LIW_EHIP, "hipMemcpy");
    return n < 0 ? 0 : n;
}

int liw_lfe_cell_lines(liw_lfe_ctx* c, const void* store, int robot, int slot, double x, double y, int* ids, int cap) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    if (r) return r < 0 ? r : LIW_LFE_NONE;
    int cc, rr;
    xy_to_index(c->P, x, y, cc, rr);
    if (!valid(c->P, rr, cc)) return LIW_LFE_NONE;
    const int ne = h.n_entries < 0 ? 0 : (h.n_entries < c->L.max_entries ? h.n_entries : c->L.max_entries);
    std::vector<u64> ent((size_t)ne + 1);
    if (!pull(store, (size_t)robot * c->L.robot_bytes + slot_off(c->L, phys) + kHdrBytes + 80 * (size_t)c->L.max_lines, ent.data(), (size_t)ne))
        return fail(c, LIW_EHIP, "hipMemcpy");
    const u64 key = (u64)(unsigned)(rr * c->P.w + cc);
    int k = 0;
    for (int j = lower_bound(ent.data(), ne, key << 32); j < ne && (ent[j] >> 32) == key; ++j, ++k)
        if (ids && k < cap) ids[k] = (int)(unsigned)(ent[j] & 0xffffffffull);
    return k;
}

int liw_lfe_submap_pose(liw_lfe_ctx* c, const void* store, int robot, int slot, double* p3, double* q3) {
    if (int r = getter_head(c, store, robot, slot == LIW_LFE_REF || slot == LIW_LFE_SPAWNING)) return r;
    Mgr m;
    int sub;
    if (int r = host_mgr(c, store, robot, slot, m, sub)) return r;
    if (sub < 0) return LIW_LFE_NONE;
    for (int k = 0; k < 3; ++k) {
        if (p3) p3[k] = m.sub_p[sub][k];
        if (q3) q3[k] = m.sub_q[sub][k];
    }
    return 0;
}

}  // extern "C"
