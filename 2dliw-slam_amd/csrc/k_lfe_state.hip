// k_lfe_state.hip — fleet laser front-end, the per-robot state machines (C ABI include/liw_laser_batch.h, host side
// liw_laser_batch.cpp): the glue of a tracking frame (k_lfe_track_*) and the INITIALIZING state machine (k_lfe_init_*), each on a
// 256-byte record per robot, and the diagnostic entry of liw_crmath.hpp.  No atomics, no scratch; the sin / cos / atan2 of the pose
// predictions are the correctly rounded ones (CR, k_lfe_dev.hpp).
#pragma clang fp contract(off)   // the x86-64 host build of liw_laser.cpp does not contract; hipcc contracts device code by default

#include <hip/hip_runtime.h>

#include "k_lfe.hpp"
#include "k_lfe_dev.hpp"

namespace lfe {

// ------------------------------------------------------------------------------------------------------ tracking glue
// lvio_2d::trajectory::add_sensor_data(laser) around the stages of the other units (trajectory.cpp:140-148, :176-184, :82-92, the
// key-frame decision after do_tracking): the de-skew twist, the min_delta_t gate, the window roll and the pose prediction from the
// wheel increment before the scan; the key-frame decision after the solve.  A lane per robot, work-groups of 256, no LDS: a few
// hundred fp64 operations and a handful of strided 8-byte accesses each.
__host__ __device__ inline Trk* trk_at(void* track, int b) { return (Trk*)((char*)track + (size_t)b * kTrkBytes); }

__global__ void __launch_bounds__(256) k_lfe_track_init(int B, void* track, const double* x, long long robot_stride, const double* ang,
                                                       const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    const Iso<double> T = tf6(x + (long long)b * robot_stride);
    double* z = (double*)t;
    for (size_t k = 0; k < kTrkBytes / 8; ++k) z[k] = 0.0;
    for (int k = 0; k < 9; ++k) t->kf_R[k] = T.R.m[k];
    t->kf_t[0] = T.t.x; t->kf_t[1] = T.t.y; t->kf_t[2] = T.t.z;
    if (ang) for (int k = 0; k < 3; ++k) t->ang[k] = ang[3 * (size_t)b + k];
}

__global__ void __launch_bounds__(256) k_lfe_track_begin(int B, DP P, TP tp, void* track, double* x, const double* imu_X, const double* imu_Dt,
                                                        const double* wheel_T, const double* stamps, const unsigned char* mask, double* linear,
                                                        double* angular, double* pose_new, unsigned char* skip) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    double* x0 = x + 30 * (size_t)b;
    double* x1 = x0 + 15;
    typedef V3<CR> VC;
    const Iso<CR> Twi = liw::make_tf(liw::cast_v3<CR>(x1), liw::cast_v3<CR>(x1 + 3)), Til = liw::cast_iso<CR>(P.Til_R, P.Til_t);
    // de-skew with the current body twist (:140-148): R_w_laser^T v and log_SO3(R_il^T exp_so3(current_angular_local) R_il)
    const VC lin = liw::mulT(liw::mul(Twi, Til).R, liw::cast_v3<CR>(x1 + 6));
    const VC ang = liw::log_SO3(liw::mul(liw::mul(liw::transpose(Til.R), liw::exp_so3(liw::cast_v3<CR>(t->ang))), Til.R));
    linear[3 * (size_t)b] = lin.x.v; linear[3 * (size_t)b + 1] = lin.y.v; linear[3 * (size_t)b + 2] = lin.z.v;
    angular[3 * (size_t)b] = ang.x.v; angular[3 * (size_t)b + 1] = ang.y.v; angular[3 * (size_t)b + 2] = ang.z.v;
    const double Dt = imu_Dt[b];
    const bool sk = Dt < tp.min_dt;
    skip[b] = sk ? 1 : 0;
    if (sk) { t->skipped += 1; return; }
    for (int k = 0; k < 15; ++k) x0[k] = x1[k];   // pop_frame_for_tracking: the newest frame becomes the window's front
    // update_current_status with wheel_delta_to_imu_delta: T_w_i * (T_iw * dT * T_iw^-1)
    const Iso<CR> Tiw = liw::cast_iso<CR>(tp.Tiw_R, tp.Tiw_t);
    const double* w = wheel_T + 12 * (size_t)b;
    const Iso<CR> delta = liw::mul(liw::mul(Tiw, liw::cast_iso<CR>(w, w + 9)), liw::inverse(Tiw));
    const Iso<CR> N = liw::mul(Twi, delta);
    const VC q = liw::log_SO3(N.R);
    x1[0] = N.t.x.v; x1[1] = N.t.y.v; x1[2] = N.t.z.v; x1[3] = q.x.v; x1[4] = q.y.v; x1[5] = q.z.v;
    for (int k = 0; k < 3; ++k) t->ang[k] = imu_X[15 * (size_t)b + 6 + k] / Dt;   // gamma / Dt
    t->stamp = stamps[b];
    for (int k = 0; k < 6; ++k) pose_new[6 * (size_t)b + k] = x1[k];
}

__global__ void __launch_bounds__(256) k_lfe_track_end(const void* store, Lay L, DP P, TP tp, void* track, int slot, const double* x, const int* count,
                                                      const unsigned char* mask, unsigned char* key, double* pose) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    const double* x1 = x + 30 * (size_t)b + 15;
    for (int k = 0; k < 6; ++k) pose[6 * (size_t)b + k] = x1[k];
    const Iso<double> Twl = liw::mul(tf6(x1), til(P));
    const Iso<double> d = liw::mul(liw::inverse(liw::cast_iso<double>(t->kf_R, t->kf_t)), Twl);
    const bool is_static = vnorm(d.t) < tp.p_thr && vnorm(liw::log_SO3(d.R)) < tp.q_thr;
    const Slot s = slot_at(const_cast<void*>(store), L, b, slot);
    const int n_match = count[b], n_no_match = n_lines(s, L) - n_match;
    const bool kf = !is_static || n_match < n_no_match;
    key[b] = kf ? 1 : 0;
    t->tracked += 1;
    if (kf) {
        t->keys += 1;
        for (int k = 0; k < 9; ++k) t->kf_R[k] = Twl.R.m[k];
        t->kf_t[0] = Twl.t.x; t->kf_t[1] = Twl.t.y; t->kf_t[2] = Twl.t.z;
    }
}

// ---------------------------------------------------------------------------------------------------- initialisation glue
// lvio_2d::trajectory::add_sensor_data(laser) while status == INITIALIZING (trajectory.cpp: the is_static gate, update_current_status,
// the frame pushed into the window) and the bookkeeping of check_and_processing_initialize around the INIT solve.
__host__ __device__ inline Ini* ini_at(void* init, int b) { return (Ini*)((char*)init + (size_t)b * kIniBytes); }
constexpr int kIvDoubles = 15 + 225 + 225 + 1 + 12 + 9;   // one interval of the liw_batch arrays

// init_current_status: p, q = log_SE3(T_imu_to_wheel^-1), the rest 0, INITIALIZING with an empty window.  The counters are left
// as they are (a failed window restarts with them; liw_lfe_init_reset zeroes the whole record first)
__device__ inline void ini_restart(Ini* r, const IP& ip) {
    const Iso<CR> inv = liw::inverse(liw::cast_iso<CR>(ip.Tiw_R, ip.Tiw_t));
    const V3<CR> q = liw::log_SO3(inv.R);
    r->p[0] = inv.t.x.v; r->p[1] = inv.t.y.v; r->p[2] = inv.t.z.v;
    r->q[0] = q.x.v; r->q[1] = q.y.v; r->q[2] = q.z.v;
    for (int k = 0; k < 3; ++k) r->v[k] = r->ang[k] = 0.0;
    for (int k = 0; k < 6; ++k) r->bs[k] = 0.0;
    r->status = LIW_LFE_INITIALIZING;
    r->n_frames = 0;
}

__global__ void __launch_bounds__(256) k_lfe_init_reset(int B, IP ip, void* init, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Ini* r = ini_at(init, b);
    double* z = (double*)r;
    for (size_t k = 0; k < kIniBytes / 8; ++k) z[k] = 0.0;
    ini_restart(r, ip);
}

// Two launches.  k_lfe_init_begin: a lane per robot decides (gate, prediction, the record, the state row) and leaves in `row` (B
// ints of the ctx, not caller memory) the interval row the robot's arrays go to, -1 for a robot that copies nothing.
// k_lfe_init_rows: a wavefront per robot copies the 487 doubles of an accepted robot, 64 consecutive doubles at a time, so the copy
// runs B waves wide instead of a lane reading and writing 8 bytes at a stride.  No LDS, no atomics.
__global__ void __launch_bounds__(256) k_lfe_init_begin(int B, DP P, IP ip, void* init, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                                                       const unsigned char* mask, double* x_init, unsigned char* drop, int* slot_of, int* rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int row = -1;   // the interval row this robot's arrays go to (k - 1); -1: nothing to copy
    if (!(mask && !mask[b])) {
        Ini* r = ini_at(init, b);
        const int k = r->n_frames;
        if (r->status == LIW_LFE_INITIALIZING && k >= 0 && k < ip.N) {
            typedef V3<CR> VC;
            const Iso<CR> Tiw = liw::cast_iso<CR>(ip.Tiw_R, ip.Tiw_t), Til = liw::cast_iso<CR>(P.Til_R, P.Til_t);
            const double* w = wheel_T + 12 * (size_t)b;
            const Iso<CR> dW = liw::cast_iso<CR>(w, w + 9);
            // wheel_delta_to(T_imu_to_laser, delta): T_lw * delta * T_lw^-1 with T_lw = T_il^-1 * T_iw; is_static on its log_SE3
            const Iso<CR> Tlw = liw::mul(liw::inverse(Til), Tiw);
            const Iso<CR> dL = liw::mul(liw::mul(Tlw, dW), liw::inverse(Tlw));
            const bool st = liw::norm(dL.t).v < ip.p_thr && liw::norm(liw::log_SO3(dL.R)).v < ip.q_thr;
            drop[b] = st ? 1 : 0;
            if (st) {
                r->dropped += 1;
            } else {
                // update_current_status with wheel_delta_to_imu_delta: T_w_i * (T_iw * dT * T_iw^-1)
                const Iso<CR> N = liw::mul(liw::make_tf(liw::cast_v3<CR>(r->p), liw::cast_v3<CR>(r->q)), liw::mul(liw::mul(Tiw, dW), liw::inverse(Tiw)));
                const VC q = liw::log_SO3(N.R);
                r->p[0] = N.t.x.v; r->p[1] = N.t.y.v; r->p[2] = N.t.z.v; r->q[0] = q.x.v; r->q[1] = q.y.v; r->q[2] = q.z.v;
                double* x = x_init + ((size_t)b * ip.N + k) * 15;
                for (int i = 0; i < 3; ++i) { x[i] = r->p[i]; x[3 + i] = r->q[i]; x[6 + i] = r->v[i]; }
                for (int i = 0; i < 6; ++i) x[9 + i] = r->bs[i];
                const double Dt = imu_Dt[b];
                for (int i = 0; i < 3; ++i) r->ang[i] = imu_X[15 * (size_t)b + 6 + i] / Dt;   // gamma / Dt
                slot_of[b] = 1 + k;
                r->n_frames = k + 1;
                row = k - 1;   // frame 0's interval is not stored
            }
        }
    }
    rows[b] = row;
}

__global__ void __launch_bounds__(kBlock) k_lfe_init_rows(int F, const int* rows, const double* imu_X, const double* imu_J, const double* imu_sqrtP,
                                                         const double* imu_Dt, const double* wheel_T, const double* wheel_sqrtP, double* w_imu_X,
                                                         double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt, double* w_wheel_T, double* w_wheel_sqrtP) {
    const size_t src = blockIdx.x;
    const int r = rows[src];
    if (r < 0) return;
    const size_t dst = src * F + r;
    for (int e = threadIdx.x; e < kIvDoubles; e += kBlock) {
        if (e < 15) w_imu_X[dst * 15 + e] = imu_X[src * 15 + e];
        else if (e < 240) w_imu_J[dst * 225 + (e - 15)] = imu_J[src * 225 + (e - 15)];
        else if (e < 465) w_imu_sqrtP[dst * 225 + (e - 240)] = imu_sqrtP[src * 225 + (e - 240)];
        else if (e < 466) w_imu_Dt[dst] = imu_Dt[src];
        else if (e < 478) w_wheel_T[dst * 12 + (e - 466)] = wheel_T[src * 12 + (e - 466)];
        else w_wheel_sqrtP[dst * 9 + (e - 478)] = wheel_sqrtP[src * 9 + (e - 478)];
    }
}

// ready[b] = INITIALIZING with a full window; sel = the ready robots in ascending order, n_sel[0] = their number.  One block of 1024 as
// k_lfe_scan_init: positions are prefix counts, so the list does not depend on the order the lanes run in.
__global__ void __launch_bounds__(1024) k_lfe_init_select(int B, int N, const void* init, unsigned char* ready, int* sel, int* n_sel) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = lo + per < B ? lo + per : B;
    auto is_ready = [&](int b) { const Ini* r = ini_at(const_cast<void*>(init), b); return r->status == LIW_LFE_INITIALIZING && r->n_frames == N; };
    int s = 0;
    for (int b = lo; b < hi; ++b) s += is_ready(b) ? 1 : 0;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = lo; b < hi; ++b) {
        const bool r = is_ready(b);
        ready[b] = r ? 1 : 0;
        if (r) sel[run++] = b;
    }
    if (t == 1023) n_sel[0] = part[1023];
}

// After the INIT solve and the marginalisation, a lane per selected robot b = sel[r].  init_ok[r]: take_back_state (the record's
// p q v bs := the last solved frame), the solved window back into x_init (what liw_lfe_rebuild reads), both rows of the tracking
// window := the last solved frame, the tracking record as k_lfe_track_init makes it (the same make_tf, so a robot committed here and
// one handed to liw_lfe_track_init start from the same bytes) with current_angular_local from the record, TRACKING.  Otherwise
// init_current_status and the failed-window counter.
__global__ void __launch_bounds__(256) k_lfe_init_commit(int R, IP ip, void* init, void* track, const int* sel, const unsigned char* init_ok,
                                                        const double* x_sol, double* x_init, double* x_track) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int b = sel[r], N = ip.N;
    Ini* rec = ini_at(init, b);
    if (!init_ok[r]) {
        ini_restart(rec, ip);
        rec->failed += 1;
        return;
    }
    const double* xs = x_sol + (size_t)r * N * 15;
    double* xi = x_init + (size_t)b * N * 15;
    for (int k = 0; k < N * 15; ++k) xi[k] = xs[k];
    const double* last = xs + (size_t)(N - 1) * 15;
    double* xt = x_track + 30 * (size_t)b;
    for (int k = 0; k < 15; ++k) xt[k] = xt[15 + k] = last[k];
    for (int k = 0; k < 3; ++k) { rec->p[k] = last[k]; rec->q[k] = last[3 + k]; rec->v[k] = last[6 + k]; }
    for (int k = 0; k < 6; ++k) rec->bs[k] = last[9 + k];
    rec->status = LIW_LFE_TRACKING;
    rec->inits += 1;
    Trk* t = trk_at(track, b);
    const Iso<double> T = tf6(last);
    double* z = (double*)t;
    for (size_t k = 0; k < kTrkBytes / 8; ++k) z[k] = 0.0;
    for (int k = 0; k < 9; ++k) t->kf_R[k] = T.R.m[k];
    t->kf_t[0] = T.t.x; t->kf_t[1] = T.t.y; t->kf_t[2] = T.t.z;
    for (int k = 0; k < 3; ++k) t->ang[k] = rec->ang[k];
}

// liw_lfe_crmath_eval: the three functions of liw_crmath.hpp as the CR scalar calls them, a lane per element (a diagnostic
// entry: tests/test_gpu_crmath.py compares the device compile of the header with a multi-precision reference).  out may alias a:
// a lane reads its element before it writes it.
__global__ void __launch_bounds__(256) k_lfe_crmath(int op, int n, const double* a, const double* b, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    out[i] = op == 0 ? liw_cr::cr_sin(x) : (op == 1 ? liw_cr::cr_cos(x) : liw_cr::cr_atan2(x, b[i]));
}

int launch_track_init(int B, void* track, const double* x, long long robot_stride, const double* ang, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_track_init, dim3(blocks(B, 256)), dim3(256), 0, s, B, track, x, robot_stride, ang, mask);
    return launched();
}

int launch_track_begin(int B, const DP& P, const TP& tp, void* track, double* x, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                       const double* stamps, const unsigned char* mask, double* linear, double* angular, double* pose_new, unsigned char* skip,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_track_begin, dim3(blocks(B, 256)), dim3(256), 0, s, B, P, tp, track, x, imu_X, imu_Dt, wheel_T, stamps, mask, linear, angular,
                       pose_new, skip);
    return launched();
}

int launch_track_end(const void* store, const Lay& L, const DP& P, const TP& tp, void* track, int slot, const double* x, const int* count,
                     const unsigned char* mask, unsigned char* key, double* pose, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_track_end, dim3(blocks(L.B, 256)), dim3(256), 0, s, store, L, P, tp, track, slot, x, count, mask, key, pose);
    return launched();
}

int launch_init_reset(int B, const IP& ip, void* init, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_init_reset, dim3(blocks(B, 256)), dim3(256), 0, s, B, ip, init, mask);
    return launched();
}

int launch_init_begin(int B, const DP& P, const IP& ip, void* init, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                      const unsigned char* mask, double* x_init, unsigned char* drop, int* slot_of, int* rows, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_init_begin, dim3(blocks(B, 256)), dim3(256), 0, s, B, P, ip, init, imu_X, imu_Dt, wheel_T, mask, x_init, drop, slot_of, rows);
    return launched();
}

int launch_init_rows(int B, int F, const int* rows, const double* imu_X, const double* imu_J, const double* imu_sqrtP, const double* imu_Dt,
                     const double* wheel_T, const double* wheel_sqrtP, double* w_imu_X, double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt,
                     double* w_wheel_T, double* w_wheel_sqrtP, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_init_rows, dim3(B), dim3(kBlock), 0, s, F, rows, imu_X, imu_J, imu_sqrtP, imu_Dt, wheel_T, wheel_sqrtP, w_imu_X, w_imu_J,
                       w_imu_sqrtP, w_imu_Dt, w_wheel_T, w_wheel_sqrtP);
    return launched();
}

int launch_init_select(int B, int N, const void* init, unsigned char* ready, int* sel, int* n_sel, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_init_select, dim3(1), dim3(1024), 0, s, B, N, init, ready, sel, n_sel);
    return launched();
}

int launch_init_commit(int R, const IP& ip, void* init, void* track, const int* sel, const unsigned char* init_ok, const double* x_sol, double* x_init,
                       double* x_track, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_init_commit, dim3(blocks(R, 256)), dim3(256), 0, s, R, ip, init, track, sel, init_ok, x_sol, x_init, x_track);
    return launched();
}

int launch_crmath(int op, int n, const double* a, const double* b, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_crmath, dim3(blocks((size_t)n, 256)), dim3(256), 0, s, op, n, a, b, out);
    return launched();
}

}  // namespace lfe
