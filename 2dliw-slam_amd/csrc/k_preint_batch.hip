// k_preint_batch.hip — the fleet's persistent pre-integration accumulators on the device (C ABI include/liw_preint_batch.h; host
// side liw_preint_batch.cpp).  One accumulator pair per robot lives in the store between calls; a push resumes it:
//   k_fpre_reset   a work-group per robot: the state liw_imu_preint_create / liw_wheel_preint_create leave, latches off
//   k_fpre_imu     k_preint_imu's mapping: 16 lanes per robot, four robots per wave, lane c owns column c of J and of P, one LDS
//                  transpose per step (imu_step of k_preint_dev.hpp).  Loads the region, walks this call's messages, stores the
//                  persisted (un-aligned) state and the pending stamp / bias, then runs update_only_t(stamp) in registers and writes
//                  the rows X, J, Dt and the aligned P (shared tail of the store, read by k_preint_imu_sqrt).  The wave walks as
//                  many steps as its longest robot; the shorter ones idle through imu_step's `act`.
//   k_fpre_wheel   a lane per robot: wheel_add per message, the persisted state, update_only_t(stamp) on a copy, the rows, `ready`
//   k_fpre_commit  16 lanes per robot: reset_imu_measure(stamp, bias) / reset_wheel_odom_measure(stamp) of the taken, ready robots
// A masked-out robot is never written: every store below is behind `on`.
#include "k_preint_batch.hpp"
#include "k_preint_dev.hpp"

namespace liw_fpre_dev {

using liw::PreintNoise;
using liw::WheelAcc;

__device__ __forceinline__ bool robot_on(const unsigned char* mask, int b, int B) { return b < B && (!mask || mask[b]); }
__device__ __forceinline__ double* region(char* store, const Lay& L, int b) { return (double*)(store + (size_t)b * L.robot_bytes); }

// the value of double i of a fresh region
__device__ __forceinline__ double fresh(int i) {
    if (i >= R_J && i < R_P) { const int r = (i - R_J) / kPitch, c = (i - R_J) % kPitch; return r == c ? 1.0 : 0.0; }
    if (i >= R_P && i < R_LACC) { const int r = (i - R_P) / kPitch, c = (i - R_P) % kPitch; return r == c ? 0.00001 : 0.0; }
    if (i == R_ILAST || i == R_WUPD) return -1.0;
    if (i >= R_WDELTA && i < R_WDELTA + 9) return (i - R_WDELTA) % 4 == 0 ? 1.0 : 0.0;
    if (i >= R_WPOSE && i < R_WPOSE + 9) return (i - R_WPOSE) % 4 == 0 ? 1.0 : 0.0;
    return 0.0;
}

__global__ __launch_bounds__(64) void k_fpre_reset(char* store, Lay L, const unsigned char* __restrict__ mask) {
    const int b = blockIdx.x;
    if (!robot_on(mask, b, L.B)) return;
    double* R = region(store, L, b);
    for (int i = threadIdx.x; i < kRobotDoubles; i += 64) R[i] = fresh(i);   // the latch word and the tail are zero bytes
}

__global__ __launch_bounds__(64) void k_fpre_imu(char* store, Lay L, PreintNoise N, const int* __restrict__ imu_off, const double* __restrict__ imu,
                                                 const double* __restrict__ stamps, const double* __restrict__ bias,
                                                 const unsigned char* __restrict__ mask, double* Xout, double* Jout, double* Dtout) {
    __shared__ double Tt[4][16 * 16];
    const int lane = threadIdx.x & 63, grp = lane >> 4, c = lane & 15;
    const int b = blockIdx.x * 4 + grp;
    const bool on = robot_on(mask, b, L.B);
    const int bb = on ? b : 0;
    double* R = region(store, L, bb);
    // ---- resume: the region into registers (rows of J and P are 128-byte pieces across the robot's 16 lanes)
    double X[15], Jc[15], Pc[15];
#pragma unroll
    for (int r = 0; r < 15; ++r) { X[r] = R[R_X + r]; Jc[r] = R[R_J + r * kPitch + c]; Pc[r] = R[R_P + r * kPitch + c]; }
    double la[3] = {R[R_LACC], R[R_LACC + 1], R[R_LACC + 2]};
    double lg[3] = {R[R_LGYR], R[R_LGYR + 1], R[R_LGYR + 2]};
    double last_t = R[R_ILAST], Dt = R[R_IDT];
    unsigned char inited = ((const unsigned char*)(R + R_LATCH))[0];
    const int s0 = imu_off[bb], s1 = imu_off[bb + 1];
    const int n = on && s1 > s0 ? s1 - s0 : 0;
    int nmax = n;
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
    // ---- add_imu_measure per message (liw_imu_preint_add): integrate from the previous message unless there is none yet
    for (int i = 0; i < nmax; ++i) {
        const bool have = i < n;
        const size_t si = (size_t)(s0 + (have ? i : 0)) * 7;
        const double tn = have ? imu[si] : 0.0;
        const bool act = have && last_t != -1.0;
        const double dt = act ? tn - last_t : 0.0;
        liw::imu_step(X, Jc, Pc, la, lg, dt, act, N, Tt[grp], c);
        if (act) { Dt += dt; inited = 1; }
        if (have) {
            la[0] = imu[si + 1]; la[1] = imu[si + 2]; la[2] = imu[si + 3];
            lg[0] = imu[si + 4]; lg[1] = imu[si + 5]; lg[2] = imu[si + 6];
            last_t = tn;
        }
    }
    const double stamp = stamps[bb];
    // ---- the persisted, un-aligned accumulator and what a commit resets with
    if (on) {
        if (c < 15) {
            R[R_X + c] = X[c];
#pragma unroll
            for (int r = 0; r < 15; ++r) { R[R_J + r * kPitch + c] = Jc[r]; R[R_P + r * kPitch + c] = Pc[r]; }
        }
        if (c < 6) R[R_BIAS + c] = bias[(size_t)b * 6 + c];
        if (c == 15) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { R[R_LACC + k] = la[k]; R[R_LGYR + k] = lg[k]; }
            R[R_ILAST] = last_t; R[R_IDT] = Dt; R[R_STAMP] = stamp;
            ((unsigned char*)(R + R_LATCH))[0] = inited;
        }
    }
    // ---- update_only_t(stamp) on the copy in registers, and its result
    {
        const bool act = on && last_t != -1.0;
        const double dt = act ? stamp - last_t : 0.0;
        liw::imu_step(X, Jc, Pc, la, lg, dt, act, N, Tt[grp], c);
        if (act) Dt += dt;
    }
    if (on) liw::imu_write_rows((size_t)b, c, X, Jc, Pc, Dt, Xout, Jout, (double*)(store + L.s_P), Dtout);
}

__global__ __launch_bounds__(64) void k_fpre_wheel(char* store, Lay L, PreintNoise N, const int* __restrict__ wheel_off, const double* __restrict__ wheel,
                                                   const double* __restrict__ stamps, const unsigned char* __restrict__ mask, double* T12,
                                                   double* sq9, double* Dtout, unsigned char* ready) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (!robot_on(mask, b, L.B)) return;
    double* R = region(store, L, b);
    WheelAcc A;
#pragma unroll
    for (int k = 0; k < 9; ++k) { A.delta.R.m[k] = R[R_WDELTA + k]; A.last_pose.R.m[k] = R[R_WPOSE + k]; }
    A.delta.t = liw::V3<double>(R[R_WDELTA + 9], R[R_WDELTA + 10], R[R_WDELTA + 11]);
    A.last_pose.t = liw::V3<double>(R[R_WPOSE + 9], R[R_WPOSE + 10], R[R_WPOSE + 11]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { A.v[k] = R[R_WV + k]; A.om[k] = R[R_WOM + k]; }
    A.last_update = R[R_WUPD]; A.last_add = R[R_WADD]; A.Dt = R[R_WDT];
    unsigned char* latch = (unsigned char*)(R + R_LATCH);
    unsigned char inited = latch[1];
    const int s0 = wheel_off[b], s1 = wheel_off[b + 1];
    for (int s = s0; s < s1; ++s)
        if (liw::wheel_add(A, wheel + (size_t)s * 13)) inited = 1;
#pragma unroll
    for (int k = 0; k < 9; ++k) { R[R_WDELTA + k] = A.delta.R.m[k]; R[R_WPOSE + k] = A.last_pose.R.m[k]; }
    R[R_WDELTA + 9] = A.delta.t.x; R[R_WDELTA + 10] = A.delta.t.y; R[R_WDELTA + 11] = A.delta.t.z;
    R[R_WPOSE + 9] = A.last_pose.t.x; R[R_WPOSE + 10] = A.last_pose.t.y; R[R_WPOSE + 11] = A.last_pose.t.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) { R[R_WV + k] = A.v[k]; R[R_WOM + k] = A.om[k]; }
    R[R_WUPD] = A.last_update; R[R_WADD] = A.last_add; R[R_WDT] = A.Dt;
    latch[1] = inited;
    ready[b] = (latch[0] && inited) ? 1 : 0;   // byte 0 is k_fpre_imu's, which ran before on the same stream
    // update_only_t(stamp) on the copy
    if (A.last_update >= 0) { liw::wheel_update_by_v(A, stamps[b] - A.last_update); A.last_update = stamps[b]; }
    liw::wheel_write_rows((size_t)b, A, N, T12, sq9, Dtout);
}

__global__ __launch_bounds__(64) void k_fpre_commit(char* store, Lay L, const unsigned char* __restrict__ taken, const unsigned char* __restrict__ mask) {
    const int lane = threadIdx.x & 63, c = lane & 15;
    const int b = blockIdx.x * 4 + (lane >> 4);
    if (!robot_on(mask, b, L.B) || !taken[b]) return;
    double* R = region(store, L, b);
    const unsigned char* latch = (const unsigned char*)(R + R_LATCH);
    if (!latch[0] || !latch[1]) return;
    const double stamp = R[R_STAMP];
    if (c < 15) {
        R[R_X + c] = c >= 9 ? R[R_BIAS + c - 9] : 0.0;
#pragma unroll
        for (int r = 0; r < 15; ++r) { R[R_J + r * kPitch + c] = r == c ? 1.0 : 0.0; R[R_P + r * kPitch + c] = r == c ? 0.00001 : 0.0; }
        if (c < 12) R[R_WDELTA + c] = (c < 9 && c % 4 == 0) ? 1.0 : 0.0;
    } else {
        R[R_ILAST] = stamp; R[R_IDT] = 0.0;
        R[R_WUPD] = stamp; R[R_WDT] = 0.0;
    }
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fpre_reset, dim3(L.B), dim3(64), 0, s, store, L, mask);
    return launched();
}

int launch_push(char* store, const Lay& L, const PreintNoise& N, const int* imu_off, const double* imu, const int* wheel_off, const double* wheel,
                const double* stamps, const double* bias, const unsigned char* mask, const Rows& out, hipStream_t s) {
    hipLaunchKernelGGL(k_fpre_imu, dim3((L.B + 3) / 4), dim3(64), 0, s, store, L, N, imu_off, imu, stamps, bias, mask, out.imu_X, out.imu_J, out.imu_Dt);
    liw::launch_preint_imu_sqrt(L.B, (const double*)(store + L.s_P), out.imu_sqrtP, mask, s);
    hipLaunchKernelGGL(k_fpre_wheel, dim3((L.B + 63) / 64), dim3(64), 0, s, store, L, N, wheel_off, wheel, stamps, mask, out.wheel_T, out.wheel_sqrtP,
                       out.wheel_Dt, out.ready);
    return launched();
}

int launch_commit(char* store, const Lay& L, const unsigned char* taken, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fpre_commit, dim3((L.B + 3) / 4), dim3(64), 0, s, store, L, taken, mask);
    return launched();
}

}  // namespace liw_fpre_dev
