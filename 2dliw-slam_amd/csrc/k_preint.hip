// k_preint.hip — batched pre-integration on the device ("batch replay" form of SURVEY §8 rows a5 / a6).
//
// The reference integrates one interval at a time on the CPU while messages arrive
// (imu_preintegraption::update, src/factor/imu_preintegraption.h:170-208; wheel_odom_preintegration,
// src/factor/wheel_odom_preintegration.h:62-152).  When whole logs are replayed, every interval between two frames is
// independent, so M intervals are integrated in parallel here:
//   k_preint_imu       4 intervals per wave, 16 lanes each; lane c owns COLUMN c of J and of the covariance P.
//                      F = I + dt*Fc only mixes rows, so J <- F J and T = F P are per-lane; P' = F P F^T uses the
//                      symmetry P' = (F T^T)^T: one 15x15 transpose through LDS, then the same per-lane row update.
//   k_preint_imu_sqrt  one wave per interval: sqrt_inverse_P = LLT(P^-1).matrixL().transpose() (:149) with the
//                      register-resident fused Cholesky: P = L L^T with identity right-hand sides gives W = L^-1,
//                      P^-1 = W^T W on the fp64 matrix cores, a second Cholesky gives the result.
//   k_preint_wheel     one thread per interval (a handful of odometry samples each).
// Same quirks as the reference (SURVEY Appendix C 5,6): previous sample drives the whole Euler step, F(gamma,gamma)
// is built from hat_gyro - last_ba, P0 = 1e-5 I.  Replay semantics = the host pre-integrators of liw_preint.cpp:
// sample 0 of an interval seeds last_info, the accumulator is reset at t_start, integrated to t_end.
// The per-sample IMU step and the wheel add / update_by_v bodies are in k_preint_dev.hpp, shared with the fleet's persistent
// accumulators (k_preint_batch.hip).
#include "k_preint_dev.hpp"
#include "liw_kernels.hpp"

namespace liw {

typedef double d4p __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double rdl(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(64) void k_preint_imu(int M, const int* sample_off, const double* samples, const double* t_start,
                                                   const double* t_end, const double* bias6, PreintNoise N, double* Xout, double* Jout,
                                                   double* Pout, double* Dtout) {
    __shared__ double Tt[4][16 * 16];
    const int lane = threadIdx.x & 63, grp = lane >> 4, c = lane & 15;
    const int m = blockIdx.x * 4 + grp;
    const bool on = m < M;
    const int mm = on ? m : 0;
    const int s0 = sample_off[mm], s1 = sample_off[mm + 1];
    double X[15], Jc[15], Pc[15];
#pragma unroll
    for (int r = 0; r < 15; ++r) { X[r] = 0.0; Jc[r] = r == c ? 1.0 : 0.0; Pc[r] = r == c ? 0.00001 : 0.0; }
#pragma unroll
    for (int k = 0; k < 6; ++k) X[9 + k] = bias6[mm * 6 + k];
    double last_t = t_start[mm], Dt = 0.0;
    double la[3] = {samples[(size_t)s0 * 7 + 1], samples[(size_t)s0 * 7 + 2], samples[(size_t)s0 * 7 + 3]};
    double lg[3] = {samples[(size_t)s0 * 7 + 4], samples[(size_t)s0 * 7 + 5], samples[(size_t)s0 * 7 + 6]};
    // the wave walks as many steps as its longest interval; shorter intervals idle (exec-masked through `act`)
    int nsteps = on ? (s1 - s0) : 0;   // samples 1..cnt-1 plus the final update_only_t
    int nmax = nsteps;
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
    for (int step = 1; step <= nmax; ++step) {
        const bool act = step <= nsteps;
        const bool is_last = step == nsteps;
        const size_t si = (size_t)(s0 + (act && !is_last ? step : 0)) * 7;
        const double tn = (act && !is_last) ? samples[si] : t_end[mm];
        const double dt = act ? tn - last_t : 0.0;
        imu_step(X, Jc, Pc, la, lg, dt, act, N, Tt[grp], c);   // update(dt) with the PREVIOUS sample
        if (act) {
            Dt += dt;
            last_t = tn;
            if (!is_last) {
                la[0] = samples[si + 1]; la[1] = samples[si + 2]; la[2] = samples[si + 3];
                lg[0] = samples[si + 4]; lg[1] = samples[si + 5]; lg[2] = samples[si + 6];
            }
        }
    }
    if (on) imu_write_rows((size_t)m, c, X, Jc, Pc, Dt, Xout, Jout, Pout, Dtout);
}

// right-looking Cholesky + forward substitution, column-per-lane (same routine as k_lm.hip's fused_chol_solve)
__device__ __forceinline__ void fused_chol15(double (&a)[15]) {
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        const double piv = rdl(a[k], k);
        const double inv = 1.0 / sqrt(piv);
        const double wk = a[k] * inv;
        a[k] = wk;
#pragma unroll
        for (int r = k + 1; r < 15; ++r) a[r] -= rdl(wk, r) * wk;
    }
}

__global__ __launch_bounds__(64) void k_preint_imu_sqrt(int M, const double* P, double* sqrtP, const unsigned char* mask) {
    __shared__ double W[256];
    const int m = blockIdx.x, lane = threadIdx.x & 63;
    if (m >= M || (mask && !mask[m])) return;   // mask [M] (nullptr = all): no row of a masked-out interval is written
    for (int e = lane; e < 256; e += 64) W[e] = 0.0;
    __syncthreads();
    double col[15];
#pragma unroll
    for (int r = 0; r < 15; ++r) {
        double v = 0.0;
        if (lane < 15) v = P[(size_t)m * 225 + r * 15 + lane];
        else if (lane >= 16 && lane < 31) v = (r == lane - 16) ? 1.0 : 0.0;     // identity right-hand sides
        col[r] = v;
    }
    fused_chol15(col);                       // lanes 16..30: columns of L^-1
    if (lane >= 16 && lane < 31) {
#pragma unroll
        for (int r = 0; r < 15; ++r) W[r * 16 + (lane - 16)] = col[r];
    }
    __syncthreads();
    // P^-1 = L^-T L^-1 = W^T W  (fp64 MFMA 16x16x4, operand = W[k][i])
    d4p acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const int k = (lane >> 4) + 4 * cc;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(W[k * 16 + (lane & 15)], W[k * 16 + (lane & 15)], acc, 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) W[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];   // W <- P^-1
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 15; ++r) col[r] = lane < 15 ? W[r * 16 + lane] : 0.0;
    fused_chol15(col);                       // lane j: row j of M, P^-1 = M M^T ; sqrt_inverse_P = M^T
    if (lane < 15) {
#pragma unroll
        for (int k = 0; k < 15; ++k) sqrtP[(size_t)m * 225 + k * 15 + lane] = k <= lane ? col[k] : 0.0;   // U[k][j] = M[j][k]
    }
}

// wheel_odom_preintegration replay, one thread per interval (samples: t, R(9 row-major), t(3))
__global__ __launch_bounds__(128) void k_preint_wheel(int M, const int* sample_off, const double* samples, const double* t_start, const double* t_end,
                               PreintNoise N, double* T12, double* sq9, double* Dtout) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int s0 = sample_off[m], s1 = sample_off[m + 1];
    WheelAcc A;
    wheel_set_identity(A.delta);
    A.last_pose = A.delta;
    A.last_update = -1.0; A.last_add = 0.0; A.Dt = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) A.v[k] = A.om[k] = 0.0;
    bool did_reset = false;
    const double ts = t_start[m], te = t_end[m];
    for (int s = s0; s < s1; ++s) {
        const double* q = samples + (size_t)s * 13;
        if (!did_reset && q[0] > ts) {
            if (A.last_update >= 0) wheel_update_by_v(A, ts - A.last_update);
            wheel_reset(A, ts);
            did_reset = true;
        }
        wheel_add(A, q);
    }
    if (!did_reset) { if (A.last_update >= 0) wheel_update_by_v(A, ts - A.last_update); wheel_reset(A, ts); }
    if (A.last_update >= 0) { wheel_update_by_v(A, te - A.last_update); A.last_update = te; }
    wheel_write_rows((size_t)m, A, N, T12, sq9, Dtout);
}

void launch_preint_imu(int M, const int* sample_off, const double* samples, const double* t_start, const double* t_end, const double* bias6,
                       const PreintNoise& N, double* X, double* J, double* Pscratch, double* sqrtP, double* Dt, hipStream_t s) {
    hipLaunchKernelGGL(k_preint_imu, dim3((M + 3) / 4), dim3(64), 0, s, M, sample_off, samples, t_start, t_end, bias6, N, X, J, Pscratch, Dt);
    launch_preint_imu_sqrt(M, Pscratch, sqrtP, nullptr, s);
}
void launch_preint_imu_sqrt(int M, const double* P, double* sqrtP, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_preint_imu_sqrt, dim3(M), dim3(64), 0, s, M, P, sqrtP, mask);
}
void launch_preint_wheel(int M, const int* sample_off, const double* samples, const double* t_start, const double* t_end,
                         const PreintNoise& N, double* T12, double* sq9, double* Dt, hipStream_t s) {
    hipLaunchKernelGGL(k_preint_wheel, dim3((M + 127) / 128), dim3(128), 0, s, M, sample_off, samples, t_start, t_end, N, T12, sq9, Dt);
}

}  // namespace liw
