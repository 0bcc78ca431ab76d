// k_preint_dev.hpp — device bodies of the pre-integration accumulators, shared by the batch-replay kernels (k_preint.hip: closed,
// independent intervals) and the fleet's persistent accumulators (k_preint_batch.hip: one resumable accumulator pair per robot), so
// that both run the same instructions per IMU sample and per wheel message:
//   imu_step            imu_preintegraption::update(dt) (src/factor/imu_preintegraption.h:170-208) for 16 lanes of one accumulator,
//                       lane c owning column c of J and of P; one 15x15 transpose through LDS per step
//   WheelAcc, wheel_*   wheel_odom_preintegration (src/factor/wheel_odom_preintegration.h:62-152): add_wheel_odom_measure,
//                       update_by_v and the result (delta_Tij, sqrt information), a lane per accumulator
// Same quirks as the reference (SURVEY Appendix C 5,6): the previous sample drives the whole Euler step, F(gamma,gamma) is built from
// hat_gyro - last_ba, P0 = 1e-5 I.
#pragma once
#include "liw_kernels.hpp"

namespace liw {

// rows alpha(0:3) beta(3:6) gamma(6:9) <- F * (old column); ba, bw rows are unchanged.  col = one column (15 rows).
__device__ __forceinline__ void apply_F(double (&col)[15], double dt, const double (&Fbg)[3][3], const double (&Fbb)[3][3], const double (&Fgg)[3][3]) {
    double na[3], nb[3], ng[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        na[i] = col[i] + dt * col[3 + i];
        double sb = col[3 + i], sg = -dt * col[12 + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sb += Fbg[i][k] * col[6 + k] + Fbb[i][k] * col[9 + k];
            sg += Fgg[i][k] * col[6 + k];
        }
        nb[i] = sb; ng[i] = sg;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { col[i] = na[i]; col[3 + i] = nb[i]; col[6 + i] = ng[i]; }
}

// update(dt) with the PREVIOUS sample la / lg (imu_preintegraption.h:170-208).  X is held by every lane of the accumulator's 16,
// Jc / Pc are column c of J / P, Tt the accumulator's 16x16 doubles of LDS.  Every lane of the work-group must call it (it holds two
// barriers).  An accumulator that has nothing to integrate runs the step with dt = 0 and act = false: F = I and the added noise is 0,
// so X, J, P stay bit-identical except gamma (log(exp(gamma)) round trip) and the transpose of P (P is symmetric only up to rounding),
// which are therefore only taken while active: an accumulator's result does not depend on how long its wave's neighbours run.
__device__ __forceinline__ void imu_step(double (&X)[15], double (&Jc)[15], double (&Pc)[15], const double (&la)[3], const double (&lg)[3],
                                         const double dt, const bool act, const PreintNoise& N, double* Tt, const int c) {
    const V3<double> a_unb(la[0] - X[9], la[1] - X[10], la[2] - X[11]);
    const V3<double> w_unb(lg[0] - X[12], lg[1] - X[13], lg[2] - X[14]);
    const M3<double> Rz = exp_so3(V3<double>(X[6], X[7], X[8]));
    const V3<double> Ra = mul(Rz, a_unb);
    const double ra[3] = {Ra.x, Ra.y, Ra.z};
    const double b0[3] = {X[3], X[4], X[5]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        X[k] = X[k] + b0[k] * dt + 0.5 * ra[k] * dt * dt;
        X[3 + k] = b0[k] + ra[k] * dt;
    }
    const V3<double> g2 = log_SO3(mul(Rz, exp_so3(V3<double>(w_unb.x * dt, w_unb.y * dt, w_unb.z * dt))));
    X[6] = act ? g2.x : X[6]; X[7] = act ? g2.y : X[7]; X[8] = act ? g2.z : X[8];
    // F blocks
    double Fbg[3][3], Fbb[3][3], Fgg[3][3];
    {
        const double ax[3] = {a_unb.x, a_unb.y, a_unb.z};
        const double wx[3] = {lg[0] - X[9], lg[1] - X[10], lg[2] - X[11]};   // sic: gyro minus ACC bias (:192)
        // skew(v)[i][j]
        auto sk = [](const double* v, int i, int j) {
            if (i == j) return 0.0;
            if (i == 0 && j == 1) return -v[2];
            if (i == 1 && j == 0) return v[2];
            if (i == 0 && j == 2) return v[1];
            if (i == 2 && j == 0) return -v[1];
            if (i == 1 && j == 2) return -v[0];
            return v[0];
        };
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double rax = Rz(i, 0) * sk(ax, 0, j) + Rz(i, 1) * sk(ax, 1, j) + Rz(i, 2) * sk(ax, 2, j);
                Fbg[i][j] = -rax * dt;
                Fbb[i][j] = -Rz(i, j) * dt;
                Fgg[i][j] = (i == j ? 1.0 : 0.0) - sk(wx, i, j) * dt;
            }
    }
    // J <- F J ; T = F P (both per column, i.e. per lane)
    apply_F(Jc, dt, Fbg, Fbb, Fgg);
    apply_F(Pc, dt, Fbg, Fbb, Fgg);
    // P' = T F^T = (F T^T)^T, P' symmetric: transpose T through LDS, apply F again
    __syncthreads();
    if (c < 15) {
#pragma unroll
        for (int r = 0; r < 15; ++r) Tt[c * 16 + r] = Pc[r];     // T[r][c] stored as Tt[c][r]
    }
    __syncthreads();
    if (c < 15 && act) {   // an idle accumulator keeps its column: P is symmetric only up to rounding, a transpose would change its bits
#pragma unroll
        for (int r = 0; r < 15; ++r) Pc[r] = Tt[r * 16 + c];     // column c of T^T: T[c][r]
    }
    apply_F(Pc, dt, Fbg, Fbb, Fgg);                               // column c of F T^T = row c of P' = column c of P'
    // + (G dt) Q (G dt)^T : (beta,beta) += dt^2 Rz Q_na Rz^T ; diag gamma / ba / bw += q dt^2   (:195-206)
    const double dt2 = dt * dt;
    if (c >= 3 && c < 6) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += Rz(i, k) * N.q_na[k] * (c == 3 ? Rz(0, k) : (c == 4 ? Rz(1, k) : Rz(2, k)));
            Pc[3 + i] += s * dt2;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (c == 6 + k) Pc[6 + k] += N.q_nw[k] * dt2;
        if (c == 9 + k) Pc[9 + k] += N.q_nba[k] * dt2;
        if (c == 12 + k) Pc[12 + k] += N.q_nbw[k] * dt2;
    }
}

// the rows of the liw_batch layout from the registers of an accumulator's 16 lanes: X [15], J and P [15][15] row-major, Dt
__device__ __forceinline__ void imu_write_rows(const size_t m, const int c, const double (&X)[15], const double (&Jc)[15], const double (&Pc)[15],
                                               const double Dt, double* Xout, double* Jout, double* Pout, double* Dtout) {
    if (c < 15) {
#pragma unroll
        for (int r = 0; r < 15; ++r) { Jout[m * 225 + r * 15 + c] = Jc[r]; Pout[m * 225 + r * 15 + c] = Pc[r]; }
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 15; ++r) Xout[m * 15 + r] = X[r];
            Dtout[m] = Dt;
        }
    }
}

// wheel_odom_preintegration's members
struct WheelAcc {
    Iso<double> delta, last_pose;
    double last_update, last_add, Dt, v[3], om[3];
};

__device__ __forceinline__ void wheel_set_identity(Iso<double>& T) {
#pragma unroll
    for (int k = 0; k < 9; ++k) T.R.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
    T.t = V3<double>(0.0, 0.0, 0.0);
}

__device__ __forceinline__ void wheel_update_by_v(WheelAcc& A, const double dt) {
    if (dt <= 0 || dt >= 10) return;   // wheel_odom_preintegration.h:143-147
    A.Dt += dt;
    Iso<double> dT = make_tf(V3<double>(A.v[0] * dt, A.v[1] * dt, A.v[2] * dt), V3<double>(A.om[0] * dt, A.om[1] * dt, A.om[2] * dt));
    A.delta = mul(A.delta, dT);
}

__device__ __forceinline__ void wheel_reset(WheelAcc& A, const double t) { A.last_update = t; wheel_set_identity(A.delta); A.Dt = 0.0; }

// add_wheel_odom_measure of the message q = (t, R 9 row-major, t 3); true when it passed the 0.05 s gate and was integrated
__device__ __forceinline__ bool wheel_add(WheelAcc& A, const double* q) {
    Iso<double> pose = cast_iso<double>(q + 1, q + 10);
    if (A.last_update < 0) {   // :65-75
        A.last_pose = pose; A.last_add = q[0]; A.last_update = q[0];
        wheel_set_identity(A.delta);
#pragma unroll
        for (int k = 0; k < 3; ++k) A.v[k] = A.om[k] = 0.0;
        return false;
    }
    const double dt = q[0] - A.last_add;
    Iso<double> rel = mul(inverse(A.last_pose), pose);
    const V3<double> dth = log_SO3(rel.R);
    if (dt < 0.05) return false;
    A.v[0] = rel.t.x / dt; A.v[1] = rel.t.y / dt; A.v[2] = rel.t.z / dt;
    A.om[0] = dth.x / dt; A.om[1] = dth.y / dt; A.om[2] = dth.z / dt;
    wheel_update_by_v(A, q[0] - A.last_update);
    A.last_pose = pose; A.last_add = q[0]; A.last_update = q[0];
    return true;
}

// get_preintegraption_result: delta_Tij (R row-major 9, t), the diagonal sqrt information and Dt as row m of the liw_batch layout
__device__ __forceinline__ void wheel_write_rows(const size_t m, const WheelAcc& A, const PreintNoise& N, double* T12, double* sq9, double* Dtout) {
    const V3<double> dq = log_SO3(A.delta.R);
    const double len_norm = fmax(A.delta.t.x * A.delta.t.x + A.delta.t.y * A.delta.t.y + A.delta.t.z * A.delta.t.z, 0.005 * 0.005);
    const double yaw_norm = fmax(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z, 0.005 * 0.005);
    const double kd[3] = {len_norm, len_norm, yaw_norm};
#pragma unroll
    for (int k = 0; k < 9; ++k) { sq9[m * 9 + k] = 0.0; T12[m * 12 + k] = A.delta.R.m[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) sq9[m * 9 + k * 4] = sqrt(1.0 / (N.wheel_cov[k] * kd[k]));
    T12[m * 12 + 9] = A.delta.t.x; T12[m * 12 + 10] = A.delta.t.y; T12[m * 12 + 11] = A.delta.t.z;
    Dtout[m] = A.Dt;
}

}  // namespace liw
