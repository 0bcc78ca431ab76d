// k_posegraph_dev.hpp — the per-edge, per-key-frame and per-segment device code of the pose graph, shared by the single-graph solver
// (k_posegraph.hip), the fleet solver (k_posegraph_batch.hip), the group graph (k_group_graph.hip) and the joint graph of a group
// (k_group_joint.hip): edge_factor / ground_factor residuals, the so3 Plus Jacobian, what a lane of a linearisation or assembly block
// does (pg_edge_column, pg_ground_column, pg_row_times_plus_jac, pg_node_ground / pg_node_edge / pg_edge_cross), and the
// wave-per-segment chain elimination and back-substitution: the bodies of k_pg_seg_elim / k_pg_seg_backsub with the segment's arrays as
// arguments, so all solvers run the same instructions.
#pragma once
#include "liw_kernels.hpp"

namespace liw {

constexpr double kPiG = 3.141592653589793238462643383279, kTwoPiG = 6.283185307179586476925286766559;

struct PgNoise { double J[36]; double ground_on_p, ground_on_q; };

__device__ __forceinline__ double rdl64(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}
// d Plus(x, delta) / d delta at delta = 0 of the so3 parameterisation (src/factor/factor_common.h:37-60): identity unless |x| > pi
__device__ __forceinline__ bool plus_jac(const double* x, double* P9) {
    const double a = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(a > kPiG)) return false;
    const double k = floor((a + kPiG) / kTwoPiG);
    const double c = kTwoPiG * k / a;
    const double u[3] = {x[0] / a, x[1] / a, x[2] / a};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P9[i * 3 + j] = (i == j ? 1.0 : 0.0) - c * ((i == j ? 1.0 : 0.0) - u[i] * u[j]);
    return true;
}

// ---- edge_factor::operator() (edge_factor.h:88-117): res = weight * J_noise * log_SE3(tf_j^-1 tf_i tf12)
template <class T>
__device__ __forceinline__ void edge_res(const double* tf12, double weight, const double* Jn, const T* pi, const T* qi, const T* pj, const T* qj, T* res) {
    Iso<T> tf_i = make_tf(V3<T>(pi[0], pi[1], pi[2]), V3<T>(qi[0], qi[1], qi[2]));
    Iso<T> tf_j = make_tf(V3<T>(pj[0], pj[1], pj[2]), V3<T>(qj[0], qj[1], qj[2]));
    Iso<T> err = mul(mul(inverse(tf_j), tf_i), cast_iso<T>(tf12, tf12 + 9));
    V3<T> rq = log_SO3(err.R);
    T raw[6] = {err.t.x, err.t.y, err.t.z, rq.x, rq.y, rq.z};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        T s(0.0);
#pragma unroll
        for (int c = 0; c < 6; ++c) s = s + T(Jn[r * 6 + c]) * raw[c];
        res[r] = T(weight) * s;
    }
}
template <class T>
__device__ __forceinline__ void pg_ground_res(const DevParams& P, const T* p_, const T* q_, T* res) {   // ground_factor.h:27-82
    Iso<T> tf_w_o = mul(make_tf(V3<T>(p_[0], p_[1], p_[2]), V3<T>(q_[0], q_[1], q_[2])), cast_iso<T>(P.Riw, P.tiw));
    res[0] = T(P.ground_p_info) * tf_w_o.t.z;
    V3<T> ABC(T(0.0), T(0.0), T(1.0));
    V3<T> z_axis(tf_w_o.R(0, 2), tf_w_o.R(1, 2), tf_w_o.R(2, 2));
    T sinn = norm(cross(z_axis, ABC));
    res[1] = T(P.ground_q_info) * dasin(sinn);
}

// ---- the lanes of a block.  A kernel keeps its slot arithmetic, its phase tests, its barriers and its stores; these are what a lane does.
// local parameterisation of three rotation columns of a Jacobian row: row <- row * dPlus/ddelta at the rotation vector q
__device__ __forceinline__ void pg_row_times_plus_jac(double* row, const double* q) {
    double Pq[9];
    if (plus_jac(q, Pq)) {
        const double t0 = row[0] * Pq[0] + row[1] * Pq[3] + row[2] * Pq[6];
        const double t1 = row[0] * Pq[1] + row[1] * Pq[4] + row[2] * Pq[7];
        const double t2 = row[0] * Pq[2] + row[1] * Pq[5] + row[2] * Pq[8];
        row[0] = t0; row[1] = t1; row[2] = t2;
    }
}
// lane d of an edge's sixteen writes column d of Y [6][13] = [J | r]: the dual direction d of (p_i, q_i, p_j, q_j) for d < 12 (only when
// jac), the value for d = 12
__device__ __forceinline__ void pg_edge_column(const double* tf12, double weight, const double* Jn, const double* xi, const double* xj, int d, bool jac,
                                               double* Y) {
    if (!(d == 12 || (jac && d < 12))) return;
    LJ pi[3], qi[3], pj[3], qj[3], res[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pi[k] = LJ(xi[k], d == k ? 1.0 : 0.0);
        qi[k] = LJ(xi[3 + k], d == 3 + k ? 1.0 : 0.0);
        pj[k] = LJ(xj[k], d == 6 + k ? 1.0 : 0.0);
        qj[k] = LJ(xj[3 + k], d == 9 + k ? 1.0 : 0.0);
    }
    edge_res<LJ>(tf12, weight, Jn, pi, qi, pj, qj, res);
#pragma unroll
    for (int r = 0; r < 6; ++r) Y[r * 13 + d] = d < 12 ? res[r].d : res[r].v;
}
// lane dir of a node's eight writes column dir of Yl [2][7] = [J | r] of its ground factor: direction dir < 6 (only when jac), value 6
__device__ __forceinline__ void pg_ground_column(const DevParams& P, double on_p, double on_q, const double* s_, int dir, bool jac, double* Yl) {
    if (!(dir == 6 || (jac && dir < 6))) return;
    LJ p[3], q[3], res[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = LJ(s_[k], dir == k ? 1.0 : 0.0); q[k] = LJ(s_[3 + k], dir == 3 + k ? 1.0 : 0.0); }
    pg_ground_res<LJ>(P, p, q, res);
    Yl[dir] = (dir < 6 ? res[0].d : res[0].v) * on_p;
    Yl[7 + dir] = (dir < 6 ? res[1].d : res[1].v) * on_q;
}
// A wave gathers a node's 6x6 block of J'J (lanes 0..35: entry (lane / 6, lane % 6)) and its J'r (lanes 36..41): what the node's ground
// block Yg [2][7] and side `side` of an incident edge's Y [6][13] add for this lane, and for lanes 0..35 the edge's block H[index1, index2]
__device__ __forceinline__ double pg_node_ground(const double* Yg, int lane) {
    const int r = lane / 6, c = lane % 6;
    if (lane < 36) return Yg[r] * Yg[c] + Yg[7 + r] * Yg[7 + c];
    if (lane < 42) return Yg[lane - 36] * Yg[6] + Yg[7 + (lane - 36)] * Yg[13];
    return 0.0;
}
__device__ __forceinline__ double pg_node_edge(const double* Y, int side, int lane) {
    const int r = lane / 6, c = lane % 6;
    double s = 0.0;
    if (lane < 36) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Y[k * 13 + 6 * side + r] * Y[k * 13 + 6 * side + c];
    } else if (lane < 42) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Y[k * 13 + 6 * side + (lane - 36)] * Y[k * 13 + 12];
    }
    return s;
}
__device__ __forceinline__ double pg_edge_cross(const double* Y, int lane) {   // sum_k J1[k][r] J2[k][c]
    const int r = lane / 6, c = lane % 6;
    double o = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) o += Y[k * 13 + r] * Y[k * 13 + 6 + c];
    return o;
}

// every PG_STRIDE-th key frame of the chain is a separator (k_posegraph.hip, "sparse path")
constexpr int PG_STRIDE = 48;
// Schur terms of one segment (doubles): aa[36] (on H[a,a]), ba[36] (H[b,a], rows b), bb[36], ga[6], gb[6]
constexpr int PG_SEG = 36 * 3 + 12;

// One wave eliminates the interior frames a+1 .. b-1 of a segment in chain order; returns false when a pivot is not positive and finite.
__device__ __forceinline__ bool pg_seg_elim_wave(int a, int b, int lane, const double* Dd, const double* gd, const double* Os, const double* scale,
                                                 const double* dgn, double radius, double* out, double* rec) {
    // lane roles: j < 6 column j of the pivot block, 6..11 columns of H[f, f+1], 12..17 columns of H[f, a], 18 the gradient
    const int role = lane < 6 ? 0 : (lane < 12 ? 1 : (lane < 18 ? 2 : (lane == 18 ? 3 : 4)));
    const int cj = lane < 18 ? lane % 6 : 0;
    double cD[6] = {0, 0, 0, 0, 0, 0}, cB[6] = {0, 0, 0, 0, 0, 0}, cg[6] = {0, 0, 0, 0, 0, 0}, aAA[6] = {0, 0, 0, 0, 0, 0}, aGa[6] = {0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (int f = a + 1; f < b; ++f) {
        const double* sf = scale + (size_t)f * 6;
        double col[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = 0.0;
            if (role == 0) v = Dd[(size_t)f * 36 + r * 6 + cj] * sf[r] * sf[cj] + cD[r] + (r == cj ? dgn[(size_t)f * 6 + cj] / radius : 0.0);
            else if (role == 1) v = Os[(size_t)f * 36 + r * 6 + cj] * sf[r] * scale[(size_t)(f + 1) * 6 + cj];
            else if (role == 2) v = (f == a + 1 ? Os[(size_t)a * 36 + cj * 6 + r] * scale[(size_t)a * 6 + cj] * sf[r] : 0.0) + cB[r];
            else if (role == 3) v = gd[(size_t)f * 6 + r] * sf[r] + cg[r];
            col[r] = v;
        }
        // right-looking Cholesky of the 6x6 pivot fused with the forward substitution of the other columns
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double piv = rdl64(col[k], k);
            if (!(piv > 0.0) || !isfinite(piv)) ok = false;
            const double wk = col[k] * rsqrt(piv);
            col[k] = wk;
#pragma unroll
            for (int r = k + 1; r < 6; ++r) col[r] -= rdl64(wk, r) * wk;
        }
        // record [Yo | Yb | yz] = L^-T [Wo | Wb | z]: y_f = yz - Yo y_{f+1} - Yb y_a
        {
            double xs[6];
#pragma unroll
            for (int k = 5; k >= 0; --k) {
                double t = col[k];
#pragma unroll
                for (int r = k + 1; r < 6; ++r) t -= rdl64(col[k], r) * xs[r];      // L[r][k] lives in lane r, register k
                xs[k] = t / rdl64(col[k], k);
            }
            if (lane >= 6 && lane < 19) {
#pragma unroll
                for (int k = 0; k < 6; ++k) rec[(size_t)f * 78 + k * 13 + (lane - 6)] = xs[k];
            }
        }
        // Schur terms: P(p, own) = W_p . W_own for the columns p of [Wo | Wb]
        double P[12];
#pragma unroll
        for (int p_ = 0; p_ < 12; ++p_) {
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) d += rdl64(col[k], 6 + p_) * col[k];
            P[p_] = d;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double fromO = __shfl(P[q], (lane + 6) & 63, 64);   // lane j < 6 <- P(Wo_q, Wo_j) held by lane 6 + j
            if (role == 0) cD[q] = -fromO;
            if (role == 2) { cB[q] = -P[q]; aAA[q] -= P[6 + q]; }
            if (role == 3) { cg[q] = -P[q]; aGa[q] -= P[6 + q]; }
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (role == 0) out[72 + r * 6 + cj] = cD[r];                                 // bb
        if (role == 2) { out[36 + r * 6 + cj] = cB[r]; out[r * 6 + cj] = aAA[r]; }   // ba (rows b), aa
        if (role == 3) { out[108 + r] = aGa[r]; out[114 + r] = cg[r]; }              // ga, gb
    }
    return ok;
}

// One wave recovers the interior frames b-1 .. a+1 of a segment from y[a], y[b] and the records of pg_seg_elim_wave.
__device__ __forceinline__ void pg_seg_backsub_wave(int a, int b, int lane, const double* rec, double* y) {
    const int k = lane < 6 ? lane : 0;
    double ya[6], yn[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { ya[q] = y[(size_t)a * 6 + q]; yn[q] = y[(size_t)b * 6 + q]; }
    for (int f = b - 1; f > a; --f) {
        const double* R = rec + (size_t)f * 78 + k * 13;
        double t = R[12];
#pragma unroll
        for (int q = 0; q < 6; ++q) t -= R[q] * yn[q] + R[6 + q] * ya[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) yn[q] = rdl64(t, q);
        if (lane < 6) y[(size_t)f * 6 + lane] = t;
    }
}

}  // namespace liw
