// k_posegraph_lm_dev.hpp — what the device pose-graph solvers with their LM bookkeeping on the device share: the fleet back-end
// (k_posegraph_batch.hip), the group graph (k_group_graph.hip) and the joint graph of a group (k_group_joint.hip) include it.
//   - the correctly rounded double CR and the transforms on Iso<CR>, the wave reductions, Plus of the so3 parameterisation, the index of
//     the packed triangle, robot_on / clampi / launched;
//   - pg_reduced_system: the separators' system of a graph of chains (k_fpg_reduced, k_gj_reduced);
//   - the LM loop: PH_*, PgLmCore, the constant-node policies, pg_lm_head / pg_lm_decide1 / pg_lm_decide2, which apply the rules of
//     liw_lm_rules.hpp.  A new graph solver takes its loop from here and supplies the policy, the cost and its finish.
// The Cholesky with both triangular solves behind pg_reduced_system is the text of k_pg_chol_body.inc, which the three kernels
// include: a function call changed k_fpg_reduced's register allocation, a textual include keeps its bytes.
#pragma once
#include "liw_crmath.hpp"
#include "liw_kernels.hpp"
#include "liw_lm_rules.hpp"
#include "k_posegraph_dev.hpp"

namespace liw {

// A double whose sin / cos / atan2 are the correctly rounded ones of liw_crmath.hpp (as the tracking glue's and k_loop_batch.hip's)
struct CR {
    double v;
    __host__ __device__ CR() : v(0.0) {}
    __host__ __device__ CR(double c) : v(c) {}  // NOLINT(implicit)
};
__host__ __device__ inline CR operator+(const CR& a, const CR& b) { return CR(a.v + b.v); }
__host__ __device__ inline CR operator-(const CR& a, const CR& b) { return CR(a.v - b.v); }
__host__ __device__ inline CR operator-(const CR& a) { return CR(-a.v); }
__host__ __device__ inline CR operator*(const CR& a, const CR& b) { return CR(a.v * b.v); }
__host__ __device__ inline CR operator/(const CR& a, const CR& b) { return CR(a.v / b.v); }
__host__ __device__ inline bool operator>(const CR& a, const CR& b) { return a.v > b.v; }
__host__ __device__ inline bool operator<(const CR& a, const CR& b) { return a.v < b.v; }
__host__ __device__ inline CR dsqrt(const CR& a) { return CR(sqrt(a.v)); }
__host__ __device__ inline CR dsin(const CR& a) { return CR(liw_cr::cr_sin(a.v)); }
__host__ __device__ inline CR dcos(const CR& a) { return CR(liw_cr::cr_cos(a.v)); }
__host__ __device__ inline CR datan2(const CR& y, const CR& x) { return CR(liw_cr::cr_atan2(y.v, x.v)); }
__host__ __device__ inline CR dfloor(const CR& a) { return CR(floor(a.v)); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// std::max as the host loop folds it: a NaN operand never replaces the running maximum
__device__ __forceinline__ double max_skip_nan(double m, double v) { return (m < v) ? v : m; }
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max_skip_nan(v, __shfl_xor(v, o, 64));
    return v;
}

// Plus of the so3 parameterisation (factor_common.h:41-53): the rotation vectors add, then wrap
__device__ __forceinline__ void plus6(const double* x, const double* d, double* out) {
    for (int k = 0; k < 3; ++k) out[k] = x[k] + d[k];
    const V3<double> r = normalize_so3(V3<double>(x[3] + d[3], x[4] + d[4], x[5] + d[5]));
    out[3] = r.x; out[4] = r.y; out[5] = r.z;
}

__device__ __forceinline__ size_t tri(int r, int c) { return (size_t)r * (r + 1) / 2 + c; }   // packed lower triangle, c <= r

// ---- small things every solver module had a copy of
__device__ __forceinline__ bool robot_on(const unsigned char* a, int b) { return !a || a[b] != 0; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

__device__ __forceinline__ void store_tf(const Iso<CR>& T, double* tf) {
    for (int k = 0; k < 9; ++k) tf[k] = T.R.m[k].v;
    tf[9] = T.t.x.v; tf[10] = T.t.y.v; tf[11] = T.t.z.v;
}
__device__ __forceinline__ Iso<CR> load_tf(const double* tf) { return cast_iso<CR>(tf, tf + 9); }
__device__ __forceinline__ Iso<CR> tf_of_pose(const double* ps) { return make_tf(V3<CR>(ps[0], ps[1], ps[2]), V3<CR>(ps[3], ps[4], ps[5])); }
// log_SE3: p = t, q = log_SO3(R)
__device__ __forceinline__ void pose_of_tf(const Iso<CR>& T, double* ps) {
    const V3<CR> q = log_SO3(T.R);
    ps[0] = T.t.x.v; ps[1] = T.t.y.v; ps[2] = T.t.z.v; ps[3] = q.x.v; ps[4] = q.y.v; ps[5] = q.z.v;
}

// ------------------------------------------------------------------------------------------------------------- the separators' system
// All 256 threads of a work-group build A y = g_s of the ns separators (packed lower triangle A of order 6 ns, rhs) as k_pg_reduced +
// k_pg_reduced_loops of k_posegraph.hip do: a wave per separator takes the diagonal block, the block to the separator on its left and
// the gradient from the node's own blocks and the Schur terms of the segments beside it; then ONE wave adds the loop blocks in list
// order (several edges may share a block).  nmem names the chain of every node: two consecutive separators of different chains have
// neither a segment nor a block between them; null: the nodes are one chain.  cn is the constant node.  Ends behind a barrier.
__device__ __forceinline__ void pg_reduced_system(double* A, double* rhs, int ns, int nl, int cn, const int* sep, const int* sepidx, const int* lidx,
                                                  const int* nmem, const double* Dd, const double* gd, const double* Os, const double* Lb,
                                                  const double* Sred, const double* scale, const double* dgn, double radius, int tid) {
    const int lane = tid & 63, wave = tid >> 6, r = lane / 6, c = lane % 6;
    const int nr = 6 * ns, tri_n = nr * (nr + 1) / 2;
    for (int e = tid; e < tri_n; e += 256) A[e] = 0.0;
    __syncthreads();
    for (int t = wave; t < ns; t += 4) {
        const int f = sep[t];
        const double* sf = scale + (size_t)f * 6;
        const bool is_const = f == cn;
        // neighbours in the same chain; segments with interior nodes
        const bool lchain = t > 0 && (!nmem || nmem[sep[t - 1]] == nmem[f]), rchain = t + 1 < ns && (!nmem || nmem[sep[t + 1]] == nmem[f]);
        const bool left = lchain && sep[t] - sep[t - 1] > 1, right = rchain && sep[t + 1] - sep[t] > 1;
        if (lane < 36) {
            double v = is_const ? (r == c ? 1.0 : 0.0) : Dd[(size_t)f * 36 + lane] * sf[r] * sf[c] + (r == c ? dgn[(size_t)f * 6 + c] / radius : 0.0);
            if (!is_const) {
                if (right) v += Sred[(size_t)t * PG_SEG + lane];
                if (left) v += Sred[(size_t)(t - 1) * PG_SEG + 72 + lane];
            }
            if (r >= c) A[tri(t * 6 + r, t * 6 + c)] = v;
            if (lchain) {   // block (t, t-1): direct edge when the separators are chain neighbours, else the segment's fill; none across chains
                const int fa = sep[t - 1];
                const double o = left ? Sred[(size_t)(t - 1) * PG_SEG + 36 + lane] : Os[(size_t)fa * 36 + c * 6 + r] * scale[(size_t)fa * 6 + c] * sf[r];
                A[tri(t * 6 + r, (t - 1) * 6 + c)] = (is_const || fa == cn) ? 0.0 : o;
            }
        } else if (lane < 42) {
            const int k = lane - 36;
            double v = is_const ? 0.0 : gd[(size_t)f * 6 + k] * sf[k];
            if (!is_const) {
                if (right) v += Sred[(size_t)t * PG_SEG + 108 + k];
                if (left) v += Sred[(size_t)(t - 1) * PG_SEG + 114 + k];
            }
            rhs[t * 6 + k] = v;
        }
    }
    __syncthreads();
    if (wave == 0 && lane < 36)
        for (int e = 0; e < nl; ++e) {
            const int i1 = lidx[2 * e], i2 = lidx[2 * e + 1];
            if (i1 == cn || i2 == cn || i1 == i2) continue;
            const int t1 = sepidx[i1], t2 = sepidx[i2];
            const double v = Lb[(size_t)e * 36 + lane] * scale[(size_t)i1 * 6 + r] * scale[(size_t)i2 * 6 + c];   // H[i1, i2](r, c)
            if (t1 > t2) A[tri(t1 * 6 + r, t2 * 6 + c)] += v;
            else A[tri(t2 * 6 + c, t1 * 6 + r)] += v;
        }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------- the LM loop
// One wave keeps the trust-region state of a graph and takes its decisions in three places of an iteration: pg_lm_head in front of the
// linear solve, pg_lm_decide1 behind it, pg_lm_decide2 behind the candidate's residuals.  The three work on a local copy of the state
// and on the graph's arrays (6 doubles per node) and RETURN what they decided.  What a module supplies: the policy that names its
// constant nodes, its cost, and, around the call, its early-outs, its finish and the single write-back of the state by lane 0.
enum { PH_IDLE = 0, PH_SOLVE = 1, PH_CAND = 2, PH_ASM = 3, PH_INIT = 4 };
// The head of every module's LM state; a module's Lm derives from it and adds its own integers.
struct PgLmCore {
    double radius, dec, x_cost, x_norm, gmax, mcc, init_cost, step_norm;
    int iter, invalid, succ, last_ok, term, reuse, done, phase;
};
__device__ __forceinline__ void pg_lm_start(PgLmCore& s, int done) {
    s.radius = kInitRadius; s.dec = 2.0; s.x_cost = 0.0; s.x_norm = 0.0; s.gmax = 0.0; s.mcc = 0.0; s.init_cost = 0.0; s.step_norm = 0.0;
    s.iter = 0; s.invalid = 0; s.succ = 0; s.last_ok = 1; s.term = 0; s.reuse = 0; s.done = done; s.phase = PH_INIT;
}

// Constant-node policies.  A wave's strided loops start at node `first` and skip the nodes that is_const names; the sums are not
// associative, so which of the two a module uses fixes every lane's index set and order, and the results with them.
struct PgConstFirst {   // node 0 is the constant one: the loops start behind it and test nothing
    static constexpr int first = 1;
    __device__ __forceinline__ bool is_const(int) const { return false; }
};
struct PgConstNode {    // one node, anywhere
    int cn;
    static constexpr int first = 0;
    __device__ __forceinline__ bool is_const(int f) const { return f == cn; }
};
struct PgConstFlags {   // a flag per node
    const int* cst;
    static constexpr int first = 0;
    __device__ __forceinline__ bool is_const(int f) const { return cst[f] != 0; }
};
template <class Pol> __device__ __forceinline__ bool pg_held(const Pol& pol, int f) { return f < Pol::first || pol.is_const(f); }

// cost / norms of a new point, termination 1 / 4 / 5, the LM diagonal.  cost() is called for a graph in PH_INIT only.  Returns the
// termination code, or 0 with the state in PH_SOLVE.
template <class Pol, class Cost>
__device__ __forceinline__ int pg_lm_head(PgLmCore& s, const Pol& pol, Cost cost, int N, int max_iters, const double* x, const double* gd, const double* Dd,
                                          double* scale, double* dgn, int lane) {
    const int n = 6 * N;
    if (s.phase == PH_INIT) {
        s.x_cost = cost();
        s.init_cost = s.x_cost;
        for (int i = lane; i < n; i += 64) scale[i] = pg_held(pol, i / 6) ? 1.0 : 1.0 / (1.0 + sqrt(Dd[(size_t)(i / 6) * 36 + (i % 6) * 7]));
    }
    if (s.phase == PH_INIT || s.phase == PH_ASM) {
        double sq = 0.0, m = 0.0;
        for (int i = 6 * Pol::first + lane; i < n; i += 64)
            if (!pol.is_const(i / 6)) sq += x[i] * x[i];
        s.x_norm = sqrt(wave_sum(sq));
        for (int f = Pol::first + lane; f < N; f += 64) {   // max |x - Plus(x, -g)|
            if (pol.is_const(f)) continue;
            double ng[6], xp[6];
            for (int k = 0; k < 6; ++k) ng[k] = -gd[f * 6 + k];
            plus6(x + (size_t)f * 6, ng, xp);
            for (int k = 0; k < 6; ++k) m = max_skip_nan(m, fabs(x[f * 6 + k] - xp[k]));
        }
        s.gmax = wave_max(m);
    }
    if (lm_cap_reached(s.iter, max_iters, s.phase == PH_INIT)) return 4;
    const int term = lm_gradient_term(s.iter == 0, s.last_ok != 0, s.gmax, s.radius > kMinRadius);
    if (term) return term;
    ++s.iter;
    if (!s.reuse)
        for (int i = lane; i < n; i += 64) {
            const double sc = scale[i];
            double v = Dd[(size_t)(i / 6) * 36 + (i % 6) * 7] * sc * sc;   // clamped as std::min(std::max(v, lo), hi) does: a NaN stays
            v = (v < kMinDiag) ? kMinDiag : v;
            v = (kMaxDiag < v) ? kMaxDiag : v;
            dgn[i] = pg_held(pol, i / 6) ? 0.0 : v;
        }
    s.reuse = 1;
    s.phase = PH_SOLVE;
    return 0;
}

// step validity, model cost change, Plus into the candidate, step norm.  factored: no pivot of the linear solve was refused.  Returns
// termination 6 (the iteration count already taken back), PG_LM_REJECTED with the state in PH_IDLE, or 0 with the candidate ready
// and the state in PH_CAND.
constexpr int PG_LM_REJECTED = -1;
template <class Pol>
__device__ __forceinline__ int pg_lm_decide1(PgLmCore& s, const Pol& pol, bool factored, int N, const double* x, double* cand, const double* y,
                                             const double* scale, const double* dgn, const double* gd, int lane) {
    const int n = 6 * N;
    bool fin = true;
    for (int i = lane; i < n; i += 64) fin = fin && isfinite(y[i]);
    const bool solved = factored && __ballot(!fin) == 0ull;
    // model cost change with (A + D^2) y = g_s, step = -y:  (y'g_s + y'D^2 y) / 2
    double mcc = 0.0;
    if (solved) {
        double ytg = 0.0, dsum = 0.0;
        for (int i = 6 * Pol::first + lane; i < n; i += 64) {
            if (pol.is_const(i / 6)) continue;
            const double yi = y[i];
            ytg += yi * (gd[i] * scale[i]);
            dsum += dgn[i] / s.radius * yi * yi;
        }
        mcc = 0.5 * (wave_sum(ytg) + wave_sum(dsum));
    }
    if (!lm_step_valid(solved, mcc)) {
        if (lm_gives_up(s.invalid++)) {
            --s.iter;
            return 6;
        }
        lm_step_rejected(s.radius, s.dec, s.reuse);
        s.last_ok = 0;
        s.phase = PH_IDLE;
        return PG_LM_REJECTED;
    }
    s.invalid = 0;
    s.mcc = mcc;
    double sq = 0.0;
    for (int f = Pol::first + lane; f < N; f += 64) {
        if (pol.is_const(f)) continue;
        double dl[6], xc[6];
        for (int k = 0; k < 6; ++k) dl[k] = -y[f * 6 + k] * scale[f * 6 + k];
        plus6(x + (size_t)f * 6, dl, xc);
        for (int k = 0; k < 6; ++k) {
            cand[f * 6 + k] = xc[k];
            const double df = x[f * 6 + k] - xc[k];
            sq += df * df;
        }
    }
    s.step_norm = sqrt(wave_sum(sq));
    s.phase = PH_CAND;
    return 0;
}

// the candidate's cost cc: termination 2 / 3 (returned, the state untouched), else rho, accept (x <- candidate, PH_ASM) or reject
// (PH_IDLE), the radius; returns 0
__device__ __forceinline__ int pg_lm_decide2(PgLmCore& s, double cc, int N, double* x, const double* cand, int lane) {
    if (!isfinite(cc)) cc = kFailedEvalCost;
    const int term = lm_candidate_term(s.step_norm, s.x_norm, s.x_cost, cc);
    if (term) return term;
    const double rho = (s.x_cost - cc) / s.mcc;
    if (lm_accepts(rho)) {
        for (int i = lane; i < 6 * N; i += 64) x[i] = cand[i];
        s.x_cost = cc;
        lm_step_accepted(rho, s.radius, s.dec, s.reuse);
        ++s.succ;
        s.last_ok = 1;
        s.phase = PH_ASM;
    } else {
        lm_step_rejected(s.radius, s.dec, s.reuse);
        s.last_ok = 0;
        s.phase = PH_IDLE;
    }
    return 0;
}

}  // namespace liw
