// k_group_graph.hip — the group pose graph of the fleet on the MI355X (C ABI include/liw_group_graph.h, host side
// liw_group_graph.cpp): the cross edges of a group are kept, and T_g_w of its linked robots is refined from all of them and from the
// back-end's current corrected poses.
//   k_ggraph_reset      a work-group per group: header and edge records cleared.
//   k_ggraph_add_edges  a wave per group walks the fleet 64 robots at a time: the checks, the duplicate scan of the held list by the
//                       lanes, the position by ballot and prefix count in robot order.
//   k_ggraph_partner    a wave per robot counts and picks the other linked members of its group with ballots (k_xloop_partner's
//                       body with the robot itself left out, which changes nothing for an unlinked robot).
//   k_ggraph_solve      a work-group per group runs the WHOLE Levenberg-Marquardt loop in one launch: node list by ballots, Z per
//                       edge, then per iteration what k_posegraph_batch.hip spreads over eight launches: 16 lanes per edge with a
//                       dual direction per lane (edge_res / plus_jac of k_posegraph_dev.hpp), a wave per node gathers its blocks in
//                       edge order, the packed triangle (LDS when it fits, else the work area: the same instructions on another
//                       pointer), right-looking Cholesky and both triangular solves, and wave 0 takes the decisions of
//                       liw_lm_rules.hpp.  A group is small (a few dozen nodes), so the loop is bound by latency, not by width.
//   k_ggate             (include/liw_group_gate.h) a work-group per group: the squared residual of every used edge at the last solve's
//                       x, the edges of a robot pair counted as each other's support, a fixed-order block arg-max, one edge retired.
// No atomics.  Every sum runs in an order fixed by the group's own graph: results are reproducible bit for bit.
#pragma clang fp contract(off)   // Z is liw_lie_mul's product bit for bit

#include <hip/hip_runtime.h>

#include "k_group_graph.hpp"
#include "k_posegraph_dev.hpp"
#include "k_posegraph_lm_dev.hpp"
#include "liw_dual.hpp"
#include "liw_lm_rules.hpp"

namespace liw_ggraph_dev {

using namespace liw;

using IsoD = Iso<double>;

// LM state of a group (head of its work area)
struct Lm : PgLmCore { int N, ne, used, anyfixed; };
static_assert(sizeof(Lm) <= 256, "the LM state has 256 bytes");

struct Wk {   // a group's work area
    Lm* lm; int *nodes, *cst, *enode; double *x, *cand, *y, *scale, *dgn, *gd, *Dd, *Ye, *Z, *Hr, *rhs;
};
__device__ __forceinline__ char* region(char* store, const Lay& L, int g) { return store + (size_t)g * L.group_bytes; }
__device__ __forceinline__ Wk work_of(char* store, const Lay& L, int g) {
    char* W = store + L.work_off + (size_t)g * L.work_group_bytes;
    Wk w;
    w.lm = (Lm*)W;
    w.nodes = (int*)(W + L.w_nodes); w.cst = (int*)(W + L.w_const); w.enode = (int*)(W + L.w_enode);
    w.x = (double*)(W + L.w_x); w.cand = (double*)(W + L.w_cand); w.y = (double*)(W + L.w_y); w.scale = (double*)(W + L.w_scale);
    w.dgn = (double*)(W + L.w_dgn); w.gd = (double*)(W + L.w_gd); w.Dd = (double*)(W + L.w_Dd); w.Ye = (double*)(W + L.w_Ye);
    w.Z = (double*)(W + L.w_Z); w.Hr = (double*)(W + L.w_Hr); w.rhs = (double*)(W + L.w_rhs);
    return w;
}

// plain-double transforms: the products below are liw_lie_mul's, so these do not go through Iso<CR> as liw::tf_of_pose / pose_of_tf do
__device__ __forceinline__ IsoD load_iso(const double* T) { return cast_iso<double>(T, T + 9); }
__device__ __forceinline__ void store_iso(const IsoD& A, double* T) {
    for (int k = 0; k < 9; ++k) T[k] = A.R.m[k];
    T[9] = A.t.x; T[10] = A.t.y; T[11] = A.t.z;
}
__device__ __forceinline__ IsoD tf_of_pose(const double* ps) {   // make_tf with the correctly rounded sin / cos
    const Iso<CR> T = make_tf(V3<CR>(ps[0], ps[1], ps[2]), V3<CR>(ps[3], ps[4], ps[5]));
    IsoD o;
    for (int k = 0; k < 9; ++k) o.R.m[k] = T.R.m[k].v;
    o.t = V3<double>(T.t.x.v, T.t.y.v, T.t.z.v);
    return o;
}
__device__ __forceinline__ void pose_of_tf(const double* tf, double* ps) {   // log_SE3: p = t, q = log_SO3(R)
    const V3<CR> q = log_SO3(cast_iso<CR>(tf, tf + 9).R);
    ps[0] = tf[9]; ps[1] = tf[10]; ps[2] = tf[11]; ps[3] = q.x.v; ps[4] = q.y.v; ps[5] = q.z.v;
}


// ------------------------------------------------------------------------------------------------------------- the edge lists
__global__ __launch_bounds__(256) void k_ggraph_reset(char* store, Lay L, const unsigned char* __restrict__ gmask) {
    const int g = blockIdx.x;
    if (!robot_on(gmask, g)) return;
    int* R = (int*)region(store, L, g);
    const size_t words = L.group_bytes / 4;
    for (size_t k = threadIdx.x; k < words; k += 256) R[k] = 0;
}

__global__ __launch_bounds__(64) void k_ggraph_add_edges(char* store, Lay L, const int* __restrict__ group_of, const unsigned char* __restrict__ found,
                                                         const int* __restrict__ edge, const double* __restrict__ tf12, const unsigned char* __restrict__ mask) {
    const int g = blockIdx.x, lane = threadIdx.x;
    char* R = region(store, L, g);
    int* hdr = (int*)R;
    const int n0 = min(max(hdr[H_NE], 0), L.E);   // held before this call: a robot is walked once, so a duplicate can only be among these
    int n = n0;
    bool bad_any = false, full_any = false;
    for (int a0 = 0; a0 < L.B; a0 += 64) {
        const int a = a0 + lane;
        const bool cand = a < L.B && robot_on(mask, a) && found[a] != 0 && group_of[a] == g;
        int q = 0, b = 0, i = 0, size = 0;
        if (cand) { q = edge[(size_t)a * 4]; b = edge[(size_t)a * 4 + 1]; i = edge[(size_t)a * 4 + 2]; size = edge[(size_t)a * 4 + 3]; }
        const bool bad = cand && (b < 0 || b >= L.B || b == a || group_of[b] != g);
        bool keep = cand && !bad;
        if (keep)
            for (int e = 0; e < n0; ++e) {
                const int* rec = (const int*)(R + kHeaderBytes + (size_t)e * kEdgeBytes);
                if (rec[0] == a && rec[1] == q && rec[2] == b && rec[3] == i) keep = false;
            }
        const unsigned long long m = __ballot(keep);
        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < L.E) {
            char* rec = R + kHeaderBytes + (size_t)pos * kEdgeBytes;
            int* ri = (int*)rec;
            ri[0] = a; ri[1] = q; ri[2] = b; ri[3] = i; ri[4] = size; ri[5] = 0; ri[6] = 0; ri[7] = 0;
            double* rt = (double*)(rec + kEdgeTf);
            for (int k = 0; k < 12; ++k) rt[k] = tf12[(size_t)a * 12 + k];
        }
        bad_any = bad_any || __ballot(bad) != 0ull;
        full_any = full_any || n + __popcll(m) > L.E;
        n = min(n + __popcll(m), L.E);
    }
    if (lane == 0) {
        if (n != n0) hdr[H_NE] = n;
        if (full_any) hdr[H_EFULL] = 1;
        if (bad_any) hdr[H_BAD] = 1;
    }
}

__global__ __launch_bounds__(64) void k_ggraph_partner(int B, const int* __restrict__ group_of, const unsigned char* __restrict__ linked, int round,
                                                       int* __restrict__ partner) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const int g = group_of[a];
    int pick = -1;
    if (g >= 0) {
        int n = 0;
        for (int m0 = 0; m0 < B; m0 += 64) {
            const int m = m0 + lane;
            n += __popcll(__ballot(m < B && m != a && linked[m] && group_of[m] == g));
        }
        if (n > 0) {
            int want = round % n;    // the want-th other linked member in index order
            for (int m0 = 0; m0 < B && pick < 0; m0 += 64) {
                const int m = m0 + lane;
                unsigned long long bal = __ballot(m < B && m != a && linked[m] && group_of[m] == g);
                const int c = __popcll(bal);
                if (want >= c) { want -= c; continue; }
                for (int k = 0; k < want; ++k) bal &= bal - 1;   // drop the lowest `want` set bits
                pick = m0 + __ffsll(bal) - 1;
            }
        }
    }
    if (lane == 0) partner[a] = pick;
}

// ------------------------------------------------------------------------------------------------------------- the solve

// Y of edge e [6][13] = [J | r] at x (which = 0) or at the candidate; all 256 threads, 16 edges a pass
__device__ __forceinline__ void linearize(const Wk& w, const Noise& noise, int ne, int which, int tid) {
    const int sub = tid >> 4, d = tid & 15;
    const double* x = which ? w.cand : w.x;
    for (int e0 = 0; e0 < ne; e0 += 16) {
        const int e = e0 + sub;
        const bool on = e < ne && w.enode[3 * e + 2] != 0;
        const int i = on ? w.enode[3 * e] : 0, j = on ? w.enode[3 * e + 1] : 0;
        const double* xi = x + (size_t)i * 6;
        const double* xj = x + (size_t)j * 6;
        double* Y = w.Ye + (size_t)(on ? e : 0) * 78;
        if (on) pg_edge_column(w.Z + (size_t)e * 36, 1.0, noise.J, xi, xj, d, true, Y);
        __syncthreads();
        if (on && d < 12) {   // local parameterisation: J_theta <- J_theta * dPlus/ddelta  (lane = (row r, pose side))
            const int r = d % 6, side = d / 6;
            pg_row_times_plus_jac(&Y[r * 13 + 6 * side + 3], (side ? xj : xi) + 3);
        }
        __syncthreads();
    }
}

// a wave per node: 6x6 diagonal block and gradient, gathered over the node's edges in list order; a constant node gets the identity
__device__ __forceinline__ void assemble(const Wk& w, int N, int ne, int wave, int lane) {
    const int r = lane / 6, c = lane % 6;
    for (int k = wave; k < N; k += 4) {
        const bool is_const = w.cst[k] != 0;
        double acc = 0.0;
        if (!is_const)
            for (int e = 0; e < ne; ++e) {
                if (!w.enode[3 * e + 2]) continue;
                int side;
                if (w.enode[3 * e] == k) side = 0; else if (w.enode[3 * e + 1] == k) side = 1; else continue;
                const double* Y = w.Ye + (size_t)e * 78;
                acc += pg_node_edge(Y, side, lane);
            }
        if (is_const && lane < 36) acc = r == c ? 1.0 : 0.0;
        if (lane < 36) w.Dd[(size_t)k * 36 + lane] = acc;
        else if (lane < 42) w.gd[k * 6 + (lane - 36)] = acc;
    }
}

// 1/2 sum r^2 of the used edges, by one wave
__device__ __forceinline__ double cost_of(const Wk& w, int ne, int lane) {
    double s = 0.0;
    for (int e = lane; e < ne; e += 64)
        if (w.enode[3 * e + 2])
#pragma unroll
            for (int r = 0; r < 6; ++r) { const double v = w.Ye[(size_t)e * 78 + r * 13 + 12]; s += v * v; }
    return 0.5 * wave_sum(s);
}

// the group is done (wave 0): T_g_w of its non-constant nodes unless the solve failed, the summary, the header
__device__ __forceinline__ void finish(int* hdr, const Wk& w, int N, int iter, int succ, double init_cost, double x_cost, int term, double* T_g_w,
                                       liw_summary* summary_g, int lane) {
    const bool failed = term == 6 || !isfinite(x_cost) || !isfinite(init_cost);
    if (!failed)
        for (int k = lane; k < N; k += 64)
            if (!w.cst[k]) store_iso(tf_of_pose(w.x + (size_t)k * 6), T_g_w + (size_t)w.nodes[k] * 12);
    if (lane == 0) {
        liw_summary sm;
        sm.iterations = iter; sm.successful_steps = succ; sm.termination = term; sm.initial_cost = init_cost; sm.final_cost = x_cost;
        *(liw_summary*)((char*)hdr + HB_SUMMARY) = sm;
        *summary_g = sm;
        hdr[H_SOLVES] += 1;
        w.lm->term = term;   // the rest of the state is not read again
        w.lm->done = 1;
    }
}

// wave 0: cost / norms of a new point, termination 1 / 4 / 5, the LM diagonal (k_fpg_head)
__device__ __forceinline__ void head(int* hdr, const Wk& w, int max_iters, double* T_g_w, liw_summary* summary_g, int lane) {
    Lm s = *w.lm;
    const int term = pg_lm_head(s, PgConstFlags{w.cst}, [&] { return cost_of(w, s.ne, lane); }, s.N, max_iters, w.x, w.gd, w.Dd, w.scale, w.dgn, lane);
    if (term) {
        finish(hdr, w, s.N, s.iter, s.succ, s.init_cost, s.x_cost, term, T_g_w, summary_g, lane);
        return;
    }
    if (lane == 0) *w.lm = s;
}

// all 256 threads: (J'J scaled + D^2 / radius) y = g scaled on the packed triangle A; false when a pivot is not positive and finite
__device__ __forceinline__ bool reduced(const Wk& w, double* A, int N, int ne, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int nr = 6 * N, tri_n = nr * (nr + 1) / 2;
    double* rhs = w.rhs;
    const double radius = w.lm->radius;
    for (int e = tid; e < tri_n; e += 256) A[e] = 0.0;
    __syncthreads();
    for (int t = wave; t < N; t += 4) {
        const int r = lane / 6, c = lane % 6;
        const double* sf = w.scale + (size_t)t * 6;
        const bool is_const = w.cst[t] != 0;
        if (lane < 36) {
            const double v = is_const ? (r == c ? 1.0 : 0.0) : w.Dd[(size_t)t * 36 + lane] * sf[r] * sf[c] + (r == c ? w.dgn[(size_t)t * 6 + c] / radius : 0.0);
            if (r >= c) A[tri(t * 6 + r, t * 6 + c)] = v;
        } else if (lane < 42) {
            const int k = lane - 36;
            rhs[t * 6 + k] = is_const ? 0.0 : w.gd[(size_t)t * 6 + k] * sf[k];
        }
    }
    __syncthreads();
    if (wave == 0 && lane < 36) {   // off-diagonal blocks in list order by one wave (several edges may share a block); a lane owns the
        const int r = lane / 6, c = lane % 6;   // same entry (row r of the higher node, column c of the lower) whatever the edge's direction
        for (int e = 0; e < ne; ++e) {
            if (!w.enode[3 * e + 2]) continue;
            const int i1 = w.enode[3 * e], i2 = w.enode[3 * e + 1];
            if (w.cst[i1] || w.cst[i2]) continue;
            const double* Y = w.Ye + (size_t)e * 78;
            const int ra = i1 > i2 ? r : c, cb = i1 > i2 ? c : r;   // H[i1, i2](ra, cb) = sum_k J1[k][ra] J2[k][cb]
            double o = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) o += Y[k * 13 + ra] * Y[k * 13 + 6 + cb];
            const double v = o * w.scale[(size_t)i1 * 6 + ra] * w.scale[(size_t)i2 * 6 + cb];
            const int hi = i1 > i2 ? i1 : i2, lo = i1 > i2 ? i2 : i1;
            A[tri(hi * 6 + r, lo * 6 + c)] += v;
        }
    }
    __syncthreads();
#include "k_pg_chol_body.inc"
    for (int e = tid; e < nr; e += 256) w.y[e] = rhs[e];
    return ok;
}

// wave 0: step validity, model cost change, Plus into the candidate, step norm; termination 6 (k_fpg_decide1)
__device__ __forceinline__ void decide1(int* hdr, const Wk& w, bool chol_ok, double* T_g_w, liw_summary* summary_g, int lane) {
    Lm s = *w.lm;
    const int term = pg_lm_decide1(s, PgConstFlags{w.cst}, chol_ok, s.N, w.x, w.cand, w.y, w.scale, w.dgn, w.gd, lane);
    if (term > 0) {
        finish(hdr, w, s.N, s.iter, s.succ, s.init_cost, s.x_cost, term, T_g_w, summary_g, lane);
        return;
    }
    if (lane == 0) *w.lm = s;
}

// wave 0: candidate cost, termination 2 / 3, rho, accept / reject, radius (k_fpg_decide2)
__device__ __forceinline__ void decide2(int* hdr, const Wk& w, double* T_g_w, liw_summary* summary_g, int lane) {
    Lm s = *w.lm;
    const int term = pg_lm_decide2(s, cost_of(w, s.ne, lane), s.N, w.x, w.cand, lane);
    if (term) {
        finish(hdr, w, s.N, s.iter, s.succ, s.init_cost, s.x_cost, term, T_g_w, summary_g, lane);
        return;
    }
    if (lane == 0) *w.lm = s;
}

// what wave 0 left in the LM state, read by every thread between two barriers (wave 0 may write the state again right afterwards)
__device__ __forceinline__ void state(const Wk& w, int& done, int& phase) {
    __syncthreads();
    const volatile Lm* s = w.lm;
    done = s->done; phase = s->phase;
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_ggraph_solve(char* store, Lay L, Noise noise, const double* __restrict__ poses, long long robot_stride,
                                                      const int* __restrict__ n_keyframes, const int* __restrict__ group_of,
                                                      const unsigned char* __restrict__ linked, const unsigned char* __restrict__ fixed, double* T_g_w,
                                                      const unsigned char* __restrict__ gsel, int max_iters, int lds_doubles, liw_summary* summary) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!gsel[g]) return;
    char* R = region(store, L, g);
    int* hdr = (int*)R;
    Wk w = work_of(store, L, g);
    // nodes: the linked members in index order, by ballots and prefix counts
    if (wave == 0) {
        int base = 0;
        bool anyfixed = false;
        for (int r0 = 0; r0 < L.B; r0 += 64) {
            const int r = r0 + lane;
            const bool flag = r < L.B && linked[r] != 0 && group_of[r] == g;
            const bool fx = flag && fixed[r] != 0;
            const unsigned long long m = __ballot(flag);
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (flag && pos < L.M) { w.nodes[pos] = r; w.cst[pos] = fx ? 1 : 0; }
            anyfixed = anyfixed || __ballot(fx) != 0ull;
            base += __popcll(m);
        }
        if (lane == 0) { w.lm->N = base; w.lm->anyfixed = anyfixed ? 1 : 0; w.lm->ne = min(max(hdr[H_NE], 0), L.E); }
    }
    __syncthreads();
    const int N = w.lm->N, ne = w.lm->ne;
    if (N > L.M) {
        if (tid == 0) hdr[H_MFULL] = 1;
        return;
    }
    if (N < 2 || ne < 1) return;
    if (tid == 0 && !w.lm->anyfixed) w.cst[0] = 1;
    __syncthreads();
    // edges: node indices, the use flag, Z from the corrected poses
    for (int e = tid; e < ne; e += 256) {
        const char* rec = R + kHeaderBytes + (size_t)e * kEdgeBytes;
        const int* ri = (const int*)rec;
        const int a = ri[0], q = ri[1], b = ri[2], i = ri[3];
        int ia = -1, ib = -1;
        for (int k = 0; k < N; ++k) { const int r = w.nodes[k]; if (r == a) ia = k; if (r == b) ib = k; }
        bool use = ia >= 0 && ib >= 0 && a != b;   // nodes are robots of 0 .. B-1
        use = use && q >= 0 && q < n_keyframes[a] && i >= 0 && i < n_keyframes[b] && !(w.cst[ia] && w.cst[ib]);
        use = use && ri[R_STATE] == 0;   // an edge that k_ggate rejected
        w.enode[3 * e] = ia; w.enode[3 * e + 1] = ib; w.enode[3 * e + 2] = use ? 1 : 0;
        if (use) {
            const IsoD Ta = tf_of_pose(poses + (size_t)a * robot_stride + (size_t)q * 6);
            const IsoD Tb = tf_of_pose(poses + (size_t)b * robot_stride + (size_t)i * 6);
            double* z = w.Z + (size_t)e * 36;
            store_iso(mul(mul(Ta, load_iso((const double*)(rec + kEdgeTf))), inverse(Tb)), z);
            store_iso(Ta, z + 12);
            store_iso(Tb, z + 24);
        }
    }
    __syncthreads();
    if (wave == 0) {
        int used = 0;
        for (int e0 = 0; e0 < ne; e0 += 64) used += __popcll(__ballot(e0 + lane < ne && w.enode[3 * (e0 + lane) + 2] != 0));
        if (lane == 0) w.lm->used = used;
    }
    __syncthreads();
    const int used = w.lm->used;
    if (used < 1) return;
    for (int k = tid; k < N; k += 256) {
        double ps[6];
        pose_of_tf(T_g_w + (size_t)w.nodes[k] * 12, ps);
        for (int t = 0; t < 6; ++t) { w.x[k * 6 + t] = ps[t]; w.cand[k * 6 + t] = ps[t]; w.y[k * 6 + t] = 0.0; }
    }
    if (tid == 0) {
        Lm s;
        pg_lm_start(s, 0);
        s.N = N; s.ne = ne; s.used = used; s.anyfixed = w.lm->anyfixed;
        *w.lm = s;
        hdr[H_SKIPPED] = ne - used; hdr[H_NODES] = N; hdr[H_USED] = used;
    }
    __syncthreads();
    const int K = max_iters > 0 ? max_iters : 50;
    const int nr = 6 * N, tri_n = nr * (nr + 1) / 2;
    double* A = tri_n <= lds_doubles ? lds : w.Hr;   // the same instructions either way
    liw_summary* sg = summary + g;
    linearize(w, noise, ne, 0, tid);
    assemble(w, N, ne, wave, lane);
    __syncthreads();
    for (;;) {   // ends by termination: the iteration cap (4) at the latest
        int done, phase;
        if (wave == 0) head(hdr, w, K, T_g_w, sg, lane);
        state(w, done, phase);
        if (done) break;
        const bool ok = reduced(w, A, N, ne, tid);
        __syncthreads();
        if (wave == 0) decide1(hdr, w, ok, T_g_w, sg, lane);
        state(w, done, phase);
        if (done) break;
        if (phase != PH_CAND) continue;
        linearize(w, noise, ne, 1, tid);
        if (wave == 0) decide2(hdr, w, T_g_w, sg, lane);
        state(w, done, phase);
        if (done) break;
        if (phase == PH_ASM) assemble(w, N, ne, wave, lane);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------- the edge gate
// include/liw_group_gate.h: a work-group per group works on what the group's last solve left in its work area.  Edges are strided over
// the threads: c = |edge_res|^2 at the accepted x into the record, the support by a scan of that solve's edge list (E^2 / 256 pair
// tests a thread), the thread's best candidate; then a block arg-max on (c, index) in a fixed order, and thread 0 retires the winner.
__global__ __launch_bounds__(256) void k_ggate(char* store, Lay L, Noise noise, const unsigned char* __restrict__ gsel, double chi2_max, int min_support,
                                               unsigned char* __restrict__ changed) {
    __shared__ double best_c[256];
    __shared__ int best_e[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    char* R = region(store, L, g);
    int* hdr = (int*)R;
    const int solves = hdr[H_SOLVES];
    const liw_summary sm = *(const liw_summary*)(R + HB_SUMMARY);
    const bool eligible = gsel[g] != 0 && solves > 0 && solves != hdr[H_GATED] && sm.termination != 6 && isfinite(sm.final_cost);
    if (!eligible) {   // the same for every thread of the group
        if (tid == 0) changed[g] = 0;
        return;
    }
    const Wk w = work_of(store, L, g);
    const int N = min(max(hdr[H_NODES], 0), L.M);                      // of the last completed solve; edges appended since are beyond ne
    const int ne = min(max(hdr[H_USED] + hdr[H_SKIPPED], 0), L.E);
    double bc = 0.0;
    int be = -1;
    for (int e = tid; e < ne; e += 256) {
        const int ia = w.enode[3 * e], ib = w.enode[3 * e + 1];
        if (!w.enode[3 * e + 2] || ia < 0 || ia >= N || ib < 0 || ib >= N) continue;
        double res[6];
        const double *xa = w.x + (size_t)ia * 6, *xb = w.x + (size_t)ib * 6;
        edge_res<double>(w.Z + (size_t)e * 36, 1.0, noise.J, xa, xa + 3, xb, xb + 3, res);
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) c += res[r] * res[r];
        *(double*)(R + kHeaderBytes + (size_t)e * kEdgeBytes + kEdgeChi2) = c;
        const int lo = min(ia, ib), hi = max(ia, ib);
        int support = 0;
        for (int f = 0; f < ne; ++f) {
            if (f == e || !w.enode[3 * f + 2]) continue;
            const int ja = w.enode[3 * f], jb = w.enode[3 * f + 1];
            if (min(ja, jb) == lo && max(ja, jb) == hi) ++support;
        }
        if (c > chi2_max && support >= min_support && (be < 0 || c > bc)) { bc = c; be = e; }   // a NaN compares false; e ascends: ties keep the lowest
    }
    best_c[tid] = bc; best_e[tid] = be;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const double oc = best_c[tid + s];
            const int oe = best_e[tid + s];
            const int me = best_e[tid];
            if (oe >= 0 && (me < 0 || oc > best_c[tid] || (oc == best_c[tid] && oe < me))) { best_c[tid] = oc; best_e[tid] = oe; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int e = best_e[0];
        if (e >= 0) {
            ((int*)(R + kHeaderBytes + (size_t)e * kEdgeBytes))[R_STATE] = 1;
            hdr[H_REJECTED] += 1;
        }
        hdr[H_GATED] = solves;
        changed[g] = e >= 0 ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------- launches
int launch_reset(char* store, const Lay& L, const unsigned char* gmask, hipStream_t s) {
    hipLaunchKernelGGL(k_ggraph_reset, dim3(L.G), dim3(256), 0, s, store, L, gmask);
    return launched();
}
int launch_add_edges(char* store, const Lay& L, const int* group_of, const unsigned char* found, const int* edge, const double* tf12,
                     const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_ggraph_add_edges, dim3(L.G), dim3(64), 0, s, store, L, group_of, found, edge, tf12, mask);
    return launched();
}
int launch_partner(int B, const int* group_of, const unsigned char* linked, int round, int* partner, hipStream_t s) {
    hipLaunchKernelGGL(k_ggraph_partner, dim3(B), dim3(64), 0, s, B, group_of, linked, round, partner);
    return launched();
}
int launch_solve(char* store, const Lay& L, const Noise& noise, const double* poses, long long robot_stride, const int* n_keyframes, const int* group_of,
                 const unsigned char* linked, const unsigned char* fixed, double* T_g_w, const unsigned char* gsel, int max_iters, int lds_cap_doubles,
                 liw_summary* summary, hipStream_t s) {
    // LDS for the triangle: what a full group of this store needs, 64 KiB at the most; a larger triangle runs from the work area
    const int nr = 6 * L.M, tri_max = nr * (nr + 1) / 2;
    const int lds_doubles = tri_max <= lds_cap_doubles ? tri_max : lds_cap_doubles;
    hipLaunchKernelGGL(k_ggraph_solve, dim3(L.G), dim3(256), sizeof(double) * (size_t)lds_doubles, s, store, L, noise, poses, robot_stride, n_keyframes,
                       group_of, linked, fixed, T_g_w, gsel, max_iters, lds_doubles, summary);
    return launched();
}
int launch_gate(char* store, const Lay& L, const Noise& noise, const unsigned char* gsel, double chi2_max, int min_support, unsigned char* changed,
                hipStream_t s) {
    hipLaunchKernelGGL(k_ggate, dim3(L.G), dim3(256), 0, s, store, L, noise, gsel, chi2_max, min_support, changed);
    return launched();
}

}  // namespace liw_ggraph_dev
