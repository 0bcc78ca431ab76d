// k_group_joint.hip — the joint pose graph of a group of fleet robots on the MI355X (C ABI include/liw_group_joint.h, host side
// liw_group_joint.cpp): the key frames of all members of a group are the nodes of one graph, tied by the members' sequential and own
// loop edges (read in place from the back-end store) and by the group's held cross edges (read in place from the group-graph store).
// The graph is several chains tied by a few edges, so k_posegraph_batch.hip's chain-segment method carries over kernel for kernel; what
// is new is the chain boundary: two consecutive separators of different chains have no segment and no coupling block between them.
// Every kernel has a fixed grid over (group, item) slots; a wave whose group is finished, not selected, or not in the phase the kernel
// serves exits at once, so the launches of all iterations can be enqueued without a read-back.
//   k_gj_setup      wave per group: members, node offsets, the loop list (own loops, then used cross edges) and the separator list by
//                   ballots and prefix counts; header, LM state.
//   k_gj_x0         lane per (robot, key frame): x0 = log_SE3(T_g_w * make_tf(P)) into the pose row and, for a group that is solved, x.
//   k_gj_linearize  16 lanes per (group, edge slot) and 8 per (group, node): edge_res / pg_ground_res with a dual direction per lane.
//   k_gj_assemble   wave per (group, node): the sequential edge into the node, the one out of it, then the loop list in order.
//   k_gj_head       wave per group: cost / norms of a new point, termination 1 / 4 / 5, the LM diagonal.
//   k_gj_seg_elim   wave per (group, segment): pg_seg_elim_wave on arrays indexed by joint node.
//   k_gj_reduced    work-group per group: the separators' packed triangle (LDS when it fits, else the work area: the same instructions on
//                   another pointer), loop and cross blocks in list order by one wave, k_pg_chol_body.inc, scatter.
//   k_gj_backsub    wave per (group, segment): pg_seg_backsub_wave.
//   k_gj_decide1/2  wave per group: the trust-region decisions of liw_lm_rules.hpp.
//   k_gj_finish     lane per (group, node): the solved poses into the pose rows, unless the solve failed.
// No atomic decides a position or a value (one atomic OR raises a group's "pivot not positive" flag).
#pragma clang fp contract(off)   // x0 is liw_lie_mul's product

#include "k_group_joint.hpp"
#include "k_posegraph_dev.hpp"
#include "k_posegraph_lm_dev.hpp"
#include "liw_dual.hpp"
#include "liw_lm_rules.hpp"

namespace liw_gjoint_dev {

using namespace liw;

// LM state of a group (head of its work area)
struct Lm : PgLmCore { int ns, N, nl, status, nm, cn, ran; };
static_assert(sizeof(Lm) <= 256, "the LM state has 256 bytes");

struct Wk {   // a group's work area
    Lm* lm; int *mem, *moff, *nmem, *nrow, *lidx, *sep, *sepidx;
    double *ltf, *x, *cand, *y, *scale, *dgn, *Ye, *Yg, *Dd, *gd, *Os, *Lb, *Sred, *rec, *Hr, *rhs;
};
__device__ __forceinline__ Wk work_of(char* store, const Lay& L, int g) {
    char* W = store + L.work_off + (size_t)g * L.work_group_bytes;
    Wk w;
    w.lm = (Lm*)W;
    w.mem = (int*)(W + L.w_mem); w.moff = (int*)(W + L.w_moff); w.nmem = (int*)(W + L.w_nmem); w.nrow = (int*)(W + L.w_nrow);
    w.lidx = (int*)(W + L.w_lidx); w.sep = (int*)(W + L.w_sep); w.sepidx = (int*)(W + L.w_sepidx);
    w.ltf = (double*)(W + L.w_ltf); w.x = (double*)(W + L.w_x); w.cand = (double*)(W + L.w_cand); w.y = (double*)(W + L.w_y);
    w.scale = (double*)(W + L.w_scale); w.dgn = (double*)(W + L.w_dgn); w.Ye = (double*)(W + L.w_Ye); w.Yg = (double*)(W + L.w_Yg);
    w.Dd = (double*)(W + L.w_Dd); w.gd = (double*)(W + L.w_gd); w.Os = (double*)(W + L.w_Os); w.Lb = (double*)(W + L.w_Lb);
    w.Sred = (double*)(W + L.w_Sred); w.rec = (double*)(W + L.w_rec); w.Hr = (double*)(W + L.w_Hr); w.rhs = (double*)(W + L.w_rhs);
    return w;
}
__device__ __forceinline__ int* header_of(char* store, const Lay& L, int g) { return (int*)(store + L.hdr_off + (size_t)g * kHeaderBytes); }
__device__ __forceinline__ const char* robot_of(const In& in, const Lay& L, int r) { return in.fpg + (size_t)r * L.f_robot_bytes; }
__device__ __forceinline__ int nkf_of(const In& in, const Lay& L, int r) { return clampi(((const int*)robot_of(in, L, r))[0], 0, L.K); }
__device__ __forceinline__ int nloop_of(const In& in, const Lay& L, int r) { return clampi(((const int*)robot_of(in, L, r))[1], 0, L.RL); }

// ------------------------------------------------------------------------------------------------------------- setup
__global__ __launch_bounds__(64) void k_gj_setup(char* store, Lay L, In in, liw_summary* summary) {
    const int g = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, g);
    if (!in.gsel[g]) {
        if (lane == 0) w.lm->done = 1;
        return;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int* roff = (int*)(store + L.roff_off);
    // members: the linked robots of the group that hold a key frame, in index order
    int nm = 0, cmem = -1;
    for (int r0 = 0; r0 < L.B; r0 += 64) {
        const int r = r0 + lane;
        const bool flag = r < L.B && in.group_of[r] == g && in.linked[r] != 0 && nkf_of(in, L, r) >= 1;
        const bool fx = flag && in.fixed[r] != 0;
        const unsigned long long m = __ballot(flag), fm = __ballot(fx);
        const int pos = nm + __popcll(m & below);
        if (flag && pos < L.M) w.mem[pos] = r;
        if (cmem < 0 && fm != 0ull) cmem = nm + __popcll(m & ((1ull << (__ffsll((long long)fm) - 1)) - 1ull));
        nm += __popcll(m);
    }
    if (cmem < 0) cmem = 0;
    const bool mfull = nm > L.M;
    __syncthreads();
    // offsets: prefix sums of the key-frame counts; own loops, members in order and loops in list order
    int N = 0, nlo = 0;
    if (!mfull) {
        for (int m0 = 0; m0 < nm; m0 += 64) {
            const int mi = m0 + lane;
            const bool on = mi < nm;
            const int r = on ? w.mem[mi] : 0;
            const int cnt = on ? nkf_of(in, L, r) : 0, lc = on ? nloop_of(in, L, r) : 0;
            int sc = cnt, sl = lc;
            for (int o = 1; o < 64; o <<= 1) {
                const int a = __shfl_up(sc, o, 64), b = __shfl_up(sl, o, 64);
                if (lane >= o) { sc += a; sl += b; }
            }
            const int off = N + sc - cnt, lpos = nlo + sl - lc;
            if (on) {
                w.moff[mi] = off;
                roff[r] = off;
                const char* R = robot_of(in, L, r);
                const int* li = (const int*)(R + L.f_lidx);
                const double* lt = (const double*)(R + L.f_ltf);
                for (int l = 0; l < lc; ++l) {
                    const int pos = lpos + l;
                    if (pos >= L.ML) break;
                    w.lidx[2 * pos] = off + clampi(li[2 * l], 0, cnt - 1);
                    w.lidx[2 * pos + 1] = off + clampi(li[2 * l + 1], 0, cnt - 1);
                    for (int k = 0; k < 12; ++k) w.ltf[(size_t)pos * 12 + k] = lt[(size_t)l * 12 + k];
                }
            }
            N += __shfl(sc, 63, 64);
            nlo += __shfl(sl, 63, 64);
        }
        if (lane == 0) w.moff[nm] = N;
    }
    const bool nfull = !mfull && N > L.N;
    __syncthreads();
    // cross edges, in list order; the use rule of liw_ggraph_solve
    int cused = 0, ne = 0;
    if (!mfull && !nfull) {
        const char* GR = in.gg + (size_t)g * L.gg_group_bytes;
        ne = clampi(((const int*)GR)[0], 0, L.E);
        for (int e0 = 0; e0 < ne; e0 += 64) {
            const int e = e0 + lane;
            const bool on = e < ne;
            const char* rec = GR + 256 + (size_t)(on ? e : 0) * 128;
            const int* ri = (const int*)rec;
            const int a = ri[0], q = ri[1], b = ri[2], i = ri[3], st = ri[5];
            int ia = -1, ib = -1;
            for (int k = 0; k < nm; ++k) { const int r = w.mem[k]; if (r == a) ia = k; if (r == b) ib = k; }
            bool use = on && a != b && ia >= 0 && ib >= 0 && st == 0;
            use = use && q >= 0 && q < nkf_of(in, L, a) && i >= 0 && i < nkf_of(in, L, b);
            const unsigned long long m = __ballot(use);
            const int pos = nlo + cused + __popcll(m & below);
            if (use && pos < L.ML) {
                w.lidx[2 * pos] = w.moff[ia] + q;
                w.lidx[2 * pos + 1] = w.moff[ib] + i;
                const double* tf = (const double*)(rec + 32);
                for (int k = 0; k < 12; ++k) w.ltf[(size_t)pos * 12 + k] = tf[k];
            }
            cused += __popcll(m);
        }
    }
    const int nl = nlo + cused;
    const bool lfull = !mfull && !nfull && nl > L.ML;
    const bool counted = !mfull && !nfull && !lfull;
    __syncthreads();
    // nodes: member and pose row of every node, the separator list
    int ns = 0;
    if (counted) {
        for (int n0 = 0; n0 < N; n0 += 64) {
            const int n = n0 + lane;
            const bool on = n < N;
            int mi = 0;
            for (int k = 1; k < nm; ++k)
                if (on && w.moff[k] <= n) mi = k;
            const int k = n - w.moff[mi], cnt = w.moff[mi + 1] - w.moff[mi];
            bool flag = on && (k == 0 || k == cnt - 1 || k % PG_STRIDE == 0);
            if (on && !flag)
                for (int l = 0; l < nl; ++l) flag = flag || w.lidx[2 * l] == n || w.lidx[2 * l + 1] == n;
            const unsigned long long m = __ballot(flag);
            const int pos = ns + __popcll(m & below);
            if (on) {
                w.sepidx[n] = flag ? pos : -1;
                w.nmem[n] = mi;
                w.nrow[n] = w.mem[mi] * L.K + k;
            }
            if (flag && pos < L.NS) w.sep[pos] = n;
            ns += __popcll(m);
        }
    }
    const bool solve = counted && N >= 2 && (N - nm) + nl >= 1 && ns <= L.NS;
    if (lane == 0) {
        int* hdr = header_of(store, L, g);
        hdr[H_RESERVED] = 0; hdr[H_MFULL] = mfull; hdr[H_NFULL] = nfull; hdr[H_LFULL] = lfull; hdr[H_MEMBERS] = nm; hdr[H_NODES] = mfull ? 0 : N;
        hdr[H_SEQ] = counted || lfull ? N - nm : 0; hdr[H_OWN] = counted || lfull ? nlo : 0; hdr[H_USED] = counted || lfull ? cused : 0;
        hdr[H_SKIPPED] = counted || lfull ? ne - cused : 0; hdr[H_SEPS] = counted ? ns : 0; hdr[H_SOLVED] = solve; hdr[H_CONST] = counted ? w.moff[cmem] : 0;
        Lm s;
        pg_lm_start(s, solve ? 0 : 1);
        s.ns = ns; s.N = N; s.nl = nl; s.status = 0; s.nm = nm; s.cn = counted ? w.moff[cmem] : 0; s.ran = solve;
        *w.lm = s;
        if (!solve) {
            liw_summary sm;
            sm.iterations = 0; sm.successful_steps = 0; sm.termination = 0; sm.initial_cost = 0.0; sm.final_cost = 0.0;
            *(liw_summary*)((char*)hdr + HB_SUMMARY) = sm;
            summary[g] = sm;
        }
    }
}

__global__ __launch_bounds__(64) void k_gj_x0(char* store, Lay L, In in) {
    const long long slot = (long long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= (long long)L.B * L.K) return;
    const int r = (int)(slot / L.K), k = (int)(slot % L.K);
    const int g = in.group_of[r];
    if (g < 0 || g >= L.G || !in.gsel[g] || !in.linked[r] || k >= nkf_of(in, L, r)) return;
    double ps[6];
    pose_of_tf(mul(load_tf(in.T_g_w + (size_t)r * 12), tf_of_pose((const double*)(robot_of(in, L, r) + L.f_pose) + (size_t)k * 6)), ps);
    double* row = (double*)(store + L.pose_off) + (size_t)slot * 6;
    for (int t = 0; t < 6; ++t) row[t] = ps[t];
    Wk w = work_of(store, L, g);
    if (w.lm->done) return;
    const int n = ((const int*)(store + L.roff_off))[r] + k;
    if (n < 0 || n >= w.lm->N) return;
    for (int t = 0; t < 6; ++t) { w.x[(size_t)n * 6 + t] = ps[t]; w.cand[(size_t)n * 6 + t] = ps[t]; w.y[(size_t)n * 6 + t] = 0.0; }
}

// ------------------------------------------------------------------------------------------------------------- the LM loop
// node n follows node n - 1 in the same chain: slot n holds the sequential edge (n - 1, n)
__device__ __forceinline__ bool has_prev(const Wk& w, int n) { return n > 0 && w.nmem[n] == w.nmem[n - 1]; }

// Y of edge slot e [6][13] = [J | r], of node f [2][7]; which = 0: at x for groups in PH_INIT, 1: at the candidate for PH_CAND
__global__ __launch_bounds__(64) void k_gj_linearize(char* store, Lay L, In in, Noise noise, DevParams P, int which) {
    __shared__ double Y[4][6 * 13];
    const int lane = threadIdx.x & 63, grp = lane >> 4, d = lane & 15;
    const long long edge_slots = (long long)L.G * L.NE;
    const long long edge_blocks = (edge_slots + 3) / 4;
    const int want = which ? PH_CAND : PH_INIT;
    if ((long long)blockIdx.x < edge_blocks) {
        const long long slot = (long long)blockIdx.x * 4 + grp;
        const int g = slot < edge_slots ? (int)(slot / L.NE) : 0, e = (int)(slot % L.NE);
        Wk w = work_of(store, L, g);
        bool on = slot < edge_slots && !w.lm->done && w.lm->phase == want;
        int i = 0, j = 0;
        const double* tf = nullptr;
        double weight = 1.0;
        if (on) {
            const int N = w.lm->N, nl = w.lm->nl;
            if (e < L.N) {
                on = e < N && has_prev(w, e);
                if (on) {
                    i = e - 1; j = e;
                    const int row = w.nrow[e];
                    tf = (const double*)(robot_of(in, L, row / L.K) + L.f_seq) + (size_t)(row % L.K) * 12;
                }
            } else {
                const int l = e - L.N;
                on = l < nl;
                if (on) { i = w.lidx[2 * l]; j = w.lidx[2 * l + 1]; }
                tf = w.ltf + (size_t)l * 12;
                weight = noise.loop_edge_k;
            }
        }
        const double* x = which ? w.cand : w.x;
        const double* xi = x + (size_t)i * 6;
        const double* xj = x + (size_t)j * 6;
        if (on) pg_edge_column(tf, weight, noise.J, xi, xj, d, true, Y[grp]);
        __syncthreads();
        if (on && d < 12) {   // local parameterisation: J_theta <- J_theta * dPlus/ddelta  (lane = (row r, pose side))
            const int r = d % 6, side = d / 6;
            pg_row_times_plus_jac(&Y[grp][r * 13 + 6 * side + 3], (side ? xj : xi) + 3);
        }
        __syncthreads();
        if (on && d < 13)
#pragma unroll
            for (int r = 0; r < 6; ++r) w.Ye[(size_t)e * 78 + r * 13 + d] = Y[grp][r * 13 + d];
    } else {
        // ground factors: 8 nodes per wave, 6 dual directions + value
        const int sub = lane >> 3, dir = lane & 7;
        const long long slot = ((long long)blockIdx.x - edge_blocks) * 8 + sub;
        const long long slots = (long long)L.G * L.N;
        const int g = slot < slots ? (int)(slot / L.N) : 0, f = (int)(slot % L.N);
        Wk w = work_of(store, L, g);
        const bool on = slot < slots && !w.lm->done && w.lm->phase == want && f < w.lm->N;
        const double* x = which ? w.cand : w.x;
        double* Yl = &Y[0][0] + sub * 16;
        if (on) pg_ground_column(P, noise.ground_on_p, noise.ground_on_q, x + (size_t)f * 6, dir, true, Yl);
        __syncthreads();
        if (on && dir < 2) {
            pg_row_times_plus_jac(Yl + dir * 7 + 3, x + (size_t)f * 6 + 3);
        }
        __syncthreads();
        if (on && dir < 7) {
            w.Yg[(size_t)f * 14 + dir] = Yl[dir];
            w.Yg[(size_t)f * 14 + 7 + dir] = Yl[7 + dir];
        }
    }
}

// wave per (group, node), for groups in PH_INIT or PH_ASM.  The constant node: identity block, zero gradient.
__global__ __launch_bounds__(64) void k_gj_assemble(char* store, Lay L) {
    const int g = blockIdx.x / L.N, i = blockIdx.x % L.N, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, g);
    if (w.lm->done || (w.lm->phase != PH_INIT && w.lm->phase != PH_ASM)) return;
    const int N = w.lm->N, nl = w.lm->nl, cn = w.lm->cn;
    if (i >= N) return;
    const int* lidx = w.lidx;
    const double *Ye = w.Ye, *Yg = w.Yg;
    const int r = lane / 6, c = lane % 6;
    double acc = 0.0;
    const bool is_const = i == cn;
    const bool prev = has_prev(w, i), next = i + 1 < N && has_prev(w, i + 1);
    if (!is_const) {
        acc = pg_node_ground(Yg + (size_t)i * 14, lane);
    }
    // incident edges in edge order: the sequential edge into i (side 1), the one out of i (side 0), then the loops that name i
    const int n_inc = 2 + nl;
    for (int t = 0; t < n_inc; ++t) {
        int e, side, j;
        if (t == 0) { if (!prev) continue; e = i; side = 1; j = i - 1; }
        else if (t == 1) { if (!next) continue; e = i + 1; side = 0; j = i + 1; }
        else {
            const int l = t - 2, i1 = lidx[2 * l], i2 = lidx[2 * l + 1];
            if (i1 == i) { side = 0; j = i2; } else if (i2 == i) { side = 1; j = i1; } else continue;
            e = L.N + l;
        }
        const double* Y = Ye + (size_t)e * 78;
        if (!is_const) {
            acc += pg_node_edge(Y, side, lane);
        }
        if (side == 0 && lane < 36) {   // H[index1, index2](r, c) = sum_k J1[k][r] J2[k][c]; zero against the constant node
            const double o = !is_const && j != cn ? pg_edge_cross(Y, lane) : 0.0;
            if (t == 1) w.Os[(size_t)i * 36 + lane] = o;
            else w.Lb[(size_t)(t - 2) * 36 + lane] = o;
        }
    }
    if (!next && lane < 36) w.Os[(size_t)i * 36 + lane] = 0.0;   // the last node of a chain has no block to the right
    if (is_const && lane < 36) acc = r == c ? 1.0 : 0.0;
    if (lane < 36) w.Dd[(size_t)i * 36 + lane] = acc;
    else if (lane < 42) w.gd[i * 6 + (lane - 36)] = acc;
}

// 1/2 sum r^2 of the group's blocks in Ye / Yg (the constant node's ground block is not part of the cost), by one wave
__device__ __forceinline__ double cost_of(const Lay& L, const Wk& w, int N, int nl, int cn, int lane) {
    double s = 0.0;
    for (int e = lane; e < N; e += 64)
        if (has_prev(w, e))
#pragma unroll
            for (int r = 0; r < 6; ++r) { const double v = w.Ye[(size_t)e * 78 + r * 13 + 12]; s += v * v; }
    for (int l = lane; l < nl; l += 64)
#pragma unroll
        for (int r = 0; r < 6; ++r) { const double v = w.Ye[(size_t)(L.N + l) * 78 + r * 13 + 12]; s += v * v; }
    for (int f = lane; f < N; f += 64)
        if (f != cn) { const double a = w.Yg[(size_t)f * 14 + 6], c = w.Yg[(size_t)f * 14 + 13]; s += a * a; s += c * c; }
    return 0.5 * wave_sum(s);
}

// the group is done: summary, header
__device__ __forceinline__ void finish(char* store, const Lay& L, int g, const Wk& w, int term, liw_summary* summary, int lane) {
    if (lane == 0) {
        int* hdr = header_of(store, L, g);
        liw_summary sm;
        sm.iterations = w.lm->iter; sm.successful_steps = w.lm->succ; sm.termination = term; sm.initial_cost = w.lm->init_cost; sm.final_cost = w.lm->x_cost;
        *(liw_summary*)((char*)hdr + HB_SUMMARY) = sm;
        summary[g] = sm;
        w.lm->term = term;
        w.lm->done = 1;
    }
}

__global__ __launch_bounds__(64) void k_gj_head(char* store, Lay L, int max_iters, liw_summary* summary) {
    const int g = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, g);
    if (w.lm->done) return;
    Lm s = *w.lm;
    const int term = pg_lm_head(s, PgConstNode{s.cn}, [&] { return cost_of(L, w, s.N, s.nl, s.cn, lane); }, s.N, max_iters, w.x, w.gd, w.Dd, w.scale, w.dgn,
                                lane);
    if (term) {
        if (lane == 0) *w.lm = s;
        finish(store, L, g, w, term, summary, lane);
        return;
    }
    s.status = 0;
    if (lane == 0) *w.lm = s;
}

// a segment lies between two consecutive separators of the same chain
__global__ __launch_bounds__(64) void k_gj_seg_elim(char* store, Lay L) {
    const int nsg = L.NS - 1;
    const int g = blockIdx.x / nsg, sg = blockIdx.x % nsg, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, g);
    if (w.lm->done || w.lm->phase != PH_SOLVE || sg >= w.lm->ns - 1) return;
    const int a = w.sep[sg], bb = w.sep[sg + 1];
    if (w.nmem[a] != w.nmem[bb]) return;
    const bool ok = pg_seg_elim_wave(a, bb, lane, w.Dd, w.gd, w.Os, w.scale, w.dgn, w.lm->radius, w.Sred + (size_t)sg * PG_SEG, w.rec);
    if (!ok && lane == 0) atomicOr(&w.lm->status, 1);
}

// work-group per group: the separators' system A y = g_s, Cholesky, both solves, scatter
__global__ __launch_bounds__(256) void k_gj_reduced(char* store, Lay L, int lds_doubles) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int g = blockIdx.x, tid = threadIdx.x;
    Wk w = work_of(store, L, g);
    if (w.lm->done || w.lm->phase != PH_SOLVE) return;
    const int ns = w.lm->ns, nr = 6 * ns;
    double* A = nr * (nr + 1) / 2 <= lds_doubles ? lds : w.Hr;   // the same instructions either way
    double* rhs = w.rhs;
    const int* sep = w.sep;
    pg_reduced_system(A, rhs, ns, w.lm->nl, w.lm->cn, sep, w.sepidx, w.lidx, w.nmem, w.Dd, w.gd, w.Os, w.Lb, w.Sred, w.scale, w.dgn, w.lm->radius, tid);
#include "k_pg_chol_body.inc"
    for (int e = tid; e < nr; e += 256) w.y[(size_t)sep[e / 6] * 6 + e % 6] = rhs[e];
    if (!ok && tid == 0) atomicOr(&w.lm->status, 1);
}

__global__ __launch_bounds__(64) void k_gj_backsub(char* store, Lay L) {
    const int nsg = L.NS - 1;
    const int g = blockIdx.x / nsg, sg = blockIdx.x % nsg, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, g);
    if (w.lm->done || w.lm->phase != PH_SOLVE || sg >= w.lm->ns - 1) return;
    const int a = w.sep[sg], bb = w.sep[sg + 1];
    if (w.nmem[a] != w.nmem[bb]) return;
    pg_seg_backsub_wave(a, bb, lane, w.rec, w.y);
}

__global__ __launch_bounds__(64) void k_gj_decide1(char* store, Lay L, liw_summary* summary) {
    const int g = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, g);
    if (w.lm->done || w.lm->phase != PH_SOLVE) return;
    Lm s = *w.lm;
    const int term = pg_lm_decide1(s, PgConstNode{s.cn}, s.status == 0, s.N, w.x, w.cand, w.y, w.scale, w.dgn, w.gd, lane);
    if (lane == 0) *w.lm = s;
    if (term > 0) finish(store, L, g, w, term, summary, lane);
}

__global__ __launch_bounds__(64) void k_gj_decide2(char* store, Lay L, liw_summary* summary) {
    const int g = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, g);
    if (w.lm->done || w.lm->phase != PH_CAND) return;
    Lm s = *w.lm;
    const int term = pg_lm_decide2(s, cost_of(L, w, s.N, s.nl, s.cn, lane), s.N, w.x, w.cand, lane);
    if (term) {
        finish(store, L, g, w, term, summary, lane);
        return;
    }
    if (lane == 0) *w.lm = s;
}

// groups still iterating (a sum of integers by one work-group)
__global__ __launch_bounds__(256) void k_gj_count(char* store, Lay L) {
    __shared__ int red[256];
    int cnt = 0;
    for (int g = threadIdx.x; g < L.G; g += 256) cnt += work_of(store, L, g).lm->done ? 0 : 1;
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) *(int*)(store + L.g_count) = red[0];
}

// lane per (group, node): the solved poses into the pose rows; a failed solve leaves x0 there
__global__ __launch_bounds__(64) void k_gj_finish(char* store, Lay L, In in) {
    const long long slot = (long long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= (long long)L.G * L.N) return;
    const int g = (int)(slot / L.N), n = (int)(slot % L.N);
    if (!in.gsel[g]) return;
    Wk w = work_of(store, L, g);
    const Lm* s = w.lm;
    if (!s->ran || !s->done || n >= s->N) return;
    if (s->term == 6 || !isfinite(s->x_cost) || !isfinite(s->init_cost)) return;
    const int row = w.nrow[n];
    if (row < 0 || row >= L.B * L.K) return;
    double* out = (double*)(store + L.pose_off) + (size_t)row * 6;
    for (int t = 0; t < 6; ++t) out[t] = w.x[(size_t)n * 6 + t];
}

// ------------------------------------------------------------------------------------------------------------- launches
int launch_solve(char* store, const Lay& L, const Noise& noise, const DevParams& P, const In& in, int max_iters, int check_every, int lds_cap_doubles,
                 liw_summary* summary, hipStream_t s) {
    const int K = max_iters > 0 ? max_iters : 50;
    const unsigned G = (unsigned)L.G;
    const unsigned lin_blocks = (unsigned)(((long long)L.G * L.NE + 3) / 4 + ((long long)L.G * L.N + 7) / 8);
    const unsigned asm_blocks = G * (unsigned)L.N, seg_blocks = G * (unsigned)(L.NS > 1 ? L.NS - 1 : 0);
    const unsigned x0_blocks = (unsigned)(((long long)L.B * L.K + 63) / 64), fin_blocks = (unsigned)(((long long)L.G * L.N + 63) / 64);
    // LDS for the separator systems: what the largest one of this store needs, 64 KiB at the most; a larger triangle runs from the work area
    const int nr = 6 * L.NS;
    const long long tri_max = (long long)nr * (nr + 1) / 2;
    const int lds_doubles = tri_max <= lds_cap_doubles ? (int)tri_max : lds_cap_doubles;
    hipLaunchKernelGGL(k_gj_setup, dim3(G), dim3(64), 0, s, store, L, in, summary);
    hipLaunchKernelGGL(k_gj_x0, dim3(x0_blocks), dim3(64), 0, s, store, L, in);
    hipLaunchKernelGGL(k_gj_linearize, dim3(lin_blocks), dim3(64), 0, s, store, L, in, noise, P, 0);
    hipLaunchKernelGGL(k_gj_assemble, dim3(asm_blocks), dim3(64), 0, s, store, L);
    if (launched()) return -1;
    bool all_done = false;
    for (int it = 0; it < K && !all_done; ++it) {
        hipLaunchKernelGGL(k_gj_head, dim3(G), dim3(64), 0, s, store, L, K, summary);
        if (seg_blocks) hipLaunchKernelGGL(k_gj_seg_elim, dim3(seg_blocks), dim3(64), 0, s, store, L);
        hipLaunchKernelGGL(k_gj_reduced, dim3(G), dim3(256), sizeof(double) * (size_t)lds_doubles, s, store, L, lds_doubles);
        if (seg_blocks) hipLaunchKernelGGL(k_gj_backsub, dim3(seg_blocks), dim3(64), 0, s, store, L);
        hipLaunchKernelGGL(k_gj_decide1, dim3(G), dim3(64), 0, s, store, L, summary);
        hipLaunchKernelGGL(k_gj_linearize, dim3(lin_blocks), dim3(64), 0, s, store, L, in, noise, P, 1);
        hipLaunchKernelGGL(k_gj_decide2, dim3(G), dim3(64), 0, s, store, L, summary);
        hipLaunchKernelGGL(k_gj_assemble, dim3(asm_blocks), dim3(64), 0, s, store, L);
        if (launched()) return -1;
        if (check_every > 0 && (it + 1) % check_every == 0 && it + 1 < K) {
            int left = 0;
            hipLaunchKernelGGL(k_gj_count, dim3(1), dim3(256), 0, s, store, L);
            if (hipMemcpyAsync(&left, store + L.g_count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return -1;
            all_done = left == 0;
        }
    }
    if (!all_done) hipLaunchKernelGGL(k_gj_head, dim3(G), dim3(64), 0, s, store, L, K, summary);   // the iteration cap (termination 4) of who is left
    hipLaunchKernelGGL(k_gj_finish, dim3(fin_blocks), dim3(64), 0, s, store, L, in);
    return launched();
}

}  // namespace liw_gjoint_dev
