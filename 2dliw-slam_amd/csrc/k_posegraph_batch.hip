// k_posegraph_batch.hip — the fleet's pose-graph back-end on the MI355X (C ABI include/liw_posegraph_batch.h): B key-frame queues with
// their edges, and keyframe_manager::solve for the robots that are due, all in lock-step with the LM bookkeeping on the device.
//
// Bookkeeping (add_keyframes, add_loops, due, correct): a lane per robot, make_tf / log_SE3 with liw_crmath.hpp.
// Solve: per LM iteration the linear system liw_posegraph_solve's sparse path solves (k_posegraph.hip), one robot at a time there, all
// selected robots here.  Every kernel has a fixed grid over (robot, item) slots; a wave whose robot is finished, not selected, or not
// in the phase the kernel serves exits at once, so the launches of all iterations can be enqueued without a read-back.
//   k_fpg_setup       wave per robot: poses -> x, the separator list (frame 0, the last frame, loop end points, every 48th frame) by
//                     ballots and prefix counts, LM state.
//   k_fpg_linearize   16 lanes per (robot, edge) and 8 per (robot, key frame): edge_res / pg_ground_res of k_posegraph_dev.hpp with a
//                     dual direction per lane, always with the Jacobian (a candidate that is accepted needs no second pass).
//   k_fpg_assemble    wave per (robot, key frame): 6x6 diagonal block, gradient, off-diagonal blocks.  A chain needs no incidence
//                     list: key frame f touches sequential edges f-1 and f, then the robot's loops in edge order (the order
//                     k_pg_assemble_blocks sums in).
//   k_fpg_head        wave per robot: cost / norms of a new point, termination 1 / 4 / 5, the LM diagonal.
//   k_fpg_seg_elim    wave per (robot, segment): pg_seg_elim_wave with the robot's own radius.
//   k_fpg_reduced     work-group per robot: the separator system (packed lower triangle, in LDS when it fits, else in the robot's work
//                     area: the same instructions on another pointer), loop blocks in edge order by one wave, right-looking Cholesky,
//                     both triangular solves, scatter.
//   k_fpg_backsub     wave per (robot, segment): pg_seg_backsub_wave.
//   k_fpg_decide1     wave per robot: step validity, model cost change, Plus into the candidate, step norm; termination 6.
//   k_fpg_decide2     wave per robot: candidate cost, termination 2 / 3, rho, accept / reject, radius.
// The rules are the functions of liw_lm_rules.hpp.  A robot that terminates writes its poses, summary and the commit
// (modify_delta_tf, pending flag, last_solve_time, solves) itself.
#include "k_posegraph_batch.hpp"
#include "k_posegraph_dev.hpp"
#include "k_posegraph_lm_dev.hpp"

namespace liw_fpg_dev {

using namespace liw;

// LM state of a robot (head of its work block)
struct Lm : PgLmCore { int ns, N, nl, status; };
static_assert(sizeof(Lm) <= 256, "the LM state has 256 bytes");

__device__ __forceinline__ char* region(char* store, const Lay& L, int b) { return store + (size_t)b * L.robot_bytes; }
__device__ __forceinline__ char* workblk(char* store, const Lay& L, int b) { return store + L.work_off + (size_t)b * L.work_robot_bytes; }

// ------------------------------------------------------------------------------------------------------------- bookkeeping
__global__ __launch_bounds__(256) void k_fpg_reset(char* store, Lay L, const unsigned char* __restrict__ mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b)) return;
    char* R = region(store, L, b);
    int* hdr = (int*)R;
    for (int k = 0; k < 8; ++k) hdr[k] = 0;
    *(double*)(R + HB_TLAST) = -1e300;
    double* mod = (double*)(R + HB_MOD);
    for (int k = 0; k < 12; ++k) mod[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    for (int k = 0; k < 4; ++k) ((double*)(R + HB_SUMMARY))[k] = 0.0;
}

__global__ __launch_bounds__(64) void k_fpg_add_keyframes(char* store, Lay L, const unsigned char* __restrict__ key, const double* __restrict__ pose,
                                                          const double* __restrict__ stamp, const unsigned char* __restrict__ mask,
                                                          unsigned char* __restrict__ added) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b)) return;
    if (!key[b]) {
        if (added) added[b] = 0;
        return;
    }
    char* R = region(store, L, b);
    int* hdr = (int*)R;
    const int n = hdr[H_NKF];
    if (n >= L.K) {
        hdr[H_FULL] = 1;
        if (added) added[b] = 0;
        return;
    }
    const Iso<CR> T = tf_of_pose(pose + (size_t)b * 6);
    double* tfs = (double*)(R + L.r_tf);
    store_tf(T, tfs + (size_t)n * 12);
    pose_of_tf(mul(load_tf((const double*)(R + HB_MOD)), T), (double*)(R + L.r_pose) + (size_t)n * 6);
    if (n > 0) store_tf(mul(inverse(load_tf(tfs + (size_t)(n - 1) * 12)), T), (double*)(R + L.r_seq) + (size_t)n * 12);
    ((double*)(R + L.r_stamp))[n] = stamp[b];
    hdr[H_NKF] = n + 1;
    if (added) added[b] = 1;
}

__global__ __launch_bounds__(64) void k_fpg_add_loops(char* store, Lay L, const unsigned char* __restrict__ found, const int* __restrict__ edge,
                                                      const double* __restrict__ tf12, const unsigned char* __restrict__ mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b) || !found[b]) return;
    char* R = region(store, L, b);
    int* hdr = (int*)R;
    const int n = hdr[H_NKF], i1 = edge[(size_t)b * 3], i2 = edge[(size_t)b * 3 + 1];
    if (i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || i1 == i2) { hdr[H_BAD] = 1; return; }
    const int nl = hdr[H_NLOOP];
    if (nl >= L.ML) { hdr[H_LFULL] = 1; return; }
    int* lidx = (int*)(R + L.r_lidx);
    lidx[2 * nl] = i1; lidx[2 * nl + 1] = i2;
    double* ltf = (double*)(R + L.r_ltf) + (size_t)nl * 12;
    for (int k = 0; k < 12; ++k) ltf[k] = tf12[(size_t)b * 12 + k];
    hdr[H_NLOOP] = nl + 1;
    hdr[H_PEND] = 1;
}

// one work-group: due flags and their count (a block sum of integers)
__global__ __launch_bounds__(256) void k_fpg_due(char* store, Lay L, double period, const unsigned char* __restrict__ key, const double* __restrict__ stamp,
                                                 const unsigned char* __restrict__ mask, unsigned char* __restrict__ due, int* n_due) {
    __shared__ int red[256];
    int cnt = 0;
    for (int b = threadIdx.x; b < L.B; b += 256) {
        if (!robot_on(mask, b)) continue;
        const char* R = region(store, L, b);
        const int* hdr = (const int*)R;
        const bool d = key[b] != 0 && hdr[H_PEND] != 0 && stamp[b] - *(const double*)(R + HB_TLAST) > period;
        due[b] = d ? 1 : 0;
        cnt += d ? 1 : 0;
    }
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0 && n_due) *n_due = red[0];
}

__global__ __launch_bounds__(64) void k_fpg_correct(char* store, Lay L, const double* __restrict__ pose_in, double* __restrict__ pose_out,
                                                    const unsigned char* __restrict__ mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b)) return;
    const char* R = region(store, L, b);
    pose_of_tf(mul(load_tf((const double*)(R + HB_MOD)), tf_of_pose(pose_in + (size_t)b * 6)), pose_out + (size_t)b * 6);
}

// ------------------------------------------------------------------------------------------------------------- solve
struct Wk {   // a robot's work block
    Lm* lm; double *x, *cand, *y, *scale, *dgn, *Ye, *Yg, *Dd, *gd, *Os, *Lb, *Sred, *rec, *Hr, *rhs; int *sep, *sepidx;
};
__device__ __forceinline__ Wk work_of(char* store, const Lay& L, int b) {
    char* W = workblk(store, L, b);
    Wk w;
    w.lm = (Lm*)W;
    w.x = (double*)(W + L.w_x); w.cand = (double*)(W + L.w_cand); w.y = (double*)(W + L.w_y); w.scale = (double*)(W + L.w_scale);
    w.dgn = (double*)(W + L.w_dgn); w.Ye = (double*)(W + L.w_Ye); w.Yg = (double*)(W + L.w_Yg); w.Dd = (double*)(W + L.w_Dd);
    w.gd = (double*)(W + L.w_gd); w.Os = (double*)(W + L.w_Os); w.Lb = (double*)(W + L.w_Lb); w.Sred = (double*)(W + L.w_Sred);
    w.rec = (double*)(W + L.w_rec); w.Hr = (double*)(W + L.w_Hr); w.rhs = (double*)(W + L.w_rhs);
    w.sep = (int*)(W + L.w_sep); w.sepidx = (int*)(W + L.w_sepidx);
    return w;
}

__global__ __launch_bounds__(64) void k_fpg_setup(char* store, Lay L, const unsigned char* __restrict__ sel) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const char* R = region(store, L, b);
    const int* hdr = (const int*)R;
    Wk w = work_of(store, L, b);
    const int N = hdr[H_NKF], nl = hdr[H_NLOOP];
    if (!sel[b] || N < 2) {
        if (lane == 0) w.lm->done = 1;
        return;
    }
    const double* ps = (const double*)(R + L.r_pose);
    for (int i = lane; i < 6 * N; i += 64) { const double v = ps[i]; w.x[i] = v; w.cand[i] = v; w.y[i] = 0.0; }
    const int* lidx = (const int*)(R + L.r_lidx);
    int base = 0;
    for (int f0 = 0; f0 < N; f0 += 64) {
        const int f = f0 + lane;
        bool flag = f < N && (f == 0 || f == N - 1 || f % PG_STRIDE == 0);
        if (f < N && !flag)
            for (int l = 0; l < nl; ++l) flag = flag || lidx[2 * l] == f || lidx[2 * l + 1] == f;
        const unsigned long long m = __ballot(flag);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (f < N) w.sepidx[f] = flag ? base + rank : -1;
        if (flag) w.sep[base + rank] = f;
        base += __popcll(m);
    }
    if (lane == 0) {
        Lm s;
        pg_lm_start(s, 0);
        s.ns = base; s.N = N; s.nl = nl; s.status = 0;
        *w.lm = s;
    }
}

// Y of edge slot e [6][13] = [J | r], of key frame f [2][7]; which = 0: at x for robots in PH_INIT, 1: at the candidate for PH_CAND
__global__ __launch_bounds__(64) void k_fpg_linearize(char* store, Lay L, Noise noise, DevParams P, int which) {
    __shared__ double Y[4][6 * 13];
    const int lane = threadIdx.x & 63, grp = lane >> 4, d = lane & 15;
    const long long edge_slots = (long long)L.B * L.NE;
    const long long edge_blocks = (edge_slots + 3) / 4;
    const int want = which ? PH_CAND : PH_INIT;
    if ((long long)blockIdx.x < edge_blocks) {
        const long long slot = (long long)blockIdx.x * 4 + grp;
        const int b = slot < edge_slots ? (int)(slot / L.NE) : 0, e = (int)(slot % L.NE);
        Wk w = work_of(store, L, b);
        const char* R = region(store, L, b);
        bool on = slot < edge_slots && !w.lm->done && w.lm->phase == want;
        int i = 0, j = 0;
        const double* tf = nullptr;
        double weight = 1.0;
        if (on) {
            const int N = w.lm->N, nl = w.lm->nl;
            if (e < L.K - 1) {
                on = e < N - 1;
                i = e; j = e + 1;
                tf = (const double*)(R + L.r_seq) + (size_t)(e + 1) * 12;
            } else {
                const int l = e - (L.K - 1);
                on = l < nl;
                if (on) { i = ((const int*)(R + L.r_lidx))[2 * l]; j = ((const int*)(R + L.r_lidx))[2 * l + 1]; }
                tf = (const double*)(R + L.r_ltf) + (size_t)l * 12;
                weight = noise.loop_edge_k;
            }
        }
        const double* x = which ? w.cand : w.x;
        const double* xi = x + (size_t)i * 6;
        const double* xj = x + (size_t)j * 6;
        if (on) pg_edge_column(tf, weight, noise.J, xi, xj, d, true, Y[grp]);
        __syncthreads();
        if (on && d < 12) {   // local parameterisation: J_theta <- J_theta * dPlus/ddelta  (lane = (row r, pose which))
            const int r = d % 6, side = d / 6;
            pg_row_times_plus_jac(&Y[grp][r * 13 + 6 * side + 3], (side ? xj : xi) + 3);
        }
        __syncthreads();
        if (on && d < 13)
#pragma unroll
            for (int r = 0; r < 6; ++r) w.Ye[(size_t)e * 78 + r * 13 + d] = Y[grp][r * 13 + d];
    } else {
        // ground factors: 8 key frames per wave, 6 dual directions + value
        const int sub = lane >> 3, dir = lane & 7;
        const long long slot = ((long long)blockIdx.x - edge_blocks) * 8 + sub;
        const long long slots = (long long)L.B * L.K;
        const int b = slot < slots ? (int)(slot / L.K) : 0, f = (int)(slot % L.K);
        Wk w = work_of(store, L, b);
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

// wave per (robot, key frame), for robots in PH_INIT or PH_ASM.  Key frame 0 is the constant one: identity block, zero gradient.
__global__ __launch_bounds__(64) void k_fpg_assemble(char* store, Lay L) {
    const int b = blockIdx.x / L.K, i = blockIdx.x % L.K, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, b);
    if (w.lm->done || (w.lm->phase != PH_INIT && w.lm->phase != PH_ASM)) return;
    const int N = w.lm->N, nl = w.lm->nl;
    if (i >= N) return;
    const int* lidx = (const int*)(region(store, L, b) + L.r_lidx);
    const double *Ye = w.Ye, *Yg = w.Yg;
    const int r = lane / 6, c = lane % 6;
    double acc = 0.0;
    const bool is_const = i == 0;
    if (!is_const) {
        acc = pg_node_ground(Yg + (size_t)i * 14, lane);
    }
    // incident edges in edge order: sequential i-1 (side 1), sequential i (side 0), then the loops that name i
    const int n_inc = 2 + nl;
    for (int t = 0; t < n_inc; ++t) {
        int e, side, j;
        if (t == 0) { if (i == 0) continue; e = i - 1; side = 1; j = i - 1; }
        else if (t == 1) { if (i >= N - 1) continue; e = i; side = 0; j = i + 1; }
        else {
            const int l = t - 2, i1 = lidx[2 * l], i2 = lidx[2 * l + 1];
            if (i1 == i) { side = 0; j = i2; } else if (i2 == i) { side = 1; j = i1; } else continue;
            e = L.K - 1 + l;
        }
        const double* Y = Ye + (size_t)e * 78;
        if (!is_const) {
            acc += pg_node_edge(Y, side, lane);
        }
        if (side == 0 && lane < 36) {   // H[index1, index2](r, c) = sum_k J1[k][r] J2[k][c]; zero against the constant key frame
            const double o = !is_const && j != 0 ? pg_edge_cross(Y, lane) : 0.0;
            if (t == 1) w.Os[(size_t)i * 36 + lane] = o;
            else w.Lb[(size_t)(t - 2) * 36 + lane] = o;
        }
    }
    if (i == N - 1 && lane < 36) w.Os[(size_t)i * 36 + lane] = 0.0;
    if (is_const && lane < 36) acc = r == c ? 1.0 : 0.0;
    if (lane < 36) w.Dd[(size_t)i * 36 + lane] = acc;
    else if (lane < 42) w.gd[i * 6 + (lane - 36)] = acc;
}

// 1/2 sum r^2 of the robot's blocks in Ye / Yg (the constant key frame's ground block is not part of the cost), by one wave
__device__ __forceinline__ double cost_of(const Lay& L, const Wk& w, int N, int nl, int lane) {
    double s = 0.0;
    for (int e = lane; e < N - 1; e += 64)
#pragma unroll
        for (int r = 0; r < 6; ++r) { const double v = w.Ye[(size_t)e * 78 + r * 13 + 12]; s += v * v; }
    for (int l = lane; l < nl; l += 64)
#pragma unroll
        for (int r = 0; r < 6; ++r) { const double v = w.Ye[(size_t)(L.K - 1 + l) * 78 + r * 13 + 12]; s += v * v; }
    for (int f = 1 + lane; f < N; f += 64) { const double a = w.Yg[(size_t)f * 14 + 6], c = w.Yg[(size_t)f * 14 + 13]; s += a * a; s += c * c; }
    return 0.5 * wave_sum(s);
}


// the robot is done: poses, summary and keyframe_manager's commit after a solve (mirror :178-188)
__device__ __forceinline__ void finish(char* store, const Lay& L, int b, const Wk& w, int term, const double* stamp, liw_summary* summary, int lane) {
    char* R = region(store, L, b);
    const int N = w.lm->N;
    double* ps = (double*)(R + L.r_pose);
    for (int i = lane; i < 6 * N; i += 64) ps[i] = w.x[i];
    if (lane == 0) {
        liw_summary sm;
        sm.iterations = w.lm->iter; sm.successful_steps = w.lm->succ; sm.termination = term; sm.initial_cost = w.lm->init_cost; sm.final_cost = w.lm->x_cost;
        *(liw_summary*)(R + HB_SUMMARY) = sm;
        summary[b] = sm;
        const Iso<CR> cur = tf_of_pose(w.x + (size_t)(N - 1) * 6);
        const Iso<CR> last = load_tf((const double*)(R + L.r_tf) + (size_t)(N - 1) * 12);
        store_tf(mul(cur, inverse(last)), (double*)(R + HB_MOD));
        int* hdr = (int*)R;
        hdr[H_PEND] = 0;
        hdr[H_SOLVES] += 1;
        *(double*)(R + HB_TLAST) = stamp[b];
        w.lm->term = term;
        w.lm->done = 1;
    }
}

__global__ __launch_bounds__(64) void k_fpg_head(char* store, Lay L, int max_iters, const double* __restrict__ stamp, liw_summary* summary) {
    const int b = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, b);
    if (w.lm->done) return;
    Lm s = *w.lm;
    const int term = pg_lm_head(s, PgConstFirst(), [&] { return cost_of(L, w, s.N, s.nl, lane); }, s.N, max_iters, w.x, w.gd, w.Dd, w.scale, w.dgn, lane);
    if (term) {
        if (lane == 0) *w.lm = s;
        finish(store, L, b, w, term, stamp, summary, lane);
        return;
    }
    s.status = 0;
    if (lane == 0) *w.lm = s;
}

__global__ __launch_bounds__(64) void k_fpg_seg_elim(char* store, Lay L) {
    const int nsg = L.NS - 1;
    const int b = blockIdx.x / nsg, sg = blockIdx.x % nsg, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, b);
    if (w.lm->done || w.lm->phase != PH_SOLVE || sg >= w.lm->ns - 1) return;
    const int a = w.sep[sg], bb = w.sep[sg + 1];
    const bool ok = pg_seg_elim_wave(a, bb, lane, w.Dd, w.gd, w.Os, w.scale, w.dgn, w.lm->radius, w.Sred + (size_t)sg * PG_SEG, w.rec);
    if (!ok && lane == 0) atomicOr(&w.lm->status, 1);
}


// work-group per robot: the separators' system A y = g_s (as k_pg_reduced + k_pg_reduced_loops build it), Cholesky, both solves, scatter
__global__ __launch_bounds__(256) void k_fpg_reduced(char* store, Lay L, int lds_doubles) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    Wk w = work_of(store, L, b);
    if (w.lm->done || w.lm->phase != PH_SOLVE) return;
    const int ns = w.lm->ns, nr = 6 * ns;
    double* A = nr * (nr + 1) / 2 <= lds_doubles ? lds : w.Hr;   // the same instructions either way
    double* rhs = w.rhs;
    const int* sep = w.sep;
    pg_reduced_system(A, rhs, ns, w.lm->nl, 0, sep, w.sepidx, (const int*)(region(store, L, b) + L.r_lidx), nullptr, w.Dd, w.gd, w.Os, w.Lb, w.Sred, w.scale,
                      w.dgn, w.lm->radius, tid);
#include "k_pg_chol_body.inc"
    for (int e = tid; e < nr; e += 256) w.y[(size_t)sep[e / 6] * 6 + e % 6] = rhs[e];
    if (!ok && tid == 0) atomicOr(&w.lm->status, 1);
}

__global__ __launch_bounds__(64) void k_fpg_backsub(char* store, Lay L) {
    const int nsg = L.NS - 1;
    const int b = blockIdx.x / nsg, sg = blockIdx.x % nsg, lane = threadIdx.x & 63;
    Wk w = work_of(store, L, b);
    if (w.lm->done || w.lm->phase != PH_SOLVE || sg >= w.lm->ns - 1) return;
    pg_seg_backsub_wave(w.sep[sg], w.sep[sg + 1], lane, w.rec, w.y);
}

// Its own copy of pg_lm_decide1 with PgConstFirst: through the shared function the kernel takes 74 VGPRs for 72 and drops from 7 waves
// per SIMD to 6 (the same text inlined by hand keeps 72).  A change to pg_lm_decide1 belongs here too.
__global__ __launch_bounds__(64) void k_fpg_decide1(char* store, Lay L, const double* __restrict__ stamp, liw_summary* summary) {
    const int b = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, b);
    if (w.lm->done || w.lm->phase != PH_SOLVE) return;
    Lm s = *w.lm;
    const int N = s.N, n = 6 * N;
    bool fin = true;
    for (int i = lane; i < n; i += 64) fin = fin && isfinite(w.y[i]);
    const bool solved = s.status == 0 && __ballot(!fin) == 0ull;
    // model cost change with (A + D^2) y = g_s, step = -y:  (y'g_s + y'D^2 y) / 2
    double mcc = 0.0;
    if (solved) {
        double ytg = 0.0, dsum = 0.0;
        for (int i = 6 + lane; i < n; i += 64) {
            const double yi = w.y[i];
            ytg += yi * (w.gd[i] * w.scale[i]);
            dsum += w.dgn[i] / s.radius * yi * yi;
        }
        mcc = 0.5 * (wave_sum(ytg) + wave_sum(dsum));
    }
    if (!lm_step_valid(solved, mcc)) {
        if (lm_gives_up(s.invalid++)) {
            --s.iter;
            if (lane == 0) *w.lm = s;
            finish(store, L, b, w, 6, stamp, summary, lane);
            return;
        }
        lm_step_rejected(s.radius, s.dec, s.reuse);
        s.last_ok = 0;
        s.phase = PH_IDLE;
        if (lane == 0) *w.lm = s;
        return;
    }
    s.invalid = 0;
    s.mcc = mcc;
    double sq = 0.0;
    for (int f = 1 + lane; f < N; f += 64) {
        double dl[6], xc[6];
        for (int k = 0; k < 6; ++k) dl[k] = -w.y[f * 6 + k] * w.scale[f * 6 + k];
        plus6(w.x + (size_t)f * 6, dl, xc);
        for (int k = 0; k < 6; ++k) {
            w.cand[f * 6 + k] = xc[k];
            const double df = w.x[f * 6 + k] - xc[k];
            sq += df * df;
        }
    }
    s.step_norm = sqrt(wave_sum(sq));
    s.phase = PH_CAND;
    if (lane == 0) *w.lm = s;
}

__global__ __launch_bounds__(64) void k_fpg_decide2(char* store, Lay L, const double* __restrict__ stamp, liw_summary* summary) {
    const int b = blockIdx.x, lane = threadIdx.x;
    Wk w = work_of(store, L, b);
    if (w.lm->done || w.lm->phase != PH_CAND) return;
    Lm s = *w.lm;
    const int term = pg_lm_decide2(s, cost_of(L, w, s.N, s.nl, lane), s.N, w.x, w.cand, lane);
    if (term) {
        finish(store, L, b, w, term, stamp, summary, lane);
        return;
    }
    if (lane == 0) *w.lm = s;
}

// robots still iterating (a sum of integers by one work-group)
__global__ __launch_bounds__(256) void k_fpg_count(char* store, Lay L) {
    __shared__ int red[256];
    int cnt = 0;
    for (int b = threadIdx.x; b < L.B; b += 256) cnt += ((const Lm*)workblk(store, L, b))->done ? 0 : 1;
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) *(int*)(store + L.g_count) = red[0];
}

// ------------------------------------------------------------------------------------------------------------- launches
int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fpg_reset, dim3((L.B + 255) / 256), dim3(256), 0, s, store, L, mask);
    return launched();
}
int launch_add_keyframes(char* store, const Lay& L, const unsigned char* key, const double* pose, const double* stamp, const unsigned char* mask,
                         unsigned char* added, hipStream_t s) {
    hipLaunchKernelGGL(k_fpg_add_keyframes, dim3((L.B + 63) / 64), dim3(64), 0, s, store, L, key, pose, stamp, mask, added);
    return launched();
}
int launch_add_loops(char* store, const Lay& L, const unsigned char* found, const int* edge, const double* tf12, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fpg_add_loops, dim3((L.B + 63) / 64), dim3(64), 0, s, store, L, found, edge, tf12, mask);
    return launched();
}
int launch_due(char* store, const Lay& L, double period, const unsigned char* key, const double* stamp, const unsigned char* mask, unsigned char* due,
               int* n_due, hipStream_t s) {
    hipLaunchKernelGGL(k_fpg_due, dim3(1), dim3(256), 0, s, store, L, period, key, stamp, mask, due, n_due);
    return launched();
}
int launch_correct(char* store, const Lay& L, const double* pose_in, double* pose_out, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_fpg_correct, dim3((L.B + 63) / 64), dim3(64), 0, s, store, L, pose_in, pose_out, mask);
    return launched();
}

int launch_solve(char* store, const Lay& L, const Noise& noise, const DevParams& P, const unsigned char* sel, const double* stamp, int max_iters,
                 int check_every, int lds_cap_doubles, liw_summary* summary, hipStream_t s) {
    const int K = max_iters > 0 ? max_iters : 50;
    const unsigned B = (unsigned)L.B;
    const unsigned lin_blocks = (unsigned)(((long long)L.B * L.NE + 3) / 4 + ((long long)L.B * L.K + 7) / 8);
    const unsigned asm_blocks = B * (unsigned)L.K, seg_blocks = B * (unsigned)(L.NS > 1 ? L.NS - 1 : 0);
    // LDS for the separator systems: what the largest one of this store needs, 64 KB at the most (two work-groups per CU); a robot
    // whose own triangle is larger than that runs from its work area
    const int nr = 6 * L.NS, tri_max = nr * (nr + 1) / 2;
    const int lds_doubles = tri_max <= lds_cap_doubles ? tri_max : lds_cap_doubles;
    hipLaunchKernelGGL(k_fpg_setup, dim3(B), dim3(64), 0, s, store, L, sel);
    hipLaunchKernelGGL(k_fpg_linearize, dim3(lin_blocks), dim3(64), 0, s, store, L, noise, P, 0);
    hipLaunchKernelGGL(k_fpg_assemble, dim3(asm_blocks), dim3(64), 0, s, store, L);
    for (int it = 0; it < K; ++it) {
        hipLaunchKernelGGL(k_fpg_head, dim3(B), dim3(64), 0, s, store, L, K, stamp, summary);
        if (seg_blocks) hipLaunchKernelGGL(k_fpg_seg_elim, dim3(seg_blocks), dim3(64), 0, s, store, L);
        hipLaunchKernelGGL(k_fpg_reduced, dim3(B), dim3(256), sizeof(double) * (size_t)lds_doubles, s, store, L, lds_doubles);
        if (seg_blocks) hipLaunchKernelGGL(k_fpg_backsub, dim3(seg_blocks), dim3(64), 0, s, store, L);
        hipLaunchKernelGGL(k_fpg_decide1, dim3(B), dim3(64), 0, s, store, L, stamp, summary);
        hipLaunchKernelGGL(k_fpg_linearize, dim3(lin_blocks), dim3(64), 0, s, store, L, noise, P, 1);
        hipLaunchKernelGGL(k_fpg_decide2, dim3(B), dim3(64), 0, s, store, L, stamp, summary);
        hipLaunchKernelGGL(k_fpg_assemble, dim3(asm_blocks), dim3(64), 0, s, store, L);
        if (launched()) return -1;
        if (check_every > 0 && (it + 1) % check_every == 0 && it + 1 < K) {
            int left = 0;
            hipLaunchKernelGGL(k_fpg_count, dim3(1), dim3(256), 0, s, store, L);
            if (hipMemcpyAsync(&left, store + L.g_count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return -1;
            if (left == 0) return 0;
        }
    }
    hipLaunchKernelGGL(k_fpg_head, dim3(B), dim3(64), 0, s, store, L, K, stamp, summary);   // the iteration cap (termination 4) of who is left
    return launched();
}

}  // namespace liw_fpg_dev
