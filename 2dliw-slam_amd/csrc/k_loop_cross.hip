// k_loop_cross.hip — cross-robot loop detection of the fleet (C ABI include/liw_loop_cross.h, host side liw_loop_cross.cpp): the
// kernels of k_loop_batch.hip's detection with the query side in one robot region and the candidate side in another, a frame-free
// residual gate in place of the tracking-pose gates, and the partner / link kernels that chain accepted edges into T_g_w.
//
// liw_xloop_detect:
//   k_xloop_gates     one wave per query robot a, a lane per candidate i = 0, s, ... < K_b of its partner b: the null / points gates,
//                     the five draws, the rank among a's launched candidates by ballot prefix (64 candidates at a time).
//   k_floop_scan      of k_loop_batch.hip, unchanged: the pair list's bases, the pair total, max n2.
//   k_xloop_pairs     a lane per (robot, candidate): the compact XPair list in robot-then-candidate order.
//   k_xloop_match     match_rows of k_loop_dev.hpp on the fixed grid: the drawn query row from a's region, the candidate rows from b's.
//   k_xloop_select    a wave strides over pairs: select_best of k_loop_dev.hpp.
//   k_xloop_icp       a lane per pair above min_match: k_floop_icp's closed form with tf_a[q] and tf_b[i], then the residual.
//   k_xloop_choose    one wave per robot: max-reduction over (size, -candidate) of the passing pairs, the stats, T_w1_w2.
// liw_xloop_partner:  k_xloop_partner, a wave per robot counts and picks the linked members of its group with ballots.
// liw_xloop_link:     k_xloop_decide (a wave per robot, reads the flags of before the call, stages its decision in group_linked[r])
//                     and k_xloop_apply (a lane per robot composes and writes only its own entries).
// No global atomics; positions come from prefix counts; results are reproducible bit for bit.
#pragma clang fp contract(off)   // T_w1_w2 and T_g_w are liw_lie_mul's products bit for bit

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/liw_loop_cross.h"
#include "k_loop_cross.hpp"
#include "k_loop_dev.hpp"
#include "liw_crmath.hpp"
#include "liw_dual.hpp"

namespace liw_xloop_dev {

using liw_floop_dev::feature_slot;
using liw_floop_dev::Pre;
using liw_loop_dev::Geom;
using liw_loop_dev::kRowsPerBlock;
using liw_loop_dev::match_rows;
using liw_loop_dev::select_best;

using IsoD = liw::Iso<double>;

__device__ __forceinline__ const char* region(const char* store, const Lay& L, int b) { return store + (size_t)b * L.robot_bytes; }
__device__ __forceinline__ bool robot_on(const unsigned char* a, int b) { return !a || a[b] != 0; }
__device__ __forceinline__ IsoD load_iso(const double* T) { return liw::cast_iso<double>(T, T + 9); }
__device__ __forceinline__ void store_iso(const IsoD& A, double* T) {
    for (int k = 0; k < 9; ++k) T[k] = A.R.m[k];
    T[9] = A.t.x; T[10] = A.t.y; T[11] = A.t.z;
}

__global__ __launch_bounds__(64) void k_xloop_gates(char* store, Lay L, Prm p, const unsigned char* __restrict__ key, const int* __restrict__ partner,
                                                    const unsigned char* __restrict__ mask, unsigned char* __restrict__ found, int* __restrict__ edge,
                                                    long long* __restrict__ stats) {
    const int a = blockIdx.x, lane = threadIdx.x;
    int* cnt = (int*)(store + L.f_cnt);
    int* cmax = (int*)(store + L.f_cmax);
    if (!robot_on(mask, a) || !key[a]) {
        if (lane == 0) {
            cnt[a] = 0;
            cmax[a] = 0;
            if (robot_on(mask, a)) found[a] = 0;
        }
        return;
    }
    const int b = partner[a];
    int nvis = 0, total = 0, n2max = 0;
    long long tasks = 0;
    if (b >= 0 && b < L.B && b != a) {
        const char* Ra = region(store, L, a);
        const char* Rb = region(store, L, b);
        const int Ka = ((const int*)Ra)[0], Kb = ((const int*)Rb)[0];
        const int q = Ka - 1;
        if (Ka > 0 && Ka <= L.K && Kb > 0 && Kb <= L.K && ((const int*)(Ra + L.r_state))[q] == LIW_LOOP_VALID) {
            const int* state = (const int*)(Rb + L.r_state);
            const int* npts = (const int*)(Rb + L.r_npts);
            nvis = (Kb + L.step - 1) / L.step;          // <= NC, as Kb <= max_keyframes
            const int n1 = ((const int*)(Ra + L.r_npts))[q], thr = p.g.thr;
            Pre* pre = (Pre*)(store + L.f_pre) + (size_t)a * L.NC;
            for (int c0 = 0; c0 < L.NC; c0 += 64) {
                const int ci = c0 + lane, i = ci * L.step;
                bool ok = false;
                int n2 = 0;
                if (ci < nvis && state[i] == LIW_LOOP_VALID) {
                    n2 = npts[i];
                    ok = !(n1 < thr || n2 < thr || n1 == 0 || n2 == 0);
                }
                const unsigned long long bal = __ballot(ok);
                if (ci < L.NC) {
                    Pre* x = pre + ci;
                    x->rank = ok ? total + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
                    x->n2 = n2;
                    if (ok) {
                        int r0 = -1, r1 = -1, r2 = -1, r3 = -1, r4 = -1;
                        for (int d = 0; d < kDraws; ++d) {
                            int row = liw_loop_dev::draw_row(p.seed, q, i, d, n1);
                            if (row == r0 || row == r1 || row == r2 || row == r3) row = -1;
                            if (d == 0) r0 = row; else if (d == 1) r1 = row; else if (d == 2) r2 = row; else if (d == 3) r3 = row; else r4 = row;
                            tasks += row >= 0 ? n2 : 0;
                        }
                        x->rows[0] = r0; x->rows[1] = r1; x->rows[2] = r2; x->rows[3] = r3; x->rows[4] = r4;
                        n2max = n2 > n2max ? n2 : n2max;
                    }
                }
                total += __popcll(bal);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        tasks += __shfl_xor(tasks, o, 64);
        const int x = __shfl_xor(n2max, o, 64);
        n2max = x > n2max ? x : n2max;
    }
    if (lane == 0) {
        cnt[a] = total;
        cmax[a] = n2max;
        found[a] = 0;
        int* e = edge + 4 * (size_t)a;
        e[0] = -1; e[1] = -1; e[2] = -1; e[3] = 0;
        long long* st = stats + (size_t)a * 6;
        st[0] = nvis; st[1] = total; st[2] = tasks; st[3] = 0; st[4] = 0; st[5] = 0;
    }
}

__global__ __launch_bounds__(256) void k_xloop_pairs(char* store, Lay L, const int* __restrict__ partner) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)L.B * L.NC) return;
    const int a = (int)(idx / L.NC), ci = (int)(idx - (long long)a * L.NC);
    if (((const int*)(store + L.f_cnt))[a] == 0) return;   // the robot's Pre records are this call's only when it launched something
    const Pre* x = (const Pre*)(store + L.f_pre) + idx;
    if (x->rank < 0) return;
    const char* Ra = region(store, L, a);
    const int K = ((const int*)Ra)[0];
    XPair* o = (XPair*)(store + L.f_pairs) + ((const int*)(store + L.f_base))[a] + x->rank;
    o->robot = a;
    o->partner = partner[a];                                // in range: the gates launched the pair
    o->cand = ci * L.step;
    o->query = K - 1;
    o->n1 = ((const int*)(Ra + L.r_npts))[K - 1];
    o->n2 = x->n2;
    for (int d = 0; d < kDraws; ++d) o->rows[d] = x->rows[d];
    o->pad = 0;
}

__global__ __launch_bounds__(256) void k_xloop_match(char* store, Lay L, Geom g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int* hdr = (const int*)(store + L.f_hdr);
    const int npairs = hdr[0], rb = (hdr[1] + kRowsPerBlock - 1) / kRowsPerBlock;
    const long long items = (long long)npairs * kDraws * rb;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int pi = (int)(item / (kDraws * rb)), rem = (int)(item - (long long)pi * kDraws * rb);
        const int d = rem / rb, r0 = (rem - d * rb) * kRowsPerBlock;
        const XPair* c = (const XPair*)(store + L.f_pairs) + pi;
        const int n1 = c->n1, n2 = c->n2, row1 = c->rows[d];
        if (r0 >= n2) continue;
        int2* out = (int2*)(store + L.f_tres) + ((size_t)pi * kDraws + d) * L.P;
        if (row1 < 0) {   // a repeated draw: no task
            for (int r = r0 + threadIdx.x; r < n2 && r < r0 + kRowsPerBlock; r += blockDim.x) out[r] = make_int2(0, 0);
            continue;
        }
        const char* Ra = region(store, L, c->robot);
        const char* Rb = region(store, L, c->partner);
        const size_t qrow = (size_t)feature_slot(L, c->query) * L.P + row1;
        const size_t cslot = (size_t)feature_slot(L, c->cand) * L.P;
        match_rows(n1, n2, r0, (const uint32_t*)(Ra + L.r_keys) + qrow * L.P, (const double*)(Ra + L.r_aij) + qrow * L.P,
                   (const uint64_t*)(Ra + L.r_quick) + qrow * L.W, (const uint32_t*)(Rb + L.r_keys) + cslot * L.P,
                   (const double*)(Rb + L.r_aij) + cslot * L.P, (const uint64_t*)(Rb + L.r_quick) + cslot * L.W, g, smem, out);
    }
}

__global__ __launch_bounds__(64) void k_xloop_select(char* store, Lay L, Geom g) {
    const int npairs = ((const int*)(store + L.f_hdr))[0];
    for (int pi = blockIdx.x; pi < npairs; pi += gridDim.x) {
        const XPair* c = (const XPair*)(store + L.f_pairs) + pi;   // read through the pointer, as Pair in k_loop_batch.hip
        const char* Ra = region(store, L, c->robot);
        const char* Rb = region(store, L, c->partner);
        const size_t qs = (size_t)feature_slot(L, c->query) * L.P * L.P, cs = (size_t)feature_slot(L, c->cand) * L.P * L.P;
        select_best(c->rows, c->n1, c->n2, (const int2*)(store + L.f_tres) + (size_t)pi * kDraws * L.P, (const uint32_t*)(Ra + L.r_keys) + qs,
                    (const double*)(Ra + L.r_aij) + qs, (const uint32_t*)(Rb + L.r_keys) + cs, (const double*)(Rb + L.r_aij) + cs, g,
                    (int*)(store + L.f_summary) + (size_t)pi * 8, (int*)(store + L.f_lists) + (size_t)pi * L.P * 2);
    }
}

__device__ __forceinline__ void apply_xy(const IsoD& A, const double* x, double& ox, double& oy) {   // liw_lie_apply, z dropped
    const liw::V3<double> r = liw::mul(A.R, liw::V3<double>(x[0], x[1], x[2]));
    ox = r.x + A.t.x;
    oy = r.y + A.t.y;
}

// k_floop_icp's closed form over one accepted pair, with the two poses from two robots; then the residual of the planar pairs
__global__ __launch_bounds__(64) void k_xloop_icp(char* store, Lay L, Prm p, XPrm xp) {
    const int npairs = ((const int*)(store + L.f_hdr))[0];
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= npairs) return;
    XRes* res = (XRes*)(store + L.f_res) + pi;
    const int* sm = (const int*)(store + L.f_summary) + (size_t)pi * 8;
    const int size = sm[0], len = sm[5];
    if (size <= xp.min_match || len != size || len > L.P) {   // min_match >= thr: a pair above it has its list
        res->rms = -1.0;
        return;
    }
    const XPair* c = (const XPair*)(store + L.f_pairs) + pi;
    const char* Ra = region(store, L, c->robot);
    const char* Rb = region(store, L, c->partner);
    const IsoD f1 = load_iso((const double*)(Ra + L.r_tf) + (size_t)c->query * 12), f2 = load_iso((const double*)(Rb + L.r_tf) + (size_t)c->cand * 12);
    const IsoD Tiw = load_iso(p.Tiw);
    const IsoD inv1 = liw::inverse(liw::mul(f1, Tiw)), inv2 = liw::inverse(liw::mul(f2, Tiw)), inv_iw = liw::inverse(Tiw);
    const double* P1 = (const double*)(Ra + L.r_pts) + (size_t)feature_slot(L, c->query) * L.P * 3;
    const double* P2 = (const double*)(Rb + L.r_pts) + (size_t)feature_slot(L, c->cand) * L.P * 3;
    const int* Ls = (const int*)(store + L.f_lists) + (size_t)pi * L.P * 2;
    double c1x = 0, c1y = 0, c2x = 0, c2y = 0;
    for (int k = 0; k < len; ++k) {
        double ax, ay, bx, by;
        apply_xy(inv1, P1 + (size_t)Ls[2 * k] * 3, ax, ay);
        apply_xy(inv2, P2 + (size_t)Ls[2 * k + 1] * 3, bx, by);
        c1x += ax; c1y += ay; c2x += bx; c2y += by;
    }
    c1x /= len; c1y /= len; c2x /= len; c2y /= len;
    double sdot = 0, scross = 0;
    for (int k = 0; k < len; ++k) {
        double p1x, p1y, p2x, p2y;
        apply_xy(inv1, P1 + (size_t)Ls[2 * k] * 3, p1x, p1y);
        apply_xy(inv2, P2 + (size_t)Ls[2 * k + 1] * 3, p2x, p2y);
        const double ax = p1x - c1x, ay = p1y - c1y, bx = p2x - c2x, by = p2y - c2y;
        sdot += ax * bx + ay * by;
        scross += bx * ay - by * ax;
    }
    const double yaw = liw_cr::cr_atan2(scross, sdot), cs = liw_cr::cr_cos(yaw), sn = liw_cr::cr_sin(yaw);
    const double tx = c1x - (cs * c2x - sn * c2y), ty = c1y - (sn * c2x + cs * c2y);
    double ss = 0;
    for (int k = 0; k < len; ++k) {
        double p1x, p1y, p2x, p2y;
        apply_xy(inv1, P1 + (size_t)Ls[2 * k] * 3, p1x, p1y);
        apply_xy(inv2, P2 + (size_t)Ls[2 * k + 1] * 3, p2x, p2y);
        const double dx = p1x - ((cs * p2x - sn * p2y) + tx), dy = p1y - ((sn * p2x + cs * p2y) + ty);
        ss += dx * dx + dy * dy;
    }
    IsoD w;
    w.R.m[0] = cs; w.R.m[1] = -sn; w.R.m[2] = 0; w.R.m[3] = sn; w.R.m[4] = cs; w.R.m[5] = 0; w.R.m[6] = 0; w.R.m[7] = 0; w.R.m[8] = 1;
    w.t = liw::V3<double>(tx, ty, 0.0);
    store_iso(liw::mul(liw::mul(Tiw, w), inv_iw), res->tf12);
    res->rms = sqrt(ss / len);
}

__global__ __launch_bounds__(64) void k_xloop_choose(char* store, Lay L, XPrm xp, const unsigned char* __restrict__ key, const unsigned char* __restrict__ mask,
                                                     unsigned char* __restrict__ found, int* __restrict__ edge, double* __restrict__ tf12,
                                                     double* __restrict__ T_w1_w2, double* __restrict__ rms, long long* __restrict__ stats) {
    const int a = blockIdx.x, lane = threadIdx.x;
    if (!robot_on(mask, a) || !key[a]) return;
    const int n = ((const int*)(store + L.f_cnt))[a];
    if (n == 0) return;
    const int base = ((const int*)(store + L.f_base))[a];
    const XRes* res = (const XRes*)(store + L.f_res) + base;
    const int* sm = (const int*)(store + L.f_summary) + (size_t)base * 8;
    unsigned long long best = 0;
    int accepted = 0;
    long long qp = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int ci = c0 + lane;
        if (ci < n) {
            qp += sm[(size_t)ci * 8 + 4];
            const double r = res[ci].rms;
            if (!(r == -1.0)) {
                ++accepted;
                if (!(r > xp.max_rms)) {   // largest size, then the lowest position = the lowest candidate index
                    const unsigned long long v = (unsigned long long)(unsigned)sm[(size_t)ci * 8] << 32 | (unsigned long long)(0xFFFFFFFFu - (unsigned)ci);
                    best = v > best ? v : best;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        qp += __shfl_xor(qp, o, 64);
        accepted += __shfl_xor(accepted, o, 64);
        const unsigned long long x = __shfl_xor(best, o, 64);
        best = x > best ? x : best;
    }
    if (lane != 0) return;
    long long* st = stats + (size_t)a * 6;
    st[3] = qp; st[4] = accepted; st[5] = accepted;
    if (best == 0) return;
    const int win = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    const XPair* c = (const XPair*)(store + L.f_pairs) + base + win;
    const XRes* w = res + win;
    found[a] = 1;
    int* e = edge + 4 * (size_t)a;
    e[0] = c->query; e[1] = c->partner; e[2] = c->cand; e[3] = sm[(size_t)win * 8];
    for (int k = 0; k < 12; ++k) tf12[(size_t)a * 12 + k] = w->tf12[k];
    rms[a] = w->rms;
    const IsoD f1 = load_iso((const double*)(region(store, L, c->robot) + L.r_tf) + (size_t)c->query * 12);
    const IsoD f2 = load_iso((const double*)(region(store, L, c->partner) + L.r_tf) + (size_t)c->cand * 12);
    store_iso(liw::mul(liw::mul(f1, load_iso(w->tf12)), liw::inverse(f2)), T_w1_w2 + (size_t)a * 12);
}

// ------------------------------------------------------------------------------------------------------------ partner and link
__global__ __launch_bounds__(64) void k_xloop_partner(int B, const int* __restrict__ group_of, const unsigned char* __restrict__ linked, int round,
                                                      int* __restrict__ partner) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const int g = group_of[a];
    int pick = -1;
    if (g >= 0 && !linked[a]) {
        int n = 0;
        for (int m0 = 0; m0 < B; m0 += 64) {
            const int m = m0 + lane;
            n += __popcll(__ballot(m < B && linked[m] && group_of[m] == g));
        }
        if (n > 0) {
            int want = round % n;    // the want-th linked member in index order
            for (int m0 = 0; m0 < B && pick < 0; m0 += 64) {
                const int m = m0 + lane;
                unsigned long long bal = __ballot(m < B && linked[m] && group_of[m] == g);
                const int c = __popcll(bal);
                if (want >= c) { want -= c; continue; }
                for (int k = 0; k < want; ++k) bal &= bal - 1;   // drop the lowest `want` set bits
                pick = m0 + __ffsll(bal) - 1;
            }
        }
    }
    if (lane == 0) partner[a] = pick;
}

// staged decision of robot r in group_linked[r]: -2 linked before the call, -1 stays unlinked, else source * 2 + rule (0: (i), 1: (ii))
__global__ __launch_bounds__(64) void k_xloop_decide(int B, const int* __restrict__ group_of, const int* __restrict__ partner,
                                                     const unsigned char* __restrict__ found, const unsigned char* __restrict__ linked,
                                                     int* __restrict__ group_linked) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int g = group_of[r];
    int code = -1;
    if (linked[r]) code = -2;
    else if (g >= 0) {
        const int p = partner[r];
        if (found[r] && p >= 0 && p < B && p != r && linked[p] && group_of[p] == g) code = p * 2;
        else {
            for (int a0 = 0; a0 < B && code < 0; a0 += 64) {
                const int a = a0 + lane;
                const unsigned long long bal = __ballot(a < B && a != r && partner[a] == r && found[a] && linked[a] && group_of[a] == g);
                if (bal) code = (a0 + __ffsll(bal) - 1) * 2 + 1;
            }
        }
    }
    if (lane == 0) group_linked[r] = code;
}

__global__ __launch_bounds__(64) void k_xloop_apply(int B, const int* __restrict__ group_of, const int* __restrict__ edge, const double* __restrict__ T_w1_w2,
                                                    unsigned char* __restrict__ linked, double* T_g_w, int* __restrict__ via, int* __restrict__ group_linked) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const int code = group_linked[r];
    if (code < 0) {
        group_linked[r] = code == -2 ? group_of[r] : -1;
        return;
    }
    const int src = code >> 1, own = r, rule = code & 1;
    const int e = rule ? src : own;                           // the robot whose query made the edge
    const IsoD E = load_iso(T_w1_w2 + (size_t)e * 12), G = load_iso(T_g_w + (size_t)src * 12);   // src was linked before: not written here
    store_iso(liw::mul(G, rule ? E : liw::inverse(E)), T_g_w + (size_t)r * 12);
    const int* ed = edge + 4 * (size_t)e;
    int* v = via + 4 * (size_t)r;
    v[0] = src; v[1] = rule ? ed[2] : ed[0]; v[2] = rule ? ed[0] : ed[2]; v[3] = ed[3];
    linked[r] = 1;
    group_linked[r] = group_of[r];
}

static int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

int launch_cross_detect(char* store, const Lay& L, const Prm& p, const XPrm& x, const unsigned char* key, const int* partner,
                        const unsigned char* mask, unsigned char* found, int* edge, double* tf12, double* T_w1_w2, double* rms, long long* stats,
                        hipStream_t s) {
    const long long slots = (long long)L.B * L.NC;
    hipLaunchKernelGGL(k_xloop_gates, dim3(L.B), dim3(64), 0, s, store, L, p, key, partner, mask, found, edge, stats);
    if (liw_floop_dev::launch_scan(store, L, s)) return -1;
    hipLaunchKernelGGL(k_xloop_pairs, dim3(blocks(slots, 256)), dim3(256), 0, s, store, L, partner);
    const long long items = slots * kDraws * ((L.P + kRowsPerBlock - 1) / kRowsPerBlock);
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);   // as launch_detect: 16 work-groups per CU of a 256-CU device
    hipLaunchKernelGGL(k_xloop_match, dim3(grid), dim3(256), liw_floop_dev::match_lds(L, p.g), s, store, L, p.g);
    hipLaunchKernelGGL(k_xloop_select, dim3((unsigned)(slots < 16384 ? slots : 16384)), dim3(64), 0, s, store, L, p.g);
    hipLaunchKernelGGL(k_xloop_icp, dim3(blocks(slots, 64)), dim3(64), 0, s, store, L, p, x);
    hipLaunchKernelGGL(k_xloop_choose, dim3(L.B), dim3(64), 0, s, store, L, x, key, mask, found, edge, tf12, T_w1_w2, rms, stats);
    return ok();
}

int launch_partner(int B, const int* group_of, const unsigned char* linked, int round, int* partner, hipStream_t s) {
    hipLaunchKernelGGL(k_xloop_partner, dim3(B), dim3(64), 0, s, B, group_of, linked, round, partner);
    return ok();
}

int launch_link(int B, const int* group_of, const int* partner, const unsigned char* found, const int* edge, const double* T_w1_w2,
                unsigned char* linked, double* T_g_w, int* via, int* group_linked, hipStream_t s) {
    hipLaunchKernelGGL(k_xloop_decide, dim3(B), dim3(64), 0, s, B, group_of, partner, found, linked, group_linked);
    hipLaunchKernelGGL(k_xloop_apply, dim3(blocks(B, 64)), dim3(64), 0, s, B, group_of, edge, T_w1_w2, linked, T_g_w, via, group_linked);
    return ok();
}

}  // namespace liw_xloop_dev
