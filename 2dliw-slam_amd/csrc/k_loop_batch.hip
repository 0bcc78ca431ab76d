// k_loop_batch.hip — the fleet loop detector's device work (C ABI include/liw_loop_batch.h, host side liw_loop_batch.cpp).
//
// liw_floop_add_keyframes:
//   k_floop_gather    one wavefront per robot: the key frame's pose record and corner list go into the store, then the sub-map's
//                     corner lists are walked newest first and de-duplicated.  The reference's inner loop breaks at the first
//                     kept point within 5 d_res and blends only within d_res / 2; every point in front of the first hit is farther
//                     than 5 d_res, so per corner the lanes test the kept points (in LDS) 64 at a time, a ballot finds the
//                     first hit, and its lane blends if it is also within d_res / 2; no hit appends.  Serial over corners.
//   k_floop_describe  one wave per (robot, point): describe_point of k_loop_dev.hpp, the body k_loop_describe runs (dij, aij, bitonic
//                     sort of dij << 12 | j, quick_des), at the fleet's point stride of 3 doubles.
// liw_floop_detect:
//   k_floop_gates     one wave per robot, a lane per candidate i = 0, s, ...: the null / points / origin-distance gates, the five
//                     draws (splitmix64, a 64-bit modulo), the rank among the robot's launched candidates by ballot prefix.
//   k_floop_scan      one work-group: exclusive scan of the per-robot counts -> the pair list's bases, the pair total, max n2.
//   k_floop_pairs     a lane per (robot, candidate): the compact pair list in robot-then-candidate order.
//   k_floop_match     match_rows of k_loop_dev.hpp, the body k_loop_match runs (16 rows per work-group, the drawn query row staged
//                     once), on a fixed grid that strides over (pair, draw, 16-row) items.
//   k_floop_select    a wave strides over pairs: select_best of k_loop_dev.hpp, the body k_loop_select runs.
//   k_floop_icp       a lane per pair above the threshold: the planar closed-form ICP over the list in list order, the
//                     T_imu_to_wheel conjugation, the tf gate through log_SO3, all with liw_dual.hpp and liw_crmath.hpp.
//   k_floop_choose    one wave per robot: the lowest passing candidate, the stats.
// LDS atomics as in k_loop.hip (per-task histogram, quick_des bitmap); no global atomics; positions come from prefix counts.
#pragma clang fp contract(off)   // the de-duplicated points and dij must be bit-identical to the host arithmetic

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/liw_loop_batch.h"
#include "k_loop_batch.hpp"
#include "k_loop_dev.hpp"
#include "liw_crmath.hpp"
#include "liw_dual.hpp"

namespace liw_floop_dev {

using liw_loop_dev::describe_point;
using liw_loop_dev::kRowsPerBlock;
using liw_loop_dev::match_rows;
using liw_loop_dev::select_best;

// A double whose sin / cos / atan2 are the correctly rounded ones of liw_crmath.hpp (as the tracking glue's): make_tf of a key
// frame's pose is then the host's for all but the arguments where the host libm itself is not correctly rounded.
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

using IsoD = liw::Iso<double>;

__device__ __forceinline__ char* robot_region(char* store, const Lay& L, int b) { return store + (size_t)b * L.robot_bytes; }
__device__ __forceinline__ bool robot_on(const unsigned char* a, int b) { return !a || a[b] != 0; }

__device__ __forceinline__ IsoD load_iso(const double* T) { return liw::cast_iso<double>(T, T + 9); }
__device__ __forceinline__ IsoD identity_iso() {
    IsoD r;
    for (int k = 0; k < 9; ++k) r.R.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
    r.t = liw::V3<double>(0.0, 0.0, 0.0);
    return r;
}

__global__ __launch_bounds__(256) void k_floop_reset(char* store, Lay L, const unsigned char* __restrict__ mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || !robot_on(mask, b)) return;
    int* hdr = (int*)robot_region(store, L, b);
    hdr[0] = 0;
    hdr[1] = 0;
}

__global__ __launch_bounds__(64) void k_floop_gather(char* store, Lay L, double d_res, const unsigned char* __restrict__ key,
                                                     const double* __restrict__ pose, const double* __restrict__ corners, int stride,
                                                     const int* __restrict__ n_corners, const unsigned char* __restrict__ mask,
                                                     unsigned char* __restrict__ added) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* pts = (double*)smem;   // [P + 1][3] kept points
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!robot_on(mask, b)) return;
    if (!key[b]) {
        if (added && lane == 0) added[b] = 0;
        return;
    }
    int* work = (int*)(store + L.f_work);
    char* R = robot_region(store, L, b);
    int* hdr = (int*)R;
    const int K = hdr[0];
    if (K >= L.K) {
        if (lane == 0) {
            hdr[1] = 1;
            work[b] = 0;
            if (added) added[b] = 0;
        }
        return;
    }
    if (lane == 0) {
        const double* ps = pose + (size_t)b * 6;
        const liw::Iso<CR> T = liw::make_tf(liw::V3<CR>(ps[0], ps[1], ps[2]), liw::V3<CR>(ps[3], ps[4], ps[5]));
        double* tf = (double*)(R + L.r_tf) + (size_t)K * 12;
        for (int k = 0; k < 9; ++k) tf[k] = T.R.m[k].v;
        tf[9] = T.t.x.v; tf[10] = T.t.y.v; tf[11] = T.t.z.v;
    }
    int n = n_corners[b];
    n = n < 0 ? 0 : n;
    const int ccap = L.C < stride ? L.C : stride;
    const bool over = n > ccap;
    int* ringn = (int*)(R + L.r_ringn);
    double* ring = (double*)(R + L.r_ring);
    const int rs = K % L.S;
    if (!over) {
        const double* src = corners + (size_t)b * stride * 3;
        double* dst = ring + (size_t)rs * L.C * 3;
        for (int e = lane; e < 3 * n; e += 64) dst[e] = src[e];
    }
    if (lane == 0) ringn[rs] = over ? -1 : n;
    __syncthreads();
    // spawn_laser_map_feature (:898-929) + the de-duplication (:955-980): newest key frame first, at most S of them
    const double near = d_res / 2, far = d_res * 5;
    int np = 0;
    bool bad = false, overcap = false;
    for (int t = 0; t < L.S && t <= K && !bad && !overcap; ++t) {
        const int slot = (K - t) % L.S;
        const int nc = ringn[slot];
        if (nc < 0) { bad = true; break; }
        const double* cs = ring + (size_t)slot * L.C * 3;
        for (int j = 0; j < nc && !overcap; ++j) {
            const double c0 = cs[3 * j], c1 = cs[3 * j + 1], c2 = cs[3 * j + 2];
            bool dup = false;
            for (int k0 = 0; k0 < np && !dup; k0 += 64) {
                const int k = k0 + lane;
                bool hit = false;
                double nrm = 0.0;
                if (k < np) {
                    const double dx = c0 - pts[3 * k], dy = c1 - pts[3 * k + 1];
                    nrm = sqrt(dx * dx + dy * dy);
                    hit = nrm < far;
                }
                const unsigned long long bal = __ballot(hit);
                if (bal) {
                    if (lane == __ffsll(bal) - 1 && nrm < near) {
                        pts[3 * k] = (pts[3 * k] * 3 + c0) / 4;
                        pts[3 * k + 1] = (pts[3 * k + 1] * 3 + c1) / 4;
                        pts[3 * k + 2] = (pts[3 * k + 2] * 3 + c2) / 4;
                    }
                    dup = true;
                }
            }
            if (!dup) {
                if (lane == 0) { pts[3 * np] = c0; pts[3 * np + 1] = c1; pts[3 * np + 2] = c2; }
                ++np;
                overcap = np > L.P;   // the LDS array holds max_points + 1 points: one more is enough to know
            }
            __syncthreads();
        }
    }
    const bool valid = !bad && !overcap;
    if (valid) {
        double* out = (double*)(R + L.r_pts) + (size_t)feature_slot(L, K) * L.P * 3;
        for (int e = lane; e < 3 * np; e += 64) out[e] = pts[e];
    }
    if (lane == 0) {
        ((int*)(R + L.r_state))[K] = bad ? LIW_FLOOP_OVER_CORNERS : (overcap ? LIW_LOOP_OVER_CAP : LIW_LOOP_VALID);
        ((int*)(R + L.r_npts))[K] = bad ? 0 : np;
        work[b] = valid ? np : 0;
        hdr[0] = K + 1;
        if (added) added[b] = 1;
    }
}

// blockIdx.x = robot * gx + first point; the block's wave takes the points first, first + gx, ...
__global__ __launch_bounds__(64) void k_floop_describe(char* store, Lay L, Geom g, double d_res, int gx, const unsigned char* __restrict__ key,
                                                       const unsigned char* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x / gx, i0 = blockIdx.x - b * gx, lane = threadIdx.x;
    if (!robot_on(mask, b) || !key[b]) return;
    const int n = ((const int*)(store + L.f_work))[b];
    if (i0 >= n) return;
    char* R = robot_region(store, L, b);
    const int kf = ((const int*)R)[0] - 1;
    const int fs = feature_slot(L, kf);
    const double* pts = (const double*)(R + L.r_pts) + (size_t)fs * L.P * 3;
    bool bad = false;
    for (int i = i0; i < n; i += gx) {
        const size_t row = (size_t)fs * L.P + i;
        bad |= describe_point<3>(pts, n, i, g, d_res, smem, (uint32_t*)(R + L.r_keys) + row * L.P, (double*)(R + L.r_aij) + row * L.P,
                                 (uint64_t*)(R + L.r_quick) + row * L.W);
        __syncthreads();
    }
    if (bad) ((int*)(R + L.r_state))[kf] = LIW_LOOP_DIJ_OVERFLOW;   // every writer stores the same value
}

__global__ __launch_bounds__(64) void k_floop_gates(char* store, Lay L, Prm p, const unsigned char* __restrict__ key,
                                                    const unsigned char* __restrict__ mask, unsigned char* __restrict__ found, int* __restrict__ edge,
                                                    long long* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int* cnt = (int*)(store + L.f_cnt);
    int* cmax = (int*)(store + L.f_cmax);
    if (!robot_on(mask, b) || !key[b]) {
        if (lane == 0) {
            cnt[b] = 0;
            cmax[b] = 0;
            if (robot_on(mask, b)) found[b] = 0;
        }
        return;
    }
    char* R = robot_region(store, L, b);
    const int K = ((const int*)R)[0];
    const int* state = (const int*)(R + L.r_state);
    const int* npts = (const int*)(R + L.r_npts);
    const double* tf = (const double*)(R + L.r_tf);
    const int q = K - 1;
    int nvis = 0, total = 0, n2max = 0;
    long long tasks = 0;
    if (K >= p.min_interval && K > 0 && state[q] == LIW_LOOP_VALID) {
        const int lim = K - p.min_interval;
        nvis = lim > 0 ? (lim + L.step - 1) / L.step : 0;
        const int n1 = npts[q], thr = p.g.thr;
        const IsoD inv1 = liw::inverse(L.S > 1 ? load_iso(tf + (size_t)q * 12) : identity_iso());
        Pre* pre = (Pre*)(store + L.f_pre) + (size_t)b * L.NC;
        for (int c0 = 0; c0 < L.NC; c0 += 64) {
            const int ci = c0 + lane, i = ci * L.step;
            bool ok = false;
            int n2 = 0;
            if (ci < nvis && state[i] == LIW_LOOP_VALID) {
                n2 = npts[i];
                if (!(n1 < thr || n2 < thr || n1 == 0 || n2 == 0)) {
                    const IsoD o2 = L.S > 1 ? load_iso(tf + (size_t)i * 12) : identity_iso();
                    const liw::V3<double> t = liw::mul(inv1.R, o2.t) + inv1.t;
                    ok = !(sqrt(t.x * t.x + t.y * t.y + t.z * t.z) > p.max_dis);
                }
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
    for (int o = 32; o > 0; o >>= 1) {
        tasks += __shfl_xor(tasks, o, 64);
        const int x = __shfl_xor(n2max, o, 64);
        n2max = x > n2max ? x : n2max;
    }
    if (lane == 0) {
        cnt[b] = total;
        cmax[b] = n2max;
        found[b] = 0;
        edge[3 * (size_t)b] = -1; edge[3 * (size_t)b + 1] = -1; edge[3 * (size_t)b + 2] = 0;
        long long* st = stats + (size_t)b * 6;
        st[0] = nvis; st[1] = total; st[2] = tasks; st[3] = 0; st[4] = 0; st[5] = 0;
    }
}

// exclusive scan of cnt[0 .. B) -> base; hdr = {pairs, max n2}.  One work-group of 1 024: a contiguous segment per thread.
__global__ __launch_bounds__(1024) void k_floop_scan(char* store, Lay L) {
    __shared__ int part[1024];
    __shared__ int pmax[1024];
    const int* cnt = (const int*)(store + L.f_cnt);
    const int* cmax = (const int*)(store + L.f_cmax);
    int* base = (int*)(store + L.f_base);
    const int tid = threadIdx.x, seg = (L.B + 1023) / 1024;
    const int lo = tid * seg, hi = lo + seg < L.B ? lo + seg : L.B;
    int s = 0, mx = 0;
    for (int b = lo; b < hi; ++b) { s += cnt[b]; mx = cmax[b] > mx ? cmax[b] : mx; }
    part[tid] = s;
    pmax[tid] = mx;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        const int w = tid >= o ? pmax[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        pmax[tid] = w > pmax[tid] ? w : pmax[tid];
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int b = lo; b < hi; ++b) { base[b] = run; run += cnt[b]; }
    if (tid == 1023) {
        int* hdr = (int*)(store + L.f_hdr);
        hdr[0] = part[1023];
        hdr[1] = pmax[1023];
    }
}

__global__ __launch_bounds__(256) void k_floop_pairs(char* store, Lay L) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)L.B * L.NC) return;
    const int b = (int)(idx / L.NC), ci = (int)(idx - (long long)b * L.NC);
    if (((const int*)(store + L.f_cnt))[b] == 0) return;   // the robot's Pre records are this call's only when it launched something
    const Pre* x = (const Pre*)(store + L.f_pre) + idx;
    if (x->rank < 0) return;
    const char* R = store + (size_t)b * L.robot_bytes;
    const int K = ((const int*)R)[0];
    Pair* o = (Pair*)(store + L.f_pairs) + ((const int*)(store + L.f_base))[b] + x->rank;
    o->robot = b;
    o->cand = ci * L.step;
    o->query = K - 1;
    o->n1 = ((const int*)(R + L.r_npts))[K - 1];
    o->n2 = x->n2;
    for (int d = 0; d < kDraws; ++d) o->rows[d] = x->rows[d];
}

__global__ __launch_bounds__(256) void k_floop_match(char* store, Lay L, Geom g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int* hdr = (const int*)(store + L.f_hdr);
    const int npairs = hdr[0], rb = (hdr[1] + kRowsPerBlock - 1) / kRowsPerBlock;
    const long long items = (long long)npairs * kDraws * rb;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int pi = (int)(item / (kDraws * rb)), rem = (int)(item - (long long)pi * kDraws * rb);
        const int d = rem / rb, r0 = (rem - d * rb) * kRowsPerBlock;
        const Pair* c = (const Pair*)(store + L.f_pairs) + pi;
        const int n1 = c->n1, n2 = c->n2, row1 = c->rows[d];
        if (r0 >= n2) continue;
        int2* out = (int2*)(store + L.f_tres) + ((size_t)pi * kDraws + d) * L.P;
        if (row1 < 0) {   // a repeated draw: no task
            for (int r = r0 + threadIdx.x; r < n2 && r < r0 + kRowsPerBlock; r += blockDim.x) out[r] = make_int2(0, 0);
            continue;
        }
        const char* R = store + (size_t)c->robot * L.robot_bytes;
        const uint32_t* keys = (const uint32_t*)(R + L.r_keys);
        const double* aij = (const double*)(R + L.r_aij);
        const uint64_t* quick = (const uint64_t*)(R + L.r_quick);
        const size_t qrow = (size_t)feature_slot(L, c->query) * L.P + row1;
        const size_t cslot = (size_t)feature_slot(L, c->cand) * L.P;
        match_rows(n1, n2, r0, keys + qrow * L.P, aij + qrow * L.P, quick + qrow * L.W, keys + cslot * L.P, aij + cslot * L.P, quick + cslot * L.W, g,
                   smem, out);
    }
}

__global__ __launch_bounds__(64) void k_floop_select(char* store, Lay L, Geom g) {
    const int npairs = ((const int*)(store + L.f_hdr))[0];
    for (int pi = blockIdx.x; pi < npairs; pi += gridDim.x) {
        const Pair* c = (const Pair*)(store + L.f_pairs) + pi;   // read through the pointer, as Cand in k_loop.hip
        const char* R = store + (size_t)c->robot * L.robot_bytes;
        const size_t qs = (size_t)feature_slot(L, c->query) * L.P * L.P, cs = (size_t)feature_slot(L, c->cand) * L.P * L.P;
        const uint32_t* keys = (const uint32_t*)(R + L.r_keys);
        const double* aij = (const double*)(R + L.r_aij);
        select_best(c->rows, c->n1, c->n2, (const int2*)(store + L.f_tres) + (size_t)pi * kDraws * L.P, keys + qs, aij + qs, keys + cs, aij + cs, g,
                    (int*)(store + L.f_summary) + (size_t)pi * 8, (int*)(store + L.f_lists) + (size_t)pi * L.P * 2);
    }
}

__device__ __forceinline__ void apply_xy(const IsoD& A, const double* x, double& ox, double& oy) {   // liw_lie_apply, z dropped
    const liw::V3<double> r = liw::mul(A.R, liw::V3<double>(x[0], x[1], x[2]));
    ox = r.x + A.t.x;
    oy = r.y + A.t.y;
}

// liw_loop_detect's walk over one accepted candidate: liw_loop_icp over the list in list order, the conjugation, the tf gate
__global__ __launch_bounds__(64) void k_floop_icp(char* store, Lay L, Prm p) {
    const int npairs = ((const int*)(store + L.f_hdr))[0];
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= npairs) return;
    Res* res = (Res*)(store + L.f_res) + pi;
    const int* sm = (const int*)(store + L.f_summary) + (size_t)pi * 8;
    const int size = sm[0], len = sm[5];
    if (size <= p.g.thr || len != size || len > L.P) {
        res->checked = 0;
        res->pass = 0;
        return;
    }
    const Pair* c = (const Pair*)(store + L.f_pairs) + pi;
    const char* R = store + (size_t)c->robot * L.robot_bytes;
    const double* tf = (const double*)(R + L.r_tf);
    const IsoD f1 = load_iso(tf + (size_t)c->query * 12), f2 = load_iso(tf + (size_t)c->cand * 12), Tiw = load_iso(p.Tiw);
    const IsoD inv1 = liw::inverse(liw::mul(f1, Tiw)), inv2 = liw::inverse(liw::mul(f2, Tiw)), inv_iw = liw::inverse(Tiw);
    const double* P1 = (const double*)(R + L.r_pts) + (size_t)feature_slot(L, c->query) * L.P * 3;
    const double* P2 = (const double*)(R + L.r_pts) + (size_t)feature_slot(L, c->cand) * L.P * 3;
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
    IsoD w;
    w.R.m[0] = cs; w.R.m[1] = -sn; w.R.m[2] = 0; w.R.m[3] = sn; w.R.m[4] = cs; w.R.m[5] = 0; w.R.m[6] = 0; w.R.m[7] = 0; w.R.m[8] = 1;
    w.t = liw::V3<double>(c1x - (cs * c2x - sn * c2y), c1y - (sn * c2x + cs * c2y), 0.0);
    const IsoD it12 = liw::mul(liw::mul(Tiw, w), inv_iw);
    const IsoD err = liw::mul(liw::inverse(it12), liw::mul(liw::inverse(f1), f2));
    liw::M3<CR> Rc;
    for (int k = 0; k < 9; ++k) Rc.m[k] = CR(err.R.m[k]);
    const liw::V3<CR> dq = liw::log_SO3(Rc);
    const double np_ = sqrt(err.t.x * err.t.x + err.t.y * err.t.y + err.t.z * err.t.z);
    const double nq = sqrt(dq.x.v * dq.x.v + dq.y.v * dq.y.v + dq.z.v * dq.z.v);
    for (int k = 0; k < 9; ++k) res->tf12[k] = it12.R.m[k];
    res->tf12[9] = it12.t.x; res->tf12[10] = it12.t.y; res->tf12[11] = it12.t.z;
    res->checked = 1;
    res->pass = !(np_ > p.max_tf_p || nq > p.max_tf_q);
}

__global__ __launch_bounds__(64) void k_floop_choose(char* store, Lay L, const unsigned char* __restrict__ key, const unsigned char* __restrict__ mask,
                                                     unsigned char* __restrict__ found, int* __restrict__ edge, double* __restrict__ tf12,
                                                     long long* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!robot_on(mask, b) || !key[b]) return;
    const int n = ((const int*)(store + L.f_cnt))[b];
    if (n == 0) return;
    const int base = ((const int*)(store + L.f_base))[b];
    const Res* res = (const Res*)(store + L.f_res) + base;
    const int* sm = (const int*)(store + L.f_summary) + (size_t)base * 8;
    int first = -1, accepted = 0, before = 0;
    long long qp = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int ci = c0 + lane;
        const bool in = ci < n;
        const bool chk = in && res[ci].checked, pass = in && res[ci].pass;
        qp += in ? sm[(size_t)ci * 8 + 4] : 0;
        const unsigned long long bc = __ballot(chk), bp = __ballot(pass);
        accepted += __popcll(bc);
        if (first < 0) {
            if (bp) {
                const int l = __ffsll(bp) - 1;
                first = c0 + l;
                before += __popcll(bc & ((2ull << l) - 1ull));   // those walked up to and including the one that passed
            } else before += __popcll(bc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) qp += __shfl_xor(qp, o, 64);
    if (lane == 0) {
        long long* st = stats + (size_t)b * 6;
        st[3] = qp; st[4] = accepted; st[5] = before;
        if (first >= 0) {
            const Pair* c = (const Pair*)(store + L.f_pairs) + base + first;
            found[b] = 1;
            edge[3 * (size_t)b] = c->query; edge[3 * (size_t)b + 1] = c->cand; edge[3 * (size_t)b + 2] = sm[(size_t)first * 8];
        }
    }
    if (first >= 0 && lane < 12) tf12[(size_t)b * 12 + lane] = res[first].tf12[lane];
}

size_t gather_lds(const Lay& L) { return (size_t)(L.P + 1) * 24; }

size_t describe_lds(const Lay& L) {
    int N2 = 1;
    while (N2 < L.P - 1) N2 <<= 1;
    return (size_t)L.P * 8 + (size_t)L.W * 8 + (size_t)N2 * 4;
}

size_t match_lds(const Lay& L, const Geom& g) {
    const int MW = (g.nb + 31) >> 5;
    return (size_t)(L.P - 1) * 12 + 4 * ((size_t)g.nb * 8 + (size_t)MW * 64 * 4);
}

static int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_floop_reset, dim3(blocks(L.B, 256)), dim3(256), 0, s, store, L, mask);
    return ok();
}

int launch_add(char* store, const Lay& L, const Prm& p, const unsigned char* key, const double* pose, const double* corners, int stride,
               const int* n_corners, const unsigned char* mask, unsigned char* added, hipStream_t s) {
    hipLaunchKernelGGL(k_floop_gather, dim3(L.B), dim3(64), gather_lds(L), s, store, L, p.d_res, key, pose, corners, stride, n_corners, mask, added);
    const int gx = L.P < 128 ? L.P : 128;
    hipLaunchKernelGGL(k_floop_describe, dim3(blocks((long long)L.B * gx, 1)), dim3(64), describe_lds(L), s, store, L, p.g, p.d_res, gx, key, mask);
    return ok();
}

int launch_scan(char* store, const Lay& L, hipStream_t s) {
    hipLaunchKernelGGL(k_floop_scan, dim3(1), dim3(1024), 0, s, store, L);
    return ok();
}

int launch_detect(char* store, const Lay& L, const Prm& p, const unsigned char* key, const unsigned char* mask, unsigned char* found, int* edge,
                  double* tf12, long long* stats, hipStream_t s) {
    const long long slots = (long long)L.B * L.NC;
    hipLaunchKernelGGL(k_floop_gates, dim3(L.B), dim3(64), 0, s, store, L, p, key, mask, found, edge, stats);
    hipLaunchKernelGGL(k_floop_scan, dim3(1), dim3(1024), 0, s, store, L);
    hipLaunchKernelGGL(k_floop_pairs, dim3(blocks(slots, 256)), dim3(256), 0, s, store, L);
    const long long items = slots * kDraws * ((L.P + kRowsPerBlock - 1) / kRowsPerBlock);
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);   // 16 work-groups per CU of a 256-CU device; the rest by stride
    hipLaunchKernelGGL(k_floop_match, dim3(grid), dim3(256), match_lds(L, p.g), s, store, L, p.g);
    hipLaunchKernelGGL(k_floop_select, dim3((unsigned)(slots < 16384 ? slots : 16384)), dim3(64), 0, s, store, L, p.g);
    hipLaunchKernelGGL(k_floop_icp, dim3(blocks(slots, 64)), dim3(64), 0, s, store, L, p);
    hipLaunchKernelGGL(k_floop_choose, dim3(L.B), dim3(64), 0, s, store, L, key, mask, found, edge, tf12, stats);
    return ok();
}

}  // namespace liw_floop_dev
