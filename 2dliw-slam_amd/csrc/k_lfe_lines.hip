// k_lfe_lines.hip — fleet laser front-end, the lines of scans and of sub-maps (C ABI include/liw_laser_batch.h, host side
// liw_laser_batch.cpp).  First from a scan to its lines: ranges -> points, the de-skew, spawn_scan lane-per-scan and wave-per-scan,
// the corners into the world frame.  Then the managers' sub-maps: the resets, laser_manager::add_scan lane-per-robot and
// wave-per-robot (the latter also the whole liw_lfe_rebuild), the copy of a scan slot.
// Every step of the host front-end (liw_laser.cpp) is a serial chain over one scan (the 1 cm filter compares against the previously
// KEPT point, the segment merge carries `last`, a line's cells are de-duplicated against its earlier cells), so a lane walks its
// scan in the host's order and rounds as the host does; the batch is the parallelism.
// The two stages stay in one translation unit because the spawn and the add_scan kernels share add_line and its fit: compiled apart,
// the inliner orders those bodies differently and k_lfe_spawn, k_lfe_add_scan and k_lfe_add_scan_wave (236 VGPRs, at the ceiling of
// two waves per SIMD) come out as other code.
#pragma clang fp contract(off)   // the x86-64 host build of liw_laser.cpp does not contract; hipcc contracts device code by default

#include <hip/hip_runtime.h>

#include "k_lfe.hpp"
#include "k_lfe_dev.hpp"

namespace lfe {

constexpr int kStep = 3;

// smallest eigenvector of a symmetric 3x3 (cyclic Jacobi), liw_laser.cpp smallest_eigvec3
__device__ inline Vec smallest_eigvec3(double M[3][3]) {
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = fabs(M[0][1]) + fabs(M[0][2]) + fabs(M[1][2]);
        const double diag = fabs(M[0][0]) + fabs(M[1][1]) + fabs(M[2][2]);
        if (off <= 1e-300 || off <= 1e-17 * diag) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (M[p][q] == 0.0) continue;
                const double theta = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double mkp = M[k][p], mkq = M[k][q];
                    M[k][p] = c * mkp - s * mkq; M[k][q] = s * mkp + c * mkq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double mpk = M[p][k], mqk = M[q][k];
                    M[p][k] = c * mpk - s * mqk; M[q][k] = s * mpk + c * mqk;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    if (M[1][1] < M[m][m]) m = 1;
    if (M[2][2] < M[m][m]) m = 2;
    return m == 0 ? Vec(V[0][0], V[1][0], V[2][0]) : (m == 1 ? Vec(V[0][1], V[1][1], V[2][1]) : Vec(V[0][2], V[1][2], V[2][2]));
}

// heap sort of a slot's entries (in place, no scratch)
__device__ inline void sort_entries(u64* a, int n) {
    auto sift = [&](int i, int m) {
        for (;;) {
            int c = 2 * i + 1;
            if (c >= m) return;
            if (c + 1 < m && a[c + 1] > a[c]) ++c;
            if (!(a[c] > a[i])) return;
            const u64 t = a[c]; a[c] = a[i]; a[i] = t;
            i = c;
        }
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int m = n - 1; m > 0; --m) {
        const u64 t = a[0]; a[0] = a[m]; a[m] = t;
        sift(0, m);
    }
}

// one line's registration into the slot's line_map: "ids.back() == id" de-duplication = (cell, id) already pushed by this line
struct Reg {
    Slot& s; const Lay& L; const DP& P; unsigned& st; int id, tail; bool registered; u64 last;
    __device__ void push(double x, double y) {
        int c, r;
        xy_to_index(P, x, y, c, r);
        if (!valid(P, r, c)) return;
        const u64 e = ((u64)(unsigned)(r * P.w + c) << 32) | (unsigned)id;
        if (e == last) return;                 // the common case: the previous point's cell
        const int n = n_entries(s, L);
        for (int j = n - 1; j >= tail; --j)
            if (s.ent[j] == e) return;
        registered = true;
        if (n >= L.max_entries) { st |= LIW_LFE_ST_CELLS; return; }
        s.ent[n] = e;
        s.h->n_entries = n + 1;
        last = e;
    }
};

// scan::add_line(points, index1, index2, add_concers) (laser_manager.cpp:137-212) without corners; from_points selects the
// point-cell registration (spawn) over the 0.05 m rasterisation (sub-map segments)
// the fit of add_line (moment sums in index order, eigenvector, max_dis, the projected end points) and its two rejections:
// one body for the lane kernels and k_lfe_add_scan_wave, so that they round alike
__device__ __forceinline__ bool line_fit(const DP& P, const double* pts, int i1, int i2, Vec& p1, Vec& p2, Vec& abc, double& len) {
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = i1; i <= i2; ++i) {
        const double x = pts[i * 3], y = pts[i * 3 + 1];
        M[0][0] += x * x; M[0][1] += x * y; M[0][2] += x; M[1][1] += y * y; M[1][2] += y; M[2][2] += 1.0;
    }
    M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
    abc = smallest_eigvec3(M);
    Vec a(0, 0, 0), b(0, 0, 0);
    if (fabs(abc.y) < 0.5) {
        a.y = 0; a.x = -abc.z / abc.x; b.y = 1; b.x = (-abc.z - abc.y) / abc.x;
    } else {
        a.x = 0; b.x = 1; a.y = -abc.z / abc.y; b.y = (-abc.z - abc.x) / abc.y;
    }
    double max_dis = 0;
    for (int i = i1; i <= i2; ++i) { const double d = dis_from_line(ld3(pts + 3 * i), a, b); max_dis = (max_dis < d) ? d : max_dis; }
    p1 = project_to_line(ld3(pts + 3 * i1), a, b);
    p2 = project_to_line(ld3(pts + 3 * i2), a, b);
    len = vnorm(vsub(p1, p2));
    if (max_dis > P.max_dis) return false;
    if (len < P.min_len) return false;
    return true;
}
__device__ inline bool add_line(Slot& s, const Lay& L, const DP& P, const double* pts, int i1, int i2, bool from_points, unsigned& st) {
    if (i2 - i1 < 2) return false;
    Vec p1, p2, abc;
    double len;
    if (!line_fit(P, pts, i1, i2, p1, p2, abc, len)) return false;
    const int id = n_lines(s, L);
    if (id >= L.max_lines) { st |= LIW_LFE_ST_LINES; return false; }
    Reg g{s, L, P, st, id, n_entries(s, L), false, ~0ull};
    if (from_points) {
        for (int i = i1; i <= i2; ++i) g.push(pts[3 * i], pts[3 * i + 1]);
    } else {
        const Vec unit = vunit_div(vsub(p2, p1));
        for (double tr = 0; tr <= len; tr += 0.05) {
            const Vec t = vadd(p1, vscale(unit, tr));
            g.push(t.x, t.y);
        }
    }
    if (g.registered) {
        double* o = s.lines + 10 * (size_t)id;
        o[0] = p1.x; o[1] = p1.y; o[2] = p1.z; o[3] = p2.x; o[4] = p2.y; o[5] = p2.z; o[6] = abc.x; o[7] = abc.y; o[8] = abc.z; o[9] = len;
        s.h->n_lines = id + 1;
    }
    return true;
}
// scan::add_line(p1, p2, add_concers = false) (:213-222)
__device__ inline bool add_segment(Slot& s, const Lay& L, const DP& P, const Vec& p1, const Vec& p2, unsigned& st) {
    const Vec mid = Vec((p2.x + p1.x) / 2, (p2.y + p1.y) / 2, (p2.z + p1.z) / 2);
    const double fake[9] = {p1.x, p1.y, p1.z, mid.x, mid.y, mid.z, p2.x, p2.y, p2.z};
    return add_line(s, L, P, fake, 0, 2, false, st);
}

// ascending sort of n unique keys by one wave: bitonic network whose exchanges all put the smaller key at the lower index, so
// the keys behind n behave as +inf without being stored
__device__ inline void wave_sort(u64* a, int n, int lane) {
    auto pass = [&](int mask) {
        for (int i = lane; i < n; i += kBlock) {
            const int l = i ^ mask;
            if (l > i && l < n) { const u64 p = a[i], q = a[l]; if (q < p) { a[i] = q; a[l] = p; } }
        }
        __syncthreads();
    };
    for (int k = 2; (k >> 1) < n; k <<= 1) {
        pass(k - 1);
        for (int j = k >> 2; j > 0; j >>= 1) pass(j);
    }
}

// the rasterisation walk of add_line for a segment: f(k, cell) for the k-th distinct valid cell; returns their number
template <class F> __device__ __forceinline__ int seg_cells(const DP& P, const Vec& p1, const Vec& p2, double len, F f) {
    const Vec unit = vunit_div(vsub(p2, p1));
    unsigned last = ~0u;
    int n = 0;
    for (double tr = 0; tr <= len; tr += 0.05) {
        const Vec t = vadd(p1, vscale(unit, tr));
        int c, r;
        xy_to_index(P, t.x, t.y, c, r);
        if (!valid(P, r, c)) continue;
        const unsigned cell = (unsigned)(r * P.w + c);
        if (cell == last) continue;
        last = cell;
        f(n, cell);
        ++n;
    }
    return n;
}

// one continuous run [s, e] of laser_manager::spawn_scan (:376-420): maxima found as the host loop finds them (i += step after
// a maximum), the merge over `ends` streamed (ends[last], ends[i], ends[i + 1])
__device__ void spawn_run(Slot& sl, const Lay& L, const DP& P, const double* X, int s, int e, unsigned& st) {
    auto Pt = [&](int i) { return ld3(X + 3 * i); };
    auto resp = [&](int i) { return clac_cos(Pt(i), Pt(i - kStep > s ? i - kStep : s), Pt(i + kStep < e ? i + kStep : e)); };
    int gi = s + 1;
    bool done = false;
    auto next_end = [&]() -> int {
        while (gi <= e - 1) {
            const int i = gi;
            const double ri = resp(i);
            bool is_max = true;
            const int bj = i - kStep > s + 1 ? i - kStep : s + 1, ej = i + kStep < e - 1 ? i + kStep : e - 1;
            for (int j = bj; j <= ej; ++j)
                if (j != i && resp(j) >= ri) { is_max = false; break; }
            if (is_max) { gi = i + kStep + 1; return i; }
            gi = i + 1;
        }
        done = true;
        return e;
    };
    int last = s;
    int cur = next_end();
    bool cur_end = done;
    while (!cur_end) {
        const int nxt = next_end();
        const bool nxt_end = done;
        const double angle = acos(clac_cos(Pt(cur), Pt(last), Pt(nxt)));
        if (fabs(angle) < P.tol) {
            add_line(sl, L, P, X, last, cur, true, st);
            last = cur;
        }
        cur = nxt;
        cur_end = nxt_end;
    }
    add_line(sl, L, P, X, last, e, true, st);
}

// ranges -> points (+ times), a lane per scan: the (cosf, sinf) table of the geometry comes from the host libm (ctx)
__global__ void __launch_bounds__(kBlock) k_lfe_ranges(void* store, Lay L, const float* ranges, int n_rays, const float2* cs, float tinc,
                                                      const double* stamps, double* pts, double* times, int* n_pts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    const float* R = ranges + (size_t)b * n_rays;
    double* X = pts + (size_t)b * L.max_points * 3;
    double* T = times + (size_t)b * L.max_points;
    const double stamp = stamps[b];
    int m = 0;
    double lx = 0, ly = 0, lz = 0;
    unsigned st = 0;
    for (int i = 0; i < n_rays; ++i) {
        const float rg = R[i];
        if (isnan(rg) || isinf(rg) || !(rg > 0.1)) continue;
        const float2 c = cs[i];
        const double x = (double)(c.x * rg), y = (double)(c.y * rg);
        if (m > 0) {
            const double dx = x - lx, dy = y - ly, dz = 0.0 - lz;
            if (sqrt(dx * dx + dy * dy + dz * dz) < 0.01) continue;
        }
        if (m >= L.max_points) { st |= LIW_LFE_ST_POINTS; break; }
        X[3 * m] = x; X[3 * m + 1] = y; X[3 * m + 2] = 0.0;
        T[m] = stamp + (double)((float)(size_t)i * tinc);
        lx = x; ly = y; lz = 0.0;
        ++m;
    }
    n_pts[b] = st ? L.max_points + 1 : m;   // an overflow marks the scan itself: spawn rejects n_pts > max_points
    if (st && store) ((Mgr*)robot_ptr(store, L, b))->status |= st;
}

// one lane per point: make_tf(dt * twist) * p
__global__ void __launch_bounds__(256) k_lfe_deskew(Lay L, double* pts, const double* times, const int* n_pts, const double* stamps,
                                                   const double* lin, const double* ang) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)L.B * L.max_points) return;
    const int b = (int)(g / L.max_points), i = (int)(g % L.max_points);
    if (i >= n_pts[b]) return;
    const double dt = times[g] - stamps[b];
    const double* l = lin + 3 * (size_t)b;
    const double* a = ang + 3 * (size_t)b;
    const Iso<double> T = liw::make_tf(Vec(dt * l[0], dt * l[1], dt * l[2]), Vec(dt * a[0], dt * a[1], dt * a[2]));
    const Vec r = apply(T, ld3(pts + 3 * g));
    pts[3 * g] = r.x; pts[3 * g + 1] = r.y; pts[3 * g + 2] = r.z;
}

// the lane-per-scan spawn (continuous runs -> corner response -> strict local maxima -> merge -> add_line -> cell entries,
// heap-sorted): the checker behind LIW_LFE_SPAWN=lane, and the path of dimensions whose LDS need exceeds a work-group's 64 KiB.
// No corners.
__global__ void __launch_bounds__(kBlock) k_lfe_spawn(void* store, Lay L, DP P, int slot, const double* pts, const int* n_pts, const double* times) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    Slot sl = slot_at(store, L, b, slot);
    slot_clear(sl, times ? times[b] : 0.0);
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    unsigned st = 0;
    const int N = n_pts[b];
    if (N < 0 || N > L.max_points) {
        st = LIW_LFE_ST_POINTS;
    } else {
        const double* X = pts + (size_t)b * L.max_points * 3;
        int start = 0;   // continuous runs (:361-374)
        for (int i = 1; i < N; ++i)
            if (!(vnorm(vsub(ld3(X + 3 * (i - 1)), ld3(X + 3 * i))) <= P.cont_thr)) { spawn_run(sl, L, P, X, start, i - 1, st); start = i; }
        spawn_run(sl, L, P, X, start, N - 1, st);
        sort_entries(sl.ent, n_entries(sl, L));
    }
    sl.h->status = (int)st;
    if (st) m->status |= st;
}

// largest run start <= i (0 when there is none), and the last point of the run that holds i
__device__ inline int run_start(const u64* brk, int i) {
    int w = i >> 6;
    u64 m = brk[w] & (~0ull >> (63 - (i & 63)));
    while (!m) { if (--w < 0) return 0; m = brk[w]; }
    return (w << 6) + 63 - __clzll((long long)m);
}
// first set bit at an index >= j in words [0, W), or -1
__device__ inline int next_bit(const u64* a, int W, int j) {
    int w = j >> 6;
    if (w >= W) return -1;
    u64 m = a[w] & (~0ull << (j & 63));
    while (!m) { if (++w >= W) return -1; m = a[w]; }
    return (w << 6) + __ffsll((unsigned long long)m) - 1;
}
__device__ inline int run_end(const u64* brk, int W, int N, int i) { const int j = next_bit(brk, W, i + 1); return j < 0 ? N - 1 : j - 1; }
// calc_angle_and_intersection + the neighbourhood test of scan::add_line for lines l0, l1 ([p1 p2 abc len]) meeting in cell (r, c)
__device__ inline bool corner_of(const DP& P, const double* l0, const double* l1, int r, int c, double& ix, double& iy) {
    if (!(l0[9] > 0.1 && l1[9] > 0.1)) return false;
    const double angle = acos(vdot(vunit_div(vsub(ld3(l0), ld3(l0 + 3))), vunit_div(vsub(ld3(l1), ld3(l1 + 3)))));
    if (!(angle < 150.0 / 180.0 * kPi && angle > 30.0 / 180.0 * kPi)) return false;
    const double det = l0[6] * l1[7] - l0[7] * l1[6];
    ix = (-l0[8] * l1[7] + l1[8] * l0[7]) / det;
    iy = (-l0[6] * l1[8] + l1[6] * l0[8]) / det;
    int cc, cr;
    xy_to_index(P, ix, iy, cc, cr);
    const int dr = cr - r, dc = cc - c;
    return dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1;
}

// spawn_scan, one wavefront per scan, points and intermediates in LDS (layout at wave_lds, k_lfe.hpp): runs, corner response and the
// maxima's window test a lane per point; the skip after a maximum one lane over the maxima bits; the merge 64 tests at a time from
// the standing `last`; add_line a lane per candidate segment for the sums the host makes in index order (moment matrix, cyclic
// Jacobi, create_line), a lane per point for max_dis and the cells; ids by ballot prefix; the (cell, line) entries through a hash
// set in the dead point array, compacted and bitonic-sorted in LDS; scan::concers from the sorted entries.  Same store bytes as
// k_lfe_spawn for every valid slot (tests/test_gpu_laser_spawn_wave.py); an overflowed slot is left empty and invalid.
// 105 VGPRs, no scratch, 39 840 B of LDS at 1 080 points / 256 lines: four work-groups per CU (one wave per SIMD; the fp64 points
// alone are 25.9 KB, so LDS, not registers, sets the occupancy).
__global__ void __launch_bounds__(kBlock) k_lfe_spawn_wave(void* store, Lay L, DP P, WaveLds O, int slot, const double* pts, const int* n_pts,
                                                          const double* times, int max_corners, double* corners, int* n_corners) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= L.B) return;
    double* X = (double*)(lds + O.x);
    u64* brk = (u64*)(lds + O.brk);
    u64* mx = (u64*)(lds + O.mx);
    int* misc = (int*)(lds + O.misc);
    int* lbase = (int*)(lds + O.lbase);
    int* lcnt = (int*)(lds + O.lcnt);
    double* resp = (double*)(lds + O.u);
    unsigned* cell = (unsigned*)(lds + O.u);
    int2* cand = (int2*)(lds + O.cand);
    Slot sl = slot_at(store, L, b, slot);
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const double time = times ? times[b] : 0.0;
    const int N = n_pts[b];
    auto invalid = [&](unsigned st) {
        if (lane == 0) {
            slot_clear(sl, time);
            sl.h->status = (int)st;
            m->status |= st;
            if (n_corners) n_corners[b] = 0;
        }
    };
    if (N < 0 || N > L.max_points) { invalid(LIW_LFE_ST_POINTS); return; }
    const int W = (N + 63) >> 6;
    {
        const double* G = pts + (size_t)b * L.max_points * 3;
        for (int k = lane; k < 3 * N; k += kBlock) X[k] = G[k];
    }
    __syncthreads();
    auto Pt = [&](int i) { return ld3(X + 3 * i); };
    // continuous runs (:361-374): a lane per point, the run boundaries from the ballot
    for (int c = 0; c < W; ++c) {
        const int i = (c << 6) + lane;
        const bool bk = i >= 1 && i < N && !(vnorm(vsub(Pt(i - 1), Pt(i))) <= P.cont_thr);
        const u64 mask = __ballot(bk);
        if (lane == 0) brk[c] = mask;
    }
    __syncthreads();
    // corner response, once per interior point of a run
    for (int c = 0; c < W; ++c) {
        const int i = (c << 6) + lane;
        if (i < N) {
            const int s = run_start(brk, i), e = run_end(brk, W, N, i);
            double r = -1.0;
            if (i >= s + 1 && i <= e - 1) r = clac_cos(Pt(i), Pt(i - kStep > s ? i - kStep : s), Pt(i + kStep < e ? i + kStep : e));
            resp[i] = r;
        }
    }
    __syncthreads();
    // the window test of the strict local maxima (it does not depend on the skip after a maximum)
    for (int c = 0; c < W; ++c) {
        const int i = (c << 6) + lane;
        bool is_max = false;
        if (i < N) {
            const int s = run_start(brk, i), e = run_end(brk, W, N, i);
            if (i >= s + 1 && i <= e - 1) {
                const double ri = resp[i];
                is_max = true;
                const int bj = i - kStep > s + 1 ? i - kStep : s + 1, ej = i + kStep < e - 1 ? i + kStep : e - 1;
                for (int j = bj; j <= ej; ++j)
                    if (j != i && resp[j] >= ri) { is_max = false; break; }
            }
        }
        const u64 mask = __ballot(is_max);
        if (lane == 0) mx[c] = mask;
    }
    __syncthreads();
    // the skip after a maximum is a serial walk over the maxima bits: lane 0 lists, per run of at least three points, its
    // `ends` as [m, s, maxima .., e] in the cell region
    int* ends = (int*)cell;
    if (lane == 0) {
        int k = 0;
        for (int s = 0; s < N;) {
            const int e = run_end(brk, W, N, s);
            if (e - s >= 2) {
                const int hdr = k++;
                ends[k++] = s;
                for (int gi = s + 1; gi <= e - 1;) {
                    const int i = next_bit(mx, W, gi);
                    if (i < 0 || i > e - 1) break;
                    ends[k++] = i;
                    gi = i + kStep + 1;
                }
                ends[k++] = e;
                ends[hdr] = k - hdr - 1;
            }
            s = e + 1;
        }
        misc[1] = k;
    }
    __syncthreads();
    // the merge over `ends` (:294-302): while `last` stands, the tests of the following ends are independent, so the wave makes
    // 64 of them at once and the first that passes is the host's next split
    int nc_ = 0;
    {
        const int total = misc[1];
        auto emit = [&](int i1, int i2) { if (i2 - i1 >= 2) { if (lane == 0) cand[nc_] = make_int2(i1, i2); ++nc_; } };
        for (int k = 0; k < total;) {
            const int m = ends[k];
            const int* E = ends + k + 1;
            int last = 0;
            for (int i = 1; i + 1 < m;) {
                const int ii = i + lane;
                bool split = false;
                if (ii + 1 < m) {
                    const double angle = acos(clac_cos(Pt(E[ii]), Pt(E[last]), Pt(E[ii + 1])));
                    split = fabs(angle) < P.tol;
                }
                const u64 mask = __ballot(split);
                if (mask) {
                    const int hit = i + __ffsll((unsigned long long)mask) - 1;
                    emit(E[last], E[hit]);
                    last = hit;
                    i = hit + 1;
                } else {
                    i += kBlock;
                }
            }
            emit(E[last], E[m - 1]);
            k += m + 1;
        }
    }
    __syncthreads();
    const int nc = nc_;
    // add_line: a lane per candidate segment for what the host sums in index order (the six moment sums) and for the line's
    // cell list; the distances for max_dis (a maximum: any order gives the host's value, a NaN distance never wins on the host
    // either) and the points' cells are a lane per point.  Ids and entry offsets by prefix over the wave.
    u64* maxb = (u64*)(misc + 4);
    int* anyb = misc + 4 + 2 * kBlock;
    int id_base = 0;
    unsigned st = 0;
    for (int c0 = 0; c0 < nc; c0 += kBlock) {
        const int j = c0 + lane, cend = c0 + kBlock < nc ? c0 + kBlock : nc;
        bool accepted = false;
        int i1 = 0, i2 = 0;
        Vec p1(0, 0, 0), p2(0, 0, 0), abc(0, 0, 0), a(0, 0, 0), bb(0, 0, 0);
        double len = 0;
        if (j < nc) {
            i1 = cand[j].x; i2 = cand[j].y;
            double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int i = i1; i <= i2; ++i) {
                const double x = X[i * 3], y = X[i * 3 + 1];
                M[0][0] += x * x; M[0][1] += x * y; M[0][2] += x; M[1][1] += y * y; M[1][2] += y; M[2][2] += 1.0;
            }
            M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
            abc = smallest_eigvec3(M);
            if (fabs(abc.y) < 0.5) {
                a.y = 0; a.x = -abc.z / abc.x; bb.y = 1; bb.x = (-abc.z - abc.y) / abc.x;
            } else {
                a.x = 0; bb.x = 1; a.y = -abc.z / abc.y; bb.y = (-abc.z - abc.x) / abc.y;
            }
            p1 = project_to_line(Pt(i1), a, bb);
            p2 = project_to_line(Pt(i2), a, bb);
            len = vnorm(vsub(p1, p2));
        }
        maxb[lane] = 0;
        anyb[lane] = 0;
        __syncthreads();
        // a lane per point of the chunk's candidates; a point that ends one candidate and starts the next serves both
        const int lo = cand[c0].x, hi = cand[cend - 1].y;
        for (int i0 = lo; i0 <= hi; i0 += kBlock) {
            const bool in = i0 + lane <= hi;
            const int ii = in ? i0 + lane : hi;
            int jl = c0, jh = cend - 1;       // the last candidate of the chunk that starts at or before ii
            while (jl < jh) { const int mid = (jl + jh + 1) >> 1; if (cand[mid].x <= ii) jl = mid; else jh = mid - 1; }
            int c = 0, r = 0;
            xy_to_index(P, X[3 * ii], X[3 * ii + 1], c, r);
            const unsigned key = valid(P, r, c) ? (unsigned)(r * P.w + c) : ~0u;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int jj = jl - pass;
                const bool ok = in && (pass == 0 ? ii <= cand[jl].y : (jl > c0 && cand[jl - 1].y == ii));
                const int src = ok ? jj - c0 : 0;
                Vec la(__shfl(a.x, src), __shfl(a.y, src), 0.0), lb(__shfl(bb.x, src), __shfl(bb.y, src), 0.0);
                if (ok) {
                    const double d = dis_from_line(Pt(ii), la, lb);
                    if (d == d) atomicMax(&maxb[src], (u64)__double_as_longlong(d));
                    cell[ii + jj] = key;
                    if (key != ~0u) anyb[src] = 1;
                }
            }
        }
        __syncthreads();
        if (j < nc) {
            const double max_dis = __longlong_as_double((long long)maxb[lane]);
            accepted = !(max_dis > P.max_dis) && !(len < P.min_len);
        }
        const bool reg = accepted && anyb[lane] != 0;   // registers at least one valid cell: the line takes an id
        const u64 rm = __ballot(reg);
        const int id = id_base + __popcll(rm & ((1ull << lane) - 1));
        if (__ballot(accepted && id >= L.max_lines)) st |= LIW_LFE_ST_LINES;
        if (reg && id < L.max_lines) {
            double* o = sl.lines + 10 * (size_t)id;
            o[0] = p1.x; o[1] = p1.y; o[2] = p1.z; o[3] = p2.x; o[4] = p2.y; o[5] = p2.z; o[6] = abc.x; o[7] = abc.y; o[8] = abc.z; o[9] = len;
            lbase[id] = i1 + j;
            lcnt[id] = i2 - i1 + 1;
        }
        id_base += __popcll(rm);
        __syncthreads();
    }
    if (st) { invalid(st); return; }
    const int nl = id_base;
    // The line_map entries are the distinct (cell, line) pairs.  The points are dead: their bytes become a hash set the wave fills
    // a line at a time (lanes over the line's points), which is then compacted and sorted in place.
    u64* S = (u64*)X;
    const unsigned tmask = (unsigned)O.tcap - 1;
    for (int k = lane; k < O.tcap; k += kBlock) S[k] = ~0ull;
    __syncthreads();
    for (int id = 0; id < nl; ++id) {
        const int base = lbase[id], n = lcnt[id];
        for (int t = lane; t < n; t += kBlock) {
            const unsigned key = cell[base + t];
            if (key == ~0u) continue;
            const u64 item = ((u64)key << 32) | (unsigned)id;
            unsigned h = (unsigned)((item * 0x9E3779B97F4A7C15ull) >> 40) & tmask;
            for (unsigned probe = 0; probe <= tmask; ++probe) {   // the set is never full: fewer pairs than slots (wave_lds)
                const u64 old = atomicCAS((unsigned long long*)&S[h], ~0ull, (unsigned long long)item);
                if (old == ~0ull || old == item) break;
                h = (h + 1) & tmask;
            }
        }
    }
    __syncthreads();
    int ne = 0;
    for (int k0 = 0; k0 < O.tcap; k0 += kBlock) {
        const u64 v = k0 + lane < O.tcap ? S[k0 + lane] : ~0ull;
        const bool has = v != ~0ull;
        const u64 mask = __ballot(has);
        __syncthreads();
        if (has) S[ne + __popcll(mask & ((1ull << lane) - 1))] = v;
        ne += __popcll(mask);
        __syncthreads();
    }
    if (ne > L.max_entries) { invalid(LIW_LFE_ST_CELLS); return; }
    wave_sort(S, ne, lane);
    for (int k = lane; k < ne; k += kBlock) sl.ent[k] = S[k];
    if (lane == 0) { sl.h->status = 0; sl.h->n_lines = nl; sl.h->n_entries = ne; sl.h->time = time; }
    if (!corners) return;
    // scan::concers: the entry that is second in its cell belongs to the line l1 that made the host's test there, the entry before
    // it to l0.  Push order = (l1, first point of l1 in the cell): the hits are listed behind the entries as (l1, point, l0) (16
    // bits each for point and l0: max_points and max_lines are far below that where the LDS fits), sorted and written.
    double* C = corners + (size_t)b * max_corners * 3;
    u64* R = S + ne;
    int nr = 0;
    for (int p0 = 0; p0 < ne; p0 += kBlock) {
        const int p = p0 + lane;
        u64 rec = 0;
        bool hit = false;
        if (p >= 1 && p < ne) {
            const u64 e1 = S[p], e0 = S[p - 1];
            const unsigned key = (unsigned)(e1 >> 32);
            if ((unsigned)(e0 >> 32) == key && (p < 2 || (unsigned)(S[p - 2] >> 32) != key)) {
                const unsigned l1 = (unsigned)(e1 & 0xffffffffull), l0 = (unsigned)(e0 & 0xffffffffull);
                double ix, iy;
                if (corner_of(P, sl.lines + 10 * (size_t)l0, sl.lines + 10 * (size_t)l1, (int)(key / (unsigned)P.w), (int)(key % (unsigned)P.w), ix, iy)) {
                    const int base = lbase[l1], n = lcnt[l1];
                    int t = 0;
                    while (t < n - 1 && cell[base + t] != key) ++t;
                    rec = ((u64)l1 << 32) | ((u64)(unsigned)t << 16) | l0;
                    hit = true;
                }
            }
        }
        const u64 mask = __ballot(hit);
        if (hit) R[nr + __popcll(mask & ((1ull << lane) - 1))] = rec;
        nr += __popcll(mask);
    }
    __syncthreads();
    wave_sort(R, nr, lane);
    for (int q = lane; q < nr && q < max_corners; q += kBlock) {
        const u64 rec = R[q];
        const double* l0 = sl.lines + 10 * (size_t)(rec & 0xffffull);
        const double* l1 = sl.lines + 10 * (size_t)(rec >> 32);
        const double det = l0[6] * l1[7] - l0[7] * l1[6];
        C[3 * q] = (-l0[8] * l1[7] + l1[8] * l0[7]) / det;
        C[3 * q + 1] = (-l0[6] * l1[8] + l1[6] * l0[8]) / det;
        C[3 * q + 2] = 0.0;
    }
    if (lane == 0) {
        n_corners[b] = nr > max_corners ? max_corners + 1 : nr;
        if (nr > max_corners) m->status |= LIW_LFE_ST_CORNERS;
    }
}

// lvio_2d::trajectory's accumulation of the corners between key frames: world = make_tf(pose) * T_imu_to_laser * corner
__global__ void __launch_bounds__(kBlock) k_lfe_corners_world(void* store, Lay L, DP P, int max_corners, const double* corners, const int* n_corners,
                                                             const double* pose, const unsigned char* mask, const unsigned char* clear, int acc_cap,
                                                             double* acc, int* n_acc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    int n = (clear && clear[b]) ? 0 : n_acc[b];
    if (n < 0) n = 0;
    if (!mask || mask[b]) {
        const int nc = n_corners[b];
        if (n > acc_cap || nc > max_corners || (nc > 0 && n + nc > acc_cap)) {
            n = acc_cap + 1;
            if (store) ((Mgr*)robot_ptr(store, L, b))->status |= LIW_LFE_ST_CORNERS;
        } else if (nc > 0) {
            const Iso<double> T = liw::mul(tf6(pose + 6 * (size_t)b), til(P));
            const double* C = corners + (size_t)b * max_corners * 3;
            double* A = acc + ((size_t)b * acc_cap + n) * 3;
            for (int k = 0; k < nc; ++k) {
                const Vec y = apply(T, ld3(C + 3 * k));
                A[3 * k] = y.x; A[3 * k + 1] = y.y; A[3 * k + 2] = y.z;
            }
            n += nc;
        }
    }
    n_acc[b] = n;
}

// ---------------------------------------------------------------------------------------------------------------- sub-maps
// laser_manager::clear_all_scan: the manager record, every scan slot and both sub-maps
__global__ void __launch_bounds__(kBlock) k_lfe_reset(void* store, Lay L, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    char* mz = (char*)m;
    for (size_t k = 0; k < kMgrBytes; ++k) mz[k] = 0;
    for (int k = 0; k < L.slots + 2; ++k) { Slot s = slot_at(store, L, b, k); slot_clear(s, 0.0); }
}

// clear_all_scan's effect on the manager alone: state, status word and both sub-maps; the scan slots stay (liw_lfe_rebuild)
__global__ void __launch_bounds__(kBlock) k_lfe_reset_mgr(void* store, Lay L, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    char* mz = robot_ptr(store, L, b);
    for (size_t k = 0; k < kMgrBytes; ++k) mz[k] = 0;
    for (int k = L.slots; k < L.slots + 2; ++k) { Slot s = slot_at(store, L, b, k); slot_clear(s, 0.0); }
}

// fresh_submap (laser_manager.cpp / liw_laser.cpp): the scan's lines as segments, untransformed
// src_st: the source scan's status (nonzero: the sub-map is invalid as well)
__device__ void fresh_submap(void* store, const Lay& L, const DP& P, int b, Mgr* m, int sub, const Slot& src, unsigned src_st, const double* pose) {
    Slot s = slot_at(store, L, b, L.slots + sub);
    slot_clear(s, 0.0);
    unsigned st = src_st;
    for (int i = 0, nl = n_lines(src, L); i < nl; ++i) add_segment(s, L, P, ld3(src.lines + 10 * (size_t)i), ld3(src.lines + 10 * (size_t)i + 3), st);
    sort_entries(s.ent, n_entries(s, L));
    s.h->status = (int)st;
    m->status |= st;
    for (int k = 0; k < 3; ++k) { m->sub_p[sub][k] = pose[k]; m->sub_q[sub][k] = pose[3 + k]; }
}
__device__ inline void set_last(Mgr* m, const Iso<double>& T) {
    for (int k = 0; k < 9; ++k) m->last_R[k] = T.R.m[k];
    m->last_t[0] = T.t.x; m->last_t[1] = T.t.y; m->last_t[2] = T.t.z;
}

// laser_manager::add_scan (:424-496) without the key-frame deque
// pose of robot b at pose + b * pose_stride doubles (6 for a packed [B][6] array); flags (may be null): LIW_LFE_ADD_* per robot
__global__ void __launch_bounds__(kBlock) k_lfe_add_scan(void* store, Lay L, DP P, int src_slot, const double* pose, long long pose_stride,
                                                        const unsigned char* mask, unsigned char* flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    if (mask && !mask[b]) { if (flags) flags[b] = 0; return; }
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const Slot src = slot_at(store, L, b, src_slot);
    // an invalid source scan invalidates every sub-map this call writes (until that sub-map is replaced)
    const unsigned src_st = src.h->status ? ((unsigned)src.h->status | LIW_LFE_ST_INVALID) : 0u;
    m->status |= src_st;
    const double* pq = pose + (long long)b * pose_stride;
    const Iso<double> cur = tf6(pq);
    if (m->has_ref) {
        const Iso<double> last = liw::cast_iso<double>(m->last_R, m->last_t);
        const Iso<double> d = liw::mul(liw::inverse(last), cur);
        const Vec dq = liw::log_SO3(d.R);
        if (vnorm(d.t) < P.mf_p && vnorm(dq) < P.mf_q) { if (flags) flags[b] = 0; return; }
    } else {
        fresh_submap(store, L, P, b, m, m->ref_sub & 1, src, src_st, pq);
        m->has_ref = 1;
        set_last(m, cur);
        m->count = 1;
        if (flags) flags[b] = LIW_LFE_ADD_ADDED | LIW_LFE_ADD_FIRST;
        return;
    }
    unsigned fl = LIW_LFE_ADD_ADDED;
    const Iso<double> Ti = til(P);
    auto accumulate = [&](int sub) {
        const double sp[6] = {m->sub_p[sub][0], m->sub_p[sub][1], m->sub_p[sub][2], m->sub_q[sub][0], m->sub_q[sub][1], m->sub_q[sub][2]};
        const Iso<double> rel = liw::mul(liw::inverse(tf6(sp)), cur);
        return liw::mul(liw::mul(liw::inverse(Ti), rel), Ti);
    };
    const int rs = m->ref_sub & 1, ss = 1 - rs;
    const bool has_sp = m->has_spawn != 0;
    const Iso<double> l_ref = accumulate(rs);
    const Iso<double> l_sp = has_sp ? accumulate(ss) : l_ref;
    Slot sr = slot_at(store, L, b, L.slots + rs), sp = slot_at(store, L, b, L.slots + ss);
    unsigned st_r = src_st, st_s = src_st;
    for (int i = 0, nl = n_lines(src, L); i < nl; ++i) {
        const Vec a = ld3(src.lines + 10 * (size_t)i), c = ld3(src.lines + 10 * (size_t)i + 3);
        add_segment(sr, L, P, apply(l_ref, a), apply(l_ref, c), st_r);
        if (has_sp) add_segment(sp, L, P, apply(l_sp, a), apply(l_sp, c), st_s);
    }
    sort_entries(sr.ent, n_entries(sr, L));
    sr.h->status |= (int)st_r;
    if (has_sp) { sort_entries(sp.ent, n_entries(sp, L)); sp.h->status |= (int)st_s; }
    m->status |= st_r | st_s;
    ++m->count;
    if (!m->has_spawn && m->count == P.n_acc / 2) {
        fresh_submap(store, L, P, b, m, ss, src, src_st, pq);
        m->has_spawn = 1;
        fl |= LIW_LFE_ADD_SPAWNED;
    }
    if (m->count == P.n_acc) {   // ref = spawning (which may not exist: the /2 quirk of ref_n_accumulation 2); spawning = fresh
        const int nr = 1 - rs;
        m->has_ref = m->has_spawn;
        m->ref_sub = nr;
        fresh_submap(store, L, P, b, m, 1 - nr, src, src_st, pq);
        m->has_spawn = 1;
        m->count = P.n_acc / 2;
        fl |= LIW_LFE_ADD_SWAPPED;
    }
    set_last(m, cur);
    if (flags) flags[b] = (unsigned char)fl;
}

// ------------------------------------------------------------------------------------------------ wave-per-robot add_scan
// One work-group of one wave per robot.  The manager's branch (make_tf, the motion filter, count, the n_acc / 2 spawn, the swap) is
// evaluated by every lane from the same bytes with the device functions of k_lfe_add_scan, so it is wave-uniform and decides as
// the lane kernel does; lane 0 writes the Mgr record.  The call's targets (reference, spawning sub-map, then the fresh
// sub-maps) are independent slots and are done one after another by the one wave (add_target_wave).
//
// A target, in two passes over the source lines in chunks of 64, a lane per line:
//   pass 1  apply + line_fit (the body of add_line) and a first walk of the lane's own segment, the lane kernel's
//           `for (tr = 0; tr <= len; tr += 0.05)` with tr the running sum, which counts the line's cells.  Ids: the running n_lines
//           plus the ballot prefix over the accepted lines with a valid cell; entry offsets: the running total plus the prefix sum
//           of the counts.  The line record goes to lines[id] at once (bytes past the header's n_lines are nobody's until the
//           header moves); id and offset of every source line stay in LDS (lid, loff [max_lines]).
//   pass 2  the second walk writes (cell << 32 | id) at the line's offset of the new-entry buffer in LDS (nw [ecap]).
// De-duplication: the lane kernel's backward search only meets cells of the line itself.  x = p1.x + unit.x * tr is monotone
// in tr (a rounded product and a rounded sum are monotone in one operand), so are x / res + w / 2 and its truncation, and
// likewise the row: the cell sequence of a walk is monotone in each coordinate and cannot return to a cell it has left, also
// after the invalid cells are dropped.  Distinct cells = consecutive-distinct cells, which is what seg_cells keeps.
// Then wave_sort of nw in LDS and the merge into the sorted old entries in place: the final index of new entry j is j + the
// number of old entries below it (binary search, kept in pos [ecap] before anything moves), of old entry i it is i + the number of
// new entries below it; the old entries move back to front in chunks of 64 (read, barrier, write: an entry only moves to an
// index at or above its own, and everything above the chunk has moved), stopping at the first chunk nothing of which moves.
// (cell, id) pairs are all distinct, so the sorted list, hence every byte below n_lines / n_entries, is the lane kernel's.
// No atomics; positions are prefix counts.
//
// Escape: when pass 1 finds that the lane kernel would flag the target (an accepted line at id >= max_lines, or n_old + new >
// max_cell_entries), or that the call's new entries exceed ecap (kAddNewCap), lane 0 alone runs the lane kernel's serial code
// on that target (add_target_serial: add_segment + sort_entries), from the untouched header: the bytes of an overflowed
// sub-map are then the lane kernel's too, and nothing is truncated.
//
// Same manager record, sub-map headers, lines[0 .. n_lines) and ent[0 .. n_entries) as k_lfe_add_scan
// (tests/test_gpu_laser_add_scan_wave.py).  236 VGPRs, no scratch, 26 624 B of LDS at 256 lines: two waves per SIMD by registers,
// six work-groups per CU by LDS.

// exclusive prefix sum over the wave (all 64 lanes must call it)
__device__ inline int wave_excl(int v, int lane, int& total) {
    int x = v;
#pragma unroll
    for (int d = 1; d < kBlock; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
    total = __shfl(x, kBlock - 1);
    return x - v;
}

// one target of k_lfe_add_scan as the lane kernel does it (one lane); returns the status bits of the target
__device__ unsigned add_target_serial(Slot s, const Lay& L, const DP& P, const Slot& src, const Iso<double>* xf, unsigned src_st) {
    if (!xf) slot_clear(s, 0.0);
    unsigned st = src_st;
    for (int i = 0, nl = n_lines(src, L); i < nl; ++i) {
        const Vec a = ld3(src.lines + 10 * (size_t)i), c = ld3(src.lines + 10 * (size_t)i + 3);
        if (xf) add_segment(s, L, P, apply(*xf, a), apply(*xf, c), st);
        else add_segment(s, L, P, a, c, st);
    }
    sort_entries(s.ent, n_entries(s, L));
    if (xf) s.h->status |= (int)st;
    else s.h->status = (int)st;
    return st;
}

// one target by the wave: xf != null accumulates the transformed lines into the existing sub-map, xf == null makes it afresh from
// the untransformed lines (fresh_submap).  Wave-uniform control flow; returns the target's status bits (uniform).
__device__ unsigned add_target_wave(Slot s, const Lay& L, const DP& P, const AddLds& O, unsigned char* lds, const Slot& src, const Iso<double>* xf,
                                    unsigned src_st, int lane) {
    u64* nw = (u64*)(lds + O.nw);
    int* pos = (int*)(lds + O.pos);
    int* lid = (int*)(lds + O.lid);
    int* loff = (int*)(lds + O.loff);
    const int nl = n_lines(src, L);
    const int n0l = xf ? n_lines(s, L) : 0, n0e = xf ? n_entries(s, L) : 0;
    int run_l = n0l, tot = 0;
    bool ovf = false;
    for (int base = 0; base < nl; base += kBlock) {
        const int i = base + lane;
        bool acc = false;
        int cnt = 0;
        Vec p1, p2, abc;
        double len = 0;
        if (i < nl) {
            Vec a = ld3(src.lines + 10 * (size_t)i), c = ld3(src.lines + 10 * (size_t)i + 3);
            if (xf) { a = apply(*xf, a); c = apply(*xf, c); }
            const Vec mid = Vec((c.x + a.x) / 2, (c.y + a.y) / 2, (c.z + a.z) / 2);   // add_segment
            const double fake[9] = {a.x, a.y, a.z, mid.x, mid.y, mid.z, c.x, c.y, c.z};
            acc = line_fit(P, fake, 0, 2, p1, p2, abc, len);
            if (acc) cnt = seg_cells(P, p1, p2, len, [](int, unsigned) {});
        }
        const bool reg = acc && cnt > 0;
        const u64 rm = __ballot(reg);
        const int id = run_l + __popcll(rm & ((1ull << lane) - 1));
        if (__ballot(acc && id >= L.max_lines)) ovf = true;
        int total;
        const int off = wave_excl(reg ? cnt : 0, lane, total);
        if (ovf) break;
        if (i < nl) { lid[i] = reg ? id : -1; loff[i] = tot + off; }
        if (reg) {
            double* o = s.lines + 10 * (size_t)id;
            o[0] = p1.x; o[1] = p1.y; o[2] = p1.z; o[3] = p2.x; o[4] = p2.y; o[5] = p2.z; o[6] = abc.x; o[7] = abc.y; o[8] = abc.z; o[9] = len;
        }
        run_l += __popcll(rm);
        tot += total;
        if (tot > O.ecap || n0e + tot > L.max_entries) { ovf = true; break; }
    }
    __syncthreads();
    if (ovf) {
        unsigned st = 0;
        if (lane == 0) st = add_target_serial(s, L, P, src, xf, src_st);
        __syncthreads();
        return (unsigned)__shfl((int)st, 0);
    }
    for (int base = 0; base < nl; base += kBlock) {
        const int i = base + lane;
        if (i < nl && lid[i] >= 0) {
            const int id = lid[i], o0 = loff[i];
            const double* o = s.lines + 10 * (size_t)id;   // this lane's own record of pass 1
            seg_cells(P, ld3(o), ld3(o + 3), o[9], [&](int k, unsigned cell) { if (o0 + k < O.ecap) nw[o0 + k] = ((u64)cell << 32) | (unsigned)id; });   // o0 + k < tot <= ecap: the walk of pass 1
        }
    }
    __syncthreads();
    wave_sort(nw, tot, lane);
    if (n0e == 0) {
        for (int j = lane; j < tot; j += kBlock) s.ent[j] = nw[j];
    } else if (tot > 0) {
        for (int j = lane; j < tot; j += kBlock) pos[j] = j + lower_bound(s.ent, n0e, nw[j]);
        __syncthreads();
        for (int top = n0e; top > 0; top -= kBlock) {
            const int i = top - kBlock + lane;
            u64 v = 0;
            int r = 0;
            if (i >= 0) { v = s.ent[i]; r = lower_bound(nw, tot, v); }
            __syncthreads();
            if (r > 0) s.ent[i + r] = v;
            __syncthreads();
            if (!__ballot(r > 0)) break;
        }
        for (int j = lane; j < tot; j += kBlock) s.ent[pos[j]] = nw[j];
    }
    if (lane == 0) {
        if (xf) s.h->status |= (int)src_st;
        else { s.h->status = (int)src_st; s.h->time = 0.0; }
        s.h->n_lines = run_l;
        s.h->n_entries = n0e + tot;
    }
    __syncthreads();
    return src_st;
}

// add_scan of one robot's scan slot by its wave; returns the LIW_LFE_ADD_* flags (uniform)
__device__ unsigned add_scan_wave_one(void* store, const Lay& L, const DP& P, const AddLds& O, unsigned char* lds, int b, int src_slot, const double* pq,
                                      int lane) {
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const Slot src = slot_at(store, L, b, src_slot);
    const unsigned src_st = src.h->status ? ((unsigned)src.h->status | LIW_LFE_ST_INVALID) : 0u;
    unsigned mst = (unsigned)m->status | src_st;
    int has_ref = m->has_ref, has_spawn = m->has_spawn, count = m->count;
    const int rs = m->ref_sub & 1, ss = 1 - rs;
    int ref_sub = m->ref_sub;
    auto fresh = [&](int sub) {   // fresh_submap
        mst |= add_target_wave(slot_at(store, L, b, L.slots + sub), L, P, O, lds, src, nullptr, src_st, lane);
        if (lane == 0)
            for (int k = 0; k < 3; ++k) { m->sub_p[sub][k] = pq[k]; m->sub_q[sub][k] = pq[3 + k]; }
    };
    if (has_ref) {
        const Iso<double> last = liw::cast_iso<double>(m->last_R, m->last_t);
        const Iso<double> d = liw::mul(liw::inverse(last), tf6(pq));
        const Vec dq = liw::log_SO3(d.R);
        if (vnorm(d.t) < P.mf_p && vnorm(dq) < P.mf_q) {
            if (lane == 0) m->status = (int)mst;
            return 0u;
        }
    } else {
        fresh(rs);
        if (lane == 0) { m->status = (int)mst; m->has_ref = 1; set_last(m, tf6(pq)); m->count = 1; }
        return LIW_LFE_ADD_ADDED | LIW_LFE_ADD_FIRST;
    }
    unsigned fl = LIW_LFE_ADD_ADDED;
    const Iso<double> Ti = til(P);
    auto accumulate = [&](int sub) {
        const double sp[6] = {m->sub_p[sub][0], m->sub_p[sub][1], m->sub_p[sub][2], m->sub_q[sub][0], m->sub_q[sub][1], m->sub_q[sub][2]};
        const Iso<double> rel = liw::mul(liw::inverse(tf6(sp)), tf6(pq));   // make_tf of the pose again, not kept live across the targets
        return liw::mul(liw::mul(liw::inverse(Ti), rel), Ti);
    };
    {   // one transform live at a time (registers); both sub-map poses are read before a fresh sub-map below replaces them
        const Iso<double> l_ref = accumulate(rs);
        mst |= add_target_wave(slot_at(store, L, b, L.slots + rs), L, P, O, lds, src, &l_ref, src_st, lane);
    }
    if (has_spawn) {
        const Iso<double> l_sp = accumulate(ss);
        mst |= add_target_wave(slot_at(store, L, b, L.slots + ss), L, P, O, lds, src, &l_sp, src_st, lane);
    }
    ++count;
    if (!has_spawn && count == P.n_acc / 2) {
        fresh(ss);
        has_spawn = 1;
        fl |= LIW_LFE_ADD_SPAWNED;
    }
    if (count == P.n_acc) {
        const int nr = 1 - rs;
        has_ref = has_spawn;
        ref_sub = nr;
        fresh(1 - nr);
        has_spawn = 1;
        count = P.n_acc / 2;
        fl |= LIW_LFE_ADD_SWAPPED;
    }
    if (lane == 0) {
        m->status = (int)mst; m->has_ref = has_ref; m->has_spawn = has_spawn; m->ref_sub = ref_sub; m->count = count;
        set_last(m, tf6(pq));
    }
    return fl;
}

// liw_lfe_add_scan (F = 1, reset = 0) and liw_lfe_rebuild (reset = 1: k_lfe_reset_mgr, then frames 0 .. F-1 in program order) for
// robot b = blockIdx.x; pose of frame k at pose + b * robot_stride + k * frame_stride; flags (may be null): of the last frame
__global__ void __launch_bounds__(kBlock) k_lfe_add_scan_wave(void* store, Lay L, DP P, AddLds O, int first_slot, int F, int reset, const double* pose,
                                                             long long robot_stride, long long frame_stride, const unsigned char* mask,
                                                             unsigned char* flags) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= L.B) return;
    if (mask && !mask[b]) {
        if (flags && lane == 0) flags[b] = 0;
        return;
    }
    if (reset) {
        ((int*)robot_ptr(store, L, b))[lane] = 0;   // kMgrBytes = 64 lanes x 4
        if (lane < 2) { Slot s = slot_at(store, L, b, L.slots + lane); slot_clear(s, 0.0); }
        __syncthreads();
    }
    unsigned fl = 0;
    for (int k = 0; k < F; ++k) {
        fl = add_scan_wave_one(store, L, P, O, lds, b, first_slot + k, pose + (long long)b * robot_stride + (long long)k * frame_stride, lane);
        __syncthreads();
    }
    if (flags && lane == 0) flags[b] = (unsigned char)fl;
}
static_assert(kMgrBytes == 4 * kBlock, "k_lfe_add_scan_wave clears the manager record a lane per word");

// Scan slot 0 -> slot dst_slot[b] of the same robot: the 32-byte header (status word, n_lines, n_entries, time), lines[0 .. n_lines)
// and ent[0 .. n_entries).  A work-group of 256 per robot, 16-byte loads and stores: slots start on 256-byte boundaries, a line is
// five 16-byte words and the entries start on one; an odd entry count ends with one 8-byte copy.  Nothing is computed: the kernel
// is bounded by the store traffic, at most slot_bytes read and written per robot (about 86 KB at 256 lines / 8 192 entries).
__global__ void __launch_bounds__(256) k_lfe_slot_copy(void* store, Lay L, const int* dst_slot, const unsigned char* mask) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    const int d = dst_slot[b];
    if (d < 1 || d >= L.slots) {
        if (t == 0) ((Mgr*)robot_ptr(store, L, b))->status |= LIW_LFE_ST_INVALID;
        return;
    }
    const Slot s = slot_at(store, L, b, 0), o = slot_at(store, L, b, d);
    const int nl = n_lines(s, L), ne = n_entries(s, L);
    typedef ulonglong2 W;   // 16 bytes
    const W* sl = (const W*)s.lines;
    W* ol = (W*)o.lines;
    for (int i = t; i < 5 * nl; i += 256) ol[i] = sl[i];
    const W* se = (const W*)s.ent;
    W* oe = (W*)o.ent;
    for (int i = t; i < ne / 2; i += 256) oe[i] = se[i];
    if ((ne & 1) && t == 0) o.ent[ne - 1] = s.ent[ne - 1];
    if (t < 2) ((W*)o.h)[t] = ((const W*)s.h)[t];
}

int launch_ranges(void* store, const Lay& L, const float* ranges, int n_rays, const float2* cs, float tinc, const double* stamps, double* pts,
                  double* times, int* n_pts, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_ranges, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, ranges, n_rays, cs, tinc, stamps, pts, times, n_pts);
    return launched();
}

int launch_deskew(const Lay& L, double* pts, const double* times, const int* n_pts, const double* stamps, const double* lin, const double* ang,
                  hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_deskew, dim3(blocks((size_t)L.B * L.max_points, 256)), dim3(256), 0, s, L, pts, times, n_pts, stamps, lin, ang);
    return launched();
}

int launch_spawn(void* store, const Lay& L, const DP& P, int slot, const double* pts, const int* n_pts, const double* times, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_spawn, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, P, slot, pts, n_pts, times);
    return launched();
}

int launch_spawn_wave(void* store, const Lay& L, const DP& P, const WaveLds& O, int slot, const double* pts, const int* n_pts, const double* times,
                      int max_corners, double* corners, int* n_corners, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_spawn_wave, dim3(L.B), dim3(kBlock), O.total, s, store, L, P, O, slot, pts, n_pts, times, max_corners, corners, n_corners);
    return launched();
}

int launch_corners_world(void* store, const Lay& L, const DP& P, int max_corners, const double* corners, const int* n_corners, const double* pose,
                         const unsigned char* mask, const unsigned char* clear, int acc_cap, double* acc, int* n_acc, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_corners_world, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, P, max_corners, corners, n_corners, pose, mask, clear,
                       acc_cap, acc, n_acc);
    return launched();
}

int launch_reset(void* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_reset, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, mask);
    return launched();
}

int launch_reset_mgr(void* store, const Lay& L, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_reset_mgr, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, mask);
    return launched();
}

int launch_add_scan(void* store, const Lay& L, const DP& P, int src_slot, const double* pose, long long pose_stride, const unsigned char* mask,
                    unsigned char* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_add_scan, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, P, src_slot, pose, pose_stride, mask, flags);
    return launched();
}

int launch_add_scan_wave(void* store, const Lay& L, const DP& P, const AddLds& O, int first_slot, int F, int reset, const double* pose,
                         long long robot_stride, long long frame_stride, const unsigned char* mask, unsigned char* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_add_scan_wave, dim3(L.B), dim3(kBlock), O.total, s, store, L, P, O, first_slot, F, reset, pose, robot_stride, frame_stride,
                       mask, flags);
    return launched();
}

int launch_slot_copy(void* store, const Lay& L, const int* dst_slot, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_slot_copy, dim3(L.B), dim3(256), 0, s, store, L, dst_slot, mask);
    return launched();
}

}  // namespace lfe
