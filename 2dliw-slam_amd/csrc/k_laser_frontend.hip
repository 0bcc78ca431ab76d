// k_laser_frontend.hip — the batched laser front-end on the MI355X (C ABI include/liw_laser_batch.h): liw_laser.cpp's
// tracking-time work for B robots at once, its output landing in the device arrays liw_batch takes.
//
// Mapping: one lane per (robot, scan).  Every step of the host front-end is a serial chain over one scan (the 1 cm filter
// compares against the previously KEPT point, the corner maxima skip `step` after each maximum, the segment merge carries
// `last`, a line's cells are de-duplicated against its earlier cells, the mean match distance is summed in match order),
// so a lane walks its scan in the host's order and rounds as the host does; the batch is the parallelism.
//   k_lfe_ranges   ranges -> points (+ times): the (cosf, sinf) table of the geometry comes from the host libm (ctx)
//   k_lfe_deskew   one lane per point: make_tf(dt * twist) * p
//   k_lfe_spawn    continuous runs -> corner response -> strict local maxima -> merge -> add_line (moment matrix, cyclic
//                  Jacobi, create_line, gates) -> cell entries; then the slot's entries are heap-sorted by (cell, line)
//   k_lfe_match    per line of s2 in scan::lines order: candidates of the (2kk+3)^2 cells by binary search of the sorted
//                  entries (dr, dc, push order), strict-< argmin of the angle, 10 degree gate; two passes (mean, then keep)
//   k_lfe_add_scan laser_manager::add_scan: motion filter, fresh sub-maps, add_segment rasterisation, the swap
//   k_lfe_scan / k_lfe_pack   laser_off exclusive scan (one block), then the component-major laser arrays
// The line_map of a slot is a list of 64-bit entries (cell key << 32 | line index) kept sorted: within a cell the host
// pushes line ids in increasing order (ids only grow and a cell never takes the same id twice in a row), so sorting by
// (cell, line index) reproduces the host's push order exactly.
// No floating-point atomics, no inter-lane communication in the per-robot kernels: runs are bitwise reproducible.
#pragma clang fp contract(off)   // the x86-64 host build of liw_laser.cpp does not contract; hipcc contracts device code by default

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_laser_batch.h"
#include "liw_dual.hpp"

void liw_normalize_rotation_host(double* R9);   // liw_capi.hip (params.cpp:44-54 round trip)

namespace lfe {

using liw::Iso;
using liw::M3;
using liw::V3;
typedef V3<double> Vec;
typedef unsigned long long u64;

constexpr double kEps = 0.0008;             // epsilo, laser_manager.cpp:3
constexpr double kPi = 3.14159265358979323846;
constexpr int kStep = 3;
constexpr int kBlock = 64;

struct DP {                // laser parameters as the kernels use them
    double res, cont_thr, min_len, max_dis, tol, mf_p, mf_q;
    int w, h, n_acc;
    double Til_R[9], Til_t[3];
};
struct Lay {
    size_t robot_bytes, slot_bytes;
    int B, slots, max_points, max_lines, max_entries;
};
struct Mgr {               // laser_manager state of one robot (256 bytes in the store)
    int status, has_ref, has_spawn, ref_sub;
    int count, pad0, pad1, pad2;
    double sub_p[2][3], sub_q[2][3];
    double last_R[9], last_t[3];
};
struct SlotHdr { int status, n_lines, n_entries, pad; double time, pad2; };
constexpr size_t kMgrBytes = 256, kHdrBytes = 32;
static_assert(sizeof(Mgr) <= kMgrBytes, "manager record");
static_assert(sizeof(SlotHdr) == kHdrBytes, "slot header");

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
// store: robot-major; robot b = [Mgr | slot 0 .. slots-1 | sub-map 0 | sub-map 1]; slot = [SlotHdr | lines [max_lines][10] | entries]
inline bool make_lay(const liw_lfe_dims* d, Lay& L) {
    if (!d || d->B <= 0 || d->slots <= 0 || d->max_points <= 0 || d->max_lines <= 0 || d->max_cell_entries <= 0) return false;
    L.B = d->B; L.slots = d->slots; L.max_points = d->max_points; L.max_lines = d->max_lines; L.max_entries = d->max_cell_entries;
    L.slot_bytes = align256(kHdrBytes + 80 * (size_t)d->max_lines + 8 * (size_t)d->max_cell_entries);
    L.robot_bytes = kMgrBytes + (size_t)(d->slots + 2) * L.slot_bytes;
    return true;
}

struct Slot { SlotHdr* h; double* lines; u64* ent; };
__host__ __device__ inline char* robot_ptr(void* store, const Lay& L, int b) { return (char*)store + (size_t)b * L.robot_bytes; }
__host__ __device__ inline size_t slot_off(const Lay& L, int phys) { return kMgrBytes + (size_t)phys * L.slot_bytes; }
__device__ inline Slot slot_at(void* store, const Lay& L, int b, int phys) {
    char* p = robot_ptr(store, L, b) + slot_off(L, phys);
    Slot s;
    s.h = (SlotHdr*)p;
    s.lines = (double*)(p + kHdrBytes);
    s.ent = (u64*)(p + kHdrBytes + 80 * (size_t)L.max_lines);
    return s;
}
__device__ inline int n_lines(const Slot& s, const Lay& L) { const int n = s.h->n_lines; return n < 0 ? 0 : (n > L.max_lines ? L.max_lines : n); }
__device__ inline int n_entries(const Slot& s, const Lay& L) { const int n = s.h->n_entries; return n < 0 ? 0 : (n > L.max_entries ? L.max_entries : n); }
__device__ inline void slot_clear(Slot& s, double time) { s.h->status = 0; s.h->n_lines = 0; s.h->n_entries = 0; s.h->time = time; }

// ------------------------------------------------------------------ geometry, as liw_laser.cpp does it (same operation order)
__device__ inline Vec vsub(const Vec& a, const Vec& b) { return Vec(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline Vec vadd(const Vec& a, const Vec& b) { return Vec(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline Vec vscale(const Vec& a, double s) { return Vec(a.x * s, a.y * s, a.z * s); }
__device__ inline double vdot(const Vec& a, const Vec& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline double vnorm(const Vec& a) { return sqrt(vdot(a, a)); }
__device__ inline Vec vunit_div(const Vec& a) { const double z = vdot(a, a); if (!(z > 0.0)) return a; const double n = sqrt(z); return Vec(a.x / n, a.y / n, a.z / n); }
__device__ inline Vec apply(const Iso<double>& T, const Vec& p) { return vadd(liw::mul(T.R, p), T.t); }
__device__ inline Vec ld3(const double* p) { return Vec(p[0], p[1], p[2]); }

__device__ inline double dis_from_line(const Vec& p, const Vec& p1, const Vec& p2) {
    const Vec line = vunit_div(vsub(p2, p1));
    const Vec p2p = vsub(p, p2);
    const double t = vdot(vunit_div(line), p2p);
    return vnorm(vsub(p2p, vscale(line, t)));
}
__device__ inline Vec project_to_line(const Vec& p, const Vec& a, const Vec& b) {
    if (vnorm(vsub(b, a)) < kEps) return p;
    const Vec u = vunit_div(vsub(b, a));
    return vadd(a, vscale(u, vdot(vsub(p, a), u)));
}
__device__ inline double clac_cos(const Vec& pj, const Vec& pi, const Vec& pk) {
    if (vnorm(vsub(pi, pj)) < kEps) return -1;
    if (vnorm(vsub(pj, pk)) < kEps) return -1;
    return vdot(vunit_div(vsub(pi, pj)), vunit_div(vsub(pk, pj)));
}
__host__ __device__ inline void xy_to_index(const DP& P, double x, double y, int& c, int& r) {
    c = (int)(x / P.res + (double)(P.w / 2));
    r = (int)(y / P.res + (double)(P.h / 2));
}
__host__ __device__ inline bool valid(const DP& P, int r, int c) { return r >= 0 && r < P.h && c >= 0 && c < P.w; }

// smallest eigenvector of a symmetric 3x3 (cyclic Jacobi), liw_laser.cpp smallest_eigvec3
__device__ Vec smallest_eigvec3(double M[3][3]) {
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
__device__ void sort_entries(u64* a, int n) {
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
// first entry with key >= k (entries sorted)
__host__ __device__ inline int lower_bound(const u64* a, int n, u64 k) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
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
__device__ bool add_line(Slot& s, const Lay& L, const DP& P, const double* pts, int i1, int i2, bool from_points, unsigned& st) {
    if (i2 - i1 < 2) return false;
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = i1; i <= i2; ++i) {
        const double x = pts[i * 3], y = pts[i * 3 + 1];
        M[0][0] += x * x; M[0][1] += x * y; M[0][2] += x; M[1][1] += y * y; M[1][2] += y; M[2][2] += 1.0;
    }
    M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
    const Vec abc = smallest_eigvec3(M);
    Vec a(0, 0, 0), b(0, 0, 0);
    if (fabs(abc.y) < 0.5) {
        a.y = 0; a.x = -abc.z / abc.x; b.y = 1; b.x = (-abc.z - abc.y) / abc.x;
    } else {
        a.x = 0; b.x = 1; a.y = -abc.z / abc.y; b.y = (-abc.z - abc.x) / abc.y;
    }
    double max_dis = 0;
    for (int i = i1; i <= i2; ++i) { const double d = dis_from_line(ld3(pts + 3 * i), a, b); max_dis = (max_dis < d) ? d : max_dis; }
    const Vec p1 = project_to_line(ld3(pts + 3 * i1), a, b), p2 = project_to_line(ld3(pts + 3 * i2), a, b);
    const double len = vnorm(vsub(p1, p2));
    if (max_dis > P.max_dis) return false;
    if (len < P.min_len) return false;
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
__device__ bool add_segment(Slot& s, const Lay& L, const DP& P, const Vec& p1, const Vec& p2, unsigned& st) {
    const Vec mid = Vec((p2.x + p1.x) / 2, (p2.y + p1.y) / 2, (p2.z + p1.z) / 2);
    const double fake[9] = {p1.x, p1.y, p1.z, mid.x, mid.y, mid.z, p2.x, p2.y, p2.z};
    return add_line(s, L, P, fake, 0, 2, false, st);
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

__device__ inline Iso<double> til(const DP& P) { return liw::cast_iso<double>(P.Til_R, P.Til_t); }
__device__ inline Iso<double> tf6(const double* p6) { return liw::make_tf(ld3(p6), ld3(p6 + 3)); }

// ------------------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(kBlock) k_lfe_reset(void* store, Lay L, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    char* mz = (char*)m;
    for (size_t k = 0; k < kMgrBytes; ++k) mz[k] = 0;
    for (int k = 0; k < L.slots + 2; ++k) { Slot s = slot_at(store, L, b, k); slot_clear(s, 0.0); }
}

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

// laser_manager::do_match (:244-348) for one robot
__global__ void __launch_bounds__(kBlock) k_lfe_match(void* store, Lay L, DP P, int slot1, int slot2, const double* pose1, const double* pose2, int kk,
                                                     int cap, int* count, double* recs, int* idx1, int* idx2, double* match_pose) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const double* p2 = pose2 + 6 * (size_t)b;
    double* mp = match_pose + 12 * (size_t)b;
    double p1[6];
    int phys1 = slot1;
    if (slot1 == LIW_LFE_REF) {
        if (!m->has_ref) {   // empty_match(p, q)
            for (int k = 0; k < 6; ++k) { mp[k] = p2[k]; mp[6 + k] = p2[k]; }
            count[b] = 0;
            return;
        }
        const int rs = m->ref_sub & 1;
        phys1 = L.slots + rs;
        for (int k = 0; k < 3; ++k) { p1[k] = m->sub_p[rs][k]; p1[3 + k] = m->sub_q[rs][k]; }
    } else {
        for (int k = 0; k < 6; ++k) p1[k] = pose1[6 * (size_t)b + k];
    }
    for (int k = 0; k < 6; ++k) { mp[k] = p1[k]; mp[6 + k] = p2[k]; }
    count[b] = 0;
    const Slot s1 = slot_at(store, L, b, phys1), s2 = slot_at(store, L, b, slot2);
    if (s1.h->status || s2.h->status) { m->status |= LIW_LFE_ST_INVALID; return; }
    const Iso<double> Ti = til(P);
    const Iso<double> T12 = liw::mul(liw::inverse(liw::mul(tf6(p1), Ti)), liw::mul(tf6(p2), Ti));
    const int n2 = n_lines(s2, L), ne = n_entries(s1, L), n1 = n_lines(s1, L);
    const int a = 1 + kk;
    // -> best line of s1 for line i of s2 and the pair's distance; false when the host skips the line
    auto pair = [&](int i, int& best, double& d) -> bool {
        const double* l2 = s2.lines + 10 * (size_t)i;
        const Vec l2p1 = ld3(l2), l2p2 = ld3(l2 + 3);
        const Vec mid((l2p1.x + l2p2.x) / 2, (l2p1.y + l2p2.y) / 2, (l2p1.z + l2p2.z) / 2);
        const Vec tm = apply(T12, mid);
        int c, r;
        xy_to_index(P, tm.x, tm.y, c, r);
        best = -1;
        bool any = false;
        double best_angle = kPi * 2;
        const Vec v2 = vsub(apply(T12, l2p2), apply(T12, l2p1));
        for (int dr = -a; dr <= a; ++dr)
            for (int dc = -a; dc <= a; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if (!valid(P, rr, cc)) continue;
                const u64 key = (u64)(unsigned)(rr * P.w + cc);
                for (int j = lower_bound(s1.ent, ne, key << 32); j < ne && (s1.ent[j] >> 32) == key; ++j) {
                    const unsigned id = (unsigned)(s1.ent[j] & 0xffffffffull);
                    if (id >= (unsigned)n1) continue;   // only a store that was never reset holds such an entry
                    any = true;
                    const double* l1 = s1.lines + 10 * (size_t)id;
                    const double angle = acos(fabs(vdot(vunit_div(vsub(ld3(l1 + 3), ld3(l1))), vunit_div(v2))));
                    if (angle < best_angle) { best = (int)id; best_angle = angle; }
                }
            }
        if (!any) return false;
        if (best_angle / kPi * 180 > 10) return false;
        const double* l1 = s1.lines + 10 * (size_t)best;
        const Vec a1 = ld3(l1), a2 = ld3(l1 + 3);
        d = 0.5 * (dis_from_line(apply(T12, l2p1), a1, a2) + dis_from_line(apply(T12, l2p2), a1, a2));
        return true;
    };
    double aver = 0;
    int nm = 0;
    for (int i = 0; i < n2; ++i) {
        int best; double d;
        if (pair(i, best, d)) { aver += d; ++nm; }
    }
    aver /= (double)nm;
    int n = 0;
    for (int i = 0; i < n2; ++i) {
        int best; double d;
        if (!pair(i, best, d)) continue;
        if (!(d < aver * 1.2)) continue;
        if (n >= cap) { m->status |= LIW_LFE_ST_MATCH; count[b] = 0; return; }
        const double* l1 = s1.lines + 10 * (size_t)best;
        const double* l2 = s2.lines + 10 * (size_t)i;
        double* o = recs + ((size_t)b * cap + n) * 12;
        for (int k = 0; k < 6; ++k) { o[k] = l1[k]; o[6 + k] = l2[k]; }
        if (idx1) idx1[(size_t)b * cap + n] = best;
        if (idx2) idx2[(size_t)b * cap + n] = i;
        ++n;
    }
    count[b] = n;
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
__global__ void __launch_bounds__(kBlock) k_lfe_add_scan(void* store, Lay L, DP P, int src_slot, const double* pose, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const Slot src = slot_at(store, L, b, src_slot);
    // an invalid source scan invalidates every sub-map this call writes (until that sub-map is replaced)
    const unsigned src_st = src.h->status ? ((unsigned)src.h->status | LIW_LFE_ST_INVALID) : 0u;
    m->status |= src_st;
    const double* pq = pose + 6 * (size_t)b;
    const Iso<double> cur = tf6(pq);
    if (m->has_ref) {
        const Iso<double> last = liw::cast_iso<double>(m->last_R, m->last_t);
        const Iso<double> d = liw::mul(liw::inverse(last), cur);
        const Vec dq = liw::log_SO3(d.R);
        if (vnorm(d.t) < P.mf_p && vnorm(dq) < P.mf_q) return;
    } else {
        fresh_submap(store, L, P, b, m, m->ref_sub & 1, src, src_st, pq);
        m->has_ref = 1;
        set_last(m, cur);
        m->count = 1;
        return;
    }
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
    }
    if (m->count == P.n_acc) {   // ref = spawning (which may not exist: the /2 quirk of ref_n_accumulation 2); spawning = fresh
        const int nr = 1 - rs;
        m->has_ref = m->has_spawn;
        m->ref_sub = nr;
        fresh_submap(store, L, P, b, m, 1 - nr, src, src_st, pq);
        m->has_spawn = 1;
        m->count = P.n_acc / 2;
    }
    set_last(m, cur);
}

// laser_off = exclusive scan of count (one block of 1024; counts clamped to [0, cap])
__global__ void __launch_bounds__(1024) k_lfe_scan(int B, int cap, const int* count, int* off) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = lo + per < B ? lo + per : B;
    long long s = 0;
    for (int b = lo; b < hi; ++b) { const int c = count[b]; s += c < 0 ? 0 : (c > cap ? cap : c); }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - s;
    for (int b = lo; b < hi; ++b) {
        off[b] = (int)run;
        const int c = count[b];
        run += c < 0 ? 0 : (c > cap ? cap : c);
    }
    if (t == 1023) off[B] = (int)part[1023];
}

__global__ void __launch_bounds__(256) k_lfe_pack(int B, int n, int frame, int cap, int Ltot, const int* off, const double* recs, const double* match_pose,
                                                 int* laser_frame, double* laser_pts, double* mp_out, unsigned char* has_match) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)B * cap) return;
    const int b = (int)(g / cap), j = (int)(g % cap);
    if (j == 0) {
        for (int k = 0; k < 12; ++k) mp_out[((size_t)b * n + frame) * 12 + k] = match_pose[12 * (size_t)b + k];
        has_match[(size_t)b * n + frame] = 1;
    }
    const int o0 = off[b], cnt = off[b + 1] - o0;
    if (j >= cnt) return;
    const int o = o0 + j;
    laser_frame[o] = frame;
    const double* r = recs + g * 12;
    for (int k = 0; k < 12; ++k) laser_pts[(size_t)k * Ltot + o] = r[k];
}

}  // namespace lfe

using namespace lfe;

struct liw_lfe_ctx {
    liw_laser_params prm;
    Lay L;
    DP P;
    int device = 0;
    bool have_device = false;
    std::string err;
    float2* d_cs = nullptr;
    int n_rays = 0;
    float tinc = 0.0f;
};

namespace {
int fail(liw_lfe_ctx* c, int code, const char* what) {
    if (c) c->err = what;
    return code;
}
#define LFE_DEV(c)                                                                                                   \
    do {                                                                                                             \
        if (!(c)) return LIW_EINVAL;                                                                                 \
        if (!(c)->have_device) return fail((c), LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");             \
        (void)hipSetDevice((c)->device);                                                                             \
    } while (0)
int launched(liw_lfe_ctx* c) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LIW_OK : fail(c, LIW_EHIP, hipGetErrorString(e));
}
inline int blocks(size_t n, int bs) { return (int)((n + bs - 1) / bs); }
// host copy of a slot: header + lines + entries of robot / selector (-1 when a sub-map does not exist)
int host_slot(liw_lfe_ctx* c, const void* store, int robot, int slot, SlotHdr& h, int& phys) {
    if (!c || !store || robot < 0 || robot >= c->L.B || slot < LIW_LFE_SPAWNING || slot >= c->L.slots) return LIW_EINVAL;
    if (!c->have_device) return fail(c, LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");
    (void)hipSetDevice(c->device);
    const char* rp = (const char*)store + (size_t)robot * c->L.robot_bytes;
    phys = slot;
    if (slot < 0) {
        Mgr m;
        if (hipMemcpy(&m, rp, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
        const bool has = slot == LIW_LFE_REF ? m.has_ref : m.has_spawn;
        if (!has) return 1;
        phys = c->L.slots + (slot == LIW_LFE_REF ? (m.ref_sub & 1) : 1 - (m.ref_sub & 1));
    }
    if (hipMemcpy(&h, rp + slot_off(c->L, phys), sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    return 0;
}
}  // namespace

extern "C" {

int liw_lfe_store_layout(const liw_lfe_dims* dims, size_t* bytes) {
    Lay L;
    if (!bytes || !make_lay(dims, L)) return LIW_EINVAL;
    *bytes = (size_t)dims->B * L.robot_bytes;
    return LIW_OK;
}

liw_lfe_ctx* liw_lfe_create(const liw_laser_params* prm, const liw_lfe_dims* dims, int device) {
    Lay L;
    if (!prm || !make_lay(dims, L) || !(prm->laser_resolution > 0)) return nullptr;
    liw_lfe_ctx* c = new liw_lfe_ctx();
    c->prm = *prm;
    c->L = L;
    c->device = device;
    DP& P = c->P;
    P.res = prm->laser_resolution; P.cont_thr = prm->line_continuous_threshold; P.min_len = prm->line_min_len; P.max_dis = prm->line_max_dis;
    P.tol = prm->line_max_tolerance_angle / 180.0 * kPi;   // deg2rad as liw_laser.cpp
    P.mf_p = prm->ref_motion_filter_p; P.mf_q = prm->ref_motion_filter_q; P.n_acc = prm->ref_n_accumulation;
    P.w = (int)(prm->w_laser_each_scan / prm->laser_resolution + 1);   // laser_manager ctor (:229-241)
    P.h = (int)(prm->h_laser_each_scan / prm->laser_resolution + 1);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.Til_R[i * 3 + j] = prm->T_imu_to_laser[i * 4 + j]; P.Til_t[i] = prm->T_imu_to_laser[i * 4 + 3]; }
    if (prm->normalize_extrinsics) liw_normalize_rotation_host(P.Til_R);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev) {
        hipDeviceProp_t props;
        if (hipGetDeviceProperties(&props, device) == hipSuccess) {
            if (std::strstr(props.gcnArchName, "gfx950") != nullptr) c->have_device = true;
            else c->err = std::string("device is ") + props.gcnArchName + ", this library is built for gfx950 only";
        }
    }
    (void)hipGetLastError();
    if (!c->have_device && c->err.empty()) c->err = "no HIP device";
    return c;
}

void liw_lfe_destroy(liw_lfe_ctx* c) {
    if (!c) return;
    if (c->d_cs) { (void)hipSetDevice(c->device); (void)hipFree(c->d_cs); }
    delete c;
}

const char* liw_lfe_last_error(liw_lfe_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_lfe_set_geometry(liw_lfe_ctx* c, int n_rays, float angle_min, float angle_increment, float time_increment) {
    LFE_DEV(c);
    if (n_rays <= 0 || !(angle_increment > 0)) return fail(c, LIW_EINVAL, "liw_lfe_set_geometry: n_rays > 0 and angle_increment > 0");
    // exactly the float arithmetic of liw_laser_to_points (common.cpp:22-24): float angle, cosf / sinf of the host libm
    std::vector<float2> cs(n_rays);
    for (int i = 0; i < n_rays; ++i) {
        const volatile float prod = (float)(size_t)i * angle_increment;
        const float ang = angle_min + prod;
        cs[i].x = std::cos(ang);
        cs[i].y = std::sin(ang);
    }
    if (c->d_cs) { (void)hipFree(c->d_cs); c->d_cs = nullptr; }
    if (hipMalloc(&c->d_cs, sizeof(float2) * n_rays) != hipSuccess) return fail(c, LIW_ENOMEM, "hipMalloc");
    if (hipMemcpy(c->d_cs, cs.data(), sizeof(float2) * n_rays, hipMemcpyHostToDevice) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    c->n_rays = n_rays;
    c->tinc = time_increment;
    return LIW_OK;
}

int liw_lfe_store_reset(liw_lfe_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LFE_DEV(c);
    if (!store) return fail(c, LIW_EINVAL, "liw_lfe_store_reset: store");
    hipLaunchKernelGGL(k_lfe_reset, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, mask);
    return launched(c);
}

int liw_lfe_ranges_to_points(liw_lfe_ctx* c, void* store, const float* ranges, const double* stamps, double* pts, double* times, int* n_pts, void* stream) {
    LFE_DEV(c);
    if (!c->d_cs) return fail(c, LIW_ESTATE, "liw_lfe_ranges_to_points: no geometry (liw_lfe_set_geometry)");
    if (!ranges || !stamps || !pts || !times || !n_pts) return fail(c, LIW_EINVAL, "liw_lfe_ranges_to_points: null array");
    hipLaunchKernelGGL(k_lfe_ranges, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, ranges, c->n_rays,
                       (const float2*)c->d_cs, c->tinc, stamps, pts, times, n_pts);
    return launched(c);
}

int liw_lfe_deskew(liw_lfe_ctx* c, double* pts, const double* times, const int* n_pts, const double* stamps, const double* linear, const double* angular,
                   void* stream) {
    LFE_DEV(c);
    if (!pts || !times || !n_pts || !stamps || !linear || !angular) return fail(c, LIW_EINVAL, "liw_lfe_deskew: null array");
    hipLaunchKernelGGL(k_lfe_deskew, dim3(blocks((size_t)c->L.B * c->L.max_points, 256)), dim3(256), 0, (hipStream_t)stream, c->L, pts, times, n_pts,
                       stamps, linear, angular);
    return launched(c);
}

int liw_lfe_spawn(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, void* stream) {
    LFE_DEV(c);
    if (!store || !pts || !n_pts || slot < 0 || slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_spawn: bad argument");
    hipLaunchKernelGGL(k_lfe_spawn, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, slot, pts, n_pts, times);
    return launched(c);
}

int liw_lfe_match(liw_lfe_ctx* c, void* store, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap, int* count, double* recs,
                  int* idx1, int* idx2, double* match_pose, void* stream) {
    LFE_DEV(c);
    if (!store || !pose2 || !count || !recs || !match_pose || cap < 1 || kk < 0 || slot2 < 0 || slot2 >= c->L.slots ||
        !(slot1 == LIW_LFE_REF || (slot1 >= 0 && slot1 < c->L.slots)) || (slot1 != LIW_LFE_REF && !pose1))
        return fail(c, LIW_EINVAL, "liw_lfe_match: bad argument");
    hipLaunchKernelGGL(k_lfe_match, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, slot1, slot2, pose1, pose2, kk,
                       cap, count, recs, idx1, idx2, match_pose);
    return launched(c);
}

int liw_lfe_add_scan(liw_lfe_ctx* c, void* store, int src_slot, const double* pose, const unsigned char* mask, void* stream) {
    LFE_DEV(c);
    if (!store || !pose || src_slot < 0 || src_slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_add_scan: bad argument");
    hipLaunchKernelGGL(k_lfe_add_scan, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, src_slot, pose, mask);
    return launched(c);
}

int liw_lfe_pack_track(liw_lfe_ctx* c, int n, int frame, int cap, const int* count, const double* recs, const double* match_pose, int L_cap,
                       int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match, void* stream) {
    LFE_DEV(c);
    if (n < 1 || frame < 0 || frame >= n || cap < 1 || L_cap < 0 || !count || !recs || !match_pose || !laser_off || !laser_frame || !laser_pts ||
        !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_track: bad argument");
    if ((long long)c->L.B * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_track: B * cap must fit in int32");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfe_scan, dim3(1), dim3(1024), 0, s, c->L.B, cap, count, laser_off);
    if (int r = launched(c)) return r;
    int Ltot = 0;
    if (hipMemcpyAsync(&Ltot, laser_off + c->L.B, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(c, LIW_EHIP, "liw_lfe_pack_track: read-back of Ltot");
    if (Ltot > L_cap) return fail(c, LIW_ENOMEM, "liw_lfe_pack_track: Ltot exceeds L_cap");
    hipLaunchKernelGGL(k_lfe_pack, dim3(blocks((size_t)c->L.B * cap, 256)), dim3(256), 0, s, c->L.B, n, frame, cap, Ltot, laser_off, recs, match_pose,
                       laser_frame, laser_pts, match_pose_out, has_match);
    if (int r = launched(c)) return r;
    return Ltot;
}

int liw_lfe_status(liw_lfe_ctx* c, const void* store, int robot, int slot) {
    if (slot == LIW_LFE_ROBOT) {
        if (!c || !store || robot < 0 || robot >= c->L.B) return LIW_EINVAL;
        if (!c->have_device) return fail(c, LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");
        (void)hipSetDevice(c->device);
        Mgr m;
        if (hipMemcpy(&m, (const char*)store + (size_t)robot * c->L.robot_bytes, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
        return m.status;
    }
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    return r < 0 ? r : (r == 1 ? LIW_LFE_NONE : h.status);
}

int liw_lfe_num_lines(liw_lfe_ctx* c, const void* store, int robot, int slot) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    return r < 0 ? r : (r == 1 ? LIW_LFE_NONE : h.n_lines);
}

int liw_lfe_get_lines(liw_lfe_ctx* c, const void* store, int robot, int slot, double* out, int cap) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    if (r) return r < 0 ? r : 0;
    const int nl = h.n_lines < c->L.max_lines ? h.n_lines : c->L.max_lines;
    const int n = nl < cap ? nl : cap;
    if (n > 0 && out) {
        const char* p = (const char*)store + (size_t)robot * c->L.robot_bytes + slot_off(c->L, phys) + kHdrBytes;
        if (hipMemcpy(out, p, sizeof(double) * 10 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    }
    return n < 0 ? 0 : n;
}

int liw_lfe_cell_lines(liw_lfe_ctx* c, const void* store, int robot, int slot, double x, double y, int* ids, int cap) {
    SlotHdr h;
    int phys;
    const int r = host_slot(c, store, robot, slot, h, phys);
    if (r) return r < 0 ? r : LIW_LFE_NONE;
    int cc, rr;
    xy_to_index(c->P, x, y, cc, rr);
    if (!valid(c->P, rr, cc)) return LIW_LFE_NONE;
    const int ne = h.n_entries < 0 ? 0 : (h.n_entries < c->L.max_entries ? h.n_entries : c->L.max_entries);
    std::vector<u64> ent((size_t)ne + 1);
    const char* p = (const char*)store + (size_t)robot * c->L.robot_bytes + slot_off(c->L, phys) + kHdrBytes + 80 * (size_t)c->L.max_lines;
    if (ne > 0 && hipMemcpy(ent.data(), p, sizeof(u64) * ne, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    const u64 key = (u64)(unsigned)(rr * c->P.w + cc);
    int k = 0;
    for (int j = lower_bound(ent.data(), ne, key << 32); j < ne && (ent[j] >> 32) == key; ++j, ++k)
        if (ids && k < cap) ids[k] = (int)(unsigned)(ent[j] & 0xffffffffull);
    return k;
}

int liw_lfe_submap_pose(liw_lfe_ctx* c, const void* store, int robot, int slot, double* p3, double* q3) {
    if (!c || !store || robot < 0 || robot >= c->L.B || !(slot == LIW_LFE_REF || slot == LIW_LFE_SPAWNING)) return LIW_EINVAL;
    if (!c->have_device) return fail(c, LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");
    (void)hipSetDevice(c->device);
    Mgr m;
    if (hipMemcpy(&m, (const char*)store + (size_t)robot * c->L.robot_bytes, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    if (!(slot == LIW_LFE_REF ? m.has_ref : m.has_spawn)) return LIW_LFE_NONE;
    const int sub = slot == LIW_LFE_REF ? (m.ref_sub & 1) : 1 - (m.ref_sub & 1);
    for (int k = 0; k < 3; ++k) {
        if (p3) p3[k] = m.sub_p[sub][k];
        if (q3) q3[k] = m.sub_q[sub][k];
    }
    return 0;
}

}  // extern "C"
