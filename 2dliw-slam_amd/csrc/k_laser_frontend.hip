// k_laser_frontend.hip — the batched laser front-end on the MI355X (C ABI include/liw_laser_batch.h): liw_laser.cpp's
// tracking-time work for B robots at once, its output landing in the device arrays liw_batch takes.
//
// Mapping: one lane per (robot, scan), except spawn, the INIT window's match and add_scan / rebuild.  Every step of the host front-end is a serial chain over one scan (the 1 cm
// filter compares against the previously KEPT point, the segment merge carries `last`, a line's cells are de-duplicated against
// its earlier cells, the mean match distance is summed in match order), so a lane walks its scan in the host's order and rounds
// as the host does; the batch is the parallelism.
//   k_lfe_ranges   ranges -> points (+ times): the (cosf, sinf) table of the geometry comes from the host libm (ctx)
//   k_lfe_deskew   one lane per point: make_tf(dt * twist) * p
//   k_lfe_spawn_wave  spawn_scan, one wavefront per scan, points and intermediates in LDS (layout at wave_lds): runs, corner
//                  response and the maxima's window test a lane per point; the skip after a maximum one lane over the maxima
//                  bits; the merge 64 tests at a time from the standing `last`; add_line a lane per candidate segment for the
//                  sums the host makes in index order (moment matrix, cyclic Jacobi, create_line), a lane per point for max_dis
//                  and the cells; ids by ballot prefix; the (cell, line) entries through a hash set in the dead point array,
//                  compacted and bitonic-sorted in LDS; scan::concers from the sorted entries.  Same store bytes as k_lfe_spawn
//                  for every valid slot (tests/test_gpu_laser_spawn_wave.py); an overflowed slot is left empty and invalid.
//                  105 VGPRs, no scratch, 39 840 B of LDS at 1 080 points / 256 lines: four work-groups per CU (one wave per
//                  SIMD; the fp64 points alone are 25.9 KB, so LDS, not registers, sets the occupancy).
//   k_lfe_spawn    the lane-per-scan spawn (continuous runs -> corner response -> strict local maxima -> merge -> add_line ->
//                  cell entries, heap-sorted): the checker behind LIW_LFE_SPAWN=lane, and the path of dimensions whose LDS
//                  need exceeds a work-group's 64 KiB.  No corners.
//   k_lfe_corners_world  the corners of a tracked scan into the world frame, appended per robot
//   k_lfe_match    per line of s2 in scan::lines order: candidates of the (2kk+3)^2 cells by binary search of the sorted
//                  entries (dr, dc, push order), strict-< argmin of the angle, 10 degree gate; two passes (mean, then keep)
//   k_lfe_match_wave  match_with_front of a whole INIT window, one wavefront per (robot, frame): lanes over the frame's lines, each
//                  line's search once (best, d in LDS); the mean in line order, the pairs by ballot prefix on a running base:
//                  bit-identical to k_lfe_match (tests/test_gpu_laser_init.py)
//   k_lfe_add_scan_wave  laser_manager::add_scan (motion filter, fresh sub-maps, add_segment rasterisation, the swap) and the whole
//                  liw_lfe_rebuild, one wavefront per robot: the manager's branch wave-uniform, a lane per source line for the fit
//                  and the 0.05 m walk, ids and entry positions by prefix counts, the call's new entries sorted in LDS and merged
//                  into the sorted sub-map in place (design and proof of the de-duplication at the kernel).  Same manager record,
//                  sub-map headers, lines[0 .. n_lines) and ent[0 .. n_entries) as k_lfe_add_scan
//                  (tests/test_gpu_laser_add_scan_wave.py); a target beyond the LDS buffer or the slot's capacity is built by
//                  one lane with the lane kernel's code.  236 VGPRs, no scratch, 26 624 B of LDS at 256 lines: two waves per
//                  SIMD by registers, six work-groups per CU by LDS.
//   k_lfe_add_scan the lane-per-robot add_scan: the checker behind LIW_LFE_ADD_SCAN=lane, and the path of dimensions whose LDS
//                  need exceeds a work-group's 64 KiB.  Both kernels write the LIW_LFE_ADD_* flags.
//   k_lfe_reset_mgr   clear_all_scan that keeps the scan slots (the lane path of liw_lfe_rebuild = this + add_scan per frame)
//   k_lfe_track_init / _begin / _end   the glue of a tracking frame on a 256-byte record per robot (last_keyframe_tf,
//                  current_angular_local, stamp, counters): the de-skew twist, the min_delta_t gate, the window roll and the pose
//                  prediction from the wheel increment before the scan; the key-frame decision after the solve.  A lane per robot,
//                  work-groups of 256, no LDS, no atomics, no scratch; _begin evaluates its sin / cos / atan2
//                  correctly rounded (liw_crmath.hpp)
//   k_lfe_init_reset / _begin / _select / _commit   the per-robot INITIALIZING state machine on a 256-byte record per robot (current
//                  state, status, n_frames, counters): the is_static gate and the pose prediction, correctly rounded as in
//                  _track_begin, with the frame's state and interval rows written into the robot's window (a lane per robot
//                  decides, then k_lfe_init_rows copies the rows a wavefront per robot); the ascending list of robots whose window is full, by prefix
//                  counts in one block; take_back_state / init_current_status after the INIT solve.  No atomics, no scratch
//   k_lfe_slot_copy   scan slot 0 -> a slot per robot, a work-group per robot, 16-byte words (header, lines, entries)
//   k_lfe_scan_init_sel / k_lfe_pack_init_sel   k_lfe_scan_init / k_lfe_pack_init for a list of robots (one body each)
//   k_lfe_crmath   liw_crmath.hpp's sin / cos / atan2 element by element (liw_lfe_crmath_eval: a diagnostic entry for the tests)
//   k_lfe_scan / k_lfe_pack   laser_off exclusive scan (one block), then the component-major laser arrays
//   k_lfe_scan_init / k_lfe_pack_init   the same for INIT windows: blocks of frames 1 .. n-1, a work-group per window
// The line_map of a slot is a list of 64-bit entries (cell key << 32 | line index) kept sorted: within a cell the host
// pushes line ids in increasing order (ids only grow and a cell never takes the same id twice in a row), so sorting by
// (cell, line index) reproduces the host's push order exactly.
// No floating-point atomics on sums (the one LDS atomic is a maximum of non-negative doubles, and the hash set's content does
// not depend on the insertion order): runs are bitwise reproducible.
#pragma clang fp contract(off)   // the x86-64 host build of liw_laser.cpp does not contract; hipcc contracts device code by default

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_laser_batch.h"
#include "liw_dual.hpp"
#include "liw_crmath.hpp"
#include "liw_host_common.hpp"

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
__device__ bool add_line(Slot& s, const Lay& L, const DP& P, const double* pts, int i1, int i2, bool from_points, unsigned& st) {
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

// clear_all_scan's effect on the manager alone: state, status word and both sub-maps; the scan slots stay (liw_lfe_rebuild)
__global__ void __launch_bounds__(kBlock) k_lfe_reset_mgr(void* store, Lay L, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    char* mz = robot_ptr(store, L, b);
    for (size_t k = 0; k < kMgrBytes; ++k) mz[k] = 0;
    for (int k = L.slots; k < L.slots + 2; ++k) { Slot s = slot_at(store, L, b, k); slot_clear(s, 0.0); }
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

// ------------------------------------------------------------------------------------------ wave-per-scan spawn (+ corners)
// One work-group of one wave per (robot, scan); everything a step reads more than once lives in LDS (offsets in bytes):
//   X     [max_points][3] doubles   the scan's points; after the last add_line the same bytes are the hash set / sort buffer of the entries
//   brk   bit i: a continuous run starts at point i          mx   bit i: point i is a strict local maximum of the response
//   misc  counters, then per candidate of a chunk max_dis (bit pattern of a non-negative double, LDS atomic max) and `has a cell`
//   lbase / lcnt [max_lines]       where line id keeps its cells in `cell`, and how many
//   U     resp [max_points] doubles, until the maxima are known; afterwards
//         cell [max_points * 3 / 2 + 2] (first the `ends` lists of the runs; then a candidate i1 .. i2 with index j owns
//         cell[i1 + j ..]: ranges of consecutive candidates share at most one point) and cand [max_points / 2 + 1] (i1, i2) of
//         the candidate segments with i2 - i1 >= 2
struct WaveLds { unsigned x, brk, mx, misc, lbase, lcnt, u, cand; int tcap; size_t total; };
__host__ __device__ inline size_t up8(size_t x) { return (x + 7) / 8 * 8; }
inline WaveLds wave_lds(const Lay& L) {
    const size_t MP = (size_t)L.max_points, W = (MP + 63) / 64, ML = (size_t)L.max_lines;
    WaveLds O;
    size_t o = 0;
    O.x = (unsigned)o; o += 24 * MP;
    O.brk = (unsigned)o; o += 8 * W;
    O.mx = (unsigned)o; o += 8 * W;
    O.misc = (unsigned)o; o += 16 + 12 * kBlock;
    O.lbase = (unsigned)o; o += up8(4 * ML);
    O.lcnt = (unsigned)o; o += up8(4 * ML);
    O.u = (unsigned)o;
    const size_t cells = up8(4 * (MP + MP / 2 + 2)), cands = 8 * (MP / 2 + 1);
    O.cand = (unsigned)(o + cells);
    const size_t u = cells + cands > 8 * MP ? cells + cands : 8 * MP;
    O.total = o + u;
    O.tcap = 1;   // slots of the hash set in X's bytes: the largest power of two <= 3 * max_points, more than the 1.5 * max_points
    while ((size_t)O.tcap * 2 <= 3 * MP) O.tcap *= 2;   // (cell, line) pairs the candidates' points can make
    return O;
}
constexpr size_t kWaveLdsMax = 64 * 1024;   // a work-group's limit (two of them still share a CU); larger dimensions go to the lane kernel

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
// exclusive prefix sum over the wave (all 64 lanes must call it)
__device__ inline int wave_excl(int v, int lane, int& total) {
    int x = v;
#pragma unroll
    for (int d = 1; d < kBlock; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
    total = __shfl(x, kBlock - 1);
    return x - v;
}
// ascending sort of n unique keys by one wave: bitonic network whose exchanges all put the smaller key at the lower index, so
// the keys behind n behave as +inf without being stored
__device__ void wave_sort(u64* a, int n, int lane) {
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

// laser_manager::match_with_front for a whole INIT window: one wavefront per (robot, frame) task, task (b, k) =
// k_lfe_match(front_slot, first_slot + k) with frame k's pose at poses + b * rs + k * fs.  Lanes stride over the lines of the
// frame's scan; a lane does for its line exactly the arithmetic of k_lfe_match's `pair`, once (best and d stay in LDS:
// 12 bytes per line of max_lines).  Two steps stay ordered so that the result equals the lane kernel's bit for bit: the mean
// distance is summed in increasing line order (every lane walks the d values in LDS, so no broadcast is needed), and the kept
// pairs are written in increasing line order by a ballot / prefix count per 64-line chunk on a running base, to which the cap
// test applies.  Outputs are indexed by task: count [B][F], recs [B][F][cap][12], idx1 / idx2 [B][F][cap], match_pose [B][F][12].
__global__ void __launch_bounds__(kBlock) k_lfe_match_wave(void* store, Lay L, DP P, int front_slot, int first_slot, int F, const double* pose_front,
                                                          const double* poses, long long rs, long long fs, int kk, int cap, int* count, double* recs,
                                                          int* idx1, int* idx2, double* match_pose) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* dL = (double*)lds;
    int* bestL = (int*)(lds + 8 * (size_t)L.max_lines);
    const int lane = threadIdx.x;
    const size_t task = blockIdx.x;
    const int b = (int)(task / (unsigned)F), k = (int)(task % (unsigned)F);
    if (b >= L.B) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const double* p1 = pose_front + 6 * (size_t)b;
    const double* p2 = poses + (long long)b * rs + (long long)k * fs;
    double* mp = match_pose + 12 * task;
    if (lane < 6) { mp[lane] = p1[lane]; mp[6 + lane] = p2[lane]; }
    const Slot s1 = slot_at(store, L, b, front_slot), s2 = slot_at(store, L, b, first_slot + k);
    if (s1.h->status || s2.h->status) {
        if (lane == 0) { atomicOr(&m->status, LIW_LFE_ST_INVALID); count[task] = 0; }
        return;
    }
    const Iso<double> Ti = til(P);
    const Iso<double> T12 = liw::mul(liw::inverse(liw::mul(tf6(p1), Ti)), liw::mul(tf6(p2), Ti));
    const int n2 = n_lines(s2, L), ne = n_entries(s1, L), n1 = n_lines(s1, L);
    const int a = 1 + kk;
    for (int i = lane; i < n2; i += kBlock) {
        const double* l2 = s2.lines + 10 * (size_t)i;
        const Vec l2p1 = ld3(l2), l2p2 = ld3(l2 + 3);
        const Vec mid((l2p1.x + l2p2.x) / 2, (l2p1.y + l2p2.y) / 2, (l2p1.z + l2p2.z) / 2);
        const Vec tm = apply(T12, mid);
        int c, r;
        xy_to_index(P, tm.x, tm.y, c, r);
        int best = -1;
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
                    if (id >= (unsigned)n1) continue;
                    any = true;
                    const double* l1 = s1.lines + 10 * (size_t)id;
                    const double angle = acos(fabs(vdot(vunit_div(vsub(ld3(l1 + 3), ld3(l1))), vunit_div(v2))));
                    if (angle < best_angle) { best = (int)id; best_angle = angle; }
                }
            }
        double d = 0.0;
        if (!any || best_angle / kPi * 180 > 10) {
            best = -1;
        } else {
            const double* l1 = s1.lines + 10 * (size_t)best;
            const Vec a1 = ld3(l1), a2 = ld3(l1 + 3);
            d = 0.5 * (dis_from_line(apply(T12, l2p1), a1, a2) + dis_from_line(apply(T12, l2p2), a1, a2));
        }
        bestL[i] = best;
        dL[i] = d;
    }
    __syncthreads();
    double aver = 0;   // in line order, as the lane kernel sums it
    int nm = 0;
    for (int i = 0; i < n2; ++i)
        if (bestL[i] >= 0) { aver += dL[i]; ++nm; }
    aver /= (double)nm;
    const double thr = aver * 1.2;
    int base = 0;
    for (int c0 = 0; c0 < n2; c0 += kBlock) {
        const int i = c0 + lane;
        const int best = i < n2 ? bestL[i] : -1;
        const bool keep = best >= 0 && dL[i] < thr;
        const u64 mask = __ballot(keep);
        const int n = base + __popcll(mask & ((1ull << lane) - 1));
        if (keep && n < cap) {   // a pair past cap is never written: the match then counts 0
            const double* l1 = s1.lines + 10 * (size_t)best;
            const double* l2 = s2.lines + 10 * (size_t)i;
            double* o = recs + (task * cap + n) * 12;
            for (int q = 0; q < 6; ++q) { o[q] = l1[q]; o[6 + q] = l2[q]; }
            if (idx1) idx1[task * cap + n] = best;
            if (idx2) idx2[task * cap + n] = i;
        }
        base += __popcll(mask);
    }
    if (lane == 0) {
        if (base > cap) { atomicOr(&m->status, LIW_LFE_ST_MATCH); base = 0; }
        count[task] = base;
    }
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
struct AddLds { unsigned nw, pos, lid, loff; int ecap; size_t total; };
constexpr int kAddNewCap = 2048;   // new entries of one target held in LDS (24 KiB with pos); beyond it the serial escape
inline AddLds add_lds(const Lay& L) {
    AddLds O;
    O.ecap = L.max_entries < kAddNewCap ? L.max_entries : kAddNewCap;
    size_t o = 0;
    O.nw = (unsigned)o; o += 8 * (size_t)O.ecap;
    O.pos = (unsigned)o; o += up8(4 * (size_t)O.ecap);
    O.lid = (unsigned)o; o += up8(4 * (size_t)L.max_lines);
    O.loff = (unsigned)o; o += up8(4 * (size_t)L.max_lines);
    O.total = o;
    return O;
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

// laser_off of B INIT windows = exclusive scan over the robots of their F = n - 1 clamped counts (frame 0 has no blocks, so the
// offset of (b, frame 0) is the window's); one block of 1024 as k_lfe_scan.  With `sel` window r is robot sel[r] (count stays
// robot-major): liw_lfe_pack_init_sel
template <bool SEL> __device__ __forceinline__ void scan_init_body(int B, int F, int cap, const int* count, const int* sel, int* off) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = lo + per < B ? lo + per : B;
    auto total = [&](int b) {
        const size_t rb = SEL ? (size_t)sel[b] : (size_t)b;
        long long s = 0;
        for (int k = 0; k < F; ++k) { const int c = count[rb * F + k]; s += c < 0 ? 0 : (c > cap ? cap : c); }
        return s;
    };
    long long s = 0;
    for (int b = lo; b < hi; ++b) s += total(b);
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
        run += total(b);
    }
    if (t == 1023) off[B] = (int)part[1023];
}
__global__ void __launch_bounds__(1024) k_lfe_scan_init(int B, int F, int cap, const int* count, int* off) {
    scan_init_body<false>(B, F, cap, count, nullptr, off);
}
__global__ void __launch_bounds__(1024) k_lfe_scan_init_sel(int R, int F, int cap, const int* count, const int* sel, int* off) {
    scan_init_body<true>(R, F, cap, count, sel, off);
}

// one work-group per window: the frames' offsets inside the window in LDS (fo [n + 1], frame 0 empty), then a thread per block of
// the window, ascending by owning frame; match_pose / has_match rows of all n frames and init_ok.  With `sel` window b of the output
// is robot sel[b] of the inputs, and the front pose is read at pose_front + robot * front_stride (liw_lfe_pack_init_sel)
template <bool SEL> __device__ __forceinline__ void pack_init_body(int B, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                                   const double* match_pose, const double* pose_front, long long front_stride,
                                                                   const int* sel, int* laser_frame, double* laser_pts, double* mp_out,
                                                                   unsigned char* has_match, unsigned char* init_ok) {
    extern __shared__ __align__(16) unsigned char lds[];
    int* fo = (int*)lds;
    const int b = blockIdx.x, t = threadIdx.x, F = n - 1;
    if (b >= B) return;
    const size_t rb = SEL ? (size_t)sel[b] : (size_t)b;
    const int* cnt = count + rb * F;
    const double* pf = SEL ? pose_front + (long long)rb * front_stride : pose_front + 6 * rb;
    if (t == 0) {
        int run = 0, ok = 1;
        fo[0] = 0;
        for (int f = 1; f <= F; ++f) {
            fo[f] = run;
            const int c = cnt[f - 1];
            if (c < 2) ok = 0;
            run += c < 0 ? 0 : (c > cap ? cap : c);
        }
        fo[n] = run;
        if (init_ok) init_ok[b] = (unsigned char)ok;
    }
    for (int e = t; e < n * 12; e += 256) {
        const int f = e / 12, q = e % 12;
        mp_out[(size_t)b * n * 12 + e] = f == 0 ? pf[q % 6] : match_pose[(rb * F + f - 1) * 12 + q];
    }
    for (int f = t; f < n; f += 256) has_match[(size_t)b * n + f] = 1;
    __syncthreads();
    const int o0 = off[b], tot = fo[n];
    for (int j = t; j < tot; j += 256) {
        int lo = 1, hi = F;   // the last frame f in 1 .. F with fo[f] <= j
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (fo[mid] <= j) lo = mid; else hi = mid - 1; }
        const int f = lo, o = o0 + j;
        laser_frame[o] = f;
        const double* r = recs + ((rb * F + f - 1) * cap + (j - fo[f])) * 12;
        for (int q = 0; q < 12; ++q) laser_pts[(size_t)q * Ltot + o] = r[q];
    }
}
__global__ void __launch_bounds__(256) k_lfe_pack_init(int B, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                      const double* match_pose, const double* pose_front, int* laser_frame, double* laser_pts,
                                                      double* mp_out, unsigned char* has_match, unsigned char* init_ok) {
    pack_init_body<false>(B, n, cap, Ltot, off, count, recs, match_pose, pose_front, 6, nullptr, laser_frame, laser_pts, mp_out, has_match, init_ok);
}
__global__ void __launch_bounds__(256) k_lfe_pack_init_sel(int R, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                          const double* match_pose, const double* pose_front, long long front_stride, const int* sel,
                                                          int* laser_frame, double* laser_pts, double* mp_out, unsigned char* has_match,
                                                          unsigned char* init_ok) {
    pack_init_body<true>(R, n, cap, Ltot, off, count, recs, match_pose, pose_front, front_stride, sel, laser_frame, laser_pts, mp_out, has_match, init_ok);
}

// ------------------------------------------------------------------------------------------------------ tracking glue
// lvio_2d::trajectory::add_sensor_data(laser) around the stages above (trajectory.cpp:140-148, :176-184, :82-92, the key-frame
// decision after do_tracking).  A lane per robot: a few hundred fp64 operations and a handful of strided 8-byte accesses each.
struct Trk {               // tracking record of one robot (256 bytes, caller-owned, apart from the store)
    double kf_R[9], kf_t[3];   // last_keyframe_tf
    double ang[3];             // current_angular_local
    double stamp;              // of the last accepted frame
    int tracked, keys, skipped, pad;
};
constexpr size_t kTrkBytes = 256;
static_assert(sizeof(Trk) <= kTrkBytes, "tracking record");
struct TP { double Tiw_R[9], Tiw_t[3], min_dt, p_thr, q_thr; };
__host__ __device__ inline Trk* trk_at(void* track, int b) { return (Trk*)((char*)track + (size_t)b * kTrkBytes); }

__global__ void __launch_bounds__(256) k_lfe_track_init(int B, void* track, const double* x, long long robot_stride, const double* ang,
                                                       const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    const Iso<double> T = tf6(x + (long long)b * robot_stride);
    double* z = (double*)t;
    for (size_t k = 0; k < kTrkBytes / 8; ++k) z[k] = 0.0;
    for (int k = 0; k < 9; ++k) t->kf_R[k] = T.R.m[k];
    t->kf_t[0] = T.t.x; t->kf_t[1] = T.t.y; t->kf_t[2] = T.t.z;
    if (ang) for (int k = 0; k < 3; ++k) t->ang[k] = ang[3 * (size_t)b + k];
}

// A double whose sin / cos / atan2 are the correctly rounded ones of liw_crmath.hpp; + - * / sqrt are the IEEE operations either
// way.  k_lfe_track_begin runs liw_dual.hpp's make_tf / exp_so3 / log_SO3 on it: its twist goes into the de-skew of every point and
// its pose is where the solve starts, and what a last-bit difference against the host's libm there becomes after a few free-running
// solves is measured in docs/WIDENING.md ("Fleet tracking frame").
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

__global__ void __launch_bounds__(256) k_lfe_track_begin(int B, DP P, TP tp, void* track, double* x, const double* imu_X, const double* imu_Dt,
                                                        const double* wheel_T, const double* stamps, const unsigned char* mask, double* linear,
                                                        double* angular, double* pose_new, unsigned char* skip) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    double* x0 = x + 30 * (size_t)b;
    double* x1 = x0 + 15;
    typedef V3<CR> VC;
    const Iso<CR> Twi = liw::make_tf(liw::cast_v3<CR>(x1), liw::cast_v3<CR>(x1 + 3)), Til = liw::cast_iso<CR>(P.Til_R, P.Til_t);
    // de-skew with the current body twist (:140-148): R_w_laser^T v and log_SO3(R_il^T exp_so3(current_angular_local) R_il)
    const VC lin = liw::mulT(liw::mul(Twi, Til).R, liw::cast_v3<CR>(x1 + 6));
    const VC ang = liw::log_SO3(liw::mul(liw::mul(liw::transpose(Til.R), liw::exp_so3(liw::cast_v3<CR>(t->ang))), Til.R));
    linear[3 * (size_t)b] = lin.x.v; linear[3 * (size_t)b + 1] = lin.y.v; linear[3 * (size_t)b + 2] = lin.z.v;
    angular[3 * (size_t)b] = ang.x.v; angular[3 * (size_t)b + 1] = ang.y.v; angular[3 * (size_t)b + 2] = ang.z.v;
    const double Dt = imu_Dt[b];
    const bool sk = Dt < tp.min_dt;
    skip[b] = sk ? 1 : 0;
    if (sk) { t->skipped += 1; return; }
    for (int k = 0; k < 15; ++k) x0[k] = x1[k];   // pop_frame_for_tracking: the newest frame becomes the window's front
    // update_current_status with wheel_delta_to_imu_delta: T_w_i * (T_iw * dT * T_iw^-1)
    const Iso<CR> Tiw = liw::cast_iso<CR>(tp.Tiw_R, tp.Tiw_t);
    const double* w = wheel_T + 12 * (size_t)b;
    const Iso<CR> delta = liw::mul(liw::mul(Tiw, liw::cast_iso<CR>(w, w + 9)), liw::inverse(Tiw));
    const Iso<CR> N = liw::mul(Twi, delta);
    const VC q = liw::log_SO3(N.R);
    x1[0] = N.t.x.v; x1[1] = N.t.y.v; x1[2] = N.t.z.v; x1[3] = q.x.v; x1[4] = q.y.v; x1[5] = q.z.v;
    for (int k = 0; k < 3; ++k) t->ang[k] = imu_X[15 * (size_t)b + 6 + k] / Dt;   // gamma / Dt
    t->stamp = stamps[b];
    for (int k = 0; k < 6; ++k) pose_new[6 * (size_t)b + k] = x1[k];
}

__global__ void __launch_bounds__(256) k_lfe_track_end(const void* store, Lay L, DP P, TP tp, void* track, int slot, const double* x, const int* count,
                                                      const unsigned char* mask, unsigned char* key, double* pose) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B || (mask && !mask[b])) return;
    Trk* t = trk_at(track, b);
    const double* x1 = x + 30 * (size_t)b + 15;
    for (int k = 0; k < 6; ++k) pose[6 * (size_t)b + k] = x1[k];
    const Iso<double> Twl = liw::mul(tf6(x1), til(P));
    const Iso<double> d = liw::mul(liw::inverse(liw::cast_iso<double>(t->kf_R, t->kf_t)), Twl);
    const bool is_static = vnorm(d.t) < tp.p_thr && vnorm(liw::log_SO3(d.R)) < tp.q_thr;
    const Slot s = slot_at(const_cast<void*>(store), L, b, slot);
    const int n_match = count[b], n_no_match = n_lines(s, L) - n_match;
    const bool kf = !is_static || n_match < n_no_match;
    key[b] = kf ? 1 : 0;
    t->tracked += 1;
    if (kf) {
        t->keys += 1;
        for (int k = 0; k < 9; ++k) t->kf_R[k] = Twl.R.m[k];
        t->kf_t[0] = Twl.t.x; t->kf_t[1] = Twl.t.y; t->kf_t[2] = Twl.t.z;
    }
}

// ---------------------------------------------------------------------------------------------------- initialisation glue
// lvio_2d::trajectory::add_sensor_data(laser) while status == INITIALIZING (trajectory.cpp: the is_static gate, update_current_status,
// the frame pushed into the window) and the bookkeeping of check_and_processing_initialize around the INIT solve.
struct Ini {               // initialisation record of one robot (256 bytes, caller-owned, apart from the store and the tracking record)
    double p[3], q[3], v[3], bs[6];   // current_p / q / v / bs
    double ang[3];                    // current_angular_local
    int status, n_frames;             // LIW_LFE_INITIALIZING / _TRACKING; frames in the window being filled
    int inits, failed, dropped, pad;  // initialisations, failed windows, dropped frames
};
constexpr size_t kIniBytes = 256;
static_assert(sizeof(Ini) <= kIniBytes, "initialisation record");
struct IP { double Tiw_R[9], Tiw_t[3], p_thr, q_thr; int N; };
__host__ __device__ inline Ini* ini_at(void* init, int b) { return (Ini*)((char*)init + (size_t)b * kIniBytes); }
constexpr int kIvDoubles = 15 + 225 + 225 + 1 + 12 + 9;   // one interval of the liw_batch arrays

// init_current_status: p, q = log_SE3(T_imu_to_wheel^-1), the rest 0, INITIALIZING with an empty window.  The counters are left
// as they are (a failed window restarts with them; liw_lfe_init_reset zeroes the whole record first)
__device__ inline void ini_restart(Ini* r, const IP& ip) {
    const Iso<CR> inv = liw::inverse(liw::cast_iso<CR>(ip.Tiw_R, ip.Tiw_t));
    const V3<CR> q = liw::log_SO3(inv.R);
    r->p[0] = inv.t.x.v; r->p[1] = inv.t.y.v; r->p[2] = inv.t.z.v;
    r->q[0] = q.x.v; r->q[1] = q.y.v; r->q[2] = q.z.v;
    for (int k = 0; k < 3; ++k) r->v[k] = r->ang[k] = 0.0;
    for (int k = 0; k < 6; ++k) r->bs[k] = 0.0;
    r->status = LIW_LFE_INITIALIZING;
    r->n_frames = 0;
}

__global__ void __launch_bounds__(256) k_lfe_init_reset(int B, IP ip, void* init, const unsigned char* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    Ini* r = ini_at(init, b);
    double* z = (double*)r;
    for (size_t k = 0; k < kIniBytes / 8; ++k) z[k] = 0.0;
    ini_restart(r, ip);
}

// Two launches.  k_lfe_init_begin: a lane per robot decides (gate, prediction, the record, the state row) and leaves in `row` (B
// ints of the ctx, not caller memory) the interval row the robot's arrays go to, -1 for a robot that copies nothing.
// k_lfe_init_rows: a wavefront per robot copies the 487 doubles of an accepted robot, 64 consecutive doubles at a time, so the copy
// runs B waves wide instead of a lane reading and writing 8 bytes at a stride.  No LDS, no atomics.
__global__ void __launch_bounds__(256) k_lfe_init_begin(int B, DP P, IP ip, void* init, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                                                       const unsigned char* mask, double* x_init, unsigned char* drop, int* slot_of, int* rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int row = -1;   // the interval row this robot's arrays go to (k - 1); -1: nothing to copy
    if (!(mask && !mask[b])) {
        Ini* r = ini_at(init, b);
        const int k = r->n_frames;
        if (r->status == LIW_LFE_INITIALIZING && k >= 0 && k < ip.N) {
            typedef V3<CR> VC;
            const Iso<CR> Tiw = liw::cast_iso<CR>(ip.Tiw_R, ip.Tiw_t), Til = liw::cast_iso<CR>(P.Til_R, P.Til_t);
            const double* w = wheel_T + 12 * (size_t)b;
            const Iso<CR> dW = liw::cast_iso<CR>(w, w + 9);
            // wheel_delta_to(T_imu_to_laser, delta): T_lw * delta * T_lw^-1 with T_lw = T_il^-1 * T_iw; is_static on its log_SE3
            const Iso<CR> Tlw = liw::mul(liw::inverse(Til), Tiw);
            const Iso<CR> dL = liw::mul(liw::mul(Tlw, dW), liw::inverse(Tlw));
            const bool st = liw::norm(dL.t).v < ip.p_thr && liw::norm(liw::log_SO3(dL.R)).v < ip.q_thr;
            drop[b] = st ? 1 : 0;
            if (st) {
                r->dropped += 1;
            } else {
                // update_current_status with wheel_delta_to_imu_delta: T_w_i * (T_iw * dT * T_iw^-1)
                const Iso<CR> N = liw::mul(liw::make_tf(liw::cast_v3<CR>(r->p), liw::cast_v3<CR>(r->q)), liw::mul(liw::mul(Tiw, dW), liw::inverse(Tiw)));
                const VC q = liw::log_SO3(N.R);
                r->p[0] = N.t.x.v; r->p[1] = N.t.y.v; r->p[2] = N.t.z.v; r->q[0] = q.x.v; r->q[1] = q.y.v; r->q[2] = q.z.v;
                double* x = x_init + ((size_t)b * ip.N + k) * 15;
                for (int i = 0; i < 3; ++i) { x[i] = r->p[i]; x[3 + i] = r->q[i]; x[6 + i] = r->v[i]; }
                for (int i = 0; i < 6; ++i) x[9 + i] = r->bs[i];
                const double Dt = imu_Dt[b];
                for (int i = 0; i < 3; ++i) r->ang[i] = imu_X[15 * (size_t)b + 6 + i] / Dt;   // gamma / Dt
                slot_of[b] = 1 + k;
                r->n_frames = k + 1;
                row = k - 1;   // frame 0's interval is not stored
            }
        }
    }
    rows[b] = row;
}

__global__ void __launch_bounds__(kBlock) k_lfe_init_rows(int F, const int* rows, const double* imu_X, const double* imu_J, const double* imu_sqrtP,
                                                         const double* imu_Dt, const double* wheel_T, const double* wheel_sqrtP, double* w_imu_X,
                                                         double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt, double* w_wheel_T, double* w_wheel_sqrtP) {
    const size_t src = blockIdx.x;
    const int r = rows[src];
    if (r < 0) return;
    const size_t dst = src * F + r;
    for (int e = threadIdx.x; e < kIvDoubles; e += kBlock) {
        if (e < 15) w_imu_X[dst * 15 + e] = imu_X[src * 15 + e];
        else if (e < 240) w_imu_J[dst * 225 + (e - 15)] = imu_J[src * 225 + (e - 15)];
        else if (e < 465) w_imu_sqrtP[dst * 225 + (e - 240)] = imu_sqrtP[src * 225 + (e - 240)];
        else if (e < 466) w_imu_Dt[dst] = imu_Dt[src];
        else if (e < 478) w_wheel_T[dst * 12 + (e - 466)] = wheel_T[src * 12 + (e - 466)];
        else w_wheel_sqrtP[dst * 9 + (e - 478)] = wheel_sqrtP[src * 9 + (e - 478)];
    }
}

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

// ready[b] = INITIALIZING with a full window; sel = the ready robots in ascending order, n_sel[0] = their number.  One block of 1024 as
// k_lfe_scan: positions are prefix counts, so the list does not depend on the order the lanes run in.
__global__ void __launch_bounds__(1024) k_lfe_init_select(int B, int N, const void* init, unsigned char* ready, int* sel, int* n_sel) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = lo + per < B ? lo + per : B;
    auto is_ready = [&](int b) { const Ini* r = ini_at(const_cast<void*>(init), b); return r->status == LIW_LFE_INITIALIZING && r->n_frames == N; };
    int s = 0;
    for (int b = lo; b < hi; ++b) s += is_ready(b) ? 1 : 0;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = lo; b < hi; ++b) {
        const bool r = is_ready(b);
        ready[b] = r ? 1 : 0;
        if (r) sel[run++] = b;
    }
    if (t == 1023) n_sel[0] = part[1023];
}

// After the INIT solve and the marginalisation, a lane per selected robot b = sel[r].  init_ok[r]: take_back_state (the record's
// p q v bs := the last solved frame), the solved window back into x_init (what liw_lfe_rebuild reads), both rows of the tracking
// window := the last solved frame, the tracking record as k_lfe_track_init makes it (the same make_tf, so a robot committed here and
// one handed to liw_lfe_track_init start from the same bytes) with current_angular_local from the record, TRACKING.  Otherwise
// init_current_status and the failed-window counter.
__global__ void __launch_bounds__(256) k_lfe_init_commit(int R, IP ip, void* init, void* track, const int* sel, const unsigned char* init_ok,
                                                        const double* x_sol, double* x_init, double* x_track) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int b = sel[r], N = ip.N;
    Ini* rec = ini_at(init, b);
    if (!init_ok[r]) {
        ini_restart(rec, ip);
        rec->failed += 1;
        return;
    }
    const double* xs = x_sol + (size_t)r * N * 15;
    double* xi = x_init + (size_t)b * N * 15;
    for (int k = 0; k < N * 15; ++k) xi[k] = xs[k];
    const double* last = xs + (size_t)(N - 1) * 15;
    double* xt = x_track + 30 * (size_t)b;
    for (int k = 0; k < 15; ++k) xt[k] = xt[15 + k] = last[k];
    for (int k = 0; k < 3; ++k) { rec->p[k] = last[k]; rec->q[k] = last[3 + k]; rec->v[k] = last[6 + k]; }
    for (int k = 0; k < 6; ++k) rec->bs[k] = last[9 + k];
    rec->status = LIW_LFE_TRACKING;
    rec->inits += 1;
    Trk* t = trk_at(track, b);
    const Iso<double> T = tf6(last);
    double* z = (double*)t;
    for (size_t k = 0; k < kTrkBytes / 8; ++k) z[k] = 0.0;
    for (int k = 0; k < 9; ++k) t->kf_R[k] = T.R.m[k];
    t->kf_t[0] = T.t.x; t->kf_t[1] = T.t.y; t->kf_t[2] = T.t.z;
    for (int k = 0; k < 3; ++k) t->ang[k] = rec->ang[k];
}

// liw_lfe_crmath_eval: the three functions of liw_crmath.hpp as the CR scalar above calls them, a lane per element (a diagnostic
// entry: tests/test_gpu_crmath.py compares the device compile of the header with a multi-precision reference).  out may alias a:
// a lane reads its element before it writes it.
__global__ void __launch_bounds__(256) k_lfe_crmath(int op, int n, const double* a, const double* b, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    out[i] = op == 0 ? liw_cr::cr_sin(x) : (op == 1 ? liw_cr::cr_cos(x) : liw_cr::cr_atan2(x, b[i]));
}

}  // namespace lfe

using namespace lfe;

struct liw_lfe_ctx : liw_fleet_ctx_base {
    liw_laser_params prm;
    Lay L;
    DP P;
    float2* d_cs = nullptr;
    int* d_rows = nullptr;   // B ints between the two launches of liw_lfe_init_begin
    int n_rays = 0;
    float tinc = 0.0f;
    int add_path = -1;   // the kernel of the last add_scan / rebuild: 0 lane, 1 wave (liw_lfe_add_scan_path)
};

namespace {
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
// liw_lfe_spawn / liw_lfe_spawn_corners: the wave-per-scan kernel unless LIW_LFE_SPAWN=lane (read per call) asks for the
// lane-per-scan kernel, or the dimensions need more LDS than a work-group has (then the lane kernel; it knows no corners)
int spawn_launch(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, int max_corners, double* corners,
                 int* n_corners, void* stream) {
    const char* env = std::getenv("LIW_LFE_SPAWN");
    bool lane = false;
    if (env && *env) {
        if (!std::strcmp(env, "lane")) lane = true;
        else if (std::strcmp(env, "wave")) return fail(c, LIW_EINVAL, "LIW_LFE_SPAWN must be lane or wave");
    }
    const WaveLds O = wave_lds(c->L);
    if (corners && lane) return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: the lane kernel (LIW_LFE_SPAWN=lane) does not compute corners");
    if (corners && O.total > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: max_points / max_lines need more than 64 KiB of LDS");
    if (lane || O.total > kWaveLdsMax)
        hipLaunchKernelGGL(k_lfe_spawn, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, slot, pts, n_pts, times);
    else
        hipLaunchKernelGGL(k_lfe_spawn_wave, dim3(c->L.B), dim3(kBlock), O.total, (hipStream_t)stream, store, c->L, c->P, O, slot, pts, n_pts, times,
                           max_corners, corners, n_corners);
    return launched(c);
}
// liw_lfe_add_scan(_flags) (F = 1, reset = false) and liw_lfe_rebuild: the wave-per-robot kernel in one launch unless
// LIW_LFE_ADD_SCAN=lane (read per call) asks for the lane-per-robot kernel, or the dimensions need more LDS than a work-group has
int add_scan_launch(liw_lfe_ctx* c, void* store, int first_slot, int F, bool reset, const double* poses, long long robot_stride, long long frame_stride,
                    const unsigned char* mask, unsigned char* flags, void* stream) {
    const char* env = std::getenv("LIW_LFE_ADD_SCAN");
    bool lane = false;
    if (env && *env) {
        if (!std::strcmp(env, "lane")) lane = true;
        else if (std::strcmp(env, "wave")) return fail(c, LIW_EINVAL, "LIW_LFE_ADD_SCAN must be lane or wave");
    }
    const AddLds O = add_lds(c->L);
    hipStream_t s = (hipStream_t)stream;
    if (lane || O.total > kWaveLdsMax) {
        c->add_path = 0;
        if (reset) hipLaunchKernelGGL(k_lfe_reset_mgr, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, s, store, c->L, mask);
        for (int k = 0; k < F; ++k)
            hipLaunchKernelGGL(k_lfe_add_scan, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, s, store, c->L, c->P, first_slot + k,
                               poses + (long long)k * frame_stride, robot_stride, mask, flags);
    } else {
        c->add_path = 1;
        hipLaunchKernelGGL(k_lfe_add_scan_wave, dim3(c->L.B), dim3(kBlock), O.total, s, store, c->L, c->P, O, first_slot, F, reset ? 1 : 0, poses,
                           robot_stride, frame_stride, mask, flags);
    }
    return launched(c);
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
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_lfe_destroy(liw_lfe_ctx* c) {
    if (!c) return;
    if (c->d_cs) { (void)hipSetDevice(c->device); (void)hipFree(c->d_cs); }
    if (c->d_rows) { (void)hipSetDevice(c->device); (void)hipFree(c->d_rows); }
    delete c;
}

const char* liw_lfe_last_error(liw_lfe_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_lfe_set_geometry(liw_lfe_ctx* c, int n_rays, float angle_min, float angle_increment, float time_increment) {
    LIW_FLEET_DEV(c);
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
    LIW_FLEET_DEV(c);
    if (!store) return fail(c, LIW_EINVAL, "liw_lfe_store_reset: store");
    hipLaunchKernelGGL(k_lfe_reset, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, mask);
    return launched(c);
}

int liw_lfe_ranges_to_points(liw_lfe_ctx* c, void* store, const float* ranges, const double* stamps, double* pts, double* times, int* n_pts, void* stream) {
    LIW_FLEET_DEV(c);
    if (!c->d_cs) return fail(c, LIW_ESTATE, "liw_lfe_ranges_to_points: no geometry (liw_lfe_set_geometry)");
    if (!ranges || !stamps || !pts || !times || !n_pts) return fail(c, LIW_EINVAL, "liw_lfe_ranges_to_points: null array");
    hipLaunchKernelGGL(k_lfe_ranges, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, ranges, c->n_rays,
                       (const float2*)c->d_cs, c->tinc, stamps, pts, times, n_pts);
    return launched(c);
}

int liw_lfe_deskew(liw_lfe_ctx* c, double* pts, const double* times, const int* n_pts, const double* stamps, const double* linear, const double* angular,
                   void* stream) {
    LIW_FLEET_DEV(c);
    if (!pts || !times || !n_pts || !stamps || !linear || !angular) return fail(c, LIW_EINVAL, "liw_lfe_deskew: null array");
    hipLaunchKernelGGL(k_lfe_deskew, dim3(blocks((size_t)c->L.B * c->L.max_points, 256)), dim3(256), 0, (hipStream_t)stream, c->L, pts, times, n_pts,
                       stamps, linear, angular);
    return launched(c);
}

int liw_lfe_spawn(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pts || !n_pts || slot < 0 || slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_spawn: bad argument");
    return spawn_launch(c, store, slot, pts, n_pts, times, 0, nullptr, nullptr, stream);
}

int liw_lfe_spawn_corners(liw_lfe_ctx* c, void* store, int slot, const double* pts, const int* n_pts, const double* times, int max_corners,
                          double* corners, int* n_corners, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pts || !n_pts || slot < 0 || slot >= c->L.slots || max_corners < 1 || !corners || !n_corners)
        return fail(c, LIW_EINVAL, "liw_lfe_spawn_corners: bad argument");
    return spawn_launch(c, store, slot, pts, n_pts, times, max_corners, corners, n_corners, stream);
}

int liw_lfe_corners_to_world(liw_lfe_ctx* c, void* store, int max_corners, const double* corners, const int* n_corners, const double* pose,
                             const unsigned char* mask, const unsigned char* clear, int acc_cap, double* acc, int* n_acc, void* stream) {
    LIW_FLEET_DEV(c);
    if (max_corners < 1 || !corners || !n_corners || !pose || acc_cap < 1 || !acc || !n_acc) return fail(c, LIW_EINVAL, "liw_lfe_corners_to_world: bad argument");
    hipLaunchKernelGGL(k_lfe_corners_world, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, max_corners, corners,
                       n_corners, pose, mask, clear, acc_cap, acc, n_acc);
    return launched(c);
}

int liw_lfe_match(liw_lfe_ctx* c, void* store, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap, int* count, double* recs,
                  int* idx1, int* idx2, double* match_pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose2 || !count || !recs || !match_pose || cap < 1 || kk < 0 || slot2 < 0 || slot2 >= c->L.slots ||
        !(slot1 == LIW_LFE_REF || (slot1 >= 0 && slot1 < c->L.slots)) || (slot1 != LIW_LFE_REF && !pose1))
        return fail(c, LIW_EINVAL, "liw_lfe_match: bad argument");
    hipLaunchKernelGGL(k_lfe_match, dim3(blocks(c->L.B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, store, c->L, c->P, slot1, slot2, pose1, pose2, kk,
                       cap, count, recs, idx1, idx2, match_pose);
    return launched(c);
}

int liw_lfe_add_scan(liw_lfe_ctx* c, void* store, int src_slot, const double* pose, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose || src_slot < 0 || src_slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_add_scan: bad argument");
    return add_scan_launch(c, store, src_slot, 1, false, pose, 6LL, 0LL, mask, nullptr, stream);
}

int liw_lfe_add_scan_flags(liw_lfe_ctx* c, void* store, int src_slot, const double* pose, const unsigned char* mask, unsigned char* flags, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose || !flags || src_slot < 0 || src_slot >= c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_add_scan_flags: bad argument");
    return add_scan_launch(c, store, src_slot, 1, false, pose, 6LL, 0LL, mask, flags, stream);
}

int liw_lfe_add_scan_path(liw_lfe_ctx* c) {
    if (!c) return LIW_EINVAL;
    if (!c->have_device) return fail(c, LIW_ENODEV, "no usable gfx950 device (no CPU fallback)");
    return c->add_path < 0 ? fail(c, LIW_EINVAL, "liw_lfe_add_scan_path: no add_scan or rebuild yet") : c->add_path;
}

int liw_lfe_pack_track(liw_lfe_ctx* c, int n, int frame, int cap, const int* count, const double* recs, const double* match_pose, int L_cap,
                       int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match, void* stream) {
    LIW_FLEET_DEV(c);
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

int liw_lfe_match_front(liw_lfe_ctx* c, void* store, int front_slot, int first_slot, int F, const double* pose_front, const double* poses,
                        long long robot_stride, long long frame_stride, int kk, int cap, int* count, double* recs, int* idx1, int* idx2,
                        double* match_pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !pose_front || !poses || !count || !recs || !match_pose || cap < 1 || kk < 0 || F < 1 || first_slot < 0 ||
        (long long)first_slot + F > c->L.slots || front_slot < 0 || front_slot >= c->L.slots)
        return fail(c, LIW_EINVAL, "liw_lfe_match_front: bad argument");
    if ((long long)c->L.B * F >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_match_front: B * F must fit in int32");
    const size_t lds = 12 * (size_t)c->L.max_lines;   // best and d per line of the frame's scan
    if (lds > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_match_front: max_lines needs more than 64 KiB of LDS");
    hipLaunchKernelGGL(k_lfe_match_wave, dim3((unsigned)((size_t)c->L.B * F)), dim3(kBlock), lds, (hipStream_t)stream, store, c->L, c->P, front_slot,
                       first_slot, F, pose_front, poses, robot_stride, frame_stride, kk, cap, count, recs, idx1, idx2, match_pose);
    return launched(c);
}

int liw_lfe_pack_init(liw_lfe_ctx* c, int n, int cap, const int* count, const double* recs, const double* match_pose, const double* pose_front,
                      int L_cap, int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match,
                      unsigned char* init_ok, void* stream) {
    LIW_FLEET_DEV(c);
    if (n < 2 || cap < 1 || L_cap < 0 || !count || !recs || !match_pose || !pose_front || !laser_off || !laser_frame || !laser_pts ||
        !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_init: bad argument");
    if ((long long)c->L.B * (n - 1) * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_init: B * (n - 1) * cap must fit in int32");
    const size_t lds = 4 * ((size_t)n + 1);
    if (lds > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_pack_init: n needs more than 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfe_scan_init, dim3(1), dim3(1024), 0, s, c->L.B, n - 1, cap, count, laser_off);
    if (int r = launched(c)) return r;
    int Ltot = 0;
    if (hipMemcpyAsync(&Ltot, laser_off + c->L.B, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(c, LIW_EHIP, "liw_lfe_pack_init: read-back of Ltot");
    if (Ltot > L_cap) return fail(c, LIW_ENOMEM, "liw_lfe_pack_init: Ltot exceeds L_cap");
    hipLaunchKernelGGL(k_lfe_pack_init, dim3(c->L.B), dim3(256), lds, s, c->L.B, n, cap, Ltot, laser_off, count, recs, match_pose, pose_front,
                       laser_frame, laser_pts, match_pose_out, has_match, init_ok);
    if (int r = launched(c)) return r;
    return Ltot;
}

int liw_lfe_rebuild(liw_lfe_ctx* c, void* store, int first_slot, int F, const double* poses, long long robot_stride, long long frame_stride,
                    const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !poses || F < 1 || first_slot < 0 || (long long)first_slot + F > c->L.slots) return fail(c, LIW_EINVAL, "liw_lfe_rebuild: bad argument");
    return add_scan_launch(c, store, first_slot, F, true, poses, robot_stride, frame_stride, mask, nullptr, stream);
}

int liw_lfe_track_layout(const liw_lfe_dims* dims, size_t* bytes) {
    Lay L;
    if (!bytes || !make_lay(dims, L)) return LIW_EINVAL;
    *bytes = (size_t)dims->B * kTrkBytes;
    return LIW_OK;
}

namespace {
TP track_tp(const liw_lfe_track_params* tp) {   // the extrinsic as liw_lie_from_matrix16 loads it
    TP t;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) t.Tiw_R[i * 3 + j] = tp->T_imu_to_wheel[i * 4 + j]; t.Tiw_t[i] = tp->T_imu_to_wheel[i * 4 + 3]; }
    if (tp->normalize_extrinsics) liw_normalize_rotation_host(t.Tiw_R);
    t.min_dt = tp->min_delta_t; t.p_thr = tp->key_frame_p_motion_threshold; t.q_thr = tp->key_frame_q_motion_threshold;
    return t;
}
}  // namespace

int liw_lfe_track_init(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, const double* x, long long robot_stride, const double* angular_local,
                       const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !x || robot_stride < 1) return fail(c, LIW_EINVAL, "liw_lfe_track_init: bad argument");
    hipLaunchKernelGGL(k_lfe_track_init, dim3(blocks(c->L.B, 256)), dim3(256), 0, (hipStream_t)stream, c->L.B, track, x, robot_stride, angular_local, mask);
    return launched(c);
}

int liw_lfe_track_begin(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, double* x, const double* imu_X, const double* imu_Dt,
                        const double* wheel_T, const double* stamps, const unsigned char* mask, double* linear, double* angular, double* pose_new,
                        unsigned char* skip, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !x || !imu_X || !imu_Dt || !wheel_T || !stamps || !linear || !angular || !pose_new || !skip)
        return fail(c, LIW_EINVAL, "liw_lfe_track_begin: null argument");
    hipLaunchKernelGGL(k_lfe_track_begin, dim3(blocks(c->L.B, 256)), dim3(256), 0, (hipStream_t)stream, c->L.B, c->P, track_tp(tp), track, x, imu_X, imu_Dt,
                       wheel_T, stamps, mask, linear, angular, pose_new, skip);
    return launched(c);
}

int liw_lfe_track_end(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* track, const void* store, int slot, const double* x, const int* count,
                      const unsigned char* mask, unsigned char* key, double* pose, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !track || !store || !x || !count || !key || !pose || slot < 0 || slot >= c->L.slots)
        return fail(c, LIW_EINVAL, "liw_lfe_track_end: bad argument");
    hipLaunchKernelGGL(k_lfe_track_end, dim3(blocks(c->L.B, 256)), dim3(256), 0, (hipStream_t)stream, store, c->L, c->P, track_tp(tp), track, slot, x, count,
                       mask, key, pose);
    return launched(c);
}

int liw_lfe_track_get(liw_lfe_ctx* c, const void* track, int robot, double* tf12, double* angular3, double* stamp, int* counters) {
    LIW_FLEET_DEV(c);
    if (!track || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_lfe_track_get: bad argument");
    Trk t;
    if (hipMemcpy(&t, (const char*)track + (size_t)robot * kTrkBytes, sizeof t, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    if (tf12) { for (int k = 0; k < 9; ++k) tf12[k] = t.kf_R[k]; for (int k = 0; k < 3; ++k) tf12[9 + k] = t.kf_t[k]; }
    if (angular3) for (int k = 0; k < 3; ++k) angular3[k] = t.ang[k];
    if (stamp) *stamp = t.stamp;
    if (counters) { counters[0] = t.tracked; counters[1] = t.keys; counters[2] = t.skipped; }
    return LIW_OK;
}

int liw_lfe_init_layout(const liw_lfe_dims* dims, size_t* bytes) {
    Lay L;
    if (!bytes || !make_lay(dims, L)) return LIW_EINVAL;
    *bytes = (size_t)dims->B * kIniBytes;
    return LIW_OK;
}

namespace {
IP init_ip(const liw_lfe_track_params* tp, const liw_lfe_init_params* ip) {
    const TP t = track_tp(tp);
    IP p;
    for (int k = 0; k < 9; ++k) p.Tiw_R[k] = t.Tiw_R[k];
    for (int k = 0; k < 3; ++k) p.Tiw_t[k] = t.Tiw_t[k];
    p.N = ip ? ip->slide_window_size : 0;
    p.p_thr = ip ? ip->p_motion_threshold : 0.0;
    p.q_thr = ip ? ip->q_motion_threshold : 0.0;
    return p;
}
}  // namespace

int liw_lfe_init_reset(liw_lfe_ctx* c, const liw_lfe_track_params* tp, void* init, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !init) return fail(c, LIW_EINVAL, "liw_lfe_init_reset: bad argument");
    hipLaunchKernelGGL(k_lfe_init_reset, dim3(blocks(c->L.B, 256)), dim3(256), 0, (hipStream_t)stream, c->L.B, init_ip(tp, nullptr), init, mask);
    return launched(c);
}

int liw_lfe_init_get(liw_lfe_ctx* c, const void* init, int robot, int* status, int* n_frames, double* state15, double* angular3, int* counters) {
    LIW_FLEET_DEV(c);
    if (!init || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_lfe_init_get: bad argument");
    Ini r;
    if (hipMemcpy(&r, (const char*)init + (size_t)robot * kIniBytes, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LIW_EHIP, "hipMemcpy");
    if (status) *status = r.status;
    if (n_frames) *n_frames = r.n_frames;
    if (state15) {
        for (int k = 0; k < 3; ++k) { state15[k] = r.p[k]; state15[3 + k] = r.q[k]; state15[6 + k] = r.v[k]; }
        for (int k = 0; k < 6; ++k) state15[9 + k] = r.bs[k];
    }
    if (angular3) for (int k = 0; k < 3; ++k) angular3[k] = r.ang[k];
    if (counters) { counters[0] = r.inits; counters[1] = r.failed; counters[2] = r.dropped; }
    return LIW_OK;
}

int liw_lfe_init_begin(liw_lfe_ctx* c, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, const double* imu_X,
                       const double* imu_J, const double* imu_sqrtP, const double* imu_Dt, const double* wheel_T, const double* wheel_sqrtP,
                       const unsigned char* mask, double* x_init, double* w_imu_X, double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt,
                       double* w_wheel_T, double* w_wheel_sqrtP, unsigned char* drop, int* slot_of, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !ip || !init || !imu_X || !imu_J || !imu_sqrtP || !imu_Dt || !wheel_T || !wheel_sqrtP || !x_init || !w_imu_X || !w_imu_J ||
        !w_imu_sqrtP || !w_imu_Dt || !w_wheel_T || !w_wheel_sqrtP || !drop || !slot_of)
        return fail(c, LIW_EINVAL, "liw_lfe_init_begin: null argument");
    if (ip->slide_window_size < 2 || ip->slide_window_size > c->L.slots - 1)
        return fail(c, LIW_EINVAL, "liw_lfe_init_begin: slide_window_size must be 2 .. slots - 1");
    if (!c->d_rows && hipMalloc(&c->d_rows, sizeof(int) * (size_t)c->L.B) != hipSuccess) { c->d_rows = nullptr; return fail(c, LIW_ENOMEM, "hipMalloc"); }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfe_init_begin, dim3(blocks(c->L.B, 256)), dim3(256), 0, s, c->L.B, c->P, init_ip(tp, ip), init, imu_X, imu_Dt, wheel_T, mask, x_init,
                       drop, slot_of, c->d_rows);
    if (int r = launched(c)) return r;
    hipLaunchKernelGGL(k_lfe_init_rows, dim3(c->L.B), dim3(kBlock), 0, s, ip->slide_window_size - 1, c->d_rows, imu_X, imu_J, imu_sqrtP, imu_Dt, wheel_T,
                       wheel_sqrtP, w_imu_X, w_imu_J, w_imu_sqrtP, w_imu_Dt, w_wheel_T, w_wheel_sqrtP);
    return launched(c);
}

int liw_lfe_slot_copy(liw_lfe_ctx* c, void* store, const int* dst_slot, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (!store || !dst_slot) return fail(c, LIW_EINVAL, "liw_lfe_slot_copy: null argument");
    if (((size_t)store & 15) != 0) return fail(c, LIW_EINVAL, "liw_lfe_slot_copy: the store must be 16-byte aligned");
    hipLaunchKernelGGL(k_lfe_slot_copy, dim3(c->L.B), dim3(256), 0, (hipStream_t)stream, store, c->L, dst_slot, mask);
    return launched(c);
}

int liw_lfe_init_select(liw_lfe_ctx* c, const liw_lfe_init_params* ip, const void* init, unsigned char* ready, int* sel, int* n_sel, int* R_host,
                        void* stream) {
    LIW_FLEET_DEV(c);
    if (!ip || !init || !ready || !sel || !n_sel || ip->slide_window_size < 2) return fail(c, LIW_EINVAL, "liw_lfe_init_select: bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfe_init_select, dim3(1), dim3(1024), 0, s, c->L.B, ip->slide_window_size, init, ready, sel, n_sel);
    if (int r = launched(c)) return r;
    if (R_host && hipMemcpyAsync(R_host, n_sel, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(c, LIW_EHIP, "liw_lfe_init_select: copy of R");
    return LIW_OK;
}

int liw_lfe_pack_init_sel(liw_lfe_ctx* c, int R, const int* sel, int n, int cap, const int* count, const double* recs, const double* match_pose,
                          const double* pose_front, long long front_stride, int L_cap, int* laser_off, int* laser_frame, double* laser_pts,
                          double* match_pose_out, unsigned char* has_match, unsigned char* init_ok, void* stream) {
    LIW_FLEET_DEV(c);
    if (R < 1 || R > c->L.B || !sel || n < 2 || cap < 1 || L_cap < 0 || front_stride < 6 || !count || !recs || !match_pose || !pose_front || !laser_off ||
        !laser_frame || !laser_pts || !match_pose_out || !has_match)
        return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: bad argument");
    if ((long long)c->L.B * (n - 1) * cap >= (1LL << 31)) return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: B * (n - 1) * cap must fit in int32");
    const size_t lds = 4 * ((size_t)n + 1);
    if (lds > kWaveLdsMax) return fail(c, LIW_EINVAL, "liw_lfe_pack_init_sel: n needs more than 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfe_scan_init_sel, dim3(1), dim3(1024), 0, s, R, n - 1, cap, count, sel, laser_off);
    if (int r = launched(c)) return r;
    int Ltot = 0;
    if (hipMemcpyAsync(&Ltot, laser_off + R, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(c, LIW_EHIP, "liw_lfe_pack_init_sel: read-back of Ltot");
    if (Ltot > L_cap) return fail(c, LIW_ENOMEM, "liw_lfe_pack_init_sel: Ltot exceeds L_cap");
    hipLaunchKernelGGL(k_lfe_pack_init_sel, dim3(R), dim3(256), lds, s, R, n, cap, Ltot, laser_off, count, recs, match_pose, pose_front, front_stride, sel,
                       laser_frame, laser_pts, match_pose_out, has_match, init_ok);
    if (int r = launched(c)) return r;
    return Ltot;
}

int liw_lfe_init_commit(liw_lfe_ctx* c, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, void* track, int R, const int* sel,
                        const unsigned char* init_ok, const double* x_sol, double* x_init, double* x_track, void* stream) {
    LIW_FLEET_DEV(c);
    if (!tp || !ip || !init || !track || R < 1 || R > c->L.B || !sel || !init_ok || !x_sol || !x_init || !x_track || ip->slide_window_size < 2)
        return fail(c, LIW_EINVAL, "liw_lfe_init_commit: bad argument");
    hipLaunchKernelGGL(k_lfe_init_commit, dim3(blocks(R, 256)), dim3(256), 0, (hipStream_t)stream, R, init_ip(tp, ip), init, track, sel, init_ok, x_sol, x_init,
                       x_track);
    return launched(c);
}

int liw_lfe_crmath_eval(liw_lfe_ctx* c, int op, int n, const double* a, const double* b, double* out, void* stream) {
    LIW_FLEET_DEV(c);
    if (op < 0 || op > 2 || n < 0 || !a || !out || (op == 2 && !b)) return fail(c, LIW_EINVAL, "liw_lfe_crmath_eval: bad argument");
    if (n == 0) return LIW_OK;
    hipLaunchKernelGGL(k_lfe_crmath, dim3(blocks((size_t)n, 256)), dim3(256), 0, (hipStream_t)stream, op, n, a, b, out);
    return launched(c);
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
