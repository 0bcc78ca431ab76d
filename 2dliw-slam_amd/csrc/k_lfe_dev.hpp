// k_lfe_dev.hpp — device code that the kernel units of the fleet laser front-end (k_lfe_*.hip) share: a slot of the store, the
// geometry of liw_laser.cpp in its operation order, and the correctly rounded scalar of the per-robot state machines.  Everything is
// inline; a unit includes it after its `#pragma clang fp contract(off)`.  (add_line, add_segment, their fit, the sorts and the
// rasterisation walk are used by the spawn and the add_scan kernels alone, which share k_lfe_lines.hip.)
// The line_map of a slot is a list of 64-bit entries (cell key << 32 | line index) kept sorted: within a cell the host
// pushes line ids in increasing order (ids only grow and a cell never takes the same id twice in a row), so sorting by
// (cell, line index) reproduces the host's push order exactly.
// No floating-point atomics on sums (the one LDS atomic is a maximum of non-negative doubles, and the hash set's content does
// not depend on the insertion order): runs are bitwise reproducible.
#pragma once
#include "k_lfe.hpp"
#include "liw_crmath.hpp"
#include "liw_dual.hpp"

namespace lfe {

using liw::Iso;
using liw::M3;
using liw::V3;
typedef V3<double> Vec;

constexpr double kEps = 0.0008;             // epsilo, laser_manager.cpp:3

struct Slot { SlotHdr* h; double* lines; u64* ent; };
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

__device__ inline Iso<double> til(const DP& P) { return liw::cast_iso<double>(P.Til_R, P.Til_t); }
__device__ inline Iso<double> tf6(const double* p6) { return liw::make_tf(ld3(p6), ld3(p6 + 3)); }

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

}  // namespace lfe
