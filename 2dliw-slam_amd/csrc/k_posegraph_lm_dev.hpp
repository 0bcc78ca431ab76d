// k_posegraph_lm_dev.hpp — device code that the LM loops of the fleet pose graph (k_posegraph_batch.hip) and of the group pose graph
// (k_group_graph.hip) share: the correctly rounded double of their bookkeeping, the wave reductions, Plus of the so3 parameterisation, and
// the index of the packed triangle.  Moved here from k_posegraph_batch.hip line for line.  The Cholesky with both triangular solves, the
// tail of k_fpg_reduced, is the text of k_pg_chol_body.inc, which both kernels include: a function call changed k_fpg_reduced's
// register allocation, a textual include keeps its bytes.
#pragma once
#include "liw_crmath.hpp"
#include "liw_kernels.hpp"

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

}  // namespace liw
