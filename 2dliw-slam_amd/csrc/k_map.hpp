// k_map.hpp — interface between the occupancy-grid map's host code (liw_map.cpp) and its kernels (k_map.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace liw_map_dev {

constexpr int kBlock = 256;          // work-group size of every kernel
constexpr int kRayLanes = 16;        // lanes that share one ray in k_map_rays
constexpr int kLdsSteps = 1536;      // step-table entries staged in LDS (38 m at 5 cm); later entries come from global memory
constexpr unsigned kSampled = 1u, kHit1 = 2u, kHit2 = 4u;   // the three monotone bits of a cell

struct Grid {                        // what the host derived from the bounds
    int width, height;
    double origin_x, origin_y, res, step;
};

// counters[]: 0 samples, 1 cells of value 0, 2 of value 50, 3 of value 100, 4 SAMPLED atomics issued,
// 5 cell visits (samples left after dropping those that repeat the previous sample's cell), 6 HIT atomics issued
constexpr int kCounters = 8;

// lane per point: partial[block][6] = min x, max x, min y, max y, max len, valid points; then folded into bounds[6]
int launch_bounds(const double* pts, const int* sub, const double* tf, long long npts, double* partial, double* bounds, hipStream_t s);
// zero the cell bits [ncell rounded up to 16] and the counters
int launch_clear(uint8_t* bits, long long ncell, unsigned long long* counters, hipStream_t s);
// 16 lanes per ray over the step table T[nT]
int launch_rays(const double* pts, const int* sub, const double* tf, long long npts, const double* T, int nT, const Grid& g, uint8_t* bits,
                unsigned long long* counters, hipStream_t s);
// bits -> -1 / 0 / 50 / 100 and the counts
int launch_finish(const uint8_t* bits, long long ncell, signed char* grid, unsigned long long* counters, hipStream_t s);

}  // namespace liw_map_dev
