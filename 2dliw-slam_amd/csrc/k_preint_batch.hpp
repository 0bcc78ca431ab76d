// k_preint_batch.hpp — interface between the fleet pre-integration's host code (liw_preint_batch.cpp) and its kernels
// (k_preint_batch.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "liw_kernels.hpp"

namespace liw_fpre_dev {

// a robot region in doubles (include/liw_preint_batch.h)
constexpr int kPitch = 16;          // doubles per row of J and P
constexpr int R_X = 0, R_J = 16, R_P = 256, R_LACC = 496, R_LGYR = 499, R_ILAST = 502, R_IDT = 503;
constexpr int R_WDELTA = 504, R_WPOSE = 516, R_WV = 528, R_WOM = 531, R_WUPD = 534, R_WADD = 535, R_WDT = 536;
constexpr int R_STAMP = 537, R_BIAS = 538, R_LATCH = 544, R_USED = 545;
constexpr int kRobotDoubles = 576;  // 4608 bytes

struct Lay {
    int B;
    size_t robot_bytes, s_P, shared_bytes, bytes;
};

struct Rows {                        // the output rows of a push
    double *imu_X, *imu_J, *imu_sqrtP, *imu_Dt, *wheel_T, *wheel_sqrtP, *wheel_Dt;
    unsigned char* ready;
};

int launch_reset(char* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_push(char* store, const Lay& L, const liw::PreintNoise& N, const int* imu_off, const double* imu, const int* wheel_off,
                const double* wheel, const double* stamps, const double* bias, const unsigned char* mask, const Rows& out, hipStream_t s);
int launch_commit(char* store, const Lay& L, const unsigned char* taken, const unsigned char* mask, hipStream_t s);

}  // namespace liw_fpre_dev
