/* liw_preint_batch.h — C ABI of the fleet's pre-integration on the device: the front door of a fleet frame.  Every robot of a fleet
 * of B owns a persistent pair of accumulators in device memory — imu_preintegraption and wheel_odom_preintegration as liw_preint.cpp
 * holds them, field for field — and is fed the raw IMU and wheel-odometry messages that arrived before its scan.  liw_fpre_push
 * integrates them and emits the interval rows (imu_X / imu_J / imu_sqrtP / imu_Dt / wheel_T / wheel_sqrtP / wheel_Dt) of the
 * liw_batch layout that liw_lfe_track_begin, liw_lfe_init_begin and the batch solver take in place, without a host loop over robots
 * and without a read-back.  What liw_batch_imu_preint / liw_batch_wheel_preint cannot express is what a live robot needs:
 *   - the accumulators persist across scans that the gates throw away (lvio_2d_trajectory.hpp:114-115 returns before update_only_t /
 *     reset): liw_fpre_push aligns a COPY of the accumulator with the scan stamp and leaves the persisted one un-aligned; only
 *     liw_fpre_commit, called after the frame's gates and solve, resets the accumulators of the robots whose frame was taken;
 *   - the IMU accumulator is reset with current_bs, the bias at the scan's arrival (:123): liw_fpre_push stores the stamp and the bias
 *     it is given as pending, and liw_fpre_commit resets with them;
 *   - the imu_inited / wheel_odom_inited latch (:87,90,110) lives in the robot's region and is reported as `ready`.
 * The host accumulators (liw_imu_preint_*, liw_wheel_preint_*) are the per-robot checker: the kernels run the same arithmetic per
 * message (csrc/k_preint_dev.hpp, shared with the batch-replay kernels of liw_batch_*_preint).
 *
 * Conventions as liw_map_batch.h and liw_loop_batch.h:
 *   - the caller owns all device memory: the store (sized by liw_fpre_store_bytes) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no call synchronises or reads back;
 *     liw_fpre_get at the end is a synchronous copy for tests and tools;
 *   - every stage takes a `mask` [B] uint8 (NULL = all): of a masked-out robot no byte of the store's robot region or of an output
 *     row is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device liw_fpre_create still returns a ctx, but every compute entry returns
 *     LIW_ENODEV.  liw_fpre_store_bytes and liw_fpre_layout are host-only and work anywhere.
 * The store is 8-byte aligned.  A fresh store must be reset once.  Two calls on one store must not overlap on different streams.
 *
 * The robot region (liw_fpre_layout_info::robot_bytes = 4608, 256-byte aligned, independent of B and of the robot's index), in
 * doubles:
 *     0 ..  15   X [15] (alpha beta gamma ba bw), one pad
 *    16 .. 255   J [15][16]: row r at 16 r, column 15 is a zero pad, so that the 16 lanes of a robot load a row in one 128-byte piece
 *   256 .. 495   P [15][16], likewise
 *   496 .. 503   last_acc [3], last_gyro [3], last_add_imu_time (-1: no message yet), Dt
 *   504 .. 536   wheel: delta_Tij [12] (R row-major, t), last_pose [12], v [3], omega [3], last_update_time (-1: none yet),
 *                last_add_time, Dt
 *   537 .. 543   the pending stamp and the pending bias [6] (ba, bw) of the last liw_fpre_push
 *   544          the latch: byte 0 imu_inited, byte 1 wheel_odom_inited, six zero bytes
 *   545 .. 575   zero
 * Behind the B robot regions lies the shared tail (liw_fpre_layout_info::shared_off): the aligned covariances P [B][225] of the last
 * push, which the square-root kernel reads.  Two robots fed the same messages, stamps and biases hold equal bytes and get equal rows,
 * whatever B, their index and `mask`.
 *
 * Limits (LIW_EINVAL otherwise): 1 <= B <= 2^20.
 */
#ifndef LIW_PREINT_BATCH_H
#define LIW_PREINT_BATCH_H
#include <stddef.h>

#include "liw_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_fpre_dims {
    int B;                /* robots */
} liw_fpre_dims;

typedef struct liw_fpre_layout_info {
    size_t bytes;            /* whole store = B * robot_bytes + shared_bytes */
    size_t robot_bytes;      /* region of one robot; robot b starts at b * robot_bytes */
    size_t shared_off;       /* = B * robot_bytes */
    size_t shared_bytes;     /* the aligned covariances, 1800 B per robot, rounded up to 256 */
    /* parts within a robot region, in bytes */
    size_t X_off, J_off, P_off, imu_last_off, wheel_off, pending_off, latch_off;
    int mat_pitch;           /* doubles per row of J and P in the region (16) */
} liw_fpre_layout_info;

/* one robot's accumulators as liw_fpre_get copies them out (J and P dense, row-major) */
typedef struct liw_fpre_state {
    double X[15], J[225], P[225], last_acc[3], last_gyro[3], last_add_imu_time, imu_Dt;
    double delta_Tij[12], last_pose[12], v[3], omega[3], last_update_time, last_add_time, wheel_Dt;
    double pending_stamp, pending_bias[6];
    unsigned char imu_inited, wheel_odom_inited;
} liw_fpre_state;

typedef struct liw_fpre_ctx liw_fpre_ctx;

/* bytes of the store for dims; LIW_EINVAL for bad dims.  Host-only. */
int liw_fpre_store_bytes(const liw_fpre_dims* dims, size_t* bytes);
/* the same with the sizes and offsets of the parts.  Host-only. */
int liw_fpre_layout(const liw_fpre_dims* dims, liw_fpre_layout_info* out);

/* a ctx bound to the noise sigmas of params (read as liw_imu_preint_create / liw_wheel_preint_create read them) and dims; the device
 * is params->device.  NULL only on a bad argument. */
liw_fpre_ctx* liw_fpre_create(const liw_params* params, const liw_fpre_dims* dims);
void liw_fpre_destroy(liw_fpre_ctx* ctx);
const char* liw_fpre_last_error(liw_fpre_ctx* ctx);

/* The state liw_imu_preint_create / liw_wheel_preint_create leave, latches off, no pending stamp, for the robots with mask[b] != 0 (all
 * when NULL).  LIW_EINVAL: a null or misaligned (8) store. */
int liw_fpre_reset(liw_fpre_ctx* ctx, void* store, const unsigned char* mask, void* stream);

/* One scan of every robot (with mask).  Robot b's messages are the rows imu_off[b] .. imu_off[b + 1] of imu [.][7] (t, acc, gyro) and
 * wheel_off[b] .. wheel_off[b + 1] of wheel [.][13] (t, R row-major 9, t 3): the sample rows of liw_batch_imu_preint /
 * liw_batch_wheel_preint, in time order, all stamped at or before stamps[b].  A robot whose offsets do not grow has no messages.
 *   1. add_imu_measure / add_wheel_odom_measure for every message into the persisted accumulators; imu_inited is set once an add
 *      integrates, wheel_odom_inited once an add passes the 0.05 s gate;
 *   2. stamps[b] and bias[b][6] (ba, bw: current_bs at the scan's arrival) are stored as pending;
 *   3. update_only_t(stamps[b]) on a copy, and its result into row b of imu_X [B][15], imu_J [B][225], imu_sqrtP [B][225], imu_Dt
 *      [B], wheel_T [B][12], wheel_sqrtP [B][9], wheel_Dt [B]; ready [B] uint8 = both latches set.
 * All arrays are device memory and must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null store / offsets / stamps / bias / output, a null imu or wheel array (pass any valid pointer when there is no
 * message at all), a misaligned store. */
int liw_fpre_push(liw_fpre_ctx* ctx, void* store, const int* imu_off, const double* imu, const int* wheel_off, const double* wheel,
                  const double* stamps, const double* bias, const unsigned char* mask, double* imu_X, double* imu_J, double* imu_sqrtP,
                  double* imu_Dt, double* wheel_T, double* wheel_sqrtP, double* wheel_Dt, unsigned char* ready, void* stream);

/* After the frame: for the robots with taken[b] != 0 (and mask) whose two latches are set, reset_wheel_odom_measure(stamp) and
 * reset_imu_measure(stamp, bias) with the pending stamp and bias: X = 0 except the bias, J = I, P = 1e-5 I, both Dt = 0, delta_Tij
 * = I, last_add_imu_time = last_update_time = stamp.  last_acc / last_gyro, v / omega, last_pose and last_add_time stay.  A robot
 * that is not taken keeps its accumulators un-aligned, as the reference's early return does: its next interval merges with this one.
 * LIW_EINVAL: a null store / taken, a misaligned store. */
int liw_fpre_commit(liw_fpre_ctx* ctx, void* store, const unsigned char* taken, const unsigned char* mask, void* stream);

/* ---- test and inspection hook (a synchronous device -> host copy).  LIW_EINVAL: robot outside 0 .. B-1, a null store / out. */
int liw_fpre_get(liw_fpre_ctx* ctx, const void* store, int robot, liw_fpre_state* out);

#ifdef __cplusplus
}
#endif
#endif
