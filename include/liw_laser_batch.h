/* liw_laser_batch.h — C ABI of the batched laser front-end on the device: the tracking-time work of liw_laser.h for B robots
 * at once (ranges -> points -> de-skew -> lines -> matches against the reference sub-map -> sub-map update -> the laser arrays
 * of a liw_batch), so that a fleet's frame never leaves device memory, and the initialisation that comes before it (the matches
 * of a window against its front key frame, the INIT-topology laser arrays, the sub-map rebuild at the solved poses).  The
 * single-scan host front-end (liw_laser.h) is the parity reference of every entry point here.
 *
 * Conventions as the batch API of liw_window.h:
 *   - the caller owns all device memory: the store (sized by liw_lfe_store_layout) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream);
 *   - calls return 0 (or a documented count) on success and a negative LIW_E* code otherwise;
 *   - there is NO CPU fallback: without a gfx950 device liw_lfe_create still returns a ctx, but every compute entry returns
 *     LIW_ENODEV.  liw_lfe_store_layout is host-only and works anywhere.
 * fp64 everywhere except the LaserScan ranges (float32, as sensor_msgs/LaserScan).  Points are [robot][max_points][3] in the
 * LASER frame; poses [robot][6] = (p, q = rotation vector) of the IMU in the world, as in liw_laser.h.
 *
 * The store holds, per robot: a status word and the laser_manager state (reference / spawning sub-maps and their poses,
 * last_add_tf, current_count), and `slots` scan slots plus the two sub-map slots.  A scan slot holds the scan time, its
 * lines in scan::lines order ([p1 p2 abc len]) and the sparse line_map as sorted (cell, line index) entries.
 *
 * Capacity: a scan with more than max_lines lines or max_cell_entries cell entries, a robot with more than max_points points
 * and a match with more than `cap` pairs set a LIW_LFE_ST_* bit in the robot's status word (and in the slot's, for a slot).  A
 * slot with a bit set is invalid: a match against it has count 0.  Nothing is ever written outside the robot's own region of
 * the store or of an output array; other robots are unaffected.
 *
 * Numerics: the front-end kernels are compiled without FMA contraction, like the host.  ranges_to_points, spawn and the
 * end points of the lines are bit-identical to the host; transforms built by make_tf (deskew, match, add_scan) use the device
 * sin / cos and agree to round-off.  Decisions through acos (segment merge, the 10 degree gate, the argmin, the corners'
 * 30 / 150 degree gate, and the motion filter's rotation angle, via log_SO3) use the device acos, which may differ from glibc's
 * by an ulp: a decision can only differ from the host where two quantities are within an ulp of each other.
 */
#ifndef LIW_LASER_BATCH_H
#define LIW_LASER_BATCH_H
#include <stddef.h>

#include "liw_laser.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits (robot word and slot word) */
#define LIW_LFE_ST_POINTS 1    /* more kept points than max_points (the point arrays hold the first max_points) */
#define LIW_LFE_ST_LINES 2     /* more lines than max_lines */
#define LIW_LFE_ST_CELLS 4     /* more cell entries than max_cell_entries */
#define LIW_LFE_ST_MATCH 8     /* a match had more pairs than `cap` (count = 0 written) */
#define LIW_LFE_ST_INVALID 16  /* an operation read an invalid slot */
#define LIW_LFE_ST_CORNERS 32  /* more corners than max_corners / acc_cap (robot word only: the slot stays valid) */

/* slot selectors besides 0 .. slots-1 */
#define LIW_LFE_REF (-1)       /* the manager's current reference sub-map */
#define LIW_LFE_SPAWNING (-2)  /* the manager's spawning sub-map (getters only) */
#define LIW_LFE_ROBOT (-3)     /* liw_lfe_status: the robot's accumulated status word */

/* getter result for a sub-map that does not exist or a point outside the grid (distinct from every LIW_E* code) */
#define LIW_LFE_NONE (-61)

typedef struct liw_lfe_dims {
    int B;                 /* robots */
    int slots;             /* scan slots per robot (besides the two sub-map slots) */
    int max_points;        /* points per robot (ranges_to_points / deskew / spawn arrays) */
    int max_lines;         /* lines per slot (scan slots and sub-maps) */
    int max_cell_entries;  /* line_map entries per slot */
} liw_lfe_dims;

typedef struct liw_lfe_ctx liw_lfe_ctx;

/* bytes of the store for `dims`; LIW_EINVAL for a non-positive dimension.  Host-only. */
int liw_lfe_store_layout(const liw_lfe_dims* dims, size_t* bytes);

/* a ctx bound to the laser parameters and dims (device = HIP device ordinal).  NULL only on a bad argument. */
liw_lfe_ctx* liw_lfe_create(const liw_laser_params* prm, const liw_lfe_dims* dims, int device);
void liw_lfe_destroy(liw_lfe_ctx* ctx);
const char* liw_lfe_last_error(liw_lfe_ctx* ctx);

/* LaserScan geometry shared by all robots: the host computes the (cosf, sinf) table of the n_rays angles once with the host libm
 * (what liw_laser_to_points uses) and keeps it on the device; synchronous. */
int liw_lfe_set_geometry(liw_lfe_ctx* ctx, int n_rays, float angle_min, float angle_increment, float time_increment);

/* laser_manager::clear_all_scan for the robots with mask[b] != 0 (all when mask is NULL): empties their scan slots, sub-maps,
 * manager state and status word.  A fresh store must be reset once before use. */
int liw_lfe_store_reset(liw_lfe_ctx* ctx, void* store, const unsigned char* mask, void* stream);

/* liw_laser_to_points per robot: ranges [B][n_rays] float32, stamps [B] -> pts [B][max_points][3], times [B][max_points],
 * n_pts [B].  Bit-identical to the host.  A robot with more than max_points kept points gets n_pts = max_points + 1 (the arrays
 * hold its first max_points points), which liw_lfe_spawn rejects: the slot is invalid.  `store` may be NULL; otherwise an
 * overflow also sets LIW_LFE_ST_POINTS in the robot word. */
int liw_lfe_ranges_to_points(liw_lfe_ctx* ctx, void* store, const float* ranges, const double* stamps, double* pts, double* times,
                             int* n_pts, void* stream);

/* liw_laser_correct per robot, in place: linear [B][3], angular [B][3] body twist at stamps [B]. */
int liw_lfe_deskew(liw_lfe_ctx* ctx, double* pts, const double* times, const int* n_pts, const double* stamps, const double* linear,
                   const double* angular, void* stream);

/* liw_scan_spawn per robot into scan slot `slot` (0 .. slots-1): pts [B][max_points][3], n_pts [B], times [B] (scan time, may be
 * NULL = 0).  n_pts outside 0 .. max_points leaves the slot empty and invalid (LIW_LFE_ST_POINTS); so does a scan with more than
 * max_lines lines or max_cell_entries entries (its n_lines / n_entries read 0).  Corners: liw_lfe_spawn_corners.
 * One wavefront works on one scan, with the scan's points and the intermediate arrays in LDS: about 34 bytes per point of
 * max_points and 8 per line of max_lines (39 KiB at 1 080 points and 256 lines); the line_map entries are collected, made unique
 * and sorted in the bytes of the point array once the points are no longer needed.  Dimensions that need more than the 64 KiB of a
 * work-group, and every call made while the environment has LIW_LFE_SPAWN=lane (read per call), go to the lane-per-scan kernel
 * instead, which writes the same bytes for every valid slot (header, lines[0 .. n_lines), entries[0 .. n_entries)). */
int liw_lfe_spawn(liw_lfe_ctx* ctx, void* store, int slot, const double* pts, const int* n_pts, const double* times, void* stream);

/* liw_lfe_spawn that also writes scan::concers: corners [B][max_corners][3] (laser frame, z = 0) in the host's push order,
 * duplicates included, and n_corners [B].  A scan with more than max_corners corners gets n_corners = max_corners + 1 (the array
 * holds the first max_corners) and LIW_LFE_ST_CORNERS in the robot word.  An invalid scan has n_corners = 0.  The slot is written
 * exactly as by liw_lfe_spawn.  The coordinates are bit-identical to the host's; the 30 / 150 degree gate goes through the device
 * acos (the caveat above).  Only the wave-per-scan kernel computes corners: LIW_EINVAL with LIW_LFE_SPAWN=lane or when the
 * dimensions need more than 64 KiB of LDS. */
int liw_lfe_spawn_corners(liw_lfe_ctx* ctx, void* store, int slot, const double* pts, const int* n_pts, const double* times,
                          int max_corners, double* corners, int* n_corners, void* stream);

/* What lvio_2d::trajectory does with the corners after a tracking solve.  Robots with clear[b] != 0 (clear may be NULL) start from
 * n_acc[b] = 0 (a key frame handed its corners over), whatever the mask says.  Then, for the robots with mask[b] != 0 (all when
 * NULL), make_tf(pose[b]) * T_imu_to_laser * corner is appended to acc [B][acc_cap][3] at n_acc[b], and n_acc[b] advances.  An
 * append that does not fit writes nothing, leaves n_acc[b] = acc_cap + 1 (which stays until the robot is cleared) and sets
 * LIW_LFE_ST_CORNERS in the robot word (store may be NULL: no word); n_corners[b] > max_corners does the same. */
int liw_lfe_corners_to_world(liw_lfe_ctx* ctx, void* store, int max_corners, const double* corners, const int* n_corners,
                             const double* pose, const unsigned char* mask, const unsigned char* clear, int acc_cap, double* acc,
                             int* n_acc, void* stream);

/* liw_laser_do_match(slot1, slot2, pose1, pose2, kk) per robot.  slot1 = LIW_LFE_REF matches against the reference sub-map with
 * its stored pose as p1, q1 (pose1 is ignored and may be NULL), as laser_manager::match_with_ref; no reference gives count 0 and
 * the pose record (p2 q2 p2 q2) of an empty match.  Outputs: count [B], recs [B][cap][12] (lines1.p1 p1.p2 lines2.p1 lines2.p2),
 * idx1 / idx2 [B][cap] (indices in scan::lines; either may be NULL), match_pose [B][12] = p1 q1 p2 q2. */
int liw_lfe_match(liw_lfe_ctx* ctx, void* store, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap,
                  int* count, double* recs, int* idx1, int* idx2, double* match_pose, void* stream);

/* laser_manager::add_scan of scan slot `src_slot` at pose [B][6] for the robots with mask[b] != 0 (all when NULL): motion filter,
 * first-scan sub-map, rasterisation into the reference and spawning sub-maps, the ref_n_accumulation swap.  The key-frame deque
 * stays with the caller.  An invalid source slot makes every sub-map the call writes invalid (its status and
 * LIW_LFE_ST_INVALID), so matches against it have count 0 until that sub-map is replaced.
 * Mapping: one wavefront per robot (k_lfe_add_scan_wave).  The manager's decisions are wave-uniform and made with the device
 * functions of the lane-per-robot kernel; a lane fits and rasterises one source line (chunks of 64), line ids and entry positions
 * are prefix counts, the call's new entries are sorted in LDS and merged into the sorted old ones in place.  LDS: 12 bytes per
 * new entry of a call (at most 2 048 held) and 8 per line of max_lines.  The lane-per-robot kernel (k_lfe_add_scan) is the checker:
 * the environment's LIW_LFE_ADD_SCAN=lane, read per call, selects it (=wave: the default), and it takes every call whose
 * dimensions need more than 64 KiB of LDS.
 * Equal between the two kernels, bit for bit: the robot's manager record and status word, and of every sub-map slot its
 * header, lines[0 .. n_lines) and entries[0 .. n_entries) (tests/test_gpu_laser_add_scan_wave.py).  A target whose new entries
 * exceed what the wave holds in LDS, or that overflows max_lines / max_cell_entries, is built by one lane with the lane kernel's
 * code, so the same holds for it; of an overflowed sub-map (LIW_LFE_ST_LINES / _CELLS) callers may rely only on its status
 * words, the manager record, count 0 of every match against it, and that nothing outside the robot's region is written: which
 * lines and entries it keeps is unspecified. */
int liw_lfe_add_scan(liw_lfe_ctx* ctx, void* store, int src_slot, const double* pose, const unsigned char* mask, void* stream);

/* what liw_lfe_add_scan_flags did for robot b */
#define LIW_LFE_ADD_ADDED 1    /* passed the motion filter, or was the first scan: the sub-maps changed */
#define LIW_LFE_ADD_FIRST 2    /* created the first reference sub-map */
#define LIW_LFE_ADD_SPAWNED 4  /* created the spawning sub-map at count == ref_n_accumulation / 2 */
#define LIW_LFE_ADD_SWAPPED 8  /* count reached ref_n_accumulation: reference := spawning (which may not exist), fresh spawning */

/* liw_lfe_add_scan that also reports what it did: flags [B] bytes, 0 for a robot that is masked out or whose scan the motion
 * filter dropped, otherwise the OR of LIW_LFE_ADD_*.  After LIW_LFE_ADD_SWAPPED every later match against LIW_LFE_REF uses the new
 * reference, and with ref_n_accumulation = 2 the robot may have no reference at all until its next added scan
 * (LIW_LFE_ADD_FIRST again).  LIW_EINVAL for a null flags; in every other respect the same call. */
int liw_lfe_add_scan_flags(liw_lfe_ctx* ctx, void* store, int src_slot, const double* pose, const unsigned char* mask, unsigned char* flags,
                           void* stream);

/* the kernel the last liw_lfe_add_scan / _flags / liw_lfe_rebuild of this ctx launched: 0 lane-per-robot, 1 wave-per-robot;
 * LIW_EINVAL before any such call.  Host-only state, but LIW_ENODEV without a device like every call that needs one. */
int liw_lfe_add_scan_path(liw_lfe_ctx* ctx);

/* The laser arrays of a liw_batch of B n-frame windows whose laser blocks all belong to frame `frame` (n = 2 tracking: 1), from a
 * liw_lfe_match output (count, recs with row stride cap, match_pose):
 *   laser_off [B+1], laser_frame [Ltot] (= frame), laser_pts [12][Ltot] component-major, match_pose_out [B][n][12] row `frame`,
 *   has_match [B][n] row `frame` (= 1).  Rows of other frames are not touched.
 * laser_frame / laser_pts must hold L_cap blocks; Ltot > L_cap is LIW_ENOMEM (nothing but laser_off written).  Returns Ltot:
 * the one host read-back (a 4-byte copy and a synchronisation of `stream`). */
int liw_lfe_pack_track(liw_lfe_ctx* ctx, int n, int frame, int cap, const int* count, const double* recs, const double* match_pose,
                       int L_cap, int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match,
                       void* stream);

/* Initialisation (lvio_2d::trajectory while status == INITIALIZING).  The window's scans are kept in scan slots (by the caller, or per
 * robot by liw_lfe_init_begin + liw_lfe_slot_copy below); the
 * reference's per-frame add_scan calls while INITIALIZING only feed the key-frame deque (here: the caller's slots) and sub-maps
 * that clear_all_scan discards before anything reads them, so the device path does not make them: a window is
 * spawn (per frame) -> liw_lfe_match_front -> liw_lfe_pack_init -> the INIT solve -> liw_lfe_rebuild at the solved poses.
 *
 * liw_lfe_match_front: laser_manager::match_with_front of a whole window in one launch.  Task (robot b, frame k), k = 0 .. F-1, is
 * exactly liw_lfe_match(front_slot, first_slot + k, pose_front, pose_k, kk): the same count, recs[0 .. count), idx1 / idx2[0 .. count)
 * and match_pose, count 0 and LIW_LFE_ST_INVALID for an invalid slot, count 0 and LIW_LFE_ST_MATCH for more than cap pairs (bytes of
 * recs past count are unspecified).  pose_front [B][6]; the pose of frame k of robot b is read at
 * poses + b * robot_stride + k * frame_stride (strides in doubles: a packed [B][F][6] array has 6 F and 6; the states array
 * x [B][n][15] of a liw_batch, offset to its first matched frame, has 15 n and 15).  Outputs by task: count [B][F],
 * recs [B][F][cap][12], idx1 / idx2 [B][F][cap] (either may be NULL), match_pose [B][F][12].  One wavefront works on one task (lanes
 * over the lines of the frame's scan, 12 bytes of LDS per line of max_lines); the mean distance is summed and the pairs are written in
 * line order, so the result is bit-identical to liw_lfe_match's.  Tasks of one robot set its status word with an atomic OR.
 * LIW_EINVAL: F < 1, first_slot < 0, first_slot + F > slots, front_slot outside 0 .. slots-1, cap < 1, kk < 0, a null array. */
int liw_lfe_match_front(liw_lfe_ctx* ctx, void* store, int front_slot, int first_slot, int F, const double* pose_front, const double* poses,
                        long long robot_stride, long long frame_stride, int kk, int cap, int* count, double* recs, int* idx1, int* idx2,
                        double* match_pose, void* stream);

/* The laser arrays of a liw_batch of B n-frame INIT windows from a liw_lfe_match_front output with F = n - 1 (task k is frame k + 1;
 * count, recs with row stride cap, match_pose) and the front poses:
 *   laser_off [B+1]; laser_frame [Ltot]: the owning frame of every block, ascending inside each window; laser_pts [12][Ltot]
 *   component-major; match_pose_out [B][n][12]; has_match [B][n]; init_ok [B] (may be NULL).
 * Frame 0 of every window gets the empty match of the reference's first frame: no blocks, match_pose (p0 q0 p0 q0) from pose_front,
 * has_match 1.  Frame f = 1 .. n-1 gets its match's pose row, has_match 1 and its count blocks (counts clamped to 0 .. cap).
 * init_ok[b] = 1 iff every frame 1 .. n-1 of robot b has count >= 2 (check_and_processing_initialize's lines2.size() < 2 test).  A
 * failing robot is packed like any other; the caller masks it out of liw_lfe_rebuild and gives it to liw_lfe_store_reset, as the
 * reference does with pop_frame + clear_all_scan + init_current_status.  No atomics decide a position: the output is deterministic.
 * laser_frame / laser_pts must hold L_cap blocks; Ltot > L_cap is LIW_ENOMEM (nothing but laser_off written).  Returns Ltot: the one
 * host read-back (a 4-byte copy and a synchronisation of `stream`).  LIW_EINVAL: n < 2, cap < 1, L_cap < 0, a null array. */
int liw_lfe_pack_init(liw_lfe_ctx* ctx, int n, int cap, const int* count, const double* recs, const double* match_pose, const double* pose_front,
                      int L_cap, int* laser_off, int* laser_frame, double* laser_pts, double* match_pose_out, unsigned char* has_match,
                      unsigned char* init_ok, void* stream);

/* The sub-map rebuild after init_solve: for the robots with mask[b] != 0 (all when NULL) laser_manager::clear_all_scan on the manager
 * alone (state, status word, both sub-maps; every scan slot is kept), then liw_lfe_add_scan of scan slot first_slot + k at pose k for
 * k = 0 .. F-1 in order (motion filter, first-scan sub-map, the ref_n_accumulation swap, invalid-source propagation).  Poses strided
 * as in liw_lfe_match_front, with k = 0 the window's first frame.  LIW_EINVAL: F < 1, first_slot < 0, first_slot + F > slots.
 * One launch: the robot's wavefront resets its manager and walks the F frames itself, program order standing in for the launch
 * boundaries; the store's bytes are those of the F + 1 launches of the lane path (LIW_LFE_ADD_SCAN=lane), as for liw_lfe_add_scan. */
int liw_lfe_rebuild(liw_lfe_ctx* ctx, void* store, int first_slot, int F, const double* poses, long long robot_stride, long long frame_stride,
                    const unsigned char* mask, void* stream);

/* Tracking glue (lvio_2d::trajectory::add_sensor_data(laser) while status == TRACKING, around the stages above): the de-skew twist
 * from the current state, the min_delta_t gate, update_current_status (the new frame's pose from the wheel increment), the roll of
 * the two-frame window (pop_frame_for_tracking with keep_window_size = 1) and the key-frame decision against last_keyframe_tf.
 * The INITIALIZING state machine is the initialisation glue below; the key-frame deque and the sensor-inited latch (imu_inited /
 * wheel_odom_inited: the caller starts stepping once it has intervals) stay with the caller.
 *
 * The tracking record is caller-owned device memory apart from the store (whose layout does not change), robot-major, 256 bytes per
 * robot: last_keyframe_tf [12] (R row-major, then t), current_angular_local [3], the stamp of the last accepted frame, and the
 * int counters tracked frames, key frames, skipped frames; the rest is padding.
 * Mapping: a lane per robot, work-groups of 256, no LDS, no atomics.  The arithmetic is liw_lie.h's, in the reference's order, with
 * the device sin / cos / atan2: results agree with the host to round-off, and a decision can differ from the host's only where a
 * quantity is within round-off of its threshold.  liw_lfe_track_begin evaluates those three functions correctly rounded, which is
 * what the host's libm returns for all but about 0.1 % of the arguments (sin and cos of |x| <= 2^20, multiples of pi/2 included:
 * liw_lfe_crmath_eval below is how the tests see it): its twist and pose are bit-identical to the host's then,
 * so that a free-running chain of solves does not start from a last-bit difference. */
typedef struct liw_lfe_track_params {
    double T_imu_to_wheel[16];   /* 4x4 row-major, loaded as liw_lie_from_matrix16 does */
    int normalize_extrinsics;    /* re-orthonormalise its rotation (T_imu_to_laser is the ctx's, from its laser parameters) */
    double min_delta_t;          /* a frame whose IMU interval is shorter is skipped */
    double key_frame_p_motion_threshold;
    double key_frame_q_motion_threshold;
} liw_lfe_track_params;

/* bytes of the tracking record for `dims` (256 per robot); LIW_EINVAL for a non-positive dimension.  Host-only. */
int liw_lfe_track_layout(const liw_lfe_dims* dims, size_t* bytes);

/* What check_and_processing_initialize leaves behind for tracking, for the robots with mask[b] != 0 (all when NULL):
 * last_keyframe_tf = make_tf(p, q) of the state row at x + b * robot_stride (stride in doubles; the IMU pose, without T_imu_to_laser,
 * as the reference takes it), current_angular_local = angular_local [B][3] row b (zero when angular_local is NULL), stamp 0 and all
 * counters 0; the padding is zeroed.  LIW_EINVAL: a null tp / track / x, robot_stride < 1. */
int liw_lfe_track_init(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, void* track, const double* x, long long robot_stride,
                       const double* angular_local, const unsigned char* mask, void* stream);

/* Before the scan is processed.  x [B][2][15] are the states of the two-frame batch (row 1 the current state), imu_X [B][15],
 * imu_Dt [B], wheel_T [B][12] the interval's liw_batch arrays, stamps [B] the scan stamps.  Per robot with mask[b] != 0 (all when
 * NULL), in the reference's order:
 *   1. the de-skew twist from the state before the update: linear [B][3] row b = R_w_laser^T v with R_w_laser = R(q) R_il,
 *      angular [B][3] row b = log_SO3(R_il^T exp_so3(current_angular_local) R_il)  (what liw_lfe_deskew takes);
 *   2. skip [B] byte b = imu_Dt[b] < min_delta_t.  A skipped robot gets linear / angular / skip and its skipped counter advances;
 *      nothing else of it is written;
 *   3. otherwise the window rolls: x[b][0] := x[b][1], a bitwise copy;
 *   4. x[b][1].p, q := log_SE3(make_tf(p, q) * T_iw * wheel_T[b] * T_iw^-1); v, ba, bw are carried;
 *   5. current_angular_local := imu_X[b][6 .. 8] / imu_Dt[b], the stamp is stored, pose_new [B][6] row b = x[b][1][0 .. 5]
 *      (packed: what liw_lfe_match takes as pose2).
 * Of a masked-out robot no byte of x, track or any output is written.  LIW_EINVAL: a null tp or a null array other than mask. */
int liw_lfe_track_begin(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, void* track, double* x, const double* imu_X, const double* imu_Dt,
                        const double* wheel_T, const double* stamps, const unsigned char* mask, double* linear, double* angular, double* pose_new,
                        unsigned char* skip, void* stream);

/* After the solve.  Per robot with mask[b] != 0 (all when NULL; the caller masks out the robots liw_lfe_track_begin skipped):
 *   pose [B][6] row b = x[b][1][0 .. 5];  tf_w_l = make_tf(pose) * T_imu_to_laser;  delta = last_keyframe_tf^-1 * tf_w_l;
 *   static = |delta.t| < key_frame_p_motion_threshold && |log_SO3(delta.R)| < key_frame_q_motion_threshold  (both strict);
 *   n_match = count[b] (a liw_lfe_match count), n_no_match = n_lines - n_match with the clamped n_lines of scan slot `slot`;
 *   key [B] byte b = !static || n_match < n_no_match;  on a key frame last_keyframe_tf := tf_w_l;
 *   the tracked-frame counter advances, and the key-frame counter on a key frame.
 * key of frame t is the `clear` argument of liw_lfe_corners_to_world in frame t + 1: the corners of the key frame itself belong to
 * it.  The store is only read.  Of a masked-out robot nothing is written.  LIW_EINVAL: a null tp or a null array other than mask,
 * slot outside 0 .. slots-1. */
int liw_lfe_track_end(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, void* track, const void* store, int slot, const double* x,
                      const int* count, const unsigned char* mask, unsigned char* key, double* pose, void* stream);

/* the record of one robot (synchronous; tests and tools): tf12 = last_keyframe_tf, angular3, stamp, counters [3] = tracked, key,
 * skipped frames.  Any output may be NULL.  LIW_EINVAL: a null track, robot outside 0 .. B-1. */
int liw_lfe_track_get(liw_lfe_ctx* ctx, const void* track, int robot, double* tf12, double* angular3, double* stamp, int* counters);

/* Initialisation glue (lvio_2d::trajectory::add_sensor_data(laser) while status == INITIALIZING, per robot): the is_static gate on
 * the wheel increment, update_current_status, the frame and its interval pushed into the robot's window, and the bookkeeping of
 * check_and_processing_initialize around the INIT solve, so that robots whose windows fill at different frames share the uniform
 * liw_lfe_match_front / liw_lfe_rebuild calls.  Conventions as the tracking glue: no FMA contraction, of a masked-out robot no byte
 * is written, a failing call writes nothing, LIW_ENODEV without a device, the layout query is host-only.
 *
 * The initialisation record is caller-owned device memory apart from the store and from the tracking record, robot-major, 256 bytes
 * per robot: current_p / q / v [3 each], current_bs [6], current_angular_local [3], then the ints status (LIW_LFE_INITIALIZING /
 * LIW_LFE_TRACKING), n_frames (frames in the window being filled) and the counters initialisations, failed windows, dropped
 * frames; the rest is padding.  The extrinsic T_imu_to_wheel is taken from liw_lfe_track_params, which does not change. */
#define LIW_LFE_INITIALIZING 0
#define LIW_LFE_TRACKING 1

typedef struct liw_lfe_init_params {
    int slide_window_size;       /* N: frames of an INIT window */
    double p_motion_threshold;   /* is_static: a frame that moved less than both thresholds since the last one is dropped */
    double q_motion_threshold;
} liw_lfe_init_params;

/* bytes of the initialisation record for `dims` (256 per robot); LIW_EINVAL for a non-positive dimension.  Host-only. */
int liw_lfe_init_layout(const liw_lfe_dims* dims, size_t* bytes);

/* init_current_status for the robots with mask[b] != 0 (all when NULL): p, q = log_SE3(T_imu_to_wheel^-1), v, bs and
 * current_angular_local 0, INITIALIZING, n_frames 0, all counters 0; the padding is zeroed.  LIW_EINVAL: a null tp / init. */
int liw_lfe_init_reset(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, void* init, const unsigned char* mask, void* stream);

/* the record of one robot (synchronous; tests and tools): status, n_frames, state15 = p q v bs, angular3, counters [3] =
 * initialisations, failed windows, dropped frames.  Any output may be NULL.  LIW_EINVAL: a null init, robot outside 0 .. B-1. */
int liw_lfe_init_get(liw_lfe_ctx* ctx, const void* init, int robot, int* status, int* n_frames, double* state15, double* angular3, int* counters);

/* Before the scan is processed, for the robots with mask[b] != 0 (all when NULL) whose status is INITIALIZING and whose window is not
 * full (n_frames < N; a full window is committed before the next frame); of every other robot no byte is written.  imu_X [B][15],
 * imu_J [B][225], imu_sqrtP [B][225], imu_Dt [B], wheel_T [B][12], wheel_sqrtP [B][9] are the interval's liw_batch arrays.  In the
 * reference's order:
 *   1. laser_delta = T_lw * wheel_T[b] * T_lw^-1 with T_lw = T_imu_to_laser^-1 * T_imu_to_wheel (wheel_delta_to);
 *   2. drop [B] byte b = |laser_delta.t| < p_motion_threshold && |log_SO3(laser_delta.R)| < q_motion_threshold (both strict).  A
 *      dropped robot gets drop and its dropped counter advances; nothing else of it is written (the caller merges the interval into
 *      the next one, as for a skipped tracking frame);
 *   3. otherwise, with k = n_frames: p, q := log_SE3(make_tf(p, q) * T_iw * wheel_T[b] * T_iw^-1) (update_current_status); row k of
 *      x_init [B][N][15] := p q v bs; for k >= 1 the six interval arrays are copied into row k - 1 of the window arrays
 *      w_imu_X [B][N-1][15], w_imu_J [B][N-1][225], w_imu_sqrtP [B][N-1][225], w_imu_Dt [B][N-1], w_wheel_T [B][N-1][12],
 *      w_wheel_sqrtP [B][N-1][9] (the liw_batch layout of B N-frame windows; frame 0's interval is not stored);
 *      current_angular_local := imu_X[b][6 .. 8] / imu_Dt[b]; slot_of [B] int b = 1 + k, the scan slot the frame's scan belongs in
 *      (liw_lfe_slot_copy); n_frames := k + 1.
 * sin / cos / atan2 are evaluated correctly rounded, as in liw_lfe_track_begin: the predicted poses are where liw_lfe_match_front and
 * the INIT solve start.  Mapping: a lane per robot for the decision, then a second launch with a wavefront per robot for the rows; the
 * B row indices between the two launches live in the ctx, so calls on one ctx must not overlap on different streams.
 * LIW_EINVAL: a null tp / ip or a null array other than mask, slide_window_size outside 2 .. slots - 1. */
int liw_lfe_init_begin(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, const double* imu_X,
                       const double* imu_J, const double* imu_sqrtP, const double* imu_Dt, const double* wheel_T, const double* wheel_sqrtP,
                       const unsigned char* mask, double* x_init, double* w_imu_X, double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt,
                       double* w_wheel_T, double* w_wheel_sqrtP, unsigned char* drop, int* slot_of, void* stream);

/* Scan slot 0 of the robots with mask[b] != 0 (all when NULL) copied into slot dst_slot[b] of the same robot, in one launch: the
 * header with the slot's status word, lines[0 .. n_lines) and ent[0 .. n_entries), so an invalid slot stays invalid.  A dst_slot
 * outside 1 .. slots-1 sets LIW_LFE_ST_INVALID in the robot word and writes nothing else of that robot.  A work-group per robot with
 * 16-byte accesses: a pure copy, bounded by the store traffic of at most one slot read and written per robot.
 * LIW_EINVAL: a null store / dst_slot, a store that is not 16-byte aligned. */
int liw_lfe_slot_copy(liw_lfe_ctx* ctx, void* store, const int* dst_slot, const unsigned char* mask, void* stream);

/* ready [B] byte b = status == INITIALIZING && n_frames == slide_window_size; sel [B]: the ready robots in ascending order in
 * sel[0 .. R), entries past R untouched; n_sel [1] (device) = R.  Positions are prefix counts (no atomics): deterministic.  One
 * launch and no synchronisation: when R_host is not NULL, R is also copied there asynchronously on `stream` and is valid after the
 * stream's next synchronisation (the read-back of liw_lfe_pack_track's Ltot is one).
 * LIW_EINVAL: a null ip / init / ready / sel / n_sel, slide_window_size < 2. */
int liw_lfe_init_select(liw_lfe_ctx* ctx, const liw_lfe_init_params* ip, const void* init, unsigned char* ready, int* sel, int* n_sel, int* R_host,
                        void* stream);

/* liw_lfe_pack_init for the R robots of sel only: window r of the output is robot sel[r].  count, recs and match_pose are the
 * robot-major arrays liw_lfe_match_front wrote for all B robots; the front pose of robot b is read at pose_front + b * front_stride
 * (doubles; x_init itself has stride 15 N).  The outputs laser_off [R+1], laser_frame, laser_pts, match_pose_out [R][n][12],
 * has_match [R][n], init_ok [R] (may be NULL) are the bytes liw_lfe_pack_init writes for a fleet that consists of exactly those
 * robots.  Returns Ltot (one read-back); Ltot > L_cap is LIW_ENOMEM with nothing but laser_off written.
 * LIW_EINVAL: R outside 1 .. B, n < 2, cap < 1, L_cap < 0, front_stride < 6, a null array other than init_ok. */
int liw_lfe_pack_init_sel(liw_lfe_ctx* ctx, int R, const int* sel, int n, int cap, const int* count, const double* recs, const double* match_pose,
                          const double* pose_front, long long front_stride, int L_cap, int* laser_off, int* laser_frame, double* laser_pts,
                          double* match_pose_out, unsigned char* has_match, unsigned char* init_ok, void* stream);

/* After the INIT solve and the marginalisation of the compact batch whose window r is robot sel[r] (x_sol [>= R][N][15], init_ok [R]).
 * For r = 0 .. R-1 with init_ok[r]: row block sel[r] of x_init [B][N][15] := x_sol[r] (what liw_lfe_rebuild reads through strides);
 * both rows of x_track [B][2][15] := the last solved frame; the record's p q v bs := that frame (take_back_state); the robot's
 * tracking record as liw_lfe_track_init makes it from that frame, with current_angular_local from the initialisation record;
 * status := TRACKING and the initialisation counter advances.  Without init_ok[r]: init_current_status (as liw_lfe_init_reset, the
 * counters kept) and the failed-window counter advances; the caller gives the robot to liw_lfe_store_reset.  The priors of the
 * compact batch are plain row scatters and stay with the caller.  LIW_EINVAL: R outside 1 .. B, slide_window_size < 2, a null argument. */
int liw_lfe_init_commit(liw_lfe_ctx* ctx, const liw_lfe_track_params* tp, const liw_lfe_init_params* ip, void* init, void* track, int R, const int* sel,
                        const unsigned char* init_ok, const double* x_sol, double* x_init, double* x_track, void* stream);

/* A diagnostic entry, on no tracking path: the sin (op 0), cos (op 1) or atan2(a, b) (op 2) that liw_lfe_track_begin evaluates
 * (csrc/liw_crmath.hpp, as compiled for the device), element by element: out[i] = f(a[i]) or f(a[i], b[i]) for i = 0 .. n-1.  a, b,
 * out are device arrays of n doubles; b is not read and may be NULL for ops 0 and 1; out may alias a or b.  A lane per element,
 * work-groups of 256, one launch on `stream`; n = 0 launches nothing.  Results are the correctly rounded values for finite
 * |a| <= 2^20 (sin, cos) and for finite arguments below 1e300 that are not both below 1e-300 (atan2; within an ulp where the
 * result is below 2^-969); every other argument goes to the device library's function (tests/test_gpu_crmath.py).
 * LIW_EINVAL: op outside 0 .. 2, n < 0, a null a or out, a null b with op 2. */
int liw_lfe_crmath_eval(liw_lfe_ctx* ctx, int op, int n, const double* a, const double* b, double* out, void* stream);

/* getters (synchronous device -> host copies; tests and tools).  slot: 0 .. slots-1, LIW_LFE_REF or LIW_LFE_SPAWNING. */
/* status word of robot / slot (slot = LIW_LFE_ROBOT: the robot word); a missing sub-map reads LIW_LFE_NONE */
int liw_lfe_status(liw_lfe_ctx* ctx, const void* store, int robot, int slot);
/* number of lines (LIW_LFE_NONE: missing sub-map) */
int liw_lfe_num_lines(liw_lfe_ctx* ctx, const void* store, int robot, int slot);
/* lines [num_lines][10] = p1 p2 abc len in scan::lines order; returns the number written (<= cap) */
int liw_lfe_get_lines(liw_lfe_ctx* ctx, const void* store, int robot, int slot, double* out, int cap);
/* line_map of the cell containing (x, y), as liw_scan_cell_lines: ids (scan::lines indices, push order), returns the cell's size,
 * LIW_LFE_NONE outside the grid or for a missing sub-map */
int liw_lfe_cell_lines(liw_lfe_ctx* ctx, const void* store, int robot, int slot, double x, double y, int* ids, int cap);
/* pose p3, q3 of a sub-map slot (LIW_LFE_REF / LIW_LFE_SPAWNING); 0 if it exists, LIW_LFE_NONE if not */
int liw_lfe_submap_pose(liw_lfe_ctx* ctx, const void* store, int robot, int slot, double* p3, double* q3);

#ifdef __cplusplus
}
#endif
#endif
