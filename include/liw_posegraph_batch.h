/* liw_posegraph_batch.h — C ABI of the fleet's pose-graph back-end on the device: B instances of keyframe_manager (key-frame queue,
 * sequential and loop edges, solve, map-frame correction; mirror include/lvio_2d_keyframe_manager.hpp, reference
 * src/trajectory/keyframe_manager.cpp:408-482, :722-838) without a host loop over robots.  It consumes what liw_loop_batch.h produces:
 * the key / pose tensors of a tracking frame and found / edge / tf12 of liw_floop_detect.  liw_posegraph_solve of liw_posegraph.h (one
 * graph per call, LM bookkeeping on the host) is the per-robot checker: the fleet solves the same linear system per iteration and
 * takes the same trust-region decisions (liw_lm_rules.hpp), all robots in lock-step, each with its own radius and termination.
 *
 * Conventions as liw_loop_batch.h:
 *   - the caller owns all device memory: the store (sized by liw_fpg_store_bytes) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no call synchronises or reads back unless it
 *     says so (liw_fpg_solve with check_every > 0, the getters and liw_fpg_load_graph at the end);
 *   - every stage takes a `mask` [B] uint8 (NULL = all; liw_fpg_solve: `sel`, required): of a masked-out robot no byte of the store's
 *     robot region or of an output row is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device liw_fpg_create still returns a ctx, but every compute entry returns LIW_ENODEV.
 *     liw_fpg_store_bytes and liw_fpg_layout are host-only and work anywhere.
 * No atomic decides a position or a value (one atomic OR raises a robot's "pivot not positive" flag): sums run in a fixed order
 * that depends on the robot's own graph only, so two robots with equal inputs give equal bytes, whatever B and their index.
 * A fresh store must be reset once.  Two calls on one store must not overlap on different streams.
 *
 * The robot region (liw_fpg_layout_info::robot_bytes; parts 256-byte aligned), K = max_keyframes, L = max_loops:
 *   header      256 B   int32 [0] key frames, [1] loops, [2] full, [3] loops_full, [4] bad_edge, [5] has_loop_wait_for_solve, [6] solves;
 *                       double at byte 32 last_solve_time (-1e300 after reset), bytes 40..135 modify_delta_tf[12] (identity after
 *                       reset), bytes 136..167 the liw_summary of the robot's last solve
 *   stamp       8 K     time of every key frame
 *   tf12        96 K    tfs_tracking: make_tf(pose) as it was added (R row-major 9, then t)
 *   pose        48 K    the corrected pose p, q (rotation vector): log_SE3(modify_delta_tf * tf) when added, replaced by a solve
 *   seq edge    96 K    entry k: tf[k-1]^-1 * tf[k], the sequential edge (k-1, k); entry 0 is unused
 *   loop index  8 L     index1, index2 (int32)
 *   loop tf12   96 L
 * Behind the B robot regions lies the solver's work area (liw_fpg_layout_info::work_bytes = B * work_robot_bytes + 256): per robot
 * the LM state, x, candidate, step, Jacobi scale, LM diagonal (48 K each), the edge and ground blocks Y (624 (K - 1 + L) + 112 K),
 * the assembled 6x6 blocks and gradient (624 K + 288 L), the separator list, the segment records and Schur terms (624 K + 960 S) and
 * the packed lower triangle of the separator system (8 * 3 S (6 S + 1)), with S = min(K, ceil(K / 48) + 1 + 2 L) separators at most.
 * At K = 200, L = 5 a robot takes 50 944 B of region and 505 088 B of work area (S = 16): 569 MB for 1 024 robots.
 *
 * Differences from B host mirrors, all to round-off: sin / cos / atan2 of make_tf and log_SE3 are the correctly rounded ones of
 * liw_crmath.hpp; the accepted-step radius update cubes with two multiplications (liw_lm_rules.hpp) where liw_posegraph_solve calls
 * pow(); cost and norm sums run lane-strided with a butterfly; robots of fewer than four key frames take the same segment path as
 * every other robot (liw_posegraph_solve sends them to its dense factorisation).  A selected robot with fewer than two key frames
 * is treated as not selected.
 *
 * Limits (LIW_EINVAL otherwise): B, max_keyframes >= 1, max_loops >= 0, B * (max_keyframes + max_loops) < 2^31 (the grids are over
 * (robot, key frame) and (robot, edge) slots), solve_period finite.
 */
#ifndef LIW_POSEGRAPH_BATCH_H
#define LIW_POSEGRAPH_BATCH_H
#include <stddef.h>

#include "liw_posegraph.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_fpg_dims {
    int B;               /* robots */
    int max_keyframes;   /* key frames per robot */
    int max_loops;       /* loop edges per robot */
} liw_fpg_dims;

typedef struct liw_fpg_layout_info {
    size_t bytes;               /* whole store = B * robot_bytes + work_bytes */
    size_t robot_bytes;         /* region of one robot; robot b starts at b * robot_bytes */
    size_t work_off;            /* = B * robot_bytes */
    size_t work_bytes;
    size_t work_robot_bytes;    /* solver work area of one robot */
    int max_separators;         /* S */
    int edge_slots;             /* K - 1 + L */
} liw_fpg_layout_info;

typedef struct liw_fpg_ctx liw_fpg_ctx;

/* bytes of the store for dims; LIW_EINVAL for bad dims or a null pointer.  Host-only. */
int liw_fpg_store_bytes(const liw_fpg_dims* dims, size_t* bytes);
/* the same with the sizes of the parts.  Host-only. */
int liw_fpg_layout(const liw_fpg_dims* dims, liw_fpg_layout_info* out);
/* byte offset of the corrected-pose part (pose, 48 K) within a robot region, so that a consumer reads the poses in place: robot b's
 * key frame k is at store + b * robot_bytes + *off + 48 k (liw_fmap_render of liw_map_batch.h: poses = store + *off, robot_stride =
 * robot_bytes / 8).  LIW_EINVAL for bad dims or a null pointer.  Host-only. */
int liw_fpg_pose_offset(const liw_fpg_dims* dims, size_t* off);

/* a ctx bound to the solver parameters (extrinsics and ground sigmas are read), the pose-graph parameters, dims and solve_period
 * (seconds of key-frame time between two solves of a robot); device = HIP device ordinal.  NULL only on a bad argument. */
liw_fpg_ctx* liw_fpg_create(const liw_params* params, const liw_pg_params* pg, const liw_fpg_dims* dims, double solve_period, int device);
void liw_fpg_destroy(liw_fpg_ctx* ctx);
const char* liw_fpg_last_error(liw_fpg_ctx* ctx);

/* empty queue, no loops, flags clear, last_solve_time = -1e300, modify_delta_tf = identity for the robots with mask[b] != 0.
 * LIW_EINVAL: a null or misaligned (8) store. */
int liw_fpg_reset(liw_fpg_ctx* ctx, void* store, const unsigned char* mask, void* stream);

/* add_keyframe of the mirror up to the edge, for every robot with key[b] != 0 (and mask): tfs_tracking.push(make_tf(pose[b])) (pose
 * [B][6] = p, rotation vector q), corrected pose = log_SE3(modify_delta_tf * tf), sequential edge = tf[k-1]^-1 * tf[k], stamp[b] (stamp
 * [B] double) kept.  A robot that already holds max_keyframes gets its `full` flag set and nothing else of it changes.  added [B]
 * uint8 (may be NULL): 1 for a robot whose key frame was stored, 0 for one with key clear or full.  A lane per robot.
 * LIW_EINVAL: a null store / key / pose / stamp, a misaligned store. */
int liw_fpg_add_keyframes(liw_fpg_ctx* ctx, void* store, const unsigned char* key, const double* pose, const double* stamp,
                          const unsigned char* mask, unsigned char* added, void* stream);

/* the outputs of liw_floop_detect: for every robot with found[b] != 0 (and mask) append (edge[b][0], edge[b][1], tf12[b]) (edge
 * [B][3] int32, tf12 [B][12]) and set has_loop_wait_for_solve.  An index outside the robot's key frames or index1 == index2 sets
 * bad_edge and stores nothing; a robot already at max_loops sets loops_full and stores nothing.
 * LIW_EINVAL: a null store / found / edge / tf12, a misaligned store. */
int liw_fpg_add_loops(liw_fpg_ctx* ctx, void* store, const unsigned char* found, const int* edge, const double* tf12,
                      const unsigned char* mask, void* stream);

/* is_time_to_solve on key-frame stamps: due[b] = key[b] && has_loop_wait_for_solve && stamp[b] - last_solve_time > solve_period for
 * the robots in mask; n_due = their count, one int32 the caller may place in page-locked host memory (may be NULL).
 * LIW_EINVAL: a null store / key / stamp / due, a misaligned store. */
int liw_fpg_due(liw_fpg_ctx* ctx, void* store, const unsigned char* key, const double* stamp, const unsigned char* mask, unsigned char* due,
                int* n_due, void* stream);

/* keyframe_manager::solve for every robot with sel[b] != 0 and at least two key frames: Levenberg-Marquardt over its key-frame poses
 * (key frame 0 constant), at most max_iters iterations (<= 0: 50), on the device and in lock-step.  Afterwards, per such robot: the
 * corrected poses are replaced, modify_delta_tf = make_tf(p_last, q_last) * tfs_tracking.last^-1, has_loop_wait_for_solve is cleared,
 * last_solve_time = stamp[b], solves is incremented, summary[b] is written (and kept in the header).  Other robots keep their row.
 * check_every <= 0: the launches of all max_iters iterations are enqueued and the call never synchronises (a finished robot's waves
 * exit at once); check_every = n: the count of robots still iterating is read back every n iterations and launching stops at zero.
 * Both give identical bytes.  stamp and summary must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null store / sel / stamp / summary, a misaligned store. */
int liw_fpg_solve(liw_fpg_ctx* ctx, void* store, const unsigned char* sel, const double* stamp, int max_iters, int check_every,
                  liw_summary* summary, void* stream);

/* update_other_frame: pose_out[b] = log_SE3(modify_delta_tf * make_tf(pose_in[b])) (both [B][6]) for the robots in mask.
 * LIW_EINVAL: a null store / pose_in / pose_out, a misaligned store. */
int liw_fpg_correct(liw_fpg_ctx* ctx, void* store, const double* pose_in, double* pose_out, const unsigned char* mask, void* stream);

/* ---- test and inspection hooks.
 * The solver keeps a robot's separator system (3 s (6 s + 1) doubles for s separators) in LDS when it has at most `doubles` entries and
 * in the robot's work area otherwise, with the same instructions and so the same bytes.  Default and maximum 8192 (64 KB); 0 sends every
 * robot to its work area (tests).  Host-only; LIW_EINVAL outside 0 .. 8192. */
int liw_fpg_set_lds_doubles(liw_fpg_ctx* ctx, int doubles);
/* The rest are synchronous copies.  LIW_EINVAL: robot outside 0 .. B-1, a null store. */
int liw_fpg_num_keyframes(liw_fpg_ctx* ctx, const void* store, int robot);
/* flags [6] = loops, full, loops_full, bad_edge, has_loop_wait_for_solve, solves; last_solve_time may be NULL */
int liw_fpg_flags(liw_fpg_ctx* ctx, const void* store, int robot, int* flags6, double* last_solve_time);
/* the first min(n, cap) key frames: poses [.][6] corrected p, q; stamps [.]; tf12 [.][12] tfs_tracking (any may be NULL); returns n */
int liw_fpg_get_keyframes(liw_fpg_ctx* ctx, const void* store, int robot, int cap, double* poses, double* stamps, double* tf12);
/* sequential edges (k, k + 1), k < n - 1: tf12 [.][12]; returns n - 1 (0 for an empty robot) */
int liw_fpg_get_seq_edges(liw_fpg_ctx* ctx, const void* store, int robot, int cap, double* tf12);
/* loop edges: idx [.][2], tf12 [.][12]; returns their number */
int liw_fpg_get_loop_edges(liw_fpg_ctx* ctx, const void* store, int robot, int cap, int* idx, double* tf12);
int liw_fpg_get_modify_delta_tf(liw_fpg_ctx* ctx, const void* store, int robot, double* tf12);
int liw_fpg_get_summary(liw_fpg_ctx* ctx, const void* store, int robot, liw_summary* summary);
/* Replace a robot's graph from host arrays (tests and tools; the robot's flags, solves and modify_delta_tf are reset): poses [N][6]
 * become the corrected poses and tfs_tracking = make_tf(pose) (liw_lie_make_tf), stamps [N] (NULL: 0, 1, ...), seq_tf12 [N-1][12] the
 * sequential edges, n_loop loop edges which set has_loop_wait_for_solve.  LIW_EINVAL: N outside 1 .. max_keyframes, n_loop outside
 * 0 .. max_loops, a loop index outside the key frames, a null array. */
int liw_fpg_load_graph(liw_fpg_ctx* ctx, void* store, int robot, int N, const double* poses, const double* stamps, const double* seq_tf12,
                       int n_loop, const int* loop_idx, const double* loop_tf12);

#ifdef __cplusplus
}
#endif
#endif
