/* liw_loop_batch.h — C ABI of the fleet's key-frame sink and laser loop detector on the device: what liw_loop.h does for one
 * robot from host code, for B robots at once and without a host loop over robots.  Per frame the key frames of the robots whose
 * `key` byte is set (the key / pose / acc / n_acc tensors of FleetTracker.step) are appended to a per-robot store, each gets its
 * sub-map feature (spawn_laser_map_feature, the de-duplication and the descriptors of keyframe_manager.cpp:898-1032), and
 * liw_floop_detect runs laser_loop_detect (:642-712) for the newest key frame of each of them.  The single-robot detector of
 * liw_loop.h is the checker: the fleet makes the decisions of B independent liw_loop instances fed the same key frames, with
 * every deliberate difference from the reference that liw_loop.h lists (splitmix64 draws, first bin of a tie, (dij, j) order,
 * closed-form planar ICP, max_points).  Every fleet key frame is a laser key frame.
 *
 * Conventions as liw_laser_batch.h:
 *   - the caller owns all device memory: the store (sized by liw_floop_store_bytes) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no call synchronises or reads back
 *     (liw_floop_detect included: its grids are fixed and stride over work counts that stay on the device); the getters at the
 *     end are synchronous copies for tests and tools;
 *   - every stage takes a `mask` [B] uint8 (NULL = all): of a masked-out robot no byte of the store's robot region or of an
 *     output array is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device liw_floop_create still returns a ctx, but every compute entry returns
 *     LIW_ENODEV.  liw_floop_store_bytes and liw_floop_layout are host-only and work anywhere.
 * The store has a region per robot followed by a scratch area that add_keyframes and detect share (candidate pairs, match results,
 * correspondence lists): two calls on one store must not overlap on different streams.  A fresh store must be reset once.
 *
 * The robot region (liw_floop_layout_info::robot_bytes; all offsets 256-byte aligned), with K = max_keyframes, P = max_points,
 * C = max_kf_corners, S = submap_count, s = S / 3 + 1 (the stride of liw_loop_detect's candidate loop), W the quick_des words:
 *   header            256 B    key-frame count, the `full` flag
 *   tf12              96 K     tracking pose of every key frame, make_tf(pose)
 *   state, n_points   8 K
 *   corner ring       24 S C   the corner lists of the last S key frames (slot k % S), with their counts
 *   feature slots     (ceil(K / s) + 1) x (24 P + 12 P^2 + 8 P W):  points, sorted (dij << 12 | j) keys, aij, quick_des
 * Descriptors are kept only where they can ever be read: key frame k is a candidate only when k % s == 0 (slot k / s), and one
 * more slot holds the newest key frame when it is not such a k.  That is about s times smaller than the K (12 P^2 + 8 P W) bytes of
 * liw_loop_store_bytes: at the office parameters (S = 30, s = 11, W = 53), K = 1 024, P = 256, C = 64 a robot takes 85.8 MB
 * (liw_loop_store_bytes: 929 MB), and 1 024 robots 89 GB with the scratch area, which adds about ceil(K / s) (48 P + 200) bytes per
 * robot (1.2 MB here).
 *
 * Differences from B liw_loop instances, all visible in liw_floop_status:
 *   - a key frame with more than max_kf_corners corners (or more than corner_stride) is not stored; every sub-map that contains
 *     it has state LIW_FLOOP_OVER_CORNERS with n_points 0: invalid, never a query or a candidate;
 *   - an over-cap sub-map (LIW_LOOP_OVER_CAP) reports n_points = max_points + 1 however many points it has;
 *   - liw_floop_get_points / _get_row serve only the key frames whose feature is held: k % s == 0, or the newest;
 *   - the poses are (p, rotation vector q); tf12 = make_tf(p, q) with sin / cos evaluated correctly rounded (liw_crmath.hpp), which
 *     is what the host libm returns for all but about 0.1 % of the arguments, so origins agree bit for bit with liw_lie_make_tf then;
 *   - the ICP's atan2 / sin / cos and log_SE3's atan2 are the correctly rounded ones too: tf12 of an edge agrees with the host's to
 *     round-off, and a gate can differ only where a quantity is within round-off of its threshold.
 * Kernels are compiled without FMA contraction: de-duplicated points, dij, keys and quick_des are bit-identical to liw_loop's, and
 * aij is too (same device acos, same operations).  No atomic decides a position or a result: compaction is by prefix counts in
 * robot-then-candidate order, and two robots with equal key frames give equal results (every robot draws with params.seed).
 *
 * Limits (LIW_EINVAL otherwise): those of liw_loop.h on params, max_points <= 1024 (the de-duplication keeps max_points + 1 points
 * in LDS), B, max_keyframes, max_kf_corners >= 1.
 */
#ifndef LIW_LOOP_BATCH_H
#define LIW_LOOP_BATCH_H
#include <stddef.h>

#include "liw_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more liw_loop_status state: the sub-map contains a key frame with more than max_kf_corners corners */
#define LIW_FLOOP_OVER_CORNERS 4

typedef struct liw_floop_dims {
    int B;                /* robots */
    int max_keyframes;    /* key frames per robot */
    int max_points;       /* points per sub-map, at most 1024; a larger sub-map is invalid */
    int max_kf_corners;   /* most corners of one key frame the store holds */
} liw_floop_dims;

typedef struct liw_floop_layout_info {
    size_t bytes;            /* whole store = B * robot_bytes + scratch_bytes */
    size_t robot_bytes;      /* region of one robot; robot b starts at b * robot_bytes */
    size_t scratch_off;      /* = B * robot_bytes */
    size_t scratch_bytes;
    size_t feature_bytes;    /* one feature slot: points + keys + aij + quick_des */
    int feature_slots;       /* per robot: ceil(max_keyframes / stride) + 1 */
    int stride;              /* s = submap_count / 3 + 1 */
    int quick_words;         /* W */
} liw_floop_layout_info;

typedef struct liw_floop_ctx liw_floop_ctx;

/* bytes of the store for (params, dims); LIW_EINVAL for bad params or dims.  Host-only. */
int liw_floop_store_bytes(const liw_loop_params* params, const liw_floop_dims* dims, size_t* bytes);
/* the same with the sizes of the parts.  Host-only. */
int liw_floop_layout(const liw_loop_params* params, const liw_floop_dims* dims, liw_floop_layout_info* out);

/* a ctx bound to the loop parameters, dims and T_imu_to_wheel (4x4 row-major, loaded as liw_lie_from_matrix16 does with
 * `normalize_extrinsics`); device = HIP device ordinal.  NULL only on a bad argument. */
liw_floop_ctx* liw_floop_create(const liw_loop_params* params, const liw_floop_dims* dims, const double* T_imu_to_wheel16,
                                int normalize_extrinsics, int device);
void liw_floop_destroy(liw_floop_ctx* ctx);
const char* liw_floop_last_error(liw_floop_ctx* ctx);

/* no key frames and `full` clear for the robots with mask[b] != 0 (all when NULL).  LIW_EINVAL: a null or misaligned (8) store. */
int liw_floop_reset(liw_floop_ctx* ctx, void* store, const unsigned char* mask, void* stream);

/* For every robot with key[b] != 0 (and mask): append a key frame with tracking pose make_tf(pose[b]) (pose [B][6] = p, rotation
 * vector q) and the world-frame corners corners[b][0 .. n_corners[b]) (corners [B][corner_stride][3], n_corners [B] int32; a
 * negative count reads as 0), and build its sub-map feature: newest key frame first, origin = the key frame's own pose (identity
 * when submap_count == 1), de-duplication in the reference's serial order, descriptors.  These are the key, pose, acc and n_acc
 * tensors FleetTracker.step returns, with corner_stride = acc_cap.  A robot that already holds max_keyframes gets its `full` flag
 * set and nothing else of it changes.  added [B] uint8 (may be NULL): 1 for a robot whose key frame was stored, 0 for one with key
 * clear or full; it is the `key` argument liw_floop_detect wants for this frame.  Mapping: a wavefront per robot gathers and
 * de-duplicates (lanes over the kept points in LDS, a ballot per corner, the first hit blended if it is within d_res / 2), then a
 * wave per (robot, point) describes.
 * LIW_EINVAL: a null store / key / pose / corners / n_corners, corner_stride < 1, a misaligned store. */
int liw_floop_add_keyframes(liw_floop_ctx* ctx, void* store, const unsigned char* key, const double* pose, const double* corners,
                            int corner_stride, const int* n_corners, const unsigned char* mask, unsigned char* added, void* stream);

/* laser_loop_detect for the newest key frame of every robot with key[b] != 0 (and mask), exactly as liw_loop_detect: the
 * K < min_interval exit, candidates i = 0, s, ... < K - min_interval, the null / points / origin-distance gates, the draws, match and
 * select, then for every candidate above the threshold the ICP over its correspondence list in list order, the T_imu_to_wheel
 * conjugation and the tf gate; the edge is the lowest-index candidate that passes.  Outputs, per robot with key set:
 *   found [B] uint8; edge [B][3] int32 = index1, index2, size (-1, -1, 0 when not found); tf12 [B][12] (written only when found);
 *   stats [B][6] int64 = candidates, launched, tasks, quick_pass, accepted, icp_checked as liw_loop_stats.
 * A robot with key clear gets found = 0 and nothing else of it is written.  A full robot keeps its key frames, so the caller passes
 * liw_floop_add_keyframes' `added` as key if it wants no detection for a key frame that was not stored (FleetLoopDetector.push does).
 * No read-back: the match grid is fixed and strides over the compacted (robot, candidate, draw, 16-row) items.
 * LIW_EINVAL: a null store / key / found / edge / tf12 / stats, a misaligned store. */
int liw_floop_detect(liw_floop_ctx* ctx, void* store, const unsigned char* key, const unsigned char* mask, unsigned char* found,
                     int* edge, double* tf12, long long* stats, void* stream);

/* ---- test and inspection hooks (synchronous device -> host copies).  LIW_EINVAL: robot outside 0 .. B-1, a null store. */
int liw_floop_num_keyframes(liw_floop_ctx* ctx, const void* store, int robot);
/* 1 once an add_keyframes found the robot holding max_keyframes */
int liw_floop_full(liw_floop_ctx* ctx, const void* store, int robot);
/* state of key frame k's feature (LIW_LOOP_* or LIW_FLOOP_OVER_CORNERS); n_points, origin12 and tf12 may be NULL */
int liw_floop_status(liw_floop_ctx* ctx, const void* store, int robot, int k, int* n_points, double* origin12, double* tf12);
/* the de-duplicated points [n][3] of key frame k (a candidate slot, k % s == 0, or the newest; LIW_EINVAL otherwise or when the
 * feature is not valid); at most cap are written; returns n */
int liw_floop_get_points(liw_floop_ctx* ctx, const void* store, int robot, int k, int cap, double* points);
/* row i of key frame k's descriptors as liw_loop_get_row; returns n - 1 */
int liw_floop_get_row(liw_floop_ctx* ctx, const void* store, int robot, int k, int i, int cap, int* dij, int* j, double* aij,
                      unsigned long long* quick_des);

#ifdef __cplusplus
}
#endif
#endif
