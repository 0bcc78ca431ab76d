/* liw_map_batch.h — C ABI of the fleet's occupancy-grid maps on the device: what liw_map.h does for one robot from host code,
 * for B robots at once and without a host loop over robots.  Per frame the de-skewed laser-frame scan of every robot whose `key`
 * byte is set is appended to a per-robot store as a sub-map (sub-map index = key-frame index), and a render rebuilds the grids of
 * the selected robots from one world <- laser transform per sub-map, as a loop-closing solve of liw_posegraph_batch.h moves every
 * pose.  The map is the one liw_map.h defines: the world point and its sum order, the bounding box, width and height, the
 * accumulated step table T, truncation toward zero, the three monotone bits SAMPLED / HIT1 / HIT2 with the values -1 / 0 / 50 / 100,
 * what is ignored (non-finite points) and no FMA contraction anywhere.  The single-robot liw_map_* is the per-robot checker: both
 * run the same instructions per ray (csrc/k_map_dev.hpp), so a fleet robot's grid, info and counts equal those of a liw_map handle
 * fed the same sub-maps and transforms.
 *
 * Conventions as liw_loop_batch.h and liw_posegraph_batch.h:
 *   - the caller owns all device memory: the store (sized by liw_fmap_store_bytes) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no call synchronises or reads back: all
 *     capacity decisions of a render happen on the device; the getters at the end are synchronous copies for tests and tools;
 *   - every stage takes a `mask` / `sel` [B] uint8 (NULL = all): of a masked-out robot no byte of the store's robot region or of an
 *     output row is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device liw_fmap_create still returns a ctx, but every compute entry returns
 *     LIW_ENODEV.  liw_fmap_store_bytes and liw_fmap_layout are host-only and work anywhere.
 * The store is 8-byte aligned.  A fresh store must be reset once.  Two calls on one store must not overlap on different streams.
 *
 * The robot region (liw_fmap_layout_info::robot_bytes; parts 256-byte aligned), K = max_submaps, P = max_points, C = max_cells
 * rounded up to 16:
 *   header       256 B      int32 [0] sub-maps, [1] full, [2] status of the last render, [3] points held, [4] transforms composed by
 *                           the last liw_fmap_render; bytes 32..111 the held liw_map_info (the grid of the last render with
 *                           status OK or EMPTY; its samples / unknown / free_cells / hit_once / hit_more are the counters the
 *                           kernels add into)
 *   offsets      4 (K + 1)  int32: sub-map k holds the points offsets[k] .. offsets[k + 1]
 *   points       24 P       laser frame, x y z
 *   sub-map idx  4 P        per point
 *   tf           96 K       T_w_l of liw_fmap_render (R row-major 9, then t); liw_fmap_render_tf reads the caller's array in place
 *   partials     48 n       n = min(ceil(P / 256), 64) records of min x, max x, min y, max y, longest ray, valid points
 *   cell bits    C          SAMPLED 1, HIT1 2, HIT2 4
 *   grid         C          -1 / 0 / 50 / 100, row-major [height][width]
 * Behind the B robot regions lies the shared tail (liw_fmap_layout_info::shared_off): the step table T [max_steps] doubles, written
 * by every liw_fmap_reset.  The counts liw_map_probe_counts reports (atomics issued, cell visits) depend on the arrival order and
 * have no place in the region: two robots with equal sub-maps and transforms hold equal bytes, whatever B, their index and `sel`.
 *
 * Differences from B liw_map handles: the capacities max_cells and max_steps are checked on the device and reported per robot in
 * `status` (no LIW_ENOMEM / LIW_EINVAL return); liw_fmap_render composes T_w_l on the device with sin / cos evaluated correctly
 * rounded (liw_crmath.hpp), which is what the host libm returns for all but about 0.1 % of the arguments.
 *
 * Limits (LIW_EINVAL otherwise): B, max_submaps, max_points, max_cells >= 1, 4 <= max_steps <= 2^22, max_cells and max_points at
 * most 2^31 - 16, B * max_submaps < 2^31, a positive finite resolution.
 */
#ifndef LIW_MAP_BATCH_H
#define LIW_MAP_BATCH_H
#include <stddef.h>

#include "liw_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a robot's render */
#define LIW_FMAP_OK 0
#define LIW_FMAP_EMPTY 1          /* no valid point: the robot holds a 0 x 0 grid */
#define LIW_FMAP_OVER_CELLS 2     /* width * height > max_cells */
#define LIW_FMAP_RAY_TOO_LONG 3   /* the longest ray has max_steps - 2 steps or more */

typedef struct liw_fmap_dims {
    int B;                /* robots */
    int max_submaps;      /* sub-maps (laser key frames) per robot */
    int max_points;       /* points of all sub-maps of ONE robot */
    int max_cells;        /* width * height of one robot's largest grid */
    int max_steps;        /* step-table entries: the longest ray is below (max_steps - 2) * resolution / 2 */
} liw_fmap_dims;

typedef struct liw_fmap_layout_info {
    size_t bytes;            /* whole store = B * robot_bytes + shared_bytes */
    size_t robot_bytes;      /* region of one robot; robot b starts at b * robot_bytes */
    size_t shared_off;       /* = B * robot_bytes */
    size_t shared_bytes;     /* the step table */
    size_t cell_bytes;       /* max_cells rounded up to 16: the cell bits, and the grid */
    size_t offsets_off, points_off, index_off, tf_off, partial_off, bits_off, grid_off;   /* parts within a robot region */
    int partials;            /* bounds partial records per robot */
} liw_fmap_layout_info;

typedef struct liw_fmap_ctx liw_fmap_ctx;

/* bytes of the store for (params, dims); LIW_EINVAL for bad params or dims.  Host-only. */
int liw_fmap_store_bytes(const liw_map_params* params, const liw_fmap_dims* dims, size_t* bytes);
/* the same with the sizes and offsets of the parts.  Host-only. */
int liw_fmap_layout(const liw_map_params* params, const liw_fmap_dims* dims, liw_fmap_layout_info* out);

/* a ctx bound to the map parameters, dims and T_imu_to_laser (4x4 row-major, loaded as liw_lie_from_matrix16 does with
 * `normalize_extrinsics`); device = HIP device ordinal.  NULL only on a bad argument. */
liw_fmap_ctx* liw_fmap_create(const liw_map_params* params, const liw_fmap_dims* dims, const double* T_imu_to_laser16, int normalize_extrinsics,
                              int device);
void liw_fmap_destroy(liw_fmap_ctx* ctx);
const char* liw_fmap_last_error(liw_fmap_ctx* ctx);

/* no sub-maps, flags clear and a held grid of 0 x 0 for the robots with mask[b] != 0 (all when NULL).  Every reset also (re)writes
 * the step table in the shared tail, T[0] = 0, T[k + 1] = fl(T[k] + resolution / 2): the same values every time.
 * LIW_EINVAL: a null or misaligned (8) store. */
int liw_fmap_reset(liw_fmap_ctx* ctx, void* store, const unsigned char* mask, void* stream);

/* For every robot with key[b] != 0 (and mask): append points[b][0 .. n_points[b]) as sub-map k = the robot's sub-map count (points
 * [B][point_stride][3] double, laser frame; n_points [B] int32, a negative count reads as 0 and one above point_stride as
 * point_stride).  An empty sub-map is stored, so that sub-map index = key-frame index.  A robot that would exceed max_submaps or
 * max_points gets its `full` flag set and nothing else of it changes; `full` is sticky until reset (a later, smaller scan would
 * otherwise be stored under the wrong index).  added [B] uint8 (may be NULL): 1 for a robot whose key frame was stored, 0 for one
 * with key clear or full.  These are FleetTracker.scan_points() and the `added` of liw_fpg_add_keyframes.
 * LIW_EINVAL: a null store / key / points / n_points, point_stride < 1, a misaligned store. */
int liw_fmap_add_keyframes(liw_fmap_ctx* ctx, void* store, const unsigned char* key, const double* points, int point_stride, const int* n_points,
                           const unsigned char* mask, unsigned char* added, void* stream);

/* Render all sub-maps of every robot with sel[b] != 0 (all when NULL).  T_w_l is a device array of world <- laser transforms: that
 * of robot b's sub-map k is at T_w_l + b * robot_stride + 12 k (in doubles); it is read in place.  status [B] int32 and info [B]
 * liw_map_info get a row per selected robot:
 *   LIW_FMAP_OK             the grid is rebuilt; info is what liw_map_render_tf reports;
 *   LIW_FMAP_EMPTY          no valid point (or no sub-map): the robot holds a 0 x 0 grid, info says so;
 *   LIW_FMAP_OVER_CELLS,    the info row carries width, height, origin and rays (the other counts 0); the robot's held grid and
 *   LIW_FMAP_RAY_TOO_LONG   held info stay as the last OK / EMPTY render left them.
 * status and info must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null store / T_w_l / status / info, robot_stride < 0, a misaligned store. */
int liw_fmap_render_tf(liw_fmap_ctx* ctx, void* store, const double* T_w_l, long long robot_stride, const unsigned char* sel, int* status,
                       liw_map_info* info, void* stream);
/* The same from the IMU poses (p, rotation vector q), 6 doubles per key frame: that of robot b's key frame k is at
 * poses + b * robot_stride + 6 k.  T_w_l = make_tf(p, q) * T_imu_to_laser is composed on the device into the robot's region.  With
 * liw_fpg_pose_offset a liw_posegraph_batch.h store is read in place: poses = store + offset, robot_stride = robot_bytes / 8. */
int liw_fmap_render(liw_fmap_ctx* ctx, void* store, const double* poses, long long robot_stride, const unsigned char* sel, int* status,
                    liw_map_info* info, void* stream);

/* ---- test and inspection hooks (synchronous device -> host copies).  LIW_EINVAL: robot outside 0 .. B-1, a null store. */
int liw_fmap_num_submaps(liw_fmap_ctx* ctx, const void* store, int robot);
/* 1 once an add_keyframes found the robot without room */
int liw_fmap_full(liw_fmap_ctx* ctx, const void* store, int robot);
/* the points [n][3] of sub-map k; at most cap are written; returns n */
int liw_fmap_get_submap(liw_fmap_ctx* ctx, const void* store, int robot, int k, int cap, double* points);
/* the transforms [n][12] the last liw_fmap_render composed for the robot; at most cap are written; returns n */
int liw_fmap_get_tf(liw_fmap_ctx* ctx, const void* store, int robot, int cap, double* tf12);
/* info of the grid the robot holds and the status of its last render (either may be NULL) */
int liw_fmap_last_info(liw_fmap_ctx* ctx, const void* store, int robot, liw_map_info* info, int* status);
/* the held grid, row-major [height][width]; at most cap cells are written.  Returns width * height. */
long long liw_fmap_get(liw_fmap_ctx* ctx, const void* store, int robot, signed char* out, long long cap);
/* the same grid as a device pointer into the store: pure pointer arithmetic, NULL on a bad argument */
const signed char* liw_fmap_device_data(liw_fmap_ctx* ctx, const void* store, int robot);
/* <path_stem>.pgm / .yaml of the held grid through liw_map_write_pgm_grid */
int liw_fmap_write_pgm(liw_fmap_ctx* ctx, const void* store, int robot, const char* path_stem, const unsigned char* palette4);

#ifdef __cplusplus
}
#endif
#endif
