/* liw_map_locate.h — C ABI of the localisation of fleet robots in a HELD occupancy grid: a robot that was reset inside a mapped
 * building, one that joins a group which has mapped the floor already, or an operator's rough start pose get a pose in a grid of
 * liw_map_batch.h (a robot's) or liw_map_group.h (a group's) without key frames, sub-maps or a descriptor loop of their own.  The
 * method is the whole-cell correlative scan match (Olson 2009): the scan is rotated once per candidate angle and put into cells,
 * translations are whole-cell shifts, and the score of a candidate is a sum of small integers read from a dilated occupancy field.
 * Everything the device decides is integer arithmetic on cells; the cells come from + - * / floor in IEEE double with every
 * operation rounded on its own (no FMA contraction), and the angle table comes from the caller.  So a result is defined bit for
 * bit by the text below (tests/map_locate_cases.py restates it in numpy); there is no tolerance.
 *
 * Conventions as liw_map_batch.h and liw_map_group.h:
 *   - the caller owns all device memory: the store (sized by liw_floc_store_bytes) and every input / output array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no compute call synchronises or reads
 *     back; the getters at the end are synchronous copies for tests and tools;
 *   - msel [M] / mask [Q] uint8 (NULL = all): of a map or a query row that is not selected no byte of its region, of its scratch
 *     or of its output rows is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device liw_floc_create still returns a ctx, but every compute entry returns
 *     LIW_ENODEV.  liw_floc_store_bytes and liw_floc_layout are host-only and work anywhere.
 * The store is 8-byte aligned.  Every map region must have been built once (liw_floc_build; src_of[m] = -1 gives an EMPTY one)
 * before a match reads it.  Two calls on one store must not overlap on different streams.
 *
 * The store (liw_floc_layout_info; parts 256-byte aligned), C = max_cells rounded up to 16:
 *   M map regions of map_bytes each, map m at m * map_bytes:
 *     header   256 B   int32 [0] status of the last build (LIW_FLOC_FIELD_*), [1] occupied cells (field 2), [2] near cells (field 1);
 *                      bytes 32..111 the liw_map_info copied from the source (all zero when src_of[m] < 0)
 *     field    C       one byte per cell, row-major [height][width]: 2 / 1 / 0
 *   Q rows of row_bytes each behind them (partial_off): max_theta records of 8 int32, the scratch of a match: best score of the
 *     angle, its ix, its iy, candidates holding that score, n_valid, 0, 0, 0.
 * Nothing that depends on the arrival order lives in the store: equal sources and equal queries leave equal bytes.
 *
 * The field of a grid (int8 [height][width], -1 / 0 / 50 / 100):
 *   field = 2 where grid >= 50
 *           1 where any of the 8 neighbours inside the grid is >= 50
 *           0 elsewhere
 * With the plain grid instead, a scan of noisy ranges scores a fraction of its points and the best-to-second margin is a few
 * units; the one-cell dilation is part of the definition.
 *
 * The match of query q (scan points[q][0 .. n), n = n_points[q] clamped to 0 .. point_stride; prior T0[q] = (R row-major 9, t),
 * map <- laser; map m = map_of[q] with held info width, height, res = resolution, origin_x, origin_y).  Every product, sum and
 * quotient is rounded on its own:
 *   1. Qx = (R00 x + R01 y) + R02 z,  Qy = (R10 x + R11 y) + R12 z.  A point is valid iff Qx and Qy are finite and at most 1e6 in
 *      magnitude; n_valid counts the valid points (it does not depend on the angle).
 *   2. for angle j with (c, s) = table[j]:  U = c Qx - s Qy,  V = s Qx + c Qy,
 *      qx = ((U + t0x) - origin_x) / res,  qy = ((V + t0y) - origin_y) / res,  cx = floor(qx),  cy = floor(qy).
 *      floor, not the map's truncation toward zero: the two differ only for quotients in (-1, 0), which no point of the map has.
 *      A point whose floors do not lie in [-32, width + 32) x [-32, height + 32) contributes to no candidate of that angle.
 *   3. score(j, iy, ix) = sum over the valid points of field[cy + iy][cx + ix], a cell outside the grid counting 0, for the
 *      shifts ix, iy in [-W, W].
 *   4. the best candidate has the largest score; ties go to the smallest ix^2 + iy^2, then the smallest |j - (n_theta - 1) / 2|
 *      (integer division), then the lowest j, the lowest iy, the lowest ix.  `ties` = candidates holding the best score.
 * The definition is the exhaustive maximum over all n_theta (2 W + 1)^2 candidates.
 * Outputs of a row:  best = (j, ix, iy, score);  stats = (status, n_valid, ties, 0);
 *   found = status is LIW_FLOC_OK and score * 1000 >= min_permille * 2 * n_valid (64-bit integers);
 *   T_m_l: rows 0 and 1 of R are  c R0[0][e] - s R0[1][e]  and  s R0[0][e] + c R0[1][e]  (e = 0, 1, 2), row 2 is R0's row 2 bit
 *   for bit, t = (t0x + (double)ix * res, t0y + (double)iy * res, t0z).
 * The status, the first that applies:
 *   LIW_FLOC_NO_MAP      map_of[q] outside 0 .. M-1, or the field's status is not LIW_FLOC_FIELD_OK
 *   LIW_FLOC_BAD_PRIOR   an entry of T0 is not finite, or a component of t0 exceeds 1e6 in magnitude
 *   LIW_FLOC_NO_POINTS   n_valid == 0
 *   LIW_FLOC_OK
 * On any status other than OK: best is all zero, stats = (status, 0, 0, 0), T_m_l = T0 bit for bit and found = 0.
 *
 * Limits (LIW_EINVAL otherwise): Q, M, max_cells >= 1, max_cells at most 2^31 - 16, 1 <= max_theta <= 256.
 */
#ifndef LIW_MAP_LOCATE_H
#define LIW_MAP_LOCATE_H
#include <stddef.h>

#include "liw_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a map region's field */
#define LIW_FLOC_FIELD_OK 0
#define LIW_FLOC_FIELD_EMPTY 1    /* no source (src_of < 0), or a source grid of 0 x 0 */
#define LIW_FLOC_FIELD_OVER 2     /* width * height > max_cells: the region holds no field */

/* status of a query row */
#define LIW_FLOC_OK 0
#define LIW_FLOC_NO_MAP 1
#define LIW_FLOC_NO_POINTS 2
#define LIW_FLOC_BAD_PRIOR 3

#define LIW_FLOC_MAX_W 31             /* largest window half-width, in cells */
#define LIW_FLOC_MAX_THETA 256        /* largest angle table */
#define LIW_FLOC_MAX_STRIDE 1048576   /* largest point_stride: a score fits 32 bits with room */

typedef struct liw_floc_dims {
    int Q;                /* query rows: (scan, prior) pairs, not necessarily one per robot */
    int M;                /* map regions */
    int max_cells;        /* width * height of the largest field */
    int max_theta;        /* angles of the largest table, at most 256 */
} liw_floc_dims;

typedef struct liw_floc_layout_info {
    size_t bytes;            /* whole store = M * map_bytes + Q * row_bytes */
    size_t map_bytes;        /* region of one map; map m starts at m * map_bytes */
    size_t field_bytes;      /* max_cells rounded up to 16 */
    size_t field_off;        /* the field within a map region */
    size_t partial_off;      /* = M * map_bytes: the rows of partial records */
    size_t row_bytes;        /* the records of one query: 32 * max_theta, 256-byte aligned */
    int cell_chunks;         /* work-groups per map of the field kernel */
} liw_floc_layout_info;

typedef struct liw_floc_ctx liw_floc_ctx;

/* bytes of the store; LIW_EINVAL for dims outside the limits.  Host-only. */
int liw_floc_store_bytes(const liw_floc_dims* dims, size_t* bytes);
/* the same with the sizes and offsets of the parts.  Host-only. */
int liw_floc_layout(const liw_floc_dims* dims, liw_floc_layout_info* out);

/* a ctx bound to the dims and T_imu_to_laser (4x4 row-major, loaded as liw_lie_from_matrix16 does with `normalize_extrinsics`;
 * only liw_floc_link_tf uses it); device = HIP device ordinal.  NULL only on a bad argument. */
liw_floc_ctx* liw_floc_create(const liw_floc_dims* dims, const double* T_imu_to_laser16, int normalize_extrinsics, int device);
void liw_floc_destroy(liw_floc_ctx* ctx);
const char* liw_floc_last_error(liw_floc_ctx* ctx);

/* Grid to field, for every map m with msel[m] != 0 (all when NULL).  The source of map m is the region src_store + src_of[m] *
 * region_bytes: its held liw_map_info at byte 32 and its grid (int8 [height][width]) at grid_off, the layout liw_map_batch.h
 * (robot_bytes, grid_off) and liw_map_group.h (group_bytes, grid_off) both state; a hand-made region of that shape serves too.
 * The source is only read; the field is a snapshot, and a match never touches the source.  src_of [M] int32:
 *   src_of[m] < 0               LIW_FLOC_FIELD_EMPTY, the info all zero, both counts 0
 *   width <= 0 or height <= 0   LIW_FLOC_FIELD_EMPTY, the info copied, both counts 0
 *   width * height > max_cells  LIW_FLOC_FIELD_OVER, the info copied, both counts 0; no byte of the field is written
 *   else                        LIW_FLOC_FIELD_OK: info, counts, and the field's bytes 0 .. width * height rounded up to 4 (the
 *                               bytes behind the last cell are 0)
 * src_of and msel must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null or misaligned (8) lstore or src_store, a null src_of, region_bytes below 112 or no multiple of 8, grid_off
 * below 112 or not below region_bytes. */
int liw_floc_build(liw_floc_ctx* ctx, void* lstore, const void* src_store, size_t region_bytes, size_t grid_off, const int* src_of,
                   const unsigned char* msel, void* stream);

/* The search, for every query row q with mask[q] != 0 (all when NULL); see the head of this file.  map_of [Q] int32; points
 * [Q][point_stride][3] double, laser frame; n_points [Q] int32 (a negative count reads as 0 and one above point_stride as
 * point_stride, as liw_fmap_add_keyframes reads them); T0 [Q][12]; table [n_theta][2] double (cos, sin), a device array like all
 * the others; found [Q] uint8, best [Q][4] int32, stats [Q][4] int32, T_m_l [Q][12] double.  T_m_l must not alias T0.
 * LIW_EINVAL: a null or misaligned (8) lstore, any other null array but mask, point_stride outside 1 .. LIW_FLOC_MAX_STRIDE,
 * n_theta outside 1 .. max_theta, W outside 0 .. LIW_FLOC_MAX_W, min_permille < 0. */
int liw_floc_match(liw_floc_ctx* ctx, void* lstore, const int* map_of, const double* points, int point_stride, const int* n_points,
                   const double* T0, const double* table, int n_theta, int W, int min_permille, const unsigned char* mask,
                   unsigned char* found, int* best, int* stats, double* T_m_l, void* stream);

/* Hand-over to the group machinery, for every row with found[q] != 0 and mask[q] != 0 (NULL = all); no other row is written.
 * poses: the IMU pose (p, rotation vector q) of row q, 6 doubles at poses + q * robot_stride.
 *   T_w_l [Q][12] = make_tf(p, q) * T_imu_to_laser, composed exactly as liw_fmap_render composes it;
 *   T_g_w [Q][12] = T_m_l[q] * inverse(T_w_l), in the product and sum order of liw_lie_inverse and liw_lie_mul:
 * the row liw_gmap_render takes as T_g_w of that robot.
 * LIW_EINVAL: a null T_m_l / poses / found / T_w_l / T_g_w, robot_stride < 0. */
int liw_floc_link_tf(liw_floc_ctx* ctx, const double* T_m_l, const double* poses, long long robot_stride, const unsigned char* found,
                     const unsigned char* mask, double* T_w_l, double* T_g_w, void* stream);

/* ---- test and inspection hooks (synchronous device -> host copies).  LIW_EINVAL: map outside 0 .. M-1, a null lstore. */
/* the held info, the status of the last build and the two counts of a map region (any pointer may be NULL) */
int liw_floc_field_info(liw_floc_ctx* ctx, const void* lstore, int map, liw_map_info* info, int* status, int* occupied, int* near_cells);
/* the field, row-major [height][width]; at most cap bytes are written.  Returns width * height, 0 unless the status is OK. */
long long liw_floc_get_field(liw_floc_ctx* ctx, const void* lstore, int map, unsigned char* out, long long cap);
/* the same field as a device pointer into the store: pure pointer arithmetic, NULL on a bad argument */
const unsigned char* liw_floc_device_field(liw_floc_ctx* ctx, const void* lstore, int map);

#ifdef __cplusplus
}
#endif
#endif
