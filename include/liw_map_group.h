/* liw_map_group.h — C ABI of the shared occupancy-grid map of a GROUP of fleet robots: robots of a fleet that work in one building
 * get one grid in one frame, where liw_map_batch.h gives each its own.  A group's grid is exactly the grid of liw_map.h over the
 * concatenation of its members' sub-maps, sub-map k of member b placed by T_g_l[b][k] = T_g_w[b] * T_w_l[b][k]: T_w_l is the robot's
 * own world <- laser transform of liw_fmap_render_tf / liw_fmap_render, T_g_w one rigid transform per robot from its world frame
 * into the group's.  A wall cell seen once by each of two members is 100 in the group's grid (50 in either robot's own); box, cell
 * phase and counts are those of the union.  The group's grid, info and counts equal those of ONE liw_map handle fed the members'
 * sub-maps in (robot, sub-map) order with T_g_l; the kernels run the instructions of the fleet map per ray and per cell.
 *
 * The sub-maps stay in the fleet map's store (liw_map_batch.h), where liw_fmap_add_keyframes put them; the grids live in a store of
 * their own, a region per group.  Conventions as liw_map_batch.h:
 *   - the caller owns all device memory: both stores (the group store is sized by liw_gmap_store_bytes) and every array;
 *   - every launch goes on the caller's `stream` (a hipStream_t; NULL = the null stream); no compute call synchronises or reads
 *     back; the getters at the end are synchronous copies for tests and tools;
 *   - gmask / gsel [G] uint8 (NULL = all): of a group that is not selected no byte of its region or of its output rows is written;
 *   - calls return >= 0 on success and a negative LIW_E* code otherwise; nothing is written on LIW_EINVAL;
 *   - there is NO CPU fallback: without a gfx950 device every compute entry returns LIW_ENODEV.  liw_gmap_store_bytes and
 *     liw_gmap_layout are host-only and work anywhere.
 * Both stores are 8-byte aligned.  A fresh group store must be reset once.  Two calls that share a store must not overlap on
 * different streams; a group render and a liw_fmap_render of the same fleet-map store share it.
 *
 * The group region (liw_gmap_layout_info::group_bytes; parts 256-byte aligned), C = max_cells rounded up to 16:
 *   header     256 B   int32 [0] status of the last render (LIW_FMAP_*), [1] member robots and [2] sub-maps used by the last render;
 *                      bytes 32..111 the held liw_map_info (the grid of the last render with status OK or EMPTY)
 *   cell bits  C       SAMPLED 1, HIT1 2, HIT2 4
 *   grid       C       -1 / 0 / 50 / 100, row-major [height][width]
 * Nothing that depends on the arrival order, on B, on the members' robot indices or on their order lives in the region: two groups
 * whose members hold equal sub-maps and transforms hold equal bytes.
 *
 * What a render writes in the fleet map's store: of every member of a selected group the `tf` part (T_g_l), the `partials` part
 * and the header word that counts the composed transforms, all three scratch of liw_fmap_render; so liw_fmap_get_tf returns T_g_l
 * after a group render.  The members' sub-maps, `full`, status, held info, cell bits and grid do not change, and of a robot in no
 * selected group no byte changes.
 */
#ifndef LIW_MAP_GROUP_H
#define LIW_MAP_GROUP_H
#include <stddef.h>

#include "liw_map_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_gmap_dims {
    int G;                /* groups */
    int max_cells;        /* width * height of one group's largest grid */
} liw_gmap_dims;

typedef struct liw_gmap_layout_info {
    size_t bytes;            /* whole store = G * group_bytes */
    size_t group_bytes;      /* region of one group; group g starts at g * group_bytes */
    size_t cell_bytes;       /* max_cells rounded up to 16: the cell bits, and the grid */
    size_t bits_off, grid_off;   /* parts within a group region */
    int cell_chunks;         /* work-groups per group of the clear and finish kernels */
} liw_gmap_layout_info;

typedef struct liw_gmap_ctx liw_gmap_ctx;

/* bytes of the group store; LIW_EINVAL for G < 1, max_cells < 1 or max_cells > 2^31 - 16.  Host-only. */
int liw_gmap_store_bytes(const liw_gmap_dims* dims, size_t* bytes);
/* the same with the sizes and offsets of the parts.  Host-only. */
int liw_gmap_layout(const liw_gmap_dims* dims, liw_gmap_layout_info* out);

/* a ctx for G groups over the robots of `fleet`.  It takes from the fleet-map ctx the resolution, max_steps (the step table in the
 * shared tail of the fleet map's store is read in place, so that store must have been reset), T_imu_to_laser, B, max_submaps,
 * max_points and the device; they are copied, and `fleet` may be destroyed first.  NULL only on a bad argument. */
liw_gmap_ctx* liw_gmap_create(const liw_fmap_ctx* fleet, const liw_gmap_dims* dims);
void liw_gmap_destroy(liw_gmap_ctx* ctx);
const char* liw_gmap_last_error(liw_gmap_ctx* ctx);

/* a held grid of 0 x 0, status LIW_FMAP_EMPTY and zero counters for the groups with gmask[g] != 0 (all when NULL).
 * LIW_EINVAL: a null or misaligned (8) gstore. */
int liw_gmap_reset(liw_gmap_ctx* ctx, void* gstore, const unsigned char* gmask, void* stream);

/* Render the grid of every group with gsel[g] != 0 (all when NULL).  `store` is the fleet map's store, `gstore` the group store.
 * group_of [B] int32: the group of robot b; a value outside 0 .. G-1 (-1, say) means "in no group".  T_w_l as for liw_fmap_render_tf:
 * the transform of robot b's sub-map k is at T_w_l + b * robot_stride + 12 k (in doubles).  T_g_w [B][12] (R row-major 9, then t), or
 * NULL: then T_g_l is T_w_l bit for bit (no product with an identity).  Otherwise T_g_l = T_g_w[b] * T_w_l[b][k] with the product and
 * sum order of liw_lie_mul and no FMA contraction.  gstatus [G] int32 and ginfo [G] liw_map_info get a row per selected group:
 *   LIW_FMAP_OK             the grid is rebuilt; info is what liw_map_render_tf reports for the concatenation;
 *   LIW_FMAP_EMPTY          no member, or no valid point: the group holds a 0 x 0 grid, info says so;
 *   LIW_FMAP_OVER_CELLS,    the info row carries width, height, origin and rays (the other counts 0); the group's held grid and
 *   LIW_FMAP_RAY_TOO_LONG   held info stay as the last OK / EMPTY render left them.
 * The capacities are the group's max_cells and the fleet map's max_steps.  group_of, T_g_w, gsel, gstatus and ginfo must stay valid
 * until the work on `stream` has run.
 * LIW_EINVAL: a null store / gstore / T_w_l / group_of / gstatus / ginfo, robot_stride < 0, a misaligned store or gstore. */
int liw_gmap_render_tf(liw_gmap_ctx* ctx, void* store, void* gstore, const double* T_w_l, long long robot_stride, const int* group_of,
                       const double* T_g_w, const unsigned char* gsel, int* gstatus, liw_map_info* ginfo, void* stream);
/* The same from the IMU poses (p, rotation vector q), 6 doubles per key frame, that of robot b's key frame k at poses + b *
 * robot_stride + 6 k.  T_w_l = make_tf(p, q) * T_imu_to_laser is composed exactly as liw_fmap_render composes it, so with
 * liw_fpg_pose_offset a liw_posegraph_batch.h store is read in place. */
int liw_gmap_render(liw_gmap_ctx* ctx, void* store, void* gstore, const double* poses, long long robot_stride, const int* group_of,
                    const double* T_g_w, const unsigned char* gsel, int* gstatus, liw_map_info* ginfo, void* stream);

/* ---- test and inspection hooks (synchronous device -> host copies).  LIW_EINVAL: group outside 0 .. G-1, a null gstore. */
/* info of the grid the group holds and the status of its last render (either may be NULL) */
int liw_gmap_last_info(liw_gmap_ctx* ctx, const void* gstore, int group, liw_map_info* info, int* status);
/* member robots and sub-maps used by the group's last render (either may be NULL) */
int liw_gmap_members(liw_gmap_ctx* ctx, const void* gstore, int group, int* robots, int* submaps);
/* the held grid, row-major [height][width]; at most cap cells are written.  Returns width * height. */
long long liw_gmap_get(liw_gmap_ctx* ctx, const void* gstore, int group, signed char* out, long long cap);
/* the same grid as a device pointer into the group store: pure pointer arithmetic, NULL on a bad argument */
const signed char* liw_gmap_device_data(liw_gmap_ctx* ctx, const void* gstore, int group);
/* <path_stem>.pgm / .yaml of the held grid through liw_map_write_pgm_grid */
int liw_gmap_write_pgm(liw_gmap_ctx* ctx, const void* gstore, int group, const char* path_stem, const unsigned char* palette4);

#ifdef __cplusplus
}
#endif
#endif
