/* liw_map.h — C ABI of the occupancy-grid map of the back-end's laser key frames (the reference's
 * keyframe_manager::show_laser_map, src/trajectory/keyframe_manager.cpp:483-511, rendered by
 * visualization::do_laser_map_to_show / update_occupancy_grid, src/utilies/visualization.cpp:369-451 and :33-75).
 *
 * The map holds sub-maps: the laser-frame points [n][3] of one key frame each, uploaded once and kept on the device.  A render
 * takes one world <- laser transform T_w_l per sub-map and rebuilds the whole grid from them (a pose-graph solve moves every
 * pose).  The definition, in IEEE double with every product, sum, quotient and square root rounded on its own:
 *   1. world point P_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i for i = 0, 1, 2;
 *   2. bounding box of all P in x and y; width = int((max_x - min_x) / res + 1), height likewise, origin (min_x, min_y), every
 *      cell -1;
 *   3. per point a ray from the emit origin O = t to P: d = P - O, len = sqrt((dx dx + dy dy) + dz dz), unit = d / len (a
 *      division per component), step = res / 2, and for (tr = 0; tr <= len; tr += step) the sample C = O + unit tr.  The cell
 *      of a point C is x = int((C_x - origin_x) / res), y likewise: a division, and a conversion that truncates toward zero, so
 *      a quotient in (-1, 0) lands in column / row 0 and counts as inside; a cell outside [0, width) x [0, height) is skipped.
 *      A sampled cell holding -1 becomes 0.  Then the cell of P itself: -1 or 0 becomes 50, anything else 100.
 * tr is the ACCUMULATED sum (tr_k != k step from k = 6 on at res = 0.05); it depends on step alone, so the table
 * T[0] = 0, T[k + 1] = fl(T[k] + step) (liw_map_step_table) serves every ray.  The result does not depend on the order of the
 * rays: a cell ends as 100 with two or more hits, 50 with exactly one, 0 with none but at least one sample, -1 otherwise.  The
 * kernels keep three monotone bits per cell and set them with integer OR, so a render is deterministic and equal cell for cell
 * to the serial walk (tests/map_reference.py, tests/cpp/map_serial.cpp).
 *
 * Defined here, undefined in the reference: a point whose world coordinates or ray length are not finite is ignored (no
 * bounds, no ray); a ray of length 0 marks only its target cell (no sample); no valid point at all gives a 0 x 0 map.
 * A ray of more than 2^22 - 3 steps (about 100 km at 5 cm) is rejected with LIW_EINVAL.
 *
 * Conventions as in liw_loop.h: the handle is bound to a liw_ctx (device, T_imu_to_laser); the library owns the device store
 * (sized by liw_map_store_bytes) and the step table next to it; calls return >= 0 on success and a negative LIW_E* code
 * otherwise.  There is NO CPU fallback: without a gfx950 device liw_map_create still returns a handle, but every compute entry
 * returns LIW_ENODEV.  liw_map_store_bytes, liw_map_step_table and liw_map_write_pgm_grid are host-only and work anywhere.
 * A transform T12 is R (9, row-major) then t (3), as in liw_lie.h.  liw_map_render composes make_tf(p, q) * T_imu_to_laser on
 * the host with the liw_lie_* routines, so the device part is + - * / sqrt only, compiled without FMA contraction.
 */
#ifndef LIW_MAP_H
#define LIW_MAP_H
#include <stddef.h>

#include "liw_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_map_params {
    double resolution;        /* metres per cell (0.05 in the reference, visualization.cpp:389) */
} liw_map_params;

typedef struct liw_map_dims {
    int max_submaps;          /* sub-maps (laser key frames) the store can hold */
    long long max_points;     /* points of all sub-maps together */
    long long max_cells;      /* width * height of the largest grid that can be rendered */
} liw_map_dims;

typedef struct liw_map_info { /* of a render */
    int width, height;
    double resolution;
    double origin_x, origin_y;        /* world position of cell (0, 0): the bounding box's minimum */
    long long rays;                   /* valid points = rays cast */
    long long samples;                /* tr values visited over all rays */
    long long unknown, free_cells, hit_once, hit_more;   /* cells holding -1, 0, 50, 100 */
} liw_map_info;

typedef struct liw_map liw_map;

/* bytes of the device store for dims; LIW_EINVAL for a non-positive or non-finite resolution or non-positive dims.  Host-only. */
int liw_map_store_bytes(const liw_map_params* params, const liw_map_dims* dims, size_t* bytes);
/* a map bound to `ctx` (the ctx must outlive it).  NULL only on a bad argument; without a device the handle exists and every
 * compute entry returns LIW_ENODEV; if the store cannot be allocated every compute entry returns LIW_ENOMEM. */
liw_map* liw_map_create(liw_ctx* ctx, const liw_map_params* params, const liw_map_dims* dims);
void liw_map_destroy(liw_map* h);
const char* liw_map_last_error(liw_map* h);

/* upload one key frame's laser-frame points [n_points][3] (n_points may be 0).  Returns the sub-map index; LIW_ENOMEM when
 * max_submaps sub-maps or max_points points would be exceeded (nothing changes then). */
int liw_map_add_submap(liw_map* h, int n_points, const double* points);
int liw_map_num_submaps(liw_map* h);
/* forget every sub-map and the rendered grid */
int liw_map_clear(liw_map* h);

/* render sub-maps 0 .. K - 1 with the world <- laser transforms T_w_l [K][12].  info (may be NULL) is filled on success and
 * on LIW_ENOMEM (width * height > max_cells: nothing is rendered and the previous grid stays as it was). */
int liw_map_render_tf(liw_map* h, int K, const double* T_w_l, liw_map_info* info);
/* the same with the IMU poses [K][6] (p, q of the key frames): T_w_l = make_tf(p, q) * T_imu_to_laser, composed on the host */
int liw_map_render(liw_map* h, int K, const double* poses, liw_map_info* info);
/* info of the grid the handle holds (the last successful render; all zero before the first) */
int liw_map_last_info(liw_map* h, liw_map_info* info);
/* the grid, row-major [height][width], values -1 / 0 / 50 / 100 as nav_msgs/OccupancyGrid; at most cap cells are written.
 * Returns width * height. */
long long liw_map_get(liw_map* h, signed char* out, long long cap);
/* the same grid as a device pointer (valid until the next render, clear or destroy); NULL without a device */
const signed char* liw_map_device_data(liw_map* h);
/* k_map_rays of the last render: SAMPLED atomics issued, cell visits (samples left after dropping those that repeat the
 * previous sample's cell; visits - atomics is what the read-before-atomic filter saved) and HIT atomics issued (at most two
 * per ray).  Any pointer may be NULL. */
int liw_map_probe_counts(liw_map* h, long long* atomics, long long* visits, long long* hit_atomics);
/* T[0 .. n): the accumulated tr values of step = resolution / 2.  Host-only. */
int liw_map_step_table(double resolution, int n, double* T);

/* <path_stem>.pgm (binary P5, maxval 255, top row = highest y) and <path_stem>.yaml (image, resolution, origin [x, y, 0],
 * negate 0, occupied_thresh 0.65, free_thresh 0.196): the file pair ROS' map_server reads.  palette4: grey of -1, 0, 50,
 * 100; NULL = {205, 254, 0, 0}. */
int liw_map_write_pgm(liw_map* h, const char* path_stem, const unsigned char* palette4);
/* the same from a plain array [height][width] of -1 / 0 / 50 / 100 (any other value: LIW_EINVAL).  Host-only. */
int liw_map_write_pgm_grid(const char* path_stem, const signed char* data, int width, int height, double resolution, double origin_x,
                           double origin_y, const unsigned char* palette4);

#ifdef __cplusplus
}
#endif
#endif
