/* liw_loop.h — C ABI of the laser loop-closure detector of the pose-graph back-end (the reference's corner-descriptor loop
 * detection, src/trajectory/keyframe_manager.cpp:642-712 and :898-1184).
 *
 * Per laser key frame a sub-map feature is built: the world-frame corners of the last `submap_count` laser key frames,
 * de-duplicated on the host in the reference's serial order, then one descriptor row per point on the device: for every other
 * point j the quantised distance dij = int(|p_j - p_i| / d_res + 0.5) and the direction aij, sorted, plus a bitmap of the dij
 * values (quick_des).  liw_loop_detect compares the newest feature with every s-th older one (s = submap_count / 3 + 1):
 * 5 drawn rows of the newest sub-map against every row of the candidate's, a merge-join on dij with an angle-difference
 * histogram per row pair; the largest bin gives point correspondences, a planar ICP the relative pose, and a gate against the
 * tracking poses accepts it.  Each (candidate, draw, row) triple is one independent device task.
 *
 * Deliberate differences from the reference (docs/WIDENING.md "Loop detection"):
 *   - no rand() and no shuffle: points stay in de-duplication order; draw d (0..4) of query key frame q against candidate c
 *     is row splitmix64(seed ^ (q << 40) ^ (c << 8) ^ d) % n1 (splitmix64: z = x + 0x9E3779B97F4A7C15, then the standard
 *     finaliser); a repeated row is skipped, as in the reference;
 *   - among the angle bins of maximal size the one that reached that size first wins (the reference picks a random one);
 *   - descriptor rows are sorted by (dij, j) (std::sort leaves the order of equal dij open);
 *   - the ICP (ICP_solve_by_opt, Ceres LM over point_factor from identity) is the planar Procrustes optimum in closed form:
 *     yaw from the centred cross sums, t = c1 - R c2, z / roll / pitch = 0 — the minimiser that LM converges to for the planar
 *     correspondences it is given;
 *   - a sub-map with more than max_points points is invalid (never a query, never a candidate; liw_loop_status reports it);
 *     the reference has no cap;
 *   - the detector runs on the caller's thread.
 *
 * Conventions: the library owns the device store (sized by liw_loop_store_bytes); calls return >= 0 on success and a negative
 * LIW_E* code otherwise.  There is NO CPU fallback: without a gfx950 device liw_loop_create still returns a handle, but every
 * compute entry returns LIW_ENODEV.  liw_loop_store_bytes, liw_loop_sizes and liw_loop_icp are host-only and work anywhere.
 * A transform T12 is R (9, row-major) then t (3), as in liw_lie.h.  Kernels are compiled without FMA contraction, so dij and the
 * de-duplicated points are bit-identical to the host arithmetic; aij uses the device acos (within an ulp of the host's).
 *
 * Limits (LIW_EINVAL otherwise): max_points <= 4096 (the sort key is dij << 12 | j), nAngle + 1 <= 256 bins
 * (a_res >= about 0.0249), quick_des words W <= 512 (d_res >= about 0.0031), submap_count >= 1, min_interval >= 1.
 * A pair distance with dij >= 2^20 - 1 marks the feature invalid (the match kernel looks up the key dij + 1 << 12 in 32 bits).
 */
#ifndef LIW_LOOP_H
#define LIW_LOOP_H
#include <stddef.h>

#include "liw_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_loop_params {
    double a_res;             /* angle bin width (config/office.yaml:98) */
    double d_res;             /* distance quantum (:99) */
    int submap_count;         /* laser key frames per sub-map (:100) */
    int min_match_threshold;  /* laser_loop_min_match_threshold (:101) */
    int min_interval;         /* loop_detect_min_interval (:102) */
    double max_dis;           /* loop_max_dis: origin distance gate (:104) */
    double max_tf_p;          /* loop_max_tf_p (:106) */
    double max_tf_q;          /* loop_max_tf_q (:107) */
    unsigned long long seed;  /* seed of the row draws */
} liw_loop_params;

typedef struct liw_loop_dims {
    int max_keyframes;        /* key frames (laser or not) the detector can hold */
    int max_points;           /* points per sub-map; a larger sub-map is invalid */
} liw_loop_dims;

typedef struct liw_loop_edge {
    int index1, index2;       /* newest key frame, older key frame */
    int size;                 /* correspondences of the accepted match */
    double tf12[12];          /* T_imu_to_wheel * w_T12 * T_imu_to_wheel^-1 */
} liw_loop_edge;

/* liw_loop_match result */
#define LIW_LOOP_ACCEPTED 0      /* size > min_match_threshold */
#define LIW_LOOP_GATE_NULL 1     /* a null (non-laser) or invalid feature */
#define LIW_LOOP_GATE_POINTS 2   /* a feature has fewer than min_match_threshold points (or none) */
#define LIW_LOOP_GATE_DIS 3      /* |t| of origin1^-1 origin2 > max_dis */
#define LIW_LOOP_GATE_SIZE 4     /* best size <= min_match_threshold */
typedef struct liw_loop_match_info {
    int size;                 /* best match size (0: no row pair got past the quick filter with a pair) */
    int draw, row, bin;       /* winning draw (0..4), candidate row, angle bin; -1 when size == 0 */
    int query_row;            /* row of the query the winning draw picked */
    int gate;                 /* LIW_LOOP_ACCEPTED or the gate that rejected */
    int tasks, quick_pass;    /* (draw, row) tasks run and how many passed the quick filter */
} liw_loop_match_info;

/* liw_loop_status states */
#define LIW_LOOP_NULL 0          /* non-laser key frame: no feature */
#define LIW_LOOP_VALID 1
#define LIW_LOOP_OVER_CAP 2      /* more than max_points points after de-duplication */
#define LIW_LOOP_DIJ_OVERFLOW 3  /* a pair distance quantised to dij >= 2^20 - 1 */

typedef struct liw_loop_stats {   /* of the last liw_loop_detect */
    int candidates;           /* candidate key frames visited (i = 0, s, 2s, ...) */
    int launched;             /* candidates that passed the host gates and ran on the device */
    long long tasks;          /* (candidate, draw, row) tasks */
    long long quick_pass;     /* tasks that passed the quick filter */
    int accepted;             /* candidates with size > threshold (read back) */
    int icp_checked;          /* candidates that went through ICP + the tf gate */
} liw_loop_stats;

typedef struct liw_loop liw_loop;

/* bytes of the device store for (params, dims); LIW_EINVAL for bad params or dims.  Host-only. */
int liw_loop_store_bytes(const liw_loop_params* params, const liw_loop_dims* dims, size_t* bytes);
/* quick_des words W = int((100 / d_res + 1) / 64 + 1) and nAngle = int(2 pi / a_res) + 2.  Host-only. */
int liw_loop_sizes(const liw_loop_params* params, int* quick_words, int* n_angle);

/* a detector bound to `ctx` (device and T_imu_to_wheel come from it; the ctx must outlive the detector).  NULL only on a bad
 * argument; without a device the handle exists and every compute entry returns LIW_ENODEV; if the device store cannot be
 * allocated, every compute entry returns LIW_ENOMEM (liw_loop_last_error says so). */
liw_loop* liw_loop_create(liw_ctx* ctx, const liw_loop_params* params, const liw_loop_dims* dims);
void liw_loop_destroy(liw_loop* h);
const char* liw_loop_last_error(liw_loop* h);
int liw_loop_num_keyframes(liw_loop* h);

/* append a key frame: its tracking pose tf_tracking12 (world <- IMU) and, for a laser key frame, its world-frame corners
 * [n_corners][3].  Builds its feature (host de-duplication, device descriptors).  Returns the key-frame index, LIW_ENOMEM when
 * max_keyframes are held. */
int liw_loop_add_keyframe(liw_loop* h, int is_laser, const double* tf_tracking12, int n_corners, const double* corners);
/* laser_loop_detect for the newest key frame: 1 and *out filled if a loop closes, 0 if not, < 0 on error. */
int liw_loop_detect(liw_loop* h, liw_loop_edge* out);
int liw_loop_last_stats(liw_loop* h, liw_loop_stats* out);

/* ---- test and inspection hooks */
/* match_map(query, candidate) with the draws detect would use.  Returns the number of correspondences written to p1_idx /
 * p2_idx (point indices of the query / candidate, at most cap; 0 unless accepted); *info says why. */
int liw_loop_match(liw_loop* h, int query, int candidate, int cap, int* p1_idx, int* p2_idx, liw_loop_match_info* info);
/* the de-duplicated points [n][3] of key frame k's feature (at most cap); returns n */
int liw_loop_get_points(liw_loop* h, int k, int cap, double* points);
/* row i of key frame k's descriptors: n - 1 entries of dij, j, aij in sorted order (at most cap) and the W quick_des words;
 * returns n - 1 */
int liw_loop_get_row(liw_loop* h, int k, int i, int cap, int* dij, int* j, double* aij, unsigned long long* quick_des);
/* LIW_LOOP_* state of key frame k's feature; n_points and the sub-map origin (T12) may be NULL */
int liw_loop_status(liw_loop* h, int k, int* n_points, double* origin12);
/* the closed-form planar ICP: T12 with p1 ~ T12 * p2 over n >= 1 pairs [n][3] (z ignored).  Host-only. */
int liw_loop_icp(int n, const double* p1, const double* p2, double* T12);

#ifdef __cplusplus
}
#endif
#endif
