/* liw_group_joint.h — the joint pose graph of a group of fleet robots on the device: cross edges between key frames.
 * liw_group_graph.h keeps every cross edge of a group and refines one rigid T_g_w per robot, so a cross edge can only move a robot's
 * whole trajectory.  Here the key frames of all members of a group are the nodes of ONE graph in the group frame, tied by every member's
 * sequential edges and own loop edges (read in place from a liw_posegraph_batch.h store) and by the group's held cross edges (read in
 * place from a liw_group_graph.h store), so that a member's drift is corrected by what its team-mates saw.
 *
 * liw_gjoint_solve is a pure function of its inputs, per selected group g; nothing is carried from one solve to the next, and the
 * back-end store, the group-graph store and T_g_w are only read.
 *   members   the robots with group_of == g, linked != 0 and at least one key frame in the back-end store, in robot-index order.  More
 *             than max_members of them sets members_full.
 *   nodes     all key frames of the members; node index = the member's offset (the prefix sum of the members' key-frame counts) + k.
 *             The start is x0 = log_SE3(T_g_w[r] * make_tf(P_r[k])), P the corrected poses, with the correctly rounded functions of
 *             liw_crmath.hpp and liw_lie_mul's products (no FMA contraction).  More nodes than max_nodes sets nodes_full.
 *   constant  exactly ONE node is held constant: key frame 0 of the constant member, which is the lowest-index member with fixed[r] != 0,
 *             else the lowest-index member.  LIMIT: other fixed members are FREE in this solve (one constant node only).
 *   edges     the reference's edge factor J_noise * log_SE3(X_j^-1 X_i tf12) times a weight, J_noise from the loop sigmas of
 *             liw_pg_params, summed in this order:
 *               1. every member's sequential edges (k - 1, k) from the back-end store's seq edge part, weight 1;
 *               2. every member's own loop edges from that store, indices shifted by the member's offset, weight loop_edge_k, members
 *                  in robot order and loops in list order;
 *               3. the group's held cross edges {a, q, b, i, tf12} in list order, as a direct edge from node (a, q) to node (b, i) with
 *                  tf12 as held, weight loop_edge_k.  The use rule is liw_ggraph_solve's: a != b, both robots members, q and i inside
 *                  the robots' key frames, state word 0; any other cross edge is skipped and counted.
 *             More own loop edges plus used cross edges than max_loops sets loops_full.
 *   ground    the ground factors of liw_pg_params run on every node when its switches say so, evaluated on the GROUP-FRAME pose: the
 *             group frame is an anchor's world frame, and the robots of a group share a floor.
 *   solver    Levenberg-Marquardt under liw_lm_rules.hpp with Jacobi scaling and the termination tests of liw_fpg_solve, at most
 *             max_iters iterations (<= 0: 50), all selected groups in lock-step on the device.  check_every as in liw_fpg_solve:
 *             <= 0 never synchronises; n > 0 reads the count of groups still iterating back every n iterations.  Identical bytes.
 * The linear system is solved as liw_fpg_solve solves a chain: the separators are the first and last node of every member's chain,
 * every 48th key frame counted inside the chain, the constant node and both ends of every own loop and used cross edge; a wave
 * eliminates the interior of every segment between two consecutive separators of the SAME chain, and a work-group factorises the
 * separators' packed triangle (in LDS up to 8192 doubles, else in the work area, with the same instructions and so the same bytes).
 *
 * Output: the pose part [B][max_keyframes][6] at liw_gjoint_pose_offset, readable in place as liw_fmap_render's poses with
 * robot_stride = 6 * max_keyframes.  For every member of a selected group rows 0 .. K_r - 1 are written: the solved poses, or x0 when
 * the group is not solved (fewer than two nodes, no edge, or a *_full flag) or its solve failed (termination 6 or a cost that is
 * not finite).  Of robots that are no member of a selected group no byte of the pose part is written.  summary[g] (zeros for a group
 * that is not solved) is written for every selected group and kept in the header.
 *
 * The store: the pose part, G headers of 256 B, one int32 per robot (its node offset), G work areas, one count word.
 *   header  int32 [0] reserved (0), [1] members_full, [2] nodes_full, [3] loops_full, [4] members, [5] nodes, [6] sequential edges, [7] own
 *           loop edges, [8] cross edges used, [9] cross edges skipped, [10] separators, [11] solved (the last call ran the solver on
 *           it), [12] the constant node; bytes 64 .. 95 the liw_summary of the last solve.  Counts behind a raised *_full flag are 0.
 *
 * Conventions as liw_group_graph.h: the caller owns all device memory; all work goes on `stream`; there is no read-back unless
 * check_every > 0 (and in the getters at the end); nothing is written on LIW_EINVAL, and bad arguments are reported before LIW_ENODEV;
 * liw_gjoint_store_bytes / _layout / _pose_offset are host-only; there is NO CPU fallback.  No atomic decides a position or a value (one
 * atomic OR raises a group's "pivot not positive" flag); sums run in an order fixed by the group's own graph, so equal inputs give equal
 * bytes whatever G, B and the indices.  A fresh store may be all zeros; two calls on one store must not overlap on different streams.
 *
 * Limits (LIW_EINVAL otherwise): every dimension >= 1 (max_robot_loops >= 0), max_members <= 1024, G * (max_nodes + max_loops) and
 * B * max_keyframes < 2^31.
 */
#ifndef LIW_GROUP_JOINT_H
#define LIW_GROUP_JOINT_H
#include <stddef.h>

#include "liw_posegraph.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_gjoint_dims {
    int B;                 /* robots */
    int G;                 /* groups */
    int max_keyframes;     /* of the back-end store (liw_fpg_dims) */
    int max_robot_loops;   /* max_loops of the back-end store */
    int max_edges;         /* of the group-graph store (liw_ggraph_dims) */
    int max_members;       /* members a group's solve can hold */
    int max_nodes;         /* key frames of all members of a group */
    int max_loops;         /* own loop edges plus used cross edges of a group */
} liw_gjoint_dims;

typedef struct liw_gjoint_layout_info {
    size_t bytes;              /* whole store */
    size_t pose_off;           /* the pose part [B][max_keyframes][6] */
    size_t header_off;         /* group g's header at header_off + 256 g */
    size_t work_off;
    size_t work_group_bytes;   /* work area of one group */
    int max_separators;        /* S = min(max_nodes, max_nodes / 48 + 2 max_members + 2 max_loops) */
    int tri_doubles;           /* 3 S (6 S + 1) */
} liw_gjoint_layout_info;

typedef struct liw_gjoint_ctx liw_gjoint_ctx;

/* Host-only; LIW_EINVAL for bad dims or a null pointer. */
int liw_gjoint_store_bytes(const liw_gjoint_dims* dims, size_t* bytes);
int liw_gjoint_layout(const liw_gjoint_dims* dims, liw_gjoint_layout_info* out);
int liw_gjoint_pose_offset(const liw_gjoint_dims* dims, size_t* off);

/* a ctx bound to the solver parameters (extrinsics and ground sigmas), the pose-graph parameters and dims.  NULL only on a bad argument. */
liw_gjoint_ctx* liw_gjoint_create(const liw_params* params, const liw_pg_params* pg, const liw_gjoint_dims* dims, int device);
void liw_gjoint_destroy(liw_gjoint_ctx* ctx);
const char* liw_gjoint_last_error(liw_gjoint_ctx* ctx);

/* The joint solve of the groups with gsel[g] != 0 (gsel [G] uint8, required).  fpg_store: a liw_posegraph_batch.h store of
 * {B, max_keyframes, max_robot_loops}; ggraph_store: a liw_group_graph.h store of {B, G, any max_members, max_edges}; group_of [B] int32,
 * linked, fixed [B] uint8, T_g_w [B][12].  summary [G] must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null ctx / store / fpg_store / ggraph_store / group_of / linked / fixed / T_g_w / gsel / summary, a misaligned (8) store. */
int liw_gjoint_solve(liw_gjoint_ctx* ctx, void* store, const void* fpg_store, const void* ggraph_store, const int* group_of,
                     const unsigned char* linked, const unsigned char* fixed, const double* T_g_w, const unsigned char* gsel, int max_iters,
                     int check_every, liw_summary* summary, void* stream);

/* ---- test hooks.
 * Triangles of more than `doubles` entries run from the work area (0: all of them; default and maximum 8192).  Host-only. */
int liw_gjoint_set_lds_doubles(liw_gjoint_ctx* ctx, int doubles);
/* The rest are synchronous copies of what the group's last solve left.  LIW_EINVAL: group outside 0 .. G-1, a null or misaligned store,
 * cap < 0, a null output where one is required. */
int liw_gjoint_get_header(liw_gjoint_ctx* ctx, const void* store, int group, int* words16);
int liw_gjoint_get_summary(liw_gjoint_ctx* ctx, const void* store, int group, liw_summary* summary);
/* the first min(n, cap) members: robots [.], offsets [.] (either may be NULL); returns n (0 behind members_full) */
int liw_gjoint_get_members(liw_gjoint_ctx* ctx, const void* store, int group, int cap, int* robots, int* offsets);
/* the first min(n, cap) nodes: row [.] = robot * max_keyframes + key frame, sepidx [.] = the node's separator index or -1 (either may be
 * NULL); returns n (0 behind a *_full flag) */
int liw_gjoint_get_nodes(liw_gjoint_ctx* ctx, const void* store, int group, int cap, int* row, int* sepidx);
/* the first min(s, cap) separators (node indices, ascending; may be NULL); returns the separator count s */
int liw_gjoint_get_separators(liw_gjoint_ctx* ctx, const void* store, int group, int cap, int* sep);

#ifdef __cplusplus
}
#endif
#endif
