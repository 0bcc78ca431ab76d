/* liw_group_graph.h — a small pose graph per group of fleet robots on the device.  liw_loop_cross.h links every robot of a group
 * through one accepted cross edge and composes T_g_w (robot world -> group frame) once, from the tracking poses of that moment.
 * Here every cross edge is kept, linked robots go on producing edges, and T_g_w is refined from all of them and from the
 * back-end's CURRENT corrected poses: one node per linked robot, x_r = log_SE3(T_g_w[r]); one edge per kept cross edge
 * {a, q, b, i, size, tf12}, whose measurement is recomputed at solve time from the pose-independent tf12,
 *     Z = make_tf(P_a[q]) * tf12 * inverse(make_tf(P_b[i]))        (b's world in a's world; liw_lie_mul's arithmetic, no FMA contraction)
 * with P the corrected poses of liw_posegraph_batch.h read in place, and whose residual is the reference's edge factor with weight 1,
 *     J_noise * log_SE3(X_b^-1 X_a Z)                               (J_noise from the loop sigmas of liw_pg_params; no ground factors:
 *                                                                    T_g_w is not a body pose).
 *
 * Conventions as liw_posegraph_batch.h / liw_loop_cross.h: the caller owns all device memory (the store sized by
 * liw_ggraph_store_bytes and every array); every launch goes on `stream`; no call synchronises or reads back, except the test hooks
 * at the end; nothing is written on LIW_EINVAL, and bad arguments are reported before LIW_ENODEV; there is NO CPU fallback
 * (liw_ggraph_store_bytes and liw_ggraph_layout are host-only and work anywhere).  No atomic is used at all: positions come from
 * ballots and prefix counts in robot order, and sums run in a fixed order that depends on the group's own graph only (nodes in
 * robot-index order, edges in list order), so equal inputs give equal bytes whatever G, B and the group's index.
 * A fresh store must be reset once.  Two calls on one store must not overlap on different streams.
 *
 * The store: G group regions (liw_ggraph_layout_info::group_bytes each, parts 256-byte aligned), then G work areas.
 *   header   256 B   int32 [0] edges held, [1] edges_full, [2] members_full, [3] bad_edge, [4] solves, and of the last solve [5] edges
 *                    skipped, [6] nodes, [7] edges used; bytes 32..63 the liw_summary of the last solve
 *   edges    128 B each, max_edges of them: int32 a, q, b, i, size, 3 words of padding, then tf12[12]
 * liw_group_gate.h, the edge gate on this ctx and store, gives the padding words of a record (a state and a double) and header bytes
 * 64 .. 71 a meaning; here they are written as zeros, and an edge whose state is not 0 is no part of a solve.
 * Work area of a group (M = max_members, E = max_edges): the LM state (256 B), the node list and constant flags, the node indices and
 * the use flag of every edge, x, candidate, step, Jacobi scale, LM diagonal and gradient (48 M each), the diagonal blocks (288 M), the
 * edge blocks [J | r] (624 E), Z with its two pose transforms (288 E), the packed lower triangle of the 6 M unknowns (8 * 3 M (6 M + 1))
 * and the right-hand side (48 M).  The triangle is held in LDS when it has at most 8192 doubles (64 KiB: M <= 21) and in the work area
 * otherwise, with the same instructions and so the same bytes.
 *
 * Limits (LIW_EINVAL otherwise): B, G, max_members, max_edges >= 1, max_members <= 1024, max_edges <= 65536.
 */
#ifndef LIW_GROUP_GRAPH_H
#define LIW_GROUP_GRAPH_H
#include <stddef.h>

#include "liw_posegraph.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_ggraph_dims {
    int B;             /* robots */
    int G;             /* groups */
    int max_members;   /* linked robots a group's solve can hold */
    int max_edges;     /* cross edges kept per group */
} liw_ggraph_dims;

typedef struct liw_ggraph_layout_info {
    size_t bytes;              /* whole store = G * group_bytes + work_bytes */
    size_t group_bytes;        /* region of one group; group g starts at g * group_bytes */
    size_t work_off;           /* = G * group_bytes */
    size_t work_bytes;         /* = G * work_group_bytes */
    size_t work_group_bytes;   /* work area of one group */
    int tri_doubles;           /* 3 M (6 M + 1): the packed triangle of a full group */
} liw_ggraph_layout_info;

typedef struct liw_ggraph_ctx liw_ggraph_ctx;

/* bytes of the store for dims; LIW_EINVAL for bad dims or a null pointer.  Host-only. */
int liw_ggraph_store_bytes(const liw_ggraph_dims* dims, size_t* bytes);
/* the same with the sizes of the parts.  Host-only. */
int liw_ggraph_layout(const liw_ggraph_dims* dims, liw_ggraph_layout_info* out);

/* a ctx bound to the edge noise (the loop sigmas of pg; the ground switches and loop_edge_k are not used) and dims; device = HIP
 * device ordinal.  NULL only on a bad argument. */
liw_ggraph_ctx* liw_ggraph_create(const liw_pg_params* pg, const liw_ggraph_dims* dims, int device);
void liw_ggraph_destroy(liw_ggraph_ctx* ctx);
const char* liw_ggraph_last_error(liw_ggraph_ctx* ctx);

/* header and edge records cleared for the groups with gmask[g] != 0 (gmask [G] uint8, NULL = all).
 * LIW_EINVAL: a null or misaligned (8) store. */
int liw_ggraph_reset(liw_ggraph_ctx* ctx, void* store, const unsigned char* gmask, void* stream);

/* Consumes the outputs of one liw_xloop_detect call (found [B] uint8, edge [B][4] int32 = {q, b, i, size}, tf12 [B][12]).  For every
 * robot a, in index order, with found[a], mask on (mask [B] uint8, NULL = all) and group_of[a] = g in 0 .. G-1: a partner b outside
 * 0 .. B-1, b == a or group_of[b] != g sets g's bad_edge and stores nothing; an edge whose (a, q, b, i) is already held is dropped;
 * otherwise {a, q, b, i, size, tf12[a]} is appended to g's list, or, when the list is full, edges_full is set and nothing is stored.
 * A wave per group walks the fleet 64 robots at a time; the position comes from ballots and prefix counts, the lanes scan the held
 * list for the duplicate.
 * LIW_EINVAL: a null ctx / store / group_of / found / edge / tf12, a misaligned store. */
int liw_ggraph_add_edges(liw_ggraph_ctx* ctx, void* store, const int* group_of, const unsigned char* found, const int* edge, const double* tf12,
                         const unsigned char* mask, void* stream);

/* partner [B] int32 for a round of cross detection in which linked robots keep producing edges.  For robot a of group g >= 0, with
 * m_0 < m_1 < ... the linked members of g other than a (n of them): partner[a] = m_(round mod n), -1 when n = 0; -1 when a is in no
 * group.  For an unlinked robot this is exactly what liw_xloop_partner gives.  A wave per robot counts and picks with ballots.
 * LIW_EINVAL: a null ctx / group_of / linked / partner, round < 0. */
int liw_ggraph_partner(liw_ggraph_ctx* ctx, const int* group_of, const unsigned char* linked, int round, int* partner, void* stream);

/* Refines T_g_w [B][12] of the groups with gsel[g] != 0 (gsel [G] uint8, required).  poses / robot_stride as liw_fmap_render takes
 * them: robot b's corrected key frame k is at poses + b * robot_stride + 6 k (doubles); with liw_fpg_pose_offset a
 * liw_posegraph_batch.h store is read in place.  n_keyframes [B] int32: the key frames each robot holds; fixed [B] uint8: the anchors.
 * Per selected group:
 *   nodes  the linked members of g in index order, x = log_SE3(T_g_w) with the correctly rounded functions of liw_crmath.hpp.  More
 *          than max_members of them: members_full is set and the group is not solved.  Fixed members are constant (identity block,
 *          zero gradient); when no linked member is fixed, the lowest-index linked member is constant.
 *   edges  every held edge with a != b whose two robots are nodes, whose q and i are inside the robots' key frames and whose nodes
 *          are not both constant (an edge between constants has no unknown and, as in Ceres, is no part of the problem), and that
 *          the edge gate of liw_group_gate.h has not rejected (state word 0, as every edge is without the gate).  The others
 *          are skipped and counted in the header.
 *   solve  Levenberg-Marquardt under the rules of liw_lm_rules.hpp with Jacobi scaling and the termination tests of liw_fpg_solve, at
 *          most max_iters iterations (<= 0: 50).  One work-group per group runs the whole loop inside ONE launch: 16 lanes evaluate an
 *          edge with dual numbers, a wave assembles a node in edge order, Cholesky and both triangular solves on the packed triangle,
 *          cost sums lane-strided with a butterfly, wave 0 takes the trust-region decisions.
 * Afterwards T_g_w[r] = make_tf(x_r) for the non-constant nodes of a solved group, summary[g] is written and kept in the header, and
 * the solve count goes up.  A group with no usable edge or fewer than two nodes is treated as not selected: like a group that raises
 * members_full it keeps the header words skipped / nodes / used, the summary and the liw_ggraph_get_Z rows of its last completed solve.  A solve fails when it
 * ends with termination 6 (five consecutive steps whose system had a pivot that is not positive and finite) or with a cost that is
 * not finite: the summary records it, and no byte of T_g_w is written.  No byte of T_g_w is written either for constant nodes,
 * unlinked robots or robots of unselected groups.  summary [G] must stay valid until the work on `stream` has run.
 * LIW_EINVAL: a null ctx / store / poses / n_keyframes / group_of / linked / fixed / T_g_w / gsel / summary, robot_stride < 0, a
 * misaligned store. */
int liw_ggraph_solve(liw_ggraph_ctx* ctx, void* store, const double* poses, long long robot_stride, const int* n_keyframes, const int* group_of,
                     const unsigned char* linked, const unsigned char* fixed, double* T_g_w, const unsigned char* gsel, int max_iters,
                     liw_summary* summary, void* stream);

/* ---- test hooks.
 * Triangles of more than `doubles` entries run from the work area (0: all of them; default and maximum 8192).  Host-only. */
int liw_ggraph_set_lds_doubles(liw_ggraph_ctx* ctx, int doubles);
/* The rest are synchronous copies.  LIW_EINVAL: group outside 0 .. G-1, a null or misaligned store, cap < 0.
 * the first min(n, cap) held edges: idx [.][5] = a, q, b, i, size; tf12 [.][12] (either may be NULL); returns n */
int liw_ggraph_get_edges(liw_ggraph_ctx* ctx, const void* store, int group, int cap, int* idx, double* tf12);
/* flags [8]: the eight header words */
int liw_ggraph_get_flags(liw_ggraph_ctx* ctx, const void* store, int group, int* flags8);
int liw_ggraph_get_summary(liw_ggraph_ctx* ctx, const void* store, int group, liw_summary* summary);
/* of the group's last solve, for the first min(n, cap) held edges: used [.] (1: part of the solve), Z [.][12], and the two pose
 * transforms Z was composed from, Ta = make_tf(P_a[q]) and Tb = make_tf(P_b[i]) [.][12] (any may be NULL; rows of unused edges are
 * not meaningful); returns n */
int liw_ggraph_get_Z(liw_ggraph_ctx* ctx, const void* store, int group, int cap, int* used, double* Z, double* Ta, double* Tb);

#ifdef __cplusplus
}
#endif
#endif
