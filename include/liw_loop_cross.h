/* liw_loop_cross.h — inter-robot loop closure of the fleet on the device: the newest key frame of robot a is matched against the
 * candidate slots of ANOTHER robot b of the same liw_loop_batch.h store, the accepted edge gives T_w1_w2 (b's world frame in a's),
 * and accepted edges are chained into the per-robot transform T_g_w (robot world -> group frame) that liw_map_group.h renders
 * with.  The calls take the liw_floop_ctx and the store of liw_loop_batch.h and change nothing in the store's layout; the robot
 * regions are only read.  Conventions as liw_loop_batch.h: the caller owns all device memory, every launch goes on `stream`, no
 * call synchronises or reads back (fixed grids stride over work counts that stay on the device), nothing is written on
 * LIW_EINVAL, and there is no CPU fallback (LIW_ENODEV without a gfx950 device; bad arguments are reported first).
 *
 * liw_xloop_detect uses the scratch area of the store that liw_floop_add_keyframes and liw_floop_detect use (gate records, the
 * pair list, match results, summaries, correspondence lists, ICP results), under the same rule: two calls on one store must not
 * overlap on different streams.  A query robot launches at most ceil(max_keyframes / s) pairs, as in own detection, so the area
 * is large enough as it is.
 *
 * Cross detection.  For every robot a with key[a] != 0, mask on and partner[a] = b in 0 .. B-1, b != a: the query is a's newest
 * key frame q = K_a - 1 (its feature is always held), the candidates are b's key frames i = 0, s, 2 s, ... < K_b.  There is no
 * min_interval, no origin-distance gate and no tf gate: the two world frames are unrelated.  Gates, in order:
 *   1. null / invalid: state != LIW_LOOP_VALID on either side;
 *   2. points: n1 < thr || n2 < thr || n1 == 0 || n2 == 0, with thr = params.min_match_threshold of the ctx;
 *   3. the draws draw_row(seed, q, i, d, n1), repeated rows skipped; match and select exactly as liw_floop_detect runs them (the same
 *      device bodies), the query rows read from a's region and the candidate's from b's;
 *   4. size: size > min_match (min_match >= min_match_threshold, LIW_EINVAL otherwise);
 *   5. the planar closed-form ICP of liw_floop_detect over the correspondence list in list order: P1 moved by
 *      inverse(tf_a[q] T_iw), P2 by inverse(tf_b[i] T_iw), z dropped, correctly rounded atan2 / sin / cos, it12 = T_iw w T_iw^-1;
 *   6. residual: rms = sqrt(sum |p1 - (R p2 + t)|^2 / len) over the planar pairs, summed in list order; passes when !(rms > max_rms).
 * Choice: of the passing candidates the one with the largest size wins, the lowest i on a tie (own detection takes the first
 * passing candidate because its tf gate vouches for it; here nothing does).  A wave per robot reduces over (size, -i); no atomic
 * decides anything, and results are reproducible bit for bit.
 * Outputs, per robot with key set:
 *   found [B] uint8; edge [B][4] int32 = {q, b, i, size} ({-1, -1, -1, 0} when not found);
 *   tf12 [B][12] = it12; T_w1_w2 [B][12] = (tf_a[q] it12) inverse(tf_b[i]), which maps b-world coordinates into a's world (the products
 *   of liw_lie_mul, no FMA contraction); rms [B]: these three are written only when found;
 *   stats [B][6] int64 = candidates, launched, tasks, quick_pass, accepted, icp_checked as liw_loop_stats (every accepted candidate
 *   gets its ICP here, so icp_checked = accepted).
 * partner out of range, partner[a] == a, K_b == 0, K_a == 0 or an invalid query: found = 0, edge as not found, stats zero.
 * key[a] == 0: found[a] = 0 and nothing else of a is written.  Masked out: nothing of a is written.  The partner's region is only
 * read, so a may query b while b queries a in the same call.
 *
 * Partner choice and linking.  `linked` [B] uint8 and T_g_w [B][12] are the caller's state: an anchor is a robot the caller marks
 * linked with a T_g_w of its choice.  group_of [B] int32, negative: in no group.  Nothing is ever re-linked or refined.
 */
#ifndef LIW_LOOP_CROSS_H
#define LIW_LOOP_CROSS_H
#include "liw_loop_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct liw_xloop_params {
    int min_match;    /* a candidate is accepted when size > min_match; >= the ctx's min_match_threshold */
    double max_rms;   /* metres; a candidate passes when !(rms > max_rms); >= 0 */
} liw_xloop_params;

/* Mapping: gates and draws a wave per query robot and a lane per candidate (64 at a time), one work-group scans the counts, the
 * compact pair list by prefix counts, match on a fixed grid of 4 096 work-groups, select a wave per pair, ICP + rms a lane per
 * pair, the choice a wave per robot.
 * LIW_EINVAL: a null ctx / store / key / partner / params / found / edge / tf12 / T_w1_w2 / rms / stats, a misaligned (8) store,
 * min_match < min_match_threshold, max_rms negative or NaN. */
int liw_xloop_detect(liw_floop_ctx* ctx, const void* store, const unsigned char* key, const int* partner, const liw_xloop_params* params,
                     const unsigned char* mask, unsigned char* found, int* edge, double* tf12, double* T_w1_w2, double* rms,
                     long long* stats, void* stream);

/* partner [B] int32 for a round of cross detection: for an unlinked robot a of group g, with m_0 < m_1 < ... the n linked members
 * of g in index order, partner[a] = m_(round mod n); -1 when n = 0, when a is linked, or when a is in no group.  A wave per robot
 * counts and picks with ballots.  LIW_EINVAL: a null ctx / group_of / linked / partner, round < 0. */
int liw_xloop_partner(liw_floop_ctx* ctx, const int* group_of, const unsigned char* linked, int round, int* partner, void* stream);

/* Links unlinked robots through the edges of one liw_xloop_detect call (its partner, found, edge and T_w1_w2).  Two kernels, so
 * that no lane reads what another lane writes.  Decide: every unlinked robot r with a group looks at the `linked` flags as they
 * were before the call:
 *   (i)  found[r] and p = partner[r] linked and of r's group: r links through its own edge, T_g_w[r] = T_g_w[p] inverse(T_w1_w2[r]);
 *   (ii) otherwise the lowest a with partner[a] == r, found[a], linked[a] and r's group: T_g_w[r] = T_g_w[a] T_w1_w2[a].
 * The decision (source and direction) is staged in group_linked[r], which is an output for every robot.  Apply: composes the
 * transform (liw_lie_mul's arithmetic), sets linked[r], writes via[r] = {source robot, own key frame, source key frame, size},
 * and writes group_linked[r] for EVERY robot: group_of[r] if it is linked now, else -1 (the group_of argument of
 * liw_gmap_render, for which an unlinked robot is in no group).  The sources were linked before the call, so their T_g_w is not
 * written in it; via of a robot that does not link in this call is not written.  A chain a -> b -> c takes two calls.
 * LIW_EINVAL: a null ctx or array. */
int liw_xloop_link(liw_floop_ctx* ctx, const int* group_of, const int* partner, const unsigned char* found, const int* edge,
                   const double* T_w1_w2, unsigned char* linked, double* T_g_w, int* via, int* group_linked, void* stream);

/* ---- test hook (a synchronous device -> host copy): the pair (robot, candidate key frame `cand` of its partner) of the last
 * liw_xloop_detect on this store.  info[8] = {size, draw, row, bin, quick_pass, list length, query row, n2}; p1 / p2 (may be NULL)
 * get at most cap entries of the correspondence list (query points, candidate points).  Returns the list length; LIW_EINVAL when
 * the pair was not launched, for a robot outside 0 .. B-1 or a null store / info. */
int liw_xloop_get_pair(liw_floop_ctx* ctx, const void* store, int robot, int cand, int cap, int* info, int* p1, int* p2);

#ifdef __cplusplus
}
#endif
#endif
