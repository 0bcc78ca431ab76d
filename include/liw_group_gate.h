/* liw_group_gate.h — the edge gate of the group pose graph (liw_group_graph.h): inconsistent cross edges are retired on the device.
 * A cross edge is accepted on its match count and rms alone, and liw_ggraph_solve uses every held edge with weight 1, so one wrong edge
 * (two rooms that look alike) pulls T_g_w for good.  Every edge of a robot pair measures the same quantity, Z = W_a^-1 W_b whichever
 * key frames it came from, so the edges of a pair vote.  The gate is one step of the classic data-snooping loop
 *     solve, evaluate every used edge's whitened squared residual at the solution, retire the worst edge if it exceeds a threshold and
 *     its pair keeps enough other edges, solve again, repeat
 * and it works on what the group's last solve left in the work area, with no read-back: liw_ggraph_solve, liw_ggate_gate, then
 * liw_ggraph_solve with the gate's `changed` as its gsel, as often as edges are to be retired (one per call and group, because the
 * residuals redistribute after every removal).
 *
 * It takes the liw_ggraph_ctx and the store of liw_group_graph.h and follows its conventions: the stream is the caller's, no call
 * synchronises or reads back except the test hook, nothing is written on LIW_EINVAL, bad arguments are reported before LIW_ENODEV, there
 * is no CPU fallback and no atomic: the arg-max runs in a fixed order, so equal inputs give equal bytes.
 *
 * The store's layout and sizes are those of liw_group_graph.h; the gate gives a meaning to bytes that are padding there:
 *   edge record   int32 at byte 20: state (0 active, 1 rejected); double at byte 24: chi2, the value the last gate that saw this edge in
 *                 a solve computed for it, 0 until then
 *   header        int32 at byte 64: rejected (count); int32 at byte 68: gated_solves (the solve count the last gate worked on)
 * liw_ggraph_reset clears all of them.  liw_ggraph_add_edges keeps its rules: a held (a, q, b, i) is a duplicate whether the edge is
 * active or rejected, so a rejected edge does not come back.  liw_ggraph_solve does not use an edge whose state is not 0 and counts it in
 * `skipped`.  A store on which the gate is never called holds the bytes it held before the gate existed.
 *
 * chi2 is NOT a chi-square statistic in the strict sense: it is the squared norm of the residual the solver minimises, with the ctx's
 * J_noise, and the reference's edge_noise puts 1 / sigma_p[1] at J(1, 2) and leaves J(1, 1) = 1 (liw_ggraph_create keeps this as
 * written).  So chi2_max is a tuning parameter on the solver's own metric, not a quantile.
 *
 * Out of scope: reinstating a rejected edge or re-using its slot when the list is full, support from cycles over several pairs, edge
 * weights, robust losses inside the solve, un-linking a robot.
 */
#ifndef LIW_GROUP_GATE_H
#define LIW_GROUP_GATE_H
#include "liw_group_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One gate step for the groups with gsel[g] != 0 (gsel [G] uint8, required).  changed [G] uint8 is written for EVERY group: 1 where an
 * edge was retired, 0 elsewhere (unselected and not eligible groups included), so it is directly the gsel of the next liw_ggraph_solve.
 * A selected group is eligible when its solve count is positive and differs from gated_solves, and its last summary is not termination
 * 6 and has a finite final cost.  For an eligible group, over the node list, constant flags, per-edge node indices and use flags, Z and
 * the accepted state x of that last solve (T_g_w and the poses are not read; edges appended since the solve are ignored):
 *   c_e        = |J_noise log_SE3(X_b^-1 X_a Z_e)|^2 for every used edge e, the residual the solver minimised; stored in the record
 *   support_e  = the number of OTHER used edges on the same unordered robot pair
 *   candidates = the used edges with c_e > chi2_max and support_e >= min_support (a NaN c_e compares false)
 * The candidate with the largest c_e, the lowest list index among equals, gets state 1; `rejected` goes up by one and changed[g] = 1.
 * gated_solves becomes the solve count, so a second gate after the same solve writes changed[g] = 0 and nothing else.  A pair keeps at
 * least min_support used edges, so no node is ever disconnected.  One work-group of 256 per group: edges strided over the threads, the
 * support by a scan of the solve's edge list (E^2 / 256 pair tests per thread), a block arg-max on (c, index).
 * LIW_EINVAL: a null ctx / store / gsel / changed, a misaligned store, chi2_max not a positive finite number, min_support < 1. */
int liw_ggate_gate(liw_ggraph_ctx* ctx, void* store, const unsigned char* gsel, double chi2_max, int min_support, unsigned char* changed,
                   void* stream);

/* ---- test hook, a synchronous copy: for the first min(n, cap) held edges state [.] and chi2 [.], and counts2 = {rejected,
 * gated_solves} (any may be NULL); returns n.  LIW_EINVAL: group outside 0 .. G-1, a null or misaligned store, cap < 0. */
int liw_ggate_get(liw_ggraph_ctx* ctx, const void* store, int group, int cap, int* state, double* chi2, int* counts2);

#ifdef __cplusplus
}
#endif
#endif
