"""Cases of the group edge gate (include/liw_group_gate.h; tests/test_gpu_group_gate.py runs them on the device,
tests/test_group_gate_cases.py guards them on the host alone) and the host restatement of the loop solve -> gate -> solve: the active
subset of a group's edges goes through group_graph_cases.oracle_solve, c_e is twice the cost that oracle.pyoracle.posegraph_linearize
gives for the one-edge graph at the solution, and the rule is restated in gate_rule().

The fleet: B = 10 robots in G = 4 groups, max_members 4, max_edges 8, six key frames per robot, office sigmas.  The lowest robot of
every group is its anchor (the constant node).  A robot yields one edge per add_edges call, so the lists take three calls.  True edges
carry the noise of group_graph_cases (1 mm / 0.2 mrad); a wrong edge measures W_a^-1 W_b D with D a planar offset, so that its
residual at the truth is exactly D.
  group 0 (A)  robots 0, 1: the FIRST edge is wrong (robot 1's starting T_g_w is composed from it, as liw_xloop_link would), then three
               true edges, one of them stored 1 -> 0
  group 1 (B)  robots 2, 3: two different wrong edges among five
  group 2 (C)  robots 4, 5, 6: pair (4, 5) has three true edges and one wrong, pair (5, 6) one true and one wrong (support 1), pair
               (4, 6) one edge
  group 3 (D)  robots 7, 8, 9: eight consistent edges
After a rejection an active edge that starts at the constant node is still there in every group, as oracle_solve needs it.
"""
import functools

import numpy as np

import group_graph_cases as gc
import loop_batch_cases as lbc
import loop_reference as ref

B, G, MAX_MEMBERS, MAX_EDGES, KMAX = 10, 4, 4, 8, 6
GROUP_OF = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3]
LINKED = [1] * B
FIXED = [1, 0, 1, 0, 1, 0, 0, 1, 0, 0]
NKF = [KMAX] * B
NAMES = "ABCD"
CHI2_MAX, MIN_SUPPORT, GATE_ROUNDS = 12.0, 2, 2

# wrong edges: (x, y, yaw) of D in metres and radians
WRONG = dict(A=(0.6, 0.2, 0.15), B1=(0.6, -0.3, 0.15), B2=(-0.4, 0.25, -0.09), C1=(0.55, 0.2, 0.15), C2=(0.4, -0.2, 0.13))
# the three add_edges calls: robot -> (q, b, i, size, wrong offset or None)
CALLS = [
    {0: (5, 1, 0, 20, "A"), 2: (4, 3, 1, 21, "B1"), 3: (0, 2, 1, 19, None), 4: (5, 5, 0, 22, None), 5: (4, 6, 1, 18, None), 6: (3, 4, 2, 17, None),
     7: (5, 8, 0, 25, None), 8: (4, 9, 1, 24, None), 9: (3, 7, 2, 23, None)},
    {0: (4, 1, 1, 18, None), 1: (2, 0, 3, 17, None), 2: (3, 3, 2, 20, None), 3: (3, 2, 0, 22, "B2"), 4: (4, 5, 1, 21, "C1"), 5: (3, 6, 2, 16, "C2"),
     7: (4, 8, 1, 19, None), 8: (3, 9, 2, 18, None), 9: (2, 7, 3, 17, None)},
    {0: (3, 1, 2, 16, None), 2: (2, 3, 3, 15, None), 4: (3, 5, 2, 20, None), 5: (2, 4, 0, 19, None), 7: (3, 9, 4, 21, None), 8: (2, 7, 5, 20, None)},
]
# what the loop is expected to do: the list indices rejected, in order, at MIN_SUPPORT and GATE_ROUNDS
EXPECT = {0: [0], 1: [0, 3], 2: [3], 3: []}


def _offset(x, y, yaw):
    D = np.eye(4)
    D[:3, :3] = ref._exp_so3(np.array([0.0, 0.0, yaw]))
    D[:3, 3] = (x, y, 0.0)
    return D


@functools.lru_cache(maxsize=None)
def fleet():
    """as group_graph_cases.fleet(): dict(W, P, T0, calls)"""
    pose_of, mk = lbc._lie()
    rng = np.random.default_rng(41)
    W = [gc._frame(rng, 4.0) for _ in range(B)]
    P = [[pose_of(gc._frame(rng, 3.0)) for _ in range(NKF[r])] for r in range(B)]
    T0 = [W[r] if FIXED[r] else W[r] @ gc._small(rng, gc.START_P, gc.START_Q) for r in range(B)]
    calls = []
    for c in CALLS:
        found, edge, tf12 = np.zeros(B, np.uint8), np.tile(np.array([-1, -1, -1, 0], np.int32), (B, 1)), np.zeros((B, 12))
        for a, (q, b, i, size, wrong) in c.items():
            found[a], edge[a] = 1, (q, b, i, size)
            Z = ref.iso_inv(W[a]) @ W[b] @ gc._small(rng, gc.NOISE_P, gc.NOISE_Q)
            if wrong:
                Z = Z @ _offset(*WRONG[wrong])
            if wrong == "A":
                T0[b] = W[a] @ Z                      # rule (i) of liw_xloop_link from a robot's first edge: T_g_w[b] = T_g_w[a] Z
            tf12[a] = gc.tf12_of(ref.iso_inv(mk(P[a][q])) @ Z @ mk(P[b][i]))
        calls.append(dict(found=found, edge=edge, tf12=tf12, mask=np.ones(B, np.uint8)))
    return dict(W=W, P=P, T0=T0, calls=calls)


@functools.lru_cache(maxsize=None)
def lists_after(n_calls=3):
    out = gc.new_lists(G)
    for c in fleet()["calls"][:n_calls]:
        gc.add_edges(out, GROUP_OF, c["found"], c["edge"], c["tf12"], c["mask"], max_edges=MAX_EDGES)
    return out


def held_graph(L, group, poses=None, state=None):
    """-> dict(nodes, const, held: per held edge (node a, node b, Z 4x4) or None when the solve's own rules skip it, used: the flags with
    the rejected edges (state) taken out)"""
    poses = fleet()["P"] if poses is None else poses
    Gr = gc.graph_of(L, group, GROUP_OF, LINKED, FIXED, NKF, poses)
    it = iter(Gr["edges"])
    held = [next(it) if u else None for u in Gr["used"]]
    state = [0] * len(held) if state is None else state
    return dict(nodes=Gr["nodes"], const=Gr["const"], held=held, used=[int(h is not None and not s) for h, s in zip(held, state)])


def chi2_of(pyoracle, orc, pg, xa, xb, Z):
    """|J_noise log_SE3(X_b^-1 X_a Z)|^2: twice the oracle's cost of the graph that holds this edge alone"""
    cfg = dict(pg, use_ground_p_factor=False, use_ground_q_factor=False)
    _, _, cost, _ = pyoracle.posegraph_linearize(orc, cfg, np.array([xa, xb]), np.array([[0, 1]], np.int32), gc.tf12_of(Z)[None], None, None)
    return 2.0 * cost


def gate_rule(held, used, chi2, chi2_max, min_support):
    """the rule of liw_ggate_gate -> (the list index to reject or None, the candidates' indices, the support of every edge)"""
    pair = [None if h is None else (min(h[0], h[1]), max(h[0], h[1])) for h in held]
    support = [sum(1 for f in range(len(held)) if f != e and used[f] and pair[f] == pair[e]) if used[e] else 0 for e in range(len(held))]
    cands = [e for e in range(len(held)) if used[e] and chi2[e] > chi2_max and support[e] >= min_support]
    best = None
    for e in cands:                                   # the largest c, the lowest index among equals
        if best is None or chi2[e] > chi2[best]:
            best = e
    return best, cands, support


def run(pyoracle, orc, pg, group, chi2_max=CHI2_MAX, min_support=MIN_SUPPORT, gate_rounds=GATE_ROUNDS, max_iters=0, lists=None, T0=None):
    """solve, then gate_rounds times gate and (where an edge went) solve, restated -> a list of steps, alternately
    dict(kind="solve", x [n, 6], summary, used [flags], skipped) and dict(kind="gate", chi2, state, rejected, changed, reject, cands,
    support); a solve step that the loop skips (changed = 0) is None"""
    L = (lists_after() if lists is None else lists)[group]
    n = len(L["edges"])
    state, chi2, rejected = [0] * n, [0.0] * n, 0
    Gr = held_graph(L, group)
    x = gc.start_x(Gr["nodes"], fleet()["T0"] if T0 is None else T0)
    const = Gr["const"].index(1)
    steps = []

    def solve(x):
        Gs = held_graph(L, group, state=state)
        xs, sm = gc.oracle_solve(pyoracle, orc, pg, x, [h for h, u in zip(Gs["held"], Gs["used"]) if u], const, max_iters)
        steps.append(dict(kind="solve", x=xs, summary=sm, used=Gs["used"], skipped=n - sum(Gs["used"])))
        return xs, Gs

    x, Gs = solve(x)
    for _ in range(gate_rounds):
        if steps[-1] is None:                         # nothing was solved since the last gate: not eligible
            steps += [dict(kind="gate", chi2=list(chi2), state=list(state), rejected=rejected, changed=0, reject=None, cands=[], support=None), None]
            continue
        for e, h in enumerate(Gs["held"]):
            if Gs["used"][e]:
                chi2[e] = chi2_of(pyoracle, orc, pg, x[h[0]], x[h[1]], h[2])
        rej, cands, support = gate_rule(Gs["held"], Gs["used"], chi2, chi2_max, min_support)
        if rej is not None:
            state[rej], rejected = 1, rejected + 1
        steps.append(dict(kind="gate", chi2=list(chi2), state=list(state), rejected=rejected, changed=int(rej is not None), reject=rej, cands=cands,
                          support=support))
        if rej is None:
            steps.append(None)
        else:
            x, Gs = solve(x)
    return steps


def deviation_of(x, group):
    """max |make_tf(x_k) - truth| over the group's nodes"""
    _, mk = lbc._lie()
    nodes = [r for r in range(B) if GROUP_OF[r] == group]
    return max(gc.deviation(mk(x[k]), fleet()["W"][r]) for k, r in enumerate(nodes))
