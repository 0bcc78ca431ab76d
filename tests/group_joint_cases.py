"""Cases of the joint pose graph of a group (include/liw_group_joint.h; tests/test_gpu_group_joint.py runs them on the device,
tests/test_group_joint_cases.py guards them on the host alone) and their host restatement: members, node offsets, the loop list, the
separator and segment lists, and the solve through oracle.pyoracle.posegraph_solve on the concatenated chains, with the constant
member's first sequential edge listed first (the oracle holds exactly that edge's index1 constant).

The fleet: B = 13 robots, K = 64 key frames at the most, G = 5 groups (the contents below need 13 robots, not fewer).  Every robot has
a true trajectory X_r[k] in the group frame (a planar arc of its wheel frame, so that the truth satisfies the ground factors), a world
W_r (planar), noisy sequential edges, and tracking poses P_r[k] integrated from them in its own world, so they drift; the back-end has
not solved, so its corrected poses are P.  Own loops and cross edges come from the truth with about 1 mm / 0.2 mrad of noise.
  group 0 (A)  robots 0, 1, 2 of 8, 12 and 10 key frames (robot 12 is in the group but NOT linked); robot 1 has one own loop; five cross
               edges, of which one names key frame 9 of robot 0 (8 key frames) and one has state 1: counts used and skipped
  group 1 (B)  robot 3 of 60 key frames (a stride separator at 48 and an interior segment of 47 frames), robot 4 of 5, robot 5 of
               exactly 1 key frame with a cross edge to it, robot 6 linked with 0 key frames (no member): separator and segment rules
  group 2 (C)  robot 7 alone, 20 key frames, two own loops, T_g_w not the identity: a single member
  group 3 (D)  robots 8, 9, 10 of 10 key frames, 12 cross edges on distinct end points: 24 + separators, the triangle runs from the
               work area only
  group 4 (E)  robot 11, never selected: nothing written
The anchors (fixed) are robots 0, 3, 7 and 8, the lowest of their groups; their T_g_w starts on the truth, the others' 2 cm / 5 mrad off.
"""
import functools
import math

import numpy as np

import group_graph_cases as gc
import loop_batch_cases as lbc
import loop_reference as ref

B, G, K, RL = 13, 5, 64, 2
MAX_MEMBERS, MAX_EDGES, MAX_NODES, MAX_LOOPS = 4, 12, 66, 12
GROUP_OF = [0, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3, 4, 0]
LINKED = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
FIXED = [1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 0]
NKF = [8, 12, 10, 60, 5, 1, 0, 20, 10, 10, 10, 6, 7]
GSEL = [1, 1, 1, 1, 0]
STRIDE = 48
SEQ_P, SEQ_Q = 4e-3, 2e-3              # noise of a sequential edge (metres, radians), uniform per axis: the drift
NOISE_P, NOISE_Q = 1e-3, 2e-4          # of own loops and cross edges
# own loops: robot -> [(index1, index2)]
OWN = {1: [(11, 2)], 7: [(19, 1), (12, 4)]}
# cross edges per group, in list order: (a, q, b, i, state)
CROSS = {
    0: [(0, 2, 1, 3, 0), (2, 8, 1, 10, 0), (0, 9, 2, 1, 0), (2, 2, 0, 6, 1), (1, 7, 2, 5, 0)],
    1: [(4, 0, 3, 0, 0), (4, 2, 3, 48, 0), (3, 55, 4, 3, 0), (4, 4, 3, 59, 0), (5, 0, 3, 52, 0), (4, 1, 5, 0, 0)],
    3: [(8, 0, 9, 1, 0), (8, 2, 10, 3, 0), (9, 3, 10, 5, 0), (9, 5, 8, 4, 0), (10, 7, 8, 6, 0), (10, 1, 9, 7, 0),
        (8, 8, 9, 9, 0), (9, 0, 10, 9, 0), (10, 0, 8, 1, 0), (8, 3, 9, 2, 0), (9, 4, 10, 2, 0), (10, 4, 8, 5, 0)],
    4: [],
}


def _planar(x, y, yaw):
    T = np.eye(4)
    T[:3, :3] = ref._exp_so3(np.array([0.0, 0.0, yaw]))
    T[:3, 3] = (x, y, 0.0)
    return T


@functools.lru_cache(maxsize=None)
def fleet():
    """-> dict(W [B] 4x4 truth T_g_w, X [B][n] 4x4 truth poses in the group frame, P [B][n] pose6 in the robot's world, seq [B][n-1] 4x4,
    own {robot: [(i1, i2, 4x4)]}, cross {group: [(a, q, b, i, state, 4x4)]}, T0 [B] 4x4 starting T_g_w)"""
    pose_of, mk = lbc._lie()
    rng = np.random.default_rng(41)
    Tiw_inv = ref.iso_inv(lbc.T_imu_to_wheel())
    W, X, P, seq, T0 = [], [], [], [], []
    for r in range(B):
        W.append(_planar(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.5, 0.5)))
        x, y, yaw, rate = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(0.01, 0.022) * (1 if r % 2 else -1)
        Xr = []
        for k in range(NKF[r]):
            Xr.append(_planar(x, y, yaw) @ Tiw_inv)
            x, y, yaw = x + 0.2 * math.cos(yaw), y + 0.2 * math.sin(yaw), yaw + rate
        X.append(Xr)
        S = [ref.iso_inv(Xr[k - 1]) @ Xr[k] @ gc._small(rng, SEQ_P, SEQ_Q) for k in range(1, NKF[r])]
        Pr = [ref.iso_inv(W[r]) @ Xr[0]] if Xr else []
        for s in S:
            Pr.append(Pr[-1] @ s)
        seq.append(S)
        P.append([pose_of(T) for T in Pr])
        T0.append(W[r] if FIXED[r] else W[r] @ gc._small(rng, gc.START_P, gc.START_Q))
    own = {r: [(i1, i2, ref.iso_inv(X[r][i1]) @ X[r][i2] @ gc._small(rng, NOISE_P, NOISE_Q)) for i1, i2 in ls] for r, ls in OWN.items()}
    cross = {}
    for g, ls in CROSS.items():
        cross[g] = []
        for a, q, b, i, st in ls:
            qq, ii = min(q, NKF[a] - 1), min(i, NKF[b] - 1)      # any measurement will do for an edge that is never used
            cross[g].append((a, q, b, i, st, ref.iso_inv(X[a][qq]) @ X[b][ii] @ gc._small(rng, NOISE_P, NOISE_Q)))
    return dict(W=W, X=X, P=P, seq=seq, own=own, cross=cross, T0=T0)


def backend_graph(r):
    """robot r's graph as FleetBackEnd.load_graph takes it"""
    F = fleet()
    ls = F["own"].get(r, [])
    return dict(poses=np.array(F["P"][r]).reshape(-1, 6), seq_tf12=np.array([gc.tf12_of(s) for s in F["seq"][r]]).reshape(-1, 12),
                loop_idx=np.array([[l[0], l[1]] for l in ls], dtype=np.int32).reshape(-1, 2), loop_tf12=np.array([gc.tf12_of(l[2]) for l in ls]).reshape(-1, 12))


# ---------------------------------------------------------------------------------------------------------------- restatement
def structure(group, max_members=MAX_MEMBERS, max_nodes=MAX_NODES, max_loops=MAX_LOOPS, group_of=None, linked=None, fixed=None, nkf=None, own=None,
              cross=None):
    """what liw_gjoint_solve makes of a group -> dict(flags (the header words by name), members, offsets, const_node, loops [(node1, node2,
    4x4)], separators, segments [(a, b)], solved)"""
    F = fleet()
    group_of, linked, fixed, nkf = group_of or GROUP_OF, linked or LINKED, fixed or FIXED, nkf or NKF
    own = F["own"] if own is None else own
    cross = F["cross"].get(group, []) if cross is None else cross
    members = [r for r in range(len(group_of)) if group_of[r] == group and linked[r] and nkf[r] >= 1]
    fl = dict(members_full=0, nodes_full=0, loops_full=0, members=len(members), nodes=0, seq_edges=0, own_loops=0, used=0, skipped=0, separators=0,
              solved=0, const_node=0)
    out = dict(flags=fl, members=[], offsets=[], const_node=0, loops=[], separators=[], segments=[], solved=False)
    if len(members) > max_members:
        fl["members_full"] = 1
        return out
    offsets = [int(v) for v in np.cumsum([0] + [nkf[r] for r in members])]
    N = offsets[-1]
    out.update(members=members, offsets=offsets[:-1])
    fl["nodes"] = N
    if N > max_nodes:
        fl["nodes_full"] = 1
        return out
    off = dict(zip(members, offsets))
    loops = [(off[r] + i1, off[r] + i2, T) for r in members for i1, i2, T in own.get(r, [])]
    n_own = len(loops)
    for a, q, b, i, st, T in cross:
        if a != b and a in off and b in off and 0 <= q < nkf[a] and 0 <= i < nkf[b] and st == 0:
            loops.append((off[a] + q, off[b] + i, T))
    fl.update(seq_edges=N - len(members), own_loops=n_own, used=len(loops) - n_own, skipped=len(cross) - (len(loops) - n_own))
    if len(loops) > max_loops:
        fl["loops_full"] = 1
        return out
    fx = [r for r in members if fixed[r]]
    cm = fx[0] if fx else (members[0] if members else None)
    cn = off[cm] if members else 0
    ends = {n for l in loops for n in l[:2]}
    sep, chain = [], []
    for r in members:
        for k in range(nkf[r]):
            n = off[r] + k
            chain.append(r)
            if k == 0 or k == nkf[r] - 1 or k % STRIDE == 0 or n == cn or n in ends:
                sep.append(n)
    segments = [(a, b) for a, b in zip(sep, sep[1:]) if chain[a] == chain[b]]
    solved = N >= 2 and (N - len(members)) + len(loops) >= 1
    fl.update(separators=len(sep), solved=int(solved), const_node=cn)
    out.update(const_node=cn, const_member=cm, loops=loops, separators=sep, segments=segments, solved=solved, chain=chain)
    return out


def start_x(group, T0=None, P=None):
    """x0 [N, 6] = log_SE3(T_g_w * make_tf(P)) of the group's nodes, on the host"""
    pose_of, mk = lbc._lie()
    F = fleet()
    T0, P = F["T0"] if T0 is None else T0, F["P"] if P is None else P
    return np.array([pose_of(T0[r] @ mk(p)) for r in structure(group)["members"] for p in P[r]]).reshape(-1, 6)


def oracle_solve(pyoracle, orc, pg, group, x0=None, max_iters=0, **kw):
    """the joint solve through the oracle: the chains concatenated, the constant member's first sequential edge first -> x [N, 6], summary"""
    F = fleet()
    S = structure(group, **kw)
    x0 = start_x(group) if x0 is None else x0
    off = dict(zip(S["members"], S["offsets"]))
    order = [S["const_member"]] + [r for r in S["members"] if r != S["const_member"]]
    idx, tf = [], []
    for r in order:
        for k, s in enumerate(F["seq"][r]):
            idx.append((off[r] + k, off[r] + k + 1))
            tf.append(gc.tf12_of(s))
    assert idx and idx[0][0] == S["const_node"], "the constant member needs a sequential edge to be the oracle's constant node"
    li = np.array([[l[0], l[1]] for l in S["loops"]], dtype=np.int32).reshape(-1, 2)
    lt = np.array([gc.tf12_of(l[2]) for l in S["loops"]]).reshape(-1, 12)
    return pyoracle.posegraph_solve(orc, pg, np.array(x0, dtype=np.float64), np.array(idx, dtype=np.int32), np.array(tf), li if len(li) else None,
                                    lt if len(li) else None, max_iters=max_iters)


def ggraph_lists(group):
    """the held cross edges of a group as tests/group_graph_cases.py's restatement takes them; state-1 edges are no part of a solve"""
    cr = [c for c in fleet()["cross"].get(group, []) if c[4] == 0]
    return dict(edges=[(a, q, b, i, 20) for a, q, b, i, st, T in cr], tf12=[gc.tf12_of(T) for a, q, b, i, st, T in cr])


def rigid_T(pyoracle, orc, pg, group):
    """T_g_w [B] 4x4 after the group graph's solve (tests/group_graph_cases.py's restatement through the oracle) from the cases' start"""
    _, mk = lbc._lie()
    F = fleet()
    Gr = gc.graph_of(ggraph_lists(group), group, GROUP_OF, LINKED, FIXED, NKF, F["P"])
    x, sm = gc.oracle_solve(pyoracle, orc, pg, gc.start_x(Gr["nodes"], F["T0"]), Gr["edges"], Gr["const"].index(1))
    T = list(F["T0"])
    for k, r in enumerate(Gr["nodes"]):
        T[r] = mk(x[k])
    return T, sm


def position_errors(group, x):
    """|position - truth| of every node of the group for poses x [N, 6] (group frame)"""
    F = fleet()
    truth = np.array([Xk[:3, 3] for r in structure(group)["members"] for Xk in F["X"][r]])
    return np.linalg.norm(np.asarray(x)[:, :3] - truth, axis=1)


def rigid_errors(group, T):
    _, mk = lbc._lie()
    F = fleet()
    x = np.array([(T[r] @ mk(p))[:3, 3] for r in structure(group)["members"] for p in F["P"][r]])
    truth = np.array([Xk[:3, 3] for r in structure(group)["members"] for Xk in F["X"][r]])
    return np.linalg.norm(x - truth, axis=1)
