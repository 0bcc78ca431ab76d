"""Inputs that send the rotation logarithm (`log_SO3`, csrc/liw_dual.hpp) through its second half — shared by
tests/test_oracle_large_rotation.py and tests/test_gpu_large_rotation.py.

`log_SO3` builds a quaternion from the matrix.  With trace > 0 it divides by sqrt(trace + 1).  With trace <= 0 (rotation angle above
120 deg) it picks the largest diagonal entry i (the PIVOT), j = i + 1, k = j + 1 (mod 3), reads six off-diagonal entries through
select tables, and gets the scalar part as cw = (R[k,j] - R[j,k]) / (2 sqrt(..)).  cw < 0 (the pivot's axis component is negative)
takes the cos_theta < 0 arm of QuaternionToAngleAxis, whose raw angle 2 atan2(-s, -c) lies beyond pi and is brought back by
normalize_so3 (the WRAP).  So there are seven arms: trace > 0, and (pivot 0 / 1 / 2) x (cw > 0 / cw < 0).

Every builder returns, next to its data, a CLASSIFICATION of each rotation matrix the code under test will take the logarithm of —
trace, pivot, sign of R[k,j] - R[j,k], angle, gap between the two largest diagonal entries — computed here with numpy alone,
independently of product and oracle.  `assert_margins` keeps every such matrix clear of the decision boundaries (so that two correct
implementations cannot pick different arms), `assert_coverage` requires all seven arms among them.
"""
import numpy as np

PI = float(np.pi)
TRACE_MARGIN = 0.1        # |trace| >= 0.1: the trace > 0 / <= 0 decision is not a matter of round-off
DIAG_MARGIN = 0.1         # the two largest diagonal entries >= 0.1 apart: neither is the pivot
ANGLE_MARGIN = 0.01       # angle <= pi - 0.01: beyond that the sign of the axis is ill-defined in the reference itself


# ---------------------------------------------------------------- numpy-only SO3
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    K = hat(w)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def log_so3(R):
    """rotation vector of R, angle in [0, pi) (the builders stay ANGLE_MARGIN below pi, where the antisymmetric part gives the axis)"""
    c = max(-1.0, min(1.0, (float(np.trace(R)) - 1.0) * 0.5))
    th = float(np.arccos(c))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-10:
        return 0.5 * v
    assert PI - th > 1e-6
    return v * (th / (2.0 * np.sin(th)))


def turn(angle, axis):
    """rotation vector of `angle` about `axis` (normalised here)"""
    a = np.asarray(axis, dtype=np.float64)
    return angle * a / np.linalg.norm(a)


def extrinsic_rotation(T16):
    """rotation of a 4x4 extrinsic projected onto SO3 (what normalize_extrinsics does)"""
    U, _, Vt = np.linalg.svd(np.asarray(T16, dtype=np.float64).reshape(4, 4)[:3, :3])
    return U @ Vt


# ---------------------------------------------------------------- classification
def classify(R, **tags):
    """Which arm of log_SO3 the matrix R takes: dict(trace, pivot, cw_sign, angle, diag_gap, arm) + the caller's tags.
    arm = "pos" (trace > 0) or (pivot, cw_sign)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    d = np.diag(R)
    tr = float(d.sum())
    i = int(np.argmax(d))
    j, k = (i + 1) % 3, (i + 2) % 3
    num = float(R[k, j] - R[j, k])
    ds = np.sort(d)
    out = dict(trace=tr, pivot=i, cw_sign=(1 if num > 0 else -1), cw_num=num, diag_gap=float(ds[2] - ds[1]),
               angle=float(np.arccos(max(-1.0, min(1.0, (tr - 1.0) * 0.5)))))
    out["arm"] = "pos" if tr > 0.0 else (i, out["cw_sign"])
    out["wrapped"] = bool(tr <= 0.0 and num < 0.0)          # cos_theta < 0: raw angle beyond pi, normalize_so3 brings it back
    out.update(tags)
    return out


ALL_ARMS = frozenset(["pos"] + [(i, s) for i in range(3) for s in (1, -1)])


def assert_margins(classes):
    """conditions on the INPUTS, for every classified matrix: no block is exempt.  (The diagonal gap matters where a pivot is
    chosen, trace <= 0; with trace > 0 the diagonal is only summed — the three entries of a small rotation are all ~1.)"""
    for c in classes:
        assert abs(c["trace"]) >= TRACE_MARGIN, c
        assert c["angle"] <= PI - ANGLE_MARGIN, c
        if c["trace"] <= 0.0:
            assert c["diag_gap"] >= DIAG_MARGIN, c
    return True


def assert_coverage(classes, wrapped=False):
    """trace > 0, and trace <= 0 with each pivot and both signs of cw, all present; wrapped: at least one whose angle wrapped"""
    arms = {c["arm"] for c in classes}
    assert arms == ALL_ARMS, "arms missing from the inputs: %s" % sorted(map(str, ALL_ARMS - arms))
    if wrapped:
        assert any(c["wrapped"] for c in classes)
    return True


def by_role(classes, role):
    return [c for c in classes if c.get("role") == role]


# ---------------------------------------------------------------- windows
# the relative block rotations of the per-factor window, in this order so that the lanes of one wave take different arms
# (None = leave the block's small relative rotation as make_window drew it)
FACTOR_TURNS = (None, turn(2.2, (1, 0, 0)), turn(2.6, (0, 1, 0)), turn(3.0, (0, 0, 1)), turn(3.13, (0, 0, -1)), None,
                turn(2.3, (-1, .1, .1)), turn(2.8, (.1, -1, .1)), None)
FACTOR_WHEEL_ALONG = (1, 3, 6)


def _sync_match_pose(d):
    d["match_pose"] = np.array(d["match_pose"], dtype=np.float64, copy=True)
    d["match_pose"][:, 0:6] = d["states"][0, 0:6]
    d["match_pose"][:, 6:12] = d["states"][:, 0:6]


def window_classes(d, prm, blocks=None, **tags):
    """classification of the three matrices log_SO3 sees in IMU / wheel block k (frames k, k + 1) at the window's states:
    role "imu": exp(-gamma) R_k^T R_k+1 (gamma corrected for the gyro bias as the factor does), role "wheel": the relative rotation of
    the wheel frames, role "oq": the measured wheel increment (plain doubles)."""
    st = np.asarray(d["states"], dtype=np.float64).reshape(-1, 15)
    Riw = extrinsic_rotation(prm["T_imu_to_wheel"])
    out = []
    for k in (range(st.shape[0] - 1) if blocks is None else blocks):
        Ri, Rj = exp_so3(st[k, 3:6]), exp_so3(st[k + 1, 3:6])
        X, J = np.asarray(d["imu_X"])[k], np.asarray(d["imu_J"])[k].reshape(15, 15)
        gamma = X[6:9] + J[6:9, 12:15] @ (st[k, 12:15] - X[12:15])
        out.append(classify(exp_so3(-gamma) @ Ri.T @ Rj, role="imu", block=k, **tags))
        out.append(classify(Riw.T @ Ri.T @ Rj @ Riw, role="wheel", block=k, **tags))
        out.append(classify(np.asarray(d["wheel_T"])[k][:9].reshape(3, 3), role="oq", block=k, **tags))
    return out


def turned_window(d, prm, turns, wheel_along=()):
    """Copy of the make_window result `d` whose block k (frames k, k + 1) has the relative rotation exp(gamma_k) exp(turns[k]):
    frame k+1's rotation becomes log(R_k exp(gamma_k) exp(a)), so the IMU residual rotation exp(-gamma) R_k^T R_k+1 is exp(a) and the
    wheel role sees the same angle about the axis carried into the wheel frame.  turns[k] None keeps the block's own relative rotation
    (the later frames turn along).  wheel_along: blocks whose measured increment wheel_T[k] is rotated by the same `a`, so that `oq`
    takes the arm too.  Positions stay, the laser_match poses follow the states.  -> (window, classification)"""
    w = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    st0 = np.asarray(d["states"], dtype=np.float64).reshape(-1, 15)
    st = st0.copy()
    n = st.shape[0]
    assert len(turns) == n - 1
    R_new = exp_so3(st0[0, 3:6])
    for k in range(n - 1):
        a = turns[k]
        if a is None:
            rel = exp_so3(st0[k, 3:6]).T @ exp_so3(st0[k + 1, 3:6])
        else:
            X, J = np.asarray(d["imu_X"])[k], np.asarray(d["imu_J"])[k].reshape(15, 15)
            gamma = X[6:9] + J[6:9, 12:15] @ (st0[k, 12:15] - X[12:15])
            rel = exp_so3(gamma) @ exp_so3(a)
            if k in wheel_along:
                T = w["wheel_T"][k]
                T[:9] = (T[:9].reshape(3, 3) @ exp_so3(a)).reshape(9)
        R_new = R_new @ rel
        st[k + 1, 3:6] = log_so3(R_new)
    w["states"] = st
    _sync_match_pose(w)
    return w, window_classes(w, prm)


def factor_window(synth, preint, prm, seed=5, n=10, L=40, shift=0):
    """the per-factor window: FACTOR_TURNS (cyclically shifted by `shift`, cut or repeated to n - 1 blocks) on make_window(seed, n, L);
    the increment of every third block (those FACTOR_WHEEL_ALONG names, carried along by the shift) is rotated too"""
    d = synth.make_window(preint, prm, seed=seed, n=n, L=L)
    m = len(FACTOR_TURNS)
    turns = [FACTOR_TURNS[(shift + k) % m] for k in range(n - 1)]
    along = [k for k in range(n - 1) if (shift + k) % m in FACTOR_WHEEL_ALONG]
    return turned_window(d, prm, turns, along)


KIDNAP_AXIS = np.array([0.05, -0.03, 1.0]) / np.linalg.norm([0.05, -0.03, 1.0])


def kidnapped_heading(d, prm, yaw, first=None):
    """Copy of `d` whose frames n // 2 ... are turned by `yaw` about KIDNAP_AXIS (R_k <- R_k exp(yaw axis)): a solver started from a bad
    heading.  The block in front of the first turned frame sees the whole turn.  -> (window, classification of that block)"""
    w = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    st = np.array(d["states"], dtype=np.float64, copy=True).reshape(-1, 15)
    n = st.shape[0]
    first = n // 2 if first is None else first
    D = exp_so3(yaw * KIDNAP_AXIS)
    for k in range(first, n):
        R = exp_so3(st[k, 3:6]) @ D
        st[k, 3:6] = log_so3(R)
    w["states"] = st
    w["match_pose"] = np.array(d["match_pose"], dtype=np.float64, copy=True)
    w["match_pose"][first:, 6:12] = st[first:, 0:6]            # the frames' own initial guesses; the reference pose (frame 0's, never turned) stays
    return w, [c for c in window_classes(w, prm, blocks=[first - 1]) if c["role"] != "oq"]


def states_classes(x, d, prm):
    """classification of the IMU and wheel rotations of EVERY block at the states x [n, 15] (an LM iterate of window d)"""
    w = dict(d)
    w["states"] = np.asarray(x, dtype=np.float64).reshape(-1, 15)
    return [c for c in window_classes(w, prm) if c["role"] != "oq"]


# ---------------------------------------------------------------- pre-integration intervals
# (total rotation, axis): 2 s / 400-sample constant-rate turns.  The last entry is not in the issue's list: without it no interval
# ends (or passes) with pivot 0 and cw < 0
SPINS = ((2.2, (1, 0, 0)), (2.2, (0, 1, 0)), (2.2, (0, 0, 1)), (3.0, (0, 0, 1)), (3.3, (0, 0, 1)), (3.3, (.1, 1, .1)), (5.0, (0, 0, -1)),
         (6.5, (.05, .05, 1)), (2.2, (-1, 0, 0)))


def spin_intervals(total, axis, seed=0, span=2.0, cnt=400, t0=3.0):
    """IMU and wheel sample arrays of a constant-rate turn of `total` rad about `axis` over `span` seconds, `cnt` samples each.
    -> dict(imu=(samples[cnt, 7], t_start, t_end, bias6), wheel=(samples[cnt, 13], t_start, t_end), classes=[...], steps=[...])
    classes: the NOMINAL end rotation exp(total axis) of either accumulator (the gyro noise and the discretisation move it by far less
    than the margins; the tests check the distance).  steps: the nominal rotation after every IMU sample — the matrices the IMU
    accumulator takes the logarithm of on the way (they cross every boundary on purpose: next to one, either arm gives the same vector)."""
    rng = np.random.default_rng(seed)
    u = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = t0 + span * np.arange(cnt) / cnt
    t_start, t_end = float(t[0] + 0.001), float(t[-1] + 0.002)
    rate = total / (t_end - t_start)
    bias = rng.normal(0.0, 1e-2, 6)
    s = np.zeros((cnt, 7))
    s[:, 0] = t
    s[:, 1:4] = rng.normal(0.0, 0.3, (cnt, 3)) + np.array([0.0, 0.0, 9.8])
    s[:, 4:7] = rate * u + bias[3:6] + rng.normal(0.0, 1e-3, (cnt, 3))
    ws = np.zeros((cnt, 13))
    ws[:, 0] = t
    for m in range(cnt):
        ws[m, 1:10] = exp_so3(rate * (t[m] - t_start) * u).reshape(9)
        ws[m, 10:13] = 0.3 * (t[m] - t_start) * np.array([1.0, 0.2, 0.0]) + rng.normal(0.0, 2e-4, 3)
    tags = dict(total=total, axis=tuple(axis))
    steps = [classify(exp_so3(total * (m + 1) / cnt * u), role="step", **tags) for m in range(cnt)]
    return dict(imu=(s, t_start, t_end, bias), wheel=(ws, t_start, t_end), total=total, axis=u,
                classes=[classify(exp_so3(total * u), role="end", **tags)], steps=steps)


# ---------------------------------------------------------------- pose graph
def loop_edge_classes(poses, idx, tf12, **tags):
    """classification of the error rotation R_j^T R_i R12 of every edge (i, j) = idx[e] (edge_factor: tf_j^-1 tf_i tf12)"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    out = []
    for e, (i, j) in enumerate(np.asarray(idx).reshape(-1, 2)):
        R12 = np.asarray(tf12, dtype=np.float64).reshape(-1, 12)[e][:9].reshape(3, 3)
        out.append(classify(exp_so3(poses[j, 3:6]).T @ exp_so3(poses[i, 3:6]) @ R12, edge=e, **tags))
    return out


def turned_loop_edges(tf12, turns):
    """copy of the edge measurements tf12 [E, 12] with the rotation of edge e right-multiplied by exp(turns[e]) (a dict)"""
    out = np.array(tf12, dtype=np.float64, copy=True).reshape(-1, 12)
    for e, a in turns.items():
        out[e, :9] = (out[e, :9].reshape(3, 3) @ exp_so3(a)).reshape(9)
    return out


PG_LOOP_TURNS = (turn(2.6, (1, 0, 0)), turn(2.6, (-1, 0, 0)), turn(2.6, (0, 1, 0)), turn(2.6, (0, -1, 0)), turn(3.0, (0, 0, 1)),
                 turn(3.0, (0, 0, -1)))


def turned_pose_graph(G):
    """make_pose_graph(N, n_loop=6) result -> the graph of the large-rotation pose-graph tests + classification of every edge:
    one loop edge per pivot and sign, sequential edge 11 turned by 2.4 about (.1, -.2, 1), a turned loop edge on the constant key
    frame, and loop edge 2 once more in the reverse direction (inverse transform, indices swapped)."""
    G = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in G.items()}
    assert len(G["loop_idx"]) == 6
    N, const = int(G["N"]), int(G["seq_idx"][0, 0])
    G["loop_tf12"] = turned_loop_edges(G["loop_tf12"], dict(enumerate(PG_LOOP_TURNS)))
    G["seq_tf12"] = turned_loop_edges(G["seq_tf12"], {11: turn(2.4, (.1, -.2, 1))})
    # last key frame -> the constant one: their relative pose at the initial estimate, turned by 2.7 about (.1, 1, .1)
    Rl, Rc = exp_so3(G["poses"][N - 1, 3:6]), exp_so3(G["poses"][const, 3:6])
    on_const = np.concatenate([(Rl.T @ Rc).reshape(9), Rl.T @ (G["poses"][const, 0:3] - G["poses"][N - 1, 0:3])])[None, :]
    on_const = turned_loop_edges(on_const, {0: turn(2.7, (.1, 1, .1))})
    rev = G["loop_tf12"][2]
    R = rev[:9].reshape(3, 3)
    rev = np.concatenate([R.T.reshape(9), -R.T @ rev[9:12]])
    G["loop_idx"] = np.vstack([G["loop_idx"], [[N - 1, const]], [G["loop_idx"][2][::-1]]]).astype(np.int32)
    G["loop_tf12"] = np.vstack([G["loop_tf12"], on_const, rev[None, :]])
    cls = loop_edge_classes(G["poses"], G["loop_idx"], G["loop_tf12"], kind="loop") + loop_edge_classes(G["poses"], G["seq_idx"], G["seq_tf12"], kind="seq")
    return G, cls


def sub_window(d, lo, m=2):
    """frames lo .. lo + m - 1 of window `d` as an m-frame window (their states, laser_match poses and laser blocks, the IMU and wheel
    blocks between them): the window the tracking front-end holds"""
    N = int(d["n"])
    o = dict(d)
    o["n"] = m
    for k in ("states", "match_pose", "truth_states"):
        o[k] = np.asarray(d[k]).reshape(N, -1)[lo:lo + m].copy()
    o["has_match"] = np.asarray(d["has_match"])[lo:lo + m].copy()
    for k in ("imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP", "wheel_Dt"):
        o[k] = np.asarray(d[k])[lo:lo + m - 1].copy()
    lf = np.asarray(d["laser_frame"])
    msk = (lf >= lo) & (lf < lo + m)
    o["laser_frame"] = (lf[msk] - lo).astype(np.int32)
    o["laser_pts"] = np.asarray(d["laser_pts"])[msk].copy()
    return o


# ---------------------------------------------------------------- solves that pass through the arms
KIDNAP_CASES = ((42, 6, 60, -2.9, 8), (44, 8, 100, 3.0, 10))          # (seed, n, L, yaw, LM iteration cap), INIT topology
# the same windows kidnapped the other way: the second turned base window of the batched solves (other sign of cw in the same batch)
KIDNAP_MIRRORS = tuple((seed, n, L, -yaw, cap) for seed, n, L, yaw, cap in KIDNAP_CASES)
TRACK_CASES = ((51, 2.5, 10), (52, -2.9, 10))                          # (seed, yaw of the newest frame, cap), TRACK topology


def kidnapped_case(synth, preint, prm, seed, n, L, yaw):
    return kidnapped_heading(synth.make_window(preint, prm, seed=seed, n=n, L=L), prm, yaw)


def track_case(synth, pyoracle, orc, prm, seed, yaw, n=4, L=60, nudge=0.0):
    """Two-frame tracking window whose newest frame is turned by `yaw` (and moved by `nudge` metres along every axis), with the prior the
    oracle's marginalisation of the UNTURNED n-frame window (after its init solve) leaves on the older frame.
    -> (window, prior (X, J, R), classification)"""
    d = synth.make_window(orc, prm, seed=seed, n=n, L=L)
    wo = pyoracle.Window(d)
    orc.set_prior(None)
    orc.set_max_iterations(50)
    orc.init_solve(wo)
    orc.marginalization(wo)
    prior = tuple(np.array(v, copy=True) for v in orc.get_prior())
    orc.set_prior(None)
    full = dict(d)
    full["states"], full["match_pose"] = wo["states"].reshape(n, 15).copy(), wo["match_pose"].reshape(n, 12).copy()
    w, cls = kidnapped_heading(sub_window(full, n - 2), prm, yaw, first=1)
    w["states"][1, 0:3] += nudge
    w["match_pose"][1, 6:9] += nudge
    return w, prior, cls


def track_solve_sensitivity(pyoracle, orc, win, prior, its, trials=3, eps=1e-13, seed=7):
    """parity_util.init_solve_sensitivity for the tracking solve: the oracle against itself with the pre-integrated IMU means scaled
    by 1 + eps N(0, 1), per LM iteration (inf where a perturbed run takes another number of iterations)"""
    sens, rp = np.zeros(len(its)), np.random.default_rng(seed)
    for _ in range(trials):
        alt = dict(win)
        alt["imu_X"] = np.asarray(win["imu_X"]) * (1.0 + eps * rp.standard_normal(np.asarray(win["imu_X"]).shape))
        wa = pyoracle.Window(alt)
        orc.set_prior(prior)
        orc.solve(wa)
        ia = orc.iterations()
        for it in range(min(len(its), len(ia))):
            d = np.abs(ia[it]["x"] - its[it]["x"]).max() / max(np.abs(its[it]["x"]).max(), 1e-12)
            sens[it] = max(sens[it], float(d))
        if len(ia) != len(its):
            sens[min(len(ia), len(its)):] = np.inf
    orc.set_prior(None)
    return sens


def iterations_beyond_120_degrees(its, d, prm):
    """how many of the oracle's LM iterates (orc.iterations()) hold a block whose IMU or wheel rotation has trace <= 0"""
    n = int(d["n"])
    return sum(any(c["trace"] <= 0.0 for c in states_classes(it["x"].reshape(n, 15), d, prm)) for it in its)


def small_intervals(seed=7):
    """the ragged short IMU intervals of tests/test_gpu_preint.py (1, 2, 5 and 41 samples, random rates) and wheel intervals of the same
    sample counts -> (imu tuples, wheel tuples)"""
    rng = np.random.default_rng(seed)
    imu, wheel = [], []
    for cnt, span in ((1, 0.004), (2, 0.011), (5, 0.03), (41, 0.2)):
        t = 3.0 + np.sort(rng.uniform(0.0, span, cnt))
        s = np.zeros((cnt, 7))
        s[:, 0] = t
        s[:, 1:4] = rng.normal(0.0, 1.0, (cnt, 3)) + np.array([0.0, 0.0, 9.8])
        s[:, 4:7] = rng.normal(0.0, 0.5, (cnt, 3))
        imu.append((s, float(t[0] + 0.001), float(t[-1] + 0.002), rng.normal(0.0, 1e-2, 6)))
        wheel.append(spin_intervals(0.3 * 10.0 * span, (0.02, -0.01, 1), seed=seed + cnt, span=10.0 * span, cnt=cnt)["wheel"])
    return imu, wheel
