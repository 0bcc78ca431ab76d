"""The SECOND parameter set of the parity tests (tests/test_second_config.py on the CPU, tests/test_gpu_second_config.py on the GPU).

synth.office_params() has four isotropic IMU noise vectors, extrinsic rotations within a few degrees of signed permutation matrices and one
value per scalar, so whole classes of kernel error cannot fail a test that uses it: dt^2 Rz diag(q_na) Rz^T is q dt^2 I whatever Rz is, a
constant folded into a packed record equals the parameter, a transposed extrinsic moves results by little.  `skewed_params` differs from it
in every scalar, has three distinct components per vector, generic extrinsic rotations and a laser matrix that is not orthonormal, so the
quaternion round trip of the parameter loader (reference src/utilies/params.cpp:44-54) does work.

A helper module, not a conftest: it holds the configuration, the inputs the two test modules share and the mutated restatements with
which the CPU guards show that these inputs would expose each class of mistake.  Everything here is numpy.

Its second half holds the sets of the FRONT half — laser_params (a 138 x 83 grid, no two scalars equal, ref_n_accumulation = 5),
loop_params (a_res != d_res, max_dis != max_tf_p) — and the laser scene that tests/test_second_config_frontend.py (CPU guards) and
tests/test_gpu_laser_second_config.py share; the loop detector and map tests take skewed_params for their extrinsics."""
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

WHEEL_TURN, WHEEL_T = (0.21, -0.17, 0.4), (0.13, 0.71, -0.35)
LASER_TURN, LASER_T = (-0.3, 0.25, -0.6), (-0.09, 0.05, 0.21)
LASER_SKEW = 1.002 * np.eye(3) + 1e-3 * np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [0.5, 0.0, 0.0]])
SCALARS = dict(g=9.78, line_to_line_sigma=0.0025, manifold_p_sigma=0.02, manifold_q_sigma=0.0012)
VECTORS = dict(imu_noise_acc_sigma=[0.011, 0.0163, 0.031], imu_bias_acc_sigma=[0.0031, 0.00499, 0.0082],
               imu_noise_gyro_sigma=[0.0021, 0.003208, 0.0057], imu_bias_gyro_sigma=[0.00031, 0.000499, 0.00088],
               wheel_sigma=[0.3, 5000.0, 120.0])
NOISE_VECTORS = ("imu_noise_acc_sigma", "imu_bias_acc_sigma", "imu_noise_gyro_sigma", "imu_bias_gyro_sigma")
PG = dict(loop_sigma_p=[0.2, 0.1, 0.3], loop_sigma_q=[0.02, 0.01, 0.03], loop_edge_k=4.0)
SEEDS = (1, 2, 3)                       # the windows of the short solves: synth.make_window(orc, prm, seed, n, L = 4 n)
SOLVE_SHAPES = ((6, 24), (12, 48))
SOLVE_CAP = 8                           # LM iteration cap of the batched solves


def golden_modules():
    """(make_golden, make_golden_solver): the committed torch / numpy restatements"""
    import make_golden
    import make_golden_solver
    return make_golden, make_golden_solver


def _matrix16(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return [float(v) for v in T.reshape(16)]


def skewed_params(synth, normalized=True):
    """A dict with the keys of synth.office_params().  The extrinsic rotations are the office ones (through the loader's quaternion round
    trip) right-multiplied by generic rotations of 0.48 and 0.72 rad, with other translations; the laser rotation is multiplied by
    LASER_SKEW on top, so it is a per cent off orthonormal and normalize_extrinsics = True changes it.  normalized = False: the matrices
    that round trip gives, with normalize_extrinsics = False — the same solver-side parameters through the other loader path."""
    mg, _ = golden_modules()
    off = synth.office_params()
    Rw = mg.quat_round_trip(np.asarray(off["T_imu_to_wheel"]).reshape(4, 4)[:3, :3]) @ synth.exp_so3(np.array(WHEEL_TURN))
    Rl = mg.quat_round_trip(np.asarray(off["T_imu_to_laser"]).reshape(4, 4)[:3, :3]) @ synth.exp_so3(np.array(LASER_TURN)) @ LASER_SKEW
    if not normalized:
        Rw, Rl = mg.quat_round_trip(Rw), mg.quat_round_trip(Rl)
    prm = dict(off, T_imu_to_wheel=_matrix16(Rw, WHEEL_T), T_imu_to_laser=_matrix16(Rl, LASER_T), normalize_extrinsics=bool(normalized))
    prm.update(SCALARS)
    prm.update({k: list(v) for k, v in VECTORS.items()})
    return prm


def solver_rotations(prm):
    """(Riw, Ril) as the solver holds them: through the round trip when normalize_extrinsics is set, as given otherwise"""
    mg, _ = golden_modules()
    out = []
    for key in ("T_imu_to_wheel", "T_imu_to_laser"):
        R = np.asarray(prm[key], dtype=np.float64).reshape(4, 4)[:3, :3]
        out.append(mg.quat_round_trip(R) if prm.get("normalize_extrinsics", True) else R.copy())
    return out


def rotation_distance(synth, Ra, Rb):
    """angle of Ra^T Rb after projecting both onto SO3"""
    pa, pb = (synth.normalize_extrinsic(synth.se3(R, np.zeros(3)).reshape(16))[:3, :3] for R in (Ra, Rb))
    return float(np.linalg.norm(synth.log_so3(pa.T @ pb)))


class Recorder:
    """preint provider for synth.make_window that records every interval and delegates to `inner`"""

    def __init__(self, inner):
        self.inner, self.imu, self.wheel = inner, [], []

    def imu_preint(self, samples, t_start, t_end, bias6):
        self.imu.append((np.array(samples), float(t_start), float(t_end), np.array(bias6)))
        return self.inner.imu_preint(samples, t_start, t_end, bias6)

    def wheel_preint(self, samples, t_start, t_end):
        self.wheel.append((np.array(samples), float(t_start), float(t_end)))
        return self.inner.wheel_preint(samples, t_start, t_end)


def preint_intervals(synth, preint, prm):
    """The pre-integration inputs: the set of tests/test_gpu_preint.py generated at `prm` — three recorded n = 9 windows and the ragged
    1 / 2 / 5 / 41 / 400-sample intervals, M = 29: the last wave of k_preint_imu is partly filled — followed by the nine 400-sample spin
    intervals of large_rotation_cases.SPINS.  -> (imu tuples [38], wheel tuples [33])"""
    import large_rotation_cases as lr
    rec = Recorder(preint)
    for k in range(3):
        synth.make_window(rec, prm, seed=900 + k, n=9, L=0)
    rng = np.random.default_rng(7)
    for cnt, span in ((1, 0.004), (2, 0.011), (5, 0.03), (41, 0.2), (400, 2.0)):
        t = 3.0 + np.sort(rng.uniform(0.0, span, cnt))
        s = np.zeros((cnt, 7))
        s[:, 0] = t
        s[:, 1:4] = rng.normal(0.0, 1.0, (cnt, 3)) + np.array([0.0, 0.0, prm["g"]])
        s[:, 4:7] = rng.normal(0.0, 0.5, (cnt, 3))
        rec.imu.append((s, float(t[0] + 0.001), float(t[-1] + 0.002), rng.normal(0.0, 1e-2, 6)))
    assert len(rec.imu) == 29
    for i, (tot, ax) in enumerate(lr.SPINS):
        sp = lr.spin_intervals(tot, ax, seed=i)
        rec.imu.append(sp["imu"])
        rec.wheel.append(sp["wheel"])
    return rec.imu, rec.wheel


def wheel_interval_with_three_weights(wheel):
    """A wheel interval whose translation and rotation are both above the 5 mm / 5 mrad floors of wheel_odom_preintegration.h:140-146,
    so sqrt_inverse_P = diag(1 / (s0 |dp|), 1 / (s1 |dp|), 1 / (s2 |dq|)): with the three distinct wheel_sigma its entries are in the
    known ratios s1 / s0 (first two) and differ in the third.  -> index into `wheel` of the first spin interval (0.6 m, 2.2 rad)"""
    return len(wheel) - 9


def track_window(synth, pyoracle, orc, prm, seed, n=4, L=16, nudge=0.01):
    """Two-frame tracking window with a carried prior: the last two frames of an n-frame window after the oracle's init solve, the newest
    frame moved by `nudge` metres along every axis, and the prior the oracle's marginalisation of the n-frame window leaves on the
    older frame.  -> (window, prior (X, J, R))"""
    import large_rotation_cases as lr
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
    w = lr.sub_window(full, n - 2)
    w["states"][1, 0:3] += nudge
    w["match_pose"][1, 6:9] += nudge
    return w, prior


# ---------------------------------------------------------------- mutated restatements (CPU guards only)
def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def noise_mutations(prm):
    """name -> (parameter dict, noise_rotation) of imu_preint_numpy: each sigma vector reversed in turn, and Rz^T for Rz in G"""
    out = {"reversed " + k: (dict(prm, **{k: list(prm[k])[::-1]}), None) for k in NOISE_VECTORS}
    out["Rz^T in G"] = (prm, lambda Rz: Rz.T)
    return out


def sqrtP_moves(prm, imu):
    """for every mutation of noise_mutations: the largest relative change of sqrt_inverse_P over the intervals `imu`"""
    _, mgs = golden_modules()
    base = [mgs.imu_preint_numpy(prm, *iv)[2] for iv in imu]
    return {name: max(relerr(mgs.imu_preint_numpy(p, *iv, noise_rotation=rot)[2], b) for iv, b in zip(imu, base))
            for name, (p, rot) in noise_mutations(prm).items()}


def devparam_mutations(prm):
    """name -> parameter dict with ONE solver-side mistake: the gravity of the office set, the two ground weights swapped, the laser
    rotation transposed, the wheel rotation transposed (extrinsics as the solver holds them, normalize_extrinsics off)"""
    Riw, Ril = solver_rotations(prm)
    tw, tl = (np.asarray(prm[k]).reshape(4, 4)[:3, 3] for k in ("T_imu_to_wheel", "T_imu_to_laser"))
    held = dict(prm, T_imu_to_wheel=_matrix16(Riw, tw), T_imu_to_laser=_matrix16(Ril, tl), normalize_extrinsics=False)
    return {"g = 9.8": dict(prm, g=9.8),
            "ground weights swapped": dict(prm, manifold_p_sigma=prm["manifold_q_sigma"], manifold_q_sigma=prm["manifold_p_sigma"]),
            "Ril transposed": dict(held, T_imu_to_laser=_matrix16(Ril.T, tl)),
            "Riw transposed": dict(held, T_imu_to_wheel=_matrix16(Riw.T, tw))}


def factor_values(orc, d):
    """the oracle's residuals and ambient Jacobians of every block of window `d` (INIT topology), per factor type"""
    n, st = int(d["n"]), np.asarray(d["states"]).reshape(-1, 15)
    out = dict(laser=[], imu=[], wheel=[], ground=[])
    for j in range(len(d["laser_frame"])):
        k = int(d["laser_frame"][j])
        out["laser"].append(orc.eval_laser(d["laser_pts"][j], st[0, 0:3], st[0, 3:6], st[k, 0:3], st[k, 3:6]))
    for k in range(n - 1):
        out["imu"].append(orc.eval_imu(d["imu_X"][k], d["imu_J"][k], d["imu_sqrtP"][k], d["imu_Dt"][k], st[k], st[k + 1]))
        out["wheel"].append(orc.eval_wheel(d["wheel_T"][k], d["wheel_sqrtP"][k], st[k, 0:3], st[k, 3:6], st[k + 1, 0:3], st[k + 1, 3:6]))
    for i in range(n):
        out["ground"].append(orc.eval_ground(st[i, 0:3], st[i, 3:6]))
    return out


def factor_move(ref, alt, kind):
    """largest |alt - ref| / max(1, |ref|_inf) over the residuals and Jacobians of one factor type: the measure of the per-factor bar"""
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))
    return max(max(rel(a[0], b[0]), rel(a[1], b[1])) for a, b in zip(alt[kind], ref[kind]))


# ---------------------------------------------------------------- the front half: laser front-end, loop detector, map
LASER = dict(w_laser_each_scan=11.0, h_laser_each_scan=6.6, laser_resolution=0.08, line_continuous_threshold=0.14, line_min_len=0.11,
             line_max_dis=0.021, line_max_tolerance_angle=170.0, ref_motion_filter_p=0.03, ref_motion_filter_q=0.017, ref_n_accumulation=5)
LASER_W, LASER_H = 138, 83      # (int)(11.0 / 0.08 + 1), (int)(6.6 / 0.08 + 1): 137.5 and 82.5 before the + 1, no rounding decides
LASER_THRESHOLDS = ("line_max_dis", "line_min_len", "line_continuous_threshold", "line_max_tolerance_angle", "ref_motion_filter_p",
                    "ref_motion_filter_q", "laser_resolution")
N_RAYS = 1080
ANG_MIN = np.float32(-2.0 * np.pi * 0.75 / 2)
ANG_INC = np.float32(2.0 * np.pi * 0.75 / (N_RAYS - 1))
T_INC = np.float32(1.0 / (40.0 * N_RAYS))
ROOMS, POSES_PER_ROOM, FRAMES = (1, 2, 3, 4, 5, 6), 4, 16
F_SMALL_P, F_SMALL_Q = 6, 11   # frames of the manager sequence whose motion lies between the two motion-filter thresholds
MATCH_GUESS = np.array([0.01, -0.01, 0.0, 0.0, 0.0, 0.004])   # do_match: the guess of the second pose is slightly off, as in tracking

LOOP_SETS = dict(
    office=dict(a_res=0.03, d_res=0.03, min_match_threshold=5, min_interval=10, max_dis=1.0, max_tf_p=1.0, max_tf_q=0.5),
    fine=dict(a_res=0.025, d_res=0.02, min_match_threshold=7, min_interval=12, max_dis=1.4, max_tf_p=0.8, max_tf_q=0.35),
    coarse=dict(a_res=0.07, d_res=0.11, min_match_threshold=7, min_interval=12, max_dis=1.4, max_tf_p=0.8, max_tf_q=0.35),
    edge=dict(a_res=2.0 * np.pi / 253.0, d_res=0.02, min_match_threshold=7, min_interval=12, max_dis=1.4, max_tf_p=0.8, max_tf_q=0.35))


def laser_params(liw, prm):
    """The second laser set over liw.laser.office_laser_params(prm), prm = skewed_params(synth): w = 138 and h = 83 cells (one even, one
    odd, 11 m x 6.6 m against rooms of about 9 m x 7 m: narrower than the rooms in one direction, wider in the other), every scalar
    different from every other one, an odd ref_n_accumulation (spawn at count 2, swap at count 5: a 2 / 3 cycle)."""
    return dict(liw.laser.office_laser_params(prm), **LASER)


def loop_params(name="fine", **kw):
    """A loop-detector set of LOOP_SETS: `fine` (W = 79 descriptor words, 253 angle bins: two lane passes), `coarse` (W = 15, 91 bins),
    `edge` (a_res = 2 pi / 253, the smallest that check_params accepts: 2 pi / a_res + 2 is 255.0 in double arithmetic, so
    nAngle + 1 = 256 = kMaxBins bins, the largest LDS histogram; anything finer, 2 pi / 253.5 included, is LIW_EINVAL) or `office`."""
    p = dict(LOOP_SETS[name], submap_count=1, seed=12345)
    p.update(kw)
    return p


def held_extrinsic(liw, prm, key="T_imu_to_laser"):
    """the 4x4 extrinsic as the library holds it: liw_lie_from_matrix16 with the parameters' normalize_extrinsics (the loader's
    quaternion round trip), exactly"""
    import ctypes as C
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    M, T12 = np.ascontiguousarray(np.asarray(prm[key], dtype=np.float64).reshape(16)), np.zeros(12)
    liw.lib().liw_lie_from_matrix16(pd(M), C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), pd(T12))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = T12[:9].reshape(3, 3), T12[9:]
    return T


def transposed_laser_rotation(liw, lp):
    """lp with ONE mistake: the laser rotation as held, transposed (normalize_extrinsics off, so it arrives as given)"""
    T = held_extrinsic(liw, lp)
    return dict(lp, T_imu_to_laser=_matrix16(T[:3, :3].T, T[:3, 3]), normalize_extrinsics=False)


def laser_mutations(liw, lp):
    """name -> laser parameters with ONE mistake, each of which a kernel could make without an office-set test noticing"""
    off = liw.laser.office_laser_params()
    out = {"w and h exchanged": dict(lp, w_laser_each_scan=lp["h_laser_each_scan"], h_laser_each_scan=lp["w_laser_each_scan"]),
           "motion filters exchanged": dict(lp, ref_motion_filter_p=lp["ref_motion_filter_q"], ref_motion_filter_q=lp["ref_motion_filter_p"]),
           "ref_n_accumulation = 4": dict(lp, ref_n_accumulation=4),
           "laser rotation transposed": transposed_laser_rotation(liw, lp)}
    for k in ("line_min_len", "line_max_dis", "line_continuous_threshold", "line_max_tolerance_angle"):
        out["office " + k] = dict(lp, **{k: off[k]})
    return out


def pose_T(synth, pose):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.exp_so3(np.asarray(pose[3:6], dtype=np.float64)), pose[:3]
    return T


def cast_scan(segs, T_w_l, seed, noise=0.004, max_range=30.0):
    """liw.laser.cast_scan's ranges for N_RAYS rays, all rays at once (the same formulas; the noise is drawn per hit in ray order)"""
    rng = np.random.default_rng(seed)
    o, yaw = T_w_l[:2, 3], np.arctan2(T_w_l[1, 0], T_w_l[0, 0])
    a = yaw + float(ANG_MIN) + np.arange(N_RAYS) * float(ANG_INC)
    dx, dy = np.cos(a), np.sin(a)
    best = np.full(N_RAYS, np.inf)
    for p, q in segs:
        e, w = q - p, p - o
        den = dx * e[1] - dy * e[0]
        ok = np.abs(den) >= 1e-12
        den = np.where(ok, den, 1.0)
        t, u = (w[0] * e[1] - w[1] * e[0]) / den, (w[0] * dy - w[1] * dx) / den
        ok &= (t > 0.05) & (u >= 0.0) & (u <= 1.0) & (t < best)
        best = np.where(ok, t, best)
    hit = best < max_range
    ranges = np.full(N_RAYS, np.inf, dtype=np.float32)
    ranges[hit] = (best[hit] + rng.normal(0.0, noise, int(hit.sum()))).astype(np.float32)
    return ranges


WALK_SEED = 4301   # chosen so that no decision of the oracle sits within 1e-6 of a threshold (tests/test_second_config_frontend.py)
MIN_LINES, MIN_BACK_MATCHES = 5, 2   # floors of the GPU laser tests: lines per scan, matches with the scan before


def _walk(liw, synth, room, Til, rng, seed):
    """a planar walk of the LASER in the room; the IMU poses are T_w_l T_il^-1, as a robot's are, so that the relative laser motion
    T_il^-1 (T_1^-1 T_2) T_il of add_scan and do_match stays near the scan plane and generic 3D rotation vectors reach make_tf.
    The rotation of T_il here is the rotation nearest to the one the library holds, which is 0.2 % off orthonormal at this set (the
    loader's round trip does not undo LASER_SKEW): transformed lines leave the plane z = 0 by millimetres, below line_max_dis."""
    planar = np.zeros((FRAMES, 6))
    planar[0] = np.concatenate([rng.uniform(-1.0, 1.0, 2), [0.0, 0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
    for k in range(1, FRAMES):
        step, turn = rng.uniform(0.05, 0.12), rng.uniform(-0.04, 0.04)
        if k == F_SMALL_P:
            step, turn = 0.024, 0.001
        if k == F_SMALL_Q:
            step, turn = 0.001, 0.024
        d = rng.uniform(-np.pi, np.pi)
        planar[k] = planar[k - 1] + np.array([step * np.cos(d), step * np.sin(d), 0.0, 0.0, 0.0, turn])
    U, _, Vt = np.linalg.svd(Til[:3, :3])
    T_li = np.eye(4)
    T_li[:3, :3] = (U @ Vt).T
    T_li[:3, 3] = -T_li[:3, :3] @ Til[:3, 3]
    poses, pts = np.zeros((FRAMES, 6)), []
    for k in range(FRAMES):
        T_wl = pose_T(synth, planar[k])
        T_wi = T_wl @ T_li
        poses[k] = np.concatenate([T_wi[:3, 3], synth.log_so3(T_wi[:3, :3])])
        pts.append(liw.laser.laser_to_points(cast_scan(room, T_wl, seed=seed + k), ANG_MIN, ANG_INC, T_INC, 0.0)[0])
    return poses, pts


def _meets_floors(liw, lp, poses, pts):
    scans = [liw.laser.Scan.spawn(lp, p) for p in pts]
    if min(s.lines().shape[0] for s in scans) < MIN_LINES:
        return False
    return all(len(liw.laser.do_match(lp, scans[k - 1], scans[k], poses[k - 1, :3], poses[k - 1, 3:], poses[k, :3], poses[k, 3:], kk)) >= MIN_BACK_MATCHES
               for k in range(1, FRAMES) for kk in (0, 1))


_scene = {}


def laser_scene(liw, synth):
    """The inputs of the laser tests at the second set, computed once: B = 24 robots (the six rooms of
    tests/test_laser_frontend.py x four poses), each walking FRAMES = 16 frames (_walk).  Steps are up to 0.12 m and 0.04 rad; in
    frame F_SMALL_P the laser moves 0.024 m (between the two motion-filter thresholds) and 0.001 rad, in frame F_SMALL_Q 0.001 m and
    0.024 rad (the IMU 0.007 m, through the lever arm): the filter drops the first and keeps the second, and does the converse with
    its thresholds exchanged.
    -> dict(prm, lp, Til, poses [B, F, 6], points [B][F] arrays [m, 3] in the laser frame, low_edge: a hand-placed scan)"""
    if _scene:
        return _scene
    prm = skewed_params(synth)
    lp = laser_params(liw, prm)
    Til = held_extrinsic(liw, prm)
    B = len(ROOMS) * POSES_PER_ROOM
    poses = np.zeros((B, FRAMES, 6))
    points, tries = [], []
    for b in range(B):
        room = liw.laser.room_segments(ROOMS[b // POSES_PER_ROOM])
        for attempt in range(200):       # the first walk of the robot's seeds that meets the floors of the GPU tests
            pw, pts = _walk(liw, synth, room, Til, np.random.default_rng(WALK_SEED + 1000 * attempt + b), 100 * b + 10000 * attempt)
            if _meets_floors(liw, lp, pw, pts):
                break
        else:
            raise AssertionError("no walk of robot %d meets the floors" % b)
        poses[b] = pw
        points.append(pts)
        tries.append(attempt)
    # a wall whose points have grid coordinates in (-1, 0) x [0, h): xy_to_index truncates them toward zero into column 0, a valid cell
    res, w2 = LASER["laser_resolution"], LASER_W // 2
    y = np.linspace(-1.0, 1.0, 60)
    low = np.stack([np.full(60, (-w2 - 0.5) * res) + 0.002 * np.sin(7.0 * y), y, np.zeros(60)], 1)
    _scene.update(prm=prm, lp=lp, Til=Til, poses=poses, points=points, low_edge=low, tries=tries)
    return _scene


def grid_coordinates(lp, pts):
    """(gx, gy) = x / resolution + w / 2, y / resolution + h / 2 before the truncation of xy_to_index, and (w, h)"""
    res = lp["laser_resolution"]
    w, h = int(lp["w_laser_each_scan"] / res + 1), int(lp["h_laser_each_scan"] / res + 1)
    return pts[:, 0] / res + w // 2, pts[:, 1] / res + h // 2, w, h
