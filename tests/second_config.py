"""The SECOND parameter set of the parity tests (tests/test_second_config.py on the CPU, tests/test_gpu_second_config.py on the GPU).

synth.office_params() has four isotropic IMU noise vectors, extrinsic rotations within a few degrees of signed permutation matrices and one
value per scalar, so whole classes of kernel error cannot fail a test that uses it: dt^2 Rz diag(q_na) Rz^T is q dt^2 I whatever Rz is, a
constant folded into a packed record equals the parameter, a transposed extrinsic moves results by little.  `skewed_params` differs from it
in every scalar, has three distinct components per vector, generic extrinsic rotations and a laser matrix that is not orthonormal, so the
quaternion round trip of the parameter loader (reference src/utilies/params.cpp:44-54) does work.

A helper module, not a conftest: it holds the configuration, the inputs the two test modules share and the mutated restatements with
which the CPU guards show that these inputs would expose each class of mistake.  Everything here is numpy."""
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
