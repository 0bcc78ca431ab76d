#!/usr/bin/env python
"""Generates tests/golden/solver_golden.json — INDEPENDENT pins for the parts of the oracle that tests/golden/make_golden.py does
not reach: the trust-region Levenberg-Marquardt loop, the Schur marginalisation + eigen square root, and the
IMU / wheel pre-integration.  Like make_golden.py this runs in the build container only (python tests/golden/make_golden_solver.py);
the JSON it writes is data.  PARITY REMAINS UNPINNED w.r.t. the reference itself (no Ceres / Eigen here, no reference tests): what
these vectors rule out is a mistake shared by the oracle and the HIP path, because every derivation below is written from the
published algorithm, not from oracle/*.h:

  lm        numpy restatement of Ceres 1.14's TrustRegionMinimizer + LevenbergMarquardtStrategy with the options the reference
            sets (solver.cpp:161-168; defaults otherwise): dense J from PyTorch fp64 autograd of the stacked
            residual vector, Jacobi scaling 1/(1 + |col|), normal equations solved with numpy.linalg.solve (no Schur, no block
            structure), rho / radius bookkeeping, parameter / function tolerance tests on the candidate.
  marg      dense J (autograd, marginalisation topology of solver.cpp:257-442) -> H = J^T J, g = -J^T R, Schur complement onto the
            last frame and symmetric eigen-decomposition in 50-digit mpmath arithmetic (solver.cpp:4-40, :390-402).
  preint    numpy re-statement of imu_preintegraption (src/factor/imu_preintegraption.h:113-208, incl. F(gamma,gamma) built from
            hat_gyro - last_ba as written at :192, P0 = 1e-5 I, the previous sample used for the whole step) and of
            wheel_odom_preintegration (wheel_odom_preintegration.h:62-152), with numpy's inverse / Cholesky.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
torch.set_default_dtype(torch.float64)
import make_golden as mg  # noqa: E402  (the factor residuals of the first golden generator)


# ------------------------------------------------------------------------------------------------ so3 helpers (numpy)
def normalize_so3(a):
    """lie::normalize_so3 (src/utilies/common.h:121-135)"""
    nrm = np.linalg.norm(a)
    if nrm > np.pi:
        return a / nrm * (nrm - 2.0 * np.pi * np.floor((nrm + np.pi) / (2.0 * np.pi)))
    return a


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3) + hat(w)
    K = hat(w)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def log_so3(R):
    c = (np.trace(R) - 1.0) * 0.5
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(v)
    th = np.arctan2(s, c)
    if s < 1e-300:
        return 0.5 * v
    return v * (th / (2.0 * s))


# ------------------------------------------------------------------------------------------------ stacked residuals (torch)
def stacked_init(prm, d, n):
    """do_init_solve's residual blocks (solver.cpp:50-169): laser (frame 0, frame i), IMU, wheel, n copies of the ground set"""
    L = len(d["laser_frame"])

    def f(xf):
        xs = xf.reshape(n, 15)
        rs = []
        for j in range(L):
            k = int(d["laser_frame"][j])
            rs.append(mg.laser_res(prm, d["laser_pts"][j], torch.cat([xs[0, 0:6], xs[k, 0:6]])))
        for k in range(n - 1):
            rs.append(mg.imu_res(prm, d["imu_X"][k], d["imu_J"][k], d["imu_sqrtP"][k], float(d["imu_Dt"][k]), torch.cat([xs[k], xs[k + 1]])))
            rs.append(mg.wheel_res(prm, d["wheel_T"][k], d["wheel_sqrtP"][k], torch.cat([xs[k, 0:6], xs[k + 1, 0:6]])))
        for _ in range(n):
            for k in range(n):
                rs.append(mg.ground_res(prm, xs[k, 0:6]))
        return torch.cat(rs)
    return f


def stacked_marg(prm, d, n, prior):
    """solver::marginalization's rows (solver.cpp:257-442): prior rows J (X - X0) on frame n-2, every frame's laser rows against the
    constant laser_match pose (p1, q1), IMU, wheel, n copies of the ground set.  R is this vector, g = -J^T R."""
    L = len(d["laser_frame"])
    mp = torch.tensor(np.asarray(d["match_pose"]).reshape(n, 12))

    def f(xf):
        xs = xf.reshape(n, 15)
        rs = []
        if prior is not None:
            X0, J0 = torch.tensor(prior[0]), torch.tensor(prior[1])
            rs.append(J0 @ (xs[n - 2] - X0))
        for j in range(L):
            k = int(d["laser_frame"][j])
            rs.append(mg.laser_res(prm, d["laser_pts"][j], torch.cat([mp[k, 0:6], xs[k, 0:6]])))
        for k in range(n - 1):
            rs.append(mg.imu_res(prm, d["imu_X"][k], d["imu_J"][k], d["imu_sqrtP"][k], float(d["imu_Dt"][k]), torch.cat([xs[k], xs[k + 1]])))
            rs.append(mg.wheel_res(prm, d["wheel_T"][k], d["wheel_sqrtP"][k], torch.cat([xs[k, 0:6], xs[k + 1, 0:6]])))
        for _ in range(n):
            for k in range(n):
                rs.append(mg.ground_res(prm, xs[k, 0:6]))
        return torch.cat(rs)
    return f


def eval_rJ(f, x):
    xt = torch.tensor(x)
    r = f(xt).detach().numpy()
    J = torch.autograd.functional.jacobian(f, xt, vectorize=True).detach().numpy()   # batched reverse mode: one pass for all rows
    return r, J


# ------------------------------------------------------------------------------------------------ Ceres-style trust-region LM
def plus(x, delta, n):
    """so3_parameterization::Plus on every q block (factor_common.h:41-53), plain addition elsewhere"""
    y = x + delta
    for i in range(n):
        y[i * 15 + 3:i * 15 + 6] = normalize_so3(x[i * 15 + 3:i * 15 + 6] + delta[i * 15 + 3:i * 15 + 6])
    return y


def ceres_lm(f, x0, n, max_num_iterations=50):
    """TrustRegionMinimizer::Minimize with LevenbergMarquardtStrategy, Ceres 1.14 defaults:
    initial_trust_region_radius 1e4, max 1e16, min 1e-32, min_relative_decrease 1e-3, min / max_lm_diagonal 1e-6 / 1e32,
    function_tolerance 1e-6, gradient_tolerance 1e-10, parameter_tolerance 1e-8, jacobi_scaling, monotonic steps."""
    radius, decrease_factor, reuse_diagonal = 1e4, 2.0, False
    x = x0.copy()
    r, J = eval_rJ(f, x)          # every |q| < pi here, so the local parameterisation Jacobian is the identity
    cost = 0.5 * float(r @ r)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(axis=0)))
    x_norm = np.linalg.norm(x)
    diag = None
    rec = [dict(iteration=0, cost=cost, x=x.tolist(), radius=radius)]
    termination, iteration, invalid = "NO_CONVERGENCE", 0, 0
    while True:
        if iteration >= max_num_iterations:
            termination = "max_iterations"
            break
        if radius < 1e-32:
            termination = "min_radius"
            break
        iteration += 1
        Js = J * scale[None, :]
        g = Js.T @ r
        A = Js.T @ Js
        if not reuse_diagonal:
            diag = np.clip(np.diag(A), 1e-6, 1e32)
        lm = A + np.diag(diag / radius)
        step = -np.linalg.solve(lm, g)
        model = Js @ step
        model_cost_change = -float(model @ (r + 0.5 * model))
        it = dict(iteration=iteration, radius_used=radius)
        if not (model_cost_change > 0.0):
            invalid += 1
            it.update(valid=False)
            rec.append(it)
            if invalid >= 5:
                termination = "failure"
                break
            radius, decrease_factor, reuse_diagonal = radius / decrease_factor, decrease_factor * 2.0, True
            continue
        invalid = 0
        delta = step * scale
        cand = plus(x, delta, n)
        rc = f(torch.tensor(cand)).detach().numpy()
        cand_cost = 0.5 * float(rc @ rc)
        step_norm = np.linalg.norm(x - cand)
        it.update(valid=True, candidate_cost=cand_cost, model_cost_change=model_cost_change, step_norm=step_norm)
        if step_norm <= 1e-8 * (x_norm + 1e-8):
            termination = "parameter_tolerance"
            it.update(cost=cost, x=x.tolist(), successful=False)
            rec.append(it)
            break
        cost_change = cost - cand_cost
        if abs(cost_change) <= 1e-6 * cost:
            termination = "function_tolerance"
            it.update(cost=cost, x=x.tolist(), successful=False)
            rec.append(it)
            break
        rho = cost_change / model_cost_change
        it.update(relative_decrease=rho)
        if rho > 1e-3:
            x, cost = cand, cand_cost
            x_norm = np.linalg.norm(x)
            r, J = eval_rJ(f, x)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease_factor, reuse_diagonal = 2.0, False
            it.update(successful=True)
            gmax = np.abs(J.T @ r).max()
            if gmax <= 1e-10:
                it.update(cost=cost, x=x.tolist(), radius=radius)
                rec.append(it)
                termination = "gradient_tolerance"
                break
        else:
            radius, decrease_factor, reuse_diagonal = radius / decrease_factor, decrease_factor * 2.0, True
            it.update(successful=False)
        it.update(cost=cost, x=x.tolist(), radius=radius)
        rec.append(it)
    return dict(termination=termination, iterations=iteration if termination != "max_iterations" else max_num_iterations, records=rec, final_x=x.tolist(),
                final_cost=cost)


# ------------------------------------------------------------------------------------------------ 50-digit marginalisation
def marg_mpmath(J, R, keep=15, dps=50):
    import mpmath as mp
    mp.mp.dps = dps
    rows, cols = J.shape
    m = cols - keep
    Jm = [[mp.mpf(float(v)) for v in row] for row in J]
    Rm = [mp.mpf(float(v)) for v in R]
    H = mp.matrix(cols, cols)
    g = mp.matrix(cols, 1)
    nz = [[c for c in range(cols) if J[r, c] != 0.0] for r in range(rows)]
    for r in range(rows):
        for a in nz[r]:
            g[a] -= Jm[r][a] * Rm[r]
            for b in nz[r]:
                H[a, b] += Jm[r][a] * Jm[r][b]
    Hmm, Hmr, Hrm, Hrr = H[:m, :m], H[:m, m:], H[m:, :m], H[m:, m:]
    X = mp.matrix(m, keep)               # Hmm^-1 Hmr, column by column
    for j in range(keep):
        col = mp.lu_solve(Hmm, Hmr[:, j])
        for i in range(m):
            X[i, j] = col[i]
    y = mp.lu_solve(Hmm, g[:m, 0])
    dH = Hrr - Hrm * X
    dg = g[m:, 0] - Hrm * y
    dHs = (dH + dH.T) / 2
    E, V = mp.eigsy(dHs)
    eps = mp.mpf("1e-8")
    S = [E[i] if E[i] > eps else mp.mpf(0) for i in range(keep)]
    Sinv = [1 / E[i] if E[i] > eps else mp.mpf(0) for i in range(keep)]
    # linearized_jacobians = sqrt(S) V^T ; linearized_residuals = -(S^-1/2 V^T Delta_g)   (solver.cpp:399-402)
    LJ = mp.matrix(keep, keep)
    LR = mp.matrix(keep, 1)
    for i in range(keep):
        dot = sum(V[k, i] * dg[k] for k in range(keep))
        for j in range(keep):
            LJ[i, j] = mp.sqrt(S[i]) * V[j, i]
        LR[i] = -(mp.sqrt(Sinv[i]) * dot)
    JtJ = LJ.T * LJ
    JtR = LJ.T * LR
    tof = lambda M: [[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)]
    return dict(Delta_H=tof(dH), Delta_g=[float(dg[i]) for i in range(keep)], eigenvalues=[float(E[i]) for i in range(keep)],
                prior_JtJ=tof(JtJ), prior_JtR=[float(JtR[i]) for i in range(keep)])


# ------------------------------------------------------------------------------------------------ pre-integration (numpy)
def imu_preint_numpy(prm, samples, t_start, t_end, bias6, noise_rotation=None):
    """imu_preintegraption driven like trajectory.cpp:176-184: sample 0 seeds last_info, reset at t_start, add every later sample,
    update_only_t(t_end), result = X, J, LLT(P^-1).matrixL()^T, Dt.
    noise_rotation: None, or a function of Rz whose value takes the place of Rz in the noise matrix G only (imu_preintegraption.h:196) —
    for tests that ask whether their inputs would expose such a mistake (tests/test_second_config.py); never set by the generators."""
    Q = np.zeros((12, 12))
    Q[0:3, 0:3] = np.diag(np.square(prm["imu_noise_acc_sigma"]))
    Q[3:6, 3:6] = np.diag(np.square(prm["imu_noise_gyro_sigma"]))
    Q[6:9, 6:9] = np.diag(np.square(prm["imu_bias_acc_sigma"]))
    Q[9:12, 9:12] = np.diag(np.square(prm["imu_bias_gyro_sigma"]))
    Jm, P, X = np.eye(15), np.eye(15) * 0.00001, np.zeros(15)
    X[9:12], X[12:15] = bias6[0:3], bias6[3:6]
    Dt = 0.0
    last = samples[0]
    last_t = t_start

    def update(dt):
        nonlocal Jm, P, X, Dt
        al, be, ga, ba, bw = X[0:3].copy(), X[3:6].copy(), X[6:9].copy(), X[9:12].copy(), X[12:15].copy()
        Rz = exp_so3(ga)
        acc, gyro = last[1:4], last[4:7]
        X[0:3] = al + be * dt + 0.5 * Rz @ (acc - ba) * dt * dt
        X[3:6] = be + Rz @ (acc - ba) * dt
        X[6:9] = normalize_so3(log_so3(exp_so3(ga) @ exp_so3((gyro - bw) * dt)))
        F = np.zeros((15, 15))
        F[0:3, 3:6] = np.eye(3)
        F[3:6, 6:9] = -Rz @ hat(acc - ba)
        F[3:6, 9:12] = -Rz
        F[6:9, 6:9] = -hat(gyro - ba)          # the accelerometer bias, as written at imu_preintegraption.h:192
        F[6:9, 12:15] = -np.eye(3)
        G = np.zeros((15, 12))
        G[3:6, 0:3] = -(Rz if noise_rotation is None else noise_rotation(Rz))
        G[6:9, 3:6] = -np.eye(3)
        G[9:12, 6:9] = np.eye(3)
        G[12:15, 9:12] = np.eye(3)
        F = np.eye(15) + F * dt
        Jm = F @ Jm
        P = F @ P @ F.T + (G * dt) @ Q @ (G * dt).T
        Dt += dt
    for s in samples[1:]:
        update(s[0] - last_t)
        last, last_t = s, s[0]
    update(t_end - last_t)
    Pinv = np.linalg.inv(P)
    sqrtP = np.linalg.cholesky(0.5 * (Pinv + Pinv.T)).T
    return X, Jm, sqrtP, Dt


def log_se3(T):
    return T[:3, 3].copy(), normalize_so3(log_so3(T[:3, :3]))


def wheel_preint_numpy(prm, samples, t_start, t_end):
    """wheel_odom_preintegration driven like trajectory.cpp:176-184 (samples [t, R(9), t(3)]): twist from consecutive poses
    (ignored when dt < 0.05), delta_Tij *= make_tf(v dt, omega dt)"""
    def pose(s):
        T = np.eye(4)
        T[:3, :3] = s[1:10].reshape(3, 3)
        T[:3, 3] = s[10:13]
        return T
    v, om = np.zeros(3), np.zeros(3)
    delta, Dt = np.eye(4), 0.0
    last_update, last_add_t, last_pose = -1.0, None, None
    did_reset = False

    def update_by_v(dt):
        nonlocal delta, Dt
        if dt <= 0 or dt >= 10:
            return
        Dt += dt
        T = np.eye(4)
        T[:3, :3] = exp_so3(om * dt)
        T[:3, 3] = v * dt
        delta = delta @ T

    def reset(t):
        nonlocal last_update, delta, Dt
        last_update, delta, Dt = t, np.eye(4), 0.0

    def add(s):
        nonlocal v, om, last_update, last_add_t, last_pose, delta
        if last_update < 0:
            last_pose, last_add_t, last_update = pose(s), s[0], s[0]
            delta = np.eye(4)
            v, om = np.zeros(3), np.zeros(3)
            return
        dt = s[0] - last_add_t
        rel = np.linalg.inv(last_pose) @ pose(s)
        dp, dth = log_se3(rel)
        if dt < 0.05:
            return
        v, om = dp / dt, dth / dt
        update_by_v(s[0] - last_update)
        last_pose, last_add_t, last_update = pose(s), s[0], s[0]

    def update_only_t(t):
        nonlocal last_update
        if last_update < 0:
            return
        update_by_v(t - last_update)
        last_update = t
    for s in samples:
        if not did_reset and s[0] > t_start:
            update_only_t(t_start)
            reset(t_start)
            did_reset = True
        add(s)
    if not did_reset:
        update_only_t(t_start)
        reset(t_start)
    update_only_t(t_end)
    dp, dq = log_se3(delta)
    len_norm = max(float(dp @ dp), 0.005 * 0.005)
    yaw_norm = max(float(dq @ dq), 0.005 * 0.005)
    cov = np.diag(np.square(prm["wheel_sigma"])) @ np.diag([len_norm, len_norm, yaw_norm])
    sqrt_info = np.linalg.cholesky(np.linalg.inv(cov)).T
    return np.concatenate([delta[:3, :3].reshape(9), delta[:3, 3]]), sqrt_info, Dt


def preint_cases(base, count=3, wheel_count=None):
    """`count` IMU and `wheel_count` (default: as many) wheel intervals of the synthetic generator's own sample streams at the parameter
    dict `base`, with the results of the numpy restatements above -> the `preint` record"""
    synth = importlib.import_module("2dliw-slam_amd.synth")
    wheel_count = count if wheel_count is None else wheel_count
    out = {"imu": [], "wheel": []}
    tr = synth._Truth(base)
    rng = np.random.default_rng(77)
    for k in range(count):
        t0, t1 = 1.0 + 0.1 * k, 1.1 + 0.1 * k + 0.013 * k
        ts = t0 - 0.004 + np.arange(int((t1 - t0) * 200) + 1) / 200.0
        smp = np.zeros((len(ts), 7))
        for i, t in enumerate(ts):
            a, w = tr.imu(t)
            smp[i] = np.concatenate([[t], a + rng.normal(0, 0.01, 3), w + rng.normal(0, 0.001, 3)])
        bias = rng.normal(0.0, 1e-3, 6)
        X, Jm, S, Dt = imu_preint_numpy(base, smp, t0, t1, bias)
        out["imu"].append(dict(samples=smp.tolist(), t_start=t0, t_end=t1, bias=bias.tolist(), X=X.tolist(), J=Jm.tolist(), sqrt_inverse_P=S.tolist(), Dt=Dt))
        tw = np.arange(t0 - 2.5 * 0.0505, t1, 0.0505)
        ws = np.zeros((len(tw), 13))
        for i, t in enumerate(tw):
            T = tr.T_w_o(t)
            ws[i] = np.concatenate([[t], T[:3, :3].reshape(9), T[:3, 3] + rng.normal(0, 2e-4, 3)])
        if k < wheel_count:
            T12, S3, Dtw = wheel_preint_numpy(base, ws, t0, t1)
            out["wheel"].append(dict(samples=ws.tolist(), t_start=t0, t_end=t1, T=T12.tolist(), sqrt_inverse_P=S3.tolist(), Dt=Dtw))
    return out


# ------------------------------------------------------------------------------------------------ main
def main():
    synth = importlib.import_module("2dliw-slam_amd.synth")
    from oracle import pyoracle
    base = synth.office_params()
    prm = mg.torch_params(base)
    orc = pyoracle.Oracle(base)   # pre-integration provider of the synthetic generator only
    path = os.path.join(HERE, "solver_golden.json")
    only = set(sys.argv[1:])                       # e.g. `make_golden_solver.py marg preint` recomputes those sections only
    out = json.load(open(path)) if (only and os.path.exists(path)) else {}
    out["params"] = {k: base[k] for k in base}
    want = lambda name: not only or name in only
    keys = ("states", "laser_frame", "laser_pts", "match_pose", "has_match", "imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP", "wheel_Dt")

    # ---- lm: two windows, different sizes / noise levels
    if want("lm"):
        out["lm"] = []
    for seed, n, L, noise, cap in ((321, 5, 40, 1.0, 30), (322, 4, 18, 0.3, 50)) if want("lm") else ():
        d = synth.make_window(orc, base, seed=seed, n=n, L=L, state_noise=noise)
        res = ceres_lm(stacked_init(prm, d, n), np.asarray(d["states"]).reshape(-1).copy(), n, max_num_iterations=cap)
        win = {k: np.asarray(d[k]).tolist() for k in keys}
        win["n"] = n
        out["lm"].append(dict(window=win, max_num_iterations=cap, **res))
        print("lm seed %d: %s after %d iterations, cost %.6f -> %.6f" % (seed, res["termination"], res["iterations"], res["records"][0]["cost"], res["final_cost"]))

    # ---- marg: without and with a prior
    if want("marg"):
        out["marg"] = []
    for seed, n, L, with_prior in ((411, 4, 24, False), (412, 5, 30, True)) if want("marg") else ():
        d = synth.make_window(orc, base, seed=seed, n=n, L=L, laser_on_frame0=True)
        prior = None
        if with_prior:
            rng = np.random.default_rng(seed)
            A = rng.normal(0.0, 1.0, (15, 15))
            prior = (np.asarray(d["states"])[n - 2] + rng.normal(0.0, 1e-3, 15), np.triu(A) * 30.0)
        x = np.asarray(d["states"]).reshape(-1).copy()
        R, J = eval_rJ(stacked_marg(prm, d, n, prior), x)
        res = marg_mpmath(J, R)
        win = {k: np.asarray(d[k]).tolist() for k in keys}
        win["n"] = n
        out["marg"].append(dict(window=win, prior=None if prior is None else dict(X=prior[0].tolist(), J=prior[1].tolist()), rows=int(J.shape[0]), **res))
        print("marg seed %d: rows %d, eigenvalues %.3e .. %.3e" % (seed, J.shape[0], min(res["eigenvalues"]), max(res["eigenvalues"])))

    # ---- preint: intervals of the synthetic generator's own sample streams
    if want("preint"):
        out["preint"] = preint_cases(base)
    json.dump(out, open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
