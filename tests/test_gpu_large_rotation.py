"""GPU parity at LARGE ROTATIONS: the device instantiations of `log_SO3` (csrc/liw_dual.hpp) — dual numbers of one, three and four
directions in the IMU / wheel roles, the pose-graph edge residual, plain doubles in the pre-integration kernels — with the matrix
trace <= 0 (angle above 120 deg): every pivot of the quaternion construction, both signs of its scalar part (the cos_theta < 0 arm of
QuaternionToAngleAxis, whose angle normalize_so3 wraps back) next to trace > 0 blocks in the same wave.  Inputs and their numpy-only
classification come from tests/large_rotation_cases.py; every test asserts the coverage (all seven arms) and the margins to the decision
boundaries on that classification BEFORE it compares anything.  The oracle these tests compare with is checked against finite
differences on the same inputs in tests/test_oracle_large_rotation.py.

Tolerances are those of the ordinary-window tests: factors 1e-10 * max(1, |ref|_inf) (test_gpu_parity.py); H, g TOL_HG = 1e-12 entry-scaled,
1e-12 per 15x15 and 1e-11 per 3x3 block (parity_util.py); LM iterates 1e-6; pre-integration as in test_gpu_preint.py."""
import numpy as np
import pytest

import large_rotation_cases as lr
from parity_util import TOL_HG, block_rel_errors, normal_eq_errors, rel_inf

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


@pytest.fixture(scope="module")
def env(liw, synth, pyoracle):
    prm = synth.office_params()
    return prm, pyoracle.Oracle(prm)


# ------------------------------------------------------------------------------------------------ 1. per factor
@pytest.mark.parametrize("nd3", [False, True])
def test_factor_residuals_and_jacobians_in_every_arm(liw, synth, pyoracle, env, monkeypatch, nd3):
    """One window (n = 10, L = 40) whose nine blocks turn by: small, 2.2 about x, 2.6 about y, 3.0 about z, 3.13 about -z, small,
    2.3 about (-1,.1,.1), 2.8 about (.1,-1,.1), small — the IMU residual rotation is exactly that turn, the wheel role sees it carried
    into the wheel frame (other pivots), the measured increment of blocks 1, 3 and 6 is turned along.  Residuals and ambient Jacobians
    of every IMU, wheel, ground and laser block against the oracle's Jets, with one derivative direction per lane (a single window:
    k_lin_all, small_nd = 1) and with LIW_SMALL_ND3 (three directions per lane, the instantiation of the batched kernels).
    Bar 1e-10 * max(1, |ref|_inf); the test prints its measured worst errors before it asserts."""
    prm, orc = env
    if nd3:
        monkeypatch.setenv("LIW_SMALL_ND3", "1")
    else:
        monkeypatch.delenv("LIW_SMALL_ND3", raising=False)
    n, L = 10, 40
    d, cls = lr.factor_window(synth, orc, prm, seed=5, n=n, L=L)
    lr.assert_margins(cls)
    lr.assert_coverage(lr.by_role(cls, "imu"), wrapped=True)
    lr.assert_coverage(lr.by_role(cls, "wheel"), wrapped=True)
    assert sorted(c["block"] for c in lr.by_role(cls, "oq") if c["trace"] <= 0.0) == [1, 3, 6]
    slv = liw.Solver(prm)
    slv.set_window(liw.Window(d))
    f = slv.eval_factors(liw.LIW_MODE_INIT)
    st = d["states"]
    worst = dict(laser=0.0, imu=0.0, wheel=0.0, ground=0.0)
    for j in range(L):
        k = int(d["laser_frame"][j])
        r, J = orc.eval_laser(d["laser_pts"][j], st[0, 0:3], st[0, 3:6], st[k, 0:3], st[k, 3:6])
        worst["laser"] = max(worst["laser"], rel(f["laser_res"][j], r), rel(f["laser_jac"][j], J))
    for k in range(n - 1):
        r, J = orc.eval_imu(d["imu_X"][k], d["imu_J"][k], d["imu_sqrtP"][k], d["imu_Dt"][k], st[k], st[k + 1])
        e = max(rel(f["imu_res"][k], r), rel(f["imu_jac"][k], J))
        r, J = orc.eval_wheel(d["wheel_T"][k], d["wheel_sqrtP"][k], st[k, 0:3], st[k, 3:6], st[k + 1, 0:3], st[k + 1, 3:6])
        ew = max(rel(f["wheel_res"][k], r), rel(f["wheel_jac"][k], J))
        print("block %d: imu %.2e wheel %.2e" % (k, e, ew))
        worst["imu"], worst["wheel"] = max(worst["imu"], e), max(worst["wheel"], ew)
    for i in range(n):
        r, J = orc.eval_ground(st[i, 0:3], st[i, 3:6])
        worst["ground"] = max(worst["ground"], rel(f["ground_res"][i], r), rel(f["ground_jac"][i], J))
    print("per-factor worst errors (nd3=%s): %s" % (nd3, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1e-10, worst


# ------------------------------------------------------------------------------------------------ 2. normal equations
@pytest.fixture(scope="module")
def base_windows(synth, pyoracle, env):
    """eight base windows per n, built as the per-factor window with the turn list shifted per window (lanes of different windows that
    share a wave differ in arm too), and the oracle's normal equations of each: built once, shared, never modified"""
    prm, orc = env
    cache = {}

    def get(n):
        if n not in cache:
            wins, cls, ref = [], [], []
            for k in range(8):
                w, c = lr.factor_window(synth, orc, prm, seed=300 + 10 * n + k, n=n, L=4 * n, shift=(4 * k if n == 5 else 2 * k))
                wins.append(w)
                cls += [dict(x, window=k) for x in c]
                orc.set_prior(None)
                Ho, go, co = orc.linearize(pyoracle.Window(w), 0)
                orc.marginalization(pyoracle.Window(w))
                m = orc.marg_pieces()
                ref.append(dict(init=(Ho, go, co), marg=(m["H"], m["g"], 0.5 * float(m["R"] @ m["R"]))))
            cache[n] = (wins, cls, ref)
        return cache[n]
    return get


#          n   B     environment          routes
SHAPES = [(5, 8, None, ("plain",)),
          (12, 8, None, ("plain",)),
          (12, 40, None, ("plain",)),
          (5, 1024, None, ("plain", "bracket")),
          (12, 1024, None, ("plain", "bracket")),
          (5, 1024, "LIW_NO_IMU_MULTI", ("plain", "bracket")),
          (5, 1024, "LIW_NO_IMU_PACK", ("bracket",)),
          (12, 1024, "LIW_NO_IMU_PACK", ("bracket",))]
CASES = [(n, B, e, r, "init") for n, B, e, rs in SHAPES for r in rs] + [(n, B, e, "plain", "marg") for n, B, e, rs in SHAPES if "plain" in rs]


@pytest.mark.parametrize("n,B,envvar,route,mode_name", CASES)
def test_normal_equations_in_every_arm_through_every_batched_kernel(liw, synth, pyoracle, env, base_windows, monkeypatch, n, B, envvar, route, mode_name):
    """H, g, cost of windows whose blocks take every arm, against the oracle, through each linearisation kernel (launch_linearize,
    k_linearize.hip; pi_frame_format, liw_kernels.hpp):
      B = 8             !pi_frame and laser + IMU + small waves <= 256: everything in ONE k_lin_all launch (n = 5 and 12; with
                        B n + 2 blocks + ground waves <= 256 also one direction per lane)
      B = 40, n = 12    more than 256 waves, B < QUAD_MIN_BATCH: the stand-alone k_lin_laser / k_lin_imu / k_lin_small, per-block records
      B = 1024          pi_frame_format(B) (B >= QUAD_MIN_BATCH): per-frame IMU records; imu_chain_windows(n - 1) > 1 at n = 5 sends the
                        IMU role to k_lin_imu_chain_multi (four windows per wave), n = 12 to k_lin_imu_chain; k_lin_small at 31 blocks
                        per wave; the roles on forked streams.  LIW_NO_IMU_MULTI=1: k_lin_imu_chain at n = 5 as well.
      route "bracket"   liw_batch_lm_begin + liw_batch_lm_linearize(candidate 0): with B (n - 1) >= 4096 the IMU role reads the packed
                        rows liw_batch_lm_begin builds; LIW_NO_IMU_PACK=1: the caller's arrays.  ("plain": liw_batch_linearize.)
    INIT and MARG topologies; the first, a middle and the last copy of each of the eight base windows.
    Bars: cost 1e-12, H and g TOL_HG = 1e-12 entry-scaled, 15x15 blocks 1e-12, 3x3 blocks 1e-11 (INIT); MARG as test_gpu_batch.py.
    The test prints its measured worst errors before it asserts."""
    prm, orc = env
    wins, cls, ref = base_windows(n)
    lr.assert_margins(cls)
    lr.assert_coverage(lr.by_role(cls, "imu"), wrapped=True)
    lr.assert_coverage(lr.by_role(cls, "wheel"), wrapped=True)
    assert {c["arm"] for c in lr.by_role(cls, "oq")} >= {"pos", (0, 1), (0, -1), (2, 1)}
    for v in ("LIW_NO_IMU_MULTI", "LIW_NO_IMU_PACK", "LIW_SMALL_ND3", "LIW_STEP_VARIANT"):
        monkeypatch.delenv(v, raising=False)
    if envvar:
        monkeypatch.setenv(envvar, "1")
    mode = liw.LIW_MODE_INIT if mode_name == "init" else liw.LIW_MODE_MARG
    bs = liw.BatchSolver(prm, [wins[b % 8] for b in range(B)])
    if route == "bracket":
        assert B * (n - 1) >= 4096                                  # the packing threshold of liw_batch_lm_begin
        bs.lm_begin(mode, 4)
        bs.lm_linearize(mode, 0)
    else:
        bs.linearize(mode)
    if B >= 1024:
        assert bs.launch_paths()["large_batch_format"]
    picks = sorted({b for k in range(8) for b in (k, 8 * (B // 16) + k, B - 8 + k)})
    H, g, c = bs.export_dense(mode)
    import torch
    ix = torch.tensor(picks, device=H.device)
    H, g, c = H[ix].cpu().numpy(), g[ix].cpu().numpy(), c[ix].cpu().numpy()
    bs.close()
    worst = dict(cost=0.0, H=0.0, g=0.0, b15=0.0, b3=0.0)
    for q, b in enumerate(picks):
        Ho, go, co = ref[b % 8][mode_name]
        assert np.isfinite(H[q]).all() and np.isfinite(g[q]).all()
        eH, eg = normal_eq_errors(H[q], g[q], Ho, go, co)
        e = dict(H=eH, g=eg)
        if mode_name == "init":
            e.update(cost=abs(c[q] - co) / co, b15=block_rel_errors(H[q], Ho, 15), b3=block_rel_errors(H[q], Ho, 3))
        worst = {k: max(worst[k], e.get(k, 0.0)) for k in worst}
    print("n=%d B=%d %s %s %s: worst over %d sampled windows: %s" % (n, B, envvar, route, mode_name, len(picks), " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["H"] <= TOL_HG and worst["g"] <= TOL_HG, worst
    assert worst["cost"] <= 1e-12 and worst["b15"] <= 1e-12 and worst["b3"] <= 1e-11, worst


# ------------------------------------------------------------------------------------------------ 3. solves
def _check_history(hist, its, n, what):
    worst = 0.0
    assert len(hist) >= len(its), what
    for k in range(len(its)):
        e = rel_inf(hist[k], its[k]["x"].reshape(n, 15))
        worst = max(worst, e)
        assert e <= 1e-6, (what, "iteration %d" % k, e)
    return worst


@pytest.mark.parametrize("seed,n,L,yaw,cap", lr.KIDNAP_CASES)
def test_init_solves_from_a_turned_heading(liw, synth, pyoracle, env, seed, n, L, yaw, cap):
    """A window whose frames n // 2 ... start `yaw` off (kidnapped heading): the LM iterates hold a block beyond 120 deg for at least three
    iterations (asserted on the oracle's log with the numpy classifier), and those evaluations decide accept / reject.  The single-window
    solver with history, and a batch of 1 024 (k_lm_step_quad: B >= QUAD_MIN_BATCH) cycling through this window, the same window
    kidnapped the other way and two ordinary ones: same iteration count and termination as the oracle, states after EVERY iteration
    within 1e-6 relative.  The oracle's own sensitivity to round-off here is <= 1.8e-11 (tests/test_oracle_large_rotation.py).
    The test prints its measured worst errors before it asserts."""
    prm, orc = env
    base, clss = [], []
    for k, (sd, y) in enumerate(((seed, yaw), (seed + 100, None), (seed, -yaw), (seed + 101, None))):
        if y is None:
            base.append(synth.make_window(orc, prm, seed=sd, n=n, L=L))
        else:
            w, c = lr.kidnapped_case(synth, orc, prm, sd, n, L, y)
            base.append(w)
            clss += c
    lr.assert_margins(clss)
    assert all(c["trace"] <= 0.0 for c in clss) and {c["cw_sign"] for c in clss} == {1, -1}
    orc.set_max_iterations(cap)
    want = []
    try:
        for k, w in enumerate(base):
            wo = pyoracle.Window(w)
            orc.set_prior(None)
            orc.init_solve(wo)
            want.append((orc.summary(), orc.iterations(), wo["states"].reshape(n, 15).copy()))
            if k in (0, 2):
                assert lr.iterations_beyond_120_degrees(want[k][1], w, prm) >= 3
    finally:
        orc.set_max_iterations(50)
    # single window
    slv = liw.Solver(prm)
    wg = liw.Window(base[0])
    slv.set_window(wg)
    sg = slv.init_solve(cap)
    so, its, xo = want[0]
    assert (sg["iterations"], sg["termination"]) == (so["iterations"], so["termination"]), (sg, so)
    hg = slv.history()
    assert len(hg) == len(its)
    w1 = _check_history(hg, its, n, "single window")
    assert rel_inf(np.asarray(wg["states"]).reshape(n, 15), xo) <= 1e-6
    # batch of 1 024
    B = 1024
    bs = liw.BatchSolver(prm, [base[b % 4] for b in range(B)], history_records=cap + 2)
    bs.solve(liw.LIW_MODE_INIT, cap)
    assert bs.launch_paths()["large_batch_format"]
    got, summ, hist = bs.states(), bs.summaries(), bs.history()
    wb = 0.0
    for k in range(4):
        so, its, xo = want[k]
        for b in (k, 4 * (B // 8) + k, B - 4 + k):
            assert (summ[b]["iterations"], summ[b]["termination"]) == (so["iterations"], so["termination"]), (k, b, summ[b], so)
            wb = max(wb, _check_history(hist[:, b], its, n, "batch window %d" % b))
            assert rel_inf(got[b], xo) <= 1e-6, (k, b)
    bs.close()
    print("kidnapped init solve seed %d: worst state error over all iterations: single window %.2e, batch of 1024 %.2e" % (seed, w1, wb))


def test_tracking_solves_with_the_newest_frame_turned(liw, synth, pyoracle, env):
    """TRACK topology: two-frame windows whose newest frame starts 2.5 / -2.9 rad off, with the prior of the oracle's marginalisation of
    the unturned window on both sides.  The single-window solver (B = 1, n = 2: the dense two-frame step) and a batch of 1 024
    (k_lm_step_quad) cycling through the two turned windows and their unturned twins: iteration count, termination and the states after
    every iteration (1e-6) against the oracle, whose sensitivity here is <= 2e-13 (tests/test_oracle_large_rotation.py).
    The test prints its measured worst errors before it asserts."""
    import torch
    prm, orc = env
    cap = lr.TRACK_CASES[0][2]
    base, priors, clss = [], [], []
    for seed, yaw, cp in lr.TRACK_CASES:
        assert cp == cap
        for y, nudge in ((yaw, 0.0), (0.0, 0.01)):
            w, prior, c = lr.track_case(synth, pyoracle, orc, prm, seed, y, nudge=nudge)
            base.append(w)
            priors.append(prior)
            clss += [dict(x, turned=(y != 0.0)) for x in c]
    lr.assert_margins(clss)
    assert all((c["trace"] <= 0.0) == c["turned"] for c in clss) and {c["cw_sign"] for c in clss if c["turned"]} == {1, -1}
    orc.set_max_iterations(cap)
    want = []
    try:
        for w, prior in zip(base, priors):
            wo = pyoracle.Window(w)
            orc.set_prior(prior)
            orc.solve(wo)
            want.append((orc.summary(), orc.iterations(), wo["states"].reshape(2, 15).copy()))
    finally:
        orc.set_max_iterations(50)
        orc.set_prior(None)
    for k in (0, 2):
        assert lr.iterations_beyond_120_degrees(want[k][1], base[k], prm) >= 1
    w1 = 0.0
    for k in (0, 2):
        slv = liw.Solver(prm)
        wg = liw.Window(base[k])
        slv.set_prior(priors[k])
        slv.set_window(wg)
        sg = slv.solve(cap)
        so, its, xo = want[k]
        assert (sg["iterations"], sg["termination"]) == (so["iterations"], so["termination"]), (k, sg, so)
        hg = slv.history()
        assert len(hg) == len(its)
        w1 = max(w1, _check_history(hg, its, 2, "single window %d" % k))
        assert rel_inf(np.asarray(wg["states"]).reshape(2, 15), xo) <= 1e-6
    B = 1024
    bs = liw.BatchSolver(prm, [base[b % 4] for b in range(B)], history_records=cap + 2)
    for key, j, per in (("prior_X", 0, 15), ("prior_J", 1, 225), ("prior_R", 2, 15)):
        a = np.concatenate([np.asarray(priors[b % 4][j], dtype=np.float64).reshape(per) for b in range(B)])
        bs.t[key].copy_(torch.from_numpy(a).to(bs.dev))
    bs.t["has_prior"].fill_(1)
    bs.solve(liw.LIW_MODE_TRACK, cap)
    got, summ, hist = bs.states(), bs.summaries(), bs.history()
    wb = 0.0
    for k in range(4):
        so, its, xo = want[k]
        for b in (k, 4 * (B // 8) + k, B - 4 + k):
            assert (summ[b]["iterations"], summ[b]["termination"]) == (so["iterations"], so["termination"]), (k, b, summ[b], so)
            wb = max(wb, _check_history(hist[:, b], its, 2, "batch window %d" % b))
            assert rel_inf(got[b], xo) <= 1e-6, (k, b)
    bs.close()
    print("turned tracking solves: worst state error over all iterations: single window %.2e, batch of 1024 %.2e" % (w1, wb))


# ------------------------------------------------------------------------------------------------ 4. pose graph
@pytest.fixture(scope="module")
def turned_graph(liw, synth):
    prm = synth.office_params()
    return lr.turned_pose_graph(liw.posegraph.make_pose_graph(prm, N=40, seed=4, n_loop=6))


def test_posegraph_normal_equations_with_turned_edges(liw, pyoracle, env, turned_graph):
    """make_pose_graph(N = 40, n_loop = 6) with the error rotation of one loop edge per pivot and sign (2.6 about +-x, +-y, 3.0 about +-z),
    a sequential edge turned by 2.4, a turned loop edge on the constant key frame and one turned edge once more in the reverse direction:
    edge_res (k_posegraph.hip) through every arm.  cost <= 1e-12 relative, g and H <= 1e-10 of their maxima, H symmetric, five repeated
    linearisations bit-identical.  The test prints its measured worst errors before it asserts."""
    prm, orc = env
    G, cls = turned_graph
    lr.assert_margins(cls)
    lr.assert_coverage(cls, wrapped=True)
    const = int(G["seq_idx"][0, 0])
    assert any(c["kind"] == "seq" and c["trace"] <= 0.0 for c in cls)
    assert any(c["kind"] == "loop" and c["trace"] <= 0.0 and const in G["loop_idx"][c["edge"]] for c in cls)
    pairs = [tuple(sorted(e)) for e in G["loop_idx"].tolist()]
    assert len(set(pairs)) < len(pairs)                                   # the edge duplicated in reverse
    pg = liw.posegraph.office_pg_params()
    pgs = liw.posegraph.PoseGraph(prm)
    args = (G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"])
    runs = [pgs.linearize(pg, *args) for _ in range(5)]
    for Hk, gk, ck in runs[1:]:
        assert np.array_equal(Hk, runs[0][0]) and np.array_equal(gk, runs[0][1]) and ck == runs[0][2]
    Hg, gg, cg = runs[0]
    Ho, go, co, idx = pyoracle.posegraph_linearize(orc, pg, *args)
    ec, eg, eH = abs(cg - co) / co, np.abs(gg[idx] - go).max() / np.abs(go).max(), np.abs(Hg[np.ix_(idx, idx)] - Ho).max() / np.abs(Ho).max()
    print("pose graph with turned edges: cost %.2e g %.2e H %.2e" % (ec, eg, eH))
    assert np.isfinite(Hg).all() and np.isfinite(gg).all()
    assert ec <= 1e-12 and eg <= 1e-10 and eH <= 1e-10
    assert np.array_equal(Hg, Hg.T)


def test_posegraph_solve_with_turned_edges(liw, pyoracle, env, turned_graph, monkeypatch):
    """solve(max_iters = 5) on the same graph against the oracle's minimizer (same iterations, termination, successful steps; poses
    1e-6; the oracle moves 1e-13 under a 1e-15 perturbation, tests/test_oracle_large_rotation.py), and the chain-segment path against
    the dense factorisation (LIW_PG_DENSE=1) at the 1e-9 bars of test_chain_segment_path_equals_dense_path.
    The test prints its measured worst errors before it asserts."""
    prm, orc = env
    G, cls = turned_graph
    lr.assert_margins(cls)
    lr.assert_coverage(cls, wrapped=True)
    monkeypatch.delenv("LIW_PG_DENSE", raising=False)
    pg = liw.posegraph.office_pg_params()
    pgs = liw.posegraph.PoseGraph(prm)
    args = (G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"])
    xg, sg = pgs.solve(pg, *args, max_iters=5)
    xo, so = pyoracle.posegraph_solve(orc, pg, *args, max_iters=5)
    e = float(np.abs(xg - xo).max() / max(1.0, np.abs(xo).max()))
    print("pose-graph solve, 5 iterations: poses %.2e" % e)
    assert (sg["iterations"], sg["termination"], sg["successful"]) == (so["iterations"], so["termination"], so["successful"]), (sg, so)
    assert e <= 1e-6
    pgn = dict(pg, use_ground_q_factor=False)
    xs, ss = pgs.solve(pgn, *args, max_iters=12)
    monkeypatch.setenv("LIW_PG_DENSE", "1")
    xd, sd = pgs.solve(pgn, *args, max_iters=12)
    monkeypatch.delenv("LIW_PG_DENSE")
    ex, ecost = float(np.abs(xs - xd).max() / max(1.0, np.abs(xd).max())), abs(ss["final_cost"] - sd["final_cost"]) / sd["final_cost"]
    print("chain-segment path vs dense path: poses %.2e final cost %.2e" % (ex, ecost))
    assert (ss["iterations"], ss["termination"], ss["successful"]) == (sd["iterations"], sd["termination"], sd["successful"])
    assert ex <= 1e-9 and ecost <= 1e-9


# ------------------------------------------------------------------------------------------------ 5. pre-integration
def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.fixture(scope="module")
def intervals():
    """spin intervals interleaved with the 1-, 2-, 5- and 41-sample ones: lanes of a wave run different lengths and arms"""
    spins = [lr.spin_intervals(tot, ax, seed=i) for i, (tot, ax) in enumerate(lr.SPINS)]
    small_imu, small_wheel = lr.small_intervals()
    imu, wheel = [], []
    for i, sp in enumerate(spins):
        imu += [sp["imu"], small_imu[i % 4]]
        wheel += [sp["wheel"], small_wheel[i % 4]]
    return spins, imu, wheel


def _spin_coverage(spins):
    ends = [c for sp in spins for c in sp["classes"]]
    lr.assert_margins(ends)
    lr.assert_coverage(ends, wrapped=True)
    lr.assert_coverage([c for sp in spins for c in sp["steps"]], wrapped=True)
    assert sum(sp["total"] > lr.PI for sp in spins) >= 4


def test_batch_imu_preint_on_spin_intervals(liw, env, intervals):
    """One BatchPreint.imu launch over 2 s / 400-sample constant-rate turns of 2.2 about x, y, z and -x, 3.0 and 3.3 about z, 3.3 about
    (.1,1,.1), 5.0 about -z and 6.5 about (.05,.05,1) — the accumulated rotation passes 120 deg with every pivot and pi with either sign
    on the way — interleaved with short intervals.  X, J, Dt <= 1e-12, sqrt_inverse_P <= 1e-8 against the oracle's sequential
    accumulator, U upper triangular, U^T U P = I to 1e-6.  The test prints its measured worst errors before it asserts."""
    prm, orc = env
    spins, imu, _ = intervals
    _spin_coverage(spins)
    bp = liw.BatchPreint(prm)
    X, J, S, Dt = [t.cpu().numpy() for t in bp.imu(imu)]
    P = bp.last_P.cpu().numpy()
    worst = dict(X=0.0, J=0.0, S=0.0, Dt=0.0, UUP=0.0)
    for m, iv in enumerate(imu):
        Xo, Jo, So, Dto = orc.imu_preint(*iv)
        if m % 2 == 0:      # the classification is of the nominal end rotation: the accumulated one is within 0.01 rad of it
            sp = spins[m // 2]
            assert np.linalg.norm(lr.log_so3(lr.exp_so3(sp["total"] * sp["axis"]).T @ lr.exp_so3(Xo[6:9]))) <= 0.01
        e = dict(X=relerr(X[m], Xo), J=relerr(J[m], Jo), S=relerr(S[m], So), Dt=abs(Dt[m] - Dto) / max(1.0, abs(Dto)),
                 UUP=float(np.abs(S[m].T @ S[m] @ P[m] - np.eye(15)).max()))
        worst = {k: max(worst[k], e[k]) for k in e}
        assert np.abs(np.tril(S[m], -1)).max() == 0.0, m
    print("batched IMU pre-integration on spin intervals: " + " ".join("%s %.1e" % kv for kv in worst.items()))
    assert worst["X"] <= 1e-12 and worst["J"] <= 1e-12 and worst["Dt"] <= 1e-12 and worst["S"] <= 1e-8 and worst["UUP"] <= 1e-6, worst


def test_batch_wheel_preint_on_spin_intervals(liw, env, intervals):
    """One BatchPreint.wheel launch over the same turns: the final log_SO3 of the accumulated increment (k_preint.hip) takes every
    pivot with either sign.  delta_Tij <= 1e-12 (absolute, as test_gpu_preint.py), Dt <= 1e-12, sqrt_inverse_P <= 1e-10.
    The test prints its measured worst errors before it asserts."""
    prm, orc = env
    spins, _, wheel = intervals
    _spin_coverage(spins)
    bp = liw.BatchPreint(prm)
    T, S, Dt = [t.cpu().numpy() for t in bp.wheel(wheel)]
    worst = dict(T=0.0, S=0.0, Dt=0.0)
    for m, iv in enumerate(wheel):
        To, So, Dto = orc.wheel_preint(*iv)
        if m % 2 == 0:
            sp = spins[m // 2]
            assert np.linalg.norm(lr.log_so3(lr.exp_so3(sp["total"] * sp["axis"]).T @ np.asarray(To)[:9].reshape(3, 3))) <= 0.01
        e = dict(T=float(np.abs(T[m] - np.asarray(To)).max()), S=relerr(S[m], So), Dt=abs(Dt[m] - Dto) / max(1.0, abs(Dto)))
        worst = {k: max(worst[k], e[k]) for k in e}
    print("batched wheel pre-integration on spin intervals: " + " ".join("%s %.1e" % kv for kv in worst.items()))
    assert worst["T"] <= 1e-12 and worst["Dt"] <= 1e-12 and worst["S"] <= 1e-10, worst


class _Recorder:
    def __init__(self, inner):
        self.inner, self.imu, self.wheel = inner, [], []

    def imu_preint(self, samples, t_start, t_end, bias6):
        self.imu.append((np.array(samples), float(t_start), float(t_end), np.array(bias6)))
        return self.inner.imu_preint(samples, t_start, t_end, bias6)

    def wheel_preint(self, samples, t_start, t_end):
        self.wheel.append((np.array(samples), float(t_start), float(t_end)))
        return self.inner.wheel_preint(samples, t_start, t_end)


def test_spinning_window_from_device_preintegration_feeds_the_solver(liw, synth, pyoracle, env):
    """A window of four frames 8 s apart on the 0.3 rad/s arc: every IMU block accumulates 2.4 rad (trace <= 0 in the accumulator and in
    the wheel role).  Its blocks from the device pre-integration solve to the same states as the window built with the oracle's
    accumulators (1e-6, as test_batch_preint_feeds_the_solver; the oracle moves 3e-11 here under a 1e-13 perturbation of the IMU means).
    The test prints its measured worst errors before it asserts."""
    prm, orc = env
    rec = _Recorder(orc)
    w = synth.make_window(rec, prm, seed=61, n=4, L=40, frame_dt=8.0)
    cls = [c for c in lr.window_classes(w, prm) if c["role"] != "imu"] + [lr.classify(lr.exp_so3(x[6:9]), role="gamma") for x in w["imu_X"]]
    lr.assert_margins(cls)
    assert all(c["trace"] <= 0.0 for c in cls)
    bp = liw.BatchPreint(prm)
    X, J, S, Dt = [t.cpu().numpy() for t in bp.imu(rec.imu)]
    T, Sw, Dtw = [t.cpu().numpy() for t in bp.wheel(rec.wheel)]
    assert relerr(X, w["imu_X"]) <= 1e-12 and np.abs(T - w["wheel_T"]).max() <= 1e-12
    w2 = dict(w)
    w2.update(imu_X=X, imu_J=J.reshape(-1, 225), imu_sqrtP=S.reshape(-1, 225), imu_Dt=Dt, wheel_T=T, wheel_sqrtP=Sw.reshape(-1, 9), wheel_Dt=Dtw)
    out = []
    for ww in (w, w2):
        bs = liw.BatchSolver(prm, [ww])
        bs.solve(liw.LIW_MODE_INIT, 50)
        out.append((bs.states()[0].copy(), bs.summaries()[0]))
        bs.close()
    e = float(np.abs(out[0][0] - out[1][0]).max() / max(1.0, np.abs(out[0][0]).max()))
    print("spinning window, device blocks vs oracle blocks: solved states %.2e" % e)
    assert out[0][1]["iterations"] == out[1][1]["iterations"]
    assert e <= 1e-6
    wo = pyoracle.Window(w)
    orc.set_prior(None)
    orc.init_solve(wo)
    assert out[0][1]["iterations"] == orc.summary()["iterations"] and rel_inf(out[0][0], wo["states"].reshape(4, 15)) <= 1e-6
