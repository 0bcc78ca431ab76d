"""The reference the large-rotation GPU tests lean on (tests/test_gpu_large_rotation.py), checked without a GPU on the inputs of
tests/large_rotation_cases.py: the oracle's Jets against central finite differences with `log_SO3` in every arm (trace > 0; trace <= 0
with pivot 0 / 1 / 2 and either sign of the scalar part), the product's host pre-integrators (the same liw_dual.hpp templates the
device kernels instantiate) against the oracle on turns beyond 120 deg and beyond pi, and the round-off sensitivity of the solves
whose LM iterates the GPU tests compare.

Tolerances: finite differences 1e-8 relative (h = 1e-6: truncation ~ h^2, cancellation ~ 1e-16 |r| / h; measured <= 7.4e-10 on the
factors, 1.5e-9 on the pose-graph gradient); pre-integration at the bars of tests/test_gpu_preint.py."""
import numpy as np
import pytest

import large_rotation_cases as lr
from parity_util import init_solve_sensitivity


@pytest.fixture(scope="module")
def env(synth, pyoracle):
    prm = synth.office_params()
    return prm, pyoracle.Oracle(prm)


def central_differences(f, x, h=1e-6):
    x = np.array(x, dtype=np.float64)
    cols = []
    for i in range(x.size):
        a, b = x.copy(), x.copy()
        a[i] += h
        b[i] -= h
        cols.append((f(a) - f(b)) / (2.0 * h))
    return np.array(cols).T


def test_classifier_names_the_arm_of_a_known_rotation():
    """the numpy classification on rotations whose arm is known by construction"""
    for axis, pivot in (((1, .1, .1), 0), ((.1, 1, .1), 1), ((.1, .1, 1), 2)):
        for sgn in (1, -1):
            c = lr.classify(lr.exp_so3(lr.turn(2.7, sgn * np.asarray(axis))))
            assert c["arm"] == (pivot, sgn) and abs(c["angle"] - 2.7) < 1e-12 and c["wrapped"] == (sgn < 0)
    assert lr.classify(lr.exp_so3(lr.turn(2.0, (1, 2, 3))))["arm"] == "pos"           # 2.0 < 120 deg
    with pytest.raises(AssertionError):
        lr.assert_margins([lr.classify(lr.exp_so3(lr.turn(2.1, (1, 0, 0))))])          # trace = 1 + 2 cos 2.1 = -0.0097
    with pytest.raises(AssertionError):
        lr.assert_margins([lr.classify(lr.exp_so3(lr.turn(3.135, (1, 0, 0))))])
    with pytest.raises(AssertionError):
        lr.assert_margins([lr.classify(lr.exp_so3(lr.turn(2.7, (1, 1, 0.1))))])        # two pivots tie
    with pytest.raises(AssertionError):
        lr.assert_coverage([lr.classify(lr.exp_so3(lr.turn(2.7, (1, 0, 0))))])


def test_oracle_factor_jacobians_match_finite_differences(synth, env):
    prm, orc = env
    w, cls = lr.factor_window(synth, orc, prm)
    lr.assert_margins(cls)
    lr.assert_coverage(lr.by_role(cls, "imu"), wrapped=True)
    lr.assert_coverage(lr.by_role(cls, "wheel"), wrapped=True)
    assert sorted(c["block"] for c in lr.by_role(cls, "oq") if c["trace"] <= 0.0) == sorted(lr.FACTOR_WHEEL_ALONG)
    st, worst = w["states"], 0.0
    for k in range(int(w["n"]) - 1):
        imu = (w["imu_X"][k], w["imu_J"][k], w["imu_sqrtP"][k], w["imu_Dt"][k])
        r, J = orc.eval_imu(*imu, st[k], st[k + 1])
        Jf = central_differences(lambda x: orc.eval_imu(*imu, x[:15], x[15:])[0], np.concatenate([st[k], st[k + 1]]))
        assert np.isfinite(r).all() and np.isfinite(J).all()
        e_imu = float(np.abs(J - Jf).max() / max(1.0, np.abs(Jf).max()))
        whl = (w["wheel_T"][k], w["wheel_sqrtP"][k])
        r, J = orc.eval_wheel(*whl, st[k, 0:3], st[k, 3:6], st[k + 1, 0:3], st[k + 1, 3:6])
        Jf = central_differences(lambda x: orc.eval_wheel(*whl, x[0:3], x[3:6], x[6:9], x[9:12])[0], np.concatenate([st[k, :6], st[k + 1, :6]]))
        assert np.isfinite(r).all() and np.isfinite(J).all()
        e_whl = float(np.abs(J - Jf).max() / max(1.0, np.abs(Jf).max()))
        worst = max(worst, e_imu, e_whl)
        assert e_imu <= 1e-8 and e_whl <= 1e-8, (k, e_imu, e_whl)
    print("oracle Jets vs central differences, every arm: worst %.2e" % worst)


def test_oracle_posegraph_gradient_matches_finite_differences(liw, synth, pyoracle, env):
    prm, orc = env
    pg = liw.posegraph.office_pg_params()
    G, cls = lr.turned_pose_graph(liw.posegraph.make_pose_graph(prm, N=40, seed=4, n_loop=6))
    lr.assert_margins(cls)
    lr.assert_coverage(cls, wrapped=True)
    rest = (G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"])
    H, g, cost, idx = pyoracle.posegraph_linearize(orc, pg, G["poses"], *rest)
    assert np.isfinite(H).all() and np.isfinite(g).all()
    gf, h = np.zeros_like(g), 1e-6
    for t, fi in enumerate(idx):
        xp, xm = G["poses"].reshape(-1).copy(), G["poses"].reshape(-1).copy()
        xp[fi] += h
        xm[fi] -= h
        gf[t] = (pyoracle.posegraph_linearize(orc, pg, xp.reshape(-1, 6), *rest)[2] - pyoracle.posegraph_linearize(orc, pg, xm.reshape(-1, 6), *rest)[2]) / (2.0 * h)
    e = float(np.abs(g - gf).max() / np.abs(gf).max())
    print("pose-graph gradient vs central differences of the cost: %.2e" % e)
    assert e <= 1e-8


def test_posegraph_capped_solve_is_insensitive_to_round_off(liw, synth, pyoracle, env):
    """the referee for the GPU comparison of solve(max_iters=5): the oracle against itself with the poses scaled by 1 + 1e-15 N(0,1)"""
    prm, orc = env
    pg = liw.posegraph.office_pg_params()
    G, _ = lr.turned_pose_graph(liw.posegraph.make_pose_graph(prm, N=40, seed=4, n_loop=6))
    rest = (G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"])
    xo, so = pyoracle.posegraph_solve(orc, pg, G["poses"], *rest, max_iters=5)
    rp, worst = np.random.default_rng(7), 0.0
    for _ in range(3):
        xa, sa = pyoracle.posegraph_solve(orc, pg, G["poses"] * (1.0 + 1e-15 * rp.standard_normal(G["poses"].shape)), *rest, max_iters=5)
        assert (sa["iterations"], sa["termination"], sa["successful"]) == (so["iterations"], so["termination"], so["successful"])
        worst = max(worst, float(np.abs(xa - xo).max() / max(1.0, np.abs(xo).max())))
    print("pose-graph solve, 5 iterations: oracle moves %.2e under a 1e-15 perturbation" % worst)
    assert worst <= 1e-8                                       # measured 1.0e-13: the 1e-6 bar of the GPU test is a test of the kernels


def test_host_preintegrators_match_oracle_on_spin_intervals(liw, env):
    prm, orc = env
    host = liw.HostPreint(prm)
    rel = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / max(1e-300, np.abs(np.asarray(b)).max()))
    spins = [lr.spin_intervals(tot, ax, seed=i) for i, (tot, ax) in enumerate(lr.SPINS)]
    ends = [c for sp in spins for c in sp["classes"]]
    lr.assert_margins(ends)
    lr.assert_coverage(ends, wrapped=True)
    lr.assert_coverage([c for sp in spins for c in sp["steps"]], wrapped=True)
    assert sum(sp["total"] > lr.PI for sp in spins) >= 4                              # turns that pass pi on the way
    worst = dict(X=0.0, J=0.0, S=0.0, T=0.0, Sw=0.0)
    for sp in spins:
        Xo, Jo, So, Dto = orc.imu_preint(*sp["imu"])
        Xh, Jh, Sh, Dth = host.imu_preint(*sp["imu"])
        To, Swo, Dtwo = orc.wheel_preint(*sp["wheel"])
        Th, Swh, Dtwh = host.wheel_preint(*sp["wheel"])
        end = lr.exp_so3(sp["total"] * sp["axis"])                                   # the classification is of the nominal end rotation
        assert np.linalg.norm(lr.log_so3(end.T @ lr.exp_so3(Xo[6:9]))) <= 0.01 and np.linalg.norm(lr.log_so3(end.T @ np.asarray(To)[:9].reshape(3, 3))) <= 0.01
        e = dict(X=rel(Xh, Xo), J=rel(Jh, Jo), S=rel(Sh, So), T=float(np.abs(np.asarray(Th) - np.asarray(To)).max()), Sw=rel(Swh, Swo))
        worst = {k: max(worst[k], e[k]) for k in e}
        assert abs(Dth - Dto) <= 1e-12 * max(1.0, abs(Dto)) and abs(Dtwh - Dtwo) <= 1e-12 * max(1.0, abs(Dtwo))
        assert e["X"] <= 1e-12 and e["J"] <= 1e-12 and e["S"] <= 1e-8, (sp["total"], e)
        assert e["T"] <= 1e-12 and e["Sw"] <= 1e-10, (sp["total"], e)
    print("host pre-integrators vs oracle on the spin intervals: " + " ".join("%s %.1e" % kv for kv in worst.items()))


@pytest.mark.parametrize("seed,n,L,yaw,cap", lr.KIDNAP_CASES + lr.KIDNAP_MIRRORS)
def test_kidnapped_init_solves_pass_through_the_arms_and_are_well_conditioned(synth, pyoracle, env, seed, n, L, yaw, cap):
    """what the GPU solve comparison presumes of the oracle: LM iterates with a block beyond 120 deg in at least three iterations, and a
    per-iteration sensitivity to round-off (parity_util.init_solve_sensitivity) far below the 1e-6 bar (measured <= 1.8e-11)"""
    prm, orc = env
    w, cls = lr.kidnapped_case(synth, orc, prm, seed, n, L, yaw)
    lr.assert_margins(cls)
    assert all(c["trace"] <= 0.0 for c in cls)
    orc.set_prior(None)
    orc.set_max_iterations(cap)
    try:
        orc.init_solve(pyoracle.Window(w))
        its = orc.iterations()
        assert lr.iterations_beyond_120_degrees(its, w, prm) >= 3
        sens = init_solve_sensitivity(pyoracle, orc, w, its)
    finally:
        orc.set_max_iterations(50)
    print("kidnapped init solve seed %d: oracle sensitivity %.2e" % (seed, sens.max()))
    assert sens.max() <= 1e-8


@pytest.mark.parametrize("seed,yaw,cap", lr.TRACK_CASES)
def test_turned_tracking_solves_are_well_conditioned(synth, pyoracle, env, seed, yaw, cap):
    """the referee for the TRACK leg: oracle sensitivity below 1e-8 for the chosen seeds (measured <= 7e-14)"""
    prm, orc = env
    w, prior, cls = lr.track_case(synth, pyoracle, orc, prm, seed, yaw)
    lr.assert_margins(cls)
    assert all(c["trace"] <= 0.0 for c in cls)
    orc.set_max_iterations(cap)
    try:
        orc.set_prior(prior)
        orc.solve(pyoracle.Window(w))
        its = orc.iterations()
        assert lr.iterations_beyond_120_degrees(its, w, prm) >= 1
        sens = lr.track_solve_sensitivity(pyoracle, orc, w, prior, its)
    finally:
        orc.set_max_iterations(50)
        orc.set_prior(None)
    print("turned tracking solve seed %d: oracle sensitivity %.2e" % (seed, sens.max()))
    assert sens.max() < 1e-8
