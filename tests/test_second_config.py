"""CPU guards of the second, anisotropic parameter set (tests/second_config.py), which tests/test_gpu_second_config.py runs the kernels at:

  * the set differs from synth.office_params() where it has to (every scalar, three distinct components per vector, generic rotations);
  * its inputs DISCRIMINATE: a reversed sigma vector, Rz^T for Rz in the noise term, the office gravity, swapped ground weights and a
    transposed extrinsic rotation each move a reference of the GPU tests by more than 1000 x the bar that reference is compared at;
  * the oracle is pinned at this set by tests/golden/factors_golden_cfg2.json (torch autograd / numpy restatements written from the
    reference's formulas, `python tests/golden/make_golden.py cfg2`), at the bars of test_oracle_golden.py / test_oracle_golden_solver.py;
  * the host pre-integrator agrees with the numpy restatement at the bars of test_gpu_preint.py;
  * the oracle's LM path on the windows of the short solves is determined far below the 1e-6 the GPU solves are compared at."""
import json
import os

import numpy as np
import pytest

import second_config as sc
from parity_util import init_solve_sensitivity

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "factors_golden_cfg2.json")))
TOL = 1e-8            # test_oracle_golden.py
BAR_FACTOR = 1e-10    # per-factor bar of the GPU tests, relative to max(1, |ref|_inf)
BAR_SQRTP = 1e-8      # sqrt_inverse_P bar of the GPU tests


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def env(synth, pyoracle):
    prm = sc.skewed_params(synth)
    return prm, pyoracle.Oracle(prm)


@pytest.fixture(scope="module")
def intervals(synth, env):
    prm, orc = env
    return sc.preint_intervals(synth, orc, prm)


# ------------------------------------------------------------------------------------------------ the configuration
@pytest.mark.parametrize("normalized", [True, False])
def test_second_configuration_differs_from_the_office_one(synth, normalized):
    off, prm = synth.office_params(), sc.skewed_params(synth, normalized)
    assert set(prm) == set(off) and prm["normalize_extrinsics"] is normalized and prm["fast_mode"] is False
    scalars = [prm[k] for k in sc.SCALARS]
    assert all(prm[k] != off[k] for k in sc.SCALARS) and len(set(scalars)) == len(scalars)
    for k in sc.VECTORS:
        assert len(set(prm[k])) == 3 and list(prm[k]) != list(off[k]), k
    for key, Rs, Ro in zip(("T_imu_to_wheel", "T_imu_to_laser"), sc.solver_rotations(prm), sc.solver_rotations(off)):
        assert sc.rotation_distance(synth, Ro, Rs) >= 0.3, key
        # generic: no entry of the rotation is within 0.1 of 0 or within 0.03 of +-1, the way every office entry is
        assert np.abs(Rs).min() >= 0.1 and np.abs(Rs).max() <= 0.97, (key, Rs)
        assert not np.array_equal(np.asarray(prm[key]).reshape(4, 4)[:3, 3], np.asarray(off[key]).reshape(4, 4)[:3, 3])
    raw = np.asarray(sc.skewed_params(synth)["T_imu_to_laser"]).reshape(4, 4)[:3, :3]
    assert np.abs(raw.T @ raw - np.eye(3)).max() >= 1e-3                     # the loader's round trip has work to do ...
    mg, _ = sc.golden_modules()
    assert np.abs(mg.quat_round_trip(raw) - raw).max() >= 1e-3               # ... and does it
    # both variants hand the solver the same matrices
    for a, b in zip(sc.solver_rotations(sc.skewed_params(synth, True)), sc.solver_rotations(sc.skewed_params(synth, False))):
        assert np.array_equal(a, b)


def test_round_trip_restatement_matches_the_oracle_loader(synth, pyoracle):
    """mg.quat_round_trip (both arms: the wheel rotation has a negative trace) against the oracle's normalize_tf, seen through a ground
    residual (wheel) and a laser residual evaluated with the matrices given raw + normalised, and given round-tripped + as they are"""
    a, b = pyoracle.Oracle(sc.skewed_params(synth, True)), pyoracle.Oracle(sc.skewed_params(synth, False))
    assert np.trace(sc.solver_rotations(sc.skewed_params(synth))[0]) < -0.1
    d = synth.make_window(a, sc.skewed_params(synth), seed=5, n=3, L=6)
    fa, fb = sc.factor_values(a, d), sc.factor_values(b, d)
    for kind in fa:
        assert sc.factor_move(fa, fb, kind) <= 1e-13, kind


# ------------------------------------------------------------------------------------------------ the inputs discriminate
def test_preintegration_inputs_expose_noise_mistakes(env, intervals):
    """Each sigma vector reversed in turn, and Rz^T for Rz in G (imu_preintegraption.h:196): sqrt_inverse_P of the numpy restatement
    moves by >= 1e-4 relative on at least one of the intervals the GPU test runs — four orders above its 1e-8 bar.  (At the office set
    every one of these moves is zero or round-off.)"""
    prm, _ = env
    imu, _ = intervals
    moves = sc.sqrtP_moves(prm, imu)
    print("sqrt_inverse_P moves:", " ".join("%s %.2e;" % kv for kv in moves.items()))
    assert len(moves) == 5
    for name, m in moves.items():
        assert m >= 1e-4 and m >= 1000 * BAR_SQRTP, (name, m)


def test_office_noise_hides_the_same_mistakes(synth, intervals):
    """the reason for the second set: at the isotropic office noise a reversed vector changes nothing at all and Rz^T in G moves
    sqrt_inverse_P by less than the 1e-8 bar on the recorded windows"""
    imu, _ = intervals
    moves = sc.sqrtP_moves(synth.office_params(), imu[:8])
    assert all(m == 0.0 for k, m in moves.items() if k.startswith("reversed")), moves
    assert moves["Rz^T in G"] <= BAR_SQRTP, moves


def test_factor_inputs_expose_parameter_mistakes(synth, pyoracle, env):
    """The per-factor window of the GPU test (n = 6, L = 24) evaluated by the oracle at parameter sets with one mistake each.  The factor
    type that reads the parameter moves by more than 1000 x the 1e-10 per-factor bar, the others do not move."""
    prm, orc = env
    d = synth.make_window(orc, prm, seed=5, n=6, L=24)
    ref = sc.factor_values(orc, d)
    reads = {"g = 9.8": ("imu",), "ground weights swapped": ("ground",), "Ril transposed": ("laser",), "Riw transposed": ("wheel", "ground")}
    muts = sc.devparam_mutations(prm)
    assert set(muts) == set(reads)
    for name, p in muts.items():
        alt = sc.factor_values(pyoracle.Oracle(p), d)
        moves = {k: sc.factor_move(ref, alt, k) for k in ref}
        print(name, " ".join("%s %.2e" % kv for kv in moves.items()))
        for k, m in moves.items():
            if k in reads[name]:
                assert m >= 1000 * BAR_FACTOR, (name, k, m)
            else:
                assert m <= 1e-12, (name, k, m)


def test_gravity_of_the_generated_window_shows_in_the_imu_residuals(synth, env):
    """the same window generated with g = 9.8 (accelerometer samples carry g): the oracle's IMU residuals at g = 9.78 move by far
    more than 1000 x the per-factor bar — what a stale DevParams.g would do"""
    prm, orc = env
    d = synth.make_window(orc, prm, seed=5, n=6, L=24)
    d98 = synth.make_window(orc, dict(prm, g=9.8), seed=5, n=6, L=24)
    assert np.array_equal(d["states"], d98["states"]) and np.array_equal(d["wheel_T"], d98["wheel_T"])
    m = sc.factor_move(sc.factor_values(orc, d), sc.factor_values(orc, d98), "imu")
    print("IMU residuals, window generated at g = 9.8: %.2e" % m)
    assert m >= 1000 * BAR_FACTOR


# ------------------------------------------------------------------------------------------------ the oracle pinned at this set
def test_golden_file_is_of_this_configuration(synth):
    prm = sc.skewed_params(synth)
    assert G["params"] == json.loads(json.dumps(prm))


@pytest.fixture(scope="module")
def orc_golden(pyoracle):
    return pyoracle.Oracle(G["params"])


def test_factors_golden_at_the_second_configuration(orc_golden):
    orc = orc_golden
    assert len(G["laser"]) >= 3 and len(G["imu"]) >= 1 and len(G["wheel"]) >= 1 and len(G["ground"]) >= 2
    for c in G["laser"]:
        x = np.array(c["x"])
        r, J = orc.eval_laser(c["pts"], x[0:3], x[3:6], x[6:9], x[9:12])
        assert close(r, c["res"]) and close(J, c["jac"])
    for c in G["imu"]:
        x = np.array(c["x"])
        r, J = orc.eval_imu(c["X"], c["J"], c["sqrtP"], c["Dt"], x[:15], x[15:])
        assert close(r, c["res"]) and close(J, c["jac"])
    for c in G["wheel"]:
        x = np.array(c["x"])
        r, J = orc.eval_wheel(c["T"], c["sqrtP"], x[0:3], x[3:6], x[6:9], x[9:12])
        assert close(r, c["res"]) and close(J, c["jac"])
    for c in G["ground"]:
        x = np.array(c["x"])
        r, J = orc.eval_ground(x[0:3], x[3:6])
        assert close(r, c["res"]) and close(J, c["jac"])


def test_window_normal_equations_golden_at_the_second_configuration(orc_golden, pyoracle):
    w = G["window_init"]
    win = pyoracle.Window({k: (np.array(v) if k != "n" else v) for k, v in w["window"].items()})
    H, g, cost = orc_golden.linearize(win, 0)
    assert abs(cost - w["cost"]) <= 1e-10 * w["cost"]
    assert close(H, w["H"], 1e-8) and close(g, w["g"], 1e-8)


def test_preintegration_golden_at_the_second_configuration(orc_golden):
    assert len(G["preint"]["imu"]) + len(G["preint"]["wheel"]) == 5
    for c in G["preint"]["imu"]:
        X, J, S, Dt = orc_golden.imu_preint(np.array(c["samples"]), c["t_start"], c["t_end"], np.array(c["bias"]))
        assert abs(Dt - c["Dt"]) <= 1e-15
        assert rel(X, c["X"]) <= 1e-12 and rel(J, c["J"]) <= 1e-12
        assert rel(S, c["sqrt_inverse_P"]) <= 1e-8
    for c in G["preint"]["wheel"]:
        T, S, Dt = orc_golden.wheel_preint(np.array(c["samples"]), c["t_start"], c["t_end"])
        assert abs(Dt - c["Dt"]) <= 1e-15
        assert rel(T, c["T"]) <= 1e-12 and rel(S, c["sqrt_inverse_P"]) <= 1e-12


def test_oracle_and_host_preintegrators_match_the_numpy_restatement(liw, env, intervals):
    """Every interval of the GPU test through three fp64 implementations of the same recursion: the oracle and the product's host
    accumulator (liw.HostPreint: no GPU needed) against make_golden_solver.imu_preint_numpy / wheel_preint_numpy.  X, J, Dt 1e-12,
    sqrt_inverse_P 1e-8 (wheel: 1e-12 absolute on delta_Tij, 1e-10) — the bars of test_gpu_preint.py.  Measured: sqrt_inverse_P within
    1.4e-11 of the restatement in both, X and J within 1e-14."""
    prm, orc = env
    imu, wheel = intervals
    _, mgs = sc.golden_modules()
    host = liw.HostPreint(prm)
    worst = dict(X=0.0, J=0.0, S=0.0, Dt=0.0, wT=0.0, wS=0.0)
    for iv in imu:
        Xn, Jn, Sn, Dtn = mgs.imu_preint_numpy(prm, *iv)
        for Xa, Ja, Sa, Dta in (orc.imu_preint(*iv), host.imu_preint(*iv)):
            e = dict(X=rel(Xa, Xn), J=rel(Ja, Jn), S=rel(Sa, Sn), Dt=abs(Dta - Dtn) / max(1.0, abs(Dtn)))
            worst.update({k: max(worst[k], v) for k, v in e.items()})
            assert np.abs(np.tril(np.asarray(Sa).reshape(15, 15), -1)).max() == 0.0
    for iv in wheel:
        Tn, Sn, Dtn = mgs.wheel_preint_numpy(prm, *iv)
        for Ta, Sa, Dta in (orc.wheel_preint(*iv), host.wheel_preint(*iv)):
            worst["wT"], worst["wS"] = max(worst["wT"], float(np.abs(np.asarray(Ta) - Tn).max())), max(worst["wS"], rel(Sa, Sn))
            assert abs(Dta - Dtn) <= 1e-12 * max(1.0, abs(Dtn))
    print("oracle and host accumulator vs numpy restatement: " + " ".join("%s %.1e" % kv for kv in worst.items()))
    assert worst["X"] <= 1e-12 and worst["J"] <= 1e-12 and worst["Dt"] <= 1e-12 and worst["S"] <= 1e-8, worst
    assert worst["wT"] <= 1e-12 and worst["wS"] <= 1e-10, worst


def test_wheel_interval_has_three_distinct_weights(env, intervals):
    prm, orc = env
    _, wheel = intervals
    T, S, _ = orc.wheel_preint(*wheel[sc.wheel_interval_with_three_weights(wheel)])
    S, s = np.asarray(S).reshape(3, 3), prm["wheel_sigma"]
    assert np.count_nonzero(S - np.diag(np.diag(S))) == 0 and len({float(v) for v in np.diag(S)}) == 3
    assert abs(S[0, 0] / S[1, 1] - s[1] / s[0]) <= 1e-12 * s[1] / s[0]          # both scale with 1 / |dp|: their ratio is the sigmas' alone
    dp = np.asarray(T)[9:12]
    assert dp @ dp > 0.005 ** 2 and abs(S[0, 0] - 1.0 / (s[0] * np.sqrt(dp @ dp))) <= 1e-12 * S[0, 0]


# ------------------------------------------------------------------------------------------------ the solves are determined
@pytest.mark.parametrize("n,L", sc.SOLVE_SHAPES)
def test_short_solves_are_determined_far_below_their_bar(synth, pyoracle, env, n, L):
    """parity_util.init_solve_sensitivity (the oracle against itself, IMU means scaled by 1 + 1e-13 N(0,1)) on the windows the GPU
    solves run: <= 1e-11 through the 8 iterations of the capped batched solves (measured <= 3e-13) and <= 1e-7 to the natural end
    (measured <= 4.1e-8: seed 2 at n = 6 runs into the cap of 50), against the 1e-6 the GPU states are compared at"""
    prm, orc = env
    try:
        for seed in sc.SEEDS:
            w = synth.make_window(orc, prm, seed=seed, n=n, L=L)
            for cap, bar in ((sc.SOLVE_CAP, 1e-11), (50, 1e-7)):
                orc.set_max_iterations(cap)
                wo = pyoracle.Window(w)
                orc.set_prior(None)
                orc.init_solve(wo)
                its = orc.iterations()
                sens = init_solve_sensitivity(pyoracle, orc, w, its)
                print("n=%d seed %d cap %d: %d iterations, sensitivity %.2e" % (n, seed, cap, orc.summary()["iterations"], sens.max()))
                assert sens.max() <= bar, (seed, cap, sens.max())
    finally:
        orc.set_max_iterations(50)
        orc.set_prior(None)
