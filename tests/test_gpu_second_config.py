"""GPU parity at the SECOND, anisotropic parameter set (tests/second_config.py): every solver-side consumer of the parameters — DevParams
(liw_kernels.hpp) through each linearisation route, PreintNoise through the pre-integration kernels, the pose graph's use of DevParams —
against the oracle at a set where no two scalars are equal, every sigma vector has three distinct components, the extrinsic rotations are
generic and the laser matrix needs the loader's quaternion round trip.  tests/test_second_config.py shows on the CPU that a reversed
sigma vector, Rz^T for Rz in the noise term, the office gravity, swapped ground weights or a transposed extrinsic rotation would each move
a reference used here by more than 1000 x its bar, pins the oracle at this set and checks that the solves below are determined.

The structure is that of tests/test_gpu_large_rotation.py; tolerances are those of the ordinary-window tests: factors
1e-10 * max(1, |ref|_inf) (test_gpu_parity.py); H, g TOL_HG = 1e-12 entry-scaled, 1e-12 per 15x15 and 1e-11 per 3x3 block, cost 1e-12
(parity_util.py); LM iterates 1e-6; marginalisation as test_gpu_bench_shape.py; pre-integration as test_gpu_preint.py; pose graph as
test_gpu_posegraph.py.  Every test prints its measured worst errors before it asserts."""
import importlib
import os
import sys

import numpy as np
import pytest

import second_config as sc
from parity_util import TOL_HG, block_rel_errors, normal_eq_errors, rel_inf
from test_gpu_large_rotation import SHAPES

pytestmark = pytest.mark.gpu

SWITCHES = ("LIW_NO_IMU_MULTI", "LIW_NO_IMU_PACK", "LIW_NO_LASER_SLAB", "LIW_SMALL_ND3", "LIW_STEP_VARIANT", "LIW_PG_DENSE")
# The lane-per-group laser kernels read the rows liw_batch_lm_begin packs only from 2 048 (slab, frame) waves on in the INIT topology and
# from 256 slabs on in the TRACK topology (laser_slab_begin, liw_capi.hip): 172 slabs x 12 frames, and 257 slabs.  Below that — at the
# B = 1 024 of the table — LIW_NO_LASER_SLAB changes nothing and the lane-per-block kernel runs either way.
B_SLAB_INIT_N12 = 64 * 171 + 1
B_SLAB_TRACK = 64 * 256 + 5


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def clear_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def bench_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("bench")


@pytest.fixture(scope="module")
def env(liw, synth, pyoracle):
    prm = sc.skewed_params(synth)
    return prm, pyoracle.Oracle(prm)


def batch_of(liw, prm, wins, B, **kw):
    """BatchSolver over B windows cycling through `wins` (large batches: tiled on the device from the distinct windows)"""
    nb = len(wins)
    if B <= 64:
        return liw.BatchSolver(prm, [wins[b % nb] for b in range(B)], **kw)
    n = int(wins[0]["n"])
    idx = np.arange(B) % nb
    st = np.stack([np.asarray(w["states"], dtype=np.float64).reshape(n, 15) for w in wins])[idx]
    mp = np.stack([np.asarray(w["match_pose"], dtype=np.float64).reshape(n, 12) for w in wins])[idx]
    return liw.BatchSolver(prm, wins, tile=dict(B=B, states=st, match_pose=mp), **kw)


def picks_of(B, nb):
    """the first, a middle and the last copy of each of the nb base windows"""
    return sorted({b for k in range(nb) for b in (k, nb * (B // (2 * nb)) + k, k + nb * ((B - 1 - k) // nb))})


# ------------------------------------------------------------------------------------------------ 1. per factor
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("nd3", [False, True])
def test_factor_residuals_and_jacobians_at_the_second_configuration(liw, synth, pyoracle, monkeypatch, nd3, normalized):
    """One window (n = 6, L = 24): residuals and ambient Jacobians of every laser, IMU, wheel and ground block against the oracle's Jets,
    with one derivative direction per lane (k_lin_all, small_nd = 1) and with LIW_SMALL_ND3 (the instantiation of the batched kernels);
    with the extrinsics given raw + normalize_extrinsics (the laser matrix is 4e-3 off orthonormal: normalize_tf_host does work) and
    given as the round trip leaves them + normalize_extrinsics off.  Bar 1e-10 * max(1, |ref|_inf)."""
    prm = sc.skewed_params(synth, normalized)
    orc = pyoracle.Oracle(prm)
    clear_switches(monkeypatch)
    if nd3:
        monkeypatch.setenv("LIW_SMALL_ND3", "1")
    n, L = 6, 24
    d = synth.make_window(orc, prm, seed=5, n=n, L=L)
    slv = liw.Solver(prm)
    Tw, Tl = slv.extrinsics()
    Riw, Ril = sc.solver_rotations(prm)
    assert np.abs(Tw[:3, :3] - Riw).max() <= 1e-15 and np.abs(Tl[:3, :3] - Ril).max() <= 1e-15     # what the context holds
    slv.set_window(liw.Window(d))
    f = slv.eval_factors(liw.LIW_MODE_INIT)
    slv.close()
    ref = sc.factor_values(orc, d)
    worst = dict(laser=0.0, imu=0.0, wheel=0.0, ground=0.0)
    for kind in worst:
        for j, (r, J) in enumerate(ref[kind]):
            worst[kind] = max(worst[kind], rel(f[kind + "_res"][j], r), rel(f[kind + "_jac"][j], J))
    print("per-factor worst errors (nd3=%s, normalized=%s): %s" % (nd3, normalized, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1e-10, worst


# ------------------------------------------------------------------------------------------------ 2. normal equations
@pytest.fixture(scope="module")
def base_windows(synth, pyoracle, env):
    """eight base windows per n (L = 4 n) and the oracle's normal equations of each in the INIT and MARG topologies: built once, shared,
    never modified"""
    prm, orc = env
    cache = {}

    def get(n):
        if n not in cache:
            wins, ref = [], []
            for k in range(8):
                w = synth.make_window(orc, prm, seed=300 + 10 * n + k, n=n, L=4 * n)
                wins.append(w)
                orc.set_prior(None)
                Ho, go, co = orc.linearize(pyoracle.Window(w), 0)
                orc.marginalization(pyoracle.Window(w))
                m = orc.marg_pieces()
                ref.append(dict(init=(Ho, go, co), marg=(m["H"], m["g"], 0.5 * float(m["R"] @ m["R"]))))
            orc.set_prior(None)
            cache[n] = (wins, ref)
        return cache[n]
    return get


@pytest.fixture(scope="module")
def track_windows(synth, pyoracle, env):
    """eight two-frame tracking windows with carried priors, and the oracle's TRACK-topology normal equations of each"""
    prm, orc = env
    wins, priors, ref = [], [], []
    for k in range(8):
        w, prior = sc.track_window(synth, pyoracle, orc, prm, seed=700 + k)
        orc.set_prior(prior)
        ref.append(orc.linearize(pyoracle.Window(w), 1))
        wins.append(w)
        priors.append(prior)
    orc.set_prior(None)
    return wins, priors, ref


def normal_equation_errors(H, g, c, picks, refs, with_blocks):
    worst = dict(cost=0.0, H=0.0, g=0.0, b15=0.0, b3=0.0)
    for q, b in enumerate(picks):
        Ho, go, co = refs[b % len(refs)]
        assert np.isfinite(H[q]).all() and np.isfinite(g[q]).all()
        eH, eg = normal_eq_errors(H[q], g[q], Ho, go, co)
        e = dict(H=eH, g=eg)
        if with_blocks:
            e.update(cost=abs(c[q] - co) / co, b15=block_rel_errors(H[q], Ho, 15), b3=block_rel_errors(H[q], Ho, 3))
        worst = {k: max(worst[k], e.get(k, 0.0)) for k in worst}
    return worst


def linearized(liw, bs, mode, route, B, nb=8):
    import torch
    if route == "bracket":
        bs.lm_begin(mode, 4)
        bs.lm_linearize(mode, 0)
    else:
        bs.linearize(mode)
    lp = bs.launch_paths()
    picks = picks_of(B, nb)
    H, g, c = bs.export_dense(mode)
    ix = torch.tensor(picks, device=H.device)
    return lp, picks, H[ix].cpu().numpy(), g[ix].cpu().numpy(), c[ix].cpu().numpy()


#         n   B                environment          route      topology   lane-per-group laser kernel armed
CASES = ([(n, B, e, r, "init", False) for n, B, e, rs in SHAPES for r in rs]
         + [(n, B, e, "plain", "marg", False) for n, B, e, rs in SHAPES if "plain" in rs]
         + [(12, 1024, "LIW_NO_LASER_SLAB", "bracket", "init", False),
            (12, B_SLAB_INIT_N12, None, "bracket", "init", True),
            (12, B_SLAB_INIT_N12, "LIW_NO_LASER_SLAB", "bracket", "init", False)])


@pytest.mark.parametrize("n,B,envvar,route,mode_name,slab", CASES)
def test_normal_equations_through_every_batched_kernel(liw, env, base_windows, monkeypatch, n, B, envvar, route, mode_name, slab):
    """H, g, cost of eight base windows per n against the oracle through each linearisation kernel — the (n, B, environment, route) rows
    of test_gpu_large_rotation.SHAPES (see there for the kernel behind each row), INIT and MARG topologies; the first, a middle and the
    last copy of each base window.  On top of that table: LIW_NO_LASER_SLAB on the (12, 1 024) bracket row, and the same row at 10 945
    windows, where 172 slabs x 12 frames arm the lane-per-group laser kernel over the packed slab rows (k_lin_laser_slab, asserted
    through launch_paths) — with and without LIW_NO_LASER_SLAB, so both laser routes meet the oracle.
    Bars: cost 1e-12, H and g TOL_HG = 1e-12 entry-scaled, 15x15 blocks 1e-12, 3x3 blocks 1e-11 (INIT); MARG as test_gpu_batch.py."""
    prm, orc = env
    wins, ref = base_windows(n)
    clear_switches(monkeypatch)
    if envvar:
        monkeypatch.setenv(envvar, "1")
    mode = liw.LIW_MODE_INIT if mode_name == "init" else liw.LIW_MODE_MARG
    bs = batch_of(liw, prm, wins, B)
    if route == "bracket":
        assert B * (n - 1) >= 4096                                  # the packing threshold of liw_batch_lm_begin
    lp, picks, H, g, c = linearized(liw, bs, mode, route, B)
    bs.close()
    if B >= 1024:
        assert lp["large_batch_format"], lp
    assert lp["lane_per_group_laser"] == slab, lp
    worst = normal_equation_errors(H, g, c, picks, [r[mode_name] for r in ref], mode_name == "init")
    print("n=%d B=%d %s %s %s: worst over %d sampled windows: %s" % (n, B, envvar, route, mode_name, len(picks), " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["H"] <= TOL_HG and worst["g"] <= TOL_HG, worst
    assert worst["cost"] <= 1e-12 and worst["b15"] <= 1e-12 and worst["b3"] <= 1e-11, worst


@pytest.mark.parametrize("B,envvar,slab", [(1024, None, False), (B_SLAB_TRACK, None, True), (B_SLAB_TRACK, "LIW_NO_LASER_SLAB", False)])
def test_track_topology_normal_equations_with_a_carried_prior(liw, env, track_windows, monkeypatch, B, envvar, slab):
    """TRACK topology, n = 2, bracket route, every window with the prior the oracle's marginalisation left: the merged wheel / ground
    role of the large-batch record format and the prior rows.  At 1 024 windows the lane-per-block laser kernel runs; at 16 389
    (257 slabs) the one-free-pose lane-per-group kernel k_lin_laser_slab1 over the packed rows, and with LIW_NO_LASER_SLAB the
    lane-per-block kernel again.  Same bars as the INIT rows; the constant blocks (older frame's pose) must be exactly zero."""
    import torch
    prm, orc = env
    wins, priors, ref = track_windows
    clear_switches(monkeypatch)
    if envvar:
        monkeypatch.setenv(envvar, "1")
    bs = batch_of(liw, prm, wins, B)
    for key, j, per in (("prior_X", 0, 15), ("prior_J", 1, 225), ("prior_R", 2, 15)):
        a = np.stack([np.asarray(p[j], dtype=np.float64).reshape(per) for p in priors])[np.arange(B) % 8].reshape(-1)
        bs.t[key].copy_(torch.from_numpy(a).to(bs.dev))
    bs.t["has_prior"].fill_(1)
    lp, picks, H, g, c = linearized(liw, bs, liw.LIW_MODE_TRACK, "bracket", B)
    bs.close()
    assert lp["large_batch_format"], lp
    assert lp["lane_per_group_laser"] == slab, lp
    for Ho, _, _ in ref:
        assert not np.diag(Ho)[0:6].any() and np.diag(Ho)[6:].all()           # older pose constant, everything else free
    worst = normal_equation_errors(H, g, c, picks, ref, True)
    print("TRACK n=2 B=%d %s bracket: worst over %d sampled windows: %s" % (B, envvar, len(picks), " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["H"] <= TOL_HG and worst["g"] <= TOL_HG, worst
    assert worst["cost"] <= 1e-12 and worst["b15"] <= 1e-12 and worst["b3"] <= 1e-11, worst


def test_no_stale_parameters_across_contexts(liw, synth, env, base_windows, monkeypatch):
    """One process, three contexts in a row on windows of the same shapes (n = 5, B = 1 024, bracket route): office parameters, closed;
    the second set; office parameters again.  The second meets the oracle at the second set (nothing of the first context's DevParams
    or packed records survives), the third is bit-identical to the first."""
    prm, orc = env
    off = synth.office_params()
    wins, ref = base_windows(5)
    clear_switches(monkeypatch)
    B, out = 1024, []
    for p in (off, prm, off):
        bs = batch_of(liw, p, wins, B)
        lp, picks, H, g, c = linearized(liw, bs, liw.LIW_MODE_INIT, "bracket", B)
        bs.close()
        assert lp["large_batch_format"]
        out.append((H, g, c))
    worst = normal_equation_errors(*out[1], picks, [r["init"] for r in ref], True)
    moved = max(rel(out[0][2], out[1][2]), 0.0)
    print("second context after an office one: %s; cost moved by %.2e between the sets" % (" ".join("%s %.2e" % kv for kv in worst.items()), moved))
    assert moved >= 1e-3                                             # the two sets give different numbers at all
    assert worst["H"] <= TOL_HG and worst["g"] <= TOL_HG, worst
    assert worst["cost"] <= 1e-12 and worst["b15"] <= 1e-12 and worst["b3"] <= 1e-11, worst
    for a, b in zip(out[0], out[2]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. solves
def _check_history(hist, its, n, what):
    worst = 0.0
    assert len(hist) >= len(its), what
    for k in range(len(its)):
        e = rel_inf(hist[k], its[k]["x"].reshape(n, 15))
        worst = max(worst, e)
        assert e <= 1e-6, (what, "iteration %d" % k, e)
    return worst


@pytest.fixture(scope="module")
def solve_windows(synth, pyoracle, env):
    """seeds 1 - 3 at (n, L) = (6, 24) and (12, 48), with the oracle's init solve of each at the cap of the batched solves and — n = 6 —
    to its natural end: (summary, iterations, final states).  Their sensitivity to round-off: tests/test_second_config.py."""
    prm, orc = env
    out = {}
    try:
        for n, L in sc.SOLVE_SHAPES:
            wins = [synth.make_window(orc, prm, seed=s, n=n, L=L) for s in sc.SEEDS]
            want = {}
            for cap in (sc.SOLVE_CAP, 50):
                orc.set_max_iterations(cap)
                want[cap] = []
                for w in wins:
                    wo = pyoracle.Window(w)
                    orc.set_prior(None)
                    orc.init_solve(wo)
                    want[cap].append((orc.summary(), orc.iterations(), wo["states"].reshape(n, 15).copy()))
            out[n] = (wins, want)
    finally:
        orc.set_max_iterations(50)
        orc.set_prior(None)
    return out


def test_single_window_init_solves_to_their_natural_end(liw, env, solve_windows, monkeypatch):
    """liw.Solver.init_solve on seeds 1 - 3 (n = 6, L = 24) without a cap of its own: iteration count and termination equal to the
    oracle's, the states after EVERY iteration within 1e-6 relative (the oracle moves <= 4.1e-8 here under a 1e-13 perturbation)."""
    prm, orc = env
    clear_switches(monkeypatch)
    n = 6
    wins, want = solve_windows[n]
    worst = 0.0
    for k, w in enumerate(wins):
        so, its, xo = want[50][k]
        slv = liw.Solver(prm)
        wg = liw.Window(w)
        slv.set_window(wg)
        sg = slv.init_solve()
        hg = slv.history()
        slv.close()
        assert (sg["iterations"], sg["termination"]) == (so["iterations"], so["termination"]), (k, sg, so)
        assert len(hg) == len(its)
        worst = max(worst, _check_history(hg, its, n, "seed %d" % sc.SEEDS[k]))
        assert rel_inf(np.asarray(wg["states"]).reshape(n, 15), xo) <= 1e-6
    print("single-window init solves (n = 6, natural end): worst state error over all iterations %.2e" % worst)


@pytest.mark.parametrize("n", [6, 12])
@pytest.mark.parametrize("B", [8, 1024])
def test_batched_init_solves_and_the_marginalisation_behind_them(liw, pyoracle, env, solve_windows, monkeypatch, n, B):
    """BatchSolver.solve(LIW_MODE_INIT, 8) on the three seeds tiled to B = 8 (the one-wave step kernels) and to B = 1 024 (the large-batch
    record format: k_lm_step_quad, the packed IMU rows): iteration counts, terminations and the states after every iteration (1e-6)
    against the oracle (which moves <= 3e-13 here under a 1e-13 perturbation).  Then marginalize(): Delta_H, Delta_g and the new
    prior's J^T J / J^T R against the oracle at the same linearisation point, at the bars of
    test_bench_launch_shape_marginalisation_chain_and_eigq_against_the_oracle (1e-12, 1e-11 and 1e-10 of the round-off scale of the
    gradient sums, 1e-11)."""
    prm, orc = env
    bench = bench_module()
    clear_switches(monkeypatch)
    cap = sc.SOLVE_CAP
    wins, want = solve_windows[n]
    bs = batch_of(liw, prm, wins, B, history_records=cap + 2)
    bs.solve(liw.LIW_MODE_INIT, cap)
    if B >= 1024:
        assert bs.launch_paths()["large_batch_format"]
    got, summ, hist = bs.states(), bs.summaries(), bs.history()
    mpg = bs.t["match_pose"].cpu().numpy().reshape(B, n, 12)
    sH, dH, dg = bs.marginalize()
    dH, dg = dH.cpu().numpy().reshape(B, 15, 15), dg.cpu().numpy().reshape(B, 15)
    pJ, pR, pX = (bs.t[k].cpu().numpy().reshape(B, *sh) for k, sh in (("prior_J", (15, 15)), ("prior_R", (15,)), ("prior_X", (15,))))
    has = bs.t["has_prior"].cpu().numpy()
    assert np.array_equal(bs.states(), got)                          # marginalisation moves no state
    bs.close()
    ws, wm = 0.0, dict(dH=0.0, dg=0.0, JJ=0.0, JR=0.0)
    for b in picks_of(B, 3):
        k = b % 3
        so, its, xo = want[cap][k]
        assert (summ[b]["iterations"], summ[b]["termination"]) == (so["iterations"], so["termination"]), (b, summ[b], so)
        ws = max(ws, _check_history(hist[:, b], its, n, "batch window %d" % b))
        assert rel_inf(got[b], xo) <= 1e-6, b
        o = bench.marg_reference(pyoracle, orc, wins[k], got[b], mpg[b], 1)[0]
        assert has[b] == 1 and np.array_equal(pX[b], got[b, n - 1]) and np.array_equal(pX[b], o["X"])
        sc_ = np.abs(o["dH"]).max()
        e = dict(dH=np.abs(dH[b] - o["dH"]).max() / sc_, dg=np.abs(dg[b] - o["dg"]).max() / o["g_scale"],
                 JJ=np.abs(pJ[b].T @ pJ[b] - o["J"].T @ o["J"]).max() / sc_, JR=np.abs(pJ[b].T @ pR[b] - o["J"].T @ o["R"]).max() / o["g_scale"])
        wm = {key: max(wm[key], float(e[key])) for key in wm}
    orc.set_prior(None)
    print("batched init solves n=%d B=%d, cap %d: worst state error over all iterations %.2e; marginalisation: Delta_H %.2e Delta_g %.2e "
          "(of its round-off scale) prior J^T J %.2e J^T R %.2e" % (n, B, cap, ws, wm["dH"], wm["dg"], wm["JJ"], wm["JR"]))
    assert wm["dH"] <= 1e-12 and wm["dg"] <= 1e-11 and wm["JJ"] <= 1e-11 and wm["JR"] <= 1e-10, wm


def test_tracking_sequence_with_a_carried_prior(liw, synth, monkeypatch):
    """Four tracking frames (and the frame before them that leaves the first prior) of 1 024 robots, n = 2, as test_gpu_track_batch.py
    drives them (bench.TrackBatch: solve + marginalize per frame, the prior carried on the device), at the second set: every frame of
    the sampled robots within 1e-6 of the oracle fed the same states, laser_match poses and prior; equal iteration counts and
    terminations; the marginalisation at the bars of that test."""
    bench = bench_module()
    clear_switches(monkeypatch)
    prm = sc.skewed_params(synth)
    B, K, nb = 1024, 4, 8
    tb = bench.TrackBatch(liw, synth, prm, B, K, nb, "cuda:0", seed0=61240, blocks=(12, 17))
    ids = [0, 1, 2, 63, 64, B - 65, B - 1, nb + 3]
    _, its, cap = tb.run(capture_ids=ids)
    assert tb.bs.launch_paths()["large_batch_format"]
    assert all(int(r["has_out"].min()) == 1 for r in cap)
    assert int(cap[0]["has_in"].max()) == 0 and all(int(r["has_in"].min()) == 1 for r in cap[1:])
    par = tb.teacher_forced_parity(ids, cap)
    tb.bs.close()
    print("tracking sequence at the second configuration, teacher-forced:", par)
    assert par["frames"] == K * len(ids)
    assert par["within_1e_6"] == par["frames"] and par["iterations_equal"] == par["frames"] and par["terminations_equal"] == par["frames"], par
    assert par["worst_rel_state"] <= 1e-6, par
    assert par["worst_rel_Delta_H"] <= 1e-11 and par["worst_Delta_g_of_roundoff_scale"] <= 1e-10, par
    assert par["worst_rel_prior_JtJ"] <= 1e-10 and par["worst_prior_JtR_of_roundoff_scale"] <= 1e-9, par


# ------------------------------------------------------------------------------------------------ 4. pre-integration
@pytest.fixture(scope="module")
def intervals(synth, env):
    """the intervals of test_gpu_preint.py generated at the second set (M = 29) + the nine spin intervals, with the oracle's and the
    numpy restatement's results: built once"""
    prm, orc = env
    _, mgs = sc.golden_modules()
    imu, wheel = sc.preint_intervals(synth, orc, prm)
    return (imu, wheel, [orc.imu_preint(*iv) for iv in imu], [mgs.imu_preint_numpy(prm, *iv) for iv in imu],
            [orc.wheel_preint(*iv) for iv in wheel])


def test_batch_imu_preint_at_anisotropic_noise(liw, env, intervals):
    """One BatchPreint.imu launch over 38 intervals (the first 29 are those of test_gpu_preint.py: the last wave of k_preint_imu is
    partly filled; then nine 400-sample turns of 2.2 - 6.5 rad, where Rz is far from I) against the oracle's sequential accumulator
    AND the numpy restatement: X, J, Dt 1e-12, sqrt_inverse_P 1e-8, U upper triangular exactly, U^T U P = I to 1e-6.
    Reversing any sigma vector, or Rz^T for Rz in dt^2 Rz diag(q_na) Rz^T, moves sqrt_inverse_P by 2e-2 ... 5e-1 on these intervals
    (test_second_config.py); the two references agree to 1.4e-11."""
    prm, orc = env
    imu, _, ref_o, ref_n, _ = intervals
    assert len(imu) == 38
    bp = liw.BatchPreint(prm)
    X, J, S, Dt = [t.cpu().numpy() for t in bp.imu(imu)]
    P = bp.last_P.cpu().numpy()
    bp.close()
    for name, refs in (("oracle", ref_o), ("numpy restatement", ref_n)):
        worst = dict(X=0.0, J=0.0, S=0.0, Dt=0.0, UUP=0.0)
        for m, (Xo, Jo, So, Dto) in enumerate(refs):
            e = dict(X=relerr(X[m], Xo), J=relerr(J[m], Jo), S=relerr(S[m], So), Dt=abs(Dt[m] - Dto) / max(1.0, abs(Dto)),
                     UUP=float(np.abs(S[m].T @ S[m] @ P[m] - np.eye(15)).max()))
            worst = {k: max(worst[k], e[k]) for k in e}
            assert np.abs(np.tril(S[m], -1)).max() == 0.0, m
        print("batched IMU pre-integration at anisotropic noise vs %s: %s" % (name, " ".join("%s %.1e" % kv for kv in worst.items())))
        assert worst["X"] <= 1e-12 and worst["J"] <= 1e-12 and worst["Dt"] <= 1e-12 and worst["S"] <= 1e-8 and worst["UUP"] <= 1e-6, (name, worst)


def test_batch_wheel_preint_with_three_distinct_sigmas(liw, env, intervals):
    """One BatchPreint.wheel launch over the 24 recorded and nine turning intervals: delta_Tij 1e-12 (absolute), Dt 1e-12,
    sqrt_inverse_P 1e-10 against the oracle.  The first turning interval (0.6 m, 2.2 rad: both above the floors of
    wheel_odom_preintegration.h:140-146) has three different diagonal entries, the first two in the ratio of the sigmas."""
    prm, orc = env
    _, wheel, _, _, ref = intervals
    bp = liw.BatchPreint(prm)
    T, S, Dt = [t.cpu().numpy() for t in bp.wheel(wheel)]
    bp.close()
    worst = dict(T=0.0, S=0.0, Dt=0.0)
    for m, (To, So, Dto) in enumerate(ref):
        e = dict(T=float(np.abs(T[m] - np.asarray(To)).max()), S=relerr(S[m], So), Dt=abs(Dt[m] - Dto) / max(1.0, abs(Dto)))
        worst = {k: max(worst[k], e[k]) for k in e}
    k, s = sc.wheel_interval_with_three_weights(wheel), prm["wheel_sigma"]
    ratio = abs(S[k][0, 0] / S[k][1, 1] / (s[1] / s[0]) - 1.0)
    print("batched wheel pre-integration with three sigmas: %s; sigma ratio of interval %d off by %.1e" % (" ".join("%s %.1e" % kv for kv in worst.items()), k, ratio))
    assert worst["T"] <= 1e-12 and worst["Dt"] <= 1e-12 and worst["S"] <= 1e-10, worst
    assert len({float(v) for v in np.diag(S[k])}) == 3 and np.count_nonzero(S[k] - np.diag(np.diag(S[k]))) == 0
    assert ratio <= 1e-12


def test_device_preintegration_at_the_second_configuration_feeds_the_solver(liw, synth, pyoracle, env, monkeypatch):
    """A window (n = 8, L = 200, as test_batch_preint_feeds_the_solver) whose IMU / wheel blocks come from the device pre-integration
    at the second set solves to the states of the window built with the oracle's accumulators, and of the oracle's own solve, within
    1e-6 relative, in the same number of iterations."""
    prm, orc = env
    clear_switches(monkeypatch)
    rec = sc.Recorder(orc)
    n = 8
    w = synth.make_window(rec, prm, seed=31, n=n, L=200)
    bp = liw.BatchPreint(prm)
    X, J, S, Dt = [t.cpu().numpy() for t in bp.imu(rec.imu)]
    T, Sw, Dtw = [t.cpu().numpy() for t in bp.wheel(rec.wheel)]
    bp.close()
    assert relerr(X, w["imu_X"]) <= 1e-12 and np.abs(T - w["wheel_T"]).max() <= 1e-12
    w2 = dict(w)
    w2.update(imu_X=X, imu_J=J.reshape(-1, 225), imu_sqrtP=S.reshape(-1, 225), imu_Dt=Dt, wheel_T=T, wheel_sqrtP=Sw.reshape(-1, 9), wheel_Dt=Dtw)
    out = []
    for ww in (w, w2):
        bs = liw.BatchSolver(prm, [ww])
        bs.solve(liw.LIW_MODE_INIT, 50)
        out.append((bs.states()[0].copy(), bs.summaries()[0]))
        bs.close()
    wo = pyoracle.Window(w)
    orc.set_prior(None)
    orc.init_solve(wo)
    e = float(np.abs(out[0][0] - out[1][0]).max() / max(1.0, np.abs(out[0][0]).max()))
    eo = rel_inf(out[1][0], wo["states"].reshape(n, 15))
    print("window from device pre-integration: solved states vs oracle-fed window %.2e, vs the oracle's solve %.2e" % (e, eo))
    assert out[0][1]["iterations"] == out[1][1]["iterations"] == orc.summary()["iterations"]
    assert e <= 1e-6 and eo <= 1e-6


# ------------------------------------------------------------------------------------------------ 5. pose graph
@pytest.fixture(scope="module")
def graph(liw, env):
    prm, _ = env
    pg = dict(liw.posegraph.office_pg_params(), **sc.PG)
    G = liw.posegraph.make_pose_graph(prm, N=40, seed=4, n_loop=6)
    return pg, (G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"])


def test_posegraph_normal_equations_at_the_second_configuration(liw, pyoracle, env, graph, monkeypatch):
    """k_posegraph.hip reads the wheel extrinsic and both ground weights from the context's DevParams: linearize on
    make_pose_graph(N = 40, n_loop = 6) with anisotropic loop sigmas, against pyoracle.posegraph_linearize at the bars of
    test_posegraph_normal_equations_match_oracle (cost 1e-12, g and H 1e-10 of their maxima)."""
    prm, orc = env
    pg, args = graph
    clear_switches(monkeypatch)
    pgs = liw.posegraph.PoseGraph(prm)
    Hg, gg, cg = pgs.linearize(pg, *args)
    Ho, go, co, idx = pyoracle.posegraph_linearize(orc, pg, *args)
    ec, eg, eH = abs(cg - co) / co, np.abs(gg[idx] - go).max() / np.abs(go).max(), np.abs(Hg[np.ix_(idx, idx)] - Ho).max() / np.abs(Ho).max()
    print("pose graph at the second configuration: cost %.2e g %.2e H %.2e" % (ec, eg, eH))
    assert np.isfinite(Hg).all() and np.isfinite(gg).all()
    assert ec <= 1e-12 and eg <= 1e-10 and eH <= 1e-10
    const = np.setdiff1d(np.arange(240), idx)
    assert len(const) == 6 and np.array_equal(Hg[np.ix_(const, const)], np.eye(6)) and not gg[const].any()


@pytest.mark.parametrize("dense", [False, True])
def test_posegraph_solve_at_the_second_configuration(liw, pyoracle, env, graph, monkeypatch, dense):
    """solve(max_iters = 5) on the same graph against pyoracle.posegraph_solve: equal iteration counts, terminations and successful
    steps, poses within 1e-6; through the chain-segment path and through the dense factorisation (LIW_PG_DENSE=1)."""
    prm, orc = env
    pg, args = graph
    clear_switches(monkeypatch)
    if dense:
        monkeypatch.setenv("LIW_PG_DENSE", "1")
    pgs = liw.posegraph.PoseGraph(prm)
    xg, sg = pgs.solve(pg, *args, max_iters=5)
    xo, so = pyoracle.posegraph_solve(orc, pg, *args, max_iters=5)
    e = float(np.abs(xg - xo).max() / max(1.0, np.abs(xo).max()))
    print("pose-graph solve at the second configuration (dense=%s), 5 iterations: poses %.2e" % (dense, e))
    assert (sg["iterations"], sg["termination"], sg["successful"]) == (so["iterations"], so["termination"], so["successful"]), (sg, so)
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-9 * so["initial_cost"]
    assert e <= 1e-6
