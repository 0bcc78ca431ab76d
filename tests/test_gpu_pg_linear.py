"""The pose graph's linear solves against an extended-precision solve (tests/pg_linear_cases.py): the blocked Cholesky of
csrc/k_posegraph.hip through PoseGraph.dense_spd_solve, one LM step of the single-robot solver on its dense and its sparse path through
PoseGraph.step (chain-segment elimination, reduced system, back-substitution), and the fleet solver's first step (the 256-thread Cholesky of
csrc/k_pg_chol_body.inc) through FleetBackEnd.solve(max_iters=1).

Bars: 16 x the error of the float64 restatement chol64 of the same system against the long-double reference, at least 64 u — forward
max|x - x_ref| / max|x_ref| and residual max|A x - b| / (||A||_inf max|x| + max|b|), the residual formed in long double.  Every figure is
printed ("PGLIN ...") before it is asserted."""
import numpy as np
import pytest

import pg_linear_cases as pc
import second_config as sc
from test_gpu_posegraph_batch import _separators, _truth_loop, _with_loops

pytestmark = pytest.mark.gpu

_CACHE = {}
INIT_RADIUS, MAX_RADIUS = 1e4, 1e16                       # kInitRadius, kMaxRadius of csrc/liw_lm_rules.hpp
RADII_SWEEP = (1e-20, 1e-3, 1e4, 1e10, 1e16)
MIN_DIAG, MAX_DIAG = 1e-6, 1e32                           # kMinDiag, kMaxDiag


@pytest.fixture(scope="module")
def pgs(liw, synth):
    return liw.posegraph.PoseGraph(synth.office_params())


def _report(tag, fwd, fbar, res, rbar):
    print("PGLIN %s forward %.3e bar %.3e residual %.3e bar %.3e" % (tag, fwd, fbar, res, rbar))


# ------------------------------------------------------------------------------------------------------------ 3. dense solver
@pytest.mark.parametrize("fam,n", pc.dense_cases())
def test_dense_solver_under_the_bars(pgs, fam, n):
    A = pc.family(fam, n)
    names, B = pc.rhs_set(A)
    bar = pc.bars(A, B)
    worst = [0.0, 0.0, 0.0, 0.0]
    fails = []
    for j, name in enumerate(names):
        b = np.ascontiguousarray(B[:, j])
        x = pgs.dense_spd_solve(A, b)
        assert np.array_equal(x, pgs.dense_spd_solve(A, b)), (fam, n, name, "two calls differ")
        f, r = float(pc.forward_error(x, bar["x_ref"][:, j])), float(pc.scaled_residual(A, x, b))
        _report("dense %s n=%d %s" % (fam, n, name), f, bar["forward"][j], r, bar["residual"][j])
        if f / bar["forward"][j] > worst[0] / max(worst[1], 1e-300):
            worst[0], worst[1] = f, float(bar["forward"][j])
        if r / bar["residual"][j] > worst[2] / max(worst[3], 1e-300):
            worst[2], worst[3] = r, float(bar["residual"][j])
        if not (f <= bar["forward"][j] and r <= bar["residual"][j]):
            fails.append((name, f, float(bar["forward"][j]), r, float(bar["residual"][j])))
    _report("dense-worst %s n=%d" % (fam, n), *worst)
    assert not fails, (fam, n, fails)


def _good_system():
    A = pc.wellcond(130, 3)                               # three blocks, 62 padding rows
    b = np.random.default_rng(130).normal(size=130)
    return A, b


def _fails_then_recovers(liw, pgs, bad, b, good, tag):
    A, bg, xg = good
    raised = False
    try:
        x = pgs.dense_spd_solve(bad, b)
    except liw.LiwError:
        raised = True
    assert raised, (tag, "LIW_OK for a matrix without a Cholesky factor", "x finite: %s" % bool(np.isfinite(x).all()))
    assert np.array_equal(pgs.dense_spd_solve(A, bg), xg), (tag, "a good system after a failed one returns other bits")


@pytest.mark.parametrize("n", [128, 130, 192])
def test_dense_indefinite_at_every_pivot_is_reported(liw, pgs, n):
    A, bg = _good_system()
    good = (A, bg, pgs.dense_spd_solve(A, bg))
    b = np.random.default_rng(n).normal(size=n)
    for k in (0, 1, 62, 63, 64, 65, 127, 128, n - 1):
        if k < n:
            _fails_then_recovers(liw, pgs, pc.indefinite(n, k, 0), b, good, (n, k))


def _hostile(n):
    """name -> matrix that has no Cholesky factor, built on the well-conditioned family"""
    out = {}
    base = pc.wellcond(n, 5)
    for k in sorted({0, 63, 64, n - 1}):
        if k < n:
            Z = base.copy()
            Z[k, :] = 0.0
            Z[:, k] = 0.0
            out["zero_pivot_%d" % k] = Z
            D = base.copy()
            D[k, k] = np.nan
            out["nan_diag_%d" % k] = D
    if n > 1:
        for j in sorted({0, n - 2}):
            W = base.copy()
            W[n - 1, j] = W[j, n - 1] = np.nan
            out["nan_last_row_%d" % j] = W
    return out


@pytest.mark.parametrize("n", [64, 65, 130])
def test_dense_zero_pivot_and_nan_are_reported(liw, pgs, n):
    A, bg = _good_system()
    good = (A, bg, pgs.dense_spd_solve(A, bg))
    b = np.random.default_rng(n).normal(size=n)
    for name, bad in _hostile(n).items():
        _fails_then_recovers(liw, pgs, bad, b, good, (name, n))


@pytest.mark.parametrize("n", [64, 65, 128])
def test_dense_infinite_last_pivot_is_reported(liw, pgs, n):
    """+inf passes `pivot > 0`; 1 / sqrt(inf) = 0 and inf * 0 = NaN: until k_potrf64 tested isfinite as the other two Cholesky codes do, this
    came back as LIW_OK with NaN in x (order 64 and 128: the last pivot of the last block; 65: the first pivot of the padded block)."""
    A, bg = _good_system()
    good = (A, bg, pgs.dense_spd_solve(A, bg))
    bad = pc.wellcond(n, 5)
    bad[n - 1, n - 1] = np.inf
    _fails_then_recovers(liw, pgs, bad, np.random.default_rng(n).normal(size=n), good, n)


@pytest.mark.parametrize("n", [64, 65, 130])
def test_dense_contract_error_or_finite(liw, pgs, n):
    """whatever the matrix holds: an error is raised, or every entry of x is finite"""
    cases = dict(_hostile(n))
    base = pc.wellcond(n, 5)
    for name, (r, c, v) in dict(inf_diag_first=(0, 0, np.inf), inf_diag_last=(n - 1, n - 1, np.inf), minus_inf_diag=(n // 2, n // 2, -np.inf),
                                inf_diag_mid=(n // 2, n // 2, np.inf), inf_offdiag=(n - 1, 0, np.inf), minus_inf_offdiag=(n - 1, n // 2, -np.inf),
                                huge_offdiag=(n - 1, 0, 1e300)).items():
        M = base.copy()
        M[r, c] = M[c, r] = v
        cases[name] = M
    for k in (0, n - 1):
        cases["indefinite_%d" % k] = pc.indefinite(n, k, 1)
    cases["good"] = base
    b = np.random.default_rng(n).normal(size=n)
    for name, M in cases.items():
        try:
            x = pgs.dense_spd_solve(M, b)
        except liw.LiwError:
            assert name != "good"
            continue
        assert np.isfinite(x).all(), (name, n, "LIW_OK with a value in x that is not finite")


# ------------------------------------------------------------------------------------------------------------ 4. step probe
def _graphs(liw, synth):
    """name -> graph: the smallest that reach each branch of the sparse path"""
    if "graphs" in _CACHE:
        return _CACHE["graphs"]
    prm = synth.office_params()
    mp = liw.posegraph.make_pose_graph
    rng = np.random.default_rng(77)
    tl = lambda G, pairs: _with_loops(G, [_truth_loop(synth, G, j, i, rng) for j, i in pairs])
    out = {}
    out["n4"] = mp(prm, N=4, seed=13, n_loop=0)                                  # one segment, two interior frames
    out["n5_loop31"] = tl(mp(prm, N=5, seed=15, n_loop=0), [(3, 1)])             # segments with 0, 1 and 0 interior frames
    out["n49"] = mp(prm, N=49, seed=14, n_loop=0)                                # interior length 47, the longest
    out["n50"] = mp(prm, N=50, seed=16, n_loop=0)                                # separators 48 and 49 are neighbours
    G97 = mp(prm, N=97, seed=17, n_loop=0)
    ten = [(60, 10), (70, 20), (80, 30), (90, 20)]                                # 0, 48, 96 and seven loop frames
    out["n97_sep10"] = tl(G97, ten)                                               # 60 unknowns: one block
    out["n97_sep11"] = tl(G97, ten + [(85, 30)])                                  # 66 unknowns: two blocks, 62 padding rows
    out["n140_sep24"] = tl(mp(prm, N=140, seed=18, n_loop=0), [(75 + 6 * k, 5 + 6 * k) for k in range(10)])   # 144 unknowns: three blocks
    out["loop_on_0"] = tl(mp(prm, N=40, seed=5, n_loop=0), [(39, 0)])
    G = mp(prm, N=50, seed=9, n_loop=4)                                           # five loops on one pair, three one way and two the other
    e0 = next(k for k in range(len(G["loop_idx"])) if 0 not in G["loop_idx"][k])
    a, b = int(G["loop_idx"][e0, 0]), int(G["loop_idx"][e0, 1])
    extra = []
    for k in range(4):
        tf = G["loop_tf12"][e0].copy()
        tf[9:12] += rng.normal(0.0, 0.01, 3)
        if k % 2 == 0:
            extra.append(((a, b), tf))
        else:
            R = tf[:9].reshape(3, 3)
            extra.append(((b, a), np.concatenate([R.T.reshape(9), -R.T @ tf[9:12]])))
    out["dup_pair"] = _with_loops(G, extra)
    G = mp(prm, N=30, seed=7, n_loop=3)                                           # one key frame with |q| > pi
    G["poses"] = G["poses"].copy()
    G["poses"][7, 3:6] *= 3.2 / np.linalg.norm(G["poses"][7, 3:6])
    out["big_q"] = G
    assert _separators(out["n97_sep10"]) == 10 and _separators(out["n97_sep11"]) == 11 and _separators(out["n140_sep24"]) == 24
    assert all(int(G["seq_idx"][0, 0]) == 0 for G in out.values())               # key frame 0 is the constant one
    _CACHE["graphs"] = out
    return out


GRAPHS = ("n4", "n5_loop31", "n49", "n50", "n97_sep10", "n97_sep11", "n140_sep24", "loop_on_0", "dup_pair", "big_q")
SWEEP_GRAPHS = ("n5_loop31", "n97_sep10")


def _config(liw, synth, name):
    """(PoseGraph, pg dict)"""
    if ("cfg", name) not in _CACHE:
        office = liw.posegraph.office_pg_params()
        prm = sc.skewed_params(synth) if name == "anisotropic" else synth.office_params()
        pg = {"office": office, "no_ground": dict(office, use_ground_p_factor=False, use_ground_q_factor=False),
              "anisotropic": dict(office, **sc.PG), "loop_k_1e3": dict(office, loop_edge_k=1e3)}[name]
        _CACHE["cfg", name] = (liw.posegraph.PoseGraph(prm), pg)
    return _CACHE["cfg", name]


def _args(G):
    nl = len(G["loop_idx"])
    return (G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"] if nl else None, G["loop_tf12"] if nl else None)


def _linearised(liw, synth, cfg, gname):
    """dict(H, g, scale, dgn, free): float64 bits of PoseGraph.linearize taken as exact, scale and dgn as pg_run forms them"""
    key = ("lin", cfg, gname)
    if key not in _CACHE:
        pgs, pg = _config(liw, synth, cfg)
        G = _graphs(liw, synth)[gname]
        H, g, _ = pgs.linearize(pg, *_args(G))
        d = np.diag(H).copy()
        scale = 1.0 / (1.0 + np.sqrt(d))
        dgn = np.clip(d * scale * scale, MIN_DIAG, MAX_DIAG)
        scale[:6], dgn[:6] = 1.0, 0.0                                             # the constant key frame
        _CACHE[key] = dict(H=H, g=g, scale=scale, dgn=dgn, free=np.arange(6, len(g)))
    return _CACHE[key]


def _system(lin, radius, scale=None, dgn=None):
    """(A, rhs) of the free unknowns: A = S H S + diag(dgn / radius), rhs = S g"""
    scale, dgn = lin["scale"] if scale is None else scale, lin["dgn"] if dgn is None else dgn
    fr = lin["free"]
    s = scale[fr]
    A = lin["H"][np.ix_(fr, fr)] * s[:, None] * s[None, :]
    A = pc.sym_from_lower(A)
    A[np.diag_indices_from(A)] += dgn[fr] / radius
    return A, lin["g"][fr] * s


def _reference(liw, synth, cfg, gname, radius):
    key = ("ref", cfg, gname, radius)
    if key not in _CACHE:
        lin = _linearised(liw, synth, cfg, gname)
        A, rhs = _system(lin, radius)
        bar = pc.bars(A, rhs)
        ok, ratio = pc.reference_is_good(A, rhs, bar)
        e_norm, e_comp = pc.ref_error_bounds(A, bar["x_ref"], rhs)
        print("PGLIN ref %s %s r=%g reference error / forward bar: %.3e (norm bound alone %.3e, componentwise alone %.3e)" %
              (cfg, gname, radius, ratio, float(e_norm[0] / bar["forward"]), float(e_comp[0] / bar["forward"])))
        assert ok, ("the reference is not 64 times better than the forward bar", cfg, gname, radius, ratio)
        _CACHE[key] = (A, rhs, bar)
    return _CACHE[key]


def _check_step(liw, synth, cfg, gname, radius):
    pgs, pg = _config(liw, synth, cfg)
    G = _graphs(liw, synth)[gname]
    lin = _linearised(liw, synth, cfg, gname)
    A, rhs, bar = _reference(liw, synth, cfg, gname, radius)
    fr, ymax = lin["free"], float(np.abs(bar["x_ref"]).max())
    ys, fails = [], []
    for path in (0, 1):
        y, scale, dgn, solved = pgs.step(pg, *_args(G), radius=radius, path=path)
        y2, scale2, dgn2, solved2 = pgs.step(pg, *_args(G), radius=radius, path=path)
        assert solved == 1 and solved2 == 1, (cfg, gname, radius, path)
        assert np.array_equal(y, y2) and np.array_equal(scale, scale2) and np.array_equal(dgn, dgn2), "a second call returns other bits"
        same = (np.array_equal(scale, lin["scale"]), np.array_equal(dgn, lin["dgn"]))
        print("PGLIN step-bits %s %s r=%g path=%d scale_equal=%s dgn_equal=%s" % (cfg, gname, radius, path, *same))
        assert all(same), (cfg, gname, radius, path, "scale / dgn differ from 1 / (1 + sqrt(diag H)) and its clipped diagonal", same)
        assert not y[:6].any()
        f, r = float(pc.forward_error(y[fr], bar["x_ref"])), float(pc.scaled_residual(A, y[fr], rhs))
        _report("step %s %s r=%g %s" % (cfg, gname, radius, ("dense", "sparse")[path]), f, bar["forward"], r, bar["residual"])
        if not (f <= bar["forward"] and r <= bar["residual"]):
            fails.append((path, f, float(bar["forward"]), r, float(bar["residual"])))
        ys.append(y)
    apart = float(np.abs(ys[0] - ys[1]).max()) / ymax
    print("PGLIN step-paths %s %s r=%g apart %.3e bar %.3e" % (cfg, gname, radius, apart, 2.0 * bar["forward"]))
    assert not fails, (cfg, gname, radius, fails)
    assert apart <= 2.0 * bar["forward"], (cfg, gname, radius, apart)


@pytest.mark.parametrize("radius", [INIT_RADIUS, MAX_RADIUS])
@pytest.mark.parametrize("gname", GRAPHS)
def test_step_matches_extended_precision_on_both_paths(liw, synth, gname, radius):
    _check_step(liw, synth, "office", gname, radius)


@pytest.mark.parametrize("radius", [INIT_RADIUS, MAX_RADIUS])
@pytest.mark.parametrize("gname", GRAPHS)
@pytest.mark.parametrize("cfg", ["no_ground", "anisotropic", "loop_k_1e3"])
def test_step_at_other_configurations(liw, synth, cfg, gname, radius):
    """both ground factors off (the least constrained directions, the worst conditioning), the anisotropic set of second_config.py,
    loop_edge_k = 1e3"""
    _check_step(liw, synth, cfg, gname, radius)


@pytest.mark.parametrize("radius", [r for r in RADII_SWEEP if r not in (INIT_RADIUS, MAX_RADIUS)])
@pytest.mark.parametrize("gname", SWEEP_GRAPHS)
def test_step_over_the_radius_range(liw, synth, gname, radius):
    """with the two radii of the tests above: 1e-20 (the damping is the matrix), 1e-3, 1e4, 1e10, 1e16 (the damping is gone)"""
    _check_step(liw, synth, "office", gname, radius)


def test_step_with_a_nan_pose_is_unsolved_not_an_error(liw, synth):
    pgs, pg = _config(liw, synth, "office")
    G = _graphs(liw, synth)["n97_sep11"]
    before = [pgs.step(pg, *_args(G), radius=INIT_RADIUS, path=p) for p in (0, 1)]
    bad = G["poses"].copy()
    bad[20, 1] = np.nan                                                           # an interior frame of a segment
    for p in (0, 1):
        _, _, _, solved = pgs.step(pg, bad, *_args(G)[1:], radius=INIT_RADIUS, path=p)   # returns LIW_OK: no LiwError
        assert solved == 0, p
        y, scale, dgn, solved = pgs.step(pg, *_args(G), radius=INIT_RADIUS, path=p)
        assert solved == 1 and np.array_equal(y, before[p][0]) and np.array_equal(scale, before[p][1]) and np.array_equal(dgn, before[p][2])


def test_step_sparse_path_is_refused_where_solve_would_not_take_it(liw, synth):
    pgs, pg = _config(liw, synth, "office")
    G = liw.posegraph.make_pose_graph(synth.office_params(), N=3, seed=12, n_loop=0)      # fewer than four key frames: dense only
    y, _, _, solved = pgs.step(pg, *_args(G), path=0)
    assert solved == 1 and np.isfinite(y).all()
    with pytest.raises(liw.LiwError) as e:
        pgs.step(pg, *_args(G), path=1)
    assert e.value.code == liw.LIW_EINVAL


# ------------------------------------------------------------------------------------------------------------ 5. fleet step
# every graph of section 4 fits max_keyframes = 140; the condition on the graphs of this test is that LM accepts the first step (asserted,
# here and for PoseGraph.solve).  big_q does not meet it: the key frame turned to |q| = 3.2 rad leaves a cost of 4.7e6 that the first
# step does not lower, so its poses after one iteration are x0 and say nothing about the solve; the step probe covers it.
FLEET_GRAPHS = ("n4", "n5_loop31", "n49", "n50", "n97_sep10", "n97_sep11", "n140_sep24", "loop_on_0", "dup_pair")


def _plus(x, d):
    """Plus of plus6 (csrc/k_posegraph_lm_dev.hpp): positions add; rotation vectors add, then wrap into (-pi, pi]"""
    out = x + d
    for f in range(len(out)):
        q = out[f, 3:6]
        a = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        if a > np.pi:
            out[f, 3:6] = (q / a) * (a - 2.0 * np.pi * np.floor((a + np.pi) / (2.0 * np.pi)))
    return out


def _fleet_first_steps(liw, synth, lds_doubles):
    """name -> poses after solve(max_iters = 1), four graphs a call in robots 0, 1, 3, 4 of five; robot 2 holds a graph and is not selected"""
    import torch
    graphs = _graphs(liw, synth)
    fb = liw.FleetBackEnd(synth.office_params(), liw.posegraph.office_pg_params(), dict(B=5, max_keyframes=140, max_loops=24))
    if lds_doubles is not None:
        fb.set_lds_doubles(lds_doubles)
    slots = (0, 1, 3, 4)
    out = {}
    names = list(FLEET_GRAPHS)
    for r0 in range(0, len(names), 4):
        batch = names[r0:r0 + 4]
        spare = graphs[names[(r0 + 5) % len(names)]]
        for b, name in zip(slots, batch):
            fb.load_graph(b, graphs[name])
        fb.load_graph(2, spare)
        sel = np.zeros(5, dtype=np.uint8)
        sel[list(slots[:len(batch)])] = 1
        fb.solve(torch.as_tensor(sel), torch.full((5,), 100.0, dtype=torch.float64), max_iters=1)
        sm = fb.summaries()
        for b, name in zip(slots, batch):
            assert sm[b]["successful"] == 1, (name, sm[b])
            out[name] = fb.keyframes(b)["poses"].copy()
        assert np.array_equal(fb.keyframes(2)["poses"], spare["poses"]), "the robot that was not selected moved"
    return out


def test_fleet_first_step_matches_extended_precision(liw, synth):
    pgs, pg = _config(liw, synth, "office")
    graphs = _graphs(liw, synth)
    got = _fleet_first_steps(liw, synth, None)
    work = _fleet_first_steps(liw, synth, 0)
    fails = []
    for name in FLEET_GRAPHS:
        G = graphs[name]
        # (n140_sep24: 24 separators, a triangle of 10 440 doubles, over the 8 192 that liw_fpg_set_lds_doubles allows at the most, so it
        # runs from the work area both times and this line compares nothing for it; every other graph's triangle fits the LDS by default)
        assert np.array_equal(got[name], work[name]), (name, "the LDS and the work-area triangle give other bits")
        _, s1 = pgs.solve(pg, *_args(G), max_iters=1)
        assert s1["successful"] == 1, (name, s1)                                  # the condition on the graphs of this test
        lin = _linearised(liw, synth, "office", name)
        A, rhs, bar = _reference(liw, synth, "office", name, INIT_RADIUS)
        y = np.zeros(len(lin["g"]), dtype=pc.LD)
        y[lin["free"]] = bar["x_ref"]
        want = _plus(G["poses"].astype(pc.LD), (-(lin["scale"].astype(pc.LD) * y)).reshape(-1, 6))
        ymax = float(np.abs(bar["x_ref"]).max())
        smax = float(lin["scale"][lin["free"]].max())                            # over the unknowns that move (the constant key frame has 1)
        tol = float(smax * bar["forward"] * ymax + 4 * pc.U * np.abs(G["poses"]).max())
        err = float(np.abs(got[name].astype(pc.LD) - want).max())
        print("PGLIN fleet %s pose error %.3e bar %.3e (as a forward error of y: %.3e bar %.3e)" %
              (name, err, tol, err / (smax * ymax), bar["forward"]))
        assert np.array_equal(got[name][0], G["poses"][0])
        if not err <= tol:
            fails.append((name, err, tol))
    assert not fails, fails
