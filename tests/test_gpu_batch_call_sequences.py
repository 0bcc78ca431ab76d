"""What the batched context (liw_ctx behind liw_batch_* / BatchSolver) decides BETWEEN calls: the cached captured graph (gexec / gkey) and
its replay, the early exit of liw_batch_solve's loop, the packed laser rows of the last solve (lpk_on / lpk_key) that the marginalisation
behind it reuses, last_iters.  The kernels themselves are pinned to the oracle elsewhere; here one context lives through several calls.

  (a) the captured graph on the large-batch paths (active list, forked role streams, per-frame IMU records, k_lm_step_quad), first launch
      and replay, against the plain launch sequence: bit for bit, and the common result against the oracle;
  (b) the early exit against the fixed-length loop (LIW_NO_EARLY_EXIT, read per call): bit for bit;
  (c) the re-capture rule (K, mode, array pointers);
  (d) packed rows never outlive the arrays they were packed from (a replayed graph used to leave them armed);
  (e) a differential fuzz of the batched state machine against a fresh context per operation.

Bars (all carried by the same quantities elsewhere in the suite): solved states <= 1e-6 of |x|max with equal iteration counts and
terminations (tests/test_gpu_laser_slab.py); marginalisation Delta_H 1e-11 of |Delta_H|max, Delta_g 1e-10 of its round-off scale
(bench.marg_reference's g_scale), the new prior's J^T J 1e-10 of |Delta_H|max (test_one_pose_slab_kernel_marg_records_and_tracking_solves).
Everything else is exact equality: the launch forms compared run the same kernels on the same inputs."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUMMARY = np.dtype([("iterations", "<i4"), ("successful", "<i4"), ("termination", "<i4"), ("pad", "<i4"), ("initial_cost", "<f8"), ("final_cost", "<f8")])
PRIOR_KEYS = ("prior_X", "prior_J", "prior_R", "has_prior")


@pytest.fixture(scope="module")
def env(liw, synth, pyoracle):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    prm = synth.office_params()

    class Env:
        pass
    e = Env()
    e.liw, e.synth, e.pyoracle, e.prm, e.orc = liw, synth, pyoracle, prm, pyoracle.Oracle(prm)
    e.bench = importlib.import_module("bench")
    e.shapes, e.runs = {}, {}
    return e


# ------------------------------------------------------------------------------------------------ batches
def _tile(base, B, track, seed):
    """window b = base[b % nb]; the copies behind the first nb carry 2 mm of position jitter (INIT: every frame, TRACK: the new frame's
    initial guess) and laser_match poses that follow their states, as synth.make_window lays them out"""
    nb, n = len(base), int(base[0]["n"])
    idx = np.arange(B) % nb
    st = np.stack([np.asarray(w["states"], dtype=np.float64).reshape(n, 15) for w in base])[idx].copy()
    mp = np.stack([np.asarray(w["match_pose"], dtype=np.float64).reshape(n, 12) for w in base])[idx].copy()
    rng = np.random.default_rng(seed)
    if track:
        st[nb:, n - 1, 0:3] += rng.normal(0.0, 2e-3, (B - nb, 3))
    else:
        st[nb:, :, 0:3] += rng.normal(0.0, 2e-3, (B - nb, n, 3))
        mp[nb:, :, 0:6] = st[nb:, 0:1, 0:6]
    mp[nb:, :, 6:12] = st[nb:, :, 0:6]
    return dict(B=B, states=st, match_pose=mp)


def _moved(base, sign=1.0):
    """the same windows with every block's l2 end points (columns 6:12 of laser_pts) moved rigidly in the scan plane by 3 cm and 0.5 degrees:
    same counts, same owning frames, z stays 0"""
    out = []
    for k, w in enumerate(base):
        th = sign * np.deg2rad(0.5) * (1.0 if k % 2 == 0 else -1.0)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        t = sign * 0.03 * np.array([np.cos(0.7 + k), np.sin(0.7 + k)])
        p = np.array(w["laser_pts"], dtype=np.float64, copy=True).reshape(-1, 12)
        for c in (6, 9):
            p[:, c:c + 2] = p[:, c:c + 2] @ R.T + t
        d = dict(w)
        d["laser_pts"] = p
        out.append(d)
    return out


SHAPES = {   # name: (topology, B, n, K)
    "init600": ("init", 600, 7, 50),        # active list, one-wave step kernels, forked roles; every window ends by iteration ~32
    "init1101": ("init", 1101, 7, 25),      # per-frame IMU records, k_lm_step_quad, a tail wave of one window; a quarter of the windows runs into the cap
    "track1101": ("track", 1101, 2, 50),    # the tracking topology on a carried prior
    "track16400": ("track", 16400, 2, 30),  # 257 slabs: k_lin_laser_slab1, multi-window IMU chain, quad kernel (the early exit's production shape)
    "init4421": ("init", 4421, 30, 3),      # 70 slabs x 30 frames = 2 100 waves: the lane-per-group kernel of INIT solves
}


def _shape(env, name):
    if name in env.shapes:
        return env.shapes[name]
    topo, B, n, K = SHAPES[name]
    synth, orc, prm = env.synth, env.orc, env.prm
    if name == "init4421":      # the windows of tests/test_gpu_laser_slab.py::_batch (L <= 200, ragged groups)
        base = [synth.make_window(orc, prm, seed=7100 + k, n=n, L=int(L)) for k, L in enumerate((29 * 3, 29 * 5 + 11, 40, 29 * 4 + 3, 200, 64))]
        # ragged groups: window 2 has frames without any block; window 4's blocks all sit on the last seven frames (on the first seven the
        # marginalisation onto the newest frame would hardly see them: 1e-11 of |Delta_H|max for the move of _moved)
        base[4]["laser_frame"] = np.sort(np.asarray(base[4]["laser_frame"]) % 7 + 23).astype(np.int32)
    elif topo == "init":
        # (windows whose init solve converges within 18 .. 32 iterations: most 7-frame windows of this recipe crawl into a cap of 50)
        base = [synth.make_window(orc, prm, seed=seed, n=n, L=L) for seed, L in ((9103, 90), (9110, 84), (9111, 143), (9106, 120))]
    else:                       # two-frame tracking windows as in test_one_pose_slab_kernel_marg_records_and_tracking_solves
        base = [env.bench.sub_window(synth.make_window(orc, prm, seed=8100 + k, n=3, frame_counts=[0, 40 + 13 * k, 55 + 7 * k]), 1) for k in range(4)]
    S = dict(name=name, topo=topo, mode=(env.liw.LIW_MODE_INIT if topo == "init" else env.liw.LIW_MODE_TRACK), B=B, n=n, K=K, base=base,
             tile=_tile(base, B, topo == "track", seed=11 + B), prior=None)
    env.shapes[name] = S
    return S


def _window(S, b, base=None):
    d = dict((base or S["base"])[b % len(S["base"])])
    d["states"], d["match_pose"] = S["tile"]["states"][b].copy(), S["tile"]["match_pose"][b].copy()
    return d


def _sample(S):
    return list(range(len(S["base"]))) + [S["B"] - 1]


def _solver(env, S, hist=0, base=None, tile=None):
    import torch
    bs = env.liw.BatchSolver(env.prm, base or S["base"], tile=tile or S["tile"], history_records=hist)
    if S["topo"] == "track":
        # a carried prior: the marginalisation of the window pair as it stands, sat on the older frame where a tracking solve expects it
        # (computed once per shape; every solver of the shape gets the same bytes)
        if S["prior"] is None:
            bs.marginalize()
            bs.t["prior_X"].view(S["B"], 15).copy_(bs.t["x"].view(S["B"], S["n"], 15)[:, S["n"] - 2])
            torch.cuda.synchronize()
            S["prior"] = {k: bs.t[k].cpu().numpy().copy() for k in PRIOR_KEYS}
            bs.ws.zero_()
        for k in PRIOR_KEYS:
            bs.t[k].copy_(torch.from_numpy(S["prior"][k]).to(bs.dev))
    return bs


def _reset(bs, tile):
    """the caller's side of a new solve on the same arrays: initial states and laser_match poses back, a workspace like new"""
    import torch
    bs.set_states(tile["states"])
    bs.t["match_pose"].copy_(torch.from_numpy(np.ascontiguousarray(tile["match_pose"].reshape(-1))).to(bs.dev))
    bs.ws.zero_()


def _summaries(bs):
    o = int(bs.lay.info_off)
    return bs.ws[o:o + SUMMARY.itemsize * bs.B].cpu().numpy().view(SUMMARY).copy()


def _grab(bs):
    import torch
    torch.cuda.synchronize()
    h = bs.history()
    return dict(x=bs.states().copy(), mp=bs.t["match_pose"].cpu().numpy().reshape(bs.B, bs.n, 12).copy(), sm=_summaries(bs),
                hist=None if h is None else h.copy(), flags=bs.launch_paths()["flags"])


def _assert_same(a, b, what):
    for k in ("x", "mp", "hist"):
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int((a[k] != b[k]).sum()))
    for f in ("iterations", "successful", "termination", "initial_cost", "final_cost"):
        assert np.array_equal(a["sm"][f], b["sm"][f], equal_nan=(a["sm"][f].dtype.kind == "f")), (what, f)
    assert a["flags"] == b["flags"], (what, a["flags"], b["flags"])


def _run(env, monkeypatch, name, form, K=None, hist=True):
    """One solve of shape `name` on a fresh solver, memoised: "plain", "noexit" (LIW_NO_EARLY_EXIT), "graph" (-> first launch and replay)"""
    S = _shape(env, name)
    K = S["K"] if K is None else K
    key = (name, form, K)
    if key in env.runs:
        return env.runs[key]
    if form == "noexit":
        monkeypatch.setenv("LIW_NO_EARLY_EXIT", "1")
    else:
        monkeypatch.delenv("LIW_NO_EARLY_EXIT", raising=False)
    bs = _solver(env, S, hist=(K + 1) if hist else 0)
    bs.solve(S["mode"], K, use_graph=(form == "graph"))
    out = _grab(bs)
    if form == "graph":
        _reset(bs, S["tile"])
        bs.solve(S["mode"], K, use_graph=True)          # cache hit: hipGraphLaunch of the graph instantiated above
        out = (out, _grab(bs))
    bs.close()
    monkeypatch.delenv("LIW_NO_EARLY_EXIT", raising=False)
    env.runs[key] = out
    return out


def _pin_to_oracle(env, S, res, K):
    """states <= 1e-6 of |x|max, equal iteration counts and terminations, on every distinct window and the last one -> worst state error"""
    orc, po = env.orc, env.pyoracle
    orc.set_max_iterations(K)
    worst = 0.0
    for b in _sample(S):
        w = po.Window(_window(S, b))
        if S["topo"] == "track":
            P = S["prior"]
            orc.set_prior((P["prior_X"].reshape(-1, 15)[b], P["prior_J"].reshape(-1, 15, 15)[b], P["prior_R"].reshape(-1, 15)[b]))
            orc.solve(w)
        else:
            orc.set_prior(None)
            orc.init_solve(w)
        so, sg = orc.summary(), res["sm"][b]
        assert (int(sg["iterations"]), int(sg["termination"])) == (so["iterations"], so["termination"]), (S["name"], b, sg, so)
        err = np.abs(res["x"][b] - w["states"].reshape(S["n"], 15)).max() / np.abs(w["states"]).max()
        assert err <= 1e-6, (S["name"], b, err)
        worst = max(worst, float(err))
    orc.set_prior(None)
    orc.set_max_iterations(50)
    return worst


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name,flags", [("init600", 0), ("init1101", 1), ("track1101", 1)])
def test_captured_graph_and_its_replay_equal_the_plain_launches_on_the_large_batch_paths(env, monkeypatch, name, flags):
    """The three shapes lie below the arming thresholds of the lane-per-group laser kernel, so the captured sequence and the plain one run
    the same kernels: states, laser_match poses, history records and summaries (cost fields included) agree bit for bit — first launch of
    the captured graph (three parallel role branches per linearisation) and the replay of the cached one.  The common result is pinned to the
    oracle on every distinct window and on the last window of the batch (states 1e-6 of |x|max, iteration counts, terminations)."""
    S = _shape(env, name)
    plain = _run(env, monkeypatch, name, "plain")
    first, replay = _run(env, monkeypatch, name, "graph")
    assert plain["flags"] == flags and first["flags"] == flags and replay["flags"] == flags
    _assert_same(plain, first, "graph, first launch")
    _assert_same(first, replay, "graph, replay")
    assert not np.array_equal(plain["x"], S["tile"]["states"])
    worst = _pin_to_oracle(env, S, plain, S["K"])
    print("%s: worst state error against the oracle %.2e, iterations %d .. %d" % (name, worst, plain["sm"]["iterations"].min(), plain["sm"]["iterations"].max()))


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name,breaks", [("init600", True), ("init1101", False), ("track1101", True)])
def test_early_exit_equals_the_fixed_length_loop(env, monkeypatch, name, breaks):
    """liw_batch_solve stops launching once no window iterates (read-backs after iteration 3, then every 2 .. 8): bit-identical to the
    fixed-length loop (LIW_NO_EARLY_EXIT=1, read per call) and to the captured graph, which runs every iteration too.  breaks: every
    window ends at least 8 iterations before the cap (the loop does break); otherwise windows run into the cap (it must not)."""
    S = _shape(env, name)
    early, fixed = _run(env, monkeypatch, name, "plain"), _run(env, monkeypatch, name, "noexit")
    it, term = early["sm"]["iterations"], early["sm"]["termination"]
    if breaks:
        assert it.max() <= S["K"] - 8, it.max()
    else:
        assert ((it == S["K"]) & (term == 4)).any(), (it.max(), np.unique(term))
    _assert_same(early, fixed, "early exit vs fixed length")
    _assert_same(early, _run(env, monkeypatch, name, "graph")[0], "early exit vs graph")


@pytest.mark.parametrize("K", [1, 3, 4])
def test_early_exit_at_the_first_read_back(env, monkeypatch, K):
    """the first read-back sits behind iteration 3 and only when another iteration follows: caps of 1 and 3 never read back, 4 does"""
    early, fixed = _run(env, monkeypatch, "init600", "plain", K=K), _run(env, monkeypatch, "init600", "noexit", K=K)
    assert early["sm"]["iterations"].max() == K
    _assert_same(early, fixed, "K = %d" % K)


def test_early_exit_on_the_production_tracking_shape(env, monkeypatch):
    """16 400 two-frame windows on a carried prior (257 slabs: k_lin_laser_slab1 over packed rows, the multi-window IMU chain, the quad step
    kernel — flags 3): early exit against the fixed-length loop bit for bit, the result against the oracle (states 1e-6 of |x|max,
    iteration counts, terminations) on the distinct windows and on the last one."""
    name = "track16400"
    S = _shape(env, name)
    early, fixed = _run(env, monkeypatch, name, "plain"), _run(env, monkeypatch, name, "noexit")
    assert early["flags"] == 3 and fixed["flags"] == 3
    assert early["sm"]["iterations"].max() <= S["K"] - 8, early["sm"]["iterations"].max()
    _assert_same(early, fixed, "early exit vs fixed length")
    worst = _pin_to_oracle(env, S, early, S["K"])
    print("%s: worst state error against the oracle %.2e, iterations %d .. %d" % (name, worst, early["sm"]["iterations"].min(), early["sm"]["iterations"].max()))


# ------------------------------------------------------------------------------------------------ (c)
def test_the_cached_graph_is_captured_again_when_K_mode_or_arrays_change(env, monkeypatch):
    """One solver, graph solves only: K = 5, K = 9, TRACK, other arrays of the same B and n (rebind), the first arrays again, and once more
    (a cache hit).  Every result equals the plain solve of that call on a fresh solver, bit for bit."""
    import torch
    liw = env.liw
    S = _shape(env, "init600")
    tile_b = _tile(S["base"], S["B"], False, seed=977)
    live = _solver(env, S)
    other = env.liw.BatchSolver(env.prm, _moved(S["base"]), tile=tile_b)      # the second set of arrays (its own points, states, poses)
    other.close()                                                             # (only its tensors are used)
    arrays_a = dict(live.t)
    steps = [("K = 5", liw.LIW_MODE_INIT, 5, "a"), ("K = 9", liw.LIW_MODE_INIT, 9, "a"), ("TRACK", liw.LIW_MODE_TRACK, 9, "a"),
             ("rebind", liw.LIW_MODE_TRACK, 9, "b"), ("rebind back", liw.LIW_MODE_TRACK, 9, "a"), ("cache hit", liw.LIW_MODE_TRACK, 9, "a")]
    bound = "a"
    for what, mode, K, arr in steps:
        if arr != bound:
            live.rebind(other.t if arr == "b" else arrays_a, live.Ltot)
            bound = arr
        tile = S["tile"] if arr == "a" else tile_b
        _reset(live, tile)
        live.solve(mode, K, use_graph=True)
        got = _grab(live)
        fresh = env.liw.BatchSolver(env.prm, S["base"] if arr == "a" else _moved(S["base"]), tile=tile)
        fresh.solve(mode, K)
        ref = _grab(fresh)
        fresh.close()
        assert not np.array_equal(ref["x"], tile["states"]), what
        _assert_same(got, ref, what)
    torch.cuda.synchronize()
    live.close()


# ------------------------------------------------------------------------------------------------ (d)
def _marg_out(bs):
    import torch
    x = bs.states().copy()
    mp = bs.t["match_pose"].cpu().numpy().reshape(bs.B, bs.n, 12).copy()
    sH, dH, dg = bs.marginalize()
    torch.cuda.synchronize()
    return dict(x=x, mp=mp, dH=dH.cpu().numpy().reshape(bs.B, 15, 15), dg=dg.cpu().numpy().reshape(bs.B, 15),
                pX=bs.t["prior_X"].cpu().numpy().reshape(bs.B, 15).copy(), pJ=bs.t["prior_J"].cpu().numpy().reshape(bs.B, 15, 15).copy(),
                has=bs.t["has_prior"].cpu().numpy().copy())


def _check_marg(env, S, base, out, stale_base=None):
    """Delta_H 1e-11 of |Delta_H|max, Delta_g 1e-10 of g_scale, the new prior (J^T J 1e-10 of |Delta_H|max, linearised X, has_prior) against
    bench.marg_reference at the GPU's own states with the points of `base`.  stale_base: the points the marginalisation must NOT have used —
    the oracle's Delta_H for them lies at least 1e-6 of |Delta_H|max away on every compared window (1e5 bars: stale rows cannot pass), and
    the distance of the GPU result from that stale reference is returned for the record."""
    worst = dict(dH=0.0, dg=0.0, JJ=0.0, stale=0.0)
    for b in _sample(S):
        ref = env.bench.marg_reference(env.pyoracle, env.orc, _window(S, b, base), out["x"][b], out["mp"][b], 1)[0]
        sc = np.abs(ref["dH"]).max()
        if stale_base is not None:
            old = env.bench.marg_reference(env.pyoracle, env.orc, _window(S, b, stale_base), out["x"][b], out["mp"][b], 1)[0]
            assert np.abs(old["dH"] - ref["dH"]).max() >= 1e-6 * sc, b
            worst["stale"] = max(worst["stale"], float(np.abs(out["dH"][b] - ref["dH"]).max() / sc))
        e = dict(dH=np.abs(out["dH"][b] - ref["dH"]).max() / sc, dg=np.abs(out["dg"][b] - ref["dg"]).max() / ref["g_scale"],
                 JJ=np.abs(out["pJ"][b].T @ out["pJ"][b] - ref["J"].T @ ref["J"]).max() / sc)
        assert e["dH"] <= 1e-11, (b, e)
        assert e["dg"] <= 1e-10, (b, e)
        assert e["JJ"] <= 1e-10, (b, e)
        assert np.array_equal(out["pX"][b], ref["X"]) and np.array_equal(out["pX"][b], out["x"][b][S["n"] - 1]) and out["has"][b] == 1, b
        for k in ("dH", "dg", "JJ"):
            worst[k] = max(worst[k], float(e[k]))
    env.orc.set_prior(None)
    return worst


@pytest.mark.parametrize("seq", ["solve_marg", "graph_plain_rewrite_graph_marg", "plain_rewrite_plain_marg", "rebind_solve_rebind_back_marg"])
def test_packed_rows_never_outlive_the_arrays_they_were_packed_from(env, monkeypatch, seq):
    """INIT, 4 421 windows x 30 frames (2 100 (slab, frame) waves: the lane-per-group kernel arms, flags 3), then marginalize() on the same
    solver against bench.marg_reference at the GPU's own states — Delta_H 1e-11 of |Delta_H|max, Delta_g 1e-10 of g_scale, prior J^T J 1e-10 of
    |Delta_H|max (the bars of the slab marginalisation test), on the distinct windows and the last one.
      solve_marg: rows reused (bit 1 still set at the marginalisation);
      graph_plain_rewrite_graph_marg: graph solve, plain solve (arms the rows), laser_pts rewritten in place, graph solve again — a REPLAY,
        which runs no host code of the solve: the rows of the old points must be gone, the reference uses the new points;
      plain_rewrite_plain_marg: the second plain solve packs the new points;
      rebind_solve_rebind_back_marg: rows keyed to other arrays: the marginalisation of the first arrays reads those arrays.
    The rewrite keeps laser_off / laser_frame and every z = 0 and moves the l2 end points by 3 cm / 0.5 degrees: with stale rows the result
    is a wrong number (never an access outside the rows), at least 1e-6 of |Delta_H|max off — asserted from the two oracle results."""
    import torch
    monkeypatch.delenv("LIW_NO_LASER_SLAB", raising=False)
    monkeypatch.delenv("LIW_NO_EARLY_EXIT", raising=False)
    S = _shape(env, "init4421")
    M, K = S["mode"], S["K"]
    if "moved" not in S:
        S["moved"] = _moved(S["base"])
        S["tile_b"] = _tile(S["base"], S["B"], False, seed=4242)
    bs = _solver(env, S)
    other = env.liw.BatchSolver(env.prm, S["moved"], tile=S["tile_b"])
    other.close()                                   # (only its tensors are used: the moved points, the second set of arrays)
    stale = None
    if seq == "solve_marg":
        bs.solve(M, K)
        assert bs.launch_paths()["flags"] == 3
        out, base = _marg_out(bs), S["base"]
        lp = bs.launch_paths()
        assert lp["flags"] == 3 and lp["packed_rows"] > 0, lp
    elif seq == "graph_plain_rewrite_graph_marg":
        bs.solve(M, K, use_graph=True)
        assert bs.launch_paths()["flags"] == 1
        _reset(bs, S["tile"])
        bs.solve(M, K)
        assert bs.launch_paths()["flags"] == 3
        bs.t["laser_pts"].copy_(other.t["laser_pts"])
        _reset(bs, S["tile"])
        bs.solve(M, K, use_graph=True)
        lp = bs.launch_paths()
        assert not lp["lane_per_group_laser"] and lp["flags"] == 1 and lp["packed_rows"] == 0, lp
        out, base, stale = _marg_out(bs), S["moved"], S["base"]
        assert bs.launch_paths()["flags"] == 1
    elif seq == "plain_rewrite_plain_marg":
        bs.solve(M, K)
        assert bs.launch_paths()["flags"] == 3
        bs.t["laser_pts"].copy_(other.t["laser_pts"])
        _reset(bs, S["tile"])
        bs.solve(M, K)
        lp = bs.launch_paths()
        assert lp["flags"] == 3 and lp["packed_rows"] > 0, lp
        out, base, stale = _marg_out(bs), S["moved"], S["base"]
        assert bs.launch_paths()["flags"] == 3
    else:
        arrays_a = dict(bs.t)
        bs.solve(M, K)
        assert bs.launch_paths()["flags"] == 3
        bs.rebind(other.t, other.Ltot)
        bs.solve(M, K)
        assert bs.launch_paths()["flags"] == 3
        bs.rebind(arrays_a, bs.Ltot)
        lp = bs.launch_paths()
        assert not lp["lane_per_group_laser"] and lp["flags"] == 1 and lp["packed_rows"] == 0, lp
        out, base, stale = _marg_out(bs), S["base"], S["moved"]
        assert bs.launch_paths()["flags"] == 1
    assert not np.array_equal(out["x"], S["tile"]["states"])
    worst = _check_marg(env, S, base, out, stale)
    print("%s: worst Delta_H %.2e of |Delta_H|max, Delta_g %.2e of g_scale, prior J^T J %.2e of |Delta_H|max" % (seq, worst["dH"], worst["dg"], worst["JJ"]))
    torch.cuda.synchronize()
    bs.close()


# ------------------------------------------------------------------------------------------------ (e)
def _call(fn):
    try:
        return ("ok", fn())
    except Exception as e:   # noqa: BLE001  (LiwError codes are compared)
        return ("err", getattr(e, "code", repr(e)))


def _state(bs, summaries):
    out = {k: bs.t[k].cpu().numpy().copy() for k in ("x", "match_pose") + PRIOR_KEYS}
    if summaries:
        sm = _summaries(bs)
        for f in ("iterations", "successful", "termination", "initial_cost", "final_cost"):
            out["summary." + f] = sm[f].copy()
    return out


@pytest.mark.parametrize("seed", list(range(6)))
def test_random_batched_call_sequences_against_a_fresh_context_per_operation(env, monkeypatch, seed):
    """40 random operations on ONE long-lived BatchSolver — plain / graph solves (INIT, TRACK, caps 1 / 3 / 6 / 50), marginalize, the LM loop
    driven by hand (lm_begin / lm_linearize / lm_step / lm_finish), set_states, laser_pts rewritten in place (same counts), rebind to other
    arrays and back, has_prior cleared, timing on / off.  Shapes below the arming thresholds of the lane-per-group kernel (600 / 1 101
    windows of 2 / 4 frames), so every legal sequence is bit-comparable: after each computing operation the states, laser_match poses,
    summaries, prior X / J / R, has_prior and sqrt_H / Delta_H / Delta_g equal those of a FRESH solver that is handed the arrays and the
    prior as they stood and performs that operation alone; an error occurs on both sides or on neither."""
    import torch
    liw, synth, prm = env.liw, env.synth, env.prm
    monkeypatch.delenv("LIW_NO_EARLY_EXIT", raising=False)
    rng = np.random.default_rng(5200 + seed)
    B, n = [(600, 2), (1101, 4), (1101, 2), (600, 4), (1101, 4), (600, 2)][seed]
    base = [synth.make_window(env.orc, prm, seed=600 + 10 * seed + k, n=n, L=int(rng.integers(20, 120))) for k in range(4)]
    tiles = [_tile(base, B, False, seed=31 * seed + k) for k in range(2)]
    variants = [base, _moved(base), _moved(base, -1.0)]
    live = liw.BatchSolver(prm, base, tile=tiles[0])
    donors = [liw.BatchSolver(prm, v, tile=tiles[1]) for v in variants + [variants[1]]]
    for d in donors:
        d.close()                                         # (only their tensors are used)
    pts = [d.t["laser_pts"] for d in donors[:3]]          # three sets of end points; the fourth donor's tensors are the other arrays
    arrays = [dict(live.t), dict(donors[3].t)]
    bound, timing = 0, False
    keys = live.INPUT_KEYS + PRIOR_KEYS
    INIT, TRACK = liw.LIW_MODE_INIT, liw.LIW_MODE_TRACK

    def hand_loop(bs, mode, K):
        K = bs.lm_begin(mode, K)
        bs.lm_linearize(mode, 0)
        for _ in range(K):
            bs.lm_step(mode)
            bs.lm_linearize(mode, 1)
        bs.lm_step(mode)
        bs.lm_finish(mode)

    def marg(bs):
        return [t.cpu().numpy() for t in bs.marginalize()]

    ops = ["solve", "solve", "solve", "graph", "graph", "graph", "marg", "marg", "hand", "set_states", "rewrite", "rebind", "clear_prior", "timing"]
    log, moved = [], 0
    for step in range(40):
        op = ops[int(rng.integers(0, len(ops)))]
        mode, K = (INIT if rng.integers(0, 2) else TRACK), int(rng.choice([1, 3, 6, 50]))
        log.append((op, mode, K))
        if op == "set_states":
            st = tiles[bound]["states"].copy()
            st[:, :, 0:3] += rng.normal(0.0, 1e-3, st[:, :, 0:3].shape)
            live.set_states(st)
            continue
        if op == "rewrite":
            live.t["laser_pts"].copy_(pts[int(rng.integers(0, len(pts)))])
            continue
        if op == "rebind":
            bound = 1 - bound
            live.rebind(arrays[bound], live.Ltot)
            continue
        if op == "clear_prior":
            live.t["has_prior"].zero_()
            continue
        if op == "timing":
            if timing:
                live.get_timing()
            timing = not timing
            live.set_timing(timing)
            continue
        fresh = liw.BatchSolver(prm, base, tile=tiles[0])
        for k in keys:
            fresh.t[k].copy_(live.t[k])
        if op == "solve":
            f = lambda bs: bs.solve(mode, K)
        elif op == "graph":
            f = lambda bs: bs.solve(mode, K, use_graph=True)
        elif op == "hand":
            f = lambda bs: hand_loop(bs, mode, K)
        else:
            f = marg
        x0 = live.t["x"].clone()
        ra, rb = _call(lambda: f(live)), _call(lambda: f(fresh))
        torch.cuda.synchronize()
        assert ra[0] == rb[0], (step, ra, rb, log[-8:])
        if op == "marg" and ra[0] == "ok":
            for name, a, b in zip(("sqrt_H", "Delta_H", "Delta_g"), ra[1], rb[1]):
                assert np.array_equal(a, b, equal_nan=True), (step, name, log[-8:])
        elif ra[0] == "err":
            assert ra[1] == rb[1], (step, ra, rb, log[-8:])
        sa, sb = _state(live, op != "marg"), _state(fresh, op != "marg")
        for k in sa:
            assert np.array_equal(sa[k], sb[k], equal_nan=(sa[k].dtype.kind == "f")), (step, k, log[-8:])
        moved += int(ra[0] == "ok" and op != "marg" and not torch.equal(x0, live.t["x"]))
        if timing:
            live.get_timing()
        fresh.close()
    assert moved >= 5, (moved, log)                       # (the sequence did solve: 40 draws hold ~ 20 solves)
    live.close()
