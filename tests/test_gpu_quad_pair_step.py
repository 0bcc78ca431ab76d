"""k_lm_step_quad_pair (two waves per quad of windows: assembler + eliminator, csrc/k_lm_quad.hip) against k_lm_step_quad (one wave,
LIW_QUAD_PAIR=0): the pair kernel performs the one-wave kernel's operations in their order, so everything a solve leaves behind is
required to be BITWISE equal — states, summaries (iterations, successful steps, termination, costs), the whole workspace (LM states with
their Jacobi scales and LM diagonals, factor records, candidates) and, for INIT, the marginalisation that follows (sqrt_H, Delta_H,
Delta_g).  The one-wave kernel is the reference.  The two kernels are instantiations of one body (csrc/k_lm_quad.hip, lm_step_quad_body): they
share the prologue, the Jacobi scaling, the elimination and the second sweep, so this test pins what differs — the split of a frame between
two waves, the hand-off tile, the register gather table, the batched reads — and independence from the shared code rests on the oracle
parity tests of the suite, which run on whichever kernel is the default and, in test_gpu_compact_laser_records / _large_rotation, on both.

Shapes: B = 1 027 (just over the 1 023-window threshold of the quad kernels; the last wave has three live rows); INIT with n = 3, 7, 30
at about eight laser blocks per frame, one frame without any; TRACK with n = 2 on a carried prior that every other window lacks (mixed
inside every wave).  The iteration cap lets windows finish at different iterations, so the compacted list regroups rows between
launches; some windows start far from their minimum (rejected steps: the `reuse` path); one window has a rotation vector with
|theta|^2 > 9.6 (k_lm_step<true> steps it inside the same batch); one carries a NaN state (FAILURE in the prologue on both paths); in the
TRACK case one window's prior block is scaled so that its cost stays finite (about 1e306) while its gradient overflows: that window passes
the prologue and fails on the gradient checksum behind the first sweep, which the assembler wave hands to the eliminator."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUMMARY = np.dtype([("iterations", "<i4"), ("successful", "<i4"), ("termination", "<i4"), ("pad", "<i4"), ("initial_cost", "<f8"), ("final_cost", "<f8")])
PRIOR_KEYS = ("prior_X", "prior_J", "prior_R", "has_prior")
B = 1027
I_SLOW, I_NAN, I_OVF, FAR = 5, 9, 20, (12, 13, 14, 15, 700, 1026)   # windows: large rotation, NaN state, overflowing prior gradient (TRACK), far starts
# name: (topology, n, iteration cap, windows finish at different iterations).  n = 30 runs into a small cap (a few seconds per case): the
# regrouping of rows between launches is the business of the other three
CASES = {"init3": ("init", 3, 20, True), "init7": ("init", 7, 50, True), "init30": ("init", 30, 12, False), "track2": ("track", 2, 30, True)}


@pytest.fixture(scope="module")
def env(liw, synth, pyoracle):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    prm = synth.office_params()
    return dict(liw=liw, synth=synth, prm=prm, orc=pyoracle.Oracle(prm), bench=importlib.import_module("bench"), runs={})


def _batch(env, name):
    topo, n, K, _ = CASES[name]
    synth, orc, prm = env["synth"], env["orc"], env["prm"]
    if topo == "init":
        if n == 7:   # windows whose init solve converges within 18 .. 32 iterations (tests/test_gpu_batch_call_sequences.py), 12 .. 20 blocks per frame
            base = [synth.make_window(orc, prm, seed=seed, n=n, L=L) for seed, L in ((9103, 90), (9110, 84), (9111, 143), (9106, 120))]
        else:
            base = [synth.make_window(orc, prm, seed=9300 + 10 * n + k, n=n, L=8 * n + 3 * k) for k in range(4)]
        keep = np.asarray(base[2]["laser_frame"]) != 1                      # window 2: frame 1 holds no block
        assert 0 < keep.sum() < keep.size
        base[2] = dict(base[2], laser_frame=np.asarray(base[2]["laser_frame"])[keep], laser_pts=np.asarray(base[2]["laser_pts"])[keep])
    else:
        base = [env["bench"].sub_window(synth.make_window(orc, prm, seed=8100 + k, n=3, frame_counts=[0, 8 + k, 9 + k]), 1) for k in range(4)]
    nb = len(base)
    idx = np.arange(B) % nb
    st = np.stack([np.asarray(w["states"], dtype=np.float64).reshape(n, 15) for w in base])[idx].copy()
    mp = np.stack([np.asarray(w["match_pose"], dtype=np.float64).reshape(n, 12) for w in base])[idx].copy()
    rng = np.random.default_rng(77 + n)
    f = n - 1                                                               # the frame that is free in both topologies
    st[nb:, f, 0:3] += rng.normal(0.0, 2e-3, (B - nb, 3))
    for b in FAR:                                                           # far starts: steps get rejected on the way back
        st[b, f, 0:2] += rng.normal(0.0, 0.4, 2)
        st[b, f, 5] += 0.35
        st[b, f, 6:9] += rng.normal(0.0, 1.0, 3)
    st[I_SLOW, f, 3:6] = np.array([0.0, 0.0, 3.12])                         # |theta|^2 = 9.73 > 9.6, inside the |theta| <= pi ball
    st[I_NAN, f, 1] = np.nan
    mp[nb:, :, 6:12] = st[nb:, :, 0:6]
    mp[I_NAN] = mp[I_NAN % nb]
    return dict(topo=topo, n=n, K=K, base=base, tile=dict(B=B, states=st, match_pose=mp), prior=None)


def _run(env, monkeypatch, name, pair):
    import torch
    key = (name, pair)
    if key in env["runs"]:
        return env["runs"][key]
    liw = env["liw"]
    S = env["runs"].setdefault(name, None) or _batch(env, name)
    env["runs"][name] = S
    if pair:
        monkeypatch.delenv("LIW_QUAD_PAIR", raising=False)
    else:
        monkeypatch.setenv("LIW_QUAD_PAIR", "0")
    bs = liw.BatchSolver(env["prm"], S["base"], tile=S["tile"])
    track = S["topo"] == "track"
    if track:   # a carried prior (the marginalisation of the pair as it stands, on the older frame); every other window goes without
        if S["prior"] is None:
            bs.marginalize()
            bs.t["prior_X"].view(B, 15).copy_(bs.t["x"].view(B, S["n"], 15)[:, S["n"] - 2])
            bs.t["has_prior"][1::2] = 0
            # window I_OVF: J = c everywhere, x - X = delta in one entry -> residuals c delta, cost 7.5 (c delta)^2 = 1e306 (finite),
            # gradient entries 15 c^2 delta = 2 cost / delta = 2e309 (overflow)
            delta = 1e-3
            bs.t["prior_J"].view(B, 225)[I_OVF] = np.sqrt(1e306 / 7.5) / delta
            bs.t["prior_X"].view(B, 15)[I_OVF, 0] -= delta
            torch.cuda.synchronize()
            S["prior"] = {k: bs.t[k].cpu().numpy().copy() for k in PRIOR_KEYS}
            bs.ws.zero_()
        for k in PRIOR_KEYS:
            bs.t[k].copy_(torch.from_numpy(S["prior"][k]).to(bs.dev))
    bs.solve(liw.LIW_MODE_TRACK if track else liw.LIW_MODE_INIT, S["K"])
    torch.cuda.synchronize()
    lp = bs.launch_paths()
    o = int(bs.lay.info_off)
    out = dict(x=bs.states().copy(), sm=bs.ws[o:o + SUMMARY.itemsize * B].cpu().numpy().view(SUMMARY).copy(), ws=bs.ws.cpu().numpy().copy(), lp=lp)
    if not track:
        out["marg"] = [t.cpu().numpy().copy() for t in bs.marginalize()]
        torch.cuda.synchronize()
    bs.close()
    monkeypatch.delenv("LIW_QUAD_PAIR", raising=False)
    env["runs"][key] = out
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_pair_kernel_equals_the_one_wave_kernel_bit_for_bit(env, monkeypatch, name):
    new, old = _run(env, monkeypatch, name, True), _run(env, monkeypatch, name, False)
    assert new["lp"]["large_batch_format"] and new["lp"]["step_kernel"] == "k_lm_step_quad_pair", new["lp"]
    assert old["lp"]["large_batch_format"] and old["lp"]["step_kernel"] == "k_lm_step_quad", old["lp"]
    sm = old["sm"]
    print(name, "iterations", np.bincount(sm["iterations"]), "terminations", np.bincount(sm["termination"]),
          "windows with rejected steps", int((sm["successful"] < sm["iterations"]).sum()))
    # the reference run has the situations this test is about
    assert not CASES[name][3] or len(np.unique(sm["iterations"])) >= 3, "windows must finish at different iterations"
    # (an iteration that is not successful is a rejected or invalid step, or the one a window terminates in: two and more of them on a window
    # the quad kernels step — a far start — is at least one rejected step, the `reuse` path of the LM diagonal)
    far = np.array(FAR)
    print(name, "far starts: iterations", sm["iterations"][far], "successful", sm["successful"][far], "terminations", sm["termination"][far])
    assert (sm["iterations"][far] - sm["successful"][far] >= 2).any(), "no rejected step on a window of the quad kernels"
    if CASES[name][0] == "track":
        print(name, "overflow window: iterations", sm["iterations"][I_OVF], "termination", sm["termination"][I_OVF], "initial cost", sm["initial_cost"][I_OVF])
        assert np.isfinite(sm["initial_cost"][I_OVF]) and sm["initial_cost"][I_OVF] > 1e300, "the overflow window must pass the prologue"
        assert sm["termination"][I_OVF] == 6 and new["sm"]["termination"][I_OVF] == 6, "the overflow window must fail on the gradient checksum"
    assert sm["termination"][I_NAN] == 6 and new["sm"]["termination"][I_NAN] == 6, "the NaN window must end with FAILURE"
    assert sm["iterations"][I_SLOW] >= 1
    for f in SUMMARY.names:
        assert np.array_equal(_bits(new["sm"][f]), _bits(sm[f])), (name, f, int((new["sm"][f] != sm[f]).sum()))
    assert np.array_equal(_bits(new["x"]), _bits(old["x"])), (name, "states", int((_bits(new["x"]) != _bits(old["x"])).sum()))
    assert np.array_equal(_bits(new["ws"]), _bits(old["ws"])), (name, "workspace", int((_bits(new["ws"]) != _bits(old["ws"])).sum()))
    if "marg" in old:
        for what, a, b in zip(("sqrt_H", "Delta_H", "Delta_g"), new["marg"], old["marg"]):
            assert np.array_equal(_bits(a), _bits(b)), (name, what)
