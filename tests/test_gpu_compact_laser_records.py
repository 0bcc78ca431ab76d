"""Compact laser group records of the large-batch format (csrc/liw_kernels.hpp: LPC = 48 doubles per (window, frame), the 45 / 21 pair
totals the 128-slot record is a signed expansion of).  Every writer (k_lin_laser_slab / _slab1, the lane-per-block kernel, the exchange
unpack) and every reader (k_lm_step_quad, the one-wave step kernels, the marginalisation, the dense export, the exchange pack) of the
format against the 128-slot format, the lane-per-block kernel and the oracle:
  * dense H, g, cost of the compact format (LIW_STEP_VARIANT=3) against the 128-slot format (=1) and the oracle, INIT and MARG, with a
    frame without blocks and a window with 3-D end points; the expanded records of both formats slot by slot, structural zeros as +0;
  * the lane-per-group kernels writing compact records (4 400 windows: 68.75 slabs; TRACK at 16 400 two-frame windows) against the
    lane-per-block kernel writing them;
  * the per-iteration LM history of k_lm_step_quad reading compact records against the oracle, with a window the one-wave kernel takes
    over in the same launch pair;
  * the factor-sharded exchange of compact records through two lock-step rank objects."""
import importlib
import os
import sys

import numpy as np
import pytest

from parity_util import TOL_HG, normal_eq_errors

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


@pytest.fixture(scope="module")
def env(liw, synth, pyoracle):
    prm = synth.office_params()
    return prm, pyoracle.Oracle(prm)


# ---- the slot map, restated independently of csrc/liw_kernels.hpp: slot of the 128-slot record -> (pair total, negated) or None
def slot_map(both):
    nc = 9 if both else 6
    rc = nc - 1

    def pair(c1, c2):
        c1, c2 = min(c1, c2), max(c1, c2)
        return c1 * nc - c1 * (c1 - 1) // 2 + (c2 - c1)
    col_a = {0: 0, 1: 1, 3: 2, 4: 3, 5: 4}                                        # pose entry (px py pz th0 th1 th2) -> unique column; pz: none
    col_b = {0: 0, 1: 1, 3: 5, 4: 6, 5: 7} if both else {0: 0, 1: 1, 3: 2, 4: 3, 5: 4}
    neg_b = (lambda i: i < 2) if both else (lambda i: False)                     # b_x = -a_x, b_y = -a_y when both poses are free
    m = [None] * 128
    for r in range(6):
        for c in range(6):
            if both and r in col_a and c in col_a:
                m[r * 6 + c] = (pair(col_a[r], col_a[c]), False)
            if r in col_b and c in col_b:
                m[36 + r * 6 + c] = (pair(col_b[r], col_b[c]), neg_b(r) != neg_b(c))
            if both and r in col_a and c in col_b:
                m[72 + r * 6 + c] = (pair(col_a[r], col_b[c]), neg_b(c))
        if both and r in col_a:
            m[108 + r] = (pair(col_a[r], rc), False)
        if r in col_b:
            m[114 + r] = (pair(col_b[r], rc), neg_b(r))
    m[120] = (pair(rc, rc), False)
    return m


def expand(raw, both):
    """compact records [..., 48] -> 128-slot records, as the readers of the format expand them (sign-bit flip, +0 for structural zeros)"""
    out = np.zeros(raw.shape[:-1] + (128,))
    for s, e in enumerate(slot_map(both)):
        if e is not None:
            out[..., s] = -raw[..., e[0]] if e[1] else raw[..., e[0]]
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def assert_records_close(new, old, what):
    """the bars of tests/test_gpu_laser_slab.py: 6x6 blocks 1e-12 of the block's largest entry, gradients / cost 1e-11 of theirs"""
    B, n = new.shape[:2]
    for name, sl in (("Haa", slice(0, 36)), ("Hbb", slice(36, 72)), ("Hab", slice(72, 108))):
        a, o = new[:, :, sl].reshape(B, n, 6, 6), old[:, :, sl].reshape(B, n, 6, 6)
        scale = np.abs(o).max(axis=(2, 3), keepdims=True) + 1e-300
        e = float((np.abs(a - o) / scale).max())
        print("%s %s: %.2e" % (what, name, e))
        assert e <= 1e-12, (what, name, e)
    for sl in (slice(108, 114), slice(114, 120), slice(120, 121)):
        a, o = new[:, :, sl], old[:, :, sl]
        e = float((np.abs(a - o) / (np.abs(o).max(axis=2, keepdims=True) + 1e-300)).max())
        print("%s slots %d..%d: %.2e" % (what, sl.start, sl.stop - 1, e))
        assert e <= 1e-11, (what, sl, e)
    assert np.all(new[:, :, 121:] == 0.0), what


# ------------------------------------------------------------------------------------------------ 1. dense export
@pytest.fixture(scope="module")
def export_windows(synth, pyoracle, env):
    """B = 7, n = 5: five ordinary windows, one with a frame that holds no blocks, one with 3-D end points; the oracle's normal equations
    of both topologies.  Built once, shared, never modified."""
    prm, orc = env
    n = 5
    wins = [synth.make_window(orc, prm, seed=6400 + k, n=n, L=23 + 19 * k) for k in range(7)]
    keep = wins[3]["laser_frame"] != 2
    assert 0 < keep.sum() < keep.size
    wins[3] = dict(wins[3], laser_frame=wins[3]["laser_frame"][keep], laser_pts=wins[3]["laser_pts"][keep])
    pts = np.array(wins[5]["laser_pts"], dtype=np.float64)
    p43 = pts.reshape(-1, 4, 3)
    assert np.all(p43[:, :, 2] == 0.0)
    p43[3:30, :, 2] = 0.05 * np.random.default_rng(11).normal(size=(27, 4))       # end points off the scan plane
    wins[5] = dict(wins[5], laser_pts=p43.reshape(pts.shape))
    ref = []
    for w in wins:
        orc.set_prior(None)
        Ho, go, co = orc.linearize(pyoracle.Window(w), 0)
        orc.marginalization(pyoracle.Window(w))
        m = orc.marg_pieces()
        ref.append(dict(init=(Ho, go, co), marg=(m["H"], m["g"], 0.5 * float(m["R"] @ m["R"]))))
    return wins, ref


@pytest.mark.parametrize("mode_name", ["init", "marg"])
def test_dense_export_of_compact_records_matches_the_128_slot_format_and_the_oracle(liw, env, export_windows, monkeypatch, mode_name):
    prm, orc = env
    wins, ref = export_windows
    B, n = len(wins), 5
    mode = liw.LIW_MODE_INIT if mode_name == "init" else liw.LIW_MODE_MARG
    both = mode_name == "init"
    out = {}
    for variant in ("1", "3"):
        monkeypatch.setenv("LIW_STEP_VARIANT", variant)
        bs = liw.BatchSolver(prm, wins)
        stride = int(bs.lay.laser_partial_stride)
        assert stride == (48 if variant == "3" else 128) and int(bs.lay.laser_partial_bytes) == 8 * B * n * stride
        bs.linearize(mode)
        H, g, c = [t.cpu().numpy() for t in bs.export_dense(mode)]
        rec = bs.PL[0].cpu().numpy().reshape(B, n, 128).copy()
        raw = bs.PL_raw[0].cpu().numpy().reshape(B, n, stride).copy()
        out[variant] = (H, g, c, rec, raw)
        bs.close()
    H1, g1, c1, rec1, _ = out["1"]
    H3, g3, c3, rec3, raw3 = out["3"]
    # the compact record: pair totals, zeros behind them; its expansion by the library = the expansion restated here, bit for bit
    np_tot = 45 if both else 21
    assert np.all(raw3[:, :, np_tot:] == 0.0) and not np.signbit(raw3[:, :, np_tot:]).any()
    assert np.abs(raw3[:, :, :np_tot]).max() > 0.0
    assert same_bits(rec3, expand(raw3, both))
    # ... against the 128-slot format: every slot, and structural zeros (the z rows / columns, also of the window with 3-D end points;
    # H_aa, H_ab, g_a with one free pose; the padding) are +0 in both
    assert_records_close(rec3, rec1, "compact vs 128-slot records, " + mode_name)
    zero = np.array([e is None for e in slot_map(both)])
    for rec in (rec1, rec3):
        assert np.all(rec[:, :, zero] == 0.0) and not np.signbit(rec[:, :, zero]).any()
    assert np.all(rec3[3, 2] == 0.0) and np.all(raw3[3, 2] == 0.0)                 # the frame without blocks
    assert np.abs(rec3[5]).max() > 0.0
    worst = dict(H=0.0, g=0.0, cost=0.0, fH=0.0, fg=0.0, fc=0.0)
    for b in range(B):
        Ho, go, co = ref[b][mode_name]
        assert np.isfinite(H3[b]).all() and np.isfinite(g3[b]).all()
        eH, eg = normal_eq_errors(H3[b], g3[b], Ho, go, co)
        fH, fg = normal_eq_errors(H3[b], g3[b], H1[b], g1[b], c1[b])
        e = dict(H=eH, g=eg, fH=fH, fg=fg, fc=abs(c3[b] - c1[b]) / max(1.0, abs(c1[b])))
        if both:
            e["cost"] = abs(c3[b] - co) / co
        worst = {k: max(worst[k], e.get(k, 0.0)) for k in worst}
    print("%s: worst scaled errors against the oracle H %.2e g %.2e cost %.2e, against the 128-slot format H %.2e g %.2e cost %.2e"
          % (mode_name, worst["H"], worst["g"], worst["cost"], worst["fH"], worst["fg"], worst["fc"]))
    assert worst["H"] <= TOL_HG and worst["g"] <= TOL_HG and worst["cost"] <= 1e-12, worst
    assert worst["fH"] <= TOL_HG and worst["fg"] <= TOL_HG and worst["fc"] <= 1e-12, worst


# ------------------------------------------------------------------------------------------------ 2. the lane-per-group kernels
def test_slab_kernels_write_compact_records(liw, synth, pyoracle, env, monkeypatch):
    """k_lin_laser_slab (INIT) and k_lin_laser_slab1 (the MARG linearisation behind it, at the same states) at B = 4 400 (68.75 slabs),
    n = 30, ~60 blocks per window, against the lane-per-block kernel (LIW_NO_LASER_SLAB=1) writing the same compact records."""
    prm, orc = env
    monkeypatch.delenv("LIW_STEP_VARIANT", raising=False)
    B, n = 4400, 30
    base = [synth.make_window(orc, prm, seed=6500 + k, n=n, L=int(L)) for k, L in enumerate((58, 29 * 2 + 5, 40, 61, 90, 64))]
    base[4]["laser_frame"] = np.sort(np.asarray(base[4]["laser_frame"]) % 7 + 1).astype(np.int32)      # blocks on a few frames only
    rng = np.random.default_rng(3)
    wins = []
    for b in range(B):
        w = dict(base[b % len(base)])
        if b >= len(base):
            st = np.array(w["states"], copy=True)
            st[:, 0:3] += rng.normal(0.0, 2e-3, (n, 3))
            mp = np.array(w["match_pose"], copy=True)
            mp[:, 0:6] = st[0, 0:6]; mp[:, 6:12] = st[:, 0:6]
            w["states"], w["match_pose"] = st, mp
        wins.append(w)

    def run(no_slab):
        import torch
        if no_slab:
            monkeypatch.setenv("LIW_NO_LASER_SLAB", "1")
        else:
            monkeypatch.delenv("LIW_NO_LASER_SLAB", raising=False)
        bs = liw.BatchSolver(prm, wins)
        assert int(bs.lay.laser_partial_stride) == 48
        bs.lm_begin(liw.LIW_MODE_INIT, 50)
        bs.lm_linearize(liw.LIW_MODE_INIT, 0)
        torch.cuda.synchronize()
        flags = bs.launch_paths()["flags"]
        raw = bs.PL_raw[0].cpu().numpy().reshape(B, n, 48).copy()
        rec = bs.PL[0].cpu().numpy().reshape(B, n, 128).copy()
        bs.marginalize()                                   # one pose free, same states, same packed rows: into buffer 0
        torch.cuda.synchronize()
        raw_m = bs.PL_raw[0].cpu().numpy().reshape(B, n, 48).copy()
        rec_m = bs.PL[0].cpu().numpy().reshape(B, n, 128).copy()
        bs.close()
        return flags, raw, rec, raw_m, rec_m
    f_new, raw, rec, raw_m, rec_m = run(False)
    f_old, raw_o, rec_o, raw_mo, rec_mo = run(True)
    assert f_new == 3 and f_old == 1, (f_new, f_old)
    assert np.all(raw[:, :, 45:] == 0.0) and np.all(raw_m[:, :, 21:] == 0.0) and np.all(raw_o[:, :, 45:] == 0.0) and np.all(raw_mo[:, :, 21:] == 0.0)
    assert same_bits(rec, expand(raw, True)) and same_bits(rec_m, expand(raw_m, False))
    assert np.all(rec[:, 0, :] == 0.0)                                            # frame 0 owns no blocks in the init topology
    assert np.abs(rec).max() > 0.0 and not np.array_equal(raw, raw_o)             # (a different summation order, not the same kernel)
    assert np.abs(rec_m).max() > 0.0 and not np.array_equal(raw_m, raw_mo)
    assert_records_close(rec, rec_o, "slab vs block kernel, INIT")
    assert_records_close(rec_m, rec_mo, "slab vs block kernel, MARG")
    assert np.all(rec_m[:, :, 0:36] == 0.0) and np.all(rec_m[:, :, 72:114] == 0.0)


def _track_window_sensitivity(pyoracle, orc, d, eps=1e-13, trials=3):
    """Referee for the choice of tracking windows (the idea of parity_util.init_solve_sensitivity): the ORACLE against itself on the two-frame
    window `d` (prior from its own marginalisation, moved to the older frame as the test below does) with the laser end points scaled by
    1 + eps N(0, 1) — the size of the difference between two correct fp64 summation orders.  -> largest relative state difference."""
    def run(w):
        wo = pyoracle.Window(w)
        orc.set_prior(None)
        orc.marginalization(wo)
        _, J, R = orc.get_prior()
        orc.set_prior((np.array(w["states"]).reshape(2, 15)[0].copy(), J, R))
        orc.solve(wo)
        orc.set_prior(None)
        return wo["states"].reshape(2, 15).copy()
    x0, rp, worst = run(d), np.random.default_rng(7), 0.0
    for _ in range(trials):
        pts = np.asarray(d["laser_pts"])
        worst = max(worst, rel(run(dict(d, laser_pts=pts * (1.0 + eps * rp.standard_normal(pts.shape)))), x0))
    return worst


def test_one_pose_slab_kernel_writes_compact_records_for_a_tracking_solve(liw, synth, pyoracle, env, monkeypatch):
    """k_lin_laser_slab1 in a TRACK solve: 16 400 two-frame windows (257 slabs >= the 256-slab arming threshold, not a multiple of 64), a
    handful of blocks each (6 ... 16 per frame), against the lane-per-block path: same iterations / terminations, states 1e-9, Delta_H 1e-8
    (the bars of test_gpu_laser_slab.py).
    Which windows: two kernels that sum a group in different orders differ by round-off in every record, and a tracking window tied down by
    a handful of laser blocks can amplify that without bound — most such windows crawl for 25 - 50 LM iterations and the ORACLE, run against
    itself with end points 1e-13 apart, then ends 1e-9 ... 3e-7 apart (the first version of this test drew such windows — blocks [5, 7] ...
    [14, 13], seeds 6600 .. 6603, oracle self-difference up to 9e-7 — and measured 9.1e-8 between the two kernels with equal iteration counts
    and Delta_H 1.2e-11 apart).  A 1e-9 bar between two kernels only means something where the reference itself is determined far below
    it, so the windows are drawn from seeds whose oracle self-difference is <= 1e-10, a tenth of the bar; the referee runs here, on the
    CPU, and the test asserts it before it looks at a kernel."""
    prm, orc = env
    monkeypatch.delenv("LIW_STEP_VARIANT", raising=False)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    bench = importlib.import_module("bench")
    Bt = 16400
    picks = ((6604, [0, 6, 9]), (6605, [0, 9, 12]), (6606, [0, 9, 12]), (6611, [0, 12, 16]))
    tb = [bench.sub_window(synth.make_window(orc, prm, seed=seed, n=3, frame_counts=fc), 1) for seed, fc in picks]
    for (seed, fc), w in zip(picks, tb):
        sens = _track_window_sensitivity(pyoracle, orc, w)
        print("tracking window seed %d blocks %s: oracle self-difference %.1e" % (seed, fc[1:], sens))
        assert sens <= 1e-10, (seed, fc, sens)
    tw = [tb[b % 4] for b in range(Bt)]

    def track(no_slab):
        if no_slab:
            monkeypatch.setenv("LIW_NO_LASER_SLAB", "1")
        else:
            monkeypatch.delenv("LIW_NO_LASER_SLAB", raising=False)
        bs = liw.BatchSolver(prm, tw)
        bs.marginalize()
        bs.t["prior_X"].view(Bt, 15).copy_(bs.t["x"].view(Bt, 2, 15)[:, 0])     # the prior sits on the older frame of a tracking window
        bs.solve(liw.LIW_MODE_TRACK, 0)
        flags = bs.launch_paths()["flags"]
        x, sm = bs.states().copy(), bs.summaries()
        dH = bs.marginalize()[1].cpu().numpy().reshape(Bt, 15, 15)
        bs.close()
        return flags, x, sm, dH
    fn, xn, sn, hn = track(False)
    fo, xo, so, ho = track(True)
    assert fn == 3 and fo == 1, (fn, fo)
    assert [(s["iterations"], s["termination"]) for s in sn] == [(s["iterations"], s["termination"]) for s in so]
    ex = float((np.abs(xn - xo).max(axis=(1, 2)) / np.abs(xo).max(axis=(1, 2))).max())
    eh = float((np.abs(hn - ho).max(axis=(1, 2)) / np.abs(ho).max(axis=(1, 2))).max())
    print("TRACK slab vs block kernel: states %.2e Delta_H %.2e" % (ex, eh))
    assert ex <= 1e-9 and eh <= 1e-8                                              # (the bars of test_gpu_laser_slab.py)


# ------------------------------------------------------------------------------------------------ 3. the step kernels
def _oracle_history(pyoracle, orc, d, iters):
    wo = pyoracle.Window(d)
    orc.set_prior(None)
    orc.set_max_iterations(iters)
    orc.init_solve(wo)
    so, ho = orc.summary(), orc.iterations()
    orc.set_max_iterations(50)
    return wo, so, ho


def _check_against_oracle_histories(liw, pyoracle, orc, prm, wins, distinct, n, iters):
    B = len(wins)
    bs = liw.BatchSolver(prm, wins, history_records=iters + 1)
    assert int(bs.lay.laser_partial_stride) == 48
    bs.solve(liw.LIW_MODE_INIT, iters)
    got, summ, hist = bs.states(), bs.summaries(), bs.history()
    bs.close()
    worst = 0.0
    for k in range(distinct):
        wo, so, ho = _oracle_history(pyoracle, orc, wins[k], iters)
        for b in range(k, B, distinct):
            assert (summ[b]["iterations"], summ[b]["termination"]) == (so["iterations"], so["termination"]), (n, k, b, summ[b], so)
            for it in range(len(ho)):
                xo = ho[it]["x"].reshape(n, 15)
                e = float(np.abs(hist[it, b] - xo).max() / max(np.abs(xo).max(), 1e-12))
                worst = max(worst, e)
                assert e <= 1e-6, (n, k, b, it, e)
            assert rel(got[b], wo["states"].reshape(n, 15)) <= 1e-6
            assert abs(summ[b]["final_cost"] - so["final_cost"]) <= 1e-6 * max(so["final_cost"], 1e-300)
    return worst


@pytest.mark.parametrize("n", [1, 2, 7])
def test_quad_step_on_compact_records_follows_the_oracle_iteration_by_iteration(liw, synth, pyoracle, env, monkeypatch, n):
    prm, orc = env
    B, iters = 6, 20
    base = [synth.make_window(orc, prm, seed=6700 + 17 * n + k, n=n, L=(0 if (k == 3 or n == 1) else 20 * n + 37 * k)) for k in range(5)]
    monkeypatch.setenv("LIW_STEP_VARIANT", "3")
    worst = _check_against_oracle_histories(liw, pyoracle, orc, prm, [base[b % 5] for b in range(B)], 5, n, iters)
    print("n=%d: worst per-iteration state error %.2e" % (n, worst))


def test_one_wave_step_reads_compact_records_next_to_the_quad_kernel(liw, synth, pyoracle, env, monkeypatch):
    """B = 6, n = 4; windows 1 and 4 carry |theta| > pi (so3 Plus Jacobian != I): k_lm_step takes them in the same launch pair and
    reads the compact records through the slot map; every window follows the oracle per iteration."""
    prm, orc = env
    n, iters = 4, 20
    wins = [synth.make_window(orc, prm, seed=6800 + k, n=n, L=40 + 9 * k) for k in range(6)]
    for k in (1, 4):
        st = wins[k]["states"]
        for f in (0, 2):
            q = st[f, 3:6]
            a = np.linalg.norm(q)
            st[f, 3:6] = q / a * (a - 2 * np.pi)      # same rotation, |q| = 2 pi - a > pi
        assert np.linalg.norm(st[0, 3:6]) > np.pi
        wins[k]["match_pose"][:, 0:6] = st[0, 0:6]
        wins[k]["match_pose"][:, 6:12] = st[:, 0:6]
    monkeypatch.setenv("LIW_STEP_VARIANT", "3")
    worst = _check_against_oracle_histories(liw, pyoracle, orc, prm, wins, 6, n, iters)
    print("wrapped rotations: worst per-iteration state error %.2e" % worst)


# ------------------------------------------------------------------------------------------------ 4. the factor-sharded exchange
def test_factor_sharded_exchange_of_compact_records(liw, synth, pyoracle, env, monkeypatch):
    """Two lock-step rank objects in the compact format (LIW_STEP_VARIANT=3, B = 5): states identical across ranks, iteration counts and
    terminations those of the un-sharded solve, through both exchange variants."""
    import threading
    import torch
    prm, orc = env
    monkeypatch.setenv("LIW_STEP_VARIANT", "3")
    n, K, nb, B = 6, 12, 4, 5
    base = [synth.make_window(orc, prm, seed=6900 + k, n=n, L=40 + 23 * k) for k in range(nb)]
    windows = [base[b % nb] for b in range(B)]
    ref = liw.BatchSolver(prm, windows)
    assert int(ref.lay.laser_partial_stride) == 48
    ref.solve(liw.LIW_MODE_INIT, K)
    rs, rsum = ref.states(), ref.summaries()
    ref.close()
    for xch in ("allreduce", "oneshot"):
        comms = liw.batch.LockstepComm.make(2)
        ranks = [liw.BatchSolver(prm, windows, rank=r, world=2, exchange=xch, comm=comms[r]) for r in range(2)]
        errs = []

        def drive(rk):
            try:
                rk.solve(liw.LIW_MODE_INIT, K)
            except Exception as e:   # noqa: BLE001
                errs.append(e)
                comms[0].sh["bar"].abort()
        th = [threading.Thread(target=drive, args=(rk,)) for rk in ranks]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
        torch.cuda.synchronize()
        a, b = ranks[0].states(), ranks[1].states()
        assert np.array_equal(a, b), xch
        sa, sb = ranks[0].summaries(), ranks[1].summaries()
        assert [(s["iterations"], s["termination"]) for s in sa] == [(s["iterations"], s["termination"]) for s in sb], xch
        assert [(s["iterations"], s["termination"]) for s in sa] == [(s["iterations"], s["termination"]) for s in rsum], xch
        assert rel(a, rs) <= 1e-9, xch
        for rk in ranks:
            rk.close()
