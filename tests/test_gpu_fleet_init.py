"""The initialisation glue on the device (liw_lfe_init_reset / _begin / _select / _commit, liw_lfe_slot_copy, liw_lfe_pack_init_sel;
laser_batch.BatchFrontEnd) against the host restatement of lvio_2d::trajectory while INITIALIZING in tests/fleet_init_reference.py:
init_begin case by case at two parameter sets, the slot copy byte for byte, the ready list and the selected pack against
liw_lfe_pack_init on a front-end built from exactly the selected robots, the commit's bookkeeping, determinism at 4 096 robots and
the argument checks.  References: the restatement, numpy, and the entry points that were there before; never the new code's output.

Measured on an MI355X (pytest tests/test_gpu_fleet_init.py -m gpu -s): see the "Fleet cold start" section of docs/WIDENING.md."""
import numpy as np
import pytest

import fleet_init_reference as ref
from test_gpu_laser_init import (B0, R_EMPTY_FRONT, R_INVALID, R_ONE_WALL, _lane_reference, _regions, _spawned, env,  # noqa: F401
                                 gentle)

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
BAR = 1e-12   # tests/test_gpu_laser_track.py::test_begin_end_against_restatement: the same chain of 3 x 3 products and one log_SO3
G = 256
FILL, FILL_B, FILL_I = -7.25, 0xA5, -77


def _guarded(torch, n, dtype, fill):
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    return buf, buf[G:G + n]


def _guards_ok(buf, fill):
    return bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def _dims(B, slots):
    return dict(B=B, slots=slots, max_points=1080, max_lines=256, max_cell_entries=8192)


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _glue(liw, synth, name):
    _, tp, lp, ip = [s for s in ref.init_param_sets(liw, synth) if s[0] == name][0]
    return tp, lp, ip, ref.InitGlue(liw, tp, lp["T_imu_to_laser"], lp["normalize_extrinsics"], ip)


# --------------------------------------------------------------------------------------------------------- reset, getter
def test_init_reset_and_get(liw, synth):
    import torch
    tp, lp, ip, g = _glue(liw, synth, "second")
    B = 130
    fe = liw.laser_batch.BatchFrontEnd(lp, _dims(B, 2))
    buf, rec = _guarded(torch, fe.init_layout(), torch.uint8, FILL_B)
    mask = np.ones(B, dtype=np.uint8)
    mask[[0, 63, 64, 129]] = 0
    fe.init_reset(tp, rec, mask=mask)
    torch.cuda.synchronize()
    r = ref.unpack_records(rec.cpu().numpy(), B)
    on = mask.astype(bool)
    assert (r["raw"][~on] == FILL_B).all() and _guards_ok(buf, FILL_B)
    want = g.init_state()
    assert _rel(r["state"][on], np.tile(want, (int(on.sum()), 1))) <= BAR
    assert np.linalg.norm(want[0:3]) > 0.1 and np.linalg.norm(want[3:6]) > 0.1   # the second set's extrinsic is not the identity
    assert not r["state"][on][:, 6:].any() and not r["ang"][on].any() and not r["counters"][on].any()
    assert (r["status"][on] == ref.INITIALIZING).all() and (r["n_frames"][on] == 0).all() and not r["raw"][on][:, 164:].any()
    one = fe.init_get(rec, 5)
    assert one["status"] == ref.INITIALIZING and one["n_frames"] == 0 and np.array_equal(one["state"], r["state"][5])
    assert (one["inits"], one["failed"], one["dropped"]) == (0, 0, 0)
    fe.init_reset(tp, rec)   # no mask: every robot
    torch.cuda.synchronize()
    r = ref.unpack_records(rec.cpu().numpy(), B)
    assert (r["status"] == ref.INITIALIZING).all() and np.array_equal(r["raw"], np.tile(r["raw"][1], (B, 1)))
    fe.close()


# ------------------------------------------------------------------------------------------------------------ init_begin
@pytest.mark.parametrize("name", ["office", "second"])
def test_init_begin_against_restatement(liw, synth, name):
    """B = 130 (two full waves and a two-lane tail) per page; the generator's cross product of wheel increments at
    {0.5, 0.98, 1.02, 2} x each threshold with n_frames 0, 1, N - 1 and robots that are already TRACKING; five robots masked out."""
    import torch
    tp, lp, ip, g = _glue(liw, synth, name)
    N, B = ip["slide_window_size"], 130
    fe = liw.laser_batch.BatchFrontEnd(lp, _dims(B, N + 1))
    masked = np.array([3, 64, 65, 127, 129])
    mask = np.ones(B, dtype=np.uint8)
    mask[masked] = 0
    on = mask.astype(bool)
    worst, combos = dict(pose=0.0, ang=0.0), set()
    for page in range(2):
        c = ref.make_cases(g, B, seed=60 + page, page=page)
        combos.update(tuple(int(v) for v in row) for row in c["combo"])
        e = ref.expected(g, c, mask=mask)
        act = on & (c["status"] == ref.INITIALIZING)
        for b in np.nonzero(act)[0]:   # no threshold quantity within 1e-3 relative of its threshold
            for value, thr in ((e["dp"][b], ip["p_motion_threshold"]), (e["dq"][b], ip["q_motion_threshold"])):
                assert abs(value - thr) >= 1e-3 * thr, (b, value, thr)
        raw0 = ref.pack_records(c["state"], c["ang"], c["status"], c["n_frames"], c["counters"])
        rbuf, rec = _guarded(torch, B * 256, torch.uint8, FILL_B)
        rec.copy_(_up(torch, raw0.reshape(-1)))
        xbuf, x_init = _guarded(torch, B * N * 15, torch.float64, FILL)
        win = {k: _guarded(torch, B * (N - 1) * w, torch.float64, FILL) for k, w in ref.INTERVAL}
        dbuf, drop = _guarded(torch, B, torch.uint8, FILL_B)
        sbuf, slot_of = _guarded(torch, B, torch.int32, FILL_I)
        iv = {k: _up(torch, c[k]) for k, _ in ref.INTERVAL}
        fe.init_begin(tp, ip, rec, iv, dict(x_init=x_init, **{k: v[1] for k, v in win.items()}), mask=mask, out=dict(drop=drop, slot_of=slot_of))
        torch.cuda.synchronize()
        r = ref.unpack_records(rec.cpu().numpy(), B)
        xs = x_init.cpu().numpy().reshape(B, N, 15)
        d, s = drop.cpu().numpy(), slot_of.cpu().numpy()
        went, dropped, idle = e["row"] >= 0, e["drop"] == 1, e["drop"] == -1
        assert went.sum() > 20 and dropped.sum() > 5 and (idle & on).sum() > 20
        # decisions and counters
        assert np.array_equal(d[~idle], e["drop"][~idle]) and (d[idle] == FILL_B).all()
        assert np.array_equal(s[went], e["slot_of"][went]) and (s[~went] == FILL_I).all()
        assert np.array_equal(r["n_frames"], e["n_frames"]) and np.array_equal(r["status"], e["status"]) and np.array_equal(r["counters"], e["counters"])
        # masked robots and robots that are TRACKING: no byte of the record; dropped robots: the dropped counter alone
        assert np.array_equal(r["raw"][idle], raw0[idle])
        a, z = r["raw"][dropped].copy(), raw0[dropped].copy()
        a[:, 160:164] = z[:, 160:164]
        assert np.array_equal(a, z)
        # the predicted state: the record and row k of x_init; v and bs carried bit for bit
        worst["pose"] = max(worst["pose"], _rel(r["state"][went], e["state"][went]))
        rows = xs[np.nonzero(went)[0], e["row"][went]]
        assert np.array_equal(rows.view(np.int64), r["state"][went].view(np.int64))
        assert np.array_equal(rows[:, 6:15].view(np.int64), c["state"][went][:, 6:15].view(np.int64))
        worst["ang"] = max(worst["ang"], _rel(r["ang"][went], e["ang"][went]))
        written = np.zeros((B, N), dtype=bool)
        written[np.nonzero(went)[0], e["row"][went]] = True
        assert (xs[~written] == FILL).all()
        # the interval rows: row k - 1 for k >= 1, bit for bit; every other row untouched
        wrote = np.zeros((B, N - 1), dtype=bool)
        src = went & (e["row"] >= 1)
        wrote[np.nonzero(src)[0], e["row"][src] - 1] = True
        assert src.sum() > 10 and (went & (e["row"] == 0)).sum() > 5
        for k, w in ref.INTERVAL:
            wv = win[k][1].cpu().numpy().reshape(B, N - 1, w)
            assert np.array_equal(wv[np.nonzero(src)[0], e["row"][src] - 1].view(np.int64), c[k][src].view(np.int64)), k
            assert (wv[~wrote] == FILL).all(), k
        for buf, fill in [(rbuf, FILL_B), (xbuf, FILL), (dbuf, FILL_B), (sbuf, FILL_I)] + [(v[0], FILL) for v in win.values()]:
            assert _guards_ok(buf, fill)
    assert len(combos) == ref.N_COMBOS
    print("init_begin, %s set, 2 x %d robots: worst |device - restatement| / max(1, |value|): %s" % (name, B, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= BAR, (k, v)
    fe.close()


# ------------------------------------------------------------------------------------------------------------- slot_copy
def test_slot_copy(env):  # noqa: F811
    """24 robots, five slots: slot 0 holds an empty scan, the zig-zag ring, an invalid slot and rooms; every robot copies into a slot
    of its own choice that held another scan before; three robots are masked out and three give a bad destination."""
    liw, lp, sc, torch = env
    from test_gpu_laser_batch import N_RAYS, _fe, _pose
    from test_gpu_laser_init import _zigzag
    B, slots = 24, 5
    dims = _dims(B, slots)
    fe = _fe(liw, lp, B, slots=slots)
    rng = np.random.default_rng(77)
    for s in range(slots):   # every slot of every robot holds some room scan first
        P, n = liw.laser_batch.pad_points([sc.points(b, _pose(rng), seed=100 * s + b)[0] for b in range(B)], N_RAYS)
        if s == 0:
            P[0], n[0] = 0.0, 0                      # an empty scan
            z = _zigzag(liw, 9)
            P[1, :len(z)], n[1] = z, len(z)          # the ring
            n[2] = N_RAYS + 1                        # an invalid slot
        fe.spawn(s, _up(torch, P), _up(torch, n))
    torch.cuda.synchronize()
    assert fe.num_lines(0, 0) == 0 and fe.status(0, 0) == 0 and fe.num_lines(1, 0) >= 90 and fe.status(2, 0) != 0
    dst = (1 + (np.arange(B) * 3) % (slots - 1)).astype(np.int32)
    assert set(dst.tolist()) == set(range(1, slots))
    bad = {5: 0, 11: slots, 17: -1}
    for b, v in bad.items():
        dst[b] = v
    mask = np.ones(B, dtype=np.uint8)
    mask[[6, 12, 23]] = 0
    rb, sb = _regions(dims)
    before = fe.store.cpu().numpy().reshape(B, rb).copy()
    fe.slot_copy(dst, mask=mask)
    torch.cuda.synchronize()
    after = fe.store.cpu().numpy().reshape(B, rb)
    slot = lambda a, b, s: a[b, 256 + s * sb:256 + (s + 1) * sb]
    ent0 = 32 + 80 * dims["max_lines"]
    odd = 0
    for b in range(B):
        if not mask[b]:
            assert np.array_equal(after[b], before[b]), b
            continue
        if b in bad:
            assert np.array_equal(after[b, 4:], before[b, 4:]) and fe.status(b) & liw.laser_batch.ST_INVALID, b
            continue
        src, old, new = slot(before, b, 0), slot(before, b, dst[b]), slot(after, b, dst[b])
        h = src[:32].view(np.int32)
        nl, ne = int(np.clip(h[1], 0, dims["max_lines"])), int(np.clip(h[2], 0, dims["max_cell_entries"]))
        odd += ne & 1
        assert np.array_equal(new[:32], src[:32]), b                                        # header, status word included
        assert np.array_equal(new[32:32 + 80 * nl], src[32:32 + 80 * nl]), b               # lines[0 .. n_lines)
        assert np.array_equal(new[ent0:ent0 + 8 * ne], src[ent0:ent0 + 8 * ne]), b         # ent[0 .. n_entries)
        assert np.array_equal(new[32 + 80 * nl:ent0], old[32 + 80 * nl:ent0]) and np.array_equal(new[ent0 + 8 * ne:], old[ent0 + 8 * ne:]), b
        rest = np.ones(rb, dtype=bool)
        rest[256 + dst[b] * sb:256 + (dst[b] + 1) * sb] = False
        assert np.array_equal(after[b, rest], before[b, rest]), b                           # the manager, every other slot, the sub-maps
        assert fe.status(b, int(dst[b])) == fe.status(b, 0) and fe.num_lines(b, int(dst[b])) == fe.num_lines(b, 0)
    assert 0 < odd < B - 6   # odd and even entry counts: the 8-byte tail and the pure 16-byte path
    for b in set(range(B)) - set(bad):
        assert not fe.status(b) & liw.laser_batch.ST_INVALID or b == 2, b
    assert fe.status(2, int(dst[2])) != 0 and fe.num_lines(0, int(dst[0])) == 0
    fe.close()


# ------------------------------------------------------------------------------------------- init_select, pack_init_sel
def _select_case(B, N, ready_set, seed):
    """records in which exactly ready_set is INITIALIZING with a full window; the others are TRACKING with n_frames = N, or
    INITIALIZING with fewer frames"""
    rng = np.random.default_rng(seed)
    status = np.where(np.arange(B) % 3 == 0, ref.TRACKING, ref.INITIALIZING).astype(np.int32)
    n_frames = np.where(status == ref.TRACKING, N, rng.integers(0, N, B)).astype(np.int32)
    for b in ready_set:
        status[b], n_frames[b] = ref.INITIALIZING, N
    return ref.pack_records(rng.normal(0, 1, (B, 15)), rng.normal(0, 1, (B, 3)), status, n_frames, rng.integers(0, 9, (B, 3)))


@pytest.mark.parametrize("which", ["none", "one", "five", "all"])
def test_select_and_pack_sel(env, gentle, which):  # noqa: F811
    liw, lp, sc, torch = env
    B, n = B0, 6
    F = n - 1
    base = gentle
    pf, poses = base["pf"], np.ascontiguousarray(base["poses"][:, :F])
    fe = _spawned(env, base, B, n)
    probe = _lane_reference(fe, F, pf, poses, 0, 256)["count"]
    cap = int(probe.max()) - 1                       # one below the largest count: that robot's match overflows
    over = int(np.nonzero((probe > cap).any(1))[0][0])
    regular = [b for b in range(5, B) if b != over]
    S = dict(none=[], one=[regular[3]], five=sorted({R_EMPTY_FRONT, R_ONE_WALL, R_INVALID, over, regular[0]}), all=list(range(B)))[which]
    R = len(S)
    fe = _spawned(env, base, B, n)
    m = fe.match_front(0, 1, F, pf, poses, cap=cap)
    ip = dict(slide_window_size=n, p_motion_threshold=0.1, q_motion_threshold=0.1)
    raw = _select_case(B, n, S, seed=len(S))
    rec = _up(torch, raw.reshape(-1))
    bufs = dict(ready=_guarded(torch, B, torch.uint8, FILL_B), sel=_guarded(torch, B, torch.int32, FILL_I), n_sel=_guarded(torch, 1, torch.int32, FILL_I))
    R_host = torch.full((1,), -5, dtype=torch.int32).pin_memory()
    o = fe.init_select(ip, rec, out={k: v[1] for k, v in bufs.items()}, R_host=R_host)
    torch.cuda.synchronize()
    assert int(R_host[0]) == R == int(o["n_sel"].cpu()[0])
    want = np.zeros(B, dtype=np.uint8)
    want[S] = 1
    sel = o["sel"].cpu().numpy()
    assert np.array_equal(o["ready"].cpu().numpy(), want) and np.array_equal(sel[:R], np.array(S, dtype=np.int32)) and (sel[R:] == FILL_I).all()
    assert all(_guards_ok(v[0], f) for v, f in ((bufs["ready"], FILL_B), (bufs["sel"], FILL_I), (bufs["n_sel"], FILL_I)))
    assert np.array_equal(rec.cpu().numpy().reshape(B, 256), raw)   # the records are only read
    if R == 0:
        with pytest.raises(liw.LiwError) as e:
            fe.pack_init_sel(0, o["sel"], m, n, pf)
        assert e.value.code == EINVAL
        fe.close()
        return
    # the reference: liw_lfe_pack_init on a front-end that consists of exactly the selected robots
    rob = np.array(S)
    fs = _spawned(env, base, R, n, rob)
    ms = fs.match_front(0, 1, F, pf[rob], poses[rob], cap=cap)
    want_dev, Ltot, want_ok = fs.pack_init(ms, n, pf[rob])
    torch.cuda.synchronize()
    if which in ("five", "all"):
        assert (want_ok.cpu().numpy()[:R] == 0).sum() >= len({R_EMPTY_FRONT, R_ONE_WALL, R_INVALID, over}) >= 3 and (want_ok.cpu().numpy()[:R] == 1).sum() >= 1
    x_init = torch.full((B, n, 15), FILL, dtype=torch.float64, device="cuda")
    x_init[:, 0, 0:6] = _up(torch, pf)
    sizes = dict(laser_off=(R + 1, torch.int32), laser_frame=(max(Ltot, 1), torch.int32), laser_pts=(12 * max(Ltot, 1), torch.float64),
                 match_pose=(R * n * 12, torch.float64), has_match=(R * n, torch.uint8), init_ok=(R, torch.uint8))

    def run(L_cap):
        gd = {k: torch.full((s + 2 * G,), 77, dtype=dt, device="cuda") for k, (s, dt) in sizes.items()}
        v = {k: t[G:-G] for k, t in gd.items()}
        try:
            res = fe.pack_init_sel(R, o["sel"], m, n, x_init[:, 0], out={k: v[k] for k in ("match_pose", "has_match", "init_ok")}, L_cap=L_cap,
                                   bufs={k: v[k] for k in ("laser_off", "laser_frame", "laser_pts")})
        except liw.LiwError as err:
            res = err.code
        torch.cuda.synchronize()
        return gd, v, res

    gd, v, (dev, Lt, ok) = run(Ltot)
    assert Lt == Ltot
    assert np.array_equal(ok.cpu().numpy()[:R], want_ok.cpu().numpy()[:R])
    assert np.array_equal(v["laser_off"].cpu().numpy(), want_dev["laser_off"].cpu().numpy()[:R + 1])
    for k, cnt in (("laser_frame", Ltot), ("laser_pts", 12 * Ltot), ("match_pose", R * n * 12), ("has_match", R * n)):
        assert np.array_equal(v[k].cpu().numpy()[:cnt], want_dev[k].cpu().numpy()[:cnt]), k
    for k, t in gd.items():
        assert (t[:G] == 77).all() and (t[-G:] == 77).all(), k
    if Ltot > 0:   # one block too few: LIW_ENOMEM and nothing but laser_off written
        g3, v3, code = run(Ltot - 1)
        assert code == ENOMEM
        for k, t in g3.items():
            if k == "laser_off":
                assert (t[:G] == 77).all() and (t[-G:] == 77).all() and np.array_equal(v3[k].cpu().numpy(), v["laser_off"].cpu().numpy())
            else:
                assert (t == 77).all(), k
    fe.close()
    fs.close()


# ---------------------------------------------------------------------------------------------------------------- commit
def test_init_commit(liw, synth):
    """five selected robots of 37, two of them without init_ok, a compact batch padded to 8 windows: the solved windows, the tracking
    rows and both records of the committed robots, the restart of the failed ones, nothing of anybody else"""
    import torch
    tp, lp, ip, g = _glue(liw, synth, "second")
    B, N, R = 37, ip["slide_window_size"], 5
    fe = liw.laser_batch.BatchFrontEnd(lp, _dims(B, N + 1))
    rng = np.random.default_rng(8)
    S = np.array([1, 7, 8, 30, 36], dtype=np.int32)
    ok = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    raw0 = _select_case(B, N, S.tolist(), seed=3)
    rec = _up(torch, raw0.reshape(-1))
    x_sol = rng.normal(0, 1, (8, N, 15))
    x_sol[:, :, 3:6] *= 0.3
    tbuf, track = _guarded(torch, B * 256, torch.uint8, FILL_B)
    xi_buf, x_init = _guarded(torch, B * N * 15, torch.float64, FILL)
    xt_buf, x_track = _guarded(torch, B * 30, torch.float64, FILL)
    sel = torch.full((B,), FILL_I, dtype=torch.int32, device="cuda")
    sel[:R] = _up(torch, S)
    fe.init_commit(tp, ip, rec, track, R, sel, _up(torch, ok), _up(torch, x_sol), x_init, x_track)
    torch.cuda.synchronize()
    r0, r = ref.unpack_records(raw0, B), ref.unpack_records(rec.cpu().numpy(), B)
    xi, xt, tr = x_init.cpu().numpy().reshape(B, N, 15), x_track.cpu().numpy().reshape(B, 2, 15), track.cpu().numpy().reshape(B, 256)
    good, bad = S[ok == 1], S[ok == 0]
    others = np.setdiff1d(np.arange(B), S)
    assert np.array_equal(r["raw"][others], raw0[others]) and (xi[others] == FILL).all() and (xt[others] == FILL).all() and (tr[others] == FILL_B).all()
    # committed: the solved window, the tracking rows, take_back_state, TRACKING, the counter; the tracking record as track_init makes it
    assert np.array_equal(xi[good], x_sol[:R][ok == 1]) and np.array_equal(xt[good, 0], x_sol[:R][ok == 1][:, N - 1]) and np.array_equal(xt[good, 0], xt[good, 1])
    assert np.array_equal(r["state"][good], xt[good, 1]) and (r["status"][good] == ref.TRACKING).all()
    assert np.array_equal(r["counters"][good], r0["counters"][good] + np.array([1, 0, 0])) and np.array_equal(r["ang"][good], r0["ang"][good])
    want_track = torch.full((B * 256,), FILL_B, dtype=torch.uint8, device="cuda")
    m = np.zeros(B, dtype=np.uint8)
    m[good] = 1
    fe.track_init(tp, want_track, x_track.view(B, 2, 15)[:, 1], r0["ang"], mask=m)
    assert np.array_equal(tr[good], want_track.cpu().numpy().reshape(B, 256)[good])
    # failed: init_current_status with the counters kept, the failed-window counter; no x row, no tracking record
    assert _rel(r["state"][bad], np.tile(g.init_state(), (len(bad), 1))) <= BAR and not r["ang"][bad].any()
    assert (r["status"][bad] == ref.INITIALIZING).all() and (r["n_frames"][bad] == 0).all()
    assert np.array_equal(r["counters"][bad], r0["counters"][bad] + np.array([0, 1, 0]))
    assert (xi[bad] == FILL).all() and (xt[bad] == FILL).all() and (tr[bad] == FILL_B).all()
    assert _guards_ok(tbuf, FILL_B) and _guards_ok(xi_buf, FILL) and _guards_ok(xt_buf, FILL)
    fe.close()


# ----------------------------------------------------------------------------------------------------------- determinism
def test_glue_deterministic_at_4096(liw, synth):
    """4 096 robots through N + 3 frames of reset -> (init_begin -> init_select) twice: records, windows, decisions and ready lists
    bitwise identical, and the ready robots are exactly those that were not dropped N times"""
    import torch
    tp, lp, ip, g = _glue(liw, synth, "office")
    N, B = ip["slide_window_size"], 4096
    fe = liw.laser_batch.BatchFrontEnd(lp, dict(B=B, slots=N + 1, max_points=64, max_lines=8, max_cell_entries=64))
    pages = [ref.make_cases(g, 128, seed=90 + t, page=t) for t in range(N + 3)]
    runs = []
    for _ in range(2):
        rec = torch.zeros(fe.init_layout(), dtype=torch.uint8, device="cuda")
        fe.init_reset(tp, rec)
        win = fe.init_window(N)
        log = []
        for c in pages:
            iv = {k: _up(torch, np.tile(c[k], (B // 128, 1))) for k, _ in ref.INTERVAL}
            o = fe.init_begin(tp, ip, rec, iv, win)
            s = fe.init_select(ip, rec)
            log += [o["drop"].clone(), o["slot_of"].clone(), s["ready"].clone(), s["sel"].clone(), s["n_sel"].clone()]
        torch.cuda.synchronize()
        runs.append([rec] + list(win.values()) + log)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    r = ref.unpack_records(runs[0][0].cpu().numpy(), B)
    n_sel = int(runs[0][-1].cpu()[0])
    # the state machine by the restatement: a frame is dropped or taken until the window is full; a full window takes no more frames
    nf, dropped = np.zeros(128, dtype=np.int32), np.zeros(128, dtype=np.int32)
    for c in pages:
        for b in range(128):
            if nf[b] < N:
                if g.drop(c["wheel_T"][b]):
                    dropped[b] += 1
                else:
                    nf[b] += 1
    assert np.array_equal(r["n_frames"], np.tile(nf, B // 128)) and np.array_equal(r["counters"][:, 2], np.tile(dropped, B // 128))
    assert 0 < n_sel == int((nf == N).sum()) * (B // 128) and dropped.any()
    fe.close()


# ------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(env):  # noqa: F811
    """every LIW_EINVAL case of the header text leaves the store, the records and the outputs untouched"""
    import ctypes as C
    liw, lp, sc, torch = env
    lb = liw.laser_batch
    B, N = 8, 4
    fe = lb.BatchFrontEnd(lp, _dims(B, N + 1))
    L, h = fe.L, fe.h
    tps = lb.track_params_struct(lb.office_track_params())
    ips = lb.init_params_struct(dict(slide_window_size=N, p_motion_threshold=0.1, q_motion_threshold=0.1))
    big = lb.init_params_struct(dict(slide_window_size=N + 1, p_motion_threshold=0.1, q_motion_threshold=0.1))   # needs slots >= N + 2
    one = lb.init_params_struct(dict(slide_window_size=1, p_motion_threshold=0.1, q_motion_threshold=0.1))
    buf = torch.full((1 << 16,), 3.25, dtype=torch.float64, device="cuda")
    rec = torch.zeros(fe.init_layout(), dtype=torch.uint8, device="cuda")
    fe.init_reset(tps, rec)
    torch.cuda.synchronize()
    store0, rec0, buf0 = fe.store.clone(), rec.clone(), buf.clone()
    p, st, rc = C.c_void_p(buf.data_ptr()), C.c_void_p(fe.store.data_ptr()), C.c_void_p(rec.data_ptr())
    t, i = C.byref(tps), C.byref(ips)
    calls = [L.liw_lfe_init_reset(h, None, rc, None, None), L.liw_lfe_init_reset(h, t, None, None, None),
             L.liw_lfe_init_get(h, None, 0, None, None, None, None, None), L.liw_lfe_init_get(h, rc, B, None, None, None, None, None),
             L.liw_lfe_init_get(h, rc, -1, None, None, None, None, None),
             L.liw_lfe_slot_copy(h, None, p, None, None), L.liw_lfe_slot_copy(h, st, None, None, None),
             L.liw_lfe_slot_copy(h, C.c_void_p(fe.store.data_ptr() + 8), p, None, None),
             L.liw_lfe_init_select(h, None, rc, p, p, p, None, None), L.liw_lfe_init_select(h, i, None, p, p, p, None, None),
             L.liw_lfe_init_select(h, i, rc, None, p, p, None, None), L.liw_lfe_init_select(h, i, rc, p, None, p, None, None),
             L.liw_lfe_init_select(h, i, rc, p, p, None, None, None), L.liw_lfe_init_select(h, C.byref(one), rc, p, p, p, None, None)]
    begin = [t, i, rc] + [p] * 6 + [None] + [p] * 9
    for k in [0, 1, 2] + list(range(3, 9)) + list(range(10, 19)):   # every pointer but the mask
        a = list(begin)
        a[k] = None
        calls.append(L.liw_lfe_init_begin(h, *a, None))
    for bad_ip in (big, one):
        a = list(begin)
        a[1] = C.byref(bad_ip)
        calls.append(L.liw_lfe_init_begin(h, *a, None))
    pack = [1, p, N, 8, p, p, p, p, 6, 64, p, p, p, p, p, p]
    for k, v in [(0, 0), (0, B + 1), (1, None), (2, 1), (3, 0), (8, 5), (9, -1)] + [(k, None) for k in (4, 5, 6, 7, 10, 11, 12, 13, 14)]:
        a = list(pack)
        a[k] = v
        calls.append(L.liw_lfe_pack_init_sel(h, *a, None))
    commit = [t, i, rc, p, 1, p, p, p, p, p]
    for k, v in [(4, 0), (4, B + 1), (1, C.byref(one))] + [(k, None) for k in (0, 1, 2, 3, 5, 6, 7, 8, 9)]:
        a = list(commit)
        a[k] = v
        calls.append(L.liw_lfe_init_commit(h, *a, None))
    torch.cuda.synchronize()
    assert calls and all(c == EINVAL for c in calls), calls
    assert torch.equal(fe.store, store0) and torch.equal(rec, rec0) and torch.equal(buf, buf0)
    fe.close()


# ------------------------------------------------------------------------------------------------------ the driver's scenes
from test_gpu_laser_track import ANG_INC, ANG_MIN, N_RAYS, T_INC, _cast, _frame, _interval  # noqa: E402

NB, NW, FRAMES = 8, 4, 10   # trajectories, the INIT window, frames after the start frame
IP = dict(slide_window_size=NW, p_motion_threshold=0.1, q_motion_threshold=0.1)


@pytest.fixture(scope="module")
def cold(liw, synth):
    """the fleet scene of tests/test_gpu_laser_track.py with more frames: 8 trajectories x 10 frames after the start frame (0.15 m a
    frame: above the motion threshold), the intervals' pre-integrations, scans cast from the truth"""
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
    tp = dict(liw.laser_batch.office_track_params(prm), key_frame_p_motion_threshold=0.25)
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=FRAMES + 1, L=0) for j in range(NB)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(FRAMES + 1, 15) for t in trajs])
    ranges = np.stack([[_cast(liw, synth, lp, 3000 + j, truth[j, k, 0:6], seed=j * 10 + k) for k in range(FRAMES + 1)] for j in range(NB)])
    return dict(prm=prm, lp=lp, tp=tp, nb=NB, F=FRAMES, trajs=trajs, truth=truth, ranges=ranges, times=np.stack([t["times"] for t in trajs]))


def _traj_dims(B):
    return dict(B=B, slots=NW + 1, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)


def _trajectory(liw, sc, B):
    ft = liw.FleetTrajectory(sc["prm"], sc["lp"], sc["tp"], IP, _traj_dims(B))
    ft.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    return ft


def _store_parts(fe, B):
    """the manager records and the two sub-map slots of every robot (what tracking reads and writes besides scan slot 0)"""
    rb, sb = _regions(_traj_dims(B))
    v = fe.store.view(B, rb)
    return v[:, :256].clone(), v[:, 256 + (NW + 1) * sb:].clone()


def _its(bs):
    return [(s["iterations"], s["termination"]) for s in bs.summaries()]


def test_lock_step_equals_existing_path(liw, synth, cold):
    """16 robots (8 trajectories) that all move in every frame: their windows fill together, R = B, and the driver must do what the
    entry points that were there before do for such a fleet — spawn per frame, match_front, pack_init, the INIT solve at the same batch
    size, marginalisation, rebuild, FleetTracker.start and three tracking frames — fed with the restatement's predicted states.
    Expectation: bit-identical (same kernels, same inputs)."""
    import torch
    sc, B, N = cold, 16, NW
    rob = np.arange(B) % NB
    g = ref.InitGlue(liw, sc["tp"], sc["lp"]["T_imu_to_laser"], sc["lp"].get("normalize_extrinsics", True), IP)
    # ---- the driver
    ft = _trajectory(liw, sc, B)
    log = []
    for k in range(1, N + 4):
        r, st = _frame(torch, sc, rob, k)
        o = ft.step(r, st, _interval(torch, sc, rob, k))
        torch.cuda.synchronize()
        rec = dict(x=ft.x.clone(), track=ft.track.clone(), store=_store_parts(ft.fe, B), its=_its(ft.bs), Ltot=o["Ltot"],
                   **{n: ft.bs.t[n].clone() for n in ("prior_X", "prior_J", "prior_R", "has_prior")},
                   **{n: o[n].clone() for n in ("skip", "key", "flags", "status", "drop", "ready", "init_ok", "pose")})
        if k == N:
            rec.update(x_init=ft.win["x_init"].clone(), init_its=_its(ft._init_bs[B]), last_init=ft.last_init)
        if k == N - 1:
            rec.update(x_pred=ft.win["x_init"].clone())
        log.append(rec)
    for k, rec in enumerate(log, 1):
        assert not rec["drop"].any() and not rec["skip"].any(), k
        assert bool(rec["ready"].all()) == bool(rec["init_ok"].all()) == (k == N), k
        assert bool((rec["status"] == (ref.TRACKING if k >= N else ref.INITIALIZING)).all()), k
    assert log[N - 1]["last_init"][:2] == (B, B)   # no padding: the solver size of the reference
    # ---- the existing path
    rt = liw.FleetTracker(sc["prm"], sc["lp"], sc["tp"], _traj_dims(B))
    fe = rt.fe
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    wheel = np.stack([np.asarray(sc["trajs"][j]["wheel_T"]) for j in rob])        # entry k: frames k -> k + 1
    x_pred = np.zeros((B, N, 15))
    for b in range(B):
        state = g.init_state()
        for k in range(N):
            dp, dq = g.motion(wheel[b, k])
            assert not g.drop(wheel[b, k]) and min(abs(dp / IP["p_motion_threshold"] - 1), abs(dq / IP["q_motion_threshold"] - 1)) >= 1e-3
            state = state.copy()
            state[0:6] = g.predict(state, wheel[b, k])
            x_pred[b, k] = state
    d_pred = float(np.abs(log[N - 2]["x_pred"].cpu().numpy()[:, :N - 1] - x_pred[:, :N - 1]).max())
    print("lock-step: predicted window states, device chain against the restatement's: max |difference| %.3e" % d_pred)
    for k in range(N):
        r, st = _frame(torch, sc, rob, k + 1)
        pts, times, n = fe.ranges_to_points(r, st)
        fe.spawn(k, pts, n, times=torch.where(n > 0, times[:, 0], st))
    x = _up(torch, x_pred.reshape(-1))
    xv = x.view(B, N, 15)
    pf = xv[:, 0, :6].contiguous()
    m = fe.match_front(0, 1, N - 1, pf, xv[:, 1:, :6])
    assert int(m["count"].min()) >= 4
    dev, Ltot, ok = fe.pack_init(m, N, pf)
    assert bool((ok == 1).all()) and Ltot == log[N - 1]["last_init"][2]
    ibs = liw.BatchSolver(sc["prm"], [liw.fleet.placeholder_init_window(N)], tile=dict(B=B, states=np.zeros((B, N, 15)), match_pose=np.zeros((B, N, 12))))
    iv = {key: _up(torch, np.stack([np.asarray(sc["trajs"][j][key])[1:N].reshape(-1) for j in rob]).reshape(-1)) for key in liw.fleet.INTERVAL_KEYS}
    ibs.rebind(dict(iv, x=x, **dev), Ltot)
    ibs.solve(liw.LIW_MODE_INIT)
    ibs.marginalize()
    fe.rebuild(0, N, xv, mask=ok)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    assert _its(ibs) == log[N - 1]["init_its"]
    assert torch.equal(x, log[N - 1]["x_init"].reshape(-1)), float((x - log[N - 1]["x_init"].reshape(-1)).abs().max())
    last = np.asarray([sc["trajs"][j]["imu_X"][N - 1][6:9] / sc["trajs"][j]["imu_Dt"][N - 1] for j in rob])
    rt.start(xv[:, N - 1], angular_local=last, prior={n: ibs.t[n] for n in ("prior_X", "prior_J", "prior_R", "has_prior")})
    torch.cuda.synchronize()
    a = log[N - 1]
    assert torch.equal(rt.x, a["x"]) and torch.equal(rt.track, a["track"])
    for n in ("prior_X", "prior_J", "prior_R", "has_prior"):
        assert torch.equal(rt.bs.t[n], a[n]), n
    for u, v in zip(_store_parts(fe, B), a["store"]):
        assert torch.equal(u, v)
    for k in range(N + 1, N + 4):
        r, st = _frame(torch, sc, rob, k)
        o = rt.step(r, st, _interval(torch, sc, rob, k))
        torch.cuda.synchronize()
        a = log[k - 1]
        assert o["Ltot"] == a["Ltot"] > 4 * B and _its(rt.bs) == a["its"], k
        for n in ("skip", "key", "flags", "pose"):
            assert torch.equal(o[n], a[n]), (k, n)
        assert torch.equal(rt.x, a["x"]) and torch.equal(rt.track, a["track"]), k
        for n in ("prior_X", "prior_J", "prior_R", "has_prior"):
            assert torch.equal(rt.bs.t[n], a[n]), (k, n)
        for u, v in zip(_store_parts(fe, B), a["store"]):
            assert torch.equal(u, v), k
    ft.close()
    rt.close()
    ibs.close()


def _staggered_frames(liw, sc, B, frames, one_wall=None, still=None, lag_of=None):
    """the inputs of a fleet whose robot b starts moving b % 4 frames late (until then its wheel increment is the identity and it sees
    its first scan); one_wall: a robot in front of a single wall; still: a robot that never moves.  Yields (t, ranges, stamps, interval)"""
    import torch
    rob = np.arange(B) % NB
    lag = np.arange(B) % 4
    for b, v in (lag_of or {}).items():
        lag[b] = v
    rest = {}
    for key in liw.fleet.INTERVAL_KEYS:   # a robot at rest: the first interval's pre-integration with an identity wheel increment
        a = np.stack([np.asarray(sc["trajs"][j][key])[0].reshape(-1) for j in rob])
        if key == "wheel_T":
            a = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (B, 1))
        rest[key] = a
    wall = np.full(N_RAYS, np.inf, dtype=np.float32)
    wall[500:580] = (1.5 / np.cos(ANG_INC * (np.arange(500, 580) - 540))).astype(np.float32)
    for t in range(1, frames + 1):
        kf = np.clip(t - lag, 0, sc["F"])                     # the trajectory frame robot b is at
        if still is not None:
            kf[still] = 0
        moving = kf >= 1
        rg = np.stack([sc["ranges"][rob[b], max(kf[b], 1)] for b in range(B)])
        if one_wall is not None:
            rg[one_wall] = wall
        stamps = np.array([sc["times"][rob[b], max(kf[b], 1)] for b in range(B)])
        iv = {}
        for key in liw.fleet.INTERVAL_KEYS:
            a = np.stack([np.asarray(sc["trajs"][rob[b]][key])[kf[b] - 1].reshape(-1) if moving[b] else rest[key][b] for b in range(B)])
            iv[key] = _up(torch, a)
        yield t, _up(torch, rg), _up(torch, stamps), iv


def _staggered_run(liw, sc, B, frames, one_wall=None, still=None, watch=None, lag_of=None, every_store=False):
    """FleetTrajectory over _staggered_frames -> (driver, per-frame log of cloned outputs and state)"""
    import torch
    ft = _trajectory(liw, sc, B)
    log = []
    for t, rg, stamps, iv in _staggered_frames(liw, sc, B, frames, one_wall, still, lag_of):
        before = None
        if watch is not None:
            before = _robot_bytes(ft, B, watch)
        o = ft.step(rg, stamps, iv)
        torch.cuda.synchronize()
        rec = {n: (v.clone() if torch.is_tensor(v) else v) for n, v in o.items() if n not in ("acc",)}
        if t == frames or every_store:   # the whole store once, at the end: every frame's effect on it is still in it or in what the frames returned
            rec.update(store=ft.fe.store.clone())
        rec.update(x=ft.x.clone(), init=ft.init.clone(), track=ft.track.clone(), its=_its(ft.bs), last_init=ft.last_init,
                   **{n: ft.bs.t[n].clone() for n in ("prior_X", "prior_J", "prior_R", "has_prior")})
        if watch is not None:
            rec.update(before=before, after=_robot_bytes(ft, B, watch))
        log.append(rec)
    return ft, log


def _robot_bytes(ft, B, b):
    rb = ft.fe.store.numel() // B
    d = dict(x=ft.x.view(B, 30)[b], init=ft.init.view(B, 256)[b], track=ft.track.view(B, 256)[b], store=ft.fe.store.view(B, rb)[b],
             **{n: ft.bs.t[n].view(B, -1)[b] for n in ("prior_X", "prior_J", "prior_R", "has_prior")},
             **{k: ft.win[k][b] for k in ft.win})
    return {k: v.clone() for k, v in d.items()}


def test_cold_start_mixed_states(liw, synth, cold):
    """24 robots, starts of motion staggered by 0 .. 3 frames, robot 5 in front of a single wall, robot 10 never moving, 10 frames:
    the drops, the frame a robot is initialised in, the failing robot's restart and the counters are the restatement's state machine;
    robots in different states share every frame; a dropped robot is byte-identical across its frame but for its counter."""
    import torch
    sc, B, N, T = cold, 24, NW, 10
    WALL, STILL, WATCH = 5, 10, 3   # robot 3 starts three frames late: dropped in frames 1 .. 3
    g = ref.InitGlue(liw, sc["tp"], sc["lp"]["T_imu_to_laser"], sc["lp"].get("normalize_extrinsics", True), IP)
    ft, log = _staggered_run(liw, sc, B, T, one_wall=WALL, still=STILL, watch=WATCH)
    rob, lag = np.arange(B) % NB, np.arange(B) % 4
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    assert g.drop(eye)
    n_frames, dropped, inits, failed = np.zeros(B, int), np.zeros(B, int), np.zeros(B, int), np.zeros(B, int)
    status = np.zeros(B, int)
    mixed = 0
    for t in range(1, T + 1):
        rec = log[t - 1]
        kf = np.clip(t - lag, 0, sc["F"])
        kf[STILL] = 0
        e_drop, e_ready = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
        was = status.copy()
        for b in range(B):
            if status[b] == ref.TRACKING:
                continue
            w = eye if kf[b] < 1 else np.asarray(sc["trajs"][rob[b]]["wheel_T"])[kf[b] - 1]
            if kf[b] >= 1:
                dp, dq = g.motion(w)
                assert min(abs(dp / IP["p_motion_threshold"] - 1), abs(dq / IP["q_motion_threshold"] - 1)) >= 1e-3
            if g.drop(w):
                e_drop[b] = 1
                dropped[b] += 1
                continue
            n_frames[b] += 1
            if n_frames[b] == N:
                e_ready[b] = 1
                if b == WALL:
                    failed[b] += 1
                    n_frames[b] = 0
                else:
                    inits[b] += 1
                    status[b] = ref.TRACKING
        ok = e_ready.copy()
        ok[WALL] = 0
        assert np.array_equal(rec["drop"].cpu().numpy(), e_drop), t
        assert np.array_equal(rec["ready"].cpu().numpy(), e_ready) and np.array_equal(rec["init_ok"].cpu().numpy(), ok), t
        assert np.array_equal(rec["status"].cpu().numpy(), status), t
        tracking = was == ref.TRACKING
        assert not rec["skip"].any() and not rec["key"].cpu().numpy()[~tracking].any() and not rec["flags"].cpu().numpy()[~tracking].any()
        if tracking.any():
            assert rec["Ltot"] >= 4 * int(tracking.sum()), t          # real matches for every robot that tracks
            assert all(rec["its"][b][0] >= 1 for b in np.nonzero(tracking)[0]), t
        if e_ready.any():
            R = int(e_ready.sum())
            assert rec["last_init"][1] == R and rec["last_init"][0] >= R and rec["last_init"][0] in (1, 2, 4, 8, 16, B), (t, rec["last_init"])
        mixed += int(tracking.any() and (~tracking).any())
        assert torch.isfinite(rec["x"]).all()
        if e_drop[WATCH]:   # a dropped robot: every byte as it was, but for the dropped counter (bytes 160 .. 163 of its record)
            for k, v in rec["before"].items():
                a = rec["after"][k]
                if k == "init":
                    a, v = a.clone(), v.clone()
                    a[160:164] = v[160:164]
                assert torch.equal(a, v), (t, k)
    assert mixed >= 3 and dropped[WATCH] == 3
    r = ref.unpack_records(ft.init.cpu().numpy(), B)
    assert np.array_equal(r["counters"], np.stack([inits, failed, dropped], 1)) and np.array_equal(r["n_frames"][status == 0], n_frames[status == 0])
    assert failed[WALL] >= 1 and status[WALL] == ref.INITIALIZING and status[STILL] == ref.INITIALIZING and dropped[STILL] == T
    regular = np.array([b for b in range(B) if b not in (WALL, STILL)])
    assert (status[regular] == ref.TRACKING).all()
    for b in regular[::5]:
        assert ft.fe.track_get(ft.track, int(b))["tracked"] == T - (lag[b] + N) >= 3
    ft.close()


def test_cold_start_against_host_glue(liw, synth, cold):
    """The same 24 robots (staggered starts, robot 5 in front of one wall, robot 10 at rest) through FleetTrajectory.step and through
    ref.HostGlueTrajectory: the stages that were there before, driven robot group by robot group from read-backs by the host
    restatement, with the INIT solve at the same bucket size.  Every decision, block offset, iteration count and termination equal in
    every frame; states, poses and priors within the project's 1e-6 bar.  The iteration counts and terminations of the tracking solve
    are compared for the robots that track (and those of the INIT solve for the R ready windows): the rows of the other robots are
    solved from whatever each side left in them and their results are thrown away, so their counts say nothing about either side.

    Measured on an MI355X: every decision equal; max relative difference solved windows 0, records 0, x 1.5e-11, poses 2.2e-12,
    prior_X 1.5e-11, prior_J 1.1e-10, prior_R 5.1e-8; fewest matches 11 (tracking) / 18 (window frame); the closest threshold
    quantity 16 % away from its threshold."""
    import torch
    sc, B, N, T = cold, 24, NW, 10
    WALL, STILL = 5, 10
    ft = _trajectory(liw, sc, B)
    ht = ref.HostGlueTrajectory(liw, sc["prm"], sc["lp"], sc["tp"], IP, _traj_dims(B))
    ht.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    worst, inits, mixed = {}, 0, 0

    def rel(name, a, h):
        if a.numel():
            assert torch.isfinite(a).all(), name
            worst[name] = max(worst.get(name, 0.0), float((a - h).abs().max() / h.abs().max().clamp_min(1e-300)))

    for t, rg, stamps, iv in _staggered_frames(liw, sc, B, T, WALL, STILL):
        o = ft.step(rg, stamps, iv)
        h = ht.step(rg, stamps, {k: v.clone() for k, v in iv.items()})
        torch.cuda.synchronize()
        for n in ("status", "drop", "ready", "init_ok", "skip", "key"):
            assert np.array_equal(o[n].cpu().numpy(), h[n]), (t, n)
        assert torch.equal(o["flags"], h["flags"]) and o["Ltot"] == h["Ltot"] and torch.equal(ft._bufs["laser_off"], h["laser_off"]), t
        trk, keep = h["tracking"], h["keep"]
        mixed += int(trk.any() and (~trk).any())
        its = _its(ft.bs)
        assert [its[b] for b in np.nonzero(trk)[0]] == [h["its"][b] for b in np.nonzero(trk)[0]], t
        assert h["last_init"] == (ft.last_init if h["ready"].any() else None), t
        if h["ready"].any():
            inits += 1
            assert _its(ft._init_bs[h["last_init"][0]])[:h["last_init"][1]] == h["init_its"], t
        now = _up(torch, np.nonzero(h["status"] == ref.TRACKING)[0])   # robots that track after this frame: committed ones included
        rel("x", ft.x.view(B, 30)[now], ht.x_d.view(B, 30)[now])
        rel("pose", o["pose"][_up(torch, np.nonzero(keep)[0])], _up(torch, h["pose"][keep]))
        for n in ("prior_X", "prior_J", "prior_R"):
            rel(n, ft.bs.t[n].view(B, -1)[now], ht.bs.t[n].view(B, -1)[now])
        assert torch.equal(ft.bs.t["has_prior"][now], ht.bs.t["has_prior"][now]), t
        ok = _up(torch, np.nonzero(h["init_ok"])[0])
        rel("x_init", ft.win["x_init"][ok], _up(torch, ht.x_init)[ok])
        r = ref.unpack_records(ft.init.cpu().numpy(), B)
        assert np.array_equal(r["counters"], ht.counters) and np.array_equal(r["n_frames"][h["status"] == 0], ht.n_frames[h["status"] == 0]), t
        rel("record", _up(torch, r["state"].copy()), _up(torch, ht.state))
    # the conditions that keep the comparison honest, on the reference side
    assert ht.min_track >= 4 and ht.min_front >= 4 and ht.margin >= 1e-3, (ht.min_track, ht.min_front, ht.margin)
    regular = np.array([b for b in range(B) if b not in (WALL, STILL)])
    assert (ht.status[regular] == ref.TRACKING).all() and (ht.tcount[regular, 0] >= 3).all() and ht.counters[WALL, 1] >= 1
    assert ht.status[WALL] == ht.status[STILL] == ref.INITIALIZING and ht.counters[STILL, 2] == T and mixed >= 3 and inits >= 4
    for b in regular[::5]:
        tg_ = ft.fe.track_get(ft.track, int(b))
        assert [tg_["tracked"], tg_["keys"], tg_["skipped"]] == [int(v) for v in ht.tcount[b]]
    print("cold start, %d robots x %d frames, device glue against host glue: max rel. difference %s; fewest matches %d (tracking) / %d (window); "
          "closest threshold quantity %.2e relative" % (B, T, ", ".join("%s %.2e" % kv for kv in worst.items()), ht.min_track, ht.min_front, ht.margin))
    assert max(worst.values()) <= 1e-6, worst
    ft.close()
    ht.close()


def test_isolation_of_tracking_robots(liw, synth, cold):
    """The staggered fleet of 24 twice: with robot 5 in front of a single wall (its windows fail, it never tracks), and with robot 5 a
    regular robot that moves from the first frame on, so that it is tracking before most of the fleet is.  Between the runs robot 5
    sits at another place of the INIT batches of frames 4 and 5 and adds its blocks to the tracking batch, so `laser_off` of the 18
    robots behind it differs in every frame it tracks.  Every other robot that tracks must not notice: its x rows, prior rows,
    tracking record and whole store region byte-identical between the runs in every frame from its commit on."""
    import torch
    sc, B, T, WALL, STILL = cold, 24, 10, 5, 10
    ft_a, a = _staggered_run(liw, sc, B, T, one_wall=WALL, still=STILL, every_store=True)
    ft_b, b = _staggered_run(liw, sc, B, T, still=STILL, lag_of={WALL: 0}, every_store=True)
    ft_a.close()
    ft_b.close()
    rb = a[0]["store"].numel() // B
    compared, shifted, worst = 0, 0, {}
    for t, (ra, rb_) in enumerate(zip(a, b), 1):
        sa, sb = ra["status"].cpu().numpy(), rb_["status"].cpu().numpy()
        others = np.array([r for r in range(B) if r != WALL])
        assert np.array_equal(sa[others], sb[others]), t
        for n in ("drop", "ready", "init_ok", "skip", "key", "flags"):
            assert torch.equal(ra[n][_up(torch, others)], rb_[n][_up(torch, others)]), (t, n)
        trk = others[sa[others] == ref.TRACKING]
        if not trk.size:
            continue
        shifted += int(sb[WALL] == ref.TRACKING and ra["Ltot"] != rb_["Ltot"])
        i = _up(torch, trk)
        parts = dict(x=(ra["x"].view(B, 30), rb_["x"].view(B, 30)), track=(ra["track"].view(B, 256), rb_["track"].view(B, 256)),
                     store=(ra["store"].view(B, rb), rb_["store"].view(B, rb)),
                     **{n: (ra[n].view(B, -1), rb_[n].view(B, -1)) for n in ("prior_X", "prior_J", "prior_R", "has_prior")})
        for n, (u, v) in parts.items():
            compared += 1
            if not torch.equal(u[i], v[i]) and u.dtype == torch.float64:
                worst[n] = max(worst.get(n, 0.0), float((u[i] - v[i]).abs().max() / v[i].abs().max().clamp_min(1e-300)))
            assert torch.equal(u[i], v[i]), (t, n, worst)
    assert compared >= 7 * 5 and shifted >= 4   # robot 5 tracked, and moved everybody's blocks, in at least four compared frames
    assert int((b[-1]["status"] == ref.TRACKING).sum()) == B - 1 and int((a[-1]["status"] == ref.TRACKING).sum()) == B - 2


def test_driver_deterministic_at_4096(liw, synth, cold):
    """4 096 robots x (N + 3) frames of the staggered fleet, twice: the store, both records, x, the priors and every decision bitwise
    identical"""
    import torch
    sc, B = cold, 4096
    runs = []
    for _ in range(2):
        ft, log = _staggered_run(liw, sc, B, NW + 3, one_wall=5, still=10)
        runs.append(log)
        ft.close()
    for t, (a, b) in enumerate(zip(*runs), 1):
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k].view(torch.uint8) if a[k].dtype != torch.bool else a[k], b[k].view(torch.uint8) if b[k].dtype != torch.bool else b[k]), (t, k)
            else:
                assert a[k] == b[k], (t, k)
    last = runs[0][-1]
    assert int((last["status"] == ref.TRACKING).sum()) > B // 2 and int((last["status"] == ref.INITIALIZING).sum()) >= 2
