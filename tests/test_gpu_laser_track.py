"""The tracking glue on the device (liw_lfe_track_init / _begin / _end, laser_batch.BatchFrontEnd.track_*, fleet.FleetTracker)
against the host restatement of lvio_2d::trajectory::add_sensor_data(laser) in tests/track_glue_reference.py: the kernels case by
case at two parameter sets, a fleet tracked free-running against the same stages with the glue on the host, the min_delta_t gate,
the key frame -> clear hand-over of the corner accumulator, determinism at 4 096 robots, and the argument checks.

Measured on an MI355X (pytest tests/test_gpu_laser_track.py -m gpu -s): see the "Fleet tracking frame" section of docs/WIDENING.md."""
import ctypes as C

import numpy as np
import pytest

import track_glue_reference as ref

pytestmark = pytest.mark.gpu

ANG_MIN, N_RAYS = np.float32(-2.0 * np.pi * 0.75 / 2), 1080
ANG_INC = np.float32(2.0 * np.pi * 0.75 / (N_RAYS - 1))
T_INC = np.float32(1.0 / (40.0 * N_RAYS))
# 1e-12 of max(1, |value|): at most four 3 x 3 products and one log_SO3 on quantities of order 10 come to tens of ulp, the device
# sin / cos / atan2 differ from glibc's by an ulp; the bar leaves two orders above that
BAR = 1e-12
CHAIN_BAR = 1e-6   # the project's bar for chained tracking frames (tests/test_gpu_laser_batch.py::test_end_to_end_track_batch)
G = 256            # guard elements on either side of every output
FILL, FILL_B = -7.25, 0xA5


def _T4(synth, pose):
    return synth.se3(synth.exp_so3(np.asarray(pose[3:6], dtype=np.float64)), np.asarray(pose[0:3], dtype=np.float64))


def _cast(liw, synth, lp, room, pose, seed):
    Til = synth.normalize_extrinsic(lp["T_imu_to_laser"])
    r, _, _ = liw.laser.cast_scan(liw.laser.room_segments(room), _T4(synth, pose) @ Til, n_rays=N_RAYS, seed=seed)
    return np.asarray(r, dtype=np.float32)


def _dims(B, **kw):
    return dict(dict(B=B, slots=1, max_points=N_RAYS, max_lines=256, max_cell_entries=8192), **kw)


def _guarded(torch, n, dtype, fill):
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    return buf, buf[G:G + n]


def _guards_ok(buf, fill):
    return bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())


def _record(track_view, B):
    """the tracking records as arrays: kf [B, 12], ang [B, 3], stamp [B], counters [B, 3]"""
    raw = track_view.cpu().numpy().copy()
    d, i = raw.view(np.float64).reshape(B, 32), raw.view(np.int32).reshape(B, 64)
    return dict(kf=d[:, 0:12], ang=d[:, 12:15], stamp=d[:, 15], counters=i[:, 32:35], raw=raw.reshape(B, 256))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("name", ["office", "second"])
def test_begin_end_against_restatement(liw, synth, name):
    """B = 130 (two full waves and a two-lane tail), room scans in slot 0, count a free input, strided state rows for track_init, five
    robots masked out; two pages of cases cover the generator's full cross product, and a third page (make_planar_cases) is the
    workload's own geometry, rotation about z only, with yaws at and next to +-pi/2, +-3 pi/4 and +-(pi - 2e-3).  "second" is the parameter set with a 0.48 rad
    turn and a lever arm in T_imu_to_wheel and a laser extrinsic off the office value (a transposed extrinsic would show:
    tests/test_laser_track_abi.py::test_transposed_extrinsics_would_show)."""
    import torch
    _, tp, lp = [s for s in ref.param_sets(liw, synth) if s[0] == name][0]
    g = ref.Glue(liw, tp, lp["T_imu_to_laser"], lp["normalize_extrinsics"])
    B = 130
    fe = liw.laser_batch.BatchFrontEnd(lp, _dims(B))
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    # the scan pool: an empty scan and room scans, one of them with an even number of lines
    rng = np.random.default_rng(5)
    cands = []
    for room in range(12):
        pose = np.concatenate([rng.uniform(-1.0, 1.0, 2), [0.0, 0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
        r = _cast(liw, synth, lp, 3000 + room, pose, seed=room)
        nl = liw.laser.Scan.spawn(lp, liw.laser.laser_to_points(r, ANG_MIN, ANG_INC, T_INC, 0.0)[0]).lines().shape[0]
        if nl >= 4:
            cands.append((r, nl))
    even = [cd for cd in cands if cd[1] % 2 == 0][:1]
    assert even, [cd[1] for cd in cands]
    chosen = even + [cd for cd in cands if cd is not even[0]][:2]
    pool = [np.full(N_RAYS, np.inf, dtype=np.float32)] + [cd[0] for cd in chosen]
    lines = [0] + [cd[1] for cd in chosen]
    masked = np.array([3, 64, 65, 127, 129])
    mask = np.ones(B, dtype=np.uint8)
    mask[masked] = 0
    worst = dict(linear=0.0, angular=0.0, pose_new=0.0, kf=0.0, ang=0.0)
    combos = set()
    for page in range(3):   # two pages of random axes, then the planar page: yaws at and next to +-pi/2, +-3 pi/4, +-(pi - 2e-3)
        c = (ref.make_cases if page < 2 else ref.make_planar_cases)(g, synth, B, lines, seed=40 + page, page=page)
        combos.update(tuple(int(v) for v in row) for row in c["combo"])
        e = ref.expected(g, c, lines, mask=mask)
        for b in np.nonzero(mask)[0]:   # the cases keep their distance from the thresholds at this parameter set too
            for value, thr in ((c["imu_Dt"][b], tp["min_delta_t"]), (e["dp"][b], tp["key_frame_p_motion_threshold"]), (e["dq"][b], tp["key_frame_q_motion_threshold"])):
                assert abs(value - thr) >= 1e-3 * thr, (b, value, thr)
        st = torch.from_numpy(c["stamps"]).cuda()
        pts, times, n = fe.ranges_to_points(torch.from_numpy(np.stack([pool[s] for s in c["scan"]])).cuda(), st)
        fe.spawn(0, pts, n)
        torch.cuda.synchronize()
        for s in set(int(v) for v in c["scan"]):
            b = int(np.nonzero(c["scan"] == s)[0][0])
            assert fe.num_lines(b, 0) == lines[s], (s, fe.num_lines(b, 0), lines[s])
        store0 = fe.store.clone()
        tbuf, track = _guarded(torch, fe.track_layout(), torch.uint8, FILL_B)
        xbuf, x = _guarded(torch, B * 30, torch.float64, FILL)
        x.copy_(torch.from_numpy(c["x"].reshape(-1)).cuda())
        kfx = torch.full((B, 2, 15), FILL, dtype=torch.float64, device="cuda")
        kfx[:, 1, 0:6] = torch.from_numpy(c["kf_pose"]).cuda()
        fe.track_init(tp, track, kfx[:, 1], c["angular_local"], mask=mask)   # rows 30 doubles apart
        rec0 = _record(track, B)
        outs = {k: _guarded(torch, B * w, dt, f) for k, w, dt, f in (("linear", 3, torch.float64, FILL), ("angular", 3, torch.float64, FILL),
                                                                    ("pose_new", 6, torch.float64, FILL), ("skip", 1, torch.uint8, FILL_B))}
        fe.track_begin(tp, track, x, c["imu_X"], c["imu_Dt"], c["wheel_T"], c["stamps"], mask=mask, out={k: v[1] for k, v in outs.items()})
        torch.cuda.synchronize()
        rec1 = _record(track, B)
        xs = x.cpu().numpy().reshape(B, 2, 15)
        o = {k: v[1].cpu().numpy().reshape(B, -1) for k, v in outs.items()}
        on = mask.astype(bool)
        skipped = on & (e["skip"] == 1)
        went = on & (e["skip"] == 0)
        assert skipped.sum() > 20 and went.sum() > 20
        assert np.array_equal(o["skip"][on, 0], e["skip"][on])
        for k in ("linear", "angular"):
            worst[k] = max(worst[k], _rel(o[k][on], e[k][on]))
        worst["pose_new"] = max(worst["pose_new"], _rel(o["pose_new"][went], e["pose_new"][went]), _rel(xs[went, 1, 0:6], e["x"][went, 1, 0:6]))
        assert np.array_equal(o["pose_new"][went], xs[went, 1, 0:6])
        # the rolled row and the carried v, ba, bw: bitwise
        assert np.array_equal(xs[went, 0].view(np.int64), c["x"][went, 1].view(np.int64))
        assert np.array_equal(xs[went, 1, 6:15].view(np.int64), c["x"][went, 1, 6:15].view(np.int64))
        # masked and skipped robots: x byte for byte, no output row of a masked robot, no pose_new of a skipped one
        for sel in (~on, skipped):
            assert np.array_equal(xs[sel].view(np.int64), c["x"][sel].view(np.int64))
            assert (o["pose_new"][sel] == FILL).all()
        for k in ("linear", "angular"):
            assert (o[k][~on] == FILL).all()
        assert (o["skip"][~on] == FILL_B).all()
        assert (rec1["raw"][~on] == FILL_B).all() and (rec0["raw"][~on] == FILL_B).all()
        # a skipped robot's record: only the skipped counter moved
        a, z = rec1["raw"][skipped].copy(), rec0["raw"][skipped].copy()
        assert np.array_equal(rec1["counters"][skipped], np.array([[0, 0, 1]] * int(skipped.sum())))
        a[:, 128 + 8:128 + 12] = z[:, 128 + 8:128 + 12]
        assert np.array_equal(a, z)
        worst["ang"] = max(worst["ang"], _rel(rec1["ang"][on], e["ang"][on]))
        assert np.array_equal(rec1["stamp"][on], e["stamp"][on])
        # ---- track_end on the x that track_begin left, count free, the same five robots masked out
        eo = dict(key=_guarded(torch, B, torch.uint8, FILL_B), pose=_guarded(torch, B * 6, torch.float64, FILL))
        x_before = x.clone()
        fe.track_end(tp, track, 0, x, torch.from_numpy(c["count"]).cuda(), mask=mask, out={k: v[1] for k, v in eo.items()})
        torch.cuda.synchronize()
        rec2 = _record(track, B)
        key, pose = eo["key"][1].cpu().numpy(), eo["pose"][1].cpu().numpy().reshape(B, 6)
        assert np.array_equal(key[on], e["key"][on])
        assert 10 < int(key[on].sum()) < int(on.sum()) - 10
        assert (key[~on] == FILL_B).all() and (pose[~on] == FILL).all()
        assert np.array_equal(pose[on], xs[on, 1, 0:6])
        assert torch.equal(x, x_before) and torch.equal(fe.store, store0)
        worst["kf"] = max(worst["kf"], _rel(rec2["kf"][on], e["kf"][on]))
        assert np.array_equal(rec2["counters"][on], e["counters"][on])
        assert np.array_equal(rec2["ang"][on].view(np.int64), rec1["ang"][on].view(np.int64)) and np.array_equal(rec2["stamp"][on], rec1["stamp"][on])
        assert (rec2["raw"][~on] == FILL_B).all()
        stay = on & (e["key"] == 0)
        assert np.array_equal(rec2["kf"][stay].view(np.int64), rec1["kf"][stay].view(np.int64))
        # the synchronous getter reads the same record
        for b in (0, 128):
            t = fe.track_get(track, b)
            assert np.array_equal(t["last_keyframe_tf"], rec2["kf"][b]) and np.array_equal(t["angular_local"], rec2["ang"][b])
            assert t["stamp"] == rec2["stamp"][b] and [t["tracked"], t["keys"], t["skipped"]] == list(rec2["counters"][b])
        for buf, fill in [(tbuf, FILL_B), (xbuf, FILL)] + [(v[0], FILL_B if v[0].dtype == torch.uint8 else FILL) for v in list(outs.values()) + list(eo.values())]:
            assert _guards_ok(buf, fill)
    assert len(combos) == ref.N_COMBOS
    print("track_begin / track_end, %s set, 3 x %d robots: worst |device - restatement| / max(1, |value|): %s"
          % (name, B, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= BAR, (k, v)
    fe.close()


# ------------------------------------------------------------------------------------------------------------ the fleet scenes
@pytest.fixture(scope="module")
def scene(liw, synth):
    """8 trajectories x 6 frames after the start frame: truth states, the intervals' pre-integrations, scans cast from the truth"""
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)   # the reference sub-map exists at every frame
    tp = dict(liw.laser_batch.office_track_params(prm), key_frame_p_motion_threshold=0.25)   # 0.15 m a frame: not every frame is a key frame
    nb, F = 8, 6
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=F + 1, L=0) for j in range(nb)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(F + 1, 15) for t in trajs])
    ranges = np.stack([[_cast(liw, synth, lp, 3000 + j, truth[j, k, 0:6], seed=j * 10 + k) for k in range(F + 1)] for j in range(nb)])
    return dict(prm=prm, lp=lp, tp=tp, nb=nb, F=F, trajs=trajs, truth=truth, ranges=ranges, times=np.stack([t["times"] for t in trajs]))


def _interval(torch, sc, rob, k, dt_of=None):
    """the six interval tensors of frame k (the interval k - 1 -> k) for the robots `rob` (indices into the trajectories)"""
    iv = {}
    for key in liw_keys():
        a = np.stack([np.asarray(sc["trajs"][j][key])[k - 1].reshape(-1) for j in rob])
        if key == "imu_Dt" and dt_of is not None:
            a = a.copy()
            for b, v in dt_of.items():
                a[b] = v
        iv[key] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return iv


def liw_keys():
    return ("imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP")


def _seed(torch, sc, fe, rob):
    """the first scan at the truth pose as the sub-map tracking starts from"""
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    st = torch.from_numpy(sc["times"][rob, 0]).cuda()
    pts, times, n = fe.ranges_to_points(torch.from_numpy(sc["ranges"][rob, 0]).cuda(), st)
    fe.spawn(0, pts, n)
    fe.add_scan(0, sc["truth"][rob, 0, 0:6])


def _frame(torch, sc, rob, k):
    return torch.from_numpy(sc["ranges"][rob, k]).cuda(), torch.from_numpy(sc["times"][rob, k]).cuda()


def _fleet(liw, sc, B, **kw):
    return liw.FleetTracker(sc["prm"], sc["lp"], sc["tp"], _dims(B), **kw)


def _mrel(a, h):
    return float((a - h).abs().max() / h.abs().max().clamp_min(1e-300))


# --------------------------------------------------------------------------------------------------------------------- 3
def test_free_running_against_host_glue(liw, synth, scene):
    """64 robots tiled from 8 trajectories x 4 frames: FleetTracker.step against a second front-end / solver pair on the same device
    whose glue is the host restatement fed from read-backs, so the glue is the only difference.

    Measured on an MI355X: every decision, count and termination equal, and states, priors, poses and corners bit-identical in all four
    frames (difference 0).  k_lfe_track_begin evaluates its sin / cos / atan2 correctly rounded (csrc/liw_crmath.hpp), which is what
    glibc returns for all but about 0.1 % of the arguments.  With the device library's functions instead the twist and the predicted
    pose differed from the host's in the last bit from frame 2 on, and the free-running solves amplified that to 3.5e-8 in the states
    and 2.4e-6 in prior_R (the near-zero residual of the marginalised prior) after frame 4, above the bar."""
    import torch
    sc, B, F = scene, 64, 4
    rob = np.arange(B) % sc["nb"]
    ft = _fleet(liw, sc, B)
    ht = ref.HostGlueTracker(liw, sc["prm"], sc["lp"], sc["tp"], _dims(B))
    for fe in (ft.fe, ht.fe):
        _seed(torch, sc, fe, rob)
    x0 = sc["truth"][rob, 0]
    ft.start(x0)
    ht.start(x0)
    per, keys = {}, 0
    for k in range(1, F + 1):
        r, st = _frame(torch, sc, rob, k)
        iv = _interval(torch, sc, rob, k)
        o = ft.step(r, st, iv)
        h = ht.step(r, st, {kk: v.clone() for kk, v in iv.items()})
        torch.cuda.synchronize()
        assert int(h["count"].min()) >= 4, (k, h["count"])   # the reference loop tracks on real matches
        assert o["Ltot"] == h["Ltot"] > 0
        assert np.array_equal(o["skip"].cpu().numpy(), h["skip"]) and not h["skip"].any()
        assert np.array_equal(o["key"].cpu().numpy(), h["key"]), k
        assert torch.equal(o["flags"], h["flags"]), k
        assert torch.equal(ft._bufs["laser_off"], h["laser_off"]), k
        assert torch.equal(o["n_acc"], h["n_acc"]), k
        keys += int(h["key"].sum())
        sa, sh = ft.bs.summaries(), ht.bs.summaries()
        assert [(s["iterations"], s["termination"]) for s in sa] == [(s["iterations"], s["termination"]) for s in sh], k
        pairs = dict(x=(ft.x, ht.x_d), pose=(o["pose"], torch.from_numpy(h["pose"]).cuda()), **{n: (ft.bs.t[n], ht.bs.t[n]) for n in ("prior_X", "prior_J", "prior_R")})
        assert torch.equal(ft.bs.t["has_prior"], ht.bs.t["has_prior"])
        na = int(h["n_acc"].min())
        if na > 0:
            pairs["acc"] = (o["acc"][:, :na], h["acc"][:, :na])
        for n, (a, b) in pairs.items():
            assert torch.isfinite(a).all(), (k, n)
            per[n] = max(per.get(n, 0.0), _mrel(a, b))
        jtj = [t.view(B, 15, 15).transpose(1, 2) @ t.view(B, 15, 15) for t in pairs["prior_J"]]
        print("  frame %d: max rel. difference so far %s; this frame's prior J^T J %.2e" % (k, ", ".join("%s %.2e" % kv for kv in per.items()), _mrel(*jtj)))
    worst = max(per.values())
    for b in range(0, B, 9):
        t = ft.fe.track_get(ft.track, b)
        assert [t["tracked"], t["keys"], t["skipped"]] == [int(v) for v in ht.counters[b]]
        assert _rel(t["last_keyframe_tf"], ht.kf[b]) <= CHAIN_BAR
    print("free-running fleet, %d robots x %d frames, device glue against host glue: states / priors / poses / corners max rel. difference %.3e, "
          "%d key frames of %d" % (B, F, worst, keys, B * F))
    assert worst <= CHAIN_BAR
    ft.close()


# --------------------------------------------------------------------------------------------------------------------- 4
def test_gate_leaves_a_skipped_robot_untouched(liw, synth, scene):
    """robot 5 of 16 gets an imu_Dt below min_delta_t in frame 2: it is byte-identical across that step apart from its skip counter,
    and the other robots do what they do in a run without it (decisions equal; states to the chained-frame bar, since the laser
    blocks of the robots behind it move in the batch's arrays and the sums regroup)."""
    import torch
    sc, B, r5 = scene, 16, 5
    rob = np.arange(B) % sc["nb"]
    runs = []
    for gate in (False, True):
        ft = _fleet(liw, sc, B)
        _seed(torch, sc, ft.fe, rob)
        ft.start(sc["truth"][rob, 0])
        out = None
        for k in (1, 2):
            r, st = _frame(torch, sc, rob, k)
            iv = _interval(torch, sc, rob, k, dt_of={r5: 0.5 * sc["tp"]["min_delta_t"]} if (gate and k == 2) else None)
            if gate and k == 2:
                rb = ft.fe.store.numel() // B
                before = dict(x=ft.x.view(B, 30)[r5].clone(), track=ft.track.view(B, 256)[r5].clone(), store=ft.fe.store.view(B, rb)[r5].clone(),
                              acc=ft.acc[r5].clone(), n_acc=ft.n_acc[r5].clone(), **{n: ft.bs.t[n].view(B, -1)[r5].clone() for n in ("prior_X", "prior_J", "prior_R", "has_prior")})
            out = {kk: (v.clone() if torch.is_tensor(v) else v) for kk, v in ft.step(r, st, iv).items()}
        torch.cuda.synchronize()
        runs.append((ft, out))
    (fa, oa), (fb, ob) = runs
    rb = fb.fe.store.numel() // B
    after = dict(x=fb.x.view(B, 30)[r5], track=fb.track.view(B, 256)[r5], store=fb.fe.store.view(B, rb)[r5], acc=fb.acc[r5], n_acc=fb.n_acc[r5],
                 **{n: fb.bs.t[n].view(B, -1)[r5] for n in ("prior_X", "prior_J", "prior_R", "has_prior")})
    for n, v in after.items():
        if n == "track":
            a, z = v.cpu().numpy().copy(), before[n].cpu().numpy()
            assert a.view(np.int32)[34] == z.view(np.int32)[34] + 1 == 1      # the skip counter
            a.view(np.int32)[34] = z.view(np.int32)[34]
            assert np.array_equal(a, z)
        else:
            assert v.cpu().numpy().tobytes() == before[n].cpu().numpy().tobytes(), n
    skip = ob["skip"].cpu().numpy()
    assert skip[r5] == 1 and skip.sum() == 1 and ob["key"][r5] == 0 and ob["flags"][r5] == 0
    others = torch.from_numpy(np.arange(B) != r5).cuda()
    for n in ("key", "flags", "n_acc"):
        assert torch.equal(oa[n][others], ob[n][others]), n
    worst = max(_mrel(fb.x.view(B, 30)[others], fa.x.view(B, 30)[others]), _mrel(ob["pose"][others], oa["pose"][others]),
                _mrel(fb.bs.t["prior_J"].view(B, -1)[others], fa.bs.t["prior_J"].view(B, -1)[others]))
    print("gate: robot %d skipped in frame 2, byte-identical; the other %d robots against the run without the skip: max rel. difference %.3e" % (r5, B - 1, worst))
    assert worst <= CHAIN_BAR
    for ft, _ in runs:
        ft.close()


# --------------------------------------------------------------------------------------------------------------------- 5
def test_key_frame_hands_its_corners_over(liw, synth, scene):
    """6 frames x 8 robots: n_acc restarts in the frame after a key frame and holds the key frame's own corners at the key frame; the
    key decisions, last_keyframe_tf and the counters follow the restatement fed with the frame's read-backs."""
    import torch
    sc, B, F = scene, 8, 6
    rob = np.arange(B)
    g = ref.Glue(liw, sc["tp"], sc["lp"]["T_imu_to_laser"], sc["lp"]["normalize_extrinsics"])
    ft = _fleet(liw, sc, B)
    _seed(torch, sc, ft.fe, rob)
    x0 = sc["truth"][rob, 0]
    ft.start(x0)
    kf = np.stack([g.lie.make_tf(x0[b, 0:3], x0[b, 3:6]) for b in range(B)])
    n_exp, prev_key, counters = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool), np.zeros((B, 3), dtype=np.int64)
    restarts = 0
    for k in range(1, F + 1):
        r, st = _frame(torch, sc, rob, k)
        o = ft.step(r, st, _interval(torch, sc, rob, k))
        torch.cuda.synchronize()
        pose, key, n_acc = o["pose"].cpu().numpy(), o["key"].cpu().numpy(), o["n_acc"].cpu().numpy()
        count, n_corn = ft._m["count"].cpu().numpy(), ft._corners[1].cpu().numpy()
        for b in range(B):
            kb = g.key(kf[b], pose[b], count[b], ft.fe.num_lines(b, 0))
            assert int(key[b]) == int(kb), (k, b)
            counters[b, 0] += 1
            if kb:
                counters[b, 1] += 1
                kf[b] = g.tf_w_l(pose[b])
            if prev_key[b]:
                n_exp[b] = 0
                restarts += 1
            n_exp[b] += n_corn[b]
            t = ft.fe.track_get(ft.track, b)
            assert [t["tracked"], t["keys"], t["skipped"]] == list(counters[b])
            assert _rel(t["last_keyframe_tf"], kf[b]) <= BAR
        assert np.array_equal(n_acc, n_exp), (k, n_acc, n_exp)
        prev_key = key.astype(bool)
    assert restarts > 0 and int(n_corn.sum()) > 0
    print("key -> clear: %d robots x %d frames, %d key frames, %d restarts of the corner accumulator" % (B, F, int(counters[:, 1].sum()), restarts))
    ft.close()


# --------------------------------------------------------------------------------------------------------------------- 6
def test_determinism_at_4096(liw, synth, scene):
    import torch
    sc, B = scene, 4096
    rob = np.arange(B) % sc["nb"]
    ft = _fleet(liw, sc, B)
    frames = [(_frame(torch, sc, rob, k), _interval(torch, sc, rob, k)) for k in (1, 2, 3)]

    def run():
        ft.fe.reset()
        _seed(torch, sc, ft.fe, rob)
        ft.start(sc["truth"][rob, 0])
        outs = []
        for (r, st), iv in frames:
            o = ft.step(r, st, iv)
            outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
        torch.cuda.synchronize()
        return ft.fe.store.clone(), ft.track.clone(), ft.x.clone(), outs

    s1, t1, x1, o1 = run()
    s2, t2, x2, o2 = run()
    assert torch.equal(s1, s2) and torch.equal(t1, t2) and torch.equal(x1.view(torch.int64), x2.view(torch.int64))
    for a, b in zip(o1, o2):
        assert a["Ltot"] == b["Ltot"] > 0
        for k in ("skip", "key", "flags", "n_acc"):
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(a["pose"].view(torch.int64), b["pose"].view(torch.int64))
        # the accumulator is defined up to n_acc (start() empties it by n_acc = 0; what lies behind is an earlier run's)
        held = torch.arange(a["acc"].shape[1], device="cuda")[None, :] < a["n_acc"][:, None]
        assert int(held.sum()) > 0 and torch.equal(a["acc"].view(torch.int64)[held], b["acc"].view(torch.int64)[held])
    assert int(o1[-1]["flags"].ne(0).sum()) > 0
    ft.close()


# --------------------------------------------------------------------------------------------------------------------- 7
def test_einval_leaves_everything_untouched(liw, synth):
    import torch
    lb = liw.laser_batch
    B = 6
    fe = lb.BatchFrontEnd(liw.laser.office_laser_params(), _dims(B, slots=2))
    L, h = fe.L, fe.h
    tps = lb.track_params_struct(lb.office_track_params())
    tp = C.byref(tps)
    mk = lambda n, dt, f: torch.full((n,), f, dtype=dt, device="cuda")
    track, x = mk(fe.track_layout(), torch.uint8, FILL_B), mk(B * 30, torch.float64, 0.25)
    dbl, byt, cnt = mk(B * 15, torch.float64, FILL), mk(B, torch.uint8, FILL_B), torch.zeros(B, dtype=torch.int32, device="cuda")
    outs = [mk(B * 6, torch.float64, FILL) for _ in range(3)]
    everything = [track, x, dbl, byt, cnt, fe.store] + outs
    before = [t.clone() for t in everything]
    p = lambda t: C.c_void_p(t.data_ptr())
    E = -22
    # track_init: null tp / track / x, non-positive stride
    good = [h, tp, p(track), p(x), 30, p(dbl), None, None]
    for i, bad in ((1, None), (2, None), (3, None), (4, 0), (4, -30)):
        a = list(good)
        a[i] = bad
        assert L.liw_lfe_track_init(*a) == E, ("init", i)
    # track_begin: every array but mask
    good = [h, tp, p(track), p(x), p(dbl), p(dbl), p(dbl), p(dbl), None, p(outs[0]), p(outs[1]), p(outs[2]), p(byt), None]
    for i in (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12):
        a = list(good)
        a[i] = None
        assert L.liw_lfe_track_begin(*a) == E, ("begin", i)
    # track_end: every array but mask, slot outside 0 .. slots-1 (the sub-map selectors included)
    good = [h, tp, p(track), p(fe.store), 0, p(x), p(cnt), None, p(byt), p(outs[0]), None]
    for i in (1, 2, 3, 5, 6, 8, 9):
        a = list(good)
        a[i] = None
        assert L.liw_lfe_track_end(*a) == E, ("end", i)
    for slot in (-1, -2, 2, 7):
        a = list(good)
        a[4] = slot
        assert L.liw_lfe_track_end(*a) == E, ("end slot", slot)
    # track_get: null track, robot outside 0 .. B-1
    out = np.full(16, FILL)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    for tr, robot in ((None, 0), (p(track), -1), (p(track), B)):
        assert L.liw_lfe_track_get(h, tr, robot, dp, dp, dp, None) == E
    assert (out == FILL).all()
    torch.cuda.synchronize()
    for t, b in zip(everything, before):
        assert torch.equal(t, b)
    fe.close()
