"""Fleet initialisation on the device (liw_lfe_match_front / liw_lfe_pack_init / liw_lfe_rebuild, laser_batch.BatchFrontEnd):
the wave-per-(robot, frame) match kernel against the lane-per-robot kernel bit for bit, against the host front-end's
match_with_front, the INIT-window pack against a numpy pack of the same device matches, the sub-map rebuild against the host
manager, scans -> INIT solve -> rebuild -> one tracking frame against the same solver fed by the host front-end, argument checks.
References: the lane kernel (liw_lfe_match), liw.laser and numpy; never the new code's own output."""
import numpy as np
import pytest

from test_gpu_laser_batch import ANG_INC, ANG_MIN, N_RAYS, T_INC, Scene, _compare_lines, _compare_match, _fe, _pose
from test_gpu_laser_spawn_wave import zigzag_segments

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
KEYS = ("count", "recs", "idx1", "idx2", "match_pose")
# robots of the base scenario that are built to fail the initialisation (or to stress the kernel)
R_EMPTY_FRONT, R_EMPTY_FRAME, R_ONE_WALL, R_ZIGZAG, R_INVALID = 0, 1, 2, 3, 4
B0, F0 = 37, 5


@pytest.fixture(scope="module")
def env(liw):
    import torch
    lp = liw.laser.office_laser_params()
    return liw, lp, Scene(liw, lp), torch


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _zigzag(liw, seed):
    r, _, _ = liw.laser.cast_scan(zigzag_segments(), np.eye(4), n_rays=N_RAYS, seed=seed)
    return liw.laser.laser_to_points(r, ANG_MIN, ANG_INC, T_INC, 0.0)[0]


def _scenario(env, dp, dq, seed):
    """37 robots x (front + 5 frames): rooms seen from poses within dp / dq of the front pose, and by construction an empty front
    scan (robot 0), an empty frame scan (robot 1, frame 1), a one-wall frame scan (robot 2, frame 0), the zig-zag ring against
    itself (robot 3: more than 64 lines per scan), a frame slot made invalid at spawn (robot 4, frame 1).  The special frames are
    frames 0 / 1 so that a window of the first two frames still holds them.  -> dict of host arrays"""
    liw, lp, sc, torch = env
    rng = np.random.default_rng(seed)
    pf = np.stack([_pose(rng) for _ in range(B0)])
    poses = np.stack([[_pose(rng, pf[b], dp, dq) for _ in range(F0)] for b in range(B0)])
    lists = [[sc.points(b, pf[b], seed=10 * b)[0]] + [sc.points(b, poses[b, k], seed=10 * b + 1 + k)[0] for k in range(F0)] for b in range(B0)]
    lists[R_EMPTY_FRONT][0] = np.zeros((0, 3))
    lists[R_EMPTY_FRAME][2] = np.zeros((0, 3))
    lists[R_ONE_WALL][1] = np.stack([np.linspace(-0.5, 0.5, 40), np.full(40, 1.5) + rng.normal(0, 0.002, 40), np.zeros(40)], 1)
    for k in range(F0 + 1):
        lists[R_ZIGZAG][k] = _zigzag(liw, 5 + k)
    for k in range(F0):   # the ring is cast at the laser origin every time: the estimated poses differ a little, so the distances are real
        poses[R_ZIGZAG, k] = _pose(rng, pf[R_ZIGZAG], 0.02, np.deg2rad(0.5))
    P, n = [], []
    for s in range(F0 + 1):
        Ps, ns = liw.laser_batch.pad_points([lists[b][s] for b in range(B0)], N_RAYS)
        P.append(Ps)
        n.append(ns)
    n[2][R_INVALID] = N_RAYS + 1
    return dict(pf=pf, poses=poses, lists=lists, P=P, n=n)


@pytest.fixture(scope="module")
def base(env):
    """pose perturbations as in test_gpu_laser_batch.test_match: 0.3 m, 10 degrees"""
    return _scenario(env, 0.3, np.deg2rad(10), 4100)


@pytest.fixture(scope="module")
def gentle(env):
    """0.1 m, 3 degrees: every robot that is not built to fail keeps at least two pairs in every frame (the host front-end's
    do_match says so for this seed), so init_ok separates exactly the robots built to fail"""
    return _scenario(env, 0.1, np.deg2rad(3), 4300)


def _spawned(env, base, B, slots, rob=None):
    """a front-end with the base scenario's scans in slots 0 .. slots-1 (robot b = base robot rob[b])"""
    liw, lp, sc, torch = env
    fe = _fe(liw, lp, B, slots=slots)
    for s in range(slots):
        P, n = (base["P"][s], base["n"][s]) if rob is None else (base["P"][s][rob], base["n"][s][rob])
        fe.spawn(s, torch.from_numpy(np.ascontiguousarray(P)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda())
    return fe


def _lane_reference(fe, F, pf, poses, kk, cap, first=1):
    """F calls of the lane-per-robot kernel, stacked to the task layout of match_front"""
    o = [_np(fe.match(0, first + k, pf, poses[:, k], kk=kk, cap=cap)) for k in range(F)]
    return {key: np.stack([o[k][key] for k in range(F)], 1) for key in KEYS}


def _assert_same_match(w, l, what):
    assert np.array_equal(w["count"], l["count"]), what
    assert np.array_equal(w["match_pose"], l["match_pose"]), what
    B, F = w["count"].shape
    for b in range(B):
        for k in range(F):
            c = int(l["count"][b, k])
            for key in ("recs", "idx1", "idx2"):
                assert np.array_equal(w[key][b, k, :c], l[key][b, k, :c]), (what, key, b, k)


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kk", [0, 1])
def test_wave_kernel_equals_lane_kernel(env, base, kk):
    liw, lp, sc, torch = env
    lb = liw.laser_batch
    pf, poses = base["pf"], base["poses"]
    few, fel = _spawned(env, base, B0, F0 + 1), _spawned(env, base, B0, F0 + 1)
    assert few.num_lines(R_ZIGZAG, 0) > 64 and few.num_lines(R_ZIGZAG, 1) > 64
    assert few.status(R_INVALID, 2) & lb.ST_POINTS
    l = _lane_reference(fel, F0, pf, poses, kk, 256)
    w = _np(few.match_front(0, 1, F0, pf, poses, kk=kk, cap=256))
    _assert_same_match(w, l, ("cap 256", kk))
    torch.cuda.synchronize()
    assert torch.equal(few.store, fel.store)                       # every status word (robot and slot) and nothing else moved
    cnt = l["count"]
    print("match_front kk=%d: %d pairs over %d tasks; zig-zag counts %s" % (kk, int(cnt.sum()), cnt.size, cnt[R_ZIGZAG].tolist()))
    assert int(cnt.sum()) > 4 * B0 * F0
    assert (cnt[R_EMPTY_FRONT] == 0).all() and cnt[R_EMPTY_FRAME, 1] == 0 and cnt[R_ONE_WALL, 0] < 2 and cnt[R_INVALID, 1] == 0
    assert few.status(R_INVALID) & lb.ST_INVALID and not few.status(R_EMPTY_FRAME) and not few.status(R_EMPTY_FRONT)
    zz = int(np.argmax(cnt[R_ZIGZAG]))
    assert l["idx2"][R_ZIGZAG, zz, :cnt[R_ZIGZAG, zz]].max() >= 64   # the ordered write goes on past the first 64-line chunk
    # cap = the largest pair count (it fits) and one below it (overflow: count 0 and ST_MATCH for that robot only)
    cmax = int(cnt.max())
    owners = sorted(set(np.nonzero(cnt == cmax)[0].tolist()))
    assert owners == [R_ZIGZAG]
    for cap, over in ((cmax, False), (cmax - 1, True)):
        few, fel = _spawned(env, base, B0, F0 + 1), _spawned(env, base, B0, F0 + 1)
        lc = _lane_reference(fel, F0, pf, poses, kk, cap)
        wc = _np(few.match_front(0, 1, F0, pf, poses, kk=kk, cap=cap))
        _assert_same_match(wc, lc, ("cap", cap, kk))
        torch.cuda.synchronize()
        assert torch.equal(few.store, fel.store)
        flagged = [b for b in range(B0) if few.status(b) & lb.ST_MATCH]
        assert flagged == (owners if over else []), (cap, flagged)
        hit = cnt == cmax
        assert np.array_equal(wc["count"], np.where(hit, 0, cnt) if over else cnt)
    # F = 1 is a single match call
    w1 = _np(few.match_front(0, 3, 1, pf, poses[:, 2:3], kk=kk, cap=256))
    l1 = _np(fel.match(0, 3, pf, poses[:, 2], kk=kk, cap=256))
    _assert_same_match(w1, {key: l1[key][:, None] for key in KEYS}, ("F = 1", kk))
    # poses read out of a states array x [B, n, 15] through its strides
    n = F0 + 1
    x = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (B0, n, 15))).cuda()
    x[:, 0, :6] = torch.from_numpy(pf).cuda()
    x[:, 1:, :6] = torch.from_numpy(poses).cuda()
    view = x[:, 1:, :6]
    assert view.stride() == (15 * n, 15, 1) and not view.is_contiguous()
    ws = _np(few.match_front(0, 1, F0, pf, view, kk=kk, cap=256))
    _assert_same_match(ws, l, ("strided", kk))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_match_front_equals_host_front_end(env):
    liw, lp, sc, torch = env
    B, n = 16, 6
    rng = np.random.default_rng(4200)
    pf = np.stack([_pose(rng) for _ in range(B)])
    poses = np.stack([[_pose(rng, pf[b], 0.3, np.deg2rad(10)) for _ in range(n - 1)] for b in range(B)])
    lists = [[sc.points(100 + b, pf[b], seed=10 * b)[0]] + [sc.points(100 + b, poses[b, k], seed=10 * b + 1 + k)[0] for k in range(n - 1)] for b in range(B)]
    fe = _fe(liw, lp, B, slots=n)
    for s in range(n):
        P, npts = liw.laser_batch.pad_points([lists[b][s] for b in range(B)], N_RAYS)
        fe.spawn(s, torch.from_numpy(P).cuda(), torch.from_numpy(npts).cuda())
    o = _np(fe.match_front(0, 1, n - 1, pf, poses))
    worst, total = 0.0, 0
    for b in range(B):
        mgr = liw.laser.LaserManager(lp)
        mgr.add_scan(liw.laser.Scan.spawn(lp, lists[b][0]), pf[b, :3], pf[b, 3:])
        for k in range(n - 1):
            hm = mgr.match_with_front(liw.laser.Scan.spawn(lp, lists[b][1 + k]), poses[b, k, :3], poses[b, k, 3:])
            worst = max(worst, _compare_match(hm, {key: o[key][:, k] for key in KEYS}, b, ("front", k)))
            total += len(hm)
    print("match_front against the host: %d pairs, max |device - host| = %.3e" % (total, worst))
    assert total > 4 * B * (n - 1)


# ------------------------------------------------------------------------------------------------------------------ 3
def _numpy_pack(m, n, pf, cap):
    B, F = m["count"].shape
    cnt = np.clip(m["count"], 0, cap)
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(cnt.sum(1))
    frames, pts = [], []
    for b in range(B):
        for f in range(1, n):
            frames += [f] * int(cnt[b, f - 1])
            pts.append(m["recs"][b, f - 1, :cnt[b, f - 1]])
    pts = np.concatenate(pts, 0) if pts else np.zeros((0, 12))
    mp = np.zeros((B, n, 12))
    mp[:, 0, :6], mp[:, 0, 6:] = pf, pf
    mp[:, 1:] = m["match_pose"]
    return dict(laser_off=off, laser_frame=np.asarray(frames, dtype=np.int32), laser_pts=np.ascontiguousarray(pts.T).reshape(-1),
                match_pose=mp.reshape(-1), has_match=np.ones(B * n, dtype=np.uint8), init_ok=(m["count"] >= 2).all(1).astype(np.uint8)), int(off[-1])


@pytest.mark.parametrize("B,n", [(B0, 6), (1030, 3)])
def test_pack_init_equals_numpy_pack(env, gentle, B, n):
    base = gentle
    liw, lp, sc, torch = env
    F = n - 1
    rob = np.arange(B) % B0
    pf, poses = base["pf"][rob], np.ascontiguousarray(base["poses"][rob][:, :F])
    fe = _spawned(env, base, B, n, rob)
    probe = _lane_reference(fe, F, pf, poses, 0, 256)["count"]       # the lane kernel's counts decide which match overflows
    cap = int(probe.max()) - 1
    over = (probe > cap).any(1)
    fe = _spawned(env, base, B, n, rob)
    m = fe.match_front(0, 1, F, pf, poses, cap=cap)
    mh = _np(m)
    ref, Ltot = _numpy_pack(mh, n, pf, cap)
    fail = np.isin(rob, [R_EMPTY_FRONT, R_EMPTY_FRAME, R_ONE_WALL, R_INVALID]) | over
    assert np.array_equal(ref["init_ok"], (~fail).astype(np.uint8)), (np.nonzero(ref["init_ok"] == 0)[0][:10], np.nonzero(fail)[0][:10])
    assert fail.any() and (~fail).any() and Ltot > 4 * B
    assert over.any() and (mh["count"][probe > cap] == 0).all() and len(set(rob[over].tolist())) == 1
    G = 64
    sizes = dict(laser_off=(B + 1, torch.int32), laser_frame=(Ltot, torch.int32), laser_pts=(12 * Ltot, torch.float64),
                 match_pose=(B * n * 12, torch.float64), has_match=(B * n, torch.uint8), init_ok=(B, torch.uint8))

    def guarded():
        g = {k: torch.full((s + 2 * G,), 77, dtype=dt, device="cuda") for k, (s, dt) in sizes.items()}
        v = {k: t[G:-G] for k, t in g.items()}
        return g, v

    def run(L_cap):
        g, v = guarded()
        res = fe.pack_init(m, n, pf, out={k: v[k] for k in ("match_pose", "has_match", "init_ok")}, L_cap=L_cap,
                           bufs={k: v[k] for k in ("laser_off", "laser_frame", "laser_pts")})
        torch.cuda.synchronize()
        return g, v, res

    g, v, (dev, Lt, ok) = run(Ltot)
    assert Lt == Ltot
    for k, t in g.items():
        assert (t[:G] == 77).all() and (t[-G:] == 77).all(), k
        assert np.array_equal(v[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(ok.cpu().numpy()[:B], ref["init_ok"])
    for k in ("laser_off", "laser_frame", "laser_pts", "match_pose", "has_match"):
        assert np.array_equal(dev[k].cpu().numpy(), ref[k]), k
    g2, v2, (_, Lt2, _) = run(Ltot)                                # a second run is bitwise identical
    assert Lt2 == Ltot
    for k in g:
        assert torch.equal(g[k].view(torch.uint8), g2[k].view(torch.uint8)), k
    # one block too few: LIW_ENOMEM and nothing but laser_off written
    g3, v3 = guarded()
    with pytest.raises(liw.LiwError) as e:
        fe.pack_init(m, n, pf, out={k: v3[k] for k in ("match_pose", "has_match", "init_ok")}, L_cap=Ltot - 1,
                     bufs={k: v3[k] for k in ("laser_off", "laser_frame", "laser_pts")})
    assert e.value.code == ENOMEM
    torch.cuda.synchronize()
    for k, t in g3.items():
        if k == "laser_off":
            assert (t[:G] == 77).all() and (t[-G:] == 77).all() and np.array_equal(v3[k].cpu().numpy(), ref[k])
        else:
            assert (t == 77).all(), k


# ------------------------------------------------------------------------------------------------------------------ 4
def _regions(dims):
    sb = (32 + 80 * dims["max_lines"] + 8 * dims["max_cell_entries"] + 255) // 256 * 256
    return 256 + (dims["slots"] + 2) * sb, sb


@pytest.mark.parametrize("n_acc", [2, 4])
def test_rebuild_equals_host_manager(env, n_acc):
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=n_acc)
    lb = liw.laser_batch
    B, F = 24, 6
    rng = np.random.default_rng(4400 + n_acc)
    poses = np.zeros((B, F + 1, 6))
    for b in range(B):
        poses[b, 0] = _pose(rng)
        for k in range(1, F + 1):   # identical consecutive poses on a third of the steps: the motion filter fires
            poses[b, k] = poses[b, k - 1] if (k + b) % 3 == 0 and k < F else _pose(rng, poses[b, k - 1], 0.15, np.deg2rad(4))
    lists = [[sc.points(200 + b, poses[b, k], seed=10 * b + k)[0] for k in range(F + 1)] for b in range(B)]
    mask = np.array([0 if b % 5 == 2 else 1 for b in range(B)], dtype=np.uint8)
    dims = dict(B=B, slots=F + 1, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)
    fe = _fe(liw, lp, B, slots=F + 1)
    for s in range(F + 1):
        P, npts = lb.pad_points([lists[b][s] for b in range(B)], N_RAYS)
        fe.spawn(s, torch.from_numpy(P).cuda(), torch.from_numpy(npts).cuda())
    # a manager state from before the initialisation, which the rebuild has to discard (and to keep for the masked robots)
    stale = poses[:, ::-1].copy()
    for s in (F, 2, 4):
        fe.add_scan(s, stale[:, s])
    torch.cuda.synchronize()
    before = fe.store.cpu().numpy().copy()
    if n_acc == 4:                                                 # the poses as frames of a states array
        x = torch.zeros(B, F, 15, dtype=torch.float64, device="cuda")
        x[:, :, :6] = torch.from_numpy(poses[:, :F]).cuda()
        fe.rebuild(0, F, x, mask=mask)
    else:
        fe.rebuild(0, F, poses[:, :F], mask=mask)
    torch.cuda.synchronize()
    after = fe.store.cpu().numpy().copy()
    rb, sb = _regions(dims)
    assert before.size == B * rb
    for b in range(B):
        r0, r1 = before[b * rb:(b + 1) * rb], after[b * rb:(b + 1) * rb]
        assert np.array_equal(r0[256:256 + (F + 1) * sb], r1[256:256 + (F + 1) * sb]), ("scan slots", b)
        if not mask[b]:
            assert np.array_equal(r0, r1), ("masked robot", b)
        else:
            assert not np.array_equal(r0, r1), b
    o = _np(fe.match_with_ref(F, poses[:, F]))
    worst, refs, total = 0.0, 0, 0
    for b in range(B):
        if not mask[b]:
            continue
        hs = [liw.laser.Scan.spawn(lp, lists[b][k]) for k in range(F + 1)]
        mgr = liw.laser.LaserManager(lp)
        for s in (F, 2, 4):
            mgr.add_scan(hs[s], stale[b, s, :3], stale[b, s, 3:])
        mgr.clear_all_scan()
        for k in range(F):
            mgr.add_scan(hs[k], poses[b, k, :3], poses[b, k, 3:])
        r = mgr.ref_scan()
        dl = fe.get_lines(b, lb.REF)
        if r is None:
            assert dl is None, (n_acc, b)
        else:
            refs += 1
            worst = max(worst, _compare_lines(r[0].lines(), dl, ("ref", n_acc, b)))
            p, q = fe.submap_pose(b)
            assert np.array_equal(p, r[1]) and np.array_equal(q, r[2]), b
        hm = mgr.match_with_ref(hs[F], poses[b, F, :3], poses[b, F, 3:])
        worst = max(worst, _compare_match(hm, o, b, ("after rebuild", n_acc)))
        total += len(hm)
        assert fe.status(b) == 0
    print("rebuild n_acc=%d: %d reference sub-maps, %d pairs of the seventh scan, max |device - host| = %.3e" % (n_acc, refs, total, worst))
    assert refs > 0 and total > 0


# ------------------------------------------------------------------------------------------------------------------ 5
def _sub(d, lo, m):
    N = int(d["n"])
    o = dict(d)
    o["n"] = m
    for k in ("states", "match_pose", "truth_states"):
        o[k] = np.asarray(d[k]).reshape(N, -1)[lo:lo + m].copy()
    o["has_match"] = np.asarray(d["has_match"])[lo:lo + m].copy()
    for k in ("imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP", "wheel_Dt"):
        o[k] = np.asarray(d[k])[lo:lo + m - 1].copy()
    o["laser_frame"] = np.zeros(0, dtype=np.int32)
    o["laser_pts"] = np.zeros((0, 12))
    return o


def _rel(a, h):
    return float((a - h).abs().max() / h.abs().max().clamp_min(1e-300))


def test_end_to_end_init_then_track(env, synth):
    """64 robots tiled from 8 windows; each trajectory is made with one frame more than the 6-frame INIT window (same L = 0,
    state_noise = 0.5), and that seventh frame is the tracking frame that follows the initialisation"""
    liw, lp0, sc, torch = env
    lb = liw.laser_batch
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)   # a reference sub-map exists after six add_scans
    nb, B, n = 8, 64, 6
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7300 + j, n=n + 1, L=0, state_noise=0.5) for j in range(nb)]
    T_il = np.array(synth.normalize_extrinsic(prm["T_imu_to_laser"])).reshape(4, 4)
    scans = []
    for j in range(nb):
        truth = np.asarray(trajs[j]["truth_states"]).reshape(n + 1, 15)
        room = [(a + truth[0, 0:2], b + truth[0, 0:2]) for a, b in liw.laser.room_segments(3 + j)]   # centred on the first pose
        row = []
        for k in range(n + 1):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = synth.exp_so3(truth[k, 3:6]), truth[k, 0:3]
            rg, amin, inc = liw.laser.cast_scan(room, T @ T_il, seed=500 + 10 * j + k)
            row.append(liw.laser.laser_to_points(rg, amin, inc, 0.0, float(k))[0])
        scans.append(row)
    est = [np.asarray(trajs[j]["states"]).reshape(n + 1, 15) for j in range(nb)]
    rob = np.arange(B) % nb
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fe = _fe(liw, lp, B, slots=n + 1)
    for k in range(n):
        P, npts = lb.pad_points([scans[j][k] for j in rob], N_RAYS)
        fe.spawn(k, up(P), up(npts))
    wins = [_sub(trajs[j], 0, n) for j in rob]
    host = liw.batch.host_arrays(wins)
    base = {k: up(v) for k, v in host.items() if k != "_Ltot"}
    # ---- device: matches of frames 1 .. 5 against the front, poses read out of x, packed for the INIT solve
    td = {k: v.clone() for k, v in base.items()}
    xv = td["x"].view(B, n, 15)
    pf = xv[:, 0, :6].contiguous()
    m = fe.match_front(0, 1, n - 1, pf, xv[:, 1:, :6])
    dev, Ltot, ok = fe.pack_init(m, n, pf)
    assert int(m["count"].min()) >= 4 and bool((ok == 1).all())
    td.update(dev)
    # ---- host: match_with_front per distinct window, packed on the host
    mgrs, hscans, hms = [], [], []
    for j in range(nb):
        hs = [liw.laser.Scan.spawn(lp, scans[j][k], float(k)) for k in range(n + 1)]
        mgr = liw.laser.LaserManager(lp)
        mgr.add_scan(hs[0], est[j][0, 0:3], est[j][0, 3:6])
        hms.append([mgr.match_with_front(hs[k], est[j][k, 0:3], est[j][k, 3:6]) for k in range(1, n)])
        mgrs.append(mgr)
        hscans.append(hs)
    assert all(len(h) >= 4 for row in hms for h in row)
    cnt = np.array([[len(h) for h in hms[j]] for j in rob])
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(cnt.sum(1))
    mp = np.zeros((B, n, 12))
    for b, j in enumerate(rob):
        mp[b, 0] = np.concatenate([est[j][0, 0:6], est[j][0, 0:6]])
        for k in range(1, n):
            mp[b, k] = hms[j][k - 1].pose
    hpack = dict(laser_off=off, laser_frame=np.concatenate([np.repeat(np.arange(1, n), cnt[b]) for b in range(B)]).astype(np.int32),
                 laser_pts=np.ascontiguousarray(np.concatenate([h.pts for j in rob for h in hms[j]], 0).T).reshape(-1),
                 match_pose=mp.reshape(-1), has_match=np.ones(B * n, dtype=np.uint8))
    assert int(off[-1]) == Ltot
    d_pts = 0.0
    for k, v in hpack.items():
        dv = dev[k].cpu().numpy()
        if k == "laser_pts":
            assert dv.shape == v.shape
            d_pts = float(np.abs(dv - v).max())
            assert d_pts <= 1e-9, d_pts
        else:
            assert np.array_equal(dv, v), k
    th = dict({k: v.clone() for k, v in base.items()}, **{k: up(v) for k, v in hpack.items()})
    wl = [dict(w, laser_frame=np.ones(1, np.int32), laser_pts=np.zeros((1, 12))) for w in wins]
    bs_d, bs_h = liw.BatchSolver(prm, wl), liw.BatchSolver(prm, wl)
    for bs, t in ((bs_d, td), (bs_h, th)):
        bs.rebind(t, Ltot)
        bs.solve(liw.LIW_MODE_INIT, 50)
    torch.cuda.synchronize()
    assert torch.isfinite(bs_d.t["x"]).all()
    d_init = _rel(bs_d.t["x"], bs_h.t["x"])
    assert d_init <= 1e-6, d_init
    # ---- the sub-maps again from the window's scans at the solved poses, then the prior
    fe.rebuild(0, n, bs_d.t["x"].view(B, n, 15), mask=ok)
    xh = bs_h.states()
    for j in range(nb):
        mgrs[j].clear_all_scan()
        for k in range(n):
            mgrs[j].add_scan(hscans[j][k], xh[j, k, 0:3], xh[j, k, 3:6])
    for bs in (bs_d, bs_h):
        bs.marginalize()
    # ---- one tracking frame on (frame 5 as solved, frame 6)
    wins2 = [_sub(trajs[j], n - 1, 2) for j in rob]
    base2 = {k: up(v) for k, v in liw.batch.host_arrays(wins2).items() if k != "_Ltot"}
    P, npts = lb.pad_points([scans[j][n] for j in rob], N_RAYS)
    fe.spawn(n, up(P), up(npts))
    t2d, t2h = {k: v.clone() for k, v in base2.items()}, {k: v.clone() for k, v in base2.items()}
    t2d["x"].view(B, 2, 15)[:, 0] = bs_d.t["x"].view(B, n, 15)[:, n - 1]
    t2h["x"].view(B, 2, 15)[:, 0] = bs_h.t["x"].view(B, n, 15)[:, n - 1]
    pose6 = np.stack([est[j][n, 0:6] for j in rob])
    m2 = fe.match_with_ref(n, pose6, cap=256)
    dev2, L2 = fe.pack_track(m2, n=2, frame=1, out=dict(match_pose=t2d["match_pose"], has_match=t2d["has_match"]))
    t2d.update(dev2)
    hm2 = [mgrs[j].match_with_ref(hscans[j][n], est[j][n, 0:3], est[j][n, 3:6]) for j in range(nb)]
    cnt2 = np.array([len(hm2[j]) for j in rob], dtype=np.int32)
    assert (cnt2 >= 4).all()
    off2 = np.zeros(B + 1, dtype=np.int32)
    off2[1:] = np.cumsum(cnt2)
    assert int(off2[-1]) == L2
    mp2, hmask2 = base2["match_pose"].cpu().numpy().reshape(B, 2, 12).copy(), base2["has_match"].cpu().numpy().reshape(B, 2).copy()
    for b, j in enumerate(rob):
        mp2[b, 1], hmask2[b, 1] = hm2[j].pose, 1
    hpack2 = dict(laser_off=off2, laser_frame=np.ones(L2, dtype=np.int32),
                  laser_pts=np.ascontiguousarray(np.concatenate([hm2[j].pts for j in rob], 0).T).reshape(-1), match_pose=mp2.reshape(-1),
                  has_match=hmask2.reshape(-1))
    d_pts2 = 0.0
    for k, v in hpack2.items():
        dv = dev2[k].cpu().numpy()
        if k == "laser_pts":
            assert dv.shape == v.shape
            d_pts2 = float(np.abs(dv - v).max())
            assert d_pts2 <= 1e-9, d_pts2
        else:
            assert np.array_equal(dv, v), k
    t2h.update({k: up(v) for k, v in hpack2.items()})
    wl2 = [dict(w, laser_frame=np.ones(1, np.int32), laser_pts=np.zeros((1, 12))) for w in wins2]
    d_track = 0.0
    pairs = []
    for bs1, t in ((bs_d, t2d), (bs_h, t2h)):
        bs2 = liw.BatchSolver(prm, wl2)
        for name in ("prior_X", "prior_J", "prior_R", "has_prior"):   # the carried prior of the initialisation
            bs2.t[name].copy_(bs1.t[name])
        bs2.rebind(t, L2)
        bs2.solve(liw.LIW_MODE_TRACK)
        bs2.marginalize()
        pairs.append(bs2)
    torch.cuda.synchronize()
    assert torch.equal(pairs[0].t["has_prior"], pairs[1].t["has_prior"]) and bool((pairs[0].t["has_prior"] != 0).all())
    for name in ("x", "prior_X", "prior_J", "prior_R"):
        a, h = pairs[0].t[name], pairs[1].t[name]
        assert torch.isfinite(a).all(), name
        r = _rel(a, h)
        d_track = max(d_track, r)
        assert r <= 1e-6, (name, r)
    print("init end to end: %d robots, %d + %d blocks; end points max |device - host| %.3e / %.3e; states after INIT %.3e, states and priors "
          "after the tracking frame %.3e (relative)" % (B, Ltot, L2, d_pts, d_pts2, d_init, d_track))


# ------------------------------------------------------------------------------------------------------------------ 6
def test_argument_checks(env, base):
    liw, lp, sc, torch = env
    slots, cap, n = F0 + 1, 64, F0 + 1
    fe = _spawned(env, base, B0, slots)
    L, h, p = fe.L, fe.h, fe._p
    pf, poses = torch.from_numpy(base["pf"]).cuda(), torch.from_numpy(base["poses"]).cuda()
    m = fe.match_front(0, 1, F0, pf, poses, cap=cap)
    fe.add_scan(0, pf)
    torch.cuda.synchronize()
    store0 = fe.store.clone()
    z = lambda s, dt: torch.full((s,), 77, dtype=dt, device="cuda")
    o = dict(count=z(B0 * F0, torch.int32), recs=z(B0 * F0 * cap * 12, torch.float64), idx1=z(B0 * F0 * cap, torch.int32), idx2=z(B0 * F0 * cap, torch.int32),
             match_pose=z(B0 * F0 * 12, torch.float64), laser_off=z(B0 + 1, torch.int32), laser_frame=z(B0 * F0 * cap, torch.int32),
             laser_pts=z(12 * B0 * F0 * cap, torch.float64), mp_out=z(B0 * n * 12, torch.float64), has_match=z(B0 * n, torch.uint8), init_ok=z(B0, torch.uint8))

    def mf(front, first, F, cap_):
        return L.liw_lfe_match_front(h, p(fe.store), front, first, F, p(pf), p(poses), 6 * F0, 6, 0, cap_, p(o["count"]), p(o["recs"]), p(o["idx1"]),
                                     p(o["idx2"]), p(o["match_pose"]), None)

    def pk(n_, cap_):
        return L.liw_lfe_pack_init(h, n_, cap_, p(m["count"]), p(m["recs"]), p(m["match_pose"]), p(pf), B0 * F0 * cap, p(o["laser_off"]), p(o["laser_frame"]),
                                   p(o["laser_pts"]), p(o["mp_out"]), p(o["has_match"]), p(o["init_ok"]), None)

    def rb(first, F):
        return L.liw_lfe_rebuild(h, p(fe.store), first, F, p(poses), 6 * F0, 6, None, None)

    bad = [mf(0, 1, 0, cap), mf(0, 1, -1, cap), mf(0, -1, F0, cap), mf(0, 2, F0, cap), mf(0, slots, 1, cap), mf(-1, 1, F0, cap), mf(slots, 1, F0, cap),
           mf(0, 1, F0, 0), pk(1, cap), pk(0, cap), pk(n, 0), rb(0, 0), rb(-1, F0), rb(2, F0), rb(slots, 1)]
    assert bad == [EINVAL] * len(bad), bad
    torch.cuda.synchronize()
    assert torch.equal(fe.store, store0)
    for k, t in o.items():
        assert (t == 77).all(), k
    with pytest.raises(liw.LiwError) as e:
        fe.match_front(0, 2, F0, pf, poses)
    assert e.value.code == EINVAL
    assert mf(0, 1, F0, cap) == 0 and pk(n, cap) > 0 and rb(0, F0) == 0      # the same calls with good arguments go through
    torch.cuda.synchronize()
