"""The batched laser front-end on the device (laser_batch.BatchFrontEnd, include/liw_laser_batch.h) against the host
front-end (liw.laser), which the existing tests tie to the oracle: ranges -> points (bitwise), de-skew, spawn (lines, scan::lines
order, line_map cell by cell), do_match, the laser_manager sequence, the packed tracking input of BatchSolver, scale and
determinism, capacity handling."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_MIN, N_RAYS = np.float32(-2.0 * np.pi * 0.75 / 2), 1080
ANG_INC = np.float32(2.0 * np.pi * 0.75 / (N_RAYS - 1))
T_INC = np.float32(1.0 / (40.0 * N_RAYS))


def _rodrigues(q):
    th = np.linalg.norm(q)
    if th < 1e-15:
        return np.eye(3)
    k = q / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _T(p, q):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rodrigues(np.asarray(q, dtype=np.float64)), p
    return T


class Scene:
    """rooms (liw.laser.room_segments) and IMU poses; scans cast at the laser pose T_w_i @ T_imu_to_laser"""

    def __init__(self, liw, lp):
        self.liw, self.lp = liw, lp
        self.Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
        self.rooms = {}

    def ranges(self, room, pose, seed):
        if room not in self.rooms:
            self.rooms[room] = self.liw.laser.room_segments(room)
        T = _T(pose[:3], pose[3:]) @ self.Til
        r, _, _ = self.liw.laser.cast_scan(self.rooms[room], T, n_rays=N_RAYS, seed=seed)
        return r

    def points(self, room, pose, seed, stamp=0.0):
        return self.liw.laser.laser_to_points(self.ranges(room, pose, seed), ANG_MIN, ANG_INC, T_INC, stamp)


def _pose(rng, base=None, dp=0.0, dq=0.0):
    if base is None:
        return np.concatenate([rng.uniform(-1.0, 1.0, 2), [0.0], [0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
    p = base.copy()
    p[:2] += rng.uniform(-dp, dp, 2)
    p[5] += rng.uniform(-dq, dq)
    return p


@pytest.fixture(scope="module")
def env(liw):
    import torch
    lp = liw.laser.office_laser_params()
    return liw, lp, Scene(liw, lp), torch


def _fe(liw, lp, B, slots=2, max_points=N_RAYS, max_lines=256, max_cell_entries=8192, **kw):
    fe = liw.laser_batch.BatchFrontEnd(lp, dict(B=B, slots=slots, max_points=max_points, max_lines=max_lines, max_cell_entries=max_cell_entries), **kw)
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    return fe


def _compare_lines(host_lines, dev_lines, what):
    assert host_lines.shape == dev_lines.shape, (what, host_lines.shape, dev_lines.shape)
    d = float(np.abs(host_lines - dev_lines).max()) if host_lines.size else 0.0
    assert d <= 1e-9, (what, d)
    return d


def _compare_match(hm, o, b, what):
    n = int(o["count"][b])
    assert n == len(hm), (what, b, n, len(hm))
    assert np.array_equal(o["match_pose"][b], hm.pose), (what, b)
    if n:
        assert np.array_equal(o["idx1"][b, :n], hm.idx1), (what, b)
        assert np.array_equal(o["idx2"][b, :n], hm.idx2), (what, b)
        d = float(np.abs(o["recs"][b, :n] - hm.pts).max())
        assert d <= 1e-9, (what, b, d)
        return d
    return 0.0


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


# ------------------------------------------------------------------------------------------------------------------ 1
def test_ranges_to_points_bitwise(env):
    liw, lp, sc, torch = env
    B = 64
    rng = np.random.default_rng(11)
    R = np.zeros((B, N_RAYS), dtype=np.float32)
    for b in range(B):
        r = sc.ranges(b % 16, _pose(rng), seed=b)
        idx = rng.choice(N_RAYS, 40, replace=False)
        r[idx[:8]] = np.nan
        r[idx[8:16]] = np.inf
        r[idx[16:24]] = rng.uniform(-0.2, 0.1, 8).astype(np.float32)
        r[idx[24:28]] = np.float32(0.1)
        i0 = int(rng.integers(10, N_RAYS - 40))       # a run of sub-centimetre spaced returns
        r[i0:i0 + 30] = np.float32(0.6) + np.arange(30, dtype=np.float32) * np.float32(1e-4)
        R[b] = r
    stamps = rng.uniform(0, 100, B)
    fe = _fe(liw, lp, B)
    pts, times, n = fe.ranges_to_points(torch.from_numpy(R), stamps)
    pts, times, n = pts.cpu().numpy(), times.cpu().numpy(), n.cpu().numpy()
    for b in range(B):
        hp, ht = liw.laser.laser_to_points(R[b], ANG_MIN, ANG_INC, T_INC, stamps[b])
        assert n[b] == hp.shape[0], b
        assert np.array_equal(pts[b, :n[b]], hp), b
        assert np.array_equal(times[b, :n[b]], ht), b
    assert fe.status(0) == 0


# ------------------------------------------------------------------------------------------------------------------ 2
def test_deskew(env):
    liw, lp, sc, torch = env
    B = 16
    rng = np.random.default_rng(12)
    fe = _fe(liw, lp, B)
    lists, tl = [], []
    for b in range(B):
        p, t = sc.points(b, _pose(rng), seed=b, stamp=10.0)
        lists.append(p)
        tl.append(t)
    P, n = liw.laser_batch.pad_points(lists, N_RAYS)
    Tm = liw.laser_batch.pad_times(tl, N_RAYS)
    lin, ang = rng.normal(0, 0.8, (B, 3)), rng.normal(0, 0.6, (B, 3))
    stamps = np.full(B, 10.0)
    dp = torch.from_numpy(P).cuda()
    fe.deskew(dp, torch.from_numpy(Tm).cuda(), torch.from_numpy(n).cuda(), stamps, lin, ang)
    out = dp.cpu().numpy()
    worst = 0.0
    for b in range(B):
        h = liw.laser.laser_correct(lists[b], tl[b], 10.0, lin[b], ang[b])
        worst = max(worst, float(np.abs(out[b, :n[b]] - h).max()))
        assert np.array_equal(out[b, n[b]:], P[b, n[b]:])
    print("deskew max |device - host| = %.3e" % worst)
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ 3
def _edge_scans(rng):
    wall = np.stack([np.linspace(-2, 2, 300), np.full(300, 1.5) + rng.normal(0, 0.002, 300), np.zeros(300)], 1)
    arc = np.stack([2 * np.cos(np.linspace(0, 2, 400)), 2 * np.sin(np.linspace(0, 2, 400)), np.zeros(400)], 1)
    pairs = []
    for k in range(60):                      # runs of 2 points, 0.5 m apart: every run shorter than the step
        x = -3 + 0.5 * k
        pairs += [[x, 1.0, 0.0], [x + 0.02, 1.0, 0.0]]
    return [np.zeros((0, 3)), np.array([[1.0, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0], [1.0, 0.05, 0.0]]),
            np.array([[1.0, 0.0, 0.0], [1.0, 0.05, 0.0], [1.0, 0.1, 0.0]]), wall, arc, np.array(pairs)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_spawn_lines_and_cells(env, seed):
    liw, lp, sc, torch = env
    rng = np.random.default_rng(100 + seed)
    lists = [sc.points(seed * 40 + b, _pose(rng), seed=b)[0] for b in range(40)] + _edge_scans(rng)
    B = len(lists)
    fe = _fe(liw, lp, B)
    P, n = liw.laser_batch.pad_points(lists, N_RAYS)
    times = rng.uniform(0, 10, B)
    fe.spawn(0, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda(), torch.from_numpy(times).cuda())
    worst, cells = 0.0, 0
    for b in range(B):
        hs = liw.laser.Scan.spawn(lp, lists[b], times[b])
        hl = hs.lines()
        assert fe.status(b, 0) == 0
        worst = max(worst, _compare_lines(hl, fe.get_lines(b, 0), ("spawn", seed, b)))
        if b % 4 and b < 40:
            continue
        for x, y in lists[b][:, :2]:         # every cell a host line occupies holds one of the scan's points
            kh, ih = hs.cell_lines(x, y, 64)
            kd, idv = fe.cell_lines(b, 0, x, y, 64)
            assert kh == kd and np.array_equal(ih, idv), (seed, b, x, y, ih, idv)
            cells += 1
    print("spawn seed %d: max |device - host| over p1 p2 abc len = %.3e, %d cells compared" % (seed, worst, cells))


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("kk", [0, 1])
def test_match(env, kk):
    liw, lp, sc, torch = env
    rng = np.random.default_rng(200 + kk)
    B = 48
    p1 = np.stack([_pose(rng) for _ in range(B)])
    p2 = np.stack([_pose(rng, p1[b], 0.3, np.deg2rad(10)) for b in range(B)])
    l1 = [sc.points(b, p1[b], seed=2 * b)[0] for b in range(B)]
    l2 = [sc.points(b, p2[b], seed=2 * b + 1)[0] for b in range(B)]
    l1[B - 1] = np.zeros((0, 3))              # an empty reference scan
    fe = _fe(liw, lp, B)
    for slot, lists in ((0, l1), (1, l2)):
        P, n = liw.laser_batch.pad_points(lists, N_RAYS)
        fe.spawn(slot, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())
    o = _np(fe.match(0, 1, p1, p2, kk=kk, cap=256))
    worst, total = 0.0, 0
    for b in range(B):
        hm = liw.laser.do_match(lp, liw.laser.Scan.spawn(lp, l1[b]), liw.laser.Scan.spawn(lp, l2[b]), p1[b, :3], p1[b, 3:], p2[b, :3], p2[b, 3:], kk)
        worst = max(worst, _compare_match(hm, o, b, ("match", kk)))
        total += len(hm)
    assert o["count"][B - 1] == 0
    assert total > 4 * B
    print("match kk=%d: %d pairs, max |device - host| = %.3e" % (kk, total, worst))
    # the manager's reference before any add_scan: empty match with pose (p q p q)
    e = _np(fe.match_with_ref(1, p2))
    hmgr = liw.laser.LaserManager(lp)
    he = hmgr.match_with_ref(liw.laser.Scan.spawn(lp, l2[0]), p2[0, :3], p2[0, 3:])
    assert (e["count"] == 0).all() and np.array_equal(e["match_pose"][0], he.pose) and len(he) == 0


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("n_acc", [2, 4])
def test_manager_sequence(env, n_acc):
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=n_acc)
    B, F = 32, 9
    rng = np.random.default_rng(300 + n_acc)
    poses = np.zeros((F, B, 6))
    poses[0] = np.stack([_pose(rng) for _ in range(B)])
    for k in range(1, F):
        for b in range(B):
            # repeated poses (the motion filter fires) on a third of the steps
            poses[k, b] = poses[k - 1, b] if (k + b) % 3 == 0 else _pose(rng, poses[k - 1, b], 0.15, np.deg2rad(4))
    fe = _fe(liw, lp, B)
    hm = [liw.laser.LaserManager(lp) for _ in range(B)]
    worst, total, refs = 0.0, 0, 0
    for k in range(F + 1):
        kf = min(k, F - 1)
        lists = [sc.points(b, poses[kf, b], seed=1000 * k + b)[0] for b in range(B)]
        P, n = liw.laser_batch.pad_points(lists, N_RAYS)
        fe.spawn(0, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())
        if k == F:                                            # clear_all_scan: the next match is empty, as on the host
            fe.reset()
            fe.spawn(0, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())
            for m in hm:
                m.clear_all_scan()
        o = _np(fe.match_with_ref(0, poses[kf]))
        hs = [liw.laser.Scan.spawn(lp, lists[b]) for b in range(B)]
        for b in range(B):
            h = hm[b].match_with_ref(hs[b], poses[kf, b, :3], poses[kf, b, 3:])
            worst = max(worst, _compare_match(h, o, b, ("manager", n_acc, k)))
            total += len(h)
        if k == F:
            assert (o["count"] == 0).all()
            break
        fe.add_scan(0, poses[kf])
        for b in range(B):
            hm[b].add_scan(hs[b], poses[kf, b, :3], poses[kf, b, 3:])
            r = hm[b].ref_scan()
            dl = fe.get_lines(b, liw.laser_batch.REF)
            if r is None:
                assert dl is None, (n_acc, k, b)
                continue
            refs += 1
            worst = max(worst, _compare_lines(r[0].lines(), dl, ("ref", n_acc, k, b)))
            p, q = fe.submap_pose(b)
            assert np.array_equal(p, r[1]) and np.array_equal(q, r[2])
            assert fe.status(b) == 0
    assert total > 0 and refs > 0
    print("manager n_acc=%d: %d pairs, %d reference sub-maps compared, max |device - host| = %.3e" % (n_acc, total, refs, worst))


# ------------------------------------------------------------------------------------------------------------------ 6
def _sub_window(d, lo, m=2):
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


def test_end_to_end_track_batch(env, synth):
    liw, lp, sc, torch = env
    prm = synth.office_params()
    # ref_n_accumulation 4: the reference sub-map exists at every frame (with office's 2 it is dropped every other add_scan)
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
    nb, B, F = 8, 256, 4
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=F + 2, L=8) for j in range(nb)]
    st = lambda j, k: np.asarray(trajs[j]["states"]).reshape(F + 2, 15)[k]
    rooms = [3000 + j for j in range(nb)]
    pose = lambda j, k: np.asarray(st(j, k)[0:6], dtype=np.float64)
    fe = _fe(liw, lp, B, max_lines=256, max_cell_entries=8192)
    hm = [liw.laser.LaserManager(lp) for _ in range(nb)]
    rob = np.arange(B) % nb
    scans = [[sc.points(rooms[j], pose(j, k), seed=j * 10 + k)[0] for k in range(F + 1)] for j in range(nb)]
    P0, n0 = liw.laser_batch.pad_points([scans[j][0] for j in rob], N_RAYS)
    fe.spawn(0, torch.from_numpy(P0).cuda(), torch.from_numpy(n0).cuda())
    fe.add_scan(0, np.stack([pose(j, 0) for j in rob]))
    for j in range(nb):
        hm[j].add_scan(liw.laser.Scan.spawn(lp, scans[j][0]), pose(j, 0)[:3], pose(j, 0)[3:])
    bs_d = bs_h = None
    d_pts = d_state = 0.0
    for k in range(1, F + 1):
        wins = [_sub_window(trajs[j], k - 1) for j in rob]
        host = liw.batch.host_arrays(wins)
        poses = np.stack([pose(j, k) for j in rob])
        P, n = liw.laser_batch.pad_points([scans[j][k] for j in rob], N_RAYS)
        fe.spawn(0, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())
        m = fe.match_with_ref(0, poses, cap=256)
        base = {kk: torch.from_numpy(np.ascontiguousarray(v)).cuda() for kk, v in host.items() if kk != "_Ltot"}
        dev, Ltot = fe.pack_track(m, n=2, frame=1, out=dict(match_pose=base["match_pose"].clone(), has_match=base["has_match"].clone()))
        # the host front-end's matches, packed on the host
        hms = []
        for j in range(nb):
            hs = liw.laser.Scan.spawn(lp, scans[j][k])
            hms.append((hm[j].match_with_ref(hs, pose(j, k)[:3], pose(j, k)[3:]), hs))
        recs = [hms[j][0].pts for j in rob]
        cnt = np.array([r.shape[0] for r in recs], dtype=np.int32)
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum(cnt)
        Lh = int(off[-1])
        assert Lh == Ltot and Lh > 0
        mp = np.asarray(host["match_pose"]).reshape(B, 2, 12).copy()
        hmask = np.asarray(host["has_match"]).reshape(B, 2).copy()
        for b, j in enumerate(rob):
            mp[b, 1] = hms[j][0].pose
            hmask[b, 1] = 1
        hpack = dict(laser_off=off, laser_frame=np.ones(Lh, dtype=np.int32), laser_pts=np.ascontiguousarray(np.concatenate(recs, 0).T).reshape(-1),
                     match_pose=mp.reshape(-1), has_match=hmask.reshape(-1))
        # structure bitwise; end points: the reference sub-map's lines are the earlier scans' lines moved by make_tf of the stored
        # poses, whose device sin / cos differ from glibc's by an ulp, so from frame 2 on they agree to round-off, not bit for bit
        for kk, v in hpack.items():
            dv = dev[kk].cpu().numpy()
            if kk == "laser_pts":
                assert dv.shape == v.shape, k
                d_pts = max(d_pts, float(np.abs(dv - v).max()))
                assert d_pts <= 1e-9, (k, d_pts)
            else:
                assert np.array_equal(dv, v), (k, kk)
        for j in range(nb):
            hm[j].add_scan(hms[j][1], pose(j, k)[:3], pose(j, k)[3:])
        fe.add_scan(0, poses)
        # each solver gets its own copy of the inputs (solve updates x and match_pose in place)
        td = dict({kk: v.clone() for kk, v in base.items()}, **dev)
        th = dict({kk: v.clone() for kk, v in base.items()}, **{kk: torch.from_numpy(v).cuda() for kk, v in hpack.items()})
        if bs_d is None:
            wl = [dict(w, laser_frame=np.ones(1, np.int32), laser_pts=np.zeros((1, 12))) for w in wins]
            bs_d, bs_h = liw.BatchSolver(prm, wl), liw.BatchSolver(prm, wl)
        for bs, t in ((bs_d, td), (bs_h, th)):
            bs.rebind(t, Ltot)
            bs.solve(liw.LIW_MODE_TRACK)
            bs.marginalize()
        torch.cuda.synchronize()
        assert torch.equal(bs_d.t["has_prior"], bs_h.t["has_prior"])
        for name in ("x", "prior_X", "prior_J", "prior_R"):
            a, h = bs_d.t[name], bs_h.t[name]
            assert torch.isfinite(a).all(), (k, name)
            rel = float((a - h).abs().max() / h.abs().max().clamp_min(1e-300))
            d_state = max(d_state, rel)
            assert rel <= 1e-6, (k, name, rel)
    print("end to end: %d robots x %d frames; laser end points max |device - host| %.3e, states / priors max rel. difference %.3e"
          % (B, F, d_pts, d_state))


@pytest.mark.parametrize("B", [1025, 1])
def test_pack_track_offsets(env, B):
    """pack_track on its own: laser_off is the exclusive cumulative sum of the counts clamped to [0, cap], Ltot its last element,
    and laser_frame / laser_pts hold the records in robot order.  B = 1025 gives a thread of the one-block scan more than one
    robot and is no multiple of its 1 024 threads; counts below 0 and above cap hit both clamps."""
    liw, lp, sc, torch = env
    cap, n, frame = 4, 2, 1
    fe = liw.laser_batch.BatchFrontEnd(lp, dict(B=B, slots=1, max_points=8, max_lines=4, max_cell_entries=16))
    rng = np.random.default_rng(650 + B)
    count = rng.choice(np.array([-3, 0, 1, 4, 9], dtype=np.int32), B)
    if B > 1:
        assert (count < 0).any() and (count > cap).any()
    recs, pose = rng.standard_normal((B, cap, 12)), rng.standard_normal((B, 12))
    m = dict(count=torch.from_numpy(count).cuda(), recs=torch.from_numpy(recs).cuda(), match_pose=torch.from_numpy(pose).cuda(), cap=cap)
    pk, Ltot = fe.pack_track(m, n=n, frame=frame)
    torch.cuda.synchronize()
    kept = np.clip(count, 0, cap)
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(kept)
    assert np.array_equal(pk["laser_off"].cpu().numpy(), off)
    assert Ltot == int(off[-1])
    rows = np.concatenate([recs[b, :kept[b]] for b in range(B)], 0)          # [Ltot, 12] in robot order
    if Ltot:
        assert np.array_equal(pk["laser_frame"].cpu().numpy(), np.full(Ltot, frame, dtype=np.int32))
        assert np.array_equal(pk["laser_pts"].cpu().numpy().reshape(12, Ltot), rows.T)
    else:   # the one entry kept so that no array is empty
        assert pk["laser_frame"].numel() == 1 and pk["laser_pts"].numel() == 12
    assert np.array_equal(pk["match_pose"].cpu().numpy().reshape(B, n, 12)[:, frame], pose)
    assert np.array_equal(pk["has_match"].cpu().numpy().reshape(B, n)[:, frame], np.ones(B, dtype=np.uint8))
    fe.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_scale_determinism(env):
    liw, lp, sc, torch = env
    B, nd = 4096, 64
    rng = np.random.default_rng(700)
    pa = np.stack([_pose(rng) for _ in range(nd)])
    pb = np.stack([_pose(rng, pa[j], 0.2, np.deg2rad(6)) for j in range(nd)])
    la = [sc.points(j, pa[j], seed=j)[0] for j in range(nd)]
    lb_ = [sc.points(j, pb[j], seed=nd + j)[0] for j in range(nd)]
    rob = np.arange(B) % nd
    Pa, na = liw.laser_batch.pad_points([la[j] for j in rob], N_RAYS)
    Pb, nb_ = liw.laser_batch.pad_points([lb_[j] for j in rob], N_RAYS)
    fe = _fe(liw, lp, B)

    def run():
        fe.reset()
        fe.spawn(0, torch.from_numpy(Pa).cuda(), torch.from_numpy(na).cuda())
        fe.add_scan(0, pa[rob])
        fe.spawn(1, torch.from_numpy(Pb).cuda(), torch.from_numpy(nb_).cuda())
        m = fe.match_with_ref(1, pb[rob], cap=256)
        pk, Lt = fe.pack_track(m)
        torch.cuda.synchronize()
        return fe.store.clone(), {k: v.clone() for k, v in m.items() if k != "cap"}, {k: v.clone() for k, v in pk.items()}, Lt

    s1, m1, k1, L1 = run()
    s2, m2, k2, L2 = run()
    assert L1 == L2 and torch.equal(s1, s2)
    for k in m1:
        assert torch.equal(m1[k], m2[k]), k
    for k in k1:
        assert torch.equal(k1[k], k2[k]), k
    o = _np(m1)
    for b in rng.choice(B, 16, replace=False):
        j = rob[b]
        h = liw.laser.LaserManager(lp)
        h.add_scan(liw.laser.Scan.spawn(lp, la[j]), pa[j, :3], pa[j, 3:])
        hmt = h.match_with_ref(liw.laser.Scan.spawn(lp, lb_[j]), pb[j, :3], pb[j, 3:])
        _compare_match(hmt, o, b, ("scale", b))
    assert L1 == int(o["count"].sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ 8
def test_capacity_flags_and_guards(env):
    liw, lp, sc, torch = env
    lb = liw.laser_batch
    rng = np.random.default_rng(800)
    B = 16
    p1 = np.stack([_pose(rng) for _ in range(B)])
    p2 = np.stack([_pose(rng, p1[b], 0.1, np.deg2rad(3)) for b in range(B)])
    l1 = [sc.points(b, p1[b], seed=b)[0] for b in range(B)]
    l2 = [sc.points(b, p2[b], seed=B + b)[0] for b in range(B)]
    small = set(range(0, B, 2))                  # these robots see one short wall: few lines, few cells
    for b in small:
        for lst in (l1, l2):
            keep = np.abs(lst[b][:, 1] - np.median(lst[b][:, 1])) < 10
            lst[b] = lst[b][keep][:40]
    G = 4096

    def run(max_lines, max_cells, cap):
        fe = _fe(liw, lp, B, max_lines=max_lines, max_cell_entries=max_cells)
        nbytes = fe.store.numel()
        big = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        fe.store = big[G:G + nbytes]
        fe.reset()
        for slot, lists in ((0, l1), (1, l2)):
            P, n = lb.pad_points(lists, N_RAYS)
            fe.spawn(slot, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())
        fe.add_scan(0, p1)
        gb = lambda *s, dt: torch.full((int(np.prod(s)) + 2 * 64,), 7, dtype=dt, device="cuda")
        bufs = dict(count=gb(B, dt=torch.int32), recs=gb(B, cap, 12, dt=torch.float64), idx1=gb(B, cap, dt=torch.int32), idx2=gb(B, cap, dt=torch.int32),
                    match_pose=gb(B, 12, dt=torch.float64))
        shapes = dict(count=(B,), recs=(B, cap, 12), idx1=(B, cap), idx2=(B, cap), match_pose=(B, 12))
        out = {k: v[64:-64].view(*shapes[k]) for k, v in bufs.items()}
        m = fe.match(lb.REF, 1, None, p2, cap=cap, out=out)
        torch.cuda.synchronize()
        assert (big[:G] == 0xA5).all() and (big[-G:] == 0xA5).all()
        for k, v in bufs.items():
            assert (v[:64] == 7).all() and (v[-64:] == 7).all(), k
        st = [fe.status(b) for b in range(B)]
        ref = [fe.get_lines(b, lb.REF) for b in range(B)]
        return _np({k: m[k] for k in ("count", "recs", "idx1", "idx2", "match_pose")}), st, ref

    mL, stL, refL = run(256, 8192, 256)
    assert all(s == 0 for s in stL)
    assert all(mL["count"][b] > 0 for b in range(1, B, 2))
    for max_lines, max_cells, cap in ((8, 8192, 256), (256, 300, 256), (256, 8192, 4)):
        mS, stS, refS = run(max_lines, max_cells, cap)
        flagged = [b for b in range(B) if stS[b]]
        assert flagged and set(flagged).isdisjoint(small), (max_lines, max_cells, cap, flagged)
        for b in range(B):
            if stS[b]:
                assert mS["count"][b] == 0
                continue
            n = int(mL["count"][b])
            assert mS["count"][b] == n and n <= cap
            assert np.array_equal(mS["recs"][b, :n], mL["recs"][b, :n]) and np.array_equal(mS["idx1"][b, :n], mL["idx1"][b, :n])
            assert np.array_equal(mS["match_pose"][b], mL["match_pose"][b])
            assert np.array_equal(refS[b], refL[b])


def test_overflowed_scans_never_match(env):
    """a points overflow invalidates the scan spawned from it, and an invalid scan given to add_scan invalidates the sub-maps it
    writes: every match against them has count 0, while the other robots still equal the host"""
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=4)   # the reference survives the second add_scan (office's 2 drops it there)
    lb = liw.laser_batch
    B, MP = 16, 400
    rng = np.random.default_rng(900)
    pa = np.stack([_pose(rng) for _ in range(B)])
    pb = np.stack([_pose(rng, pa[b], 0.1, np.deg2rad(3)) for b in range(B)])

    def sparse(r):                        # 300 rays: fewer kept points than MP
        r = r.copy()
        r[:400] = np.inf
        r[700:] = np.inf
        return r
    RA = np.stack([sc.ranges(b, pa[b], seed=b) if b % 2 else sparse(sc.ranges(b, pa[b], seed=b)) for b in range(B)])
    lists_b = [liw.laser.laser_to_points(sparse(sc.ranges(b, pb[b], seed=B + b)), ANG_MIN, ANG_INC, T_INC, 0.0)[0] for b in range(B)]
    odd = [b for b in range(B) if b % 2]
    fe = _fe(liw, lp, B, max_points=MP)
    pts, times, n = fe.ranges_to_points(torch.from_numpy(RA), np.zeros(B))
    nh = n.cpu().numpy()
    for b in range(B):
        hp, _ = liw.laser.laser_to_points(RA[b], ANG_MIN, ANG_INC, T_INC, 0.0)
        if b % 2:
            assert hp.shape[0] > MP and nh[b] == MP + 1 and fe.status(b) & lb.ST_POINTS
            assert np.array_equal(pts[b].cpu().numpy(), hp[:MP])
        else:
            assert nh[b] == hp.shape[0] <= MP and fe.status(b) == 0
    fe.spawn(0, pts, n)
    P1, n1 = lb.pad_points(lists_b, MP)
    fe.spawn(1, torch.from_numpy(P1).cuda(), torch.from_numpy(n1).cuda())
    for b in range(B):
        assert (fe.status(b, 0) != 0) == (b % 2 == 1) and fe.status(b, 1) == 0
        if b % 2:
            assert fe.num_lines(b, 0) == 0
    o = _np(fe.match(0, 1, pa, pb))
    hA = [liw.laser.Scan.spawn(lp, liw.laser.laser_to_points(RA[b], ANG_MIN, ANG_INC, T_INC, 0.0)[0]) for b in range(B)]
    hB = [liw.laser.Scan.spawn(lp, lists_b[b]) for b in range(B)]
    for b in range(B):
        if b % 2:
            assert o["count"][b] == 0
        else:
            _compare_match(liw.laser.do_match(lp, hA[b], hB[b], pa[b, :3], pa[b, 3:], pb[b, :3], pb[b, 3:]), o, b, ("direct", b))
    # the overflowed scan goes into add_scan: the reference sub-map it creates is invalid
    fe.add_scan(0, pa)
    hm = [liw.laser.LaserManager(lp) for _ in range(B)]
    for b in range(B):
        hm[b].add_scan(hA[b], pa[b, :3], pa[b, 3:])
        st = fe.status(b, lb.REF)
        assert (st & lb.ST_INVALID and st & lb.ST_POINTS) if b % 2 else st == 0, (b, st)
    total = 0
    for step in range(2):                 # the valid scan accumulated into an invalid reference leaves it invalid
        o = _np(fe.match_with_ref(1, pb))
        for b in range(B):
            h = hm[b].match_with_ref(hB[b], pb[b, :3], pb[b, 3:])
            if b % 2:
                assert o["count"][b] == 0, (step, b)
                assert np.array_equal(o["match_pose"][b, :6], pa[b]), (step, b)   # the (invalid) reference exists
            else:
                _compare_match(h, o, b, ("ref", step, b))
                total += len(h)
        fe.add_scan(1, pb)
        for b in range(B):
            hm[b].add_scan(hB[b], pb[b, :3], pb[b, 3:])
    assert total > 0
    assert all(fe.status(b) & lb.ST_INVALID for b in odd)
