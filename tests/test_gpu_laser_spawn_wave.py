"""The wave-per-scan spawn kernel of the batched laser front-end and the corners it delivers (liw_lfe_spawn_corners,
liw_lfe_corners_to_world).  References: the host front-end (liw.laser, tied to the oracle by the CPU tests) for the corners, and
the lane-per-scan kernel kept behind LIW_LFE_SPAWN=lane for the store bytes; never the new kernel's own output."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_MIN, N_RAYS = np.float32(-2.0 * np.pi * 0.75 / 2), 1080
ANG_INC = np.float32(2.0 * np.pi * 0.75 / (N_RAYS - 1))
T_INC = np.float32(1.0 / (40.0 * N_RAYS))
HDR, MGR = 32, 256


def _rot(q):
    th = np.linalg.norm(q)
    if th < 1e-15:
        return np.eye(3)
    k = np.asarray(q) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _T(pose):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(np.asarray(pose[3:], dtype=np.float64)), pose[:3]
    return T


def _points(liw, segs, T_w_l, seed):
    r, _, _ = liw.laser.cast_scan(segs, T_w_l, n_rays=N_RAYS, seed=seed)
    return liw.laser.laser_to_points(r, ANG_MIN, ANG_INC, T_INC, 0.0)


def zigzag_segments(teeth=120, r0=2.2, r1=2.6):
    """a closed zig-zag ring around the origin: `teeth` flanks alternating between radius r0 and r1 (the flanks meet at about 35
    degrees, inside the corner gate)"""
    th = 2 * np.pi * np.arange(teeth + 1) / teeth
    r = np.where(np.arange(teeth + 1) % 2 == 0, r0, r1)
    v = np.stack([r * np.cos(th), r * np.sin(th)], 1)
    return [(v[k].copy(), v[k + 1].copy()) for k in range(teeth)]


def room_scans(liw, lp, rooms, per_room, seed):
    """per_room scans of each room at random poses -> list of point arrays [m, 3]"""
    rng = np.random.default_rng(seed)
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    out = []
    for room in rooms:
        segs = liw.laser.room_segments(room)
        for k in range(per_room):
            pose = np.concatenate([rng.uniform(-1.0, 1.0, 2), [0.0, 0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
            out.append(_points(liw, segs, _T(pose) @ Til, seed=1000 * room + k)[0])
    return out


def pillar_poses(n):
    """IMU poses on the pillar room's circle (centre (0, 5), radius 5), heading along it"""
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([5 * np.cos(a), 5 + 5 * np.sin(a), 0 * a, 0 * a, 0 * a, a + np.pi / 2], 1)


def pillar_scans(liw, lp, poses, seed=0):
    from importlib import import_module
    replay = import_module(liw.__name__ + ".replay")
    segs = replay.pillar_room()
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    return [_points(liw, segs, _T(p) @ Til, seed=seed + k)[0] for k, p in enumerate(poses)]


def zigzag_scan(liw):
    return _points(liw, zigzag_segments(), np.eye(4), seed=5)[0]


def host_margins(lines):
    """smallest distance (radians) of any line pair's angle from 30 / 150 degrees, and of any line's len from 0.1"""
    if lines.shape[0] == 0:
        return np.inf, np.inf
    d = lines[:, 0:3] - lines[:, 3:6]
    n = np.linalg.norm(d, axis=1)
    ok = n > 0
    u = d[ok] / n[ok, None]
    ang = np.arccos(np.clip(u @ u.T, -1, 1))[np.triu_indices(u.shape[0], 1)]
    ma = min(np.abs(ang - np.deg2rad(30)).min(), np.abs(ang - np.deg2rad(150)).min()) if ang.size else np.inf
    return float(ma), float(np.abs(lines[:, 9] - 0.1).min())


def slot_parts(store, dims, b, slot):
    """(header bytes [32], lines [max_lines, 10] float64, entries [max_cell_entries] uint64) of a scan slot, from the store as a
    numpy uint8 array (the layout of include/liw_laser_batch.h's store: robot-major, 256-byte manager record, then the slots)"""
    ml, me, slots = dims["max_lines"], dims["max_cell_entries"], dims["slots"]
    sb = (HDR + 80 * ml + 8 * me + 255) // 256 * 256
    rb = MGR + (slots + 2) * sb
    o = b * rb + MGR + slot * sb
    hdr = store[o:o + HDR]
    lines = store[o + HDR:o + HDR + 80 * ml].view(np.float64).reshape(ml, 10)
    ent = store[o + HDR + 80 * ml:o + HDR + 80 * ml + 8 * me].view(np.uint64)
    return hdr, lines, ent


def assert_slots_equal(store_w, store_l, dims, B, slot, what):
    """valid slots bitwise equal in header, lines[:n_lines], entries[:n_entries]; invalid slots invalid in both, sharing a bit"""
    valid = lines = 0
    for b in range(B):
        hw, lw, ew = slot_parts(store_w, dims, b, slot)
        hl, ll, el = slot_parts(store_l, dims, b, slot)
        sw, sl = int(hw[:4].view(np.int32)[0]), int(hl[:4].view(np.int32)[0])
        if sl:
            assert sw and (sw & sl), (what, b, sw, sl)
            continue
        assert np.array_equal(hw, hl), (what, b, hw.view(np.int32), hl.view(np.int32))
        nl, ne = int(hl[4:8].view(np.int32)[0]), int(hl[8:12].view(np.int32)[0])
        assert np.array_equal(lw[:nl].view(np.uint64), ll[:nl].view(np.uint64)), (what, b, "lines")
        assert np.array_equal(ew[:ne], el[:ne]), (what, b, "entries")
        valid += 1
        lines += nl
    return valid, lines


@pytest.fixture(scope="module")
def env(liw):
    import torch
    lp = liw.laser.office_laser_params()
    return liw, lp, torch


def _dims(B, slots=2, max_points=N_RAYS, max_lines=256, max_cell_entries=8192):
    return dict(B=B, slots=slots, max_points=max_points, max_lines=max_lines, max_cell_entries=max_cell_entries)


def _fe(liw, lp, dims):
    return liw.laser_batch.BatchFrontEnd(lp, dims)


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ------------------------------------------------------------------------------------------------------------------ 1
def test_corners_equal_host(env, monkeypatch):
    liw, lp, torch = env
    monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
    rooms = room_scans(liw, lp, range(12), 4, seed=41)
    pillars = pillar_scans(liw, lp, pillar_poses(12))
    lists = rooms + pillars + [zigzag_scan(liw)]
    B, MC = len(lists), 256
    dims = _dims(B)
    fe = _fe(liw, lp, dims)
    P, n = liw.laser_batch.pad_points(lists, N_RAYS)
    dP, dn = _dev(torch, P, n)
    cor, ncor = fe.spawn(0, dP, dn, corners=MC)
    cor, ncor = cor.cpu().numpy(), ncor.cpu().numpy()
    with_corner, total, m_ang, m_len = 0, 0, np.inf, np.inf
    for b in range(B):
        hs = liw.laser.Scan.spawn(lp, lists[b])
        hc = hs.concers()
        a, l = host_margins(hs.lines())
        m_ang, m_len = min(m_ang, a), min(m_len, l)
        assert fe.status(b, 0) == 0 and fe.status(b) == 0, b
        assert ncor[b] == hc.shape[0], (b, ncor[b], hc.shape[0])
        assert np.array_equal(cor[b, :ncor[b]], hc), b
        with_corner += hc.shape[0] > 0
        total += hc.shape[0]
        if len(rooms) <= b < len(rooms) + len(pillars):
            assert hc.shape[0] >= 3, (b, hc.shape[0])
    zl, zc = fe.num_lines(B - 1, 0), int(ncor[B - 1])
    print("corners: %d scans, %d with a host corner, %d corners; zig-zag %d lines %d corners; margins: angle %.3e rad, len %.3e"
          % (B, with_corner, total, zl, zc, m_ang, m_len))
    assert with_corner >= 0.9 * B
    assert zl > 64 and zc > 64
    assert m_ang > 1e-9 and m_len > 1e-9


# ------------------------------------------------------------------------------------------------------------------ 2
def _edge_lists(liw, lp, MP):
    rng = np.random.default_rng(77)
    wall = np.stack([np.linspace(-2, 2, 300), np.full(300, 1.5) + rng.normal(0, 0.002, 300), np.zeros(300)], 1)
    arc = np.stack([2 * np.cos(np.linspace(0, 2, 400)), 2 * np.sin(np.linspace(0, 2, 400)), np.zeros(400)], 1)
    pairs = []
    for k in range(60):                      # runs of 2 points, 0.5 m apart: every run shorter than the step
        x = -3 + 0.5 * k
        pairs += [[x, 1.0, 0.0], [x + 0.02, 1.0, 0.0]]
    trip = np.array([[1.0, 0.0, 0.0], [1.0, 0.05, 0.0], [1.0, 0.1, 0.0]])
    rooms = [p[:MP] for p in room_scans(liw, lp, range(20, 32), 4, seed=43)]
    assert sum(p.shape[0] == MP for p in rooms) >= 8          # n_pts == max_points
    base = room_scans(liw, lp, [33, 34, 35], 1, seed=44)
    times = np.linspace(0.0, 0.025, base[0].shape[0])
    skew = liw.laser.laser_correct(base[0], times, 0.0, np.array([0.8, -0.3, 0.2]), np.array([0.5, -0.7, 0.9]))[:MP]
    assert np.abs(skew[:, 2]).max() > 1e-4                       # de-skewed: z != 0
    nan_scan, inf_scan = base[1][:MP].copy(), base[2][:MP].copy()
    nan_scan[500, 0] = np.nan
    inf_scan[300, 1] = np.inf
    lists = rooms + [np.zeros((0, 3)), trip[:1], trip[:2], trip, wall, arc, np.array(pairs), zigzag_scan(liw)[:MP], skew, nan_scan, inf_scan,
                     rooms[0], rooms[1]]
    n_override = {len(lists) - 2: -1, len(lists) - 1: MP + 1}
    return lists, n_override


def test_store_bytes_equal_lane_kernel(env, monkeypatch):
    liw, lp, torch = env
    MP = 1000                                                      # not a multiple of 64
    lists, n_override = _edge_lists(liw, lp, MP)
    B = len(lists)
    assert B % 64                                                  # the lane kernel's last work-group is partly empty
    dims = _dims(B, max_points=MP)
    P, n = liw.laser_batch.pad_points(lists, MP)
    for b, v in n_override.items():
        n[b] = v
    times = np.random.default_rng(5).uniform(0, 10, B)
    dP, dn, dt = _dev(torch, P, n, times)
    stores = {}
    for mode in ("lane", "wave", "corners"):
        fe = _fe(liw, lp, dims)
        if mode == "lane":
            monkeypatch.setenv("LIW_LFE_SPAWN", "lane")
        else:
            monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
        fe.spawn(1, dP, dn, dt, corners=256 if mode == "corners" else None)
        torch.cuda.synchronize()
        stores[mode] = fe.store.cpu().numpy().copy()
        if mode == "lane":                                         # the lane kernel knows no corners: an error, not a fall-back
            with pytest.raises(liw.LiwError) as e:
                fe.spawn(0, dP, dn, dt, corners=256)
            assert e.value.code == -22
    valid, lines = assert_slots_equal(stores["wave"], stores["lane"], dims, B, 1, "wave")
    assert_slots_equal(stores["corners"], stores["lane"], dims, B, 1, "corners")
    print("store bytes: %d scans, %d valid, %d lines compared" % (B, valid, lines))
    assert valid == B - 2 and lines > 20 * 48
    zz = B - 6                                                     # the zig-zag scan: more candidate segments than lanes
    assert int(slot_parts(stores["lane"], dims, zz, 1)[0][4:8].view(np.int32)[0]) > 64


# ------------------------------------------------------------------------------------------------------------------ 3
def test_matches_unchanged_downstream(env, monkeypatch):
    liw, lp0, torch = env
    lp = dict(lp0, ref_n_accumulation=4)
    B, F = 24, 5
    rng = np.random.default_rng(300)
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    poses = np.zeros((F, B, 6))
    poses[0] = np.stack([np.concatenate([rng.uniform(-1, 1, 2), [0, 0, 0], rng.uniform(-np.pi, np.pi, 1)]) for _ in range(B)])
    for k in range(1, F):
        poses[k] = poses[k - 1]
        poses[k, :, :2] += rng.uniform(-0.15, 0.15, (B, 2))
        poses[k, :, 5] += rng.uniform(-0.07, 0.07, B)
    segs = [liw.laser.room_segments(60 + b) for b in range(B)]
    frames = [liw.laser_batch.pad_points([_points(liw, segs[b], _T(poses[k, b]) @ Til, seed=100 * k + b)[0] for b in range(B)], N_RAYS) for k in range(F)]
    outs = {}
    for mode in ("lane", "wave"):
        if mode == "lane":
            monkeypatch.setenv("LIW_LFE_SPAWN", "lane")
        else:
            monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
        fe = _fe(liw, lp, _dims(B))
        rec = []
        for k in range(F):
            dP, dn = _dev(torch, *frames[k])
            fe.spawn(k % 2, dP, dn)
            m = fe.match_with_ref(k % 2, poses[k])
            rec.append({kk: v.clone() for kk, v in m.items() if kk != "cap"})
            if k:
                d = fe.match((k - 1) % 2, k % 2, poses[k - 1], poses[k], kk=1)
                rec.append({kk: v.clone() for kk, v in d.items() if kk != "cap"})
            fe.add_scan(k % 2, poses[k])
        torch.cuda.synchronize()
        outs[mode] = (rec, [fe.get_lines(b, liw.laser_batch.REF) for b in range(B)], [fe.status(b) for b in range(B)])
    pairs = 0
    for a, b in zip(outs["wave"][0], outs["lane"][0]):
        for k in a:
            assert torch.equal(a[k], b[k]), k
        pairs += int(a["count"].sum())
    for a, b in zip(outs["wave"][1], outs["lane"][1]):
        assert np.array_equal(a, b)
    assert outs["wave"][2] == outs["lane"][2] == [0] * B
    assert pairs > 4 * B * F


# ------------------------------------------------------------------------------------------------------------------ 4
def test_capacity_flags_and_guards(env, monkeypatch):
    liw, lp, torch = env
    lb = liw.laser_batch
    monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
    B, G = 16, 4096
    pp = pillar_poses(B)
    pp2 = pp.copy()
    pp2[:, :2] += 0.05
    l1, l2 = pillar_scans(liw, lp, pp, seed=0), pillar_scans(liw, lp, pp2, seed=100)
    small = set(range(0, B, 2))                  # these robots see one short wall: one line, few cells, no corner
    rng = np.random.default_rng(800)
    for b in small:
        for lst, y in ((l1, 1.5), (l2, 1.45)):
            lst[b] = np.stack([np.linspace(-0.5, 0.5, 40), np.full(40, y) + rng.normal(0, 0.002, 40), np.zeros(40)], 1)
    host = [liw.laser.Scan.spawn(lp, l1[b]).concers() for b in range(B)]
    assert all(host[b].shape[0] == 0 for b in small) and all(host[b].shape[0] >= 3 for b in range(1, B, 2))

    def run(max_lines, max_cells, MC):
        dims = _dims(B, max_lines=max_lines, max_cell_entries=max_cells)
        fe = _fe(liw, lp, dims)
        nbytes = fe.store.numel()
        big = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        big[G:G + nbytes] = 0
        fe.store = big[G:G + nbytes]
        fe.reset()
        gc = torch.full((B * MC * 3 + 128,), 7.0, dtype=torch.float64, device="cuda")
        gn = torch.full((B + 128,), 7, dtype=torch.int32, device="cuda")
        out = (gc[64:-64].view(B, MC, 3), gn[64:-64])
        P1, n1 = lb.pad_points(l1, N_RAYS)
        P2, n2 = lb.pad_points(l2, N_RAYS)
        cor, ncor = fe.spawn(0, *_dev(torch, P1, n1), corners=MC, out=out)
        fe.spawn(1, *_dev(torch, P2, n2))
        fe.add_scan(0, pp)
        m = fe.match_with_ref(1, pp2)
        torch.cuda.synchronize()
        assert (big[:G] == 0xA5).all() and (big[-G:] == 0xA5).all()
        assert (gc[:64] == 7).all() and (gc[-64:] == 7).all() and (gn[:64] == 7).all() and (gn[-64:] == 7).all()
        m = {k: v.cpu().numpy() for k, v in m.items() if k != "cap"}
        st = [(fe.status(b), fe.status(b, 0), fe.status(b, 1)) for b in range(B)]
        return m, st, cor.cpu().numpy().copy(), ncor.cpu().numpy().copy(), fe.store.cpu().numpy().copy(), dims

    mL, stL, cL, nL, storeL, dimsL = run(256, 8192, 256)
    assert all(s == (0, 0, 0) for s in stL)
    assert all(mL["count"][b] > 0 for b in range(1, B, 2))
    for b in range(B):
        assert nL[b] == host[b].shape[0] and np.array_equal(cL[b, :nL[b]], host[b]), b

    def same_as_large(mS, b):
        n = int(mL["count"][b])
        assert mS["count"][b] == n
        for k in ("recs", "idx1", "idx2"):
            assert np.array_equal(mS[k][b, :n], mL[k][b, :n]), (k, b)
        assert np.array_equal(mS["match_pose"][b], mL["match_pose"][b])

    for max_lines, max_cells, bit in ((8, 8192, lb.ST_LINES), (256, 300, lb.ST_CELLS)):
        mS, stS, cS, nS, storeS, dimsS = run(max_lines, max_cells, 256)
        flagged = [b for b in range(B) if stS[b][0]]
        assert flagged and set(flagged).isdisjoint(small), (bit, flagged)
        for b in range(B):
            if stS[b][0]:
                assert stS[b][0] & bit and (stS[b][1] & bit or stS[b][2] & bit), (b, stS[b])
                assert mS["count"][b] == 0
                if stS[b][1]:
                    assert nS[b] == 0
                continue
            same_as_large(mS, b)
            assert nS[b] == nL[b] and np.array_equal(cS[b, :nS[b]], cL[b, :nL[b]])
            for slot in (0, 1):
                hs, ls, es = slot_parts(storeS, dimsS, b, slot)
                hl, ll, el = slot_parts(storeL, dimsL, b, slot)
                nl, ne = int(hl[4:8].view(np.int32)[0]), int(hl[8:12].view(np.int32)[0])
                assert np.array_equal(hs, hl) and np.array_equal(ls[:nl], ll[:nl]) and np.array_equal(es[:ne], el[:ne]), (b, slot)
    MC = 2
    mS, stS, cS, nS, storeS, dimsS = run(256, 8192, MC)
    flagged = [b for b in range(B) if stS[b][0]]
    assert flagged == [b for b in range(B) if host[b].shape[0] > MC] and flagged
    for b in range(B):
        same_as_large(mS, b)                        # the slot stays valid
        assert stS[b][1] == 0 and stS[b][2] == 0
        if b in flagged:
            assert stS[b][0] == lb.ST_CORNERS and nS[b] == MC + 1
            assert np.array_equal(cS[b], host[b][:MC])
        else:
            assert stS[b][0] == 0 and nS[b] == host[b].shape[0] and np.array_equal(cS[b, :nS[b]], host[b])


# ------------------------------------------------------------------------------------------------------------------ 5
def test_determinism_4096(env, monkeypatch):
    liw, lp, torch = env
    monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
    B, nd, MC = 4096, 32, 64
    base = room_scans(liw, lp, range(100, 100 + nd - 8), 1, seed=45) + pillar_scans(liw, lp, pillar_poses(8), seed=50)
    rob = np.arange(B) % nd
    P, n = liw.laser_batch.pad_points([base[j] for j in rob], N_RAYS)
    dP, dn = _dev(torch, P, n)
    fe = _fe(liw, lp, _dims(B, slots=1))

    def run():
        fe.reset()
        c, k = fe.spawn(0, dP, dn, corners=MC)
        torch.cuda.synchronize()
        return fe.store.clone(), c.clone(), k.clone()

    s1, c1, k1 = run()
    s2, c2, k2 = run()
    assert torch.equal(s1, s2) and torch.equal(c1.view(torch.int64), c2.view(torch.int64)) and torch.equal(k1, k2)
    c1, k1 = c1.cpu().numpy(), k1.cpu().numpy()
    for b in np.random.default_rng(1).choice(B, 16, replace=False):
        hc = liw.laser.Scan.spawn(lp, base[rob[b]]).concers()
        assert k1[b] == hc.shape[0] and np.array_equal(c1[b, :k1[b]], hc), b
    assert int(k1.sum()) > B


# ------------------------------------------------------------------------------------------------------------------ 6
def _host_world(liw, pose, Til12, corners):
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    A, T = np.zeros(12), np.zeros(12)
    p, q = np.ascontiguousarray(pose[:3], dtype=np.float64), np.ascontiguousarray(pose[3:], dtype=np.float64)
    L.liw_lie_make_tf(pd(p), pd(q), pd(A))
    L.liw_lie_mul(pd(A), pd(Til12), pd(T))
    out = np.zeros((corners.shape[0], 3))
    for i in range(corners.shape[0]):
        c, y = np.ascontiguousarray(corners[i]), np.zeros(3)
        L.liw_lie_apply(pd(T), pd(c), pd(y))
        out[i] = y
    return out


def _close(d, h, bound=1e-12):
    assert d.shape == h.shape, (d.shape, h.shape)
    if h.size == 0:
        return 0.0
    rel = float(np.abs(d - h).max() / np.abs(h).max())
    assert rel <= bound, rel
    return rel


def test_corners_to_world(env, synth, monkeypatch):
    liw, lp0, torch = env
    lb = liw.laser_batch
    monkeypatch.delenv("LIW_LFE_SPAWN", raising=False)
    lp = dict(lp0, normalize_extrinsics=False)    # the host below multiplies by T_imu_to_laser exactly as given
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    Til12 = np.ascontiguousarray(np.concatenate([Til[:3, :3].reshape(9), Til[:3, 3]]))
    B, F, MC, CAP = 8, 9, 64, 256
    a0 = 2 * np.pi * np.arange(B) / B
    poses = np.zeros((F, B, 6))
    for k in range(F):
        a = a0 + 0.12 * k
        poses[k] = np.stack([5 * np.cos(a), 5 + 5 * np.sin(a), 0 * a, 0 * a, 0 * a, a + np.pi / 2], 1)
    fe = _fe(liw, lp, _dims(B, slots=1))
    acc = torch.zeros(B, CAP, 3, dtype=torch.float64, device="cuda")
    n_acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    hacc = [np.zeros((0, 3)) for _ in range(B)]
    is_kf = lambda k, b: (k + b) % 3 == 2          # the frame is a key frame: its accumulated corners are handed over
    masked = lambda k, b: b == 3 and k % 2 == 1    # robot 3 does not track on odd frames
    kf_dev, kf_host, worst, appended = [], [], 0.0, 0
    for k in range(F):
        lists = pillar_scans(liw, lp, poses[k], seed=10 * k)
        P, n = lb.pad_points(lists, N_RAYS)
        cor, ncor = fe.spawn(0, *_dev(torch, P, n), corners=MC)
        mask = np.array([0 if masked(k, b) else 1 for b in range(B)], dtype=np.uint8)
        clear = np.array([1 if k and is_kf(k - 1, b) else 0 for b in range(B)], dtype=np.uint8)
        fe.corners_to_world(cor, ncor, poses[k], acc, n_acc, mask=mask, clear=clear)
        da, dn = acc.cpu().numpy(), n_acc.cpu().numpy()
        for b in range(B):
            if clear[b]:
                hacc[b] = np.zeros((0, 3))
            if mask[b]:
                hc = liw.laser.Scan.spawn(lp, lists[b]).concers()
                hacc[b] = np.concatenate([hacc[b], _host_world(liw, poses[k, b], Til12, hc)])
                appended += hc.shape[0]
            assert dn[b] == hacc[b].shape[0], (k, b, dn[b], hacc[b].shape[0])
            worst = max(worst, _close(da[b, :dn[b]], hacc[b]))
        if is_kf(k, 0):
            kf_dev.append((poses[k, 0], da[0, :dn[0]].copy()))
            kf_host.append((poses[k, 0], hacc[0].copy()))
    assert appended > 3 * B * F // 2 and len(kf_dev) >= 3 and all(c.shape[0] for _, c in kf_host)
    assert all(fe.status(b) == 0 for b in range(B))
    # the key frames of robot 0 through two loop detectors
    p = liw.loop.office_loop_params()
    dets = [liw.loop.LoopDetector(synth.office_params(), p, dict(max_keyframes=16, max_points=512)) for _ in range(2)]
    for det, kfs in zip(dets, (kf_dev, kf_host)):
        for pose, c in kfs:
            det.add_keyframe(_T(pose), c)
            det.detect()
    assert dets[0].num_keyframes() == dets[1].num_keyframes() == len(kf_dev)
    for i in range(len(kf_dev)):
        worst = max(worst, _close(dets[0].get_points(i), dets[1].get_points(i)))
    print("corners_to_world: %d corners appended, %d key frames, max relative difference %.3e" % (appended, len(kf_dev), worst))
    # overflow of acc_cap: flagged, nothing written outside (or at all)
    SC = 5
    g = torch.full((B * SC * 3 + 128,), 7.0, dtype=torch.float64, device="cuda")
    gn = torch.full((B + 128,), 7, dtype=torch.int32, device="cuda")
    sacc, sn = g[64:-64].view(B, SC, 3), gn[64:-64]
    sn.zero_()
    hn = np.zeros(B, dtype=np.int64)
    nc = ncor.cpu().numpy()
    for rep in range(3):
        before = g.clone()
        fe.corners_to_world(cor, ncor, poses[F - 1], sacc, sn)
        torch.cuda.synchronize()
        for b in range(B):
            over = hn[b] > SC or (nc[b] > 0 and hn[b] + nc[b] > SC)
            if over:
                assert torch.equal(sacc[b], before[64:-64].view(B, SC, 3)[b]), (rep, b)
            hn[b] = SC + 1 if over else hn[b] + nc[b]
        assert np.array_equal(sn.cpu().numpy(), hn), (rep, sn.cpu().numpy(), hn)
        assert (g[:64] == 7).all() and (g[-64:] == 7).all() and (gn[:64] == 7).all() and (gn[-64:] == 7).all()
    assert (hn == SC + 1).any()
    for b in range(B):
        assert (fe.status(b) == lb.ST_CORNERS) == (hn[b] == SC + 1), b
