"""The batched laser front-end on the device at the SECOND laser set (tests/second_config.py: a 138 x 83 grid that the rooms leave
in one direction, no two scalars equal, ref_n_accumulation = 5, the generic laser extrinsic of skewed_params) against the host
front-end liw.laser, which tests/test_second_config_frontend.py ties to the oracle on the same inputs and shows to move under every
single exchanged or office-valued parameter.  Bars of tests/test_gpu_laser_batch.py: lines and match records 1e-9, every count, index
list, cell, flag and match_pose exact; the two spawn kernels and the two add_scan kernels agree in their store bytes.

24 robots (six rooms x four poses), 1080 rays, max_lines 256, max_cell_entries 8192, 16 frames."""
import numpy as np
import pytest

import second_config as sc
from test_gpu_laser_add_scan_wave import _assert_same_state, _host_machine, _mgr
from test_gpu_laser_batch import Scene, _compare_lines, _compare_match, _np, _pose
from test_gpu_laser_spawn_wave import _close, assert_slots_equal

pytestmark = pytest.mark.gpu

B, F = len(sc.ROOMS) * sc.POSES_PER_ROOM, sc.FRAMES
N_RAYS, MC = sc.N_RAYS, 64


def _dims(slots):
    return dict(B=B, slots=slots, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)


@pytest.fixture(scope="module")
def env(liw, synth):
    import torch
    S = sc.laser_scene(liw, synth)
    host = [[liw.laser.Scan.spawn(S["lp"], S["points"][b][k]) for k in range(F)] for b in range(B)]
    return liw, torch, S, S["lp"], host


def _frame(liw, torch, S, k):
    P, n = liw.laser_batch.pad_points([S["points"][b][k] for b in range(B)], N_RAYS)
    return torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda()


def _kernels(mp, spawn="wave", add="wave"):
    for var, v in (("LIW_LFE_SPAWN", spawn), ("LIW_LFE_ADD_SCAN", add)):      # both are read per call
        if v == "lane":
            mp.setenv(var, "lane")
        else:
            mp.delenv(var, raising=False)


def _snap(torch, fe):
    torch.cuda.synchronize()
    return fe.store.cpu().numpy().copy()


def _front_end(liw, lp, slots=2):
    fe = liw.laser_batch.BatchFrontEnd(lp, _dims(slots))
    fe.set_geometry(N_RAYS, sc.ANG_MIN, sc.ANG_INC, sc.T_INC)
    return fe


# ------------------------------------------------------------------------------------------------------------------ spawn
def _spawn_run(liw, torch, S, lp, kernel):
    with pytest.MonkeyPatch.context() as mp:
        _kernels(mp, spawn=kernel)
        fe = _front_end(liw, lp)
        dP, dn = _frame(liw, torch, S, 0)
        cor = fe.spawn(0, dP, dn, corners=MC if kernel == "wave" else None)
        return fe, _snap(torch, fe), cor


def test_spawn_both_kernels(env):
    liw, torch, S, lp, host = env
    fe, wave, (cor, ncor) = _spawn_run(liw, torch, S, lp, "wave")
    fel, lane, _ = _spawn_run(liw, torch, S, lp, "lane")
    cor, ncor = cor.cpu().numpy(), ncor.cpu().numpy()
    worst, cells, outside, low, corners, min_lines = 0.0, 0, 0, 0, 0, 10 ** 9
    for b in range(B):
        pts, hs = S["points"][b][0], host[b][0]
        hl = hs.lines()
        min_lines = min(min_lines, hl.shape[0])
        for f in (fe, fel):
            assert f.status(b, 0) == 0 and f.status(b) == 0
            worst = max(worst, _compare_lines(hl, f.get_lines(b, 0), ("spawn", b)))   # scan::lines order
        gx, gy, w, h = sc.grid_coordinates(lp, pts)
        edge = (gx < 0) | (gy < 0) | (gx >= w) | (gy >= h)              # outside the grid, or inside through the truncation toward zero
        for i in sorted(set(range(0, len(pts), 3)) | set(np.nonzero(edge)[0][::4])):
            x, y = pts[i, :2]
            kh, ih = hs.cell_lines(x, y, 64)
            kd, idv = fe.cell_lines(b, 0, x, y, 64)
            assert kh == kd and np.array_equal(ih, idv), (b, i, x, y, kh, kd, ih, idv)
            cells += 1
            outside += kh < 0
            low += bool(edge[i]) and kh >= 0
        hc = hs.concers()
        assert ncor[b] == hc.shape[0] and np.array_equal(cor[b, :ncor[b]], hc), (b, ncor[b], hc.shape[0])
        corners += hc.shape[0]
    valid, lines = assert_slots_equal(wave, lane, _dims(2), B, 0, "second set")
    print("spawn at the second set: %d scans, at least %d lines each, max |device - host| %.3e; %d cells equal, %d of them outside the grid, "
          "%d in row / column 0 from a coordinate in (-1, 0); %d corners equal; wave == lane in %d slots, %d lines"
          % (B, min_lines, worst, cells, outside, low, corners, valid, lines))
    assert min_lines >= sc.MIN_LINES and valid == B
    assert outside >= 100 and low >= 5 and corners >= 1
    fe.close()
    fel.close()


# ------------------------------------------------------------------------------------------------------------------ match
@pytest.mark.parametrize("kk", [0, 1])
def test_match(env, kk):
    liw, torch, S, lp, host = env
    with pytest.MonkeyPatch.context() as mp:
        _kernels(mp)
        fe = _front_end(liw, lp)
        for slot in (0, 1):
            fe.spawn(slot, *_frame(liw, torch, S, slot))
        p1 = S["poses"][:, 0]
        p2 = S["poses"][:, 1] + sc.MATCH_GUESS
        o = _np(fe.match(0, 1, p1, p2, kk=kk, cap=256))
    worst, total, fewest = 0.0, 0, 10 ** 9
    for b in range(B):
        hm = liw.laser.do_match(lp, host[b][0], host[b][1], p1[b, :3], p1[b, 3:], p2[b, :3], p2[b, 3:], kk)
        worst = max(worst, _compare_match(hm, o, b, ("match", kk)))
        total += len(hm)
        fewest = min(fewest, len(hm))
    print("match kk=%d at the second set: %d pairs, at least %d a robot, max |device - host| %.3e" % (kk, total, fewest, worst))
    assert fewest >= sc.MIN_BACK_MATCHES
    fe.close()


# ------------------------------------------------------------------------------------------------------------------ manager sequence
def _sequence(liw, torch, S, lp, kernel, host=None):
    """16 frames of spawn, match_with_ref, add_scan under one add_scan kernel -> dict(match, flags, snaps, packs); with `host` (the
    wave run) every frame is compared with one host LaserManager per robot while the device state is there"""
    lb = liw.laser_batch
    dims = _dims(2)
    out = dict(match=[], flags=[], snaps=[], packs=[], worst=0.0, pairs=0, refs=0, cells=0, back=10 ** 9)
    mgrs = [liw.laser.LaserManager(lp) for _ in range(B)] if host else None
    with pytest.MonkeyPatch.context() as mp:
        _kernels(mp, add=kernel)
        fe = _front_end(liw, lp)
        for k in range(F):
            pose = S["poses"][:, k]
            fe.spawn(0, *_frame(liw, torch, S, k))
            m = fe.match_with_ref(0, pose, cap=256)
            if k:                                                  # the match with the scan before it, still in slot 1
                mb = _np(fe.match(1, 0, S["poses"][:, k - 1], pose, cap=256))
                out["back"] = min(out["back"], int(mb["count"].min()))
            pk, Ltot = fe.pack_track(m, n=2, frame=1)
            torch.cuda.synchronize()
            o = _np(m)
            out["match"].append(o)
            out["packs"].append(({kk: v.cpu().numpy().copy() for kk, v in pk.items()}, Ltot))
            fl = fe.add_scan(0, pose, flags=True)
            assert fe.add_scan_path() == (0 if kernel == "lane" else 1)
            out["flags"].append(fl.cpu().numpy().copy())
            out["snaps"].append(_snap(torch, fe))
            if host:
                for b in range(B):
                    hs = host[b][k]
                    h = mgrs[b].match_with_ref(hs, pose[b, :3], pose[b, 3:])
                    out["worst"] = max(out["worst"], _compare_match(h, o, b, ("ref", k)))
                    out["pairs"] += len(h)
                    if k:
                        hb = mgrs[b].match_with_back(hs, pose[b, :3], pose[b, 3:])
                        out["worst"] = max(out["worst"], _compare_match(hb, mb, b, ("back", k)))
                    mgrs[b].add_scan(hs, pose[b, :3], pose[b, 3:])
                    r = mgrs[b].ref_scan()
                    dl = fe.get_lines(b, lb.REF)
                    assert r is not None and dl is not None, (k, b)
                    out["worst"] = max(out["worst"], _compare_lines(r[0].lines(), dl, ("ref lines", k, b)))
                    p, q = fe.submap_pose(b)
                    assert np.array_equal(p, r[1]) and np.array_equal(q, r[2]), (k, b)
                    assert fe.status(b) == 0 and fe.status(b, lb.REF) == 0
                    for x, y, _z in S["points"][b][k][::16]:       # the reference sub-map's grid under the scan just added
                        kh, ih = r[0].cell_lines(x, y, 64)
                        kd, idv = fe.cell_lines(b, lb.REF, x, y, 64)
                        assert kh == kd and np.array_equal(ih, idv), (k, b, x, y, kh, kd)
                        out["cells"] += 1
                    out["refs"] += 1
            fe.slot_copy(np.ones(B, dtype=np.int32))               # the scan becomes "the scan before" of the next frame
        fe.close()
    return out


@pytest.fixture(scope="module")
def sequences(env):
    liw, torch, S, lp, host = env
    return _sequence(liw, torch, S, lp, "wave", host), _sequence(liw, torch, S, lp, "lane")


def test_manager_sequence_both_kernels(env, sequences):
    liw, torch, S, lp, host = env
    lb = liw.laser_batch
    w, l = sequences
    dims = _dims(2)
    full, margin, seen = 0, np.inf, dict(filtered=0, first=0, spawned=0, swapped=0)
    machine = [_host_machine(lb, S["poses"][b], lp["ref_n_accumulation"], lp["ref_motion_filter_p"], lp["ref_motion_filter_q"]) for b in range(B)]
    for k in range(F):
        full += _assert_same_state(w["snaps"][k], l["snaps"][k], dims, ("second set, frame", k))
        assert np.array_equal(w["flags"][k], l["flags"][k]), k
        for key in ("count", "recs", "idx1", "idx2", "match_pose"):
            assert np.array_equal(w["match"][k][key], l["match"][k][key]), (k, key)
        for b in range(B):
            flags, states, m = machine[b]
            margin = min(margin, m)
            fl = int(w["flags"][k][b])
            assert fl == flags[k], (b, k, fl, flags[k])
            g = _mgr(w["snaps"][k], dims, b)
            assert (g["has_ref"], g["has_spawn"], g["count"]) == states[k], (b, k, g, states[k])
            seen["filtered"] += fl == 0
            seen["first"] += bool(fl & lb.ADD_FIRST)
            seen["spawned"] += bool(fl & lb.ADD_SPAWNED)
            seen["swapped"] += bool(fl & lb.ADD_SWAPPED)
    for b in range(B):                                                 # the two frames between the motion filter's thresholds
        assert int(w["flags"][sc.F_SMALL_P][b]) == 0 and int(w["flags"][sc.F_SMALL_Q][b]) & lb.ADD_ADDED, b
    print("manager at the second set (n_acc = 5): %d robot-frames, %d match pairs, %d reference sub-maps and %d of their cells equal to the host, "
          "max |device - host| %.3e, fewest matches with the scan before %d; %s; wave == lane in %d sub-maps; closest step to a filter threshold %.3e"
          % (B * F, w["pairs"], w["refs"], w["cells"], w["worst"], w["back"], seen, full, margin))
    assert w["refs"] == B * F and full == 2 * B * F
    assert seen["filtered"] >= B and seen["first"] == B and seen["spawned"] == B and seen["swapped"] >= 3 * B   # the 2 / 3 cycle turns over
    assert w["back"] >= sc.MIN_BACK_MATCHES and margin > 1e-6


def test_packed_tracking_input(env, sequences):
    """liw_lfe_pack_* of frame 1: the device pack equals a numpy pack of the records it was given, bit for bit, and the pack of the
    host front-end's matches in structure, its end points within the bar of the records"""
    liw, torch, S, lp, host = env
    w, _ = sequences
    o, (pk, Ltot) = w["match"][1], w["packs"][1]
    cnt = o["count"].astype(np.int32)
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum(cnt)
    recs = np.concatenate([o["recs"][b, :cnt[b]] for b in range(B)], 0)
    mp = np.zeros((B, 2, 12))
    mp[:, 1] = o["match_pose"]
    hmask = np.zeros((B, 2), dtype=np.uint8)
    hmask[:, 1] = 1
    want = dict(laser_off=off, laser_frame=np.ones(Ltot, dtype=np.int32), laser_pts=np.ascontiguousarray(recs.T).reshape(-1), match_pose=mp.reshape(-1),
                has_match=hmask.reshape(-1))
    assert Ltot == int(off[-1]) >= sc.MIN_BACK_MATCHES * B
    for k, v in want.items():
        assert np.array_equal(pk[k], v), k
    mgr = [liw.laser.LaserManager(lp) for _ in range(B)]
    hrecs = []
    for b in range(B):
        mgr[b].add_scan(host[b][0], S["poses"][b, 0, :3], S["poses"][b, 0, 3:])
        hrecs.append(mgr[b].match_with_ref(host[b][1], S["poses"][b, 1, :3], S["poses"][b, 1, 3:]).pts)
    assert [r.shape[0] for r in hrecs] == cnt.tolist()
    d = float(np.abs(np.ascontiguousarray(np.concatenate(hrecs, 0).T).reshape(-1) - pk["laser_pts"]).max())
    print("pack of frame 1: %d records, arrays equal to the numpy pack; end points against the host front-end's %.3e" % (Ltot, d))
    assert d <= 1e-9


def test_second_run_is_bit_identical(env, sequences):
    liw, torch, S, lp, host = env
    w, _ = sequences
    again = _sequence(liw, torch, S, lp, "wave")
    for k in range(F):
        assert np.array_equal(w["snaps"][k], again["snaps"][k]), k
        assert np.array_equal(w["flags"][k], again["flags"][k]), k
        for key in ("count", "recs", "idx1", "idx2", "match_pose"):
            assert np.array_equal(w["match"][k][key], again["match"][k][key]), (k, key)
        assert w["packs"][k][1] == again["packs"][k][1]
        for key, v in w["packs"][k][0].items():
            assert np.array_equal(v, again["packs"][k][0][key]), (k, key)
    fe1, s1, (c1, n1) = _spawn_run(liw, torch, S, lp, "wave")
    fe2, s2, (c2, n2) = _spawn_run(liw, torch, S, lp, "wave")
    assert np.array_equal(s1, s2) and torch.equal(c1, c2) and torch.equal(n1, n2)
    fe1.close()
    fe2.close()


# ------------------------------------------------------------------------------------------------------------------ rebuild
def test_rebuild_in_one_launch_at_n_acc_5(env):
    """liw_lfe_rebuild of eight frames at ref_n_accumulation = 5 (spawn at count 2, hand-overs at 5 and 8) over a manager state from
    before: one launch of the wave kernel == the lane kernel == a cleared manager and eight single calls == the host manager"""
    liw, torch, S, lp, host = env
    lb = liw.laser_batch
    FR = 8
    dims = _dims(FR + 1)
    x = torch.zeros(B, FR + 2, 15, dtype=torch.float64, device="cuda")
    x[:, 1:1 + FR, :6] = torch.from_numpy(np.ascontiguousarray(S["poses"][:, :FR])).cuda()
    x[:, :, 6:] = 7.0

    def prepared(mp, before):
        _kernels(mp)
        fe = _front_end(liw, lp, FR + 1)
        for k in range(FR):
            fe.spawn(1 + k, *_frame(liw, torch, S, k))
        if before:
            _kernels(mp, add="lane")
            for s in (5, 2, 4):
                fe.add_scan(s, S["poses"][:, FR + s])
        return fe

    with pytest.MonkeyPatch.context() as mp:
        few = prepared(mp, True)
        _kernels(mp)
        few.rebuild(1, FR, x[:, 1:1 + FR])
        assert few.add_scan_path() == 1
        one = _snap(torch, few)
        fel = prepared(mp, True)
        _kernels(mp, add="lane")
        fel.rebuild(1, FR, x[:, 1:1 + FR])
        assert fel.add_scan_path() == 0
        lane = _snap(torch, fel)
        fes = prepared(mp, False)
        _kernels(mp)
        for k in range(FR):
            fes.add_scan(1 + k, S["poses"][:, k])
        single = _snap(torch, fes)
    n1 = _assert_same_state(one, lane, dims, "rebuild at n_acc 5: one launch vs lane")
    n2 = _assert_same_state(one, single, dims, "rebuild at n_acc 5: one launch vs eight calls on a cleared manager")
    worst = 0.0
    for b in range(B):
        mgr = liw.laser.LaserManager(lp)
        for k in range(FR):
            mgr.add_scan(host[b][k], S["poses"][b, k, :3], S["poses"][b, k, 3:])
        r = mgr.ref_scan()
        worst = max(worst, _compare_lines(r[0].lines(), few.get_lines(b, lb.REF), ("rebuild", b)))
        p, q = few.submap_pose(b)
        assert np.array_equal(p, r[1]) and np.array_equal(q, r[2])
        g = _mgr(one, dims, b)
        assert (g["has_ref"], g["has_spawn"]) == (1, 1) and g["count"] in (2, 3, 4)
    print("rebuild at n_acc = 5: %d / %d sub-maps equal the lane rebuild / eight single calls; reference lines against the host %.3e" % (n1, n2, worst))
    assert n1 == n2 == 2 * B
    for f in (few, fel, fes):
        f.close()


# ------------------------------------------------------------------------------------------------------------------ corners_to_world
def test_corners_to_world_at_the_skewed_extrinsic(env, synth):
    """make_tf(pose) * T_imu_to_laser * c against numpy: T_w_i from synth.exp_so3, T_il as the library holds it (the loader's round
    trip of a matrix that is a per cent off orthonormal), poses with roll and pitch; bar of test_corners_to_world, 1e-12 relative"""
    liw, torch, S, lp, host = env
    rng = np.random.default_rng(77)
    Til = S["Til"]
    assert np.abs(Til[:3, :3] - np.asarray(lp["T_imu_to_laser"]).reshape(4, 4)[:3, :3]).max() > 1e-3     # the round trip did work
    CAP = 256
    fe = _front_end(liw, lp, 1)
    acc = torch.zeros(B, CAP, 3, dtype=torch.float64, device="cuda")
    n_acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    want = [np.zeros((0, 3)) for _ in range(B)]
    worst, appended, from_scans = 0.0, 0, 0
    for k in range(4):
        if k < 2:                                                      # the corners the spawn kernel found
            cor, ncor = fe.spawn(0, *_frame(liw, torch, S, k), corners=MC)
            from_scans += int(ncor.sum())
        else:                                                          # corners anywhere, z included
            nc = rng.integers(0, MC + 1, B).astype(np.int32)
            cor = torch.from_numpy(rng.uniform(-6.0, 6.0, (B, MC, 3))).cuda()
            ncor = torch.from_numpy(nc).cuda()
        pose = S["poses"][:, k].copy()
        pose[:, 2] = rng.uniform(-0.1, 0.1, B)
        pose[:, 3:5] = rng.uniform(-0.3, 0.3, (B, 2))
        clear = np.array([1 if (k == 2 and b % 3 == 0) else 0 for b in range(B)], dtype=np.uint8)
        fe.corners_to_world(cor, ncor, pose, acc, n_acc, clear=clear)
        c_h, n_h = cor.cpu().numpy(), ncor.cpu().numpy()
        da, dn = acc.cpu().numpy(), n_acc.cpu().numpy()
        for b in range(B):
            if clear[b]:
                want[b] = np.zeros((0, 3))
            T = sc.pose_T(synth, pose[b]) @ Til
            want[b] = np.concatenate([want[b], c_h[b, :n_h[b]] @ T[:3, :3].T + T[:3, 3]])
            appended += int(n_h[b])
            assert dn[b] == want[b].shape[0], (k, b)
            worst = max(worst, _close(da[b, :dn[b]], want[b]))
    print("corners_to_world at the skewed extrinsic: %d corners appended (%d from scans), max relative difference %.3e" % (appended, from_scans, worst))
    assert appended > 20 * B and from_scans >= 1 and all(fe.status(b) == 0 for b in range(B))
    fe.close()


# ------------------------------------------------------------------------------------------------------------------ contexts
def test_no_stale_parameters_across_front_ends(env):
    """a front-end at the office set, closed, one at the second set, closed, the office one again, in one process: the third equals the
    first byte for byte and the second meets the host (no parameter survives in a constant or a cached launch argument)"""
    liw, torch, S, lp, host = env
    lb = liw.laser_batch
    off = liw.laser.office_laser_params()
    scn = Scene(liw, off)
    rng = np.random.default_rng(31)
    pa = np.stack([_pose(rng) for _ in range(B)])
    pb = np.stack([_pose(rng, pa[b], 0.2, np.deg2rad(6)) for b in range(B)])
    la = [scn.points(b % 6, pa[b], seed=b)[0] for b in range(B)]
    lb_ = [scn.points(b % 6, pb[b], seed=B + b)[0] for b in range(B)]
    Pa, na = lb.pad_points(la, N_RAYS)
    Pb, nb = lb.pad_points(lb_, N_RAYS)

    def office():
        fe = _front_end(liw, off)
        fe.spawn(0, torch.from_numpy(Pa).cuda(), torch.from_numpy(na).cuda())
        fe.add_scan(0, pa)
        fe.spawn(1, torch.from_numpy(Pb).cuda(), torch.from_numpy(nb).cuda())
        m = _np(fe.match_with_ref(1, pb, cap=256))
        store = _snap(torch, fe)
        fe.close()
        return store, m

    def second():
        fe = _front_end(liw, lp)
        fe.spawn(0, *_frame(liw, torch, S, 0))
        fe.add_scan(0, S["poses"][:, 0])
        fe.spawn(1, *_frame(liw, torch, S, 1))
        m = _np(fe.match_with_ref(1, S["poses"][:, 1], cap=256))
        lines = [fe.get_lines(b, 1) for b in range(B)]
        fe.close()
        return m, lines

    with pytest.MonkeyPatch.context() as mp:
        _kernels(mp)
        s1, m1 = office()
        m2, lines2 = second()
        s3, m3 = office()
    assert np.array_equal(s1, s3)
    for key in ("count", "recs", "idx1", "idx2", "match_pose"):
        assert np.array_equal(m1[key], m3[key]), key
    assert int(m1["count"].sum()) > 4 * B
    worst = 0.0
    for b in range(B):
        worst = max(worst, _compare_lines(host[b][1].lines(), lines2[b], ("second set between two office front-ends", b)))
        mgr = liw.laser.LaserManager(lp)
        mgr.add_scan(host[b][0], S["poses"][b, 0, :3], S["poses"][b, 0, 3:])
        worst = max(worst, _compare_match(mgr.match_with_ref(host[b][1], S["poses"][b, 1, :3], S["poses"][b, 1, 3:]), m2, b, "between"))
    print("office, second set, office in one process: stores and matches of the two office runs equal; the second set against the host %.3e" % worst)
