"""The fleet's occupancy-grid maps on the MI355X (include/liw_map_batch.h).  Every grid comparison is exact: zero differing cells,
and equal width, height, origin, rays, samples and four counts.  The per-robot checkers are gridmap.GridMap (the single-robot
kernels) and the literal serial walk of tests/map_reference.py.  Covered: the store (counts, offsets, points, `full`, masks, guard
bytes, LIW_EINVAL), parity per robot at three resolutions, the edge cases of tests/test_gpu_map.py inside one fleet, the capacity
statuses, isolation and determinism of a robot's region, render from poses, render behind a FleetBackEnd solve, and push behind a
free-running tracker."""
import ctypes as C

import numpy as np
import pytest

import map_batch_cases as mc
import map_reference as ref

pytestmark = pytest.mark.gpu
RES = mc.RES
LIW_EINVAL = -22
OK, EMPTY, OVER_CELLS, RAY_TOO_LONG = 0, 1, 2, 3


def _rows(fm):
    return fm.status.cpu().numpy().copy(), fm.infos()


# ------------------------------------------------------------------------------------------------------------------ 1. store
def test_store(liw, synth):
    import torch
    B, K, P, stride = 5, 4, 40, 16
    fm = mc.mapper(liw, synth, B, K, P, 1024, 64)
    lay = fm.lay
    rng = np.random.default_rng(1)
    mask = np.array([1, 1, 1, 0, 1], np.uint8)
    fresh = mc.regions(fm)
    #           robot 0: 8 points every frame   1: 15, 15, 15, then 5   2: every other frame, an empty and a negative count
    keys = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0], [1, 0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]], np.uint8)
    counts = np.array([[8, 8, 8, 8, 8, 8], [15, 15, 15, 5, 0, 0], [5, 9, 0, 9, -3, 9], [4, 4, 4, 4, 4, 4], [7, 7, 7, 7, 7, 7]], np.int32)
    want_added = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0], [9, 9, 9, 9, 9, 9], [0, 0, 0, 0, 0, 0]], np.uint8)
    stored = [[] for _ in range(B)]
    before_full = {}
    for f in range(6):
        pts = rng.uniform(-3, 3, (B, stride, 3))
        fm.added.fill_(9)   # a masked-out robot's row is not written
        added = fm.add_keyframes(keys[:, f], pts, counts[:, f], mask=mask).cpu().numpy()
        assert added.tolist() == want_added[:, f].tolist(), f
        for b in range(B):
            if added[b] == 1:
                stored[b].append(pts[b, :max(int(counts[b, f]), 0)].copy())
        if f == 3:      # robot 0 holds max_submaps, robot 1 was refused at max_points in frame 2 and offered a scan that fits in frame 3
            before_full = {0: mc.regions(fm)[0], 1: mc.regions(fm)[1]}
            assert fm.is_full(1) and not fm.is_full(0)
    reg = mc.regions(fm)
    assert [fm.num_submaps(b) for b in range(B)] == [4, 2, 3, 0, 0]
    assert [fm.is_full(b) for b in range(B)] == [True, True, False, False, False]
    # a full robot keeps its bytes but for the flag (int32 word 1 of the header)
    for b in (0, 1):
        a, c = before_full[b].copy(), reg[b].copy()
        a[4:8] = c[4:8] = 0
        assert a.tobytes() == c.tobytes()
    for b in range(B):
        n = [len(s) for s in stored[b]]
        off = reg[b, lay["offsets_off"]:lay["offsets_off"] + 4 * (len(n) + 1)].view(np.int32)
        assert off.tolist() == np.concatenate([[0], np.cumsum(n)]).astype(int).tolist()
        for k, s in enumerate(stored[b]):
            got = fm.submap(b, k)
            assert got.shape == s.shape and got.tobytes() == s.tobytes()
        idx = reg[b, lay["index_off"]:lay["index_off"] + 4 * sum(n)].view(np.int32)
        assert idx.tolist() == [k for k, m in enumerate(n) for _ in range(m)]
    assert [len(s) for s in stored[2]] == [5, 0, 0]
    assert reg[3].tobytes() == fresh[3].tobytes()          # masked out in every frame
    assert reg[4].tobytes() == fresh[4].tobytes()          # key never set
    G = fm.guard
    assert G >= 64 and bool((fm._buf[:G] == 0xA5).all()) and bool((fm._buf[-G:] == 0xA5).all())

    # LIW_EINVAL: nothing is written
    L, h = fm.L, fm.h
    vp = lambda t: C.c_void_p(t.data_ptr())
    key, n = torch.ones(B, dtype=torch.uint8, device="cuda"), torch.full((B,), 3, dtype=torch.int32, device="cuda")
    pts = torch.zeros(B, stride, 3, dtype=torch.float64, device="cuda")
    tfs = torch.zeros(B, K, 12, dtype=torch.float64, device="cuda")
    fm.added.fill_(9)
    fm.status.fill_(77)
    fm.info.fill_(0x5A)
    torch.cuda.synchronize()
    snap = fm._buf.cpu().numpy().copy()
    st, mis = vp(fm.store), C.c_void_p(fm.store.data_ptr() + 4)
    a, s, i = vp(fm.added), vp(fm.status), vp(fm.info)
    calls = [lambda: L.liw_fmap_reset(h, None, None, None), lambda: L.liw_fmap_reset(h, mis, None, None),
             lambda: L.liw_fmap_add_keyframes(h, None, vp(key), vp(pts), stride, vp(n), None, a, None),
             lambda: L.liw_fmap_add_keyframes(h, mis, vp(key), vp(pts), stride, vp(n), None, a, None),
             lambda: L.liw_fmap_add_keyframes(h, st, None, vp(pts), stride, vp(n), None, a, None),
             lambda: L.liw_fmap_add_keyframes(h, st, vp(key), None, stride, vp(n), None, a, None),
             lambda: L.liw_fmap_add_keyframes(h, st, vp(key), vp(pts), stride, None, None, a, None),
             lambda: L.liw_fmap_add_keyframes(h, st, vp(key), vp(pts), 0, vp(n), None, a, None)]
    for fn in (L.liw_fmap_render_tf, L.liw_fmap_render):
        calls += [lambda fn=fn: fn(h, None, vp(tfs), 12 * K, None, s, i, None), lambda fn=fn: fn(h, mis, vp(tfs), 12 * K, None, s, i, None),
                  lambda fn=fn: fn(h, st, None, 12 * K, None, s, i, None), lambda fn=fn: fn(h, st, vp(tfs), -1, None, s, i, None),
                  lambda fn=fn: fn(h, st, vp(tfs), 12 * K, None, None, i, None), lambda fn=fn: fn(h, st, vp(tfs), 12 * K, None, s, None, None)]
    for k, call in enumerate(calls):
        assert call() == LIW_EINVAL, k
    for robot in (-1, B):
        assert L.liw_fmap_num_submaps(h, st, robot) == LIW_EINVAL and L.liw_fmap_full(h, st, robot) == LIW_EINVAL
        assert L.liw_fmap_get_submap(h, st, robot, 0, 0, None) == LIW_EINVAL and L.liw_fmap_get_tf(h, st, robot, 0, None) == LIW_EINVAL
        assert L.liw_fmap_last_info(h, st, robot, None, None) == LIW_EINVAL and L.liw_fmap_get(h, st, robot, None, 0) == LIW_EINVAL
        assert L.liw_fmap_write_pgm(h, st, robot, b"x", None) == LIW_EINVAL and L.liw_fmap_device_data(h, st, robot) is None
    assert L.liw_fmap_get_submap(h, st, 0, 4, 0, None) == LIW_EINVAL     # robot 0 holds sub-maps 0 .. 3
    assert L.liw_fmap_device_data(h, st, 1) == fm.store.data_ptr() + lay["robot_bytes"] + lay["grid_off"]
    torch.cuda.synchronize()
    assert fm._buf.cpu().numpy().tobytes() == snap.tobytes()
    assert bool((fm.added == 9).all()) and bool((fm.status == 77).all()) and bool((fm.info == 0x5A).all())
    # a masked reset empties exactly the masked robots
    fm.reset(mask=np.array([0, 1, 0, 0, 0], np.uint8))
    assert [fm.num_submaps(b) for b in range(B)] == [4, 0, 3, 0, 0] and not fm.is_full(1) and fm.is_full(0)
    after = mc.regions(fm)
    assert all(after[b].tobytes() == reg[b].tobytes() for b in (0, 2, 3, 4))
    fm.close()


# ------------------------------------------------------------------------------------------------------------------ 2. parity
_PARITY = {}


def _parity_case():
    """B = 6 robots with 0, 1, 2, 3, 5, 8 sub-maps of 24 - 40 rays; the last robot sees one place twice (cells hit once and twice)"""
    if not _PARITY:
        rng = np.random.default_rng(21)
        rooms = mc.rooms(6)
        tfs_of, subs_of = [], []
        for b, K in enumerate((0, 1, 2, 3, 5, 8)):
            t, s = mc.room_case(rng, K, (24, 40), room=rooms[b])
            tfs_of.append(t)
            subs_of.append(s)
        subs_of[5][1], tfs_of[5][1] = subs_of[5][0].copy(), tfs_of[5][0].copy()
        _PARITY.update(tfs_of=tfs_of, subs_of=subs_of)
    return _PARITY["tfs_of"], _PARITY["subs_of"]


@pytest.mark.parametrize("res", [0.05, 0.1, 0.03])
def test_parity_per_robot(liw, synth, res, tmp_path):
    tfs_of, subs_of = _parity_case()
    B = len(subs_of)
    fm = mc.mapper(liw, synth, B, 8, 8 * 40, 1 << 19, 2048, res=res)
    mc.load(fm, subs_of)
    fm.render_tf(mc.pad_tfs(tfs_of, 8))
    status, rows = _rows(fm)
    assert status.tolist() == [EMPTY] + [OK] * 5
    for b in range(B):
        want = ref.render(tfs_of[b], subs_of[b], res)
        mc.assert_robot(fm, b, want, rows[b])
        single = liw.gridmap.GridMap(synth.office_params(), dict(resolution=res), dict(max_submaps=8, max_points=8 * 40, max_cells=1 << 19))
        for k, s in enumerate(subs_of[b]):
            assert single.add_submap(s) == k
        assert single.render_tf(tfs_of[b]) == rows[b]
        assert np.array_equal(single.grid(), fm.grid(b))
        if b == 5 and res == 0.05:
            assert all(want["counts"][v] > 0 for v in (-1, 0, 50, 100)), want["counts"]
            fm.write_pgm(b, tmp_path / "fleet", palette=(205, 254, 100, 0))      # the file pair of the single map, byte for byte
            single.write_pgm(tmp_path / "single", palette=(205, 254, 100, 0))
            assert (tmp_path / "fleet.pgm").read_bytes() == (tmp_path / "single.pgm").read_bytes()
            assert (tmp_path / "fleet.yaml").read_text() == (tmp_path / "single.yaml").read_text().replace("single.pgm", "fleet.pgm")
            assert fm.device_data(b) == fm.store.data_ptr() + b * fm.lay["robot_bytes"] + fm.lay["grid_off"]
    fm.close()


# ------------------------------------------------------------------------------------------------------------------ 3. edge cases
def test_edge_cases_share_a_launch(liw, synth):
    rng = np.random.default_rng(4)
    ident = np.array([mc.tf12(0.0, 0.0, 0.0)])
    # robot 0: the emit origin one cell left of / below the box: quotients in (-1, 0) land in column / row 0
    n = 40
    trunc = np.stack([rng.uniform(0.03, 3.0, n), rng.uniform(0.02, 2.0, n), rng.uniform(-0.01, 0.01, n)], axis=1)
    trunc[0], trunc[1] = (0.03, 1.0, 0.0), (1.0, 0.02, 0.0)
    # robots 1, 2: ray lengths T[k] and one ulp either side, k inside and beyond the LDS part of the table (1 536 entries)
    T = liw.gridmap.step_table(RES, 2000)
    edge = []
    for k in (1, 2, 6, 7, 40, 777, 1535, 1536, 1537, 1900):
        for v in (T[k], np.nextafter(T[k], 0.0), np.nextafter(T[k], np.inf)):
            edge += [(v, 0.0, 0.0), (0.0, -v, 0.0)]     # identity transform: len = sqrt(v * v) = v
    edge = np.array(edge)
    general = np.array([mc.tf12(1.3, -0.7, 0.61, 0.02, 0.01, -0.02)])
    # robot 3: NaN / inf points and a point at its origin among valid ones
    odd = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [np.nan, 0.2, 0.0], [0.5, np.inf, 0.0], [2.0, -1.0, 0.0], [-np.inf, np.nan, 1.0]])
    odd_tf = np.array([mc.tf12(0.4, -0.2, 0.3)])
    # robot 4: no sub-map; robot 5: only invalid points; robot 6: the zero-length ray alone
    tfs_of = [ident, ident, general, odd_tf, np.zeros((0, 12)), odd_tf, odd_tf]
    subs_of = [[trunc], [edge], [edge], [odd], [], [np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])], [np.zeros((1, 3))]]
    B = len(subs_of)
    fm = mc.mapper(liw, synth, B, 2, 64, 1 << 21, 2048)
    mc.load(fm, subs_of)
    fm.render_tf(mc.pad_tfs(tfs_of, 2))
    status, rows = _rows(fm)
    assert status.tolist() == [OK, OK, OK, OK, EMPTY, EMPTY, OK]
    wants = [ref.render(t, s, RES) for t, s in zip(tfs_of, subs_of)]
    assert wants[0]["neg_col0"] > 0 and wants[0]["neg_row0"] > 0
    assert wants[3]["rays"] == 3 and wants[6]["samples"] == 0 and wants[6]["counts"][50] == 1
    for b in (4, 5):
        assert (wants[b]["width"], wants[b]["height"], wants[b]["rays"]) == (0, 0, 0) and fm.grid(b).size == 0
    for b in range(B):
        mc.assert_robot(fm, b, wants[b], rows[b])
    fm.close()


# ------------------------------------------------------------------------------------------------------------------ 4. capacity
def _box(tfs, subs, res):
    """width, height, origin and rays of the bounding box, with the arithmetic of include/liw_map.h"""
    P = [ref.world_point([float(v) for v in T], pt) for T, s in zip(tfs, subs) for pt in np.asarray(s).reshape(-1, 3)]
    xs, ys = [p[0] for p in P], [p[1] for p in P]
    return dict(width=int((max(xs) - min(xs)) / res + 1), height=int((max(ys) - min(ys)) / res + 1), origin_x=min(xs), origin_y=min(ys), rays=len(P))


def test_capacity(liw, synth):
    rng = np.random.default_rng(31)
    rooms = mc.rooms(4)
    B, K, steps, cells = 4, 3, 1024, 1 << 18
    cases = [mc.room_case(rng, 2, 30, room=rooms[b]) for b in range(B)]
    tfs_of, subs_of = [c[0] for c in cases], [c[1] for c in cases]
    limit = (steps - 2) * RES / 2            # 25.55 m
    far = np.array([[limit + 0.4, 0.3, 0.0]])
    # second round: robot 1's sub-maps lie 40 m apart (the box needs about a million cells), robot 3 gets a key frame with a ray too long
    tfs2 = [t.copy() for t in tfs_of]
    tfs2[1][1, 9:11] += 40.0
    tfs2[0][:, 9] += 0.37        # the healthy robots' poses move too
    tfs2[2][1, 10] -= 0.81
    tfs2[3] = np.concatenate([tfs_of[3], [mc.tf12(0.0, 5.0, 0.2)]])
    subs2 = [list(s) for s in subs_of]
    subs2[3] = subs2[3] + [far]
    box1, box3 = _box(tfs2[1], subs2[1], RES), _box(tfs2[3], subs2[3], RES)
    assert box1["width"] * box1["height"] > cells >= box3["width"] * box3["height"]

    def run(failing):
        fm = mc.mapper(liw, synth, B, K, 200, cells, steps)
        mc.load(fm, subs_of)
        fm.render_tf(mc.pad_tfs(tfs_of, K))
        first = mc.regions(fm)
        st1, _ = _rows(fm)
        assert st1.tolist() == [OK] * 4
        if failing:
            fm.add_keyframes(np.array([0, 0, 0, 1], np.uint8), np.broadcast_to(far, (B, 1, 3)).copy(), np.ones(B, np.int32))
        fm.status.fill_(77)
        fm.info.fill_(0x5A)
        sel = np.array([1, 1, 1, 1] if failing else [1, 0, 1, 0], np.uint8)
        t2 = tfs2 if failing else [tfs2[0], tfs_of[1], tfs2[2], tfs_of[3]]
        fm.render_tf(mc.pad_tfs(t2, K), sel=sel)
        return fm, first, mc.regions(fm), _rows(fm)
    fm, first, second, (status, rows) = run(True)
    assert status.tolist() == [OK, OVER_CELLS, OK, RAY_TOO_LONG]
    zero = dict(resolution=RES, samples=0, unknown=0, free_cells=0, hit_once=0, hit_more=0)
    assert rows[1] == dict(zero, **box1) and rows[3] == dict(zero, **box3)
    # held grid and held info of the failing robots: byte-identical to the render before; only the status word moved
    lay = fm.lay
    for b in (1, 3):
        assert first[b][8:12].view(np.int32)[0] == OK and second[b][8:12].view(np.int32)[0] == status[b]
        assert first[b][32:112].tobytes() == second[b][32:112].tobytes()
        assert first[b][lay["grid_off"]:].tobytes() == second[b][lay["grid_off"]:].tobytes()
        assert fm.info_of(b)["status"] == status[b]
        mc.assert_info({k: v for k, v in fm.info_of(b).items() if k != "status"}, ref.render(tfs_of[b], subs_of[b], RES))
    for b in (0, 2):
        mc.assert_robot(fm, b, ref.render(tfs2[b], subs2[b], RES), rows[b])
    # the healthy robots' bytes equal those of a run without the failing robots
    fm2, _, second2, (status2, _) = run(False)
    assert status2.tolist() == [OK, 77, OK, 77]
    for b in (0, 2):
        assert second[b].tobytes() == second2[b].tobytes()
    fm.close()
    fm2.close()


# ------------------------------------------------------------------------------------------------------------------ 5. isolation
def test_isolation_and_determinism(liw, synth):
    rng = np.random.default_rng(51)
    rooms = mc.rooms(4)
    K, P, cells, steps = 3, 3 * 24, 1 << 17, 1024
    tf_x, subs_x = mc.room_case(rng, K, 24, room=rooms[0])
    others = [mc.room_case(rng, k, 24, room=rooms[1 + i]) for i, k in enumerate((3, 1, 2))]

    def run(B, tfs_of, subs_of, sel=None):
        fm = mc.mapper(liw, synth, B, K, P, cells, steps)
        mc.load(fm, subs_of, stride=24)
        before = mc.regions(fm)
        fm.status.fill_(77)
        fm.info.fill_(0x5A)
        fm.render_tf(mc.pad_tfs(tfs_of, K), sel=sel)
        out = mc.regions(fm), before, fm.status.cpu().numpy().copy(), fm.info.cpu().numpy().copy()
        if sel is None:      # robot x sits in the middle of every fleet here
            mc.assert_robot(fm, B // 2, ref.render(tfs_of[B // 2], subs_of[B // 2], RES))
        fm.close()
        return out
    alone, _, st, info = run(1, [tf_x], [subs_x])
    R = alone[0].tobytes()
    assert st.tolist() == [OK]
    again, _, _, info2 = run(1, [tf_x], [subs_x])                      # two runs
    assert again[0].tobytes() == R and info2.tobytes() == info.tobytes()
    fleet_t = [others[0][0], others[1][0], tf_x, others[2][0]]
    fleet_s = [others[0][1], others[1][1], subs_x, others[2][1]]
    among, _, st4, info4 = run(4, fleet_t, fleet_s)                    # at another index among other robots
    assert among[2].tobytes() == R and info4[2].tobytes() == info[0].tobytes() and st4.tolist() == [OK] * 4
    only, before, st_sel, info_sel = run(4, fleet_t, fleet_s, sel=np.array([0, 0, 1, 0], np.uint8))   # selected alone in the full fleet
    assert only[2].tobytes() == R
    for b in (0, 1, 3):                                                # an unselected robot: region and rows not written
        assert only[b].tobytes() == before[b].tobytes()
        assert st_sel[b] == 77 and bool((info_sel[b] == 0x5A).all())
    assert st_sel[2] == OK and info_sel[2].tobytes() == info[0].tobytes()
    tiled, _, st256, info256 = run(256, [tf_x] * 256, [subs_x] * 256)   # 256 tiled copies
    assert st256.tolist() == [OK] * 256
    assert all(tiled[b].tobytes() == R for b in range(256)) and all(info256[b].tobytes() == info[0].tobytes() for b in range(256))


# ------------------------------------------------------------------------------------------------------------------ 6. render from poses
def test_render_from_poses(liw, synth):
    _check_render_from_poses(liw, synth, synth.office_params())


def test_render_from_poses_skewed_extrinsic(liw, synth):
    """k_fmap_tf's make_tf(p, q) * T_imu_to_laser at second_config.skewed_params: a generic laser rotation that the loader's quaternion round trip changes"""
    import second_config as sc
    _check_render_from_poses(liw, synth, sc.skewed_params(synth))


def _check_render_from_poses(liw, synth, prm):
    import torch
    rng = np.random.default_rng(61)
    rooms = mc.rooms(3)
    h = np.pi / 2
    yaws = [h, -h, np.nextafter(h, 0.0), np.nextafter(h, 4.0), -np.nextafter(h, 0.0), -np.nextafter(h, 4.0), h + 1e-9, -h - 1e-9,
            np.pi - 2e-3, -(np.pi - 2e-3), 0.3, -2.2]
    B, K = 3, 4
    poses = np.zeros((B, K, 6))
    for b in range(B):
        for k in range(K):
            poses[b, k] = [rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.05, 0.05), 0.0, 0.0, yaws[b * K + k]]
    poses[1, :, 3:5] = rng.uniform(-0.03, 0.03, (K, 2))     # roll / pitch components on robot 1, pure yaw on the others
    subs_of = [mc.room_case(rng, K, 24, room=rooms[b])[1] for b in range(B)]
    fm = mc.mapper(liw, synth, B, K, K * 24, 1 << 19, 2048, prm=prm)
    mc.load(fm, subs_of)
    Til = mc.til12(liw, prm)
    # a pose source whose robot stride is larger than 6 * max_submaps
    wide = torch.full((B, K + 3, 6), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :K] = torch.as_tensor(poses)
    src = wide[:, :K]
    assert src.stride(0) == 6 * (K + 3) > 6 * K
    fm.render(src)
    status, rows = _rows(fm)
    assert status.tolist() == [OK] * B
    worst = 0.0
    for b in range(B):
        got = fm.tf(b)
        want_tf = mc.host_tf(liw, poses[b], Til)
        assert got.shape == (K, 12)
        worst = max(worst, mc.ulps(got, want_tf))
        mc.assert_robot(fm, b, ref.render(got, subs_of[b], RES), rows[b])    # the walk from the returned transforms, exactly
    print("device make_tf * T_imu_to_laser against the host's: %.2f ulp at most" % worst)
    assert worst <= 4.0
    regs = mc.regions(fm)
    fm.render(poses)                                                          # the same poses, contiguous: the same bytes
    assert mc.regions(fm).tobytes() == regs.tobytes()
    fm.close()


# ------------------------------------------------------------------------------------------------------------------ 7. behind the back-end
def test_behind_the_backend(liw, synth):
    import torch
    rng = np.random.default_rng(71)
    prm = synth.office_params()
    B, K = 4, 14
    graphs = [liw.posegraph.make_pose_graph(prm, N=n, seed=70 + b, n_loop=2) for b, n in enumerate((12, 14, 10, 13))]
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=K, max_loops=4), solve_period=1.0, max_iters=8)
    for b, G in enumerate(graphs):
        fb.load_graph(b, G)
    rooms = mc.rooms(B)
    # scans scaled to a quarter: the key frames lie on a circle, and the box around all of them stays small
    subs_of = [[0.25 * s for s in mc.room_case(rng, G["N"], 16, room=rooms[b])[1]] for b, G in enumerate(graphs)]
    fm = mc.mapper(liw, synth, B, K, K * 16, 1 << 19, 2048, prm=prm)
    mc.load(fm, subs_of)
    assert [fm.num_submaps(b) for b in range(B)] == [fb.num_keyframes(b) for b in range(B)] == [G["N"] for G in graphs]
    Til = mc.til12(liw, prm)
    fm.render_all(fb)                    # the maps of the drifting poses
    status, rows = _rows(fm)
    assert status.tolist() == [OK] * B
    first = mc.regions(fm)
    for b in range(B):
        assert np.array_equal(fb.keyframes(b)["poses"], graphs[b]["poses"])
        assert mc.ulps(fm.tf(b), mc.host_tf(liw, graphs[b]["poses"], Til)) <= 4.0
    stamps = torch.full((B,), 100.0, dtype=torch.float64)
    due, n_due = fb.due(torch.ones(B, dtype=torch.uint8), stamps, mask=torch.tensor([1, 1, 0, 1], dtype=torch.uint8))
    assert due.cpu().tolist() == [1, 1, 0, 1] and int(n_due.item()) == 3
    fb.solve(due, stamps)
    fm.status.fill_(77)
    fm.render(fb.poses(), sel=due)
    status, rows = _rows(fm)
    assert status.tolist() == [OK, OK, 77, OK]
    second = mc.regions(fm)
    moved = 0
    for b in (0, 1, 3):
        kf = fb.keyframes(b)["poses"]
        assert not np.array_equal(kf, graphs[b]["poses"])                      # the solve moved the poses
        got = fm.tf(b)
        assert got.shape == (graphs[b]["N"], 12) and mc.ulps(got, mc.host_tf(liw, kf, Til)) <= 4.0
        mc.assert_robot(fm, b, ref.render(got, subs_of[b], RES), rows[b])
        moved += second[b].tobytes() != first[b].tobytes()
    assert moved == 3
    assert second[2].tobytes() == first[2].tobytes()                           # not due: its earlier grid stays
    # push with the back-end's result of a frame: no key frame stored, and a render of the due robots exactly when n_due is non-zero
    none = torch.zeros(B, dtype=torch.uint8, device="cuda")
    scan = (torch.zeros(B, 16, 3, dtype=torch.float64, device="cuda"), torch.full((B,), 16, dtype=torch.int32, device="cuda"))
    fm.status.fill_(77)
    out = fm.push(None, scan, dict(added=none, due=due, n_due=0), fb)
    assert not out["rendered"] and out["added"].cpu().tolist() == [0] * B and fm.status.cpu().tolist() == [77] * B
    assert mc.regions(fm).tobytes() == second.tobytes()
    due2 = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
    out = fm.push(None, scan, dict(added=none, due=due2, n_due=1), fb)
    assert out["rendered"] and fm.status.cpu().tolist() == [77, 77, OK, 77]
    third = mc.regions(fm)
    assert all(third[b].tobytes() == second[b].tobytes() for b in (0, 1, 3))
    mc.assert_robot(fm, 2, ref.render(fm.tf(2), subs_of[2], RES))              # robot 2 was not solved: its map at the loaded poses
    assert mc.ulps(fm.tf(2), mc.host_tf(liw, graphs[2]["poses"], Til)) <= 4.0
    fm.close()
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 8. push behind a tracker
def test_push_behind_the_tracker(liw, synth):
    """step -> FleetLoopDetector.push -> FleetBackEnd.push -> FleetMapper.push for the free-running fleet of
    tests/test_gpu_posegraph_batch.py::test_behind_the_tracker"""
    import torch
    import test_gpu_laser_track as tlt
    import test_gpu_loop as tgl
    import test_gpu_loop_batch as tglb
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
    tp = dict(liw.laser_batch.office_track_params(prm), key_frame_p_motion_threshold=0.1)
    nb, F, B = 8, 6, 16
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=F + 1, L=0) for j in range(nb)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(F + 1, 15) for t in trajs])
    ranges = np.stack([[tlt._cast(liw, synth, lp, 3000 + j, truth[j, k, 0:6], seed=j * 10 + k) for k in range(F + 1)] for j in range(nb)])
    sc = dict(prm=prm, lp=lp, tp=tp, nb=nb, F=F, trajs=trajs, truth=truth, ranges=ranges, times=np.stack([t["times"] for t in trajs]))
    rob = np.arange(B) % nb
    ft = tlt._fleet(liw, sc, B)
    tlt._seed(torch, sc, ft.fe, rob)
    ft.start(truth[rob, 0])
    K = 16
    fl = tglb._fleet(liw, synth, tgl._params(min_interval=2, submap_count=3), B, K, 256, 256)
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=K, max_loops=4), solve_period=0.0, max_iters=5)
    fm = mc.mapper(liw, synth, B, K, F * ft.fe.max_points, 1 << 20, 2048, prm=prm)
    # every synchronous accessor of the mapper, and the back-end's one read, counted
    reads = []
    for name in ("_sync", "infos", "num_submaps", "is_full", "submap", "tf", "info_of", "grid", "write_pgm"):
        setattr(fm, name, (lambda real, name: lambda *a, **k: reads.append(name) or real(*a, **k))(getattr(fm, name), name))
    real_read = fb._read_n_due
    fb._read_n_due = lambda: reads.append("n_due") or real_read()
    scans = [[] for _ in range(B)]
    rendered = 0
    for k in range(1, F + 1):
        r, st = tlt._frame(torch, sc, rob, k)
        o = ft.step(r, st, tlt._interval(torch, sc, rob, k))
        lo = fl.push(o)
        out = fb.push(o, lo, torch.as_tensor(sc["times"][rob, k]))
        pts, n = ft.scan_points()
        assert pts.shape == (B, ft.fe.max_points, 3) and n.shape == (B,)
        before = len(reads)
        mo = fm.push(o, (pts, n), out, fb)
        assert len(reads) == before                                            # no device -> host copy in push
        assert mo["rendered"] == bool(out["n_due"])
        rendered += mo["rendered"]
        added, hp_, hn = mo["added"].cpu().numpy(), pts.cpu().numpy(), n.cpu().numpy()
        assert np.array_equal(added, out["added"].cpu().numpy())
        for b in range(B):
            if added[b]:
                scans[b].append(hp_[b, :max(int(hn[b]), 0)].copy())
            assert fm.num_submaps(b) == fb.num_keyframes(b) == len(scans[b])
        if mo["rendered"]:
            due = out["due"].cpu().numpy()
            status = fm.status.cpu().numpy()
            assert all(status[b] in (OK, EMPTY) for b in range(B) if due[b])
    total = 0
    for b in range(B):
        assert len(scans[b]) >= 3 and not fm.is_full(b)
        for j, s in enumerate(scans[b]):
            got = fm.submap(b, j)
            assert got.shape == s.shape and got.tobytes() == s.tobytes()
        total += len(scans[b])
    # the end of the log: every robot's map from the back-end's poses; robot 0's against the single-robot map at the returned transforms
    fm.render_all(fb)
    status, rows = _rows(fm)
    assert status.tolist() == [OK] * B
    single = liw.gridmap.GridMap(prm, dict(resolution=RES), dict(max_submaps=K, max_points=F * ft.fe.max_points, max_cells=1 << 20))
    for s in scans[0]:
        single.add_submap(s)
    assert single.render_tf(fm.tf(0)) == rows[0] and rows[0]["rays"] > 0
    assert np.array_equal(single.grid(), fm.grid(0))
    print("push behind the tracker: %d sub-maps stored, %d of %d frames rendered in push" % (total, rendered, F))
    fm.close()
    fb.close()
    fl.close()
    ft.close()
