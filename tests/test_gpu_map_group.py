"""The shared occupancy-grid map of a group of fleet robots on the MI355X (include/liw_map_group.h).  Every grid comparison is exact:
zero differing cells, and equal width, height, origin, rays, samples and four counts.  A group's checkers are the ones of the
single map, fed the members' sub-maps in (robot, sub-map) order with the T_g_l read back from the device: the serial walk of
tests/map_reference.py, its C++ twin tests/cpp/map_serial.cpp and gridmap.GridMap (the single-robot kernels)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_batch_cases as mc
import map_group_cases as gc
import map_reference as ref

pytestmark = pytest.mark.gpu
RES = mc.RES
LIW_EINVAL = -22
OK, EMPTY, OVER_CELLS, RAY_TOO_LONG = 0, 1, 2, 3
H_NTF = slice(16, 20)      # int32 word 4 of a robot's header: transforms composed by the last render


def _rows(gm):
    return gm.gstatus.cpu().numpy().copy(), gm.infos()


_SERIAL = {}


def _serial(tmp_path_factory):
    if not _SERIAL:
        _SERIAL["L"] = ref.build_serial(tmp_path_factory.mktemp("map_serial"))
    return _SERIAL["L"]


def _single(liw, synth, tfs, subs, res, cells):
    """(info, grid) of ONE GridMap fed the sub-maps with the transforms"""
    n = sum(len(s) for s in subs)
    single = liw.gridmap.GridMap(synth.office_params(), dict(resolution=res), dict(max_submaps=max(len(subs), 1), max_points=max(n, 1), max_cells=cells))
    for k, s in enumerate(subs):
        assert single.add_submap(s) == k
    return single.render_tf(tfs), single.grid()


def _robot_scratch_mask(lay):
    """bool [robot_bytes]: the bytes a group render may write in a robot region (tf, partials, H_NTF)"""
    m = np.zeros(lay["robot_bytes"], bool)
    m[H_NTF] = True
    m[lay["tf_off"]:lay["bits_off"]] = True       # tf, then partials, up to the cell bits
    return m


# ------------------------------------------------------------------------------------------------------------------ 1. parity, 2. composition
_ROOM = {}


def _room_case():
    """B = 6 robots in one room with 2, 3, 1, 0, 2, 1 sub-maps of 90 rays; groups {0, 3}, {1, 2, 4}, none; robot 5 in no group"""
    if not _ROOM:
        _ROOM.update(gc.shared_room(np.random.default_rng(0), (2, 3, 1, 0, 2, 1)), group_of=np.array([0, 1, 1, 0, 1, -1], np.int32), refs={})
    return _ROOM


@pytest.mark.parametrize("res", [0.05, 0.1])
def test_parity(liw, synth, res, tmp_path_factory):
    c = _room_case()
    tfs_of, subs_of, T_g_w, group_of = c["tfs_of"], c["subs_of"], c["T_g_w"], c["group_of"]
    B, G, K, cells = 6, 3, 3, 1 << 18
    fm = mc.mapper(liw, synth, B, K, K * 90, cells, 2048, res=res)
    mc.load(fm, subs_of)
    gm = liw.FleetGroupMap(fm, G, cells, guard=64)
    assert [gm.info_of(g)["status"] for g in range(G)] == [EMPTY] * G and gm.members(0) == (0, 0)
    T_w_l = mc.pad_tfs(tfs_of, K)
    gm.render_tf(T_w_l, group_of, T_g_w)
    status, rows = _rows(gm)
    assert status.tolist() == [OK, OK, EMPTY]
    assert [gm.members(g) for g in range(G)] == [(2, 2), (3, 6), (0, 0)]
    # composition: the product and sum order of liw_lie_mul
    T_g_l = [fm.tf(b) for b in range(B)]
    worst = 0.0
    for b in range(5):
        want = gc.compose([tfs_of[b]], [T_g_w[b]], mul=lambda A, Bm: gc.lie_mul(liw, A, Bm))[0]
        assert T_g_l[b].shape == want.shape
        if len(want):
            worst = max(worst, mc.ulps(T_g_l[b], want))
    print("device T_g_w * T_w_l against liw_lie_mul: %.2f ulp at most" % worst)
    assert worst <= 4.0
    serial = _serial(tmp_path_factory)
    for g, members in enumerate(([0, 3], [1, 2, 4])):
        tfs, subs = gc.concat(T_g_l, subs_of, members)
        if (res, g) not in c["refs"]:
            c["refs"][(res, g)] = (tfs.tobytes(), ref.render(tfs, subs, res))
        assert c["refs"][(res, g)][0] == tfs.tobytes()
        want = c["refs"][(res, g)][1]
        gc.assert_group(gm, g, want, rows[g])
        ws = ref.render_serial(serial, tfs, subs, res)
        mc.assert_info(rows[g], ws)
        assert np.array_equal(ws["grid"], gm.grid(g))
        info, grid = _single(liw, synth, tfs, subs, res, cells)
        assert info == rows[g] and np.array_equal(grid, gm.grid(g))
        assert gm.device_data(g) == gm.store.data_ptr() + g * gm.lay["group_bytes"] + gm.lay["grid_off"]
    if res == 0.05:      # what only the shared map shows: walls seen by several members
        own = [ref.render(tfs_of[b], subs_of[b], res)["counts"][100] for b in (1, 2, 4)]
        assert rows[1]["hit_more"] > sum(own)
    gc.assert_group(gm, 2, ref.render([], [], res), rows[2])
    fm.close()
    gm.close()


def test_composition_from_poses(liw, synth):
    rng = np.random.default_rng(62)
    prm = synth.office_params()
    B, K, G = 4, 3, 2
    poses = np.zeros((B, K, 6))
    for b in range(B):
        for k in range(K):
            poses[b, k] = [rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-3, 3)]
    subs_of = [mc.room_case(rng, K, 24)[1] for b in range(B)]
    T_g_w = gc.group_frames(rng, B)
    group_of = np.array([1, 0, 1, 0], np.int32)
    fm = mc.mapper(liw, synth, B, K, K * 24, 1 << 19, 2048, prm=prm)
    mc.load(fm, subs_of)
    gm = liw.FleetGroupMap(fm, G, 1 << 19)
    Til = mc.til12(liw, prm)
    fm.render(poses)
    own_tf = [fm.tf(b) for b in range(B)]            # what liw_fmap_render leaves
    own = mc.regions(fm)
    gm.render(poses, group_of, T_g_w)
    status, rows = _rows(gm)
    assert status.tolist() == [OK, OK]
    worst = 0.0
    for b in range(B):
        got = fm.tf(b)
        assert got.shape == (K, 12)
        # the device's own T_w_l times T_g_w: the order of liw_lie_mul, to the bit
        assert got.tobytes() == np.array([gc.lie_mul(liw, T_g_w[b], T) for T in own_tf[b]]).tobytes()
        want = np.array([gc.lie_mul(liw, T_g_w[b], T) for T in mc.host_tf(liw, poses[b], Til)])
        worst = max(worst, mc.ulps(got, want))
    print("device T_g_w * (make_tf * T_imu_to_laser) against the host's: %.2f ulp at most" % worst)
    assert worst <= 4.0
    for g, members in enumerate(([1, 3], [0, 2])):
        gc.assert_group(gm, g, ref.render(*gc.concat([fm.tf(b) for b in range(B)], subs_of, members), RES), rows[g])
    # T_g_w = None: the transforms of liw_fmap_render / liw_fmap_render_tf, bit for bit
    gm.render(poses, group_of)
    assert all(fm.tf(b).tobytes() == own_tf[b].tobytes() for b in range(B))
    T = rng.uniform(-1, 1, (B, K, 12))
    T[0, 0, 3] = -0.0
    gm.render_tf(T, group_of)
    assert all(fm.tf(b).tobytes() == T[b].tobytes() for b in range(B))
    # the robots' own maps: nothing but the scratch moved
    keep = ~_robot_scratch_mask(fm.lay)
    after = mc.regions(fm)
    assert all(after[b][keep].tobytes() == own[b][keep].tobytes() for b in range(B))
    fm.close()
    gm.close()


# ------------------------------------------------------------------------------------------------------------------ 3. one member
def test_group_of_one_is_the_robots_own_map(liw, synth):
    rng = np.random.default_rng(33)
    B, K = 3, 3
    cases = [mc.room_case(rng, k, 40, room=mc.rooms(3)[b]) for b, k in enumerate((2, 3, 1))]
    tfs_of, subs_of = [c[0] for c in cases], [c[1] for c in cases]
    fm = mc.mapper(liw, synth, B, K, K * 40, 1 << 18, 2048)
    mc.load(fm, subs_of)
    T = mc.pad_tfs(tfs_of, K)
    fm.render_tf(T)
    own_rows = fm.info.cpu().numpy().copy()
    own = mc.regions(fm)
    gm = liw.FleetGroupMap(fm, 4, 1 << 18)
    gm.render_tf(T, np.array([2, 0, 3], np.int32))
    reg = gc.gregions(gm)
    lay, glay = fm.lay, gm.lay
    for b, g in enumerate((2, 0, 3)):
        assert reg[g][32:112].tobytes() == own[b][32:112].tobytes()            # the held info
        assert gm.ginfo[g].cpu().numpy().tobytes() == own_rows[b].tobytes()
        n = gm.info_of(g)["width"] * gm.info_of(g)["height"]
        assert n > 0 and reg[g][glay["grid_off"]:glay["grid_off"] + n].tobytes() == own[b][lay["grid_off"]:lay["grid_off"] + n].tobytes()
        assert reg[g][glay["bits_off"]:glay["bits_off"] + n].tobytes() == own[b][lay["bits_off"]:lay["bits_off"] + n].tobytes()
        assert gm.members(g) == (1, len(subs_of[b]))
    assert gm.info_of(1)["status"] == EMPTY and gm.members(1) == (0, 0)
    fm.close()
    gm.close()


# ------------------------------------------------------------------------------------------------------------------ 4. edge cases
def _box(tfs, subs, res):
    """width, height, origin and rays of the bounding box, with the arithmetic of include/liw_map.h"""
    P = [ref.world_point([float(v) for v in T], pt) for T, s in zip(tfs, subs) for pt in np.asarray(s).reshape(-1, 3)]
    xs, ys = [p[0] for p in P], [p[1] for p in P]
    return dict(width=int((max(xs) - min(xs)) / res + 1), height=int((max(ys) - min(ys)) / res + 1), origin_x=min(xs), origin_y=min(ys), rays=len(P))


def test_edge_cases_share_a_launch(liw, synth, tmp_path):
    rng = np.random.default_rng(44)
    steps, cells, K = 1024, 1 << 18, 2
    same_t, same_s = gc.one_point_same_cell()
    apart_t, apart_s = gc.one_point_disjoint()
    odd = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [np.nan, 0.2, 0.0], [0.5, np.inf, 0.0], [2.0, -1.0, 0.0], [-np.inf, np.nan, 1.0]])
    odd_tf = np.array([mc.tf12(0.4, -0.2, 0.3)])
    bad_tf = odd_tf.copy()
    bad_tf[0, 4] = np.nan                        # a non-finite transform: every point of the sub-map is ignored
    plain = np.array([[0.7, 0.1, 0.0], [0.2, -0.9, 0.0]])
    room_a, room_b = mc.room_case(rng, 1, 30), mc.room_case(rng, 1, 30)
    room_c, room_d = mc.room_case(rng, 1, 30), mc.room_case(rng, 1, 30)
    limit = (steps - 2) * RES / 2
    far = np.array([[limit + 0.4, 0.3, 0.0]])
    #   robot : group      0: no sub-map -> 1      1, 2: same cell -> 2      3, 4: disjoint -> 3
    #   5 odd points, 6 non-finite transform, 7 a zero-length ray alone -> 4      8, 9 -> 5 (then too many cells)
    #   10 -> 6, 11 joins it with a ray too long      12, 13 -> 7, not selected in the second launch      group 0: nobody
    subs_of = [[], same_s[0], same_s[1], apart_s[0], apart_s[1], [odd], [plain], [np.zeros((1, 3))], room_a[1], room_b[1], room_c[1], [far],
               room_d[1], [plain]]
    tfs_of = [np.zeros((0, 12)), same_t[0], same_t[1], apart_t[0], apart_t[1], odd_tf, bad_tf, odd_tf, room_a[0], room_b[0], room_c[0],
              np.array([mc.tf12(0.0, 5.0, 0.2)]), room_d[0], odd_tf]
    B, G = len(subs_of), 8
    first_of = np.array([1, 2, 2, 3, 3, 4, 4, 4, 5, 5, 6, -1, 7, 7], np.int32)
    second_of = first_of.copy()
    second_of[11] = 6
    fm = mc.mapper(liw, synth, B, K, 64, cells, steps)
    mc.load(fm, subs_of)
    gm = liw.FleetGroupMap(fm, G, cells, guard=64)
    gm.render_tf(mc.pad_tfs(tfs_of, K), first_of)
    status, rows = _rows(gm)
    assert status.tolist() == [EMPTY, EMPTY, OK, OK, OK, OK, OK, OK]
    first = gc.gregions(gm)
    members = {2: [1, 2], 3: [3, 4], 4: [5, 6, 7], 5: [8, 9], 6: [10], 7: [12, 13]}
    wants = {g: ref.render(*gc.concat(tfs_of, subs_of, m), RES) for g, m in members.items()}
    assert wants[2]["counts"] == {-1: 0, 0: 0, 50: 0, 100: 1}
    assert (wants[3]["width"], wants[3]["height"]) == (49, 47) and wants[3]["counts"] == {-1: 2289, 0: 12, 50: 2, 100: 0}
    assert wants[4]["rays"] == 4                 # three valid odd points and the zero-length ray; the NaN transform's two are ignored
    for g in range(G):
        gc.assert_group(gm, g, wants.get(g, ref.render([], [], RES)), rows[g])
    assert gm.members(0) == (0, 0) and gm.members(1) == (1, 0) and gm.members(4) == (3, 3) and gm.grid(0).size == 0
    # second launch: group 5's members lie 40 m apart, group 6 gets the long ray, group 7 is not selected
    tfs2 = [t.copy() for t in tfs_of]
    tfs2[9][0, 9:11] += 40.0
    tfs2[12][0, 9] += 0.5
    box5, box6 = _box(*gc.concat(tfs2, subs_of, [8, 9]), RES), _box(*gc.concat(tfs2, subs_of, [10, 11]), RES)
    assert box5["width"] * box5["height"] > cells >= box6["width"] * box6["height"]
    gm.gstatus.fill_(77)
    gm.ginfo.fill_(0x5A)
    gsel = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    robots_before = mc.regions(fm)
    gm.render_tf(mc.pad_tfs(tfs2, K), second_of, gsel=gsel)
    status, rows = _rows(gm)
    assert status.tolist() == [EMPTY, EMPTY, OK, OK, OK, OVER_CELLS, RAY_TOO_LONG, 77]
    second = gc.gregions(gm)
    zero = dict(resolution=RES, samples=0, unknown=0, free_cells=0, hit_once=0, hit_more=0)
    assert rows[5] == dict(zero, **box5) and rows[6] == dict(zero, **box6)
    for g in (5, 6):      # the held grid and info stay; status, members and sub-maps are of the last render
        assert second[g][0:4].view(np.int32)[0] == status[g] and first[g][0:4].view(np.int32)[0] == OK
        assert second[g][12:].tobytes() == first[g][12:].tobytes()
        mc.assert_info({k: v for k, v in gm.info_of(g).items() if k != "status"}, wants[g])
        assert np.array_equal(gm.grid(g), wants[g]["grid"])
    assert gm.members(6) == (2, 2)
    for g in (2, 3, 4):
        assert second[g].tobytes() == first[g].tobytes()
    # not selected: no byte of the region, of the rows or of the guards; nor of its members' robot regions
    assert second[7].tobytes() == first[7].tobytes()
    assert bool((gm.ginfo[7] == 0x5A).all())
    robots_after = mc.regions(fm)
    assert all(robots_after[b].tobytes() == robots_before[b].tobytes() for b in (12, 13))
    for o in (gm, fm):
        assert o.guard >= 64 and bool((o._buf[:o.guard] == 0xA5).all()) and bool((o._buf[-o.guard:] == 0xA5).all())
    gm.write_pgm(3, tmp_path / "group", palette=(205, 254, 100, 0))
    assert (tmp_path / "group.pgm").stat().st_size > 49 * 47 and (tmp_path / "group.yaml").exists()
    # a masked reset empties exactly the masked groups
    gm.reset(gmask=np.array([0, 0, 0, 1, 0, 0, 0, 0], np.uint8))
    third = gc.gregions(gm)
    assert gm.info_of(3) == dict(width=0, height=0, resolution=RES, origin_x=0.0, origin_y=0.0, rays=0, samples=0, unknown=0, free_cells=0,
                                 hit_once=0, hit_more=0, status=EMPTY)
    assert all(third[g].tobytes() == second[g].tobytes() for g in range(G) if g != 3)
    fm.close()
    gm.close()


# ------------------------------------------------------------------------------------------------------------------ 5. isolation
def test_isolation_and_determinism(liw, synth):
    rng = np.random.default_rng(55)
    K, P, cells, steps = 3, 3 * 24, 1 << 17, 1024
    x = gc.shared_room(rng, (3, 1, 2), n_rays=24)
    others = gc.shared_room(rng, (2, 3, 1), n_rays=24, room=mc.rooms(2)[1])

    def run(tfs_of, subs_of, T_g_w, group_of, G, g, check=None):
        B = len(subs_of)
        fm = mc.mapper(liw, synth, B, K, P, cells, steps)
        mc.load(fm, subs_of, stride=24)
        T = mc.pad_tfs(tfs_of, K)
        fm.render_tf(T)
        own = mc.regions(fm), fm.status.cpu().numpy().copy(), fm.info.cpu().numpy().copy()
        gm = liw.FleetGroupMap(fm, G, cells)
        gm.render_tf(T, np.asarray(group_of, np.int32), np.asarray(T_g_w))
        out = gc.gregions(gm)[g].tobytes(), gm.ginfo[g].cpu().numpy().tobytes()
        if check is not None:
            after = mc.regions(fm)
            scratch = _robot_scratch_mask(fm.lay)
            for b in range(B):      # a group render leaves the robots' sub-maps, status, held info, cell bits and grids alone
                assert after[b][~scratch].tobytes() == own[0][b][~scratch].tobytes()
                if not 0 <= group_of[b] < G:      # in no group: no byte
                    assert after[b].tobytes() == own[0][b].tobytes()
            assert any((after[b] != own[0][b]).any() for b in check)
            gc.assert_group(gm, g, ref.render(*gc.concat([fm.tf(b) for b in range(B)], subs_of, check), RES))
            fm.render_tf(T)         # the per-robot render afterwards: what it was before
            again = mc.regions(fm)
            keep = np.ones(fm.lay["robot_bytes"], bool)
            keep[H_NTF] = False
            keep[fm.lay["tf_off"]:fm.lay["partial_off"]] = False
            assert all(again[b][keep].tobytes() == own[0][b][keep].tobytes() for b in range(B))
            assert fm.status.cpu().numpy().tobytes() == own[1].tobytes() and fm.info.cpu().numpy().tobytes() == own[2].tobytes()
        fm.close()
        gm.close()
        return out
    xt, xs, xg = x["tfs_of"], x["subs_of"], x["T_g_w"]
    ot, os_, og = others["tfs_of"], others["subs_of"], others["T_g_w"]
    R, row = run(xt, xs, xg, [0, 0, 0], 1, 0, check=[0, 1, 2])                   # a fleet of exactly its members
    assert run(xt, xs, xg, [0, 0, 0], 1, 0) == (R, row)                          # two runs
    # other robot indices, another order, other groups around it
    order = [ot[0], xt[2], ot[1], xt[0], ot[2], xt[1]], [os_[0], xs[2], os_[1], xs[0], os_[2], xs[1]], [og[0], xg[2], og[1], xg[0], og[2], xg[1]]
    assert run(*order, [0, 2, 0, 2, -1, 2], 3, 2, check=[1, 3, 5]) == (R, row)
    # 64 tiled copies, the members of a copy 64 robots apart
    fm = mc.mapper(liw, synth, 192, K, P, cells, steps)
    tiled_s = [xs[b // 64] for b in range(192)]
    mc.load(fm, tiled_s, stride=24)
    gm = liw.FleetGroupMap(fm, 64, cells)
    gm.render_tf(mc.pad_tfs([xt[b // 64] for b in range(192)], K), np.arange(192, dtype=np.int32) % 64, np.array([xg[b // 64] for b in range(192)]))
    reg, rows = gc.gregions(gm), gm.ginfo.cpu().numpy()
    assert gm.gstatus.cpu().tolist() == [OK] * 64
    assert all(reg[g].tobytes() == R for g in range(64)) and all(rows[g].tobytes() == row for g in range(64))
    fm.close()
    gm.close()


# ------------------------------------------------------------------------------------------------------------------ 6. kernel-grid edges
def test_kernel_grid_edges(liw, synth, tmp_path_factory):
    """One member holds more points than one pass of the bounds grid (partials x kBlock) and of the ray grid covers, and the group's
    grid has a cell count that is no multiple of 16 and more 16-cell items than one pass of the clear / finish grid (cell_chunks x
    kBlock) covers."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "2dliw-slam_amd", "csrc", "k_map.hpp")).read()
    kBlock = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    rng = np.random.default_rng(66)
    B, G, K, P, cells = 2, 32, 2, 17000, 310000
    fm = mc.mapper(liw, synth, B, K, P, 1 << 10, 1024)
    gm = liw.FleetGroupMap(fm, G, cells)
    n_big = 16700
    assert fm.lay["partials"] * kBlock < n_big and -(-P // 32) * (kBlock // 16) < n_big
    a = rng.uniform(-np.pi, np.pi, n_big)
    r = rng.uniform(0.05, 1.4, n_big)
    big = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.01, 0.01, n_big)], axis=1)
    small = np.array([[1.0, 0.9, 0.0], [-0.5, 0.3, 0.0], [0.2, -1.1, 0.0]])
    subs_of = [[big[:9000], big[9000:]], [small]]
    tfs_of = [np.array([mc.tf12(1.5, 1.5, 0.3, 0.01, 0.01, -0.01), mc.tf12(1.6, 1.4, -1.0)]), np.array([mc.tf12(28.6, 23.63, 2.0)])]
    mc.load(fm, subs_of)
    T = mc.pad_tfs(tfs_of, K)
    gm.render_tf(T, np.array([5, 5], np.int32))
    status, rows = _rows(gm)
    assert status[5] == OK and gm.members(5) == (2, 3)
    tfs, subs = gc.concat(tfs_of, subs_of, [0, 1])
    want = ref.render_serial(_serial(tmp_path_factory), tfs, subs, RES)
    ncell = want["width"] * want["height"]
    assert ncell % 16 != 0 and -(-ncell // 16) > gm.lay["cell_chunks"] * kBlock and ncell <= cells
    mc.assert_info(rows[5], want)
    assert np.array_equal(gm.grid(5), want["grid"])
    # the robots' own grids are too small for this: their capacity is their own
    fm.render_tf(T)
    assert fm.status.cpu().tolist()[0] == OVER_CELLS
    fm.close()
    gm.close()


# ------------------------------------------------------------------------------------------------------------------ 7. behind the back-end
def test_behind_the_backend(liw, synth):
    import torch
    rng = np.random.default_rng(77)
    prm = synth.office_params()
    B, K, G = 4, 14, 2
    graphs = [liw.posegraph.make_pose_graph(prm, N=n, seed=70 + b, n_loop=2) for b, n in enumerate((12, 14, 10, 13))]
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=K, max_loops=4), solve_period=1.0, max_iters=8)
    for b, Gr in enumerate(graphs):
        fb.load_graph(b, Gr)
    subs_of = [[0.25 * s for s in mc.room_case(rng, Gr["N"], 16)[1]] for Gr in graphs]
    fm = mc.mapper(liw, synth, B, K, K * 16, 1 << 19, 2048, prm=prm)
    mc.load(fm, subs_of)
    gm = liw.FleetGroupMap(fm, G, 1 << 21)
    stamps = torch.full((B,), 100.0, dtype=torch.float64)
    due, _ = fb.due(torch.ones(B, dtype=torch.uint8), stamps)
    fb.solve(due, stamps)
    group_of = torch.tensor([1, 0, 1, -1], dtype=torch.int32, device="cuda")
    T_g_w = torch.as_tensor(gc.group_frames(rng, B), device="cuda")
    # every synchronous accessor of both maps, and the back-end's one read, counted
    reads = []
    for o, names in ((gm, ("_sync", "infos", "info_of", "grid", "members", "write_pgm")), (fm, ("_sync", "infos", "tf", "info_of", "grid", "num_submaps"))):
        for name in names:
            setattr(o, name, (lambda real, name: lambda *a, **k: reads.append(name) or real(*a, **k))(getattr(o, name), name))
    real_read = fb._read_n_due
    fb._read_n_due = lambda: reads.append("n_due") or real_read()
    gm.render_all(fb, group_of, T_g_w)
    assert not reads                                                           # no device -> host copy in a render
    status, rows = _rows(gm)
    assert status.tolist() == [OK, OK]
    Til = mc.til12(liw, prm)
    T_g_l = [fm.tf(b) for b in range(B)]
    for b in (0, 1, 2):
        kf = fb.keyframes(b)["poses"]
        assert not np.array_equal(kf, graphs[b]["poses"])                      # the solve moved the poses
        want = np.array([gc.lie_mul(liw, T_g_w[b].cpu().numpy(), T) for T in mc.host_tf(liw, kf, Til)])
        assert T_g_l[b].shape == (graphs[b]["N"], 12) and mc.ulps(T_g_l[b], want) <= 4.0
    for g, members in enumerate(([1], [0, 2])):
        gc.assert_group(gm, g, ref.render(*gc.concat(T_g_l, subs_of, members), RES), rows[g])
    fm.close()
    gm.close()
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 8. bad calls
def test_bad_calls_write_nothing(liw, synth):
    import torch
    rng = np.random.default_rng(88)
    B, K, G = 3, 2, 2
    cases = [mc.room_case(rng, 2, 20) for _ in range(B)]
    fm = mc.mapper(liw, synth, B, K, 64, 1 << 17, 1024)
    mc.load(fm, [c[1] for c in cases])
    gm = liw.FleetGroupMap(fm, G, 1 << 17, guard=64)
    gm.render_tf(mc.pad_tfs([c[0] for c in cases], K), np.array([0, 1, 0], np.int32))
    gm.gstatus.fill_(77)
    gm.ginfo.fill_(0x5A)
    torch.cuda.synchronize()
    snap = fm._buf.cpu().numpy().copy(), gm._buf.cpu().numpy().copy()
    L, h = gm.L, gm.h
    vp = lambda t: C.c_void_p(t.data_ptr())
    tfs = torch.zeros(B, K, 12, dtype=torch.float64, device="cuda")
    go = torch.zeros(B, dtype=torch.int32, device="cuda")
    st, gst = vp(fm.store), vp(gm.store)
    mis, gmis = C.c_void_p(fm.store.data_ptr() + 4), C.c_void_p(gm.store.data_ptr() + 4)
    s, i = vp(gm.gstatus), vp(gm.ginfo)
    calls = [lambda: L.liw_gmap_reset(h, None, None, None), lambda: L.liw_gmap_reset(h, gmis, None, None)]
    for fn in (L.liw_gmap_render_tf, L.liw_gmap_render):
        calls += [lambda fn=fn: fn(h, None, gst, vp(tfs), 12 * K, vp(go), None, None, s, i, None),       # null stores
                  lambda fn=fn: fn(h, st, None, vp(tfs), 12 * K, vp(go), None, None, s, i, None),
                  lambda fn=fn: fn(h, st, gst, vp(tfs), 12 * K, None, None, None, s, i, None),           # a null group_of
                  lambda fn=fn: fn(h, mis, gst, vp(tfs), 12 * K, vp(go), None, None, s, i, None),        # misaligned stores
                  lambda fn=fn: fn(h, st, gmis, vp(tfs), 12 * K, vp(go), None, None, s, i, None),
                  lambda fn=fn: fn(h, st, gst, vp(tfs), -1, vp(go), None, None, s, i, None),             # a negative stride
                  lambda fn=fn: fn(h, st, gst, None, 12 * K, vp(go), None, None, s, i, None),
                  lambda fn=fn: fn(h, st, gst, vp(tfs), 12 * K, vp(go), None, None, None, i, None),
                  lambda fn=fn: fn(h, st, gst, vp(tfs), 12 * K, vp(go), None, None, s, None, None)]
    for k, call in enumerate(calls):
        assert call() == LIW_EINVAL, k
    for g in (-1, G):
        assert L.liw_gmap_last_info(h, gst, g, None, None) == LIW_EINVAL and L.liw_gmap_members(h, gst, g, None, None) == LIW_EINVAL
        assert L.liw_gmap_get(h, gst, g, None, 0) == LIW_EINVAL and L.liw_gmap_write_pgm(h, gst, g, b"x", None) == LIW_EINVAL
        assert L.liw_gmap_device_data(h, gst, g) is None
    assert L.liw_gmap_last_info(h, None, 0, None, None) == LIW_EINVAL
    torch.cuda.synchronize()
    assert fm._buf.cpu().numpy().tobytes() == snap[0].tobytes() and gm._buf.cpu().numpy().tobytes() == snap[1].tobytes()
    assert bool((gm.gstatus == 77).all()) and bool((gm.ginfo == 0x5A).all())
    fm.close()
    gm.close()
