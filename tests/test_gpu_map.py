"""The occupancy-grid map on the MI355X (include/liw_map.h) against the literal serial walk: tests/map_reference.py (Python)
for small cases, tests/cpp/map_serial.cpp (the same walk in C++) for large ones.  Every grid comparison is exact: zero cells
may differ, and width, height, origin, rays, samples and the four counts are equal.  Covered: synthetic rooms under random
SE(3) transforms, the truncation quirk at column / row 0, rays whose length is an exact step-table entry and one ulp either
side, degenerate inputs, sub-maps revisiting the same walls, re-rendering a store with other poses, render (poses) against
render_tf, determinism at 2 000 x 1 080 points, capacity, and an end-to-end replay with --map."""
import ctypes as C
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import map_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.05
LIW_ENOMEM, LIW_EINVAL = -12, -22   # include/liw_window.h
BIG = dict(max_submaps=2048, max_points=2300000, max_cells=1 << 22)
SMALL = dict(max_submaps=64, max_points=100000, max_cells=1 << 20)


def _replay():
    return importlib.import_module("2dliw-slam_amd.replay")


def _tf(x, y, yaw, z=0.0, roll=0.0, pitch=0.0):
    Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
    Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    return np.concatenate([(Rz @ Ry @ Rx).reshape(9), [x, y, z]])


def _scan(room, x, y, yaw, n_rays, rng, noise=0.004):
    """laser-frame points [m][3] of a scan cast from (x, y, yaw) in the world (misses dropped, as liw_laser_to_points does)"""
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = (x, y)
    rg, amin, inc = _replay().cast_scan_moving(room, lambda t: T, 0.0, n_rays, 2 * np.pi * 0.75, 0.0, noise, rng)
    a = float(amin) + float(inc) * np.arange(n_rays)
    ok = np.isfinite(rg) & (rg > 0.1)
    r = rg[ok].astype(np.float64)
    return np.stack([r * np.cos(a[ok]), r * np.sin(a[ok]), np.zeros(r.size)], axis=1)


def _room_case(rng, K, n_rays, tilt=0.03, room=None):
    """K scans of the room from random poses inside it, each with its world <- laser transform (small roll / pitch: dz != 0)"""
    room = _replay().replay_room() if room is None else room
    tfs, subs = [], []
    for _ in range(K):
        a = rng.uniform(-np.pi, np.pi)
        x, y, yaw = 5.0 * np.cos(a), 5.0 + 5.0 * np.sin(a), rng.uniform(-np.pi, np.pi)
        subs.append(_scan(room, x, y, yaw, n_rays, rng))
        tfs.append(_tf(x, y, yaw, rng.uniform(-0.05, 0.05), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)))
    return np.array(tfs), subs


def _map(liw, synth, dims=SMALL, res=RES, prm=None):
    return liw.gridmap.GridMap(synth.office_params() if prm is None else prm, dict(resolution=res), dims)


def _assert_equal(info, grid, want):
    print("map %d x %d, rays %d, samples %d, counts %s" % (want["width"], want["height"], want["rays"], want["samples"], want["counts"]))
    assert (info["width"], info["height"]) == (want["width"], want["height"])
    assert (info["origin_x"], info["origin_y"]) == (want["origin_x"], want["origin_y"])
    assert info["resolution"] == want["resolution"]
    assert (info["rays"], info["samples"]) == (want["rays"], want["samples"])
    assert {-1: info["unknown"], 0: info["free_cells"], 50: info["hit_once"], 100: info["hit_more"]} == want["counts"]
    assert grid.shape == want["grid"].shape
    assert int((grid != want["grid"]).sum()) == 0


def _render_and_check(liw, synth, tfs, subs, want, dims=SMALL, res=RES):
    m = _map(liw, synth, dims, res)
    for k, s in enumerate(subs):
        assert m.add_submap(s) == k
    info = m.render_tf(tfs)
    assert info == m.info
    _assert_equal(info, m.grid(), want)
    return m


# ------------------------------------------------------------------------------------------------------------- rooms
@pytest.mark.parametrize("K,n_rays,seed", [(6, 40, 1), (3, 300, 2), (12, 90, 3)])
def test_rooms_equal_the_python_walk(liw, synth, K, n_rays, seed):
    rng = np.random.default_rng(seed)
    tfs, subs = _room_case(rng, K, n_rays)
    if n_rays == 40:   # sparse scans of the same place: some cells are hit exactly once, some twice
        subs[1], tfs[1] = subs[0].copy(), tfs[0].copy()
    want = ref.render(tfs, subs, RES)
    if n_rays == 40:
        assert all(want["counts"][v] > 0 for v in (-1, 0, 50, 100)), want["counts"]
    assert want["counts"][0] > 0 and want["counts"][-1] > 0 and want["counts"][50] + want["counts"][100] > 0
    _render_and_check(liw, synth, tfs, subs, want)


def test_other_resolutions(liw, synth):
    rng = np.random.default_rng(8)
    tfs, subs = _room_case(rng, 3, 60)
    for res in (0.1, 0.03):
        _render_and_check(liw, synth, tfs, subs, ref.render(tfs, subs, res), res=res)


def test_truncation_toward_zero_at_column_and_row_zero(liw, synth):
    """The emit origin lies up to one cell left of / below the bounding box: samples with a quotient in (-1, 0) land in column
    0 / row 0 (int() truncates toward zero) and count as inside."""
    rng = np.random.default_rng(4)
    n = 60
    pts = np.stack([rng.uniform(0.03, 3.0, n), rng.uniform(0.02, 2.0, n), rng.uniform(-0.01, 0.01, n)], axis=1)
    pts[0] = (0.03, 1.0, 0.0)
    pts[1] = (1.0, 0.02, 0.0)
    tfs = np.array([_tf(0.0, 0.0, 0.0)])
    want = ref.render(tfs, [pts], RES)
    assert want["neg_col0"] > 0 and want["neg_row0"] > 0, (want["neg_col0"], want["neg_row0"])
    _render_and_check(liw, synth, tfs, [pts], want)
    # one cell further out the origin's own samples fall outside (quotient <= -1) and are skipped
    pts2 = pts + np.array([0.05, 0.05, 0.0])
    _render_and_check(liw, synth, tfs, [pts2], ref.render(tfs, [pts2], RES))


def test_ray_lengths_at_the_step_table_edge(liw, synth):
    """len == T[k] exactly, and one ulp either side (the `tr <= len` edge), for k inside and beyond the LDS part of the table"""
    T = liw.gridmap.step_table(RES, 2000)
    pts = []
    for k in (1, 2, 6, 7, 40, 123, 777, 1535, 1536, 1537, 1900):
        for v in (T[k], np.nextafter(T[k], 0.0), np.nextafter(T[k], np.inf)):
            pts.append((v, 0.0, 0.0))          # identity transform: len = sqrt(v * v) = v
            pts.append((0.0, -v, 0.0))
    pts = np.array(pts)
    tfs = np.array([_tf(0.0, 0.0, 0.0)])
    want = ref.render(tfs, [pts], RES)
    assert want["samples"] > 0
    _render_and_check(liw, synth, tfs, [pts], want)
    # the same lengths in a general direction and position
    tfs2 = np.array([_tf(1.3, -0.7, 0.61, 0.02, 0.01, -0.02)])
    _render_and_check(liw, synth, tfs2, [pts], ref.render(tfs2, [pts], RES))


def test_degenerate_inputs(liw, synth):
    tf = np.array([_tf(0.4, -0.2, 0.3)])
    # K = 0 and a sub-map without points: a 0 x 0 map
    m = _map(liw, synth)
    info = m.render_tf(np.zeros((0, 12)))
    assert (info["width"], info["height"], info["rays"], info["samples"]) == (0, 0, 0, 0) and m.grid().size == 0
    assert m.add_submap(np.zeros((0, 3))) == 0
    _assert_equal(m.render_tf(tf), m.grid(), ref.render(tf, [np.zeros((0, 3))], RES))
    # a single point
    one = [np.array([[1.0, 0.5, 0.0]])]
    w = ref.render(tf, one, RES)
    assert (w["width"], w["height"]) == (1, 1) and w["counts"][50] == 1
    _render_and_check(liw, synth, tf, one, w)
    # a point equal to its origin marks only its target cell; a NaN / inf point is ignored
    pts = [np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [np.nan, 0.2, 0.0], [0.5, np.inf, 0.0], [2.0, -1.0, 0.0]])]
    w = ref.render(tf, pts, RES)
    assert w["rays"] == 3
    _render_and_check(liw, synth, tf, pts, w)
    only_bad = [np.array([[np.nan, 0.0, 0.0]])]
    w = ref.render(tf, only_bad, RES)
    assert (w["width"], w["height"], w["rays"]) == (0, 0, 0)
    _render_and_check(liw, synth, tf, only_bad, w)
    # the zero-length ray alone: one cell, hit once, no sample
    zero = [np.array([[0.0, 0.0, 0.0]])]
    w = ref.render(tf, zero, RES)
    assert w["samples"] == 0 and w["counts"][50] == 1
    _render_and_check(liw, synth, tf, zero, w)


# ------------------------------------------------------------------------------------------------------------- sub-maps
def _world_consistent(rng, K, n_rays):
    """K scans of one room, each rendered at the pose it was cast from (no tilt): walls are hit by several sub-maps"""
    room = _replay().replay_room()
    tfs, subs = [], []
    for k in range(K):
        a = 2 * np.pi * k / K
        x, y, yaw = 5.0 * np.cos(a), 5.0 + 5.0 * np.sin(a), a + np.pi / 2
        subs.append(_scan(room, x, y, yaw, n_rays, rng, noise=0.0))
        tfs.append(_tf(x, y, yaw))
    return np.array(tfs), subs


def test_sub_maps_revisiting_the_same_walls(liw, synth):
    rng = np.random.default_rng(6)
    tfs, subs = _world_consistent(rng, 8, 120)
    want = ref.render(tfs, subs, RES)
    single = ref.render(tfs[:1], subs[:1], RES)
    assert want["counts"][100] > single["counts"][100] and want["counts"][50] > 0   # 50 -> 100 happens across sub-maps
    m = _render_and_check(liw, synth, tfs, subs, want)
    # the same store with other poses == a fresh handle with those poses: nothing survives from the previous render
    tfs2 = tfs.copy()
    tfs2[:, 9] += rng.uniform(-0.5, 0.5, 8)
    tfs2[:, 10] += rng.uniform(-0.5, 0.5, 8)
    want2 = ref.render(tfs2, subs, RES)
    assert (want2["width"], want2["height"]) != (want["width"], want["height"]) or not np.array_equal(want2["grid"], want["grid"])
    _assert_equal(m.render_tf(tfs2), m.grid(), want2)
    _render_and_check(liw, synth, tfs2, subs, want2)
    # a prefix of the store, then everything again
    _assert_equal(m.render_tf(tfs[:3]), m.grid(), ref.render(tfs[:3], subs[:3], RES))
    _assert_equal(m.render_tf(tfs), m.grid(), want)
    # clear() forgets the sub-maps
    m.clear()
    assert m.num_submaps() == 0 and m.info["width"] == 0
    assert m.add_submap(subs[2]) == 0
    _assert_equal(m.render_tf(tfs[2:3]), m.grid(), ref.render(tfs[2:3], subs[2:3], RES))


def _poses_case():
    """five sub-maps of the replay room and five 6-dof poses to render them at (shared with tests/test_second_config_frontend.py)"""
    rng = np.random.default_rng(9)
    _, subs = _room_case(rng, 5, 50)
    poses = np.concatenate([rng.uniform(-3, 3, (5, 3)), rng.uniform(-0.4, 0.4, (5, 3))], axis=1)
    poses[:, 5] = rng.uniform(-3, 3, 5)
    return subs, poses


def test_render_with_poses_equals_render_tf(liw, synth):
    _check_render_with_poses(liw, synth, None)


def test_render_with_poses_equals_render_tf_skewed_extrinsic(liw, synth):
    """the same at second_config.skewed_params: a generic laser rotation, which the loader's quaternion round trip changes, and another
    translation, so a transposed or office T_imu_to_laser in the composition cannot pass"""
    import second_config as sc
    _check_render_with_poses(liw, synth, sc.skewed_params(synth))


def _check_render_with_poses(liw, synth, prm):
    subs, poses = _poses_case()
    m = _map(liw, synth, prm=prm)
    if prm is not None:
        import second_config as sc
        assert np.array_equal(m.T_imu_to_laser, sc.held_extrinsic(liw, prm))
    for s in subs:
        m.add_submap(s)
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    Til = np.ascontiguousarray(np.concatenate([m.T_imu_to_laser[:3, :3].reshape(9), m.T_imu_to_laser[:3, 3]]))
    tfs = np.zeros((5, 12))
    for k in range(5):
        A = np.zeros(12)
        p, q = np.ascontiguousarray(poses[k, :3]), np.ascontiguousarray(poses[k, 3:])
        L.liw_lie_make_tf(pd(p), pd(q), pd(A))
        L.liw_lie_mul(pd(A), pd(Til), pd(tfs[k]))
    a = m.render(poses)
    ga = m.grid().copy()
    b = m.render_tf(tfs)
    assert a == b and np.array_equal(ga, m.grid())
    _assert_equal(b, m.grid(), ref.render(tfs, subs, RES))


# ------------------------------------------------------------------------------------------------------------- large
def test_large_render_is_deterministic_and_equals_the_serial_walk(liw, synth, tmp_path):
    """K = 2 000 key frames x 1 080 rays: two renders bit-identical, and equal to map_serial.cpp exactly"""
    rng = np.random.default_rng(12)
    K, n_rays = 2000, 1080
    room = _replay().pillar_room()
    tfs, subs = [], []
    for k in range(K):
        a = 2 * np.pi * 3 * k / K
        x, y, yaw = 5.0 * np.cos(a) + rng.normal(0, 0.02), 5.0 + 5.0 * np.sin(a) + rng.normal(0, 0.02), a + np.pi / 2 + rng.normal(0, 0.01)
        subs.append(_scan(room, x, y, yaw, n_rays, rng))
        tfs.append(_tf(x, y, yaw, rng.normal(0, 0.01), rng.normal(0, 0.005), rng.normal(0, 0.005)))
    tfs = np.array(tfs)
    m = _map(liw, synth, BIG)
    for s in subs:
        m.add_submap(s)
    i1 = m.render_tf(tfs)
    g1 = m.grid().copy()
    i2 = m.render_tf(tfs)
    g2 = m.grid()
    assert i1 == i2 and np.array_equal(g1, g2)
    assert i1["rays"] > 0.9 * K * n_rays
    want = ref.render_serial(ref.build_serial(tmp_path), tfs, subs, RES)
    assert all(want["counts"][v] > 0 for v in (-1, 0, 50, 100))
    _assert_equal(i1, g1, want)


def test_capacity(liw, synth):
    rng = np.random.default_rng(14)
    tfs, subs = _room_case(rng, 4, 80)
    n = [s.shape[0] for s in subs]
    want3 = ref.render(tfs[:3], subs[:3], RES)
    dims = dict(max_submaps=3, max_points=n[0] + n[1] + n[2], max_cells=want3["width"] * want3["height"])
    m = _map(liw, synth, dims)
    for k in range(3):
        assert m.add_submap(subs[k]) == k
    _assert_equal(m.render_tf(tfs[:3]), m.grid(), want3)
    keep = m.grid().copy()
    # max_submaps
    with pytest.raises(liw.LiwError) as e:
        m.add_submap(np.zeros((0, 3)))
    assert e.value.code == LIW_ENOMEM and m.num_submaps() == 3
    # max_cells: spread the poses so that the bounding box grows; info is filled, the previous grid stays
    far = tfs[:3].copy()
    far[2, 9] += 30.0
    info = liw.gridmap.MapInfoC()
    r = m.L.liw_map_render_tf(m.h, 3, far.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
    assert r == LIW_ENOMEM
    wf = ref.render(far, subs[:3], RES)
    assert (info.width, info.height, info.origin_x, info.origin_y) == (wf["width"], wf["height"], wf["origin_x"], wf["origin_y"])
    assert info.width * info.height > dims["max_cells"]
    assert m.info["width"] == want3["width"] and np.array_equal(m.grid(), keep)
    _assert_equal(m.render_tf(tfs[:3]), m.grid(), want3)
    # max_points
    m2 = _map(liw, synth, dict(max_submaps=8, max_points=n[0] + n[1] + 5, max_cells=1 << 20))
    assert m2.add_submap(subs[0]) == 0 and m2.add_submap(subs[1]) == 1
    with pytest.raises(liw.LiwError) as e:
        m2.add_submap(subs[2])
    assert e.value.code == LIW_ENOMEM and m2.num_submaps() == 2
    assert m2.add_submap(subs[2][:5]) == 2
    sub3 = [subs[0], subs[1], subs[2][:5]]
    _assert_equal(m2.render_tf(tfs[:3]), m2.grid(), ref.render(tfs[:3], sub3, RES))
    # more transforms than sub-maps is a bad argument
    with pytest.raises(liw.LiwError) as e:
        m2.render_tf(tfs)
    assert e.value.code == LIW_EINVAL


def test_write_pgm_of_a_render(liw, synth, tmp_path):
    rng = np.random.default_rng(15)
    tfs, subs = _room_case(rng, 3, 60)
    m = _map(liw, synth)
    for s in subs:
        m.add_submap(s)
    info = m.render_tf(tfs)
    stem = str(tmp_path / "map")
    m.write_pgm(stem, (205, 254, 100, 0))   # distinct greys: the four values come back
    assert np.array_equal(_read_pgm(stem + ".pgm", (205, 254, 100, 0)), m.grid())
    m.write_pgm(stem)                       # default: 50 and 100 are both black
    assert np.array_equal(_read_pgm(stem + ".pgm"), _fold(m.grid()))
    assert _read_yaml(stem + ".yaml") == ("map.pgm", info["resolution"], info["origin_x"], info["origin_y"])


# ------------------------------------------------------------------------------------------------------------- end to end
def _read_pgm(path, palette=(205, 254, 0, 0)):
    """decode a P5 file back to cell values through the palette, bottom row first.  Values that share a grey (50 and 100 in the
    default palette, both black) come back as 100: compare against _fold() of the expected grid then."""
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    assert magic == b"P5" and maxval == b"255"
    w, h = (int(v) for v in dims.split())
    img = np.frombuffer(body, dtype=np.uint8).reshape(h, w)[::-1]
    out = np.full((h, w), 127, dtype=np.int8)
    for grey, val in zip(palette, (-1, 0, 50, 100)):
        out[img == grey] = val if palette.count(grey) == 1 else 100
    assert not (out == 127).any()
    return out


def _fold(grid, palette=(205, 254, 0, 0)):
    g = grid.copy()
    if palette[2] == palette[3]:
        g[g == 50] = 100
    return g


def _read_yaml(path):
    d = {}
    for ln in open(path):
        k, v = ln.split(":", 1)
        d[k.strip()] = v.strip()
    o = [float(v) for v in d["origin"].strip("[]").split(",")]
    return d["image"], float(d["resolution"]), o[0], o[1]


def test_replay_writes_the_map_of_the_circle(liw, synth, tmp_path):
    replay = _replay()
    libdir = os.path.dirname(liw.LIB_PATH)
    exe = str(tmp_path / "replay_log")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "replay_log.cpp"), "-o",
                           exe, "-L", libdir, "-lliw_window", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    prm = synth.office_params()
    msgs, truth = replay.make_log(prm, duration=25.0, seed=3, room=replay.pillar_room())
    replay.write_log(str(tmp_path / "log.bin"), msgs)
    out = str(tmp_path) + "/"
    stem = out + "map"
    r = subprocess.run([exe, str(tmp_path / "log.bin"), out, "--detect-loops", "--loop-dims", "512", "256", "--map", stem], capture_output=True,
                       timeout=600)
    err = r.stderr.decode()
    print(err)
    assert r.returncode == 0, err
    raw = open(stem + ".in", "rb").read()
    (K,) = struct.unpack_from("<i", raw, 0)
    o = 4
    poses, subs = [], []
    for _ in range(K):
        poses.append(np.frombuffer(raw, dtype=np.float64, count=6, offset=o)); o += 48
        (n,) = struct.unpack_from("<i", raw, o); o += 4
        subs.append(np.frombuffer(raw, dtype=np.float64, count=3 * n, offset=o).reshape(n, 3)); o += 24 * n
    assert o == len(raw) and K > 100 and sum(s.shape[0] for s in subs) > 100 * 300
    nk, nloop, solves, _ = struct.unpack("<4i", open(out + "backend.bin", "rb").read()[:16])
    assert solves >= 1 and K <= nk
    # T_w_l of every sub-map with the library's own host arithmetic, then the C++ serial walk
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    M = np.zeros(16)
    ctx = C.c_void_p(L.liw_create(C.byref(liw.params_struct(prm))))
    L.liw_get_extrinsics(ctx, None, pd(M))
    L.liw_destroy(ctx)
    M = M.reshape(4, 4)
    Til = np.ascontiguousarray(np.concatenate([M[:3, :3].reshape(9), M[:3, 3]]))
    tfs = np.zeros((K, 12))
    for k in range(K):
        A = np.zeros(12)
        p, q = np.ascontiguousarray(poses[k][:3]), np.ascontiguousarray(poses[k][3:])
        L.liw_lie_make_tf(pd(p), pd(q), pd(A))
        L.liw_lie_mul(pd(A), pd(Til), pd(tfs[k]))
    want = ref.render_serial(ref.build_serial(tmp_path), tfs, subs, RES)
    print("map %d x %d, %d sub-maps, rays %d, samples %d, counts %s" % (want["width"], want["height"], K, want["rays"], want["samples"], want["counts"]))
    got = _read_pgm(stem + ".pgm")
    assert got.shape == want["grid"].shape
    assert int((got != _fold(want["grid"])).sum()) == 0
    image, res, ox, oy = _read_yaml(stem + ".yaml")
    assert (image, res, ox, oy) == ("map.pgm", RES, want["origin_x"], want["origin_y"])
    # the same input through the Python interface gives the full four-valued grid
    m = _map(liw, synth, dict(max_submaps=K, max_points=sum(s.shape[0] for s in subs), max_cells=want["width"] * want["height"]))
    for s in subs:
        m.add_submap(s)
    _assert_equal(m.render(np.array(poses)), m.grid(), want)
    # the cell of every key frame's laser position is known (the sample tr = 0 of each of its rays)
    inside = 0
    for k in range(K):
        if subs[k].shape[0] == 0:
            continue
        x, y = int((tfs[k][9] - ox) / RES), int((tfs[k][10] - oy) / RES)
        if 0 <= x < want["width"] and 0 <= y < want["height"]:
            inside += 1
            assert got[y, x] != -1, (k, x, y)
    assert inside > K // 2
