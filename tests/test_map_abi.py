"""C ABI of the occupancy-grid map (include/liw_map.h), on any machine: the two checkers (tests/map_reference.py, the literal
walk in Python, and tests/cpp/map_serial.cpp, the same walk in C++) agree with each other; every liw_map_* name is exported and
listed in gridmap.MAP_EXPORTS; the header compiles as C99; the store size is a host-only query that grows with the dims and
rejects bad ones; every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback); the step table is the accumulated
sum bit for bit; the PGM / YAML writer is byte-identical to a Python rendering of the same array."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_map.h")


def _tf(rng, xy=3.0, tilt=0.05):
    """a random SE(3) as T12 with small roll / pitch"""
    r, p, y = rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-np.pi, np.pi)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return np.concatenate([(Rz @ Ry @ Rx).reshape(9), [rng.uniform(-xy, xy), rng.uniform(-xy, xy), rng.uniform(-0.1, 0.1)]])


def test_the_two_checkers_agree(tmp_path):
    """Python walk == C++ walk on a small case that holds all four cell values, a NaN point and a zero-length ray."""
    rng = np.random.default_rng(5)
    tfs = [_tf(rng) for _ in range(6)]
    subs = []
    for k in range(6):
        a = rng.uniform(-np.pi, np.pi, 25)
        d = rng.uniform(0.3, 4.0, 25)
        subs.append(np.stack([d * np.cos(a), d * np.sin(a), rng.uniform(-0.02, 0.02, 25)], axis=1))
    subs[1][3] = (np.nan, 1.0, 0.0)
    subs[2][0] = (0.0, 0.0, 0.0)
    subs[4] = subs[3].copy()      # the same walls seen again from sub-map 3's pose: cells hit twice
    tfs[4] = tfs[3].copy()
    py = ref.render(tfs, subs, 0.05)
    cc = ref.render_serial(ref.build_serial(tmp_path), tfs, subs, 0.05)
    assert all(py["counts"][v] > 0 for v in (-1, 0, 50, 100)), py["counts"]
    assert py["rays"] == 6 * 25 - 1
    for k in ("width", "height", "origin_x", "origin_y", "rays", "samples", "counts"):
        assert py[k] == cc[k], k
    assert np.array_equal(py["grid"], cc["grid"])


def test_map_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_map_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert declared
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.gridmap.MAP_EXPORTS)) == declared


def test_map_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_map.h"\nint f(void) { liw_map_params p = {0.05}; liw_map_dims d = {10, 1000, 10000}; size_t n;\n'
                   '  liw_map_info i; (void)i; return liw_map_store_bytes(&p, &d, &n); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_store_bytes_monotone_and_rejects_bad_dims(liw):
    gm = liw.gridmap
    p = gm.office_map_params()
    last = 0
    for K, P, Cn in [(1, 1, 1), (10, 5000, 10000), (10, 50000, 10000), (10, 50000, 1000000), (2000, 50000, 1000000), (2000, 2200000, 4000000)]:
        b = gm.store_bytes(p, dict(max_submaps=K, max_points=P, max_cells=Cn))
        assert b > last
        last = b
    assert last >= 2200000 * 24 + 4000000
    for K, P, Cn in [(0, 10, 10), (-1, 10, 10), (10, 0, 10), (10, -5, 10), (10, 10, 0), (10, 10, -1), (10, 10, 1 << 31), (10, 1 << 31, 10)]:
        with pytest.raises(ValueError):
            gm.store_bytes(p, dict(max_submaps=K, max_points=P, max_cells=Cn))
    for res in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gm.store_bytes(dict(resolution=res), dict(max_submaps=1, max_points=1, max_cells=1))


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the handle exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
    gm = liw.gridmap
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    m = gm.GridMap(synth.office_params(), dims=dict(max_submaps=4, max_points=64, max_cells=4096))
    L = m.L
    pts, tf, poses, info = np.zeros((2, 3)), np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), np.zeros(6), gm.MapInfoC()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(16, dtype=np.int8)
    assert L.liw_map_add_submap(m.h, 2, pd(pts)) == liw.LIW_ENODEV
    assert L.liw_map_render_tf(m.h, 0, pd(tf), C.byref(info)) == liw.LIW_ENODEV
    assert L.liw_map_render(m.h, 0, pd(poses), C.byref(info)) == liw.LIW_ENODEV
    assert L.liw_map_get(m.h, out.ctypes.data_as(C.POINTER(C.c_byte)), 16) == liw.LIW_ENODEV
    assert L.liw_map_write_pgm(m.h, b"/nonexistent/x", None) == liw.LIW_ENODEV
    assert L.liw_map_device_data(m.h) is None
    assert L.liw_map_num_submaps(m.h) == 0
    assert b"gfx950" in L.liw_map_last_error(m.h)
    with pytest.raises(liw.LiwError):
        m.add_submap(pts)
    assert m.info["width"] == 0 and m.info["height"] == 0 and m.info["resolution"] == 0.05
    assert np.allclose(m.T_imu_to_laser[:3, 3], np.asarray(synth.office_params()["T_imu_to_laser"], dtype=float).reshape(4, 4)[:3, 3])


@pytest.mark.parametrize("res", [0.05, 0.1, 0.03])
def test_step_table_is_the_accumulated_sum(liw, res):
    n = 4000
    T = liw.gridmap.step_table(res, n)
    step = res / 2
    acc, tr = np.zeros(n), 0.0
    for k in range(n):
        acc[k] = tr
        tr += step
    assert np.array_equal(T, acc) and np.array_equal(T, ref.step_table(res, n))
    assert T[0] == 0.0 and T[1] == step
    if res == 0.05:
        prod = np.arange(n) * step
        differ = np.nonzero(T != prod)[0]
        # the input is only valid if the accumulated sum is NOT k * step: a kernel computing k * step would pass otherwise
        assert differ.size > n // 2 and differ[0] == 6, (differ.size, differ[:3])
        assert np.abs(T - prod).max() < 1e-10
    with pytest.raises(ValueError):
        liw.gridmap.step_table(0.0, 4)
    assert liw.gridmap.step_table(res, 0).size == 0


def _pgm_bytes(grid, palette):
    lut = {-1: palette[0], 0: palette[1], 50: palette[2], 100: palette[3]}
    h, w = grid.shape
    img = np.array([[lut[int(v)] for v in row] for row in grid[::-1]], dtype=np.uint8).reshape(h, w)
    return b"P5\n%d %d\n255\n" % (w, h) + img.tobytes()


def _yaml(path):
    d = {}
    for ln in open(path):
        k, v = ln.split(":", 1)
        d[k.strip()] = v.strip()
    return d


@pytest.mark.parametrize("palette", [None, (7, 200, 90, 13)])
def test_write_pgm_grid_is_byte_identical(liw, tmp_path, palette):
    gm = liw.gridmap
    rng = np.random.default_rng(3)
    grid = rng.choice(np.array([-1, 0, 50, 100], dtype=np.int8), size=(23, 37))
    res, ox, oy = 0.05, -3.4500000000000001776, 12.123456789012345
    stem = str(tmp_path / "m")
    gm.write_pgm_grid(stem, grid, res, ox, oy, palette)
    assert open(stem + ".pgm", "rb").read() == _pgm_bytes(grid, gm.DEFAULT_PALETTE if palette is None else palette)
    y = _yaml(stem + ".yaml")
    assert y["image"] == "m.pgm" and float(y["resolution"]) == res
    o = [float(v) for v in y["origin"].strip("[]").split(",")]
    assert o == [ox, oy, 0.0]
    assert (y["negate"], float(y["occupied_thresh"]), float(y["free_thresh"])) == ("0", 0.65, 0.196)
    with pytest.raises(ValueError):
        bad = grid.copy()
        bad[2, 2] = 7
        gm.write_pgm_grid(stem, bad, res, ox, oy, palette)
    gm.write_pgm_grid(stem + "e", np.zeros((0, 0), dtype=np.int8), res, ox, oy, palette)
    assert open(stem + "e.pgm", "rb").read() == b"P5\n0 0\n255\n"
