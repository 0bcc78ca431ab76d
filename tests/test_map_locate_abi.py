"""C ABI of the localisation in a held occupancy grid (include/liw_map_locate.h), on any machine: every liw_floc_* name is exported
and listed in map_locate.FLOC_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad dims and add up part
by part, and every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback) and writes nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_map_locate.h")
LIW_EINVAL = -22


def test_floc_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_floc_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 11
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.map_locate.FLOC_EXPORTS)) == declared
    assert liw.FleetLocalizer is liw.map_locate.FleetLocalizer


def test_floc_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_map_locate.h"\nint f(void) { liw_floc_dims d = {8, 3, 4096, 64}; size_t n; liw_floc_layout_info i;\n'
                   '  return liw_floc_store_bytes(&d, &n) + liw_floc_layout(&d, &i) + LIW_FLOC_FIELD_OK + LIW_FLOC_FIELD_EMPTY + LIW_FLOC_FIELD_OVER\n'
                   '         + LIW_FLOC_OK + LIW_FLOC_NO_MAP + LIW_FLOC_NO_POINTS + LIW_FLOC_BAD_PRIOR + LIW_FLOC_MAX_W + LIW_FLOC_MAX_THETA; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_size_functions_reject_bad_dims_and_add_up(liw):
    ml = liw.map_locate
    for Q, M, Cc, T in ((8, 3, 4096, 64), (1, 1, 1, 1), (4096, 64, 1 << 20, 256), (5, 2, 999, 41), (2, 1, 0x7FFFFFF0, 17)):
        lay = ml.layout(Q, M, Cc, T)
        assert ml.store_bytes(Q, M, Cc, T) == lay["bytes"] == M * lay["map_bytes"] + Q * lay["row_bytes"] > 0
        assert lay["field_bytes"] == -(-Cc // 16) * 16
        assert lay["field_off"] == 256 and lay["map_bytes"] % 256 == 0 and lay["partial_off"] == M * lay["map_bytes"]
        assert lay["field_bytes"] <= lay["map_bytes"] - lay["field_off"] < lay["field_bytes"] + 256       # room, and less than one unit wasted
        assert lay["row_bytes"] % 256 == 0 and 32 * T <= lay["row_bytes"] < 32 * T + 256
        assert lay["cell_chunks"] >= 1
    assert ml.store_bytes(9, 3, 4096, 64) > ml.store_bytes(8, 3, 4096, 64) and ml.store_bytes(8, 4, 4096, 64) > ml.store_bytes(8, 3, 4096, 64)
    assert ml.store_bytes(8, 3, 40960, 64) > ml.store_bytes(8, 3, 4096, 64) and ml.store_bytes(8, 3, 4096, 65) > ml.store_bytes(8, 3, 4096, 64)
    for dims in ((0, 3, 4096, 64), (-1, 3, 4096, 64), (8, 0, 4096, 64), (8, -2, 4096, 64), (8, 3, 0, 64), (8, 3, -5, 64), (8, 3, 0x7FFFFFF1, 64),
                 (8, 3, 4096, 0), (8, 3, 4096, -1), (8, 3, 4096, 257)):
        for f in (ml.store_bytes, ml.layout):
            with pytest.raises(liw.LiwError) as ei:
                f(*dims)
            assert ei.value.code == LIW_EINVAL, dims
    L = ml._lib()
    n = C.c_size_t(7)
    d = ml.FlocDimsC(8, 3, 4096, 64)
    assert L.liw_floc_store_bytes(None, C.byref(n)) == LIW_EINVAL and n.value == 7
    assert L.liw_floc_store_bytes(C.byref(d), None) == LIW_EINVAL
    assert L.liw_floc_layout(C.byref(d), None) == LIW_EINVAL and L.liw_floc_layout(None, C.byref(ml.FlocLayoutC())) == LIW_EINVAL


def test_angle_table():
    import importlib
    ml = importlib.import_module("2dliw-slam_amd.map_locate")
    t = ml.angle_table(np.radians(8.0), np.radians(1.0))
    assert t.shape == (17, 2) and t.dtype == np.float64 and t[8].tolist() == [1.0, 0.0]
    assert np.array_equal(t[:, 0], t[::-1, 0]) and np.array_equal(t[:, 1], -t[::-1, 1])
    assert np.allclose(np.degrees(np.arctan2(t[:, 1], t[:, 0])), np.arange(-8, 9))
    assert ml.angle_table(0.0, 0.1).tolist() == [[1.0, 0.0]] and ml.FleetLocalizer.angle_table(0.25, 0.1).shape == (5, 2)


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback) and writes nothing."""
    ml = liw.map_locate
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L = ml._lib()
    prm = synth.office_params()
    Til = np.ascontiguousarray(np.asarray(prm["T_imu_to_laser"], dtype=np.float64).reshape(16))
    pd = Til.ctypes.data_as(C.POINTER(C.c_double))
    d = ml.FlocDimsC(8, 3, 4096, 64)
    assert not L.liw_floc_create(None, pd, 1, 0)
    assert not L.liw_floc_create(C.byref(d), None, 1, 0)
    assert not L.liw_floc_create(C.byref(ml.FlocDimsC(8, 3, 4096, 300)), pd, 1, 0)
    h = C.c_void_p(L.liw_floc_create(C.byref(d), pd, 1, 0))
    assert h
    try:
        buf = np.full(64, 7.0)   # never dereferenced: the device check comes first
        snap = buf.tobytes()
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_floc_build(h, p, p, 4096, 256, p, None, None) == E
        assert L.liw_floc_match(h, p, p, p, 8, p, p, p, 5, 4, 0, None, p, p, p, p, None) == E
        assert L.liw_floc_link_tf(h, p, p, 6, p, None, p, p, None) == E
        assert L.liw_floc_field_info(h, p, 0, None, None, None, None) == E
        assert L.liw_floc_get_field(h, p, 0, None, 0) == E
        assert buf.tobytes() == snap
        # pure pointer arithmetic: map 1's field lies one map region behind map 0's
        lay = ml.layout(8, 3, 4096, 64)
        d0, d1 = L.liw_floc_device_field(h, p, 0), L.liw_floc_device_field(h, p, 1)
        assert d0 == buf.ctypes.data + lay["field_off"] and d1 - d0 == lay["map_bytes"]
        assert L.liw_floc_device_field(h, p, 3) is None and L.liw_floc_device_field(h, p, -1) is None
        assert L.liw_floc_last_error(h)
        assert L.liw_floc_build(None, p, p, 4096, 256, p, None, None) == LIW_EINVAL
    finally:
        L.liw_floc_destroy(h)
