"""C ABI of the shared map of a group of fleet robots (include/liw_map_group.h), on any machine: every liw_gmap_* name is exported and
listed in map_batch.GMAP_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad dims and add up part by
part, and every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback) and writes nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_map_group.h")
LIW_EINVAL = -22


def test_gmap_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_gmap_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 13
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.map_batch.GMAP_EXPORTS)) == declared
    assert liw.FleetGroupMap is liw.map_batch.FleetGroupMap


def test_gmap_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_map_group.h"\nint f(void) { liw_gmap_dims d = {3, 4096}; size_t n; liw_gmap_layout_info i;\n'
                   '  return liw_gmap_store_bytes(&d, &n) + liw_gmap_layout(&d, &i) + LIW_FMAP_OK + LIW_FMAP_EMPTY; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_size_functions_reject_bad_dims_and_add_up(liw):
    fm = liw.map_batch
    for G, Cc in ((3, 4096), (1, 1), (64, 1 << 20), (5, 999), (2, 0x7FFFFFF0)):
        lay = fm.group_layout(G, Cc)
        assert fm.group_store_bytes(G, Cc) == lay["bytes"] == G * lay["group_bytes"] > 0
        assert lay["cell_bytes"] == -(-Cc // 16) * 16
        offs = [lay["bits_off"], lay["grid_off"], lay["group_bytes"]]
        assert offs[0] == 256 and all(o % 256 == 0 for o in offs)     # the header, then the parts, 256-byte aligned
        for a, b in zip(offs, offs[1:]):                              # every part has room, and wastes less than one alignment unit
            assert lay["cell_bytes"] <= b - a < lay["cell_bytes"] + 256
    assert fm.group_store_bytes(4, 4096) > fm.group_store_bytes(3, 4096) and fm.group_store_bytes(3, 40960) > fm.group_store_bytes(3, 4096)
    for G, Cc in ((0, 4096), (-1, 4096), (3, 0), (3, -5), (3, 0x7FFFFFF1), (3, 0x7FFFFFFF)):
        for f in (fm.group_store_bytes, fm.group_layout):
            with pytest.raises(liw.LiwError) as ei:
                f(G, Cc)
            assert ei.value.code == LIW_EINVAL, (G, Cc)
    L = fm._lib()
    n = C.c_size_t(7)
    d = fm.GmapDimsC(3, 4096)
    assert L.liw_gmap_store_bytes(None, C.byref(n)) == LIW_EINVAL and n.value == 7
    assert L.liw_gmap_store_bytes(C.byref(d), None) == LIW_EINVAL
    assert L.liw_gmap_layout(C.byref(d), None) == LIW_EINVAL and L.liw_gmap_layout(None, C.byref(fm.GmapLayoutC())) == LIW_EINVAL


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback) and writes nothing."""
    fm = liw.map_batch
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L = fm._lib()
    prm = synth.office_params()
    Til = np.ascontiguousarray(np.asarray(prm["T_imu_to_laser"], dtype=np.float64).reshape(16))
    ps = liw.gridmap.params_struct(liw.gridmap.office_map_params())
    ds = fm.dims_struct(dict(B=4, max_submaps=10, max_points=400, max_cells=4096, max_steps=512))
    f = C.c_void_p(L.liw_fmap_create(C.byref(ps), C.byref(ds), Til.ctypes.data_as(C.POINTER(C.c_double)), 1, 0))
    assert f
    gd = fm.GmapDimsC(3, 4096)
    assert not L.liw_gmap_create(None, C.byref(gd))
    assert not L.liw_gmap_create(f, None)
    assert not L.liw_gmap_create(f, C.byref(fm.GmapDimsC(0, 4096)))
    h = C.c_void_p(L.liw_gmap_create(f, C.byref(gd)))
    assert h
    L.liw_fmap_destroy(f)       # the group ctx copied what it needs
    try:
        buf = np.full(64, 7.0)   # never dereferenced: the device check comes first
        snap = buf.tobytes()
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_gmap_reset(h, p, None, None) == E
        assert L.liw_gmap_render_tf(h, p, p, p, 120, p, p, None, p, p, None) == E
        assert L.liw_gmap_render(h, p, p, p, 60, p, None, None, p, p, None) == E
        assert L.liw_gmap_last_info(h, p, 0, None, None) == E
        assert L.liw_gmap_members(h, p, 0, None, None) == E
        assert L.liw_gmap_get(h, p, 0, None, 0) == E
        assert L.liw_gmap_write_pgm(h, p, 0, b"/nonexistent/x", None) == E
        assert buf.tobytes() == snap
        # pure pointer arithmetic: group 1's grid lies one group region behind group 0's
        lay = fm.group_layout(3, 4096)
        d0, d1 = L.liw_gmap_device_data(h, p, 0), L.liw_gmap_device_data(h, p, 1)
        assert d0 == buf.ctypes.data + lay["grid_off"] and d1 - d0 == lay["group_bytes"]
        assert L.liw_gmap_device_data(h, p, 3) is None and L.liw_gmap_device_data(h, p, -1) is None
        assert L.liw_gmap_last_error(h)
    finally:
        L.liw_gmap_destroy(h)
