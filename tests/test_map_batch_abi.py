"""C ABI of the fleet's occupancy-grid maps (include/liw_map_batch.h), on any machine: every liw_fmap_* name is exported and listed
in map_batch.FMAP_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad params / dims and add up, every
compute entry fails with LIW_ENODEV without a GPU (no CPU fallback), and liw_fpg_pose_offset is the offset of the documented region
layout of include/liw_posegraph_batch.h."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_map_batch.h")
LIW_EINVAL = -22


def test_fmap_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_fmap_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 17
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.map_batch.FMAP_EXPORTS)) == declared
    assert liw.FleetMapper is liw.map_batch.FleetMapper
    assert "liw_fpg_pose_offset" in liw.posegraph_batch.FPG_EXPORTS and hasattr(L, "liw_fpg_pose_offset")


def test_fmap_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_map_batch.h"\n#include "liw_posegraph_batch.h"\nint f(void) { liw_map_params p = {0.05};\n'
                   '  liw_fmap_dims d = {4, 10, 400, 4096, 512}; liw_fpg_dims g = {4, 10, 2}; size_t n, o; liw_fmap_layout_info i;\n'
                   '  return liw_fmap_store_bytes(&p, &d, &n) + liw_fmap_layout(&p, &d, &i) + liw_fpg_pose_offset(&g, &o)\n'
                   '         + LIW_FMAP_OK + LIW_FMAP_EMPTY + LIW_FMAP_OVER_CELLS + LIW_FMAP_RAY_TOO_LONG; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _dims(B=4, K=10, P=400, Cc=4096, S=512):
    return dict(B=B, max_submaps=K, max_points=P, max_cells=Cc, max_steps=S)


PARTS = ("offsets_off", "points_off", "index_off", "tf_off", "partial_off", "bits_off", "grid_off")


def test_size_functions_reject_bad_dims_and_add_up(liw):
    fm = liw.map_batch
    p = liw.gridmap.office_map_params()
    for d in (_dims(), _dims(B=1, K=1, P=1, Cc=1, S=4), _dims(B=1024, K=200, P=72000, Cc=1 << 20, S=2048), _dims(B=3, K=7, P=1001, Cc=999, S=77)):
        lay = fm.layout(p, d)
        B, K, P, Cc, S = (d[k] for k in fm.DIM_KEYS)
        assert fm.store_bytes(p, d) == lay["bytes"] == B * lay["robot_bytes"] + lay["shared_bytes"] > 0
        assert lay["shared_off"] == B * lay["robot_bytes"] and lay["shared_bytes"] >= 8 * S and lay["shared_bytes"] % 256 == 0
        assert lay["cell_bytes"] == -(-Cc // 16) * 16 and lay["partials"] == min(-(-P // 256), 64)
        offs = [lay[k] for k in PARTS] + [lay["robot_bytes"]]
        assert offs[0] == 256 and all(o % 256 == 0 for o in offs)
        need = [4 * (K + 1), 24 * P, 4 * P, 96 * K, 48 * lay["partials"], lay["cell_bytes"], lay["cell_bytes"]]
        for a, b, n in zip(offs, offs[1:], need):     # every part has room, and wastes less than one alignment unit
            assert n <= b - a < n + 256
    base = fm.store_bytes(p, _dims())
    for grown in (_dims(B=5), _dims(K=200), _dims(P=4000), _dims(Cc=40960), _dims(S=5120)):
        assert fm.store_bytes(p, grown) > base, grown
    bad = [_dims(B=0), _dims(B=-1), _dims(K=0), _dims(K=-3), _dims(P=0), _dims(P=-1), _dims(Cc=0), _dims(Cc=-5), _dims(S=3), _dims(S=0),
           _dims(S=(1 << 22) + 1), _dims(Cc=0x7FFFFFF1), _dims(P=0x7FFFFFF1), _dims(B=1 << 20, K=1 << 12)]
    for d in bad:
        for f in (fm.store_bytes, fm.layout):
            with pytest.raises(liw.LiwError) as ei:
                f(p, d)
            assert ei.value.code == LIW_EINVAL, d
    for res in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(liw.LiwError) as ei:
            fm.store_bytes(dict(resolution=res), _dims())
        assert ei.value.code == LIW_EINVAL, res
    L = fm._lib()
    n = C.c_size_t(0)
    ps, ds = liw.gridmap.params_struct(p), fm.dims_struct(_dims())
    assert L.liw_fmap_store_bytes(None, C.byref(ds), C.byref(n)) == LIW_EINVAL
    assert L.liw_fmap_store_bytes(C.byref(ps), None, C.byref(n)) == LIW_EINVAL
    assert L.liw_fmap_store_bytes(C.byref(ps), C.byref(ds), None) == LIW_EINVAL
    assert L.liw_fmap_layout(C.byref(ps), C.byref(ds), None) == LIW_EINVAL


def test_info_row_is_liw_map_info(liw):
    assert liw.map_batch.INFO_BYTES == 80   # the held info sits at bytes 32 .. 111 of a robot's header


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
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
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ps, ds = liw.gridmap.params_struct(liw.gridmap.office_map_params()), fm.dims_struct(_dims())
    assert not L.liw_fmap_create(None, C.byref(ds), pd(Til), 1, 0)
    assert not L.liw_fmap_create(C.byref(ps), C.byref(fm.dims_struct(_dims(S=2))), pd(Til), 1, 0)
    assert not L.liw_fmap_create(C.byref(ps), C.byref(ds), None, 1, 0)
    h = C.c_void_p(L.liw_fmap_create(C.byref(ps), C.byref(ds), pd(Til), 1, 0))
    assert h
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes first
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_fmap_reset(h, p, None, None) == E
        assert L.liw_fmap_add_keyframes(h, p, p, p, 4, p, None, p, None) == E
        assert L.liw_fmap_render_tf(h, p, p, 48, None, p, p, None) == E
        assert L.liw_fmap_render(h, p, p, 24, None, p, p, None) == E
        assert L.liw_fmap_num_submaps(h, p, 0) == E
        assert L.liw_fmap_full(h, p, 0) == E
        assert L.liw_fmap_get_submap(h, p, 0, 0, 0, None) == E
        assert L.liw_fmap_get_tf(h, p, 0, 0, None) == E
        assert L.liw_fmap_last_info(h, p, 0, None, None) == E
        assert L.liw_fmap_get(h, p, 0, None, 0) == E
        assert L.liw_fmap_write_pgm(h, p, 0, b"/nonexistent/x", None) == E
        # pure pointer arithmetic: robot 1's grid lies one robot region behind robot 0's
        lay = fm.layout(liw.gridmap.office_map_params(), _dims())
        d0, d1 = L.liw_fmap_device_data(h, p, 0), L.liw_fmap_device_data(h, p, 1)
        assert d0 == buf.ctypes.data + lay["grid_off"] and d1 - d0 == lay["robot_bytes"]
        assert L.liw_fmap_device_data(h, p, 4) is None and L.liw_fmap_device_data(h, p, -1) is None
        assert L.liw_fmap_last_error(h)
    finally:
        L.liw_fmap_destroy(h)


def test_pose_offset_is_the_documented_layout(liw):
    """The robot region of liw_posegraph_batch.h: header 256 B, stamp 8 K, tf12 96 K, then pose 48 K, parts 256-byte aligned."""
    fb = liw.posegraph_batch
    L = fb._lib()
    al = lambda v: (v + 255) & ~255
    for B, K, ML in ((4, 10, 2), (1, 1, 0), (1024, 200, 5)):
        off = C.c_size_t(0)
        d = fb.dims_struct(dict(B=B, max_keyframes=K, max_loops=ML))
        assert L.liw_fpg_pose_offset(C.byref(d), C.byref(off)) == 0
        want = al(al(256 + 8 * K) + 96 * K)
        assert off.value == want and off.value % 8 == 0 and off.value + 48 * K <= fb.layout(dict(B=B, max_keyframes=K, max_loops=ML))["robot_bytes"]
    off = C.c_size_t(7)
    for bad in (dict(B=0, max_keyframes=10, max_loops=2), dict(B=4, max_keyframes=0, max_loops=2), dict(B=4, max_keyframes=10, max_loops=-1)):
        assert L.liw_fpg_pose_offset(C.byref(fb.dims_struct(bad)), C.byref(off)) == LIW_EINVAL and off.value == 7
    assert L.liw_fpg_pose_offset(None, C.byref(off)) == LIW_EINVAL
    assert L.liw_fpg_pose_offset(C.byref(fb.dims_struct(dict(B=4, max_keyframes=10, max_loops=2))), None) == LIW_EINVAL
