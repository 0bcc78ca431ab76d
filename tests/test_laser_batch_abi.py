"""C ABI of the batched laser front-end (include/liw_laser_batch.h): every liw_lfe_* name is exported and listed in
laser_batch.LFE_EXPORTS, the header compiles as C, the store layout is a host-only query, and without a GPU every compute entry
fails with LIW_ENODEV (no CPU fallback)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_laser_batch.h")


def test_lfe_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_lfe_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert declared
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.laser_batch.LFE_EXPORTS)) == declared


def test_lfe_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_laser_batch.h"\nint f(void) { liw_lfe_dims d = {1, 1, 1, 1, 1}; size_t n; return liw_lfe_store_layout(&d, &n); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _dims(**kw):
    d = dict(B=4, slots=2, max_points=1080, max_lines=128, max_cell_entries=2048)
    d.update(kw)
    return d


def test_store_layout_monotone_and_rejects_bad_dims(liw):
    lb = liw.laser_batch
    base = lb.store_bytes(_dims())
    assert base > 0
    for k in ("B", "slots", "max_lines", "max_cell_entries"):
        big = lb.store_bytes(_dims(**{k: 2 * _dims()[k]}))
        assert big > base, k
    assert lb.store_bytes(_dims(max_points=4096)) >= base        # points live in the caller's arrays, not the store
    assert lb.store_bytes(_dims(B=8)) == 2 * base                 # robot-major, one region per robot
    for k in ("B", "slots", "max_points", "max_lines", "max_cell_entries"):
        for v in (0, -1):
            with pytest.raises(liw.LiwError) as e:
                lb.store_bytes(_dims(**{k: v}))
            assert e.value.code == -22
    L = lb._lib()
    n = C.c_size_t(0)
    assert L.liw_lfe_store_layout(None, C.byref(n)) == -22
    assert L.liw_lfe_store_layout(C.byref(lb.dims_struct(_dims())), None) == -22


def test_no_cpu_fallback(liw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(_dims())
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        ENODEV = liw.LIW_ENODEV
        buf = np.zeros(1 << 16)
        p = C.c_void_p(buf.ctypes.data)
        assert L.liw_lfe_set_geometry(h, 1080, -2.0, 0.004, 1e-5) == ENODEV
        assert L.liw_lfe_store_reset(h, p, None, None) == ENODEV
        assert L.liw_lfe_ranges_to_points(h, p, p, p, p, p, p, None) == ENODEV
        assert L.liw_lfe_deskew(h, p, p, p, p, p, p, None) == ENODEV
        assert L.liw_lfe_spawn(h, p, 0, p, p, p, None) == ENODEV
        assert L.liw_lfe_match(h, p, -1, 0, None, p, 0, 8, p, p, p, p, p, None) == ENODEV
        assert L.liw_lfe_add_scan(h, p, 0, p, None, None) == ENODEV
        assert L.liw_lfe_pack_track(h, 2, 1, 8, p, p, p, 8, p, p, p, p, p, None) == ENODEV
        for fn in (L.liw_lfe_status, L.liw_lfe_num_lines):
            assert fn(h, p, 0, 0) == ENODEV
        assert L.liw_lfe_get_lines(h, p, 0, 0, buf.ctypes.data_as(C.POINTER(C.c_double)), 1) == ENODEV
        assert L.liw_lfe_cell_lines(h, p, 0, 0, 0.0, 0.0, None, 0) == ENODEV
        assert L.liw_lfe_submap_pose(h, p, 0, -1, None, None) == ENODEV
        assert L.liw_lfe_crmath_eval(h, 0, 8, p, None, p, None) == ENODEV
        assert L.liw_lfe_crmath_eval(None, 0, 8, p, None, p, None) == -22
        assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
    finally:
        L.liw_lfe_destroy(h)
