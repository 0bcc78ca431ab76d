"""C ABI of the fleet initialisation on the device (liw_lfe_match_front, liw_lfe_pack_init, liw_lfe_rebuild in
include/liw_laser_batch.h): declared, exported and listed, and without a GPU every one of them fails with LIW_ENODEV (no CPU
fallback).  The header's C99 compile and the symbol list as a whole are tests/test_laser_batch_abi.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_laser_batch.h")
NEW = ("liw_lfe_match_front", "liw_lfe_pack_init", "liw_lfe_rebuild")


def test_init_entry_points_declared_exported_and_listed(liw):
    declared = set(re.findall(r"\b(liw_lfe_[A-Za-z_0-9]+)\s*\(", open(HDR).read()))
    L = liw.laser_batch._lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in liw.laser_batch.LFE_EXPORTS, name
        assert getattr(L, name).argtypes, name           # the Python layer binds it
    for name in ("match_front", "pack_init", "rebuild"):
        assert callable(getattr(liw.laser_batch.BatchFrontEnd, name)), name


def test_init_entry_points_have_no_cpu_fallback(liw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(dict(B=4, slots=6, max_points=1080, max_lines=128, max_cell_entries=2048))
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        buf = np.zeros(1 << 16)
        p = C.c_void_p(buf.ctypes.data)
        assert L.liw_lfe_match_front(h, p, 0, 1, 5, p, p, 30, 6, 0, 8, p, p, p, p, p, None) == liw.LIW_ENODEV
        assert L.liw_lfe_pack_init(h, 6, 8, p, p, p, p, 8, p, p, p, p, p, p, None) == liw.LIW_ENODEV
        assert L.liw_lfe_rebuild(h, p, 0, 6, p, 36, 6, None, None) == liw.LIW_ENODEV
        assert not buf.any()
        assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
    finally:
        L.liw_lfe_destroy(h)
