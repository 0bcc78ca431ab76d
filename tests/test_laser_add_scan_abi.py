"""C ABI of the add_scan that reports what it did (liw_lfe_add_scan_flags, liw_lfe_add_scan_path in include/liw_laser_batch.h):
declared, exported, listed and bound, the LIW_LFE_ADD_* bits of the header equal the Python constants, and without a GPU both
fail with LIW_ENODEV and leave their buffers alone (no CPU fallback).  With a GPU the same test checks the argument errors
instead.  The header's C99 compile and the symbol list as a whole are tests/test_laser_batch_abi.py's."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_laser_batch.h")
NEW = ("liw_lfe_add_scan_flags", "liw_lfe_add_scan_path")
EINVAL = -22


def test_add_scan_entry_points_declared_exported_listed_and_bound(liw):
    text = open(HDR).read()
    declared = set(re.findall(r"\b(liw_lfe_[A-Za-z_0-9]+)\s*\(", text))
    lb = liw.laser_batch
    L = lb._lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in lb.LFE_EXPORTS, name
        assert getattr(L, name).argtypes, name           # the Python layer binds it
    assert len(L.liw_lfe_add_scan_flags.argtypes) == 7 and len(L.liw_lfe_add_scan_path.argtypes) == 1
    for name in ("add_scan", "add_scan_path"):
        assert callable(getattr(lb.BatchFrontEnd, name)), name
    bits = dict(re.findall(r"#define\s+LIW_LFE_ADD_([A-Z]+)\s+(\d+)", text))
    assert {k: int(v) for k, v in bits.items()} == dict(ADDED=lb.ADD_ADDED, FIRST=lb.ADD_FIRST, SPAWNED=lb.ADD_SPAWNED, SWAPPED=lb.ADD_SWAPPED)
    assert (lb.ADD_ADDED, lb.ADD_FIRST, lb.ADD_SPAWNED, lb.ADD_SWAPPED) == (1, 2, 4, 8)


def test_add_scan_entry_points_without_a_device_or_with_bad_arguments(liw):
    import torch
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(dict(B=4, slots=2, max_points=1080, max_lines=128, max_cell_entries=2048))
    assert L.liw_lfe_add_scan_path(None) == EINVAL
    assert L.liw_lfe_add_scan_flags(None, None, 0, None, None, None, None) == EINVAL
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        buf = np.zeros(1 << 16)
        flags = np.full(4, 0x5A, dtype=np.uint8)
        p, f = C.c_void_p(buf.ctypes.data), C.c_void_p(flags.ctypes.data)
        if not torch.cuda.is_available():
            assert L.liw_lfe_add_scan_flags(h, p, 0, p, None, f, None) == liw.LIW_ENODEV
            assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
            assert L.liw_lfe_add_scan_flags(h, p, 0, p, None, None, None) == liw.LIW_ENODEV
            assert L.liw_lfe_add_scan_path(h) == liw.LIW_ENODEV
        else:                                             # host pointers are never touched: every call fails on its arguments
            assert L.liw_lfe_add_scan_flags(h, p, 0, p, None, None, None) == EINVAL      # null flags
            assert L.liw_lfe_add_scan_flags(h, p, 2, p, None, f, None) == EINVAL         # slot out of range
            assert L.liw_lfe_add_scan_flags(h, None, 0, p, None, f, None) == EINVAL      # null store
            assert L.liw_lfe_add_scan_path(h) == EINVAL                                  # no add_scan yet
        assert not buf.any() and (flags == 0x5A).all()
    finally:
        L.liw_lfe_destroy(h)
