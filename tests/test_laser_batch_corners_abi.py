"""The corner entry points of the batched laser front-end (include/liw_laser_batch.h): liw_lfe_spawn_corners and
liw_lfe_corners_to_world are exported, listed in laser_batch.LFE_EXPORTS and wrapped by BatchFrontEnd, and without a GPU they
fail with LIW_ENODEV like every compute entry (no CPU fallback)."""
import ctypes as C
import inspect

import numpy as np
import pytest

NEW = ("liw_lfe_spawn_corners", "liw_lfe_corners_to_world")


def test_corner_entry_points_are_exported(liw):
    L = liw.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in liw.laser_batch.LFE_EXPORTS, name
    assert liw.laser_batch.ST_CORNERS == 32
    fe = liw.laser_batch.BatchFrontEnd
    assert "corners" in inspect.signature(fe.spawn).parameters
    assert callable(getattr(fe, "corners_to_world"))


def test_corner_entry_points_have_no_cpu_fallback(liw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(dict(B=4, slots=2, max_points=1080, max_lines=128, max_cell_entries=2048))
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        buf = np.zeros(1 << 16)
        p = C.c_void_p(buf.ctypes.data)
        assert L.liw_lfe_spawn_corners(h, p, 0, p, p, p, 16, p, p, None) == liw.LIW_ENODEV
        assert L.liw_lfe_corners_to_world(h, p, 16, p, p, p, None, None, 64, p, p, None) == liw.LIW_ENODEV
        assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
    finally:
        L.liw_lfe_destroy(h)
