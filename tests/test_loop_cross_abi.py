"""C ABI of the cross-robot loop detection (include/liw_loop_cross.h), on any machine: every liw_xloop_* name is exported and listed
in loop_cross.XLOOP_EXPORTS, the header compiles as C99, bad arguments give LIW_EINVAL and write nothing (they are reported before
the missing device), and with good arguments every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_loop_cross.h")
LIW_EINVAL = -22


def test_xloop_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_xloop_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) == 4
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.loop_cross.XLOOP_EXPORTS)) == declared
    assert liw.FleetGroupAligner is liw.loop_cross.FleetGroupAligner


def test_xloop_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_loop_cross.h"\nint f(liw_floop_ctx* c, void* s) { liw_xloop_params p = {8, 0.01}; int i[8];\n'
                   '  return liw_xloop_detect(c, s, s, s, &p, s, s, s, s, s, s, s, 0) + liw_xloop_partner(c, s, s, 0, s, 0)\n'
                   '    + liw_xloop_link(c, s, s, s, s, s, s, s, s, s, 0) + liw_xloop_get_pair(c, s, 0, 0, 0, i, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _ctx(liw, synth):
    fb, lp = liw.loop_batch, liw.loop
    L = liw.loop_cross._lib()
    Tiw = np.ascontiguousarray(np.asarray(synth.office_params()["T_imu_to_wheel"], dtype=np.float64).reshape(16))
    p = lp.office_loop_params()
    d = dict(B=4, max_keyframes=10, max_points=16, max_kf_corners=8)
    h = C.c_void_p(L.liw_floop_create(C.byref(lp.params_struct(p)), C.byref(fb.dims_struct(d)), Tiw.ctypes.data_as(C.POINTER(C.c_double)), 1, 0))
    assert h
    return L, h, p


def test_einval_comes_first_and_writes_nothing(liw, synth):
    """host buffers stand in for device memory: LIW_EINVAL must return before anything is launched or copied"""
    L, h, p = _ctx(liw, synth)
    X = liw.loop_cross.XloopParamsC
    try:
        buf = np.full(512, 0x5A, dtype=np.uint8)
        snap = buf.copy()
        a = C.c_void_p(buf.ctypes.data)
        odd = C.c_void_p(buf.ctypes.data + 4)
        good = X(p["min_match_threshold"], 0.01)
        calls = [L.liw_xloop_detect(None, a, a, a, C.byref(good), None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, None, a, a, C.byref(good), None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, odd, a, a, C.byref(good), None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, a, a, a, None, None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, a, a, a, C.byref(X(p["min_match_threshold"] - 1, 0.01)), None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, a, a, a, C.byref(X(8, -1.0)), None, a, a, a, a, a, a, None),
                 L.liw_xloop_detect(h, a, a, a, C.byref(X(8, float("nan"))), None, a, a, a, a, a, a, None)]
        for i in (2, 3, 6, 7, 8, 9, 10, 11):       # key, partner, found, edge, tf12, T_w1_w2, rms, stats
            args = [h, a, a, a, C.byref(good), None, a, a, a, a, a, a, None]
            args[i] = None
            calls.append(L.liw_xloop_detect(*args))
        calls += [L.liw_xloop_partner(None, a, a, 0, a, None), L.liw_xloop_partner(h, None, a, 0, a, None), L.liw_xloop_partner(h, a, None, 0, a, None),
                  L.liw_xloop_partner(h, a, a, 0, None, None), L.liw_xloop_partner(h, a, a, -1, a, None)]
        calls.append(L.liw_xloop_link(None, *([a] * 9), None))
        for i in range(9):
            args = [a] * 9
            args[i] = None
            calls.append(L.liw_xloop_link(h, *args, None))
        info = np.zeros(8, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int))
        calls += [L.liw_xloop_get_pair(None, a, 0, 0, 0, ip, None, None), L.liw_xloop_get_pair(h, None, 0, 0, 0, ip, None, None),
                  L.liw_xloop_get_pair(h, a, -1, 0, 0, ip, None, None), L.liw_xloop_get_pair(h, a, 4, 0, 0, ip, None, None),
                  L.liw_xloop_get_pair(h, a, 0, 0, 0, None, None, None), L.liw_xloop_get_pair(h, a, 0, 0, -1, ip, None, None)]
        assert calls == [LIW_EINVAL] * len(calls), calls
        assert np.array_equal(buf, snap) and not info.any()
    finally:
        L.liw_floop_destroy(h)


def test_compute_entries_need_a_device(liw, synth):
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L, h, p = _ctx(liw, synth)
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes before any use
        a = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        good = liw.loop_cross.XloopParamsC(p["min_match_threshold"], 0.01)
        assert L.liw_xloop_detect(h, a, a, a, C.byref(good), None, a, a, a, a, a, a, None) == E
        assert L.liw_xloop_partner(h, a, a, 0, a, None) == E
        assert L.liw_xloop_link(h, *([a] * 9), None) == E
        info = np.zeros(8, np.int32)
        assert L.liw_xloop_get_pair(h, a, 0, 0, 0, info.ctypes.data_as(C.POINTER(C.c_int)), None, None) == E
        assert L.liw_floop_last_error(h)
    finally:
        L.liw_floop_destroy(h)
