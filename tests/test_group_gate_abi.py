"""C ABI of the group edge gate (include/liw_group_gate.h), on any machine: every liw_ggate_* name is exported and listed in
group_gate.EXPORTS, the header compiles as C99, bad arguments give LIW_EINVAL before the missing device and write nothing, the
compute entry fails with LIW_ENODEV without a GPU (no CPU fallback), and include/liw_group_graph.h still declares its 14 symbols."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_group_gate.h")
LIW_EINVAL = -22
DIMS = dict(B=10, G=4, max_members=4, max_edges=8)


@pytest.fixture(scope="module")
def gg(liw):
    return importlib.import_module(liw.__name__ + ".group_graph")


@pytest.fixture(scope="module")
def gate(liw):
    return importlib.import_module(liw.__name__ + ".group_gate")


def test_header_symbols_are_exported(liw, gg, gate):
    declared = sorted(set(re.findall(r"\b(liw_ggate_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert declared == ["liw_ggate_gate", "liw_ggate_get"]
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(gate.EXPORTS)) == declared
    build = importlib.import_module(liw.__name__ + ".build")
    assert any(h.endswith("liw_group_gate.h") for h in build.HEADERS)                     # part of the source hash
    # the group graph's own header is as it was
    graph = open(os.path.join(ROOT, "include", "liw_group_graph.h")).read()
    assert len(set(re.findall(r"\b(liw_ggraph_[A-Za-z_0-9]+)\s*\(", graph))) == 14 and "liw_ggate_" not in graph
    assert len(gg.EXPORTS) == 14


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_group_gate.h"\nint f(liw_ggraph_ctx* c, void* s, unsigned char* m) { int i[2]; double d[1];\n'
                   '  return liw_ggate_gate(c, s, m, 12.0, 2, m, 0) + liw_ggate_get(c, s, 0, 1, i, d, i); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _ctx(gg, gate):
    L = gate._lib()
    pg = dict(loop_sigma_p=[0.05, 0.05, 0.05], loop_sigma_q=[0.02, 0.02, 0.02], loop_edge_k=1.0, use_ground_p_factor=True, use_ground_q_factor=True)
    h = C.c_void_p(L.liw_ggraph_create(C.byref(gg.pg_struct(pg)), C.byref(gg.dims_struct(DIMS)), 0))
    assert h
    return L, h


def test_einval_comes_first_and_writes_nothing(gg, gate):
    """host buffers stand in for device memory: LIW_EINVAL must return before anything is launched or copied"""
    L, h = _ctx(gg, gate)
    try:
        buf = np.full(512, 0x5A, dtype=np.uint8)
        snap = buf.copy()
        a, odd = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 4)
        d, i = C.c_double, C.c_int
        calls = [L.liw_ggate_gate(None, a, a, d(12.0), i(2), a, None), L.liw_ggate_gate(h, None, a, d(12.0), i(2), a, None),
                 L.liw_ggate_gate(h, a, None, d(12.0), i(2), a, None), L.liw_ggate_gate(h, a, a, d(12.0), i(2), None, None),
                 L.liw_ggate_gate(h, odd, a, d(12.0), i(2), a, None)]
        calls += [L.liw_ggate_gate(h, a, a, d(v), i(2), a, None) for v in (0.0, -1.0, float("inf"), float("-inf"), float("nan"))]
        calls += [L.liw_ggate_gate(h, a, a, d(12.0), i(v), a, None) for v in (0, -3)]
        st = np.zeros(8, np.int32)
        sp = st.ctypes.data_as(C.POINTER(C.c_int))
        calls += [L.liw_ggate_get(None, a, 0, 0, None, None, None), L.liw_ggate_get(h, None, 0, 0, None, None, None),
                  L.liw_ggate_get(h, odd, 0, 0, None, None, None), L.liw_ggate_get(h, a, -1, 0, None, None, None),
                  L.liw_ggate_get(h, a, DIMS["G"], 0, None, None, None), L.liw_ggate_get(h, a, 0, -1, sp, None, sp)]
        assert calls == [LIW_EINVAL] * len(calls), calls
        assert np.array_equal(buf, snap) and not st.any()
        assert L.liw_ggraph_last_error(h)
    finally:
        L.liw_ggraph_destroy(h)


def test_compute_entries_need_a_device(liw, gg, gate):
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L, h = _ctx(gg, gate)
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes before any use
        a = C.c_void_p(buf.ctypes.data)
        assert L.liw_ggate_gate(h, a, a, C.c_double(12.0), C.c_int(2), a, None) == liw.LIW_ENODEV
        assert L.liw_ggate_get(h, a, 0, 0, None, None, None) == liw.LIW_ENODEV
        assert not buf.any()
    finally:
        L.liw_ggraph_destroy(h)
