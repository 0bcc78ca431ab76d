"""C ABI of the group pose graph (include/liw_group_graph.h), on any machine: every liw_ggraph_* name is exported and listed in
group_graph.EXPORTS, the header compiles as C99, liw_ggraph_store_bytes / liw_ggraph_layout are consistent with 256-byte parts, bad
arguments give LIW_EINVAL and write nothing (they are reported before the missing device), and with good arguments every compute
entry fails with LIW_ENODEV without a GPU (no CPU fallback)."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_group_graph.h")
LIW_EINVAL = -22
DIMS = dict(B=12, G=3, max_members=6, max_edges=8)


@pytest.fixture(scope="module")
def gg(liw):
    return importlib.import_module(liw.__name__ + ".group_graph")


def test_header_symbols_are_exported(liw, gg):
    declared = sorted(set(re.findall(r"\b(liw_ggraph_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) == 14
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(gg.EXPORTS)) == declared
    assert "liw_group_graph.cpp" in importlib.import_module(liw.__name__ + ".build").SOURCES


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_group_graph.h"\nint f(liw_ggraph_ctx* c, void* s, liw_summary* sm) { liw_ggraph_dims d = {12, 3, 6, 8}; size_t n; int i[8];\n'
                   '  return liw_ggraph_store_bytes(&d, &n) + liw_ggraph_reset(c, s, 0, 0) + liw_ggraph_add_edges(c, s, s, s, s, s, 0, 0)\n'
                   '    + liw_ggraph_partner(c, s, s, 0, s, 0) + liw_ggraph_solve(c, s, s, 6, s, s, s, s, s, s, 0, sm, 0)\n'
                   '    + liw_ggraph_get_edges(c, s, 0, 0, i, 0) + liw_ggraph_get_flags(c, s, 0, i) + liw_ggraph_get_summary(c, s, 0, sm)\n'
                   '    + liw_ggraph_get_Z(c, s, 0, 0, i, 0, 0, 0) + liw_ggraph_set_lds_doubles(c, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_layout_is_consistent(gg):
    for d in (DIMS, dict(B=1, G=1, max_members=1, max_edges=1), dict(B=4096, G=1024, max_members=16, max_edges=40),
              dict(B=64, G=2, max_members=22, max_edges=64)):
        lay = gg.layout(d)
        M, E, G = d["max_members"], d["max_edges"], d["G"]
        assert gg.store_bytes(d) == lay["bytes"] == G * lay["group_bytes"] + lay["work_bytes"]
        assert lay["work_off"] == G * lay["group_bytes"] and lay["work_bytes"] == G * lay["work_group_bytes"]
        assert all(lay[k] % 256 == 0 for k in ("bytes", "group_bytes", "work_off", "work_bytes", "work_group_bytes"))
        assert lay["group_bytes"] >= 256 + 128 * E and lay["group_bytes"] - (256 + 128 * E) < 256
        assert lay["tri_doubles"] == 3 * M * (6 * M + 1)
        # the parts the header lists: state, x / candidate / step / scale / diagonal / gradient, blocks, edge blocks, Z, triangle, rhs
        need = 256 + 6 * 48 * M + 288 * M + 624 * E + 288 * E + 8 * lay["tri_doubles"] + 48 * M + 8 * M + 12 * E
        assert need <= lay["work_group_bytes"] <= need + 14 * 256
    assert gg.layout(dict(B=8, G=1, max_members=21, max_edges=8))["tri_doubles"] <= 8192 < gg.layout(dict(B=8, G=1, max_members=22, max_edges=8))["tri_doubles"]
    L = gg._lib()
    n, out = C.c_size_t(7), gg.GgraphLayoutC()
    for bad in (dict(DIMS, B=0), dict(DIMS, G=0), dict(DIMS, max_members=0), dict(DIMS, max_edges=0), dict(DIMS, B=-3), dict(DIMS, max_members=1025),
                dict(DIMS, max_edges=65537)):
        assert L.liw_ggraph_store_bytes(C.byref(gg.dims_struct(bad)), C.byref(n)) == LIW_EINVAL and n.value == 7
        assert L.liw_ggraph_layout(C.byref(gg.dims_struct(bad)), C.byref(out)) == LIW_EINVAL and out.bytes == 0
        assert not L.liw_ggraph_create(C.byref(gg.pg_struct(_pg())), C.byref(gg.dims_struct(bad)), 0)
    good = gg.dims_struct(DIMS)
    assert L.liw_ggraph_store_bytes(None, C.byref(n)) == LIW_EINVAL and L.liw_ggraph_store_bytes(C.byref(good), None) == LIW_EINVAL
    assert L.liw_ggraph_layout(C.byref(good), None) == LIW_EINVAL and L.liw_ggraph_layout(None, C.byref(out)) == LIW_EINVAL
    assert not L.liw_ggraph_create(None, C.byref(good), 0) and not L.liw_ggraph_create(C.byref(gg.pg_struct(_pg())), None, 0)


def _pg():
    return dict(loop_sigma_p=[0.05, 0.05, 0.05], loop_sigma_q=[0.02, 0.02, 0.02], loop_edge_k=1.0, use_ground_p_factor=True, use_ground_q_factor=True)


def _ctx(gg):
    L = gg._lib()
    h = C.c_void_p(L.liw_ggraph_create(C.byref(gg.pg_struct(_pg())), C.byref(gg.dims_struct(DIMS)), 0))
    assert h
    return L, h


def _solve_args(h, a):
    return [h, a, a, 6, a, a, a, a, a, a, 0, a, None]


def test_einval_comes_first_and_writes_nothing(liw, gg):
    """host buffers stand in for device memory: LIW_EINVAL must return before anything is launched or copied"""
    L, h = _ctx(gg)
    try:
        buf = np.full(512, 0x5A, dtype=np.uint8)
        snap = buf.copy()
        a, odd = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 4)
        calls = [L.liw_ggraph_reset(None, a, None, None), L.liw_ggraph_reset(h, None, None, None), L.liw_ggraph_reset(h, odd, None, None)]
        calls += [L.liw_ggraph_add_edges(None, a, a, a, a, a, None, None), L.liw_ggraph_add_edges(h, odd, a, a, a, a, None, None)]
        for i in (1, 2, 3, 4, 5):          # store, group_of, found, edge, tf12
            args = [h, a, a, a, a, a, None, None]
            args[i] = None
            calls.append(L.liw_ggraph_add_edges(*args))
        calls += [L.liw_ggraph_partner(None, a, a, 0, a, None), L.liw_ggraph_partner(h, None, a, 0, a, None), L.liw_ggraph_partner(h, a, None, 0, a, None),
                  L.liw_ggraph_partner(h, a, a, 0, None, None), L.liw_ggraph_partner(h, a, a, -1, a, None)]
        for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 11):   # ctx, store, poses, n_keyframes, group_of, linked, fixed, T_g_w, gsel, summary
            args = _solve_args(h, a)
            args[i] = None
            calls.append(L.liw_ggraph_solve(*args))
        args = _solve_args(h, a)
        args[1] = odd
        calls.append(L.liw_ggraph_solve(*args))
        args = _solve_args(h, a)
        args[3] = -1
        calls.append(L.liw_ggraph_solve(*args))
        info = np.zeros(8, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int))
        sm = liw.SummaryC()
        calls += [L.liw_ggraph_get_edges(None, a, 0, 0, None, None), L.liw_ggraph_get_edges(h, None, 0, 0, None, None), L.liw_ggraph_get_edges(h, odd, 0, 0, None, None),
                  L.liw_ggraph_get_edges(h, a, -1, 0, None, None), L.liw_ggraph_get_edges(h, a, 3, 0, None, None), L.liw_ggraph_get_edges(h, a, 0, -1, None, None),
                  L.liw_ggraph_get_flags(None, a, 0, ip), L.liw_ggraph_get_flags(h, None, 0, ip), L.liw_ggraph_get_flags(h, a, 3, ip),
                  L.liw_ggraph_get_flags(h, a, 0, None), L.liw_ggraph_get_summary(None, a, 0, C.byref(sm)), L.liw_ggraph_get_summary(h, a, 0, None),
                  L.liw_ggraph_get_summary(h, a, -1, C.byref(sm)), L.liw_ggraph_get_Z(None, a, 0, 0, None, None, None, None),
                  L.liw_ggraph_get_Z(h, None, 0, 0, None, None, None, None), L.liw_ggraph_get_Z(h, a, 3, 0, None, None, None, None),
                  L.liw_ggraph_get_Z(h, a, 0, -1, None, None, None, None),
                  L.liw_ggraph_set_lds_doubles(None, 0), L.liw_ggraph_set_lds_doubles(h, -1), L.liw_ggraph_set_lds_doubles(h, 8193)]
        assert calls == [LIW_EINVAL] * len(calls), calls
        assert np.array_equal(buf, snap) and not info.any()
        assert L.liw_ggraph_set_lds_doubles(h, 0) == 0 and L.liw_ggraph_set_lds_doubles(h, 8192) == 0
        assert L.liw_ggraph_last_error(None) == b"null ctx"
    finally:
        L.liw_ggraph_destroy(h)


def test_compute_entries_need_a_device(liw, gg):
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L, h = _ctx(gg)
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes before any use
        a = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_ggraph_reset(h, a, None, None) == E
        assert L.liw_ggraph_add_edges(h, a, a, a, a, a, None, None) == E
        assert L.liw_ggraph_partner(h, a, a, 0, a, None) == E
        assert L.liw_ggraph_solve(*_solve_args(h, a)) == E
        info = np.zeros(8, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int))
        assert L.liw_ggraph_get_edges(h, a, 0, 0, None, None) == E and L.liw_ggraph_get_flags(h, a, 0, ip) == E
        assert L.liw_ggraph_get_summary(h, a, 0, C.byref(liw.SummaryC())) == E and L.liw_ggraph_get_Z(h, a, 0, 0, None, None, None, None) == E
        assert L.liw_ggraph_last_error(h)
    finally:
        L.liw_ggraph_destroy(h)
