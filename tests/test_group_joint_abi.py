"""C ABI of the joint pose graph of a group (include/liw_group_joint.h), on any machine: every liw_gjoint_* name is exported and listed
in group_joint.EXPORTS, the header compiles as C99, the layout arithmetic holds with 256-byte parts, bad arguments give LIW_EINVAL and
write nothing (they are reported before the missing device), and with good arguments every compute entry fails with LIW_ENODEV
without a GPU (no CPU fallback)."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_group_joint.h")
LIW_EINVAL = -22
DIMS = dict(B=13, G=5, max_keyframes=64, max_robot_loops=2, max_edges=12, max_members=4, max_nodes=66, max_loops=12)


@pytest.fixture(scope="module")
def gj(liw):
    return importlib.import_module(liw.__name__ + ".group_joint")


def test_header_symbols_are_exported(liw, gj):
    declared = sorted(set(re.findall(r"\b(liw_gjoint_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) == 13
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(gj.EXPORTS)) == declared
    build = importlib.import_module(liw.__name__ + ".build")
    assert "liw_group_joint.cpp" in build.SOURCES and "k_group_joint.hip" in build.SOURCES and "k_group_joint.hpp" in build.HEADERS


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_group_joint.h"\nint f(liw_gjoint_ctx* c, void* s, liw_summary* sm) { liw_gjoint_dims d = {13, 5, 64, 2, 12, 4, 66, 12}; size_t n; int i[16];\n'
                   '  liw_gjoint_layout_info li;\n'
                   '  return liw_gjoint_store_bytes(&d, &n) + liw_gjoint_layout(&d, &li) + liw_gjoint_pose_offset(&d, &n)\n'
                   '    + liw_gjoint_solve(c, s, s, s, s, s, s, s, s, 0, 0, sm, 0) + liw_gjoint_get_header(c, s, 0, i) + liw_gjoint_get_summary(c, s, 0, sm)\n'
                   '    + liw_gjoint_get_members(c, s, 0, 0, i, i) + liw_gjoint_get_nodes(c, s, 0, 0, i, i) + liw_gjoint_get_separators(c, s, 0, 0, i)\n'
                   '    + liw_gjoint_set_lds_doubles(c, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_layout_is_consistent(liw, gj):
    for d in (DIMS, dict(B=1, G=1, max_keyframes=1, max_robot_loops=0, max_edges=1, max_members=1, max_nodes=1, max_loops=1),
              dict(B=4096, G=1024, max_keyframes=200, max_robot_loops=2, max_edges=12, max_members=4, max_nodes=800, max_loops=20),
              dict(B=8, G=2, max_keyframes=50, max_robot_loops=5, max_edges=40, max_members=2, max_nodes=100, max_loops=6)):
        lay = gj.layout(d)
        B, G, K, M, N, ML = d["B"], d["G"], d["max_keyframes"], d["max_members"], d["max_nodes"], d["max_loops"]
        S = min(N, N // 48 + 2 * M + 2 * ML)
        assert lay["max_separators"] == S and lay["tri_doubles"] == 3 * S * (6 * S + 1)
        assert lay["pose_off"] == 0 and lay["header_off"] >= 48 * B * K and lay["header_off"] - 48 * B * K < 256
        assert lay["work_off"] >= lay["header_off"] + 256 * G + 4 * B and lay["work_off"] - (lay["header_off"] + 256 * G + 4 * B) < 256
        assert gj.store_bytes(d) == lay["bytes"] == lay["work_off"] + G * lay["work_group_bytes"] + 256
        assert all(lay[k] % 256 == 0 for k in ("bytes", "header_off", "work_off", "work_group_bytes"))
        # the parts: state, lists, loops, x / candidate / step / scale / diagonal / gradient, edge and ground blocks, node and loop blocks,
        # separator lists, Schur terms, records, triangle, right-hand side
        need = (256 + 4 * M + 4 * (M + 1) + 3 * 4 * N + 8 * ML + 96 * ML + 6 * 48 * N + 624 * (N + ML) + 112 * N + 2 * 288 * N + 288 * ML + 4 * S + 960 * S
                + 624 * N + 8 * lay["tri_doubles"] + 48 * S)
        assert need <= lay["work_group_bytes"] <= need + 23 * 256
        off = C.c_size_t(7)
        assert gj._lib().liw_gjoint_pose_offset(C.byref(gj.dims_struct(d)), C.byref(off)) == 0 and off.value == lay["pose_off"]
    L = gj._lib()
    n, out = C.c_size_t(7), gj.GjointLayoutC()
    pgs, prm = liw.posegraph.pg_struct(liw.posegraph.office_pg_params()), _prm(liw)
    bads = [dict(DIMS, **{k: 0}) for k in DIMS if k != "max_robot_loops"] + [dict(DIMS, max_robot_loops=-1), dict(DIMS, B=-3), dict(DIMS, max_members=1025),
                                                                         dict(DIMS, G=1 << 20, max_nodes=1 << 12), dict(DIMS, B=1 << 20, max_keyframes=1 << 12)]
    for bad in bads:
        assert L.liw_gjoint_store_bytes(C.byref(gj.dims_struct(bad)), C.byref(n)) == LIW_EINVAL and n.value == 7, bad
        assert L.liw_gjoint_layout(C.byref(gj.dims_struct(bad)), C.byref(out)) == LIW_EINVAL and out.bytes == 0
        assert L.liw_gjoint_pose_offset(C.byref(gj.dims_struct(bad)), C.byref(n)) == LIW_EINVAL and n.value == 7
        assert not L.liw_gjoint_create(C.byref(prm), C.byref(pgs), C.byref(gj.dims_struct(bad)), 0)
    good = gj.dims_struct(DIMS)
    assert L.liw_gjoint_store_bytes(None, C.byref(n)) == LIW_EINVAL and L.liw_gjoint_store_bytes(C.byref(good), None) == LIW_EINVAL
    assert L.liw_gjoint_layout(C.byref(good), None) == LIW_EINVAL and L.liw_gjoint_layout(None, C.byref(out)) == LIW_EINVAL
    assert L.liw_gjoint_pose_offset(C.byref(good), None) == LIW_EINVAL and L.liw_gjoint_pose_offset(None, C.byref(n)) == LIW_EINVAL
    assert not L.liw_gjoint_create(None, C.byref(pgs), C.byref(good), 0) and not L.liw_gjoint_create(C.byref(prm), None, C.byref(good), 0)
    assert not L.liw_gjoint_create(C.byref(prm), C.byref(pgs), None, 0)


def _prm(liw):
    synth = importlib.import_module(liw.__name__ + ".synth")
    return liw.params_struct(synth.office_params(), 0)


def _ctx(liw, gj):
    L = gj._lib()
    pgs, prm = liw.posegraph.pg_struct(liw.posegraph.office_pg_params()), _prm(liw)
    h = C.c_void_p(L.liw_gjoint_create(C.byref(prm), C.byref(pgs), C.byref(gj.dims_struct(DIMS)), 0))
    assert h
    return L, h


def _solve_args(h, a):
    return [h, a, a, a, a, a, a, a, a, 0, 0, a, None]


def test_einval_comes_first_and_writes_nothing(liw, gj):
    """host buffers stand in for device memory: LIW_EINVAL must return before anything is launched or copied"""
    L, h = _ctx(liw, gj)
    try:
        buf = np.full(512, 0x5A, dtype=np.uint8)
        snap = buf.copy()
        a, odd = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 4)
        calls = []
        for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11):   # ctx, store, fpg_store, ggraph_store, group_of, linked, fixed, T_g_w, gsel, summary
            args = _solve_args(h, a)
            args[i] = None
            calls.append(L.liw_gjoint_solve(*args))
        for i in (1, 2, 3):                          # a misaligned store of any of the three
            args = _solve_args(h, a)
            args[i] = odd
            calls.append(L.liw_gjoint_solve(*args))
        info = np.zeros(16, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int))
        sm = liw.SummaryC()
        calls += [L.liw_gjoint_get_header(None, a, 0, ip), L.liw_gjoint_get_header(h, None, 0, ip), L.liw_gjoint_get_header(h, odd, 0, ip),
                  L.liw_gjoint_get_header(h, a, 5, ip), L.liw_gjoint_get_header(h, a, -1, ip), L.liw_gjoint_get_header(h, a, 0, None),
                  L.liw_gjoint_get_summary(None, a, 0, C.byref(sm)), L.liw_gjoint_get_summary(h, a, 0, None), L.liw_gjoint_get_summary(h, a, -1, C.byref(sm)),
                  L.liw_gjoint_get_members(None, a, 0, 0, None, None), L.liw_gjoint_get_members(h, None, 0, 0, None, None),
                  L.liw_gjoint_get_members(h, a, 5, 0, None, None), L.liw_gjoint_get_members(h, a, 0, -1, None, None),
                  L.liw_gjoint_get_nodes(None, a, 0, 0, None, None), L.liw_gjoint_get_nodes(h, odd, 0, 0, None, None), L.liw_gjoint_get_nodes(h, a, 5, 0, None, None),
                  L.liw_gjoint_get_nodes(h, a, 0, -1, None, None), L.liw_gjoint_get_separators(None, a, 0, 0, None), L.liw_gjoint_get_separators(h, None, 0, 0, None),
                  L.liw_gjoint_get_separators(h, a, -1, 0, None), L.liw_gjoint_get_separators(h, a, 0, -1, None),
                  L.liw_gjoint_set_lds_doubles(None, 0), L.liw_gjoint_set_lds_doubles(h, -1), L.liw_gjoint_set_lds_doubles(h, 8193)]
        assert calls == [LIW_EINVAL] * len(calls), calls
        assert np.array_equal(buf, snap) and not info.any()
        assert L.liw_gjoint_set_lds_doubles(h, 0) == 0 and L.liw_gjoint_set_lds_doubles(h, 8192) == 0
        assert L.liw_gjoint_last_error(None) == b"null ctx"
    finally:
        L.liw_gjoint_destroy(h)


def test_compute_entries_need_a_device(liw, gj):
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L, h = _ctx(liw, gj)
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes before any use
        a = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_gjoint_solve(*_solve_args(h, a)) == E
        info = np.zeros(16, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int))
        assert L.liw_gjoint_get_header(h, a, 0, ip) == E and L.liw_gjoint_get_summary(h, a, 0, C.byref(liw.SummaryC())) == E
        assert L.liw_gjoint_get_members(h, a, 0, 0, None, None) == E and L.liw_gjoint_get_nodes(h, a, 0, 0, None, None) == E
        assert L.liw_gjoint_get_separators(h, a, 0, 0, None) == E
        assert L.liw_gjoint_last_error(h)
    finally:
        L.liw_gjoint_destroy(h)
