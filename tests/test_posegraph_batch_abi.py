"""C ABI of the fleet pose-graph back-end (include/liw_posegraph_batch.h), on any machine: every liw_fpg_* name is exported and
listed in posegraph_batch.FPG_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad dims and null
pointers and add up, and every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_posegraph_batch.h")
LIW_EINVAL = -22


def test_fpg_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_fpg_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 18
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.posegraph_batch.FPG_EXPORTS)) == declared
    assert liw.FleetBackEnd is liw.posegraph_batch.FleetBackEnd


def test_fpg_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_posegraph_batch.h"\nint f(void) { liw_fpg_dims d = {4, 10, 2}; size_t n; liw_fpg_layout_info i;\n'
                   '  return liw_fpg_store_bytes(&d, &n) + liw_fpg_layout(&d, &i); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _dims(B=4, K=10, ML=2):
    return dict(B=B, max_keyframes=K, max_loops=ML)


def test_size_functions_reject_bad_dims_and_add_up(liw):
    fb = liw.posegraph_batch
    for d in (_dims(), _dims(B=1, K=1, ML=0), _dims(B=1024, K=200, ML=5), _dims(B=3, K=150, ML=12)):
        lay = fb.layout(d)
        assert fb.store_bytes(d) == lay["bytes"] == d["B"] * lay["robot_bytes"] + lay["work_bytes"] > 0
        assert lay["work_off"] == d["B"] * lay["robot_bytes"] and lay["robot_bytes"] % 256 == 0 and lay["work_robot_bytes"] % 256 == 0
        assert lay["work_bytes"] >= d["B"] * lay["work_robot_bytes"]
        K, ML = d["max_keyframes"], d["max_loops"]
        assert lay["max_separators"] == min(K, -(-K // 48) + 1 + 2 * ML) and lay["edge_slots"] == K - 1 + ML
        # header, then stamp, tf12, pose, sequential edge per key frame and index, tf12 per loop
        assert lay["robot_bytes"] >= 256 + K * (8 + 96 + 48 + 96) + ML * (8 + 96)
    assert fb.store_bytes(_dims(K=11)) > fb.store_bytes(_dims(K=10)) and fb.store_bytes(_dims(ML=40)) > fb.store_bytes(_dims(ML=2))
    for d in (_dims(B=0), _dims(B=-1), _dims(K=0), _dims(K=-2), _dims(ML=-1), _dims(B=1 << 20, K=4096, ML=0), _dims(B=1, K=2, ML=1 << 30)):
        for f in (fb.store_bytes, fb.layout):
            with pytest.raises(liw.LiwError) as ei:
                f(d)
            assert ei.value.code == LIW_EINVAL, d
    L = fb._lib()
    n = C.c_size_t(0)
    assert L.liw_fpg_store_bytes(None, C.byref(n)) == LIW_EINVAL
    assert L.liw_fpg_store_bytes(C.byref(fb.dims_struct(_dims())), None) == LIW_EINVAL
    assert L.liw_fpg_layout(None, C.byref(fb.FpgLayoutC())) == LIW_EINVAL
    assert L.liw_fpg_layout(C.byref(fb.dims_struct(_dims())), None) == LIW_EINVAL


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
    fb = liw.posegraph_batch
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L = fb._lib()
    ps, pgs, dd = liw.params_struct(synth.office_params(), 0), liw.posegraph.pg_struct(liw.posegraph.office_pg_params()), fb.dims_struct(_dims())
    assert not L.liw_fpg_create(None, C.byref(pgs), C.byref(dd), 10.0, 0)
    assert not L.liw_fpg_create(C.byref(ps), None, C.byref(dd), 10.0, 0)
    assert not L.liw_fpg_create(C.byref(ps), C.byref(pgs), None, 10.0, 0)
    assert not L.liw_fpg_create(C.byref(ps), C.byref(pgs), C.byref(fb.dims_struct(_dims(K=0))), 10.0, 0)
    assert not L.liw_fpg_create(C.byref(ps), C.byref(pgs), C.byref(dd), float("nan"), 0)
    h = C.c_void_p(L.liw_fpg_create(C.byref(ps), C.byref(pgs), C.byref(dd), 10.0, 0))
    assert h
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes first
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_fpg_reset(h, p, None, None) == E
        assert L.liw_fpg_add_keyframes(h, p, p, p, p, None, p, None) == E
        assert L.liw_fpg_add_loops(h, p, p, p, p, None, None) == E
        assert L.liw_fpg_due(h, p, p, p, None, p, p, None) == E
        assert L.liw_fpg_solve(h, p, p, p, 5, 0, p, None) == E
        assert L.liw_fpg_correct(h, p, p, p, None, None) == E
        assert L.liw_fpg_num_keyframes(h, p, 0) == E
        assert L.liw_fpg_flags(h, p, 0, None, None) == E
        assert L.liw_fpg_get_keyframes(h, p, 0, 0, None, None, None) == E
        assert L.liw_fpg_get_seq_edges(h, p, 0, 0, None) == E
        assert L.liw_fpg_get_loop_edges(h, p, 0, 0, None, None) == E
        assert L.liw_fpg_get_modify_delta_tf(h, p, 0, None) == E
        assert L.liw_fpg_get_summary(h, p, 0, None) == E
        assert L.liw_fpg_load_graph(h, p, 0, 1, None, None, None, 0, None, None) == E
        assert L.liw_fpg_set_lds_doubles(h, 0) == 0 and L.liw_fpg_set_lds_doubles(h, 8192) == 0          # host-only
        assert L.liw_fpg_set_lds_doubles(h, -1) == LIW_EINVAL and L.liw_fpg_set_lds_doubles(h, 8193) == LIW_EINVAL
        assert L.liw_fpg_set_lds_doubles(None, 0) == LIW_EINVAL
        assert L.liw_fpg_last_error(h)
    finally:
        L.liw_fpg_destroy(h)
