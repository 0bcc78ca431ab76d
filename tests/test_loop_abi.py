"""C ABI of the loop detector (include/liw_loop.h), on any machine: every liw_loop_* name is exported and listed in
loop.LOOP_EXPORTS, the header compiles as C99, the store size is a host-only query that grows with the dims and rejects bad
ones, every compute entry fails with LIW_ENODEV without a GPU (no CPU fallback), and the closed-form planar ICP is the
optimum a Levenberg-Marquardt over point_factor converges to."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loop_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_loop.h")


def test_loop_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_loop_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert declared
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.loop.LOOP_EXPORTS)) == declared


def test_loop_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_loop.h"\nint f(void) { liw_loop_params p = {0.03, 0.03, 30, 5, 100, 1.0, 1.0, 0.5, 0ull};\n'
                   '  liw_loop_dims d = {10, 10}; size_t n; liw_loop_edge e; (void)e; return liw_loop_store_bytes(&p, &d, &n); }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_store_bytes_monotone_and_rejects_bad_dims(liw):
    lp = liw.loop
    p = lp.office_loop_params()
    last = 0
    for K, P in [(1, 1), (10, 50), (10, 150), (500, 150), (2000, 300)]:
        b = lp.store_bytes(p, dict(max_keyframes=K, max_points=P))
        assert b > last
        last = b
    assert lp.store_bytes(p, dict(max_keyframes=5, max_points=4096)) > lp.store_bytes(p, dict(max_keyframes=5, max_points=4095))
    for K, P in [(0, 10), (-1, 10), (10, 0), (10, -5), (10, 4097)]:
        with pytest.raises(ValueError):
            lp.store_bytes(p, dict(max_keyframes=K, max_points=P))
    for bad in [dict(a_res=0.0), dict(d_res=-1.0), dict(a_res=0.01), dict(d_res=0.001), dict(submap_count=0), dict(min_interval=0)]:
        q = dict(p)
        q.update(bad)
        with pytest.raises(ValueError):
            lp.store_bytes(q, dict(max_keyframes=10, max_points=10))
    W, n_angle = lp.sizes(p)
    assert (W, n_angle) == ref.sizes(p) == (53, 211)


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the handle exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
    lp = liw.loop
    L = liw.lib()
    ctx = C.c_void_p(L.liw_create(C.byref(liw.params_struct(synth.office_params()))))
    try:
        has_dev = False
        try:
            import torch
            has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
        except Exception:
            pass
        if has_dev:
            pytest.skip("a gfx950 device is present")
        h = C.c_void_p(lp._lib().liw_loop_create(ctx, C.byref(lp.params_struct(lp.office_loop_params())),
                                                 C.byref(lp.dims_struct(dict(max_keyframes=4, max_points=8)))))
        assert h
        tf = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
        pts = np.zeros((2, 3))
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert L.liw_loop_add_keyframe(h, 1, pd(tf), 2, pd(pts)) == liw.LIW_ENODEV
        assert L.liw_loop_detect(h, C.byref(lp.LoopEdgeC())) == liw.LIW_ENODEV
        assert L.liw_loop_match(h, 0, 0, 0, None, None, C.byref(lp.LoopMatchInfoC())) == liw.LIW_ENODEV
        assert L.liw_loop_get_row(h, 0, 0, 0, None, None, None, None) == liw.LIW_ENODEV
        assert L.liw_loop_num_keyframes(h) == 0
        assert b"gfx950" in L.liw_loop_last_error(h)
        L.liw_loop_destroy(h)
    finally:
        L.liw_destroy(ctx)


def _planar_pairs(rng, n, noise):
    yaw = rng.uniform(-np.pi, np.pi)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = rng.uniform(-3, 3, 2)
    P2 = np.zeros((n, 3))
    P2[:, :2] = rng.uniform(-8, 8, (n, 2))
    P1 = P2 @ T[:3, :3].T + T[:3, 3]
    P1[:, :2] += rng.normal(0, noise, (n, 2))
    return P1, P2, T


@pytest.mark.parametrize("noise", [0.0, 0.02, 0.2])
def test_icp_closed_form_is_the_lm_optimum(liw, noise):
    rng = np.random.default_rng(11)
    for _ in range(20):
        n = int(rng.integers(3, 40))
        P1, P2, T = _planar_pairs(rng, n, noise)
        got = liw.loop.icp(P1, P2)
        lm = ref.icp_lm(P1, P2)
        assert np.abs(got - lm).max() <= 1e-8, (got, lm)
        assert np.abs(got - ref.icp_closed_form(P1, P2)).max() <= 1e-12
        if noise == 0.0:
            assert np.abs(got - T).max() <= 1e-12


def test_icp_rejects_empty_input(liw):
    with pytest.raises(ValueError):
        liw.loop.icp(np.zeros((0, 3)), np.zeros((0, 3)))


def test_reference_tie_rule_is_the_histogram_rule():
    """The host restatement of the kernel's rule (largest count, then earliest reach time) picks what the serial walk picks."""
    rng = np.random.default_rng(3)
    p = dict(a_res=0.03, d_res=0.03, min_match_threshold=0)
    n_same = 0
    for trial in range(60):
        # lattice points give long runs of equal dij and ties between bins
        g = rng.integers(-4, 5, (int(rng.integers(4, 14)), 2)).astype(float) * 0.3
        g = np.unique(g, axis=0)
        pts = [[x, y, 0.0] for x, y in g]
        rows = ref.describe(pts, p["d_res"], 53)
        for a in range(min(3, len(rows))):
            for b in range(len(rows)):
                w = ref.match_des(rows[a], rows[b], p)
                h = _histogram_rule(rows[a], rows[b], p)
                if w is None:
                    assert h is None or h["size"] == 0
                    continue
                assert (w["size"], w["bin"], w["p1"], w["p2"]) == (h["size"], h["bin"], h["p1"], h["p2"])
                n_same += 1
    assert n_same > 100


def _histogram_rule(d1, d2, p):
    """what k_loop_match + k_loop_select compute: per bin the distinct m and the reach time (m_last, first k of m_last)"""
    import math
    n_angle = int(math.pi * 2 / p["a_res"] + 2)
    orign = n_angle // 2
    cnt, reach = {}, {}
    for m, dm in enumerate(d1["dij"]):
        seen = set()
        for k, dk in enumerate(d2["dij"]):
            if dk != dm:
                continue
            b = ref._bin(d1["aij"][m], d2["aij"][k], p["a_res"], orign, None)
            if b in seen:
                continue
            seen.add(b)
            cnt[b] = cnt.get(b, 0) + 1
            reach[b] = (m, k)
    if not cnt:
        return None
    b = min(cnt, key=lambda b: (-cnt[b], reach[b]))
    p1, p2 = [d1["i"]], [d2["i"]]
    for m, dm in enumerate(d1["dij"]):
        for k, dk in enumerate(d2["dij"]):
            if dk == dm and ref._bin(d1["aij"][m], d2["aij"][k], p["a_res"], orign, None) == b:
                p1.append(d1["j"][m])
                p2.append(d2["j"][k])
                break
    return dict(size=cnt[b] + 1, bin=b, p1=p1, p2=p2)


def test_replay_rejects_detect_loops_on_backend_only_key_frames(liw, tmp_path):
    """--backend-only key frames carry no corners, so --detect-loops would silently find nothing: the tool refuses it."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    libdir = os.path.dirname(liw.LIB_PATH)
    exe = str(tmp_path / "replay_log")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "replay_log.cpp"), "-o", exe,
                           "-L", libdir, "-lliw_window", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    kf = tmp_path / "kf.bin"
    kf.write_bytes(np.array([0], dtype=np.int32).tobytes())
    r = subprocess.run([exe, "--backend-only", str(kf), str(tmp_path) + "/", "--detect-loops"], capture_output=True)
    assert r.returncode == 2 and b"no corners" in r.stderr, r.stderr
    r = subprocess.run([exe, str(kf), str(tmp_path) + "/", "--detect-loops", "--loops", str(kf)], capture_output=True)
    assert r.returncode == 2 and b"exclude each other" in r.stderr, r.stderr
