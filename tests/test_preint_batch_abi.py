"""C ABI of the fleet's pre-integration (include/liw_preint_batch.h), on any machine: every liw_fpre_* name is exported and listed in
preint_batch.FPRE_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad dims and add up, every compute
entry fails with LIW_ENODEV without a GPU (no CPU fallback), and the checker of tests/test_gpu_preint_batch.py (the replay of
tests/preint_batch_cases.py) agrees with host accumulators that really were carried across skipped scans."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import preint_batch_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_preint_batch.h")
LIW_EINVAL = -22


def test_fpre_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_fpre_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 9
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.preint_batch.FPRE_EXPORTS)) == declared
    assert liw.FleetPreint is liw.preint_batch.FleetPreint


def test_fpre_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_preint_batch.h"\nint f(void) { liw_fpre_dims d = {4}; size_t n; liw_fpre_layout_info i; liw_fpre_state s;\n'
                   '  s.imu_inited = 0; return liw_fpre_store_bytes(&d, &n) + liw_fpre_layout(&d, &i) + (int)s.imu_inited; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_size_functions_reject_bad_dims_and_add_up(liw):
    fp = liw.preint_batch
    for B in (1, 4, 7, 1026, 1 << 20):
        lay = fp.layout(dict(B=B))
        assert fp.store_bytes(dict(B=B)) == lay["bytes"] == B * lay["robot_bytes"] + lay["shared_bytes"] > 0
        assert lay["shared_off"] == B * lay["robot_bytes"] and lay["shared_bytes"] % 256 == 0
        assert 225 * 8 * B <= lay["shared_bytes"] < 225 * 8 * B + 256          # the aligned covariances
        assert lay["robot_bytes"] == 4608 and lay["robot_bytes"] % 256 == 0      # independent of B
        offs = [lay[k] for k in fp.LAYOUT_PARTS] + [lay["robot_bytes"]]
        p = lay["mat_pitch"]
        assert p == 16
        # X (15 doubles and a pad), J and P (15 rows of `pitch`), last_acc / last_gyro / time / Dt, the wheel's 33, stamp + bias, latch
        need = [8 * 16, 8 * 15 * p, 8 * 15 * p, 8 * 8, 8 * 33, 8 * 7, 8]
        assert offs[0] == 0 and all(o % 8 == 0 for o in offs)
        for a, b, n in zip(offs[:-1], offs[1:-1], need[:-1]):     # the parts follow each other without a gap
            assert b - a == n
        assert offs[-2] + need[-1] <= offs[-1] < offs[-2] + need[-1] + 256
        assert (lay["J_off"] % 128, lay["P_off"] % 128) == (0, 0)                # a row of J / P is one aligned 128-byte piece
    assert fp.store_bytes(dict(B=5)) > fp.store_bytes(dict(B=4))
    for bad in (0, -1, (1 << 20) + 1):
        for f in (fp.store_bytes, fp.layout):
            with pytest.raises(liw.LiwError) as ei:
                f(dict(B=bad))
            assert ei.value.code == LIW_EINVAL, bad
    L = fp._lib()
    n, ds = C.c_size_t(7), fp.dims_struct(dict(B=4))
    assert L.liw_fpre_store_bytes(None, C.byref(n)) == LIW_EINVAL and n.value == 7
    assert L.liw_fpre_store_bytes(C.byref(ds), None) == LIW_EINVAL
    assert L.liw_fpre_layout(C.byref(ds), None) == LIW_EINVAL
    assert L.liw_fpre_layout(None, C.byref(fp.FpreLayoutC())) == LIW_EINVAL


def test_state_struct_is_liw_fpre_state(liw, tmp_path):
    """FpreStateC mirrors liw_fpre_state: 513 doubles and the two latch bytes"""
    assert C.sizeof(liw.preint_batch.FpreStateC) == 513 * 8 + 8
    assert liw.preint_batch.FpreStateC.imu_inited.offset == 513 * 8


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
    fp = liw.preint_batch
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L = fp._lib()
    ps, ds = liw.params_struct(synth.office_params()), fp.dims_struct(dict(B=4))
    assert not L.liw_fpre_create(None, C.byref(ds))
    assert not L.liw_fpre_create(C.byref(ps), None)
    assert not L.liw_fpre_create(C.byref(ps), C.byref(fp.dims_struct(dict(B=0))))
    h = C.c_void_p(L.liw_fpre_create(C.byref(ps), C.byref(ds)))
    assert h
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes first
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_fpre_reset(h, p, None, None) == E
        assert L.liw_fpre_push(h, p, p, p, p, p, p, p, None, p, p, p, p, p, p, p, p, None) == E
        assert L.liw_fpre_commit(h, p, p, None, None) == E
        assert L.liw_fpre_get(h, p, 0, C.byref(fp.FpreStateC())) == E
        assert L.liw_fpre_last_error(h)
        assert L.liw_fpre_reset(None, p, None, None) == LIW_EINVAL
    finally:
        L.liw_fpre_destroy(h)


def test_replay_agrees_with_carried_accumulators(liw, synth):
    """The checker of the GPU tests replays a robot's history into fresh accumulators at every frame.  Here the base case's robots are
    also run the way lvio_2d::trajectory runs them: ONE pair of accumulators per robot, fed message by message, aligned and reset only
    at the scans that are taken (a skipped scan returns before update_only_t / reset).  At every taken scan the carried accumulators'
    result must equal the replay's bit for bit, and robots 4 and 5 (not taken for one and for two frames) are among them."""
    case = cases.base_case(synth)
    prm, B, F = case["prm"], case["B"], case["F"]
    hf = cases.HostFleet(liw, prm, B)
    acc = [(liw.ImuPreintegration(prm), liw.WheelPreintegration(prm)) for _ in range(B)]
    inited = np.zeros((B, 2), dtype=bool)
    merged = {}
    since = np.zeros(B, dtype=int)
    for k in range(F):
        exp = hf.push(case["imu"][k], case["wheel"][k], case["stamps"][k], case["bias"][k])
        for b in range(B):
            for r in case["imu"][k][b]:
                inited[b, 0] |= acc[b][0].add_imu_measure(r[0], r[1:4], r[4:7])
            for r in case["wheel"][k][b]:
                inited[b, 1] |= acc[b][1].add_wheel_odom_measure(r[0], r[1:10], r[10:13])
            assert int(inited[b].all()) == exp[b]["ready"], (k, b)
            if not (inited[b].all() and case["taken"][k, b]):
                since[b] += int(inited[b].all())
                continue
            st, bias = case["stamps"][k, b], case["bias"][k, b]
            acc[b][1].update_only_t(st)
            acc[b][0].update_only_t(st)
            X, J, S, Dt = acc[b][0].get_preintegraption_result()
            T, Sw, Dtw = acc[b][1].get_preintegraption_result()
            got = dict(imu_X=X, imu_J=np.asarray(J).reshape(225), imu_sqrtP=np.asarray(S).reshape(225), imu_Dt=Dt, wheel_T=T,
                       wheel_sqrtP=np.asarray(Sw).reshape(9), wheel_Dt=Dtw)
            for key, v in got.items():
                assert np.array_equal(np.asarray(v), np.asarray(exp[b]["rows"][key])), (k, b, key)
            acc[b][1].reset_wheel_odom_measure(st)
            acc[b][0].reset_imu_measure(st, bias[0:3], bias[3:6])
            merged[b] = max(merged.get(b, 0), since[b])
            since[b] = 0
        hf.commit(case["taken"][k])
    assert merged[4] == 1 and merged[5] == 2 and merged[0] == 0
    assert {"seed", "integrated", "gated", "gap"} <= hf.arms
