"""C ABI of the fleet loop detector (include/liw_loop_batch.h), on any machine: every liw_floop_* name is exported and listed in
loop_batch.FLOOP_EXPORTS, the header compiles as C99, the size functions are host-only, reject bad params / dims and give a store
about the candidate stride smaller than B single-robot stores, every compute entry fails with LIW_ENODEV without a GPU (no CPU
fallback), and the first-hit formulation of the de-duplication that k_floop_gather uses equals the reference's serial loop bit for
bit."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loop_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_loop_batch.h")
LIW_EINVAL = -22


def test_floop_header_symbols_are_exported(liw):
    declared = sorted(set(re.findall(r"\b(liw_floop_[A-Za-z_0-9]+)\s*\(", open(HDR).read())))
    assert len(declared) >= 12
    L = liw.lib()
    assert not [s for s in declared if not hasattr(L, s)]
    assert sorted(set(liw.loop_batch.FLOOP_EXPORTS)) == declared
    assert liw.FleetLoopDetector is liw.loop_batch.FleetLoopDetector


def test_floop_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "liw_loop_batch.h"\nint f(void) { liw_loop_params p = {0.03, 0.03, 30, 5, 100, 1.0, 1.0, 0.5, 0ull};\n'
                   '  liw_floop_dims d = {4, 10, 10, 8}; size_t n; liw_floop_layout_info i;\n'
                   '  return liw_floop_store_bytes(&p, &d, &n) + liw_floop_layout(&p, &d, &i) + LIW_FLOOP_OVER_CORNERS; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _dims(B=4, K=10, P=16, Cc=8):
    return dict(B=B, max_keyframes=K, max_points=P, max_kf_corners=Cc)


def test_size_functions_reject_bad_params_and_dims(liw):
    fb, lp = liw.loop_batch, liw.loop
    p = lp.office_loop_params()
    assert fb.store_bytes(p, _dims()) == fb.layout(p, _dims())["bytes"] > 0
    assert fb.store_bytes(p, _dims(P=1024)) > fb.store_bytes(p, _dims(P=1023))
    bad_dims = [_dims(P=1025), _dims(P=4096), _dims(P=0), _dims(P=-3), _dims(B=0), _dims(B=-1), _dims(K=0), _dims(K=-2), _dims(Cc=0), _dims(Cc=-1)]
    for d in bad_dims:
        for f in (fb.store_bytes, fb.layout):
            with pytest.raises(liw.LiwError) as ei:
                f(p, d)
            assert ei.value.code == LIW_EINVAL, d
    # the limits of liw_loop.h on the parameters
    for bad in [dict(a_res=0.0), dict(d_res=-1.0), dict(a_res=0.01), dict(d_res=0.001), dict(submap_count=0), dict(min_interval=0),
                dict(min_match_threshold=-1), dict(a_res=float("nan"))]:
        q = dict(p)
        q.update(bad)
        with pytest.raises(liw.LiwError) as ei:
            fb.store_bytes(q, _dims())
        assert ei.value.code == LIW_EINVAL, bad
    L = fb._lib()
    n = C.c_size_t(0)
    assert L.liw_floop_store_bytes(None, C.byref(fb.dims_struct(_dims())), C.byref(n)) == LIW_EINVAL
    assert L.liw_floop_store_bytes(C.byref(lp.params_struct(p)), None, C.byref(n)) == LIW_EINVAL
    assert L.liw_floop_store_bytes(C.byref(lp.params_struct(p)), C.byref(fb.dims_struct(_dims())), None) == LIW_EINVAL
    assert L.liw_floop_layout(C.byref(lp.params_struct(p)), C.byref(fb.dims_struct(_dims())), None) == LIW_EINVAL


@pytest.mark.parametrize("submap_count", [1, 3, 30])
def test_store_is_smaller_than_single_stores_by_about_the_candidate_stride(liw, submap_count):
    fb, lp = liw.loop_batch, liw.loop
    p = lp.office_loop_params()
    p["submap_count"] = submap_count
    B, K, P = 8, 1024, 256
    lay = fb.layout(p, dict(B=B, max_keyframes=K, max_points=P, max_kf_corners=64))
    s = submap_count // 3 + 1
    assert lay["stride"] == s and lay["feature_slots"] == -(-K // s) + 1 and lay["quick_words"] == 53
    assert lay["bytes"] == B * lay["robot_bytes"] + lay["scratch_bytes"] and lay["scratch_off"] == B * lay["robot_bytes"]
    single = B * lp.store_bytes(p, dict(max_keyframes=K, max_points=P))
    ratio = single / lay["bytes"]
    # the single store also keeps 48 P bytes of match results per key frame, the fleet's 96 + 8 bytes of record per key frame, its ring
    # and its scratch: "about" is within 15 % of the stride, and never larger than the single stores
    assert 0.85 * s <= ratio <= 1.15 * s, (ratio, s)
    assert lay["robot_bytes"] >= lay["feature_slots"] * lay["feature_bytes"]


def test_compute_entries_need_a_device(liw, synth):
    """Without a gfx950 device the ctx exists but every compute entry returns LIW_ENODEV (no CPU fallback)."""
    fb, lp = liw.loop_batch, liw.loop
    has_dev = False
    try:
        import torch
        has_dev = torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    except Exception:
        pass
    if has_dev:
        pytest.skip("a gfx950 device is present")
    L = fb._lib()
    prm = synth.office_params()
    Tiw = np.ascontiguousarray(np.asarray(prm["T_imu_to_wheel"], dtype=np.float64).reshape(16))
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert not L.liw_floop_create(None, C.byref(fb.dims_struct(_dims())), pd(Tiw), 1, 0)
    assert not L.liw_floop_create(C.byref(lp.params_struct(lp.office_loop_params())), C.byref(fb.dims_struct(_dims(P=2000))), pd(Tiw), 1, 0)
    assert not L.liw_floop_create(C.byref(lp.params_struct(lp.office_loop_params())), C.byref(fb.dims_struct(_dims())), None, 1, 0)
    h = C.c_void_p(L.liw_floop_create(C.byref(lp.params_struct(lp.office_loop_params())), C.byref(fb.dims_struct(_dims())), pd(Tiw), 1, 0))
    assert h
    try:
        buf = np.zeros(64)   # never dereferenced: the device check comes first
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_floop_reset(h, p, None, None) == E
        assert L.liw_floop_add_keyframes(h, p, p, p, p, 4, p, None, p, None) == E
        assert L.liw_floop_detect(h, p, p, None, p, p, p, p, None) == E
        assert L.liw_floop_num_keyframes(h, p, 0) == E
        assert L.liw_floop_full(h, p, 0) == E
        assert L.liw_floop_status(h, p, 0, 0, None, None, None) == E
        assert L.liw_floop_get_points(h, p, 0, 0, 0, None) == E
        assert L.liw_floop_get_row(h, p, 0, 0, 0, 0, None, None, None, None) == E
        assert L.liw_floop_last_error(h)
    finally:
        L.liw_floop_destroy(h)


# ------------------------------------------------------------------------------------------------------------------ de-duplication
def dedup_first_hit(corner_lists, d_res, lanes=64):
    """What k_floop_gather does per corner: the kept points are tested `lanes` at a time, the first one within 5 d_res is the hit,
    it is blended if it is also within d_res / 2, and no hit appends.  float64 operations in the kernel's order."""
    near, far = d_res / 2, d_res * 5
    pts = np.zeros((0, 3))
    for cs in corner_lists:
        for c in np.asarray(cs, dtype=np.float64).reshape(-1, 3):
            dup = False
            for k0 in range(0, len(pts), lanes):
                chunk = pts[k0:k0 + lanes]
                dx, dy = c[0] - chunk[:, 0], c[1] - chunk[:, 1]
                nrm = np.sqrt(dx * dx + dy * dy)
                hit = nrm < far
                if hit.any():
                    k = k0 + int(np.argmax(hit))
                    if nrm[k - k0] < near:
                        pts[k] = (pts[k] * 3 + c) / 4
                    dup = True
                    break
            if not dup:
                pts = np.concatenate([pts, c[None]])
    return pts


def _corner_lists(rng, d_res, n_lists, n_base):
    """lists with fresh points, blends (within d_res / 2 of an earlier corner), duplicates between d_res / 2 and 5 d_res, and corners
    aimed at where a blended point has moved to"""
    base = np.concatenate([rng.uniform(-2, 2, (n_base, 2)), rng.uniform(-0.1, 0.1, (n_base, 1))], axis=1)
    lists, stats = [], dict(blend=0, dup=0)
    for _ in range(n_lists):
        cs = []
        for _ in range(int(rng.integers(0, n_base + 1))):
            kind = rng.integers(0, 5)
            b = base[rng.integers(0, n_base)]
            ang = rng.uniform(0, 2 * math.pi)
            if kind == 0:
                c = np.concatenate([rng.uniform(-2, 2, 2), rng.uniform(-0.1, 0.1, 1)])
            elif kind in (1, 2):     # a blend; repeated ones walk the kept point away from its first position
                r = rng.uniform(0, 0.49) * d_res
                c = b + [r * math.cos(ang), r * math.sin(ang), rng.uniform(-0.01, 0.01)]
                stats["blend"] += 1
            else:                    # a duplicate that is dropped, or just outside: appended, and then it catches later corners itself
                r = rng.uniform(0.51, 5.6) * d_res
                c = b + [r * math.cos(ang), r * math.sin(ang), 0.0]
                stats["dup"] += 1
            cs.append(c)
        lists.append(np.array(cs).reshape(-1, 3))
    return lists, stats


def test_first_hit_dedup_equals_the_serial_loop_bit_for_bit():
    rng = np.random.default_rng(17)
    d_res = 0.03
    blends = dups = total = moved = 0
    for trial in range(40):
        lists, st = _corner_lists(rng, d_res, int(rng.integers(1, 5)), int(rng.integers(1, 90)))
        want = np.array(ref.dedup(lists, d_res)).reshape(-1, 3)
        for lanes in (64, 7):        # more than one chunk also for short lists
            got = dedup_first_hit(lists, d_res, lanes)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), trial
        blends += st["blend"]
        dups += st["dup"]
        total += len(want)
        flat = np.concatenate(lists)
        moved += sum(1 for p in want if not (flat == p).all(axis=1).any())   # kept points that are no input corner: blended ones
    assert blends > 300 and dups > 300 and total > 500 and moved > 100
