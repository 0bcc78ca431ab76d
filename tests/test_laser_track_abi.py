"""The tracking glue of the batched laser front-end (liw_lfe_track_* in include/liw_laser_batch.h) without a GPU: the names are
declared, exported, listed and bound; the record layout is a host-only query; every compute entry fails with LIW_ENODEV and writes
nothing; the host restatement of the glue (tests/track_glue_reference.py, over liw_lie_*) agrees with an independent plain-numpy one
on the cases of the generator; and the generator's cases sit where the GPU tests need them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_glue_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_laser_batch.h")
NAMES = ("liw_lfe_track_layout", "liw_lfe_track_init", "liw_lfe_track_begin", "liw_lfe_track_end", "liw_lfe_track_get")
POOL = (0, 42, 37, 58)   # line counts of a scan pool: an empty scan, even and odd counts
BAR = 1e-12


def _dims(**kw):
    d = dict(B=4, slots=2, max_points=1080, max_lines=128, max_cell_entries=2048)
    d.update(kw)
    return d


def test_names_declared_exported_listed_bound(liw):
    declared = set(re.findall(r"\b(liw_lfe_[A-Za-z_0-9]+)\s*\(", open(HDR).read()))
    L = liw.laser_batch._lib()
    for n in NAMES:
        assert n in declared and n in liw.laser_batch.LFE_EXPORTS and hasattr(L, n), n
        assert getattr(L, n).argtypes, n
    assert "liw_lfe_track_params" in open(HDR).read()
    for m in ("track_layout", "track_init", "track_begin", "track_end", "track_get"):
        assert callable(getattr(liw.laser_batch.BatchFrontEnd, m)), m
    assert liw.FleetTracker is liw.fleet.FleetTracker
    for m in ("start", "step", "bias"):
        assert callable(getattr(liw.FleetTracker, m)), m


def test_track_layout_is_host_only(liw):
    lb = liw.laser_batch
    one = lb.track_bytes(_dims(B=1))
    assert one > 0 and one % 256 == 0
    for B in (2, 130, 49152):
        assert lb.track_bytes(_dims(B=B)) == B * one
    assert lb.track_bytes(_dims(B=1, slots=5, max_lines=512)) == one   # the record does not live in the store
    for k in ("B", "slots", "max_points", "max_lines", "max_cell_entries"):
        for v in (0, -1):
            with pytest.raises(liw.LiwError) as e:
                lb.track_bytes(_dims(**{k: v}))
            assert e.value.code == -22
    L, n = lb._lib(), C.c_size_t(7)
    assert L.liw_lfe_track_layout(None, C.byref(n)) == -22 and n.value == 7
    assert L.liw_lfe_track_layout(C.byref(lb.dims_struct(_dims())), None) == -22


def test_no_cpu_fallback(liw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(_dims())
    tps = lb.track_params_struct(lb.office_track_params())
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        buf = np.full(1 << 14, 3.25)
        before = buf.copy()
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        assert L.liw_lfe_track_init(h, C.byref(tps), p, p, 30, p, None, None) == E
        assert L.liw_lfe_track_begin(h, C.byref(tps), p, p, p, p, p, p, None, p, p, p, p, None) == E
        assert L.liw_lfe_track_end(h, C.byref(tps), p, p, 0, p, p, None, p, p, None) == E
        dp = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert L.liw_lfe_track_get(h, p, 0, dp, dp, dp, buf.ctypes.data_as(C.POINTER(C.c_int))) == E
        assert np.array_equal(buf, before)
        assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
    finally:
        L.liw_lfe_destroy(h)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


@pytest.fixture(scope="module")
def generated(liw, synth):
    """per parameter set (extrinsics projected onto SO3: two logarithm algorithms agree only on rotations): (glue, cases of two pages
    of 130 robots)"""
    out = {}
    for name, tp, lp in ref.param_sets(liw, synth, projected=True):
        g = ref.Glue(liw, tp, lp["T_imu_to_laser"], lp["normalize_extrinsics"])
        out[name] = (g, [ref.make_cases(g, synth, 130, POOL, seed=11 + page, page=page) for page in range(2)])
    return out


@pytest.mark.parametrize("name", ["office", "second"])
def test_restatement_agrees_with_plain_numpy(liw, synth, generated, name):
    g, pages = generated[name]
    gn = ref.GlueNumpy(synth, g.tp, None, None, T12_wheel=g.Tiw, T12_laser=g.Til)
    worst = 0.0
    for c in pages:
        for b in range(c["x"].shape[0]):
            st = c["x"][b, 1]
            for a, h in zip(g.twist(st, c["angular_local"][b]), gn.twist(st, c["angular_local"][b])):
                worst = max(worst, _close(h, a))
            pn = g.predict(st, c["wheel_T"][b])
            worst = max(worst, _close(gn.predict(st, c["wheel_T"][b]), pn))
            worst = max(worst, _close(gn.tf_w_l(pn), g.tf_w_l(pn)))
            kf = g.lie.make_tf(c["kf_pose"][b, 0:3], c["kf_pose"][b, 3:6])
            for pose in (pn, st[0:6]):
                worst = max(worst, _close(gn.delta(kf, pose), g.delta(kf, pose)))
    print("track glue, %s set: liw_lie restatement against plain numpy, worst |difference| / max(1, |value|) %.3e" % (name, worst))
    assert worst <= BAR, worst


@pytest.mark.parametrize("name", ["office", "second"])
def test_generator_conditions(liw, generated, name):
    g, pages = generated[name]
    tp = g.tp
    combos = set()
    for c in pages:
        e = ref.expected(g, c, POOL)
        B = c["x"].shape[0]
        for b in range(B):
            i_dt, i_p, i_q, i_c = (int(v) for v in c["combo"][b])
            combos.add((i_dt, i_p, i_q, i_c))
            # the quantities sit at the asked multiples, each at least 1e-3 of its threshold away from it
            for value, thr, f in ((c["imu_Dt"][b], tp["min_delta_t"], ref.FACTORS[i_dt]), (e["dp"][b], tp["key_frame_p_motion_threshold"], ref.FACTORS[i_p]),
                                  (e["dq"][b], tp["key_frame_q_motion_threshold"], ref.FACTORS[i_q])):
                assert abs(value / thr - f) <= 1e-9, (b, value, thr, f)
                assert abs(value - thr) >= 1e-3 * thr, (b, value, thr)
            assert e["skip"][b] == int(ref.FACTORS[i_dt] < 1.0)
            n_lines, cnt = POOL[c["scan"][b]], int(c["count"][b])
            case = ref.COUNT_CASES[i_c]
            assert 0 <= cnt <= n_lines
            if case == "fewer":
                assert cnt < n_lines - cnt
            elif case == "more":
                assert cnt > n_lines - cnt
            elif case == "equal":
                assert cnt == n_lines - cnt and n_lines > 0
            else:
                assert cnt == 0 and n_lines == 0
            static = ref.FACTORS[i_p] < 1.0 and ref.FACTORS[i_q] < 1.0
            assert e["key"][b] == int((not static) or case == "fewer"), b
            # bounded conditioning of log_SO3: every pose a logarithm is taken of or a transform is made from
            for q in (c["x"][b, 0, 3:6], c["x"][b, 1, 3:6], e["x"][b, 1, 3:6], c["kf_pose"][b, 3:6]):
                assert np.linalg.norm(q) <= ref.MAX_ANGLE
    assert len(combos) == ref.N_COMBOS == 256   # the full cross product, over the two pages


def test_transposed_extrinsics_would_show(liw, synth, generated):
    """at the second parameter set a transposed T_imu_to_wheel or T_imu_to_laser rotation moves the reference by more than 1 000 bars"""
    g, pages = generated["second"]
    c = pages[0]

    def outputs(glue):
        out = []
        for b in range(16):
            st = c["x"][b, 1]
            pn = glue.predict(st, c["wheel_T"][b])
            kf = glue.lie.make_tf(c["kf_pose"][b, 0:3], c["kf_pose"][b, 3:6])
            out.append(np.concatenate([pn, *glue.twist(st, c["angular_local"][b]), glue.delta(kf, pn)]))
        return np.array(out)

    base = outputs(g)
    for which in ("Tiw", "Til"):
        m = ref.Glue(liw, g.tp, np.eye(4).reshape(16), False)
        m.Tiw, m.Til = g.Tiw.copy(), g.Til.copy()
        T = getattr(m, which)
        T[:9] = T[:9].reshape(3, 3).T.reshape(9)
        move = np.abs(outputs(m) - base) / np.maximum(1.0, np.abs(base))
        cols = move.max(axis=0)
        # wheel: the predicted pose; laser: both twist vectors and the key-frame delta
        watched = cols[0:6] if which == "Tiw" else np.concatenate([cols[6:12], cols[12:14]])
        assert watched.max() > 1000 * BAR and np.median(watched) > 1000 * BAR, (which, cols)


@pytest.mark.parametrize("name", ["office", "second"])
def test_planar_page(liw, synth, name):
    """make_planar_cases, the page of rotations about z that tests/test_gpu_laser_track.py adds to the random axes: it holds the yaws
    it promises, its geometry is planar, every angle a logarithm returns stays within the restatements' range, its quantities keep
    make_cases's distances from the thresholds, and on it the two restatements agree at the same bar."""
    _, tp, lp = [s for s in ref.param_sets(liw, synth, projected=True) if s[0] == name][0]
    g = ref.Glue(liw, tp, lp["T_imu_to_laser"], lp["normalize_extrinsics"])
    gn = ref.GlueNumpy(synth, g.tp, None, None, T12_wheel=g.Tiw, T12_laser=g.Til)
    B = 130
    c = ref.make_planar_cases(g, synth, B, POOL, seed=42, page=2)
    e = ref.expected(g, c, POOL)
    yaws = ref.planar_yaws()
    assert len(set(yaws)) == 18 and max(abs(y) for y in yaws) < ref.PLANAR_MAX_ANGLE
    for base in (np.pi / 2, 3 * np.pi / 4, np.pi - 2e-3):
        for v in (base, np.nextafter(base, 0.0), np.nextafter(base, 4.0)):
            assert v in yaws and -v in yaws
    assert set(c["x"][:, 1, 5]) == set(yaws)
    assert not c["x"][:, :, [2, 3, 4, 8]].any() and not c["angular_local"][:, 0:2].any() and c["angular_local"][:, 2].all()
    worst = 0.0
    for b in range(B):
        W = c["wheel_T"][b]
        assert W[8] == 1.0 and W[11] == 0.0 and not W[[2, 5, 6, 7]].any() and abs(W[3]) > 5e-3   # a pure yaw, a planar translation
        i_dt, i_p, i_q, i_c = (int(v) for v in c["combo"][b])
        for value, thr, f in ((c["imu_Dt"][b], tp["min_delta_t"], ref.FACTORS[i_dt]), (e["dp"][b], tp["key_frame_p_motion_threshold"], ref.FACTORS[i_p]),
                              (e["dq"][b], tp["key_frame_q_motion_threshold"], ref.FACTORS[i_q])):
            assert abs(value / thr - f) <= 1e-9, (b, value, thr, f)
        for q in (c["x"][b, 0, 3:6], c["x"][b, 1, 3:6], e["x"][b, 1, 3:6], c["kf_pose"][b, 3:6]):
            assert np.linalg.norm(q) <= ref.PLANAR_MAX_ANGLE
        st = c["x"][b, 1]
        for a, h in zip(g.twist(st, c["angular_local"][b]), gn.twist(st, c["angular_local"][b])):
            worst = max(worst, _close(h, a))
        pn = g.predict(st, W)
        worst = max(worst, _close(gn.predict(st, W), pn), _close(gn.tf_w_l(pn), g.tf_w_l(pn)))
        kf = g.lie.make_tf(c["kf_pose"][b, 0:3], c["kf_pose"][b, 3:6])
        for pose in (pn, st[0:6]):
            worst = max(worst, _close(gn.delta(kf, pose), g.delta(kf, pose)))
    assert 20 < int(e["skip"].sum()) < B - 20 and 10 < int(e["key"].sum()) < B - 10
    print("track glue, %s set, planar page: liw_lie restatement against plain numpy, worst |difference| / max(1, |value|) %.3e" % (name, worst))
    assert worst <= BAR, worst
