"""The initialisation glue of the batched laser front-end (liw_lfe_init_*, liw_lfe_slot_copy, liw_lfe_pack_init_sel in
include/liw_laser_batch.h) without a GPU: the names are declared, exported, listed and bound; the record layout is a host-only query;
every compute entry fails with LIW_ENODEV and writes nothing; the host restatement (tests/fleet_init_reference.py, over liw_lie_*)
agrees with an independent plain-numpy one on the cases of the generator; the generator's cases sit where the GPU tests need them;
and a transposed extrinsic would show."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fleet_init_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "liw_laser_batch.h")
NAMES = ("liw_lfe_init_layout", "liw_lfe_init_reset", "liw_lfe_init_get", "liw_lfe_init_begin", "liw_lfe_slot_copy", "liw_lfe_init_select",
         "liw_lfe_pack_init_sel", "liw_lfe_init_commit")
BAR = 1e-12   # the bar of tests/test_laser_track_abi.py (2.7e-15 observed there), which is also the GPU bar of these statements


def _dims(**kw):
    d = dict(B=4, slots=5, max_points=1080, max_lines=128, max_cell_entries=2048)
    d.update(kw)
    return d


def test_names_declared_exported_listed_bound(liw):
    text = open(HDR).read()
    declared = set(re.findall(r"\b(liw_lfe_[A-Za-z_0-9]+)\s*\(", text))
    L = liw.laser_batch._lib()
    for n in NAMES:
        assert n in declared and n in liw.laser_batch.LFE_EXPORTS and hasattr(L, n), n
        assert getattr(L, n).argtypes, n
    assert "liw_lfe_init_params" in text and "LIW_LFE_INITIALIZING" in text and "LIW_LFE_TRACKING" in text
    for m in ("init_layout", "init_reset", "init_get", "init_begin", "slot_copy", "init_select", "pack_init_sel", "init_commit"):
        assert callable(getattr(liw.laser_batch.BatchFrontEnd, m)), m
    assert liw.FleetTrajectory is liw.fleet.FleetTrajectory and issubclass(liw.FleetTrajectory, liw.FleetTracker)
    for m in ("reset", "step", "status", "bias"):
        assert callable(getattr(liw.FleetTrajectory, m)), m
    assert (liw.laser_batch.INITIALIZING, liw.laser_batch.TRACKING) == (ref.INITIALIZING, ref.TRACKING) == (0, 1)
    # liw_lfe_track_params is the struct the tracking glue was merged with
    assert [f[0] for f in liw.laser_batch.TrackParamsC._fields_] == ["T_imu_to_wheel", "normalize_extrinsics", "min_delta_t",
                                                                    "key_frame_p_motion_threshold", "key_frame_q_motion_threshold"]


def test_init_layout_is_host_only(liw):
    lb = liw.laser_batch
    one = lb.init_bytes(_dims(B=1))
    assert one == ref.REC_BYTES
    for B in (2, 130, 49152):
        assert lb.init_bytes(_dims(B=B)) == B * one
    assert lb.init_bytes(_dims(B=1, slots=9, max_lines=512)) == one   # the record does not live in the store
    for k in ("B", "slots", "max_points", "max_lines", "max_cell_entries"):
        for v in (0, -1):
            with pytest.raises(liw.LiwError) as e:
                lb.init_bytes(_dims(**{k: v}))
            assert e.value.code == -22
    L, n = lb._lib(), C.c_size_t(7)
    assert L.liw_lfe_init_layout(None, C.byref(n)) == -22 and n.value == 7
    assert L.liw_lfe_init_layout(C.byref(lb.dims_struct(_dims())), None) == -22


def test_no_cpu_fallback(liw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lb = liw.laser_batch
    L = lb._lib()
    ps = liw.laser.laser_params_struct(liw.laser.office_laser_params())
    dims = lb.dims_struct(_dims())
    tps = lb.track_params_struct(lb.office_track_params())
    ips = lb.init_params_struct(dict(slide_window_size=4, p_motion_threshold=0.1, q_motion_threshold=0.1))
    h = C.c_void_p(L.liw_lfe_create(C.byref(ps), C.byref(dims), 0))
    assert h
    try:
        buf = np.full(1 << 14, 3.25)
        before = buf.copy()
        p = C.c_void_p(buf.ctypes.data)
        E = liw.LIW_ENODEV
        t, i = C.byref(tps), C.byref(ips)
        assert L.liw_lfe_init_reset(h, t, p, None, None) == E
        dp, ip_ = buf.ctypes.data_as(C.POINTER(C.c_double)), buf.ctypes.data_as(C.POINTER(C.c_int))
        assert L.liw_lfe_init_get(h, p, 0, ip_, ip_, dp, dp, ip_) == E
        assert L.liw_lfe_init_begin(h, t, i, p, p, p, p, p, p, p, None, p, p, p, p, p, p, p, p, p, None) == E
        assert L.liw_lfe_slot_copy(h, p, p, None, None) == E
        assert L.liw_lfe_init_select(h, i, p, p, p, p, p, None) == E
        assert L.liw_lfe_pack_init_sel(h, 1, p, 4, 8, p, p, p, p, 6, 64, p, p, p, p, p, p, None) == E
        assert L.liw_lfe_init_commit(h, t, i, p, p, 1, p, p, p, p, p, None) == E
        assert np.array_equal(buf, before)
        assert b"gfx950" in L.liw_lfe_last_error(h) or b"no HIP device" in L.liw_lfe_last_error(h)
    finally:
        L.liw_lfe_destroy(h)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


@pytest.fixture(scope="module")
def generated(liw, synth):
    """per parameter set (extrinsics projected onto SO3): (glue, two pages of 130 robots)"""
    out = {}
    for name, tp, lp, ip in ref.init_param_sets(liw, synth, projected=True):
        g = ref.InitGlue(liw, tp, lp["T_imu_to_laser"], lp["normalize_extrinsics"], ip)
        out[name] = (g, [ref.make_cases(g, 130, seed=21 + page, page=page) for page in range(2)])
    return out


@pytest.mark.parametrize("name", ["office", "second"])
def test_restatement_agrees_with_plain_numpy(liw, synth, generated, name):
    g, pages = generated[name]
    gn = ref.InitGlueNumpy(synth, g.tp, None, None, T12_wheel=g.Tiw, T12_laser=g.Til)
    worst = _close(gn.init_state(), g.init_state())
    for c in pages:
        for b in range(c["state"].shape[0]):
            worst = max(worst, _close(gn.motion(c["wheel_T"][b]), g.motion(c["wheel_T"][b])))
            worst = max(worst, _close(gn.predict(c["state"][b], c["wheel_T"][b]), g.predict(c["state"][b], c["wheel_T"][b])))
    print("init glue, %s set: liw_lie restatement against plain numpy, worst |difference| / max(1, |value|) %.3e" % (name, worst))
    assert worst <= BAR, worst


@pytest.mark.parametrize("name", ["office", "second"])
def test_generator_conditions(liw, generated, name):
    g, pages = generated[name]
    ip = g.ip
    N = ip["slide_window_size"]
    combos, seen = set(), dict(drop=0, go=0, tracking=0)
    for c in pages:
        e = ref.expected(g, c)
        for b in range(c["state"].shape[0]):
            i_p, i_q, i_n = (int(v) for v in c["combo"][b])
            combos.add((i_p, i_q, i_n))
            dp, dq = g.motion(c["wheel_T"][b])
            for value, thr, f in ((dp, ip["p_motion_threshold"], ref.FACTORS[i_p]), (dq, ip["q_motion_threshold"], ref.FACTORS[i_q])):
                assert abs(value / thr - f) <= 1e-9, (b, value, thr, f)
                assert abs(value - thr) >= 1e-3 * thr, (b, value, thr)
            if i_n == 3:
                assert c["status"][b] == ref.TRACKING and e["drop"][b] == -1 and e["slot_of"][b] == -1 and e["row"][b] == -1
                seen["tracking"] += 1
                continue
            assert c["n_frames"][b] == (0, 1, N - 1)[i_n]
            static = ref.FACTORS[i_p] < 1.0 and ref.FACTORS[i_q] < 1.0
            assert e["drop"][b] == int(static)
            seen["drop" if static else "go"] += 1
            if not static:
                assert e["slot_of"][b] == 1 + c["n_frames"][b] == e["n_frames"][b] <= N
                assert np.linalg.norm(e["state"][b, 3:6]) <= ref.MAX_ANGLE
    assert len(combos) == ref.N_COMBOS == 64 and min(seen.values()) >= 40, seen


def test_transposed_extrinsics_would_show(liw, synth, generated):
    """at the second parameter set a transposed T_imu_to_wheel or T_imu_to_laser rotation moves the reference by more than 1 000 bars:
    the wheel extrinsic the predicted pose and the start pose, either one the gate's two norms"""
    g, pages = generated["second"]
    c = pages[0]

    def outputs(glue):
        return np.array([np.concatenate([glue.predict(c["state"][b], c["wheel_T"][b]), glue.motion(c["wheel_T"][b]), glue.init_state()[0:6]])
                         for b in range(16)])

    base = outputs(g)

    def moved(which, negate_t=False):
        m = ref.InitGlue(liw, g.tp, np.eye(4).reshape(16), False, g.ip)
        m.Tiw, m.Til = g.Tiw.copy(), g.Til.copy()
        T = getattr(m, which)
        if negate_t:
            T[9:12] = -T[9:12]
        else:
            T[:9] = T[:9].reshape(3, 3).T.reshape(9)
        return (np.abs(outputs(m) - base) / np.maximum(1.0, np.abs(base))).max(axis=0)

    cols = moved("Tiw")   # the predicted pose, the gate's translation norm, the start pose
    watched = np.concatenate([cols[0:7], cols[8:14]])
    assert watched.max() > 1000 * BAR and np.median(watched) > 1000 * BAR, cols
    # the gate takes norms in the laser frame: |t| and the angle of T_lw * d * T_lw^-1 do not depend on the rotation of T_imu_to_laser
    # (a transposed one cannot show in any output of liw_lfe_init_begin), but they do on its lever arm
    assert moved("Til").max() <= BAR
    cols = moved("Til", negate_t=True)
    assert cols[6] > 1000 * BAR and cols[7] <= BAR, cols
