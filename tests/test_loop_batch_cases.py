"""The host restatement of the fleet loop detector's eight test sequences (tests/loop_batch_cases.py), on any machine: the cases the
GPU test relies on occur, and no gate quantity (origin distance against max_dis, |dp| and |dq| against the tf gates) is within 1e-6
relative of its threshold, so the fleet, the single detector and the restatement can only agree or be wrong."""
import ctypes as C

import numpy as np

import loop_batch_cases as cases


def test_extrinsic_is_loaded_the_same_way(liw, synth):
    """liw_floop_create loads T_imu_to_wheel with liw_lie_from_matrix16(normalize); liw_loop_create takes it from a liw_ctx"""
    prm = synth.office_params()
    M = np.ascontiguousarray(np.asarray(prm["T_imu_to_wheel"], dtype=np.float64).reshape(16))
    T12 = np.zeros(12)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    liw.lib().liw_lie_from_matrix16(pd(M), C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), pd(T12))
    want = cases.T_imu_to_wheel()
    assert np.array_equal(T12[:9].reshape(3, 3), want[:3, :3]) and np.array_equal(T12[9:], want[:3, 3])


def test_sequences_cover_the_cases_and_no_gate_is_near_its_threshold():
    res = cases.restatement()
    assert len(res) == len(cases.ROBOTS) == 8
    found = [[e is not None for e in r["edges"]] for r in res]
    # robot 0: the revisit closes loops, and a later candidate would have passed too
    assert any(found[0]) and res[0]["later_passes"] and all(e["index1"] >= 20 for e in res[0]["edges"] if e)
    # robots 1 and 7: no revisit, no edge
    assert not any(found[1]) and not any(found[7])
    # robot 2: large sub-maps, lists over several 64-wide chunks
    assert min(res[2]["n_points"]) >= 215 and max(res[2]["n_points"]) >= 446 and any(found[2])
    assert max(e["size"] for e in res[2]["edges"] if e) > 130
    # robot 4: candidate 0 matched but the tf gate rejected it, and a later candidate closed the loop
    assert any(k == "tf_q" and v > t for k, v, t in res[4]["gates"])
    assert any(found[4]) and all(e["index2"] != 0 for e in res[4]["edges"] if e)
    # submap_count = 1 robots with a revisit
    assert any(found[5]) and any(found[6]) and any(found[3])
    for i, r in enumerate(res):
        kinds = {k for k, _, _ in r["gates"]}
        assert "dis" in kinds and ("size" in kinds or i in (1, 7))   # without a revisit every candidate is too far away
        assert cases.near_threshold(r["gates"]) == []
    # the origin-distance gate both passes and rejects somewhere (the far leg of the sequences)
    dis = [(v, t) for r in res for k, v, t in r["gates"] if k == "dis"]
    assert any(v > t for v, t in dis) and any(v <= t for v, t in dis)
    # sizes on both sides of the threshold
    sz = [(v, t) for r in res for k, v, t in r["gates"] if k == "size"]
    assert any(v > t for v, t in sz) and any(v <= t for v, t in sz)
    # robots reach min_interval in different fleet frames
    for robots in cases.SETS.values():
        assert len({cases.ROBOTS[r][4] for r in robots}) == len(robots)
