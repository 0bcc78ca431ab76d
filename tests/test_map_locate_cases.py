"""The cases of tests/map_locate_cases.py on the numpy restatement alone (no device): the room trials find the truth, with a unique
maximum, and the hand-made tie, edge and threshold cases behave as they were designed.  tests/test_gpu_map_locate.py runs the same
cases on the MI355X and compares with the same restatement, so a case that shows nothing here shows nothing there."""
import numpy as np
import pytest

import map_locate_cases as lc


@pytest.mark.parametrize("seed", lc.ROOM_SEEDS)
def test_room_trials_find_the_truth(seed):
    r = lc.room_render(seed)
    assert r["width"] > 200 and r["height"] > 200 and r["counts"][50] + r["counts"][100] > 300
    field, info, table = lc.field_of(r["grid"]), lc.info_of(r), lc.room_table()
    assert len(table) == 17 and table[8].tolist() == [1.0, 0.0]
    plain = np.where(r["grid"] >= 50, 2, 0).astype(np.uint8)
    for k, q in enumerate(lc.room_queries(seed)):
        dx, dy, dyaw = q["off"]
        # the truth lies inside the window
        assert abs(dx) / lc.RES <= lc.ROOM_W and abs(dy) / lc.RES <= lc.ROOM_W and abs(np.degrees(dyaw)) <= lc.ROOM_HALF_DEG
        got = lc.match_one(field, info, q["pts"], q["T0"], table, lc.ROOM_W)
        ex, ey, et = lc.room_errors(q, got["best"])
        S = np.sort(got["S"].ravel())
        n_valid = int(got["stats"][1])
        print("seed %d trial %d: %d points, best %s, errors %.2f %.2f cells %.2f steps, margin %d; plain grid score %d" %
              (seed, k, n_valid, got["best"].tolist(), ex, ey, et, S[-1] - S[-2],
               lc.match_one(plain, info, q["pts"], q["T0"], table, lc.ROOM_W)["best"][3]))
        assert got["stats"][0] == lc.OK and n_valid == len(q["pts"]) > 60
        assert ex <= 1.0 and ey <= 1.0 and et <= 1.0
        assert got["stats"][2] == 1 and S[-1] > S[-2]                # the maximum is unique
        assert got["found"] == 1


def test_group_case_finds_the_truth():
    """the joining robot of the end-to-end test, against the serial walk's render of the mapping robot's sub-maps"""
    import map_group_cases as gc
    import map_reference as ref
    c = lc.group_case()
    r = ref.render(gc.compose(c["tfs_of"], c["T_g_w"])[0], c["subs_of"][0], lc.RES)
    got = lc.match_one(lc.field_of(r["grid"]), lc.info_of(r), c["subs_of"][1][0], c["T0"], c["table"], lc.GROUP_W)
    ex, ey, et = lc.group_errors(got["T_m_l"], c["T_g_l_true"])
    print("group case: %d points, best %s, ties %d, errors %.2f %.2f cells %.2f steps" % (got["stats"][1], got["best"].tolist(), got["stats"][2], ex, ey, et))
    assert got["stats"][0] == lc.OK and got["stats"][2] == 1
    assert ex <= 1.0 and ey <= 1.0 and et <= 1.0


def test_field_of_small_grids():
    assert lc.field_of(np.array([[50]], np.int8)).tolist() == [[2]] and lc.field_of(np.array([[0]], np.int8)).tolist() == [[0]]
    g = np.full((3, 5), -1, np.int8)
    g[0, 0], g[2, 4] = 100, 50
    assert lc.field_of(g).tolist() == [[2, 1, 0, 0, 0], [1, 1, 0, 1, 1], [0, 0, 0, 1, 2]]
    g[:] = 49
    assert not lc.field_of(g).any()


def test_tie_case():
    c = lc.tie_case()
    got = lc.match_one(lc.field_of(c["grid"]), c["info"], c["pts"], c["T0"], c["table"], c["W"])
    assert tuple(got["best"]) == c["want_best"] and got["stats"].tolist() == [lc.OK, 20, c["want_ties"], 0]
    S = got["S"][0]
    assert (S[-2 + c["W"]] == 40).all() and (np.delete(S, -2 + c["W"], axis=0) < 40).all()      # every ix of the best row ties
    # three angles that see the same cells: the middle one wins, and the ties add up
    three = lc.match_one(lc.field_of(c["grid"]), c["info"], c["pts"], c["T0"], np.array([[1.0, 0.0]] * 3), c["W"])
    assert tuple(three["best"]) == (1, 0, -2, 40) and three["stats"][2] == 3 * c["want_ties"]
    two = lc.match_one(lc.field_of(c["grid"]), c["info"], c["pts"], c["T0"], np.array([[1.0, 0.0]] * 2), c["W"])
    assert two["best"][0] == 0                                       # (n_theta - 1) / 2 = 0: the lower j


def test_edge_case():
    c = lc.edge_case()
    field = lc.field_of(c["grid"])
    fl = lc.match_one(field, c["info"], c["pts"], c["T0"], c["table"], c["W"])
    tr = lc.match_one(field, c["info"], c["pts"], c["T0"], c["table"], c["W"], cell=np.trunc)
    assert fl["stats"][1] == len(c["pts"]) == 64 and fl["best"][3] > 0
    assert fl["best"][3] == 4 and tr["best"][3] == 4 + 12            # the six quotients in (-1, 0): outside under floor
    # with a window, the points left of the grid reach column 0 at ix = 1
    wide = lc.match_one(field, c["info"], c["pts"], c["T0"], c["table"], 3)
    assert wide["S"][0][3][4] != wide["S"][0][3][3]


def test_threshold_case():
    c = lc.threshold_case()
    field = lc.field_of(c["grid"])
    at = lc.match_one(field, c["info"], c["pts"], c["T0"], c["table"], c["W"], min_permille=c["permille"])
    above = lc.match_one(field, c["info"], c["pts"], c["T0"], c["table"], c["W"], min_permille=c["permille"] + 1)
    assert at["best"][3] == c["score"] and at["stats"][1] == c["n_valid"] and c["score"] * 1000 == c["permille"] * 2 * c["n_valid"]
    assert at["found"] == 1 and above["found"] == 0 and above["best"].tolist() == at["best"].tolist()


def test_statuses():
    c = lc.threshold_case()
    field = lc.field_of(c["grid"])
    run = lambda fld, pts, T0: lc.match_one(fld, c["info"], pts, T0, c["table"], 2)
    assert run(None, c["pts"], c["T0"])["stats"].tolist() == [lc.NO_MAP, 0, 0, 0]
    bad = c["T0"].copy()
    bad[4] = np.nan
    r = run(field, c["pts"], bad)
    assert r["stats"].tolist() == [lc.BAD_PRIOR, 0, 0, 0] and r["T_m_l"].tobytes() == bad.tobytes() and r["found"] == 0
    far = c["T0"].copy()
    far[10] = -1.5e6
    assert run(field, c["pts"], far)["stats"][0] == lc.BAD_PRIOR
    odd = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2e6, 0.0, 0.0]])
    assert run(field, odd, c["T0"])["stats"].tolist() == [lc.NO_POINTS, 0, 0, 0]
    assert run(field, np.zeros((0, 3)), c["T0"])["stats"][0] == lc.NO_POINTS
    mixed = run(field, np.concatenate([odd, c["pts"]]), c["T0"])
    assert mixed["stats"][:2].tolist() == [lc.OK, 10] and mixed["best"][3] == 14
