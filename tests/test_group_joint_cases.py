"""Guards of tests/group_joint_cases.py, on the host alone: the structure every group is meant to have, that the oracle holds exactly the
intended node constant, that every case converges within the cap without ground_q, that no rotation is near +-pi, that the separator
and segment lists of the restatement cover every node exactly once, and the feature's claim on the restatement: on groups A and B the
key-frame positions after the joint solve are nearer the truth, in the worst and in the sum, than the rigid T_g_w * P with T_g_w from
the group graph's solve."""
import numpy as np
import pytest

import group_joint_cases as jc
import loop_batch_cases as lbc

CAP = 50


@pytest.fixture(scope="module")
def orc(pyoracle, synth):
    return pyoracle.Oracle(synth.office_params())


@pytest.fixture(scope="module")
def pg(liw):
    return liw.posegraph.office_pg_params()


def test_structure_of_every_group():
    S = [jc.structure(g) for g in range(jc.G)]
    assert [s["members"] for s in S] == [[0, 1, 2], [3, 4, 5], [7], [8, 9, 10], [11]]          # robot 6 holds no key frame, robot 12 is not linked
    assert [s["offsets"] for s in S] == [[0, 8, 20], [0, 60, 65], [0], [0, 10, 20], [0]]
    fl = [s["flags"] for s in S]
    assert [(f["nodes"], f["seq_edges"], f["own_loops"], f["used"], f["skipped"]) for f in fl] == [(30, 27, 1, 3, 2), (66, 63, 0, 6, 0), (20, 19, 2, 0, 0),
                                                                                                  (30, 27, 0, 12, 0), (6, 5, 0, 0, 0)]
    assert [s["const_node"] for s in S] == [0, 0, 0, 0, 0] and all(s["solved"] for s in S)
    assert S[1]["separators"] == [0, 48, 52, 55, 59, 60, 61, 62, 63, 64, 65] and (0, 48) in S[1]["segments"] and (59, 60) not in S[1]["segments"] and (64, 65) not in S[1]["segments"]
    assert S[3]["flags"]["separators"] == 25 and 3 * 25 * (6 * 25 + 1) > 8192                    # group D runs from the work area only
    assert all(3 * s["flags"]["separators"] * (6 * s["flags"]["separators"] + 1) <= 8192 for s in S[:3])
    # one below need raises the matching flag
    assert jc.structure(0, max_members=2)["flags"]["members_full"] == 1 and jc.structure(1, max_nodes=65)["flags"]["nodes_full"] == 1
    assert jc.structure(3, max_loops=11)["flags"]["loops_full"] == 1 and not jc.structure(3, max_loops=12)["flags"]["loops_full"]


@pytest.mark.parametrize("group", range(4))
def test_separators_and_segments_cover_every_node_once(group):
    S = jc.structure(group)
    seen = list(S["separators"])
    for a, b in S["segments"]:
        assert S["chain"][a] == S["chain"][b]
        seen += list(range(a + 1, b))
    assert sorted(seen) == list(range(S["flags"]["nodes"]))
    ends = {n for l in S["loops"] for n in l[:2]}
    assert ends <= set(S["separators"]) and S["const_node"] in S["separators"]
    for a, b in zip(S["separators"], S["separators"][1:]):       # two consecutive separators of different chains are chain ends
        if S["chain"][a] != S["chain"][b]:
            assert b - a == 1


def test_no_rotation_near_pi():
    F = jc.fleet()
    pose_of, _ = lbc._lie()
    rots = [pose_of(T)[3:] for T in F["W"] + F["T0"]] + [p[3:] for ps in F["P"] for p in ps] + [pose_of(T)[3:] for Xs in F["X"] for T in Xs]
    rots += [x[3:] for g in range(4) for x in jc.start_x(g)]
    rots += [pose_of(s)[3:] for ss in F["seq"] for s in ss] + [pose_of(c[5])[3:] for cs in F["cross"].values() for c in cs]
    assert max(float(np.linalg.norm(q)) for q in rots) < np.pi - 1e-3


@pytest.mark.parametrize("group", range(4))
def test_the_oracle_holds_the_intended_node_constant_and_converges(pyoracle, orc, pg, group):
    S = jc.structure(group)
    x0 = jc.start_x(group)
    x, sm = jc.oracle_solve(pyoracle, orc, dict(pg, use_ground_q_factor=False), group, max_iters=CAP)
    print("group %d without ground_q: %s" % (group, sm))
    assert sm["termination"] in (1, 2, 3) and sm["iterations"] < CAP and sm["final_cost"] < sm["initial_cost"], sm
    cn = S["const_node"]
    assert np.array_equal(x[cn], x0[cn])
    assert all(not np.array_equal(x[k], x0[k]) for k in range(len(x0)) if k != cn)


@pytest.mark.parametrize("group", (0, 1))
def test_the_joint_solve_ends_nearer_the_truth_than_the_rigid_alignment(pyoracle, orc, pg, group):
    T, smr = jc.rigid_T(pyoracle, orc, pg, group)
    rigid = jc.rigid_errors(group, T)
    x, sm = jc.oracle_solve(pyoracle, orc, pg, group)
    joint = jc.position_errors(group, x)
    start = jc.position_errors(group, jc.start_x(group))
    print("group %d: start worst %.4f sum %.4f | rigid (group graph %s) worst %.4f sum %.4f | joint (%s) worst %.4f sum %.4f"
          % (group, start.max(), start.sum(), smr["termination"], rigid.max(), rigid.sum(), sm["termination"], joint.max(), joint.sum()))
    assert smr["termination"] in (1, 2, 3) and sm["termination"] in (1, 2, 3, 4)       # with ground_q the office configuration may run into the cap
    assert joint.max() < rigid.max() and joint.sum() < rigid.sum()
