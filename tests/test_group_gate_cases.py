"""Guards of tests/group_gate_cases.py, on the host and the oracle alone.  The conditions are fixed and the cases are chosen to meet them
with room: at every rejection the rejected edge's c is at least 1.5 x chi2_max and at least 1.5 x the largest other candidate; after
the last round every edge that is still a candidate by support has c <= chi2_max / 4; every solve converges; the restated sequence
ends within gate_rounds.  And the feature's claim: the groups with wrong edges end nearer to the truth gated than ungated."""
import numpy as np
import pytest

import group_gate_cases as cs
import group_graph_cases as gc


@pytest.fixture(scope="module")
def orc(pyoracle, synth):
    return pyoracle.Oracle(synth.office_params())


@pytest.fixture(scope="module")
def pg(liw):
    return liw.posegraph.office_pg_params()


@pytest.fixture(scope="module")
def runs(pyoracle, orc, pg):
    """per group the restated loop with one round more than GATE_ROUNDS: its last gate looks at the end state"""
    return [cs.run(pyoracle, orc, pg, g, gate_rounds=cs.GATE_ROUNDS + 1) for g in range(cs.G)]


def test_the_lists():
    L = cs.lists_after()
    assert [len(l["edges"]) for l in L] == [4, 5, 7, 8] and not any(l["edges_full"] or l["bad_edge"] for l in L)
    assert [e[:3:2] for e in L[0]["edges"]] == [(0, 1), (0, 1), (1, 0), (0, 1)]                       # one of the true edges is stored 1 -> 0
    assert [e[:3:2] for e in L[2]["edges"]] == [(4, 5), (5, 6), (6, 4), (4, 5), (5, 6), (4, 5), (5, 4)]
    for g in range(cs.G):
        Gr = cs.held_graph(L[g], g)
        assert Gr["const"].count(1) == 1 and Gr["const"][0] == 1 and all(Gr["used"]), g
        # with the expected edges gone, an active edge still starts at the constant node (oracle_solve needs it)
        assert any(h[0] == 0 for e, h in enumerate(Gr["held"]) if e not in cs.EXPECT[g]), g
    assert cs.B == 10 and cs.KMAX <= 6 and all(len(c) <= cs.B for c in cs.CALLS)


@pytest.mark.parametrize("group", range(cs.G))
def test_the_rule_has_room(runs, group):
    steps = runs[group]
    gates = [s for s in steps if s is not None and s["kind"] == "gate"]
    solves = [s for s in steps if s is not None and s["kind"] == "solve"]
    assert [s["reject"] for s in gates if s["reject"] is not None] == cs.EXPECT[group]
    assert all(s["reject"] is None for s in gates[cs.GATE_ROUNDS:])                                   # the sequence ends within gate_rounds
    assert len(solves) == 1 + len(cs.EXPECT[group])
    for s in solves:
        assert s["summary"]["termination"] in (1, 2, 3) and s["summary"]["iterations"] < 20, s["summary"]
    for s in gates:
        if s["reject"] is None:
            continue
        c = s["chi2"]
        others = [c[e] for e in s["cands"] if e != s["reject"]]
        print("group %s rejects edge %d at c = %.4g; largest other candidate %.4g" % (cs.NAMES[group], s["reject"], c[s["reject"]], max(others, default=0.0)))
        assert c[s["reject"]] >= 1.5 * cs.CHI2_MAX and c[s["reject"]] >= 1.5 * max(others, default=0.0)
    end = [s for s in gates if s["support"] is not None][-1]                                             # the last gate that was eligible: it rejected nothing
    assert end["reject"] is None and end["changed"] == 0
    by_support = [e for e in range(len(end["chi2"])) if end["state"][e] == 0 and end["support"][e] >= cs.MIN_SUPPORT]
    print("group %s end: c of the edges with support %s" % (cs.NAMES[group], ["%.3g" % end["chi2"][e] for e in by_support]))
    assert by_support and all(end["chi2"][e] <= cs.CHI2_MAX / 4 for e in by_support)


def test_group_c_keeps_the_pair_of_two(runs, pyoracle, orc, pg):
    end = [s for s in runs[2] if s is not None and s["kind"] == "gate" and s["support"] is not None][-1]
    assert end["state"] == [0, 0, 0, 1, 0, 0, 0]
    assert end["chi2"][1] > cs.CHI2_MAX and end["chi2"][4] > cs.CHI2_MAX and end["support"][1] == end["support"][4] == 1      # both exceed, both stay
    # with min_support 1 the pair loses an edge too
    one = cs.run(pyoracle, orc, pg, 2, min_support=1)
    assert [s["reject"] for s in one if s is not None and s["kind"] == "gate"] == [3, 4]
    # group A alone under min_support 1: the same single rejection
    a = cs.run(pyoracle, orc, pg, 0, min_support=1)
    assert [s["reject"] for s in a if s is not None and s["kind"] == "gate"] == [0, None]


def test_one_round_retires_one_edge_of_group_b(pyoracle, orc, pg):
    steps = cs.run(pyoracle, orc, pg, 1, gate_rounds=1)
    assert [s["reject"] for s in steps if s["kind"] == "gate"] == [0] and steps[-1]["used"] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("group", (0, 1))
def test_gated_ends_nearer_to_the_truth(runs, group):
    solves = [s for s in runs[group] if s is not None and s["kind"] == "solve"]
    ungated, gated = cs.deviation_of(solves[0]["x"], group), cs.deviation_of(solves[-1]["x"], group)
    print("group %s: max |T_g_w - truth| ungated %.3e, gated %.3e" % (cs.NAMES[group], ungated, gated))
    assert gated < ungated / 20 and gated < 5e-3                          # from a share of the wrong offset down to the edge noise (1 mm / 0.2 mrad)


def test_no_rotation_near_pi():
    F = cs.fleet()
    from loop_batch_cases import _lie
    pose_of, _ = _lie()
    rots = [pose_of(T)[3:] for T in F["W"] + F["T0"]] + [p[3:] for ps in F["P"] for p in ps]
    for g in range(cs.G):
        rots += [pose_of(h[2])[3:] for h in cs.held_graph(cs.lists_after()[g], g)["held"]]
    assert max(float(np.linalg.norm(q)) for q in rots) < np.pi - 1e-3
    assert gc.MAX_EDGES == cs.MAX_EDGES
