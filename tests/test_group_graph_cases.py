"""Guards of tests/group_graph_cases.py, on the host alone: the lists the three add_edges calls leave, the partner rule against
liw_xloop_partner's restatement, that the oracle holds exactly the first edge's index1 constant on edge lists that are no chain, that
every case converges, that noise-free edges give back the truth, that no rotation is near +-pi, and the feature's claim on the
restatement: with the +-1 mm corner-noise edges of loop_cross_cases a cycle of four robots ends closer to the truth after the
refinement than the chained T_g_w that liw_xloop_link gives."""
import numpy as np
import pytest

import group_graph_cases as gc
import loop_batch_cases as lbc
import loop_cross_cases as xc
import loop_reference as ref


@pytest.fixture(scope="module")
def orc(pyoracle, synth):
    return pyoracle.Oracle(synth.office_params())


@pytest.fixture(scope="module")
def pg(liw):
    return liw.posegraph.office_pg_params()


def test_lists_after_the_three_calls():
    one, two, three = gc.lists_after(1), gc.lists_after(2), gc.lists_after(3)
    assert [len(L["edges"]) for L in one] == [2, 4, 4] and not any(L["edges_full"] or L["bad_edge"] for L in one)
    assert [len(L["edges"]) for L in two] == [2, 6, 7] and [L["bad_edge"] for L in two] == [1, 0, 0] and not any(L["edges_full"] for L in two)
    assert [len(L["edges"]) for L in three] == [2, 6, 8] and [L["edges_full"] for L in three] == [0, 0, 1] and [L["bad_edge"] for L in three] == [1, 0, 0]
    assert [e[:4] for e in three[0]["edges"]] == [(0, 5, 1, 2), (1, 4, 2, 3)]                      # the masked-out robot 0 added nothing in call 2
    assert [e[:3:2] for e in three[2]["edges"]] == [(7, 8), (8, 9), (9, 10), (10, 7), (8, 10), (9, 7), (10, 11), (7, 9)]
    assert three[2]["edges"][0][4] == 30                                                           # the duplicate did not replace the held edge
    graphs = [gc.group_graph(g) for g in range(gc.G)]
    assert [Gr["nodes"] for Gr in graphs] == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10]]
    assert [Gr["const"] for Gr in graphs] == [[1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 0]]
    assert [Gr["used"] for Gr in graphs] == [[1, 1], [1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 0, 0, 1]]      # 3 -> 5 joins two constants
    # a list that is full from the start, and a robot outside every group
    L = gc.add_edges(gc.new_lists(1), [0, 0, -1], [1, 1, 1], [(0, 1, 0, 9), (0, 0, 0, 9), (0, 0, 0, 9)], np.zeros((3, 12)), max_edges=1)
    assert len(L[0]["edges"]) == 1 and L[0]["edges_full"] == 1 and L[0]["bad_edge"] == 0


def test_partner_rule():
    for rnd in range(6):
        got = gc.choose_partners(gc.GROUP_OF, gc.LINKED, rnd)
        old = xc.choose_partners(gc.GROUP_OF, gc.LINKED, rnd)
        assert got[11] == old[11] == [7, 8, 9, 10][rnd % 4]                  # the unlinked robot: liw_xloop_partner's choice
        assert got[:3] == [[1, 2][rnd % 2], [0, 2][rnd % 2], [0, 1][rnd % 2]]
        assert got[3] == [4, 5, 6][rnd % 3] and got[8] == [7, 9, 10][rnd % 3]
        assert all(p != a for a, p in enumerate(got))
    assert gc.choose_partners([0, 0, 1, -1], [1, 0, 1, 1], 4) == [-1, 0, -1, -1]    # alone in its group: no partner


def test_no_rotation_near_pi():
    F = gc.fleet()
    pose_of, _ = lbc._lie()
    rots = [pose_of(T)[3:] for T in F["W"] + F["T0"]] + [p[3:] for ps in F["P"] for p in ps]
    for g in range(gc.G):
        rots += [pose_of(e[2])[3:] for e in gc.group_graph(g)["edges"]]
    assert max(float(np.linalg.norm(q)) for q in rots) < np.pi - 1e-3


def test_z_is_the_truth_for_noise_free_edges():
    F = gc.fleet()
    for ia, ib, Z in gc.group_graph(1)["edges"]:
        a, b = gc.group_graph(1)["nodes"][ia], gc.group_graph(1)["nodes"][ib]
        assert gc.deviation(Z, ref.iso_inv(F["W"][a]) @ F["W"][b]) < 1e-12


def test_the_oracle_holds_the_first_index_constant(pyoracle, orc, pg):
    """a cycle with a chord (node 1 has three edges), the constant node in the middle of the node list and of the edge list"""
    F = gc.fleet()
    Gr = gc.group_graph(1)
    robots = Gr["nodes"]
    _, mk = lbc._lie()
    for const in (0, 1, 3):
        if not any(e[0] == const for e in Gr["edges"]):
            continue
        T0 = [F["W"][r] @ gc._small(np.random.default_rng(5 + r), gc.START_P, gc.START_Q) for r in range(gc.B)]
        x0 = gc.start_x(robots, T0)
        x, sm = gc.oracle_solve(pyoracle, orc, pg, x0, Gr["edges"], const)
        assert sm["termination"] in (1, 2, 3) and sm["successful"] >= 2, sm
        assert np.array_equal(x[const], x0[const])
        assert all(not np.array_equal(x[k], x0[k]) for k in range(len(robots)) if k != const)
        # noise-free: everything is where the constant node's frame puts it, X_k = X_const W_const^-1 W_k
        for k, r in enumerate(robots):
            want = mk(x0[const]) @ ref.iso_inv(F["W"][robots[const]]) @ F["W"][r]
            assert gc.deviation(mk(x[k]), want) <= 1e-9, (const, k, gc.deviation(mk(x[k]), want))


@pytest.mark.parametrize("group", (0, 2))
def test_every_case_converges(pyoracle, orc, pg, group):
    Gr = gc.group_graph(group)
    assert Gr["const"].count(1) == 1
    x0 = gc.start_x(Gr["nodes"])
    x, sm = gc.oracle_solve(pyoracle, orc, pg, x0, Gr["edges"], Gr["const"].index(1))
    assert sm["termination"] in (1, 2, 3) and sm["iterations"] < 20 and sm["final_cost"] < sm["initial_cost"], sm
    _, mk = lbc._lie()
    F = gc.fleet()
    before = max(gc.deviation(F["T0"][r], F["W"][r]) for r in Gr["nodes"])
    after = max(gc.deviation(mk(x[k]), F["W"][r]) for k, r in enumerate(Gr["nodes"]))
    assert after < before / 4, (before, after)                   # from 2 cm / 5 mrad down to the edge noise


def test_a_cycle_ends_closer_to_the_truth_than_the_chain(pyoracle, orc, pg):
    """Robots 0 .. 3 of loop_cross_cases' fleet, anchor 0: liw_xloop_link chains 1, 3 and 2 through one edge each and drops the edge
    2 -> 0; the group graph keeps all four."""
    E = gc.claim_edges()
    pose_of, mk = lbc._lie()
    W0 = xc.fleet(gc.CLAIM_FLEET)["W"][0]
    truth = [W0 @ ref.iso_inv(xc.fleet(gc.CLAIM_FLEET)["W"][r]) for r in range(4)]          # T_g_w with the anchor's world as the group frame
    chained = [np.eye(4)] * 4
    for a, b in gc.CLAIM_CHAIN:
        chained[a] = chained[b] @ ref.iso_inv(E[a, b])                                      # rule (i) of liw_xloop_link
    edges = [(a, b, E[a, b]) for a, b in [gc.CLAIM_CLOSE] + gc.CLAIM_CHAIN]
    edges = [(b, a, ref.iso_inv(T)) if b == 0 else (a, b, T) for a, b, T in edges[1:2]] + edges[:1] + edges[2:]
    assert edges[0][0] == 0                                                                   # 1 -> 0 turned round, so that the anchor is index1
    x, sm = gc.oracle_solve(pyoracle, orc, pg, np.array([pose_of(T) for T in chained]), edges, 0)
    assert sm["termination"] in (1, 2, 3), sm
    refined = [mk(x[k]) for k in range(4)]
    d_chain = [gc.deviation(chained[r], truth[r]) for r in range(1, 4)]
    d_ref = [gc.deviation(refined[r], truth[r]) for r in range(1, 4)]
    print("chained   ", ["%.3e" % d for d in d_chain], "\nrefined   ", ["%.3e" % d for d in d_ref], sm)
    assert np.array_equal(x[0], pose_of(np.eye(4)))
    assert max(d_ref) < max(d_chain) and sum(d_ref) < sum(d_chain)
