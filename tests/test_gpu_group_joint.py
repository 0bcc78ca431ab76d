"""The joint pose graph of a group on the MI355X (include/liw_group_joint.h, group_joint.FleetGroupJoint) on the cases of
tests/group_joint_cases.py: structure and flags against the restatement, x0 against liw_lie_* of the device's own inputs, the solve
against the oracle at the bars of tests/test_gpu_posegraph_batch.py (also with a constant node that is not node 0), the single-member group against FleetBackEnd.solve, the claim
against FleetGroupGraph.solve's rigid alignment, bit-identity (alone, at other indices, tiled, two runs, check_every, work area), a NaN
group among healthy ones, what must stay untouched, and the pipeline FleetLoopDetector.push -> FleetBackEnd.push ->
FleetGroupGraph.push -> FleetGroupJoint.push -> FleetGroupMap.render end to end."""
import ctypes as C
import importlib

import numpy as np
import pytest

import group_graph_cases as gc
import group_joint_cases as jc
import loop_batch_cases as lbc
import loop_cross_cases as xc
import map_batch_cases as mc
import map_group_cases as mgc
import map_reference as mref
import test_gpu_loop as tgl
import test_gpu_loop_batch as tlb

pytestmark = pytest.mark.gpu
GUARD = 256
ULP_BAR = 4.0
FLAG_KEYS = ("members_full", "nodes_full", "loops_full", "members", "nodes", "seq_edges", "own_loops", "used", "skipped", "separators", "solved", "const_node")


@pytest.fixture(scope="module")
def mods(liw):
    return importlib.import_module(liw.__name__ + ".group_graph"), importlib.import_module(liw.__name__ + ".group_joint")


class Rig:
    """detector (for its handle only), back-end holding the cases' graphs, aligner in the cases' state, the group graph holding the cases'
    cross edges, and the joint graph; `tiles` copies of the thirteen robots (robot r of tile t is r + 13 t, its group g + 5 t)"""

    def __init__(self, liw, synth, mods, tiles=1, guard=0, max_members=jc.MAX_MEMBERS, max_nodes=jc.MAX_NODES, max_loops=jc.MAX_LOOPS, pg=None, cross=None,
                 fixed=None):
        import torch
        gg, gj = mods
        F = jc.fleet()
        self.liw, self.tiles, self.B, self.torch = liw, tiles, jc.B * tiles, torch
        B = self.B
        prm = synth.office_params()
        self.pg = liw.posegraph.office_pg_params() if pg is None else pg
        self.fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=jc.K, max_points=16, max_kf_corners=8))
        self.fb = liw.FleetBackEnd(prm, self.pg, dict(B=B, max_keyframes=jc.K, max_loops=jc.RL), solve_period=1e9, guard=guard)
        for r in range(B):
            if jc.NKF[r % jc.B]:
                self.fb.load_graph(r, jc.backend_graph(r % jc.B))
        self.group_of = [g + jc.G * t for t in range(tiles) for g in jc.GROUP_OF]
        self.linked, self.fixed = list(jc.LINKED) * tiles, list(jc.FIXED if fixed is None else fixed) * tiles   # the aligner's anchors are these
        self.al = liw.FleetGroupAligner(self.fl, self.group_of, {r: F["W"][r % jc.B] for r in range(B) if self.fixed[r]}, 9, xc.MAX_RMS)
        self.al.linked.copy_(torch.tensor(self.linked, dtype=torch.uint8))
        self.al.via[torch.tensor([bool(l and not f) for l, f in zip(self.linked, self.fixed)], device=self.al.dev)] = 0
        self.al.T_g_w.copy_(torch.tensor(np.array([gc.tf12_of(F["T0"][r % jc.B]) for r in range(B)])))
        self.g = gg.FleetGroupGraph(self.al, self.fb, jc.MAX_MEMBERS, jc.MAX_EDGES, groups=jc.G * tiles, guard=guard)
        self.feed(F["cross"] if cross is None else cross)
        self.j = gj.FleetGroupJoint(self.g, self.fb, max_nodes, max_loops, guard=guard, max_members=max_members)
        self.gsel = jc.GSEL * tiles

    def feed(self, cross):
        """one liw_ggraph_add_edges call per list position, so that every group's list has the cases' order; then the state words"""
        B0, torch = jc.B, self.torch
        for e in range(max(len(v) for v in cross.values())):
            found, edge, tf12 = np.zeros(self.B, np.uint8), np.zeros((self.B, 4), np.int32), np.zeros((self.B, 12))
            for ls in cross.values():
                if e < len(ls):
                    a, q, b, i, st, T = ls[e]
                    for t in range(self.tiles):
                        found[a + B0 * t], edge[a + B0 * t], tf12[a + B0 * t] = 1, (q, b + B0 * t, i, 20), gc.tf12_of(T)
            self.g.add_edges(dict(found=found, edge=edge, tf12=tf12))
        regions = self.g.group_regions()
        for g, ls in cross.items():
            for e, c in enumerate(ls):
                if c[4]:
                    for t in range(self.tiles):
                        regions[g + jc.G * t, 256 + 128 * e + 20:256 + 128 * e + 24] = torch.tensor([c[4], 0, 0, 0], dtype=torch.uint8, device=regions.device)

    def solve(self, gsel=None, **kw):
        return self.j.solve(gsel=self.gsel if gsel is None else gsel, **kw)

    def rows(self):
        self.j._sync()
        return self.j.poses().cpu().numpy().copy()

    def group_rows(self, g, rows=None, tile=0):
        """[N, 6]: the rows of group g's nodes"""
        rows = self.rows() if rows is None else rows
        return np.concatenate([rows[r + jc.B * tile, :jc.NKF[r]] for r in jc.structure(g)["members"]])

    def close(self):
        for o in (self.j, self.g, self.fb, self.fl):
            o.close()


_CACHE = {}


def _x0_rows(liw, synth, mods):
    """the device's x0 rows of every member of groups A - D: a joint graph that holds one loop edge solves none of them"""
    if "x0" not in _CACHE:
        R = Rig(liw, synth, mods, max_loops=1)
        R.solve()
        _CACHE["x0"] = R.rows()
        _CACHE["x0_flags"] = [R.j.flags(g) for g in range(jc.G)]
        _CACHE["x0_inputs"] = (R.al.T_g_w.cpu().numpy().copy(), [R.fb.keyframes(r)["poses"] if jc.NKF[r] else np.zeros((0, 6)) for r in range(jc.B)])
        R.close()
    return _CACHE["x0"]


def _baseline(liw, synth, mods, cap=20):
    """rows, headers and summaries of the cases solved together at cap iterations"""
    if ("base", cap) not in _CACHE:
        R = Rig(liw, synth, mods)
        R.solve(max_iters=cap)
        _CACHE["base", cap] = (R.rows(), R.j.header_bytes().cpu().numpy().copy(), R.j.summary.cpu().numpy().copy())
        R.close()
    return _CACHE["base", cap]


def _oracle(liw, synth, pyoracle, group, cap, ground_q):
    if (group, cap, ground_q) not in _CACHE:
        orc = _CACHE.setdefault("orc", pyoracle.Oracle(synth.office_params()))
        pg = dict(liw.posegraph.office_pg_params(), use_ground_q_factor=ground_q)
        _CACHE[group, cap, ground_q] = (pg, jc.oracle_solve(pyoracle, orc, pg, group, max_iters=cap))
    return _CACHE[group, cap, ground_q]


# --------------------------------------------------------------------------------------------------------------------- structure
def test_structure_equals_the_restatement(liw, synth, mods):
    R = Rig(liw, synth, mods, guard=GUARD)
    R.solve(max_iters=2)
    for g in range(jc.G):
        fl, S = R.j.flags(g), jc.structure(g)
        if not jc.GSEL[g]:
            assert not any(fl.values()) and R.j.members(g) == ([], [])
            continue
        assert {k: fl[k] for k in FLAG_KEYS} == S["flags"], (g, fl, S["flags"])
        assert R.j.members(g) == (S["members"], S["offsets"]), g
        row, sepidx = R.j.nodes(g)
        assert row == [r * jc.K + k for r in S["members"] for k in range(jc.NKF[r])], g
        assert R.j.separators(g) == S["separators"], g
        assert sepidx == [S["separators"].index(n) if n in S["separators"] else -1 for n in range(S["flags"]["nodes"])], g
        assert R.j.last_summary(g)["termination"] == 4 and R.j.last_summary(g)["iterations"] == 2
    assert bool((R.j._buf[:GUARD] == 0xA5).all()) and bool((R.j._buf[-GUARD:] == 0xA5).all())
    R.close()


@pytest.mark.parametrize("what", ("max_members", "max_nodes", "max_loops"))
def test_one_below_need_raises_the_flag_and_leaves_x0(liw, synth, mods, what):
    x0 = _x0_rows(liw, synth, mods)
    group, kw = {"max_members": (0, dict(max_members=2)), "max_nodes": (1, dict(max_nodes=65)), "max_loops": (3, dict(max_loops=11))}[what]
    R = Rig(liw, synth, mods, **kw)
    R.solve()
    rows = R.rows()
    for g in range(4):
        fl, S = R.j.flags(g), jc.structure(g, **kw)
        assert {k: fl[k] for k in FLAG_KEYS} == S["flags"], (g, fl, S["flags"])
        full = fl["members_full"] or fl["nodes_full"] or fl["loops_full"]
        for r in jc.structure(g)["members"]:
            same = rows[r, :jc.NKF[r]].tobytes() == x0[r, :jc.NKF[r]].tobytes()
            assert same == bool(full), (g, r)
        if full:
            assert R.j.last_summary(g) == dict(iterations=0, successful=0, termination=0, initial_cost=0.0, final_cost=0.0)
    fl = R.j.flags(group)
    assert fl[{"max_members": "members_full", "max_nodes": "nodes_full", "max_loops": "loops_full"}[what]] == 1 and fl["solved"] == 0
    R.close()


def test_x0_is_the_product_of_the_devices_own_inputs(liw, synth, mods):
    """x0 = log_SE3(T_g_w * make_tf(P)) against liw_lie_make_tf / liw_lie_mul / liw_lie_log_SE3 of the T_g_w and P read back from the device.
    The position is liw_lie_mul's translation (make_tf copies p), so its unit is the entry's own spacing.  The host's sin / cos are libm's
    (within 1 ulp of 1.0 in a matrix entry) where the device's are correctly rounded, an absolute difference that a rotation component
    far below the rotation's size cannot be measured against: the unit of the rotation vector is the spacing at its largest component."""
    x0 = _x0_rows(liw, synth, mods)
    assert [f["loops_full"] for f in _CACHE["x0_flags"][:4]] == [1, 1, 1, 1]
    T, P = _CACHE["x0_inputs"]
    pose_of, mk = lbc._lie()
    worst_p, worst_q, n = 0.0, 0.0, 0
    for r in range(jc.B):
        for k in range(jc.NKF[r]):
            if jc.GSEL[jc.GROUP_OF[r]] and jc.LINKED[r]:
                want = pose_of(gc.mat_of(mgc.lie_mul(liw, T[r], gc.tf12_of(mk(P[r][k])))))
                worst_p = max(worst_p, mc.ulps(x0[r, k, :3], want[:3]))
                worst_q = max(worst_q, float(np.abs(x0[r, k, 3:] - want[3:]).max() / np.spacing(np.abs(want[3:]).max())))
                n += 1
    print("x0: %d rows, worst distance from log_SE3(liw_lie_mul(T_g_w, make_tf(P))): position %.1f ulp, rotation %.1f ulp" % (n, worst_p, worst_q))
    assert n == 146 and worst_p <= ULP_BAR and worst_q <= ULP_BAR


# --------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("cap,ground_q", ((5, True), (20, True), (0, False)))
def test_solve_against_the_oracle(liw, synth, mods, pyoracle, cap, ground_q):
    x0 = _x0_rows(liw, synth, mods)
    pg = dict(liw.posegraph.office_pg_params(), use_ground_q_factor=ground_q)
    R = Rig(liw, synth, mods, pg=pg)
    R.solve(max_iters=cap)
    sm, rows = R.j.summaries(), R.rows()
    for g in range(4):
        _, (xo, so) = _oracle(liw, synth, pyoracle, g, cap, ground_q)
        s, x = sm[g], R.group_rows(g, rows)
        print("cap %d ground_q %d group %d device %s\n%34s %s\n   |x - oracle| %.3e" % (cap, ground_q, g, s, "oracle", so, np.abs(x - xo).max()))
        assert (s["iterations"], s["successful"], s["termination"]) == (so["iterations"], so["successful"], so["termination"]), (g, s, so)
        assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-9 * so["initial_cost"], g
        assert abs(s["final_cost"] - so["final_cost"]) <= 1e-6 * max(1.0, so["final_cost"]), g
        assert np.abs(x - xo).max() <= 1e-6 * max(1.0, np.abs(xo).max()), g
        S = jc.structure(g)
        r0 = S["const_member"]
        assert rows[r0, 0].tobytes() == x0[r0, 0].tobytes(), g                     # the constant node: bit for bit x0
        assert rows[r0, 1].tobytes() != x0[r0, 1].tobytes(), g
        assert R.j.last_summary(g) == s
        if cap == 0:
            assert s["termination"] in (1, 2, 3), s
    R.close()


# the anchors moved off the first member: robot 1 in group A (constant node 8 of 30), robot 4 in group B (constant node 60 of 66: the
# strided loops of a wave take a second pass and the constant node lies in the last full one).  Robot 5 cannot be it: it has one key
# frame, and the oracle's constant node is index1 of a sequential edge.
OTHER_FIXED = [0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0]


def test_solve_with_a_constant_node_that_is_not_node_zero(liw, synth, mods, pyoracle):
    """test_solve_against_the_oracle's assertions at its bars, for the two groups whose constant member is not their first one"""
    x0 = _x0_rows(liw, synth, mods)          # x0 = T_g_w * P does not depend on who is fixed
    cap = 20
    pg = liw.posegraph.office_pg_params()
    orc = _CACHE.setdefault("orc", pyoracle.Oracle(synth.office_params()))
    R = Rig(liw, synth, mods, pg=pg, fixed=OTHER_FIXED)
    R.solve(max_iters=cap)
    sm, rows = R.j.summaries(), R.rows()
    for g, cn, N, r0 in ((0, 8, 30, 1), (1, 60, 66, 4)):
        S = jc.structure(g, fixed=OTHER_FIXED)
        assert (S["const_node"], S["flags"]["nodes"], S["const_member"]) == (cn, N, r0)
        fl = R.j.flags(g)
        assert {k: fl[k] for k in FLAG_KEYS} == S["flags"], (g, fl, S["flags"])
        xo, so = jc.oracle_solve(pyoracle, orc, pg, g, max_iters=cap, fixed=OTHER_FIXED)
        s, x = sm[g], R.group_rows(g, rows)
        print("fixed robot %d (node %d of %d) group %d device %s\n%42s %s\n   |x - oracle| %.3e" % (r0, cn, N, g, s, "oracle", so, np.abs(x - xo).max()))
        assert (s["iterations"], s["successful"], s["termination"]) == (so["iterations"], so["successful"], so["termination"]), (g, s, so)
        assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-9 * so["initial_cost"], g
        assert abs(s["final_cost"] - so["final_cost"]) <= 1e-6 * max(1.0, so["final_cost"]), g
        assert np.abs(x - xo).max() <= 1e-6 * max(1.0, np.abs(xo).max()), g
        assert rows[r0, 0].tobytes() == x0[r0, 0].tobytes(), g                     # the constant node: bit for bit x0
        assert rows[r0, 1].tobytes() != x0[r0, 1].tobytes(), g                     # the node after it moved
        assert R.j.last_summary(g) == s
    R.close()


def test_a_single_member_equals_the_back_end(liw, synth, mods):
    """group C: robot 7 alone.  FleetBackEnd.solve of that robot in its own world, moved by T_g_w, is the same problem (the world is
    planar, so the ground factors agree)."""
    _, mk = lbc._lie()
    pg = dict(liw.posegraph.office_pg_params(), use_ground_q_factor=False)
    R = Rig(liw, synth, mods, pg=pg)
    R.solve(gsel=[0, 0, 1, 0, 0])
    x, sj = R.group_rows(2), R.j.summaries()[2]
    sel = np.zeros(jc.B, np.uint8)
    sel[7] = 1
    R.fb.solve(sel, np.zeros(jc.B), check_every=0)
    sb, pb = R.fb.summaries()[7], R.fb.keyframes(7)["poses"]
    T = gc.mat_of(R.al.T_g_w.cpu().numpy()[7])
    pose_of, _ = lbc._lie()
    want = np.array([pose_of(T @ mk(p)) for p in pb])
    print("group C: joint %s\n     back-end %s\n     |x - T_g_w * back-end| %.3e" % (sj, sb, np.abs(x - want).max()))
    assert sj["termination"] in (1, 2, 3) and sb["termination"] in (1, 2, 3)
    assert abs(sj["initial_cost"] - sb["initial_cost"]) <= 1e-9 * max(1.0, sb["initial_cost"])
    assert np.abs(x - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    R.close()


def test_nearer_the_truth_than_the_rigid_alignment(liw, synth, mods):
    _, mk = lbc._lie()
    R = Rig(liw, synth, mods)
    R.solve()
    rows, sj = R.rows(), R.j.summaries()
    R.g.solve()
    sg, T = R.g.summaries(), R.al.T_g_w.cpu().numpy()
    for g in (0, 1):
        joint = jc.position_errors(g, R.group_rows(g, rows))
        rigid = jc.rigid_errors(g, [gc.mat_of(t) for t in T])
        print("group %d: rigid (%s) worst %.4f sum %.4f | joint (%s) worst %.4f sum %.4f" % (g, sg[g]["termination"], rigid.max(), rigid.sum(), sj[g]["termination"],
                                                                                             joint.max(), joint.sum()))
        assert sg[g]["termination"] in (1, 2, 3) and sj[g]["termination"] in (1, 2, 3, 4)
        assert joint.max() < rigid.max() and joint.sum() < rigid.sum()
    R.close()


# --------------------------------------------------------------------------------------------------------------------- bit-identity
def _group_bytes(g, rows, hdr, tile=0):
    return b"".join(rows[r + jc.B * tile, :jc.NKF[r]].tobytes() for r in jc.structure(g)["members"]) + hdr[g + jc.G * tile].tobytes()


def test_bit_identity(liw, synth, mods):
    cap = 20
    rows0, hdr0, sm0 = _baseline(liw, synth, mods, cap)
    want = [_group_bytes(g, rows0, hdr0) for g in range(4)]
    R = Rig(liw, synth, mods)

    def run(gsel=None, **kw):
        R.j.poses().zero_()
        R.j.summary.zero_()
        R.solve(gsel=gsel, max_iters=cap, **kw)
        return R.rows(), R.j.header_bytes().cpu().numpy().copy(), R.j.summary.cpu().numpy().copy()
    rows, hdr, sm = run()                                                    # two runs
    assert [_group_bytes(g, rows, hdr) for g in range(4)] == want and sm.tobytes() == sm0.tobytes()
    for g in range(4):                                                       # solved alone
        rows, hdr, sm = run(gsel=[int(k == g) for k in range(jc.G)])
        assert _group_bytes(g, rows, hdr) == want[g] and sm[g].tobytes() == sm0[g].tobytes(), g
        assert not sm[[k for k in range(jc.G) if k != g]].any()
        assert not rows[[r for r in range(jc.B) if jc.GROUP_OF[r] != g]].any()
    for ce in (1, 4):                                                        # check_every
        rows, hdr, sm = run(check_every=ce)
        assert [_group_bytes(g, rows, hdr) for g in range(4)] == want and sm.tobytes() == sm0.tobytes(), ce
    R.j.set_lds_doubles(0)                                                   # every triangle from the work area
    rows, hdr, sm = run()
    assert [_group_bytes(g, rows, hdr) for g in range(4)] == want and sm.tobytes() == sm0.tobytes()
    with pytest.raises(liw.LiwError):
        R.j.set_lds_doubles(8193)
    R.close()


def test_bit_identity_in_32_tiles(liw, synth, mods):
    cap, tiles = 20, 32
    rows0, hdr0, sm0 = _baseline(liw, synth, mods, cap)
    Rt = Rig(liw, synth, mods, tiles=tiles)
    Rt.solve(max_iters=cap)
    rows, hdr, sm = Rt.rows(), Rt.j.header_bytes().cpu().numpy(), Rt.j.summary.cpu().numpy().reshape(tiles, jc.G, -1)
    for t in range(tiles):                                                   # at another group and robot index
        for g in range(4):
            assert _group_bytes(g, rows, hdr, tile=t) == _group_bytes(g, rows0, hdr0), (t, g)
        assert sm[t].tobytes() == sm0.tobytes(), t
    Rt.close()


def test_a_nan_group(liw, synth, mods):
    cap = 20
    rows0, hdr0, sm0 = _baseline(liw, synth, mods, cap)
    x0 = _x0_rows(liw, synth, mods)
    cross = {g: list(ls) for g, ls in jc.fleet()["cross"].items()}
    T = cross[0][0][5].copy()
    T[1, 1] = np.nan
    cross[0][0] = cross[0][0][:5] + (T,)
    R = Rig(liw, synth, mods, cross=cross)
    R.solve(max_iters=cap)
    rows, hdr, sm = R.rows(), R.j.header_bytes().cpu().numpy(), R.j.summaries()
    print("the NaN group ends with", sm[0])
    assert sm[0]["termination"] == 6 and sm[0]["successful"] == 0
    for r in jc.structure(0)["members"]:
        assert rows[r, :jc.NKF[r]].tobytes() == x0[r, :jc.NKF[r]].tobytes(), r
    for g in (1, 2, 3):
        assert _group_bytes(g, rows, hdr) == _group_bytes(g, rows0, hdr0), g
    assert R.j.summary.cpu().numpy()[1:].tobytes() == sm0[1:].tobytes()
    R.close()


def test_untouched_and_einval_writes_nothing(liw, synth, mods):
    import torch
    R = Rig(liw, synth, mods, guard=GUARD)
    R.j.poses().view(torch.uint8).fill_(0xC3)
    torch.cuda.synchronize()
    fb0, g0, T0 = R.fb._buf.clone(), R.g._buf.clone(), R.al.T_g_w.clone()
    R.solve(max_iters=20)
    rows = R.j.poses().view(torch.uint8).reshape(jc.B, jc.K, 48).cpu().numpy()
    assert torch.equal(R.fb._buf, fb0) and torch.equal(R.g._buf, g0) and torch.equal(R.al.T_g_w, T0)      # only read
    assert bool((R.j._buf[:GUARD] == 0xA5).all()) and bool((R.j._buf[-GUARD:] == 0xA5).all())
    for r in range(jc.B):
        member = jc.LINKED[r] and jc.GSEL[jc.GROUP_OF[r]]
        n = jc.NKF[r] if member else 0
        assert (rows[r, n:] == 0xC3).all(), r                    # rows beyond K_r, of the unlinked robot 12, of robot 11 (group E) and of robot 6
        assert n == 0 or not (rows[r, :n] == 0xC3).all(axis=1).any(), r
    snap = R.j._buf.clone()
    L, h, vp = R.j.L, R.j.h, lambda t: C.c_void_p(t.data_ptr())
    st, odd, a = vp(R.j.store), C.c_void_p(R.j.store.data_ptr() + 4), vp(R.al.T_g_w)
    calls = [L.liw_gjoint_solve(h, odd, a, a, a, a, a, a, a, 0, 0, a, None), L.liw_gjoint_solve(h, st, None, a, a, a, a, a, a, 0, 0, a, None),
             L.liw_gjoint_solve(h, st, a, odd, a, a, a, a, a, 0, 0, a, None), L.liw_gjoint_solve(h, st, a, a, a, a, a, a, None, 0, 0, a, None),
             L.liw_gjoint_solve(h, st, a, a, a, a, a, a, a, 0, 0, None, None), L.liw_gjoint_get_members(h, st, jc.G, 0, None, None),
             L.liw_gjoint_get_separators(h, st, -1, 0, None)]
    torch.cuda.synchronize()
    assert calls == [-22] * len(calls), calls
    assert torch.equal(R.j._buf, snap) and torch.equal(R.fb._buf, fb0) and torch.equal(R.g._buf, g0)
    R.close()


# --------------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_two_robots_one_room(liw, synth, mods):
    """The fixture of tests/test_gpu_group_graph.py's end-to-end case with FleetGroupJoint.push behind FleetGroupGraph.push: the joint
    push copies nothing to the host, the group grid drawn from joint.poses() equals the serial walk fed the read-back transforms, and it
    differs from the grid drawn from T_g_w * P."""
    import math
    import torch
    import loop_reference as lref
    gg, gj = mods
    prm = synth.office_params()
    rng = np.random.default_rng(5)
    pose_of, _ = lbc._lie()
    Tiw, Til = lbc.T_imu_to_wheel(), liw.loop.tf12_to_mat(mc.til12(liw, prm))
    Lm = tgl._landmarks(np.random.default_rng(900))
    room = mc._replay().replay_room()
    W = [xc._world(0, 21), xc._world(1, 21)]
    B, K, cap, n_rays = 2, 7, 8, 90
    bases = [xc._line(-2.0, 0.0, 0.0, K), xc._line(-0.8, -1.2, math.pi / 2, K)]
    fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=cap, max_points=64, max_kf_corners=32))
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=cap, max_loops=4), solve_period=1e308)
    fm = mc.mapper(liw, synth, B, cap, cap * n_rays, 1 << 19, 2048, prm=prm)
    gm = liw.FleetGroupMap(fm, 1, 1 << 21)
    al = liw.FleetGroupAligner(fl, [0, 0], [0], 9, xc.MAX_RMS)
    gr = gg.FleetGroupGraph(al, fb, 2, 16)
    jt = gj.FleetGroupJoint(gr, fb, 2 * cap, 2 * 4 + 16)      # every own loop and every held cross edge
    subs_of, frames = [[], []], []
    for t in range(K):
        items = []
        for r in range(B):
            Cn = tgl._seen(Lm, bases[r][t], r=2.5)
            Cn[:, :2] += rng.uniform(-xc.NOISE, xc.NOISE, (len(Cn), 2))
            items.append((pose_of(W[r] @ bases[r][t] @ lref.iso_inv(Tiw)), Cn @ W[r][:3, :3].T + W[r][:3, 3]))
            Tl = bases[r][t] @ lref.iso_inv(Tiw) @ Til
            subs_of[r].append(mc.scan(room, Tl[0, 3], Tl[1, 3], math.atan2(Tl[1, 0], Tl[0, 0]), n_rays, rng))
        frames.append(tlb._upload(torch, B, 48, items))
    stamps = torch.zeros(B, dtype=torch.float64, device="cuda")
    reads = []
    for nm in ("_sync", "summaries", "flags", "members", "nodes", "separators", "last_summary"):
        setattr(jt, nm, (lambda real, nm: lambda *a, **k: reads.append(nm) or real(*a, **k))(getattr(jt, nm), nm))
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item
    for t in range(K):
        loop_out = fl.push(frames[t])
        back_out = fb.push(dict(key=loop_out["added"], pose=frames[t]["pose"]), loop_out, stamps + t)
        fm.add_keyframes(*mc.frame(subs_of, t, n_rays))
        graph_out = gr.push(loop_out, back_out)
        torch.Tensor.cpu = lambda self, *a, **k: reads.append("cpu") or real_cpu(self, *a, **k)      # any device -> host copy inside the joint push
        torch.Tensor.item = lambda self, *a, **k: reads.append("item") or real_item(self, *a, **k)
        try:
            jt.push(graph_out)
        finally:
            torch.Tensor.cpu, torch.Tensor.item = real_cpu, real_item
    assert reads == []
    gm.render_all(fb, al.group_linked, al.T_g_w)
    assert gm.gstatus.cpu().numpy().tolist() == [0]
    rigid_grid, rigid_info = gm.grid(0).copy(), gm.info_of(0)
    gm.render(jt.poses(), al.group_linked)
    fl0, sm = jt.flags(0), jt.last_summary(0)
    print("end to end: joint graph %s, last solve %s" % (fl0, sm))
    assert (fl0["members"], fl0["nodes"], fl0["seq_edges"], fl0["solved"]) == (2, 2 * K, 2 * (K - 1), 1) and fl0["used"] >= 3 and fl0["skipped"] == 0
    assert sm["termination"] in (1, 2, 3, 4) and sm["successful"] >= 1 and sm["final_cost"] < sm["initial_cost"]
    assert gm.gstatus.cpu().numpy().tolist() == [0]
    rows = gm.infos()
    T_g_l = [fm.tf(b) for b in range(B)]
    want = mref.render(*mgc.concat(T_g_l, subs_of, [0, 1]), mc.RES)
    mgc.assert_group(gm, 0, want, rows[0])
    grid = gm.grid(0)
    moved = float(np.abs(jt.poses().cpu().numpy()[:, :K, :3] - np.array([[pose_of(gc.mat_of(t) @ lbc.make_tf(p))[:3] for p in fb.keyframes(b)["poses"]]
                                                                         for b, t in enumerate(al.T_g_w.cpu().numpy())])).max())
    print("end to end: the joint solve moved a key frame by up to %.4f m; grids %s vs %s" % (moved, grid.shape, rigid_grid.shape))
    assert grid.shape != rigid_grid.shape or int((grid != rigid_grid).sum()) > 0 or gm.info_of(0) != rigid_info
    for o in (jt, gr, gm, fm, fb, fl):
        o.close()
