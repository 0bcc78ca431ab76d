"""The group pose graph on the MI355X (include/liw_group_graph.h, group_graph.FleetGroupGraph) on the cases of
tests/group_graph_cases.py: the edge lists, counts and flags against the restatement over three add_edges calls; the partner rule;
Z bit-equal to liw_lie_mul / liw_lie_inverse of the device's own inputs; the solve against the oracle at the bars of
tests/test_gpu_posegraph_batch.py and, for the two-anchor group, against the truth; T_g_w after a back-end correction; isolation,
a NaN group among healthy ones, determinism, tiling and the work-area path; and the pipeline FleetLoopDetector.push ->
FleetBackEnd.push -> FleetGroupGraph.push -> FleetGroupMap.render_all end to end."""
import ctypes as C
import importlib

import numpy as np
import pytest

import group_graph_cases as gc
import loop_batch_cases as lbc
import loop_cross_cases as xc
import loop_reference as ref
import map_batch_cases as mc
import map_group_cases as mgc
import map_reference as mref
import test_gpu_loop as tgl
import test_gpu_loop_batch as tlb

pytestmark = pytest.mark.gpu
GUARD = 256
ULP_BAR = 4.0      # the bar of tests/test_gpu_loop_cross.py for a composed transform; 0 is expected
KCAP = 8           # max_keyframes of the back-end


@pytest.fixture(scope="module")
def gg(liw):
    return importlib.import_module(liw.__name__ + ".group_graph")


class Rig:
    """detector (for its handle only), back-end holding the cases' poses, aligner in the cases' state, and the group graph; `tiles` copies
    of the twelve robots (robot r of tile t is r + 12 t, its group g + 3 t)"""

    def __init__(self, liw, synth, gg, tiles=1, guard=0, group_of=None, linked=None, fixed=None, max_members=gc.MAX_MEMBERS, poses=None):
        import torch
        F = gc.fleet()
        self.liw, self.tiles, self.B = liw, tiles, gc.B * tiles
        B = self.B
        prm = synth.office_params()
        self.fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=KCAP, max_points=64, max_kf_corners=32))
        self.fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=KCAP, max_loops=1), solve_period=1e9)
        self.P = [list(p) for p in (F["P"] if poses is None else poses)]
        for r in range(B):
            self.load_poses(r, self.P[r % gc.B])
        go = gc.GROUP_OF if group_of is None else group_of
        lk = gc.LINKED if linked is None else linked
        fx = gc.FIXED if fixed is None else fixed
        self.group_of = [g + gc.G * t if g >= 0 else -1 for t in range(tiles) for g in go]
        self.linked, self.fixed = list(lk) * tiles, list(fx) * tiles
        self.al = liw.FleetGroupAligner(self.fl, self.group_of, {r: F["W"][r % gc.B] for r in range(B) if self.fixed[r]}, 9, xc.MAX_RMS)
        self.al.linked.copy_(torch.tensor(self.linked, dtype=torch.uint8))
        self.al.via[torch.tensor([bool(l and not f) for l, f in zip(self.linked, self.fixed)], device=self.al.dev)] = 0      # linked through an edge: no anchor
        self.set_T(F["T0"])
        self.g = gg.FleetGroupGraph(self.al, self.fb, max_members, gc.MAX_EDGES, groups=gc.G * tiles, guard=guard)

    def load_poses(self, r, poses):
        x = np.array(poses)
        eye = np.tile(gc.tf12_of(np.eye(4)), (max(len(x) - 1, 1), 1))
        self.fb.load_graph(r, dict(poses=x, seq_tf12=eye[:len(x) - 1], loop_idx=np.zeros((0, 2), np.int32), loop_tf12=np.zeros((0, 12))))

    def set_T(self, T):
        import torch
        self.al.T_g_w.copy_(torch.tensor(np.array([gc.tf12_of(T[r % gc.B]) for r in range(self.B)])))

    def feed(self, n_calls=3, calls=None):
        B0, out = gc.B, []
        for c in (gc.fleet()["calls"] if calls is None else calls)[:n_calls]:
            edge = np.tile(c["edge"], (self.tiles, 1))
            for t in range(self.tiles):
                b = edge[t * B0:(t + 1) * B0, 1]
                b[:] = np.where(b >= B0, self.B, np.where(b >= 0, b + B0 * t, b))       # an index outside the twelve stays outside the fleet
            self.g.add_edges(dict(found=np.tile(c["found"], self.tiles), edge=edge, tf12=np.tile(c["tf12"], (self.tiles, 1))), mask=np.tile(c["mask"], self.tiles))
        return self

    def T(self):
        return self.al.T_g_w.cpu().numpy().copy()

    def close(self):
        for o in (self.g, self.fb, self.fl):
            o.close()


def _lie(liw):
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def inv(A):
        A, out = np.ascontiguousarray(A, dtype=np.float64), np.zeros(12)
        L.liw_lie_inverse(pd(A), pd(out))
        return out
    return (lambda A, B: mgc.lie_mul(liw, A, B)), inv


_CACHE = {}


def _oracle(liw, synth, pyoracle, group, cap):
    """the oracle's solve of a group from the cases' start, computed once"""
    if (group, cap) not in _CACHE:
        Gr = gc.group_graph(group)
        orc = _CACHE.setdefault("orc", pyoracle.Oracle(synth.office_params()))
        _CACHE[group, cap] = gc.oracle_solve(pyoracle, orc, liw.posegraph.office_pg_params(), gc.start_x(Gr["nodes"]), Gr["edges"], Gr["const"].index(1), cap)
    return _CACHE[group, cap]


# --------------------------------------------------------------------------------------------------------------------- 1
def test_add_edges_equals_the_restatement(liw, synth, gg):
    import torch
    rigs = [Rig(liw, synth, gg, guard=GUARD) for _ in range(2)]
    for n in (1, 2, 3):
        for R in rigs:
            R.feed(calls=gc.fleet()["calls"][n - 1:n])
        want = gc.lists_after(n)
        R = rigs[0]
        for g in range(gc.G):
            idx, tf = R.g.edges(g)
            fl = R.g.flags(g)
            assert [tuple(e) for e in idx.tolist()] == want[g]["edges"], (n, g)
            assert tf.tobytes() == np.array(want[g]["tf12"]).reshape(-1, 12).tobytes(), (n, g)
            assert (fl["edges"], fl["edges_full"], fl["bad_edge"], fl["members_full"], fl["solves"]) == (len(want[g]["edges"]), want[g]["edges_full"], want[g]["bad_edge"], 0, 0), (n, g, fl)
        torch.cuda.synchronize()
        assert torch.equal(rigs[0].g._buf, rigs[1].g._buf)                           # two runs: equal bytes, the whole store
    R = rigs[0]
    assert bool((R.g._buf[:GUARD] == 0xA5).all()) and bool((R.g._buf[-GUARD:] == 0xA5).all())
    # reset of one group leaves the others as they are
    before = R.g.group_regions().clone()
    R.g.reset(gmask=[0, 0, 1])
    torch.cuda.synchronize()
    after = R.g.group_regions()
    assert torch.equal(after[:2], before[:2]) and not bool(after[2].any())
    for R in rigs:
        R.close()


# --------------------------------------------------------------------------------------------------------------------- 2
def test_partner_equals_the_restatement(liw, synth, gg):
    R = Rig(liw, synth, gg)
    for linked in (gc.LINKED, [0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0], [0] * 12):
        import torch
        R.al.linked.copy_(torch.tensor(linked, dtype=torch.uint8))
        for rnd in range(6):
            got = R.g.choose_partners(rnd).cpu().tolist()
            assert got == gc.choose_partners(gc.GROUP_OF, linked, rnd), (linked, rnd)
            old = R.al.choose_partners(rnd).cpu().tolist()                           # liw_xloop_partner
            assert [got[a] for a in range(12) if not linked[a]] == [old[a] for a in range(12) if not linked[a]]
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 3
def test_z_is_the_product_of_the_devices_own_inputs(liw, synth, gg):
    R = Rig(liw, synth, gg).feed()
    R.g.solve(max_iters=1)
    mul, inv = _lie(liw)
    _, mk = lbc._lie()
    worst_ulp, worst_tf, n_used = 0.0, 0.0, 0
    for g in range(gc.G):
        idx, tf = R.g.edges(g)
        z = R.g.get_Z(g)
        fl = R.g.flags(g)
        want = gc.group_graph(g)
        assert z["used"].tolist() == want["used"] and (fl["used"], fl["skipped"], fl["nodes"]) == (sum(want["used"]), len(want["used"]) - sum(want["used"]), len(want["nodes"]))
        for e, (a, q, b, i, size) in enumerate(idx.tolist()):
            if not z["used"][e]:
                continue
            n_used += 1
            prod = mul(mul(z["Ta"][e], tf[e]), inv(z["Tb"][e]))
            worst_ulp = max(worst_ulp, mc.ulps(z["Z"][e], prod))
            worst_tf = max(worst_tf, gc.deviation(gc.mat_of(z["Ta"][e]), mk(R.P[a][q])), gc.deviation(gc.mat_of(z["Tb"][e]), mk(R.P[b][i])),
                           gc.deviation(gc.mat_of(z["Z"][e]), gc.Z_of(R.P[a][q], tf[e], R.P[b][i])))
    print("Z: %d edges, worst distance from liw_lie_mul's product %.1f ulp; make_tf / Z from the host's %.3e" % (n_used, worst_ulp, worst_tf))
    assert n_used == 13 and worst_ulp <= ULP_BAR and worst_tf <= 1e-12
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("cap", (2, 5, 20, 0))     # 2: the cap ends every group (termination 4); the others end by a tolerance
def test_solve_against_the_oracle_and_the_truth(liw, synth, gg, pyoracle, cap):
    F = gc.fleet()
    pose_of, mk = lbc._lie()
    R = Rig(liw, synth, gg, guard=GUARD).feed()
    T0 = R.T()
    R.g.solve(max_iters=cap)
    sm, T = R.g.summaries(), R.T()
    for g in (0, 2):
        Gr = gc.group_graph(g)
        xo, so = _oracle(liw, synth, pyoracle, g, cap)
        s = sm[g]
        print("cap %d group %d device %s\n%22s %s" % (cap, g, s, "oracle", so))
        x = np.array([pose_of(gc.mat_of(T[r])) for r in Gr["nodes"]])
        print("   |x - oracle| %.3e" % np.abs(x - xo).max())
        assert (s["iterations"], s["successful"], s["termination"]) == (so["iterations"], so["successful"], so["termination"]), (g, s, so)
        assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-9 * so["initial_cost"], g
        assert abs(s["final_cost"] - so["final_cost"]) <= 1e-6 * max(1.0, so["final_cost"]), g
        assert np.abs(x - xo).max() <= 1e-6 * max(1.0, np.abs(xo).max()), g
        assert R.g.last_summary(g) == s and R.g.flags(g)["solves"] == 1
    # the two-anchor group, noise-free: the truth, and the anchors' rows untouched
    dev = max(gc.deviation(gc.mat_of(T[r]), F["W"][r]) for r in (4, 6))
    print("cap %d group 1 %s: max |T_g_w - truth| %.3e (start %.3e)" % (cap, sm[1], dev, max(gc.deviation(F["T0"][r], F["W"][r]) for r in (4, 6))))
    assert sm[1]["termination"] in ((4,) if cap == 2 else (1, 2, 3)), sm[1]
    if sm[1]["termination"] != 4:
        assert dev <= 1e-9, (sm[1], dev)
    for r in range(gc.B):
        if _never_written(r):
            assert T[r].tobytes() == T0[r].tobytes(), r
        elif gc.LINKED[r]:
            assert T[r].tobytes() != T0[r].tobytes(), r
    if cap == 2:
        assert [s["termination"] for s in sm] == [4, 4, 4] and [s["iterations"] for s in sm] == [2, 2, 2]
    assert bool((R.g._buf[:GUARD] == 0xA5).all()) and bool((R.g._buf[-GUARD:] == 0xA5).all())
    R.close()


def _never_written(r):
    """robots whose T_g_w a solve never writes: constant nodes and the unlinked robot"""
    return r in (0, 3, 5, 7, 11)


# --------------------------------------------------------------------------------------------------------------------- 5
def test_after_a_back_end_correction(liw, synth, gg):
    """robot 4's corrected poses move by a rigid D (its world frame is re-expressed): T_g_w[4] follows with D^-1 and T_g_w P stays"""
    pose_of, mk = lbc._lie()
    R = Rig(liw, synth, gg).feed()
    R.g.solve()
    T1 = R.T()
    D = np.eye(4)
    D[:3, :3] = ref._exp_so3(np.array([0.004, -0.003, 0.01]))          # the size of a back-end correction, and small enough for the bar of
    D[:3, 3] = (0.02, -0.015, 0.005)                                   # 1e-9 to be within reach of the parameter tolerance (group_graph_cases)
    P4 = [pose_of(D @ mk(p)) for p in R.P[4]]
    R.load_poses(4, P4)
    R.g.solve(gsel=[0, 1, 0])
    T2 = R.T()
    sm = R.g.summaries()[1]
    d_T = gc.deviation(gc.mat_of(T2[4]), gc.mat_of(T1[4]) @ ref.iso_inv(D))
    d_P = max(gc.deviation(gc.mat_of(T2[4]) @ mk(p2), gc.mat_of(T1[4]) @ mk(p1)) for p1, p2 in zip(R.P[4], P4))
    print("after the correction: %s; |T_g_w - T_g_w D^-1| %.3e, |T_g_w P| moved by %.3e; the stale T_g_w would move it by %.3e"
          % (sm, d_T, d_P, max(gc.deviation(gc.mat_of(T1[4]) @ mk(p2), gc.mat_of(T1[4]) @ mk(p1)) for p1, p2 in zip(R.P[4], P4))))
    assert sm["termination"] in (1, 2, 3) and sm["successful"] >= 1
    assert d_T <= 1e-9 and d_P <= 1e-9
    for r in range(gc.B):
        if r not in (4, 6):
            assert T2[r].tobytes() == T1[r].tobytes(), r          # the other groups were not selected, the anchors are constant
    assert R.g.flags(1)["solves"] == 2 and R.g.flags(0)["solves"] == 1
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 6
def test_isolation_and_determinism(liw, synth, gg):
    import torch
    cap = 20
    R = Rig(liw, synth, gg).feed()
    T0 = R.T()
    R.g.solve(max_iters=cap)
    want_T, want_sm = R.T(), R.g.summary.cpu().numpy().copy()
    # unselected groups: nothing of theirs is written; a group solved alone gives the bytes it gives among the others
    for g in range(gc.G):
        R.set_T(gc.fleet()["T0"])
        R.g.summary.zero_()
        R.g.solve(gsel=[int(k == g) for k in range(gc.G)], max_iters=cap)
        T, sm = R.T(), R.g.summary.cpu().numpy()
        for r in range(gc.B):
            assert T[r].tobytes() == (want_T[r] if gc.GROUP_OF[r] == g else T0[r]).tobytes(), (g, r)
        assert sm[g].tobytes() == want_sm[g].tobytes() and not sm[[k for k in range(gc.G) if k != g]].any()
    # every triangle from the work area instead of LDS: the same bytes
    R.set_T(gc.fleet()["T0"])
    R.g.set_lds_doubles(0)
    R.g.solve(max_iters=cap)
    assert R.T().tobytes() == want_T.tobytes() and R.g.summary.cpu().numpy().tobytes() == want_sm.tobytes()
    with pytest.raises(liw.LiwError):
        R.g.set_lds_doubles(8193)
    R.close()
    # 32 tiled copies: every tile gives what the twelve give, at other group and robot indices; two runs are equal
    tiles, runs = 32, []
    for _ in range(2):
        Rt = Rig(liw, synth, gg, tiles=tiles).feed()
        Rt.g.solve(max_iters=cap)
        torch.cuda.synchronize()
        runs.append((Rt.al.T_g_w.clone(), Rt.g.summary.clone(), Rt.g.group_regions().clone()))
        Rt.close()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    Tt, St = runs[0][0].cpu().numpy().reshape(tiles, gc.B, 12), runs[0][1].cpu().numpy().reshape(tiles, gc.G, -1)
    for t in range(tiles):
        assert Tt[t].tobytes() == want_T.tobytes() and St[t].tobytes() == want_sm.tobytes(), t


def test_a_nan_group_and_a_group_over_max_members(liw, synth, gg):
    cap = 20
    R = Rig(liw, synth, gg).feed()
    T0 = R.T()
    R.g.solve(max_iters=cap)
    want_T, want_sm = R.T(), R.g.summaries()
    R.close()
    calls = [dict(c, tf12=c["tf12"].copy()) for c in gc.fleet()["calls"]]
    calls[0]["tf12"][8, 4] = np.nan                              # the edge 8 -> 9 of group 2
    R = Rig(liw, synth, gg).feed(calls=calls)
    R.g.solve(max_iters=cap)
    T, sm = R.T(), R.g.summaries()
    print("the NaN group ends with", sm[2])
    assert sm[2]["termination"] == 6 and sm[2]["successful"] == 0 and R.g.flags(2)["solves"] == 1
    for r in range(gc.B):
        assert T[r].tobytes() == (T0[r] if gc.GROUP_OF[r] == 2 else want_T[r]).tobytes(), r
    assert sm[:2] == want_sm[:2]
    R.close()
    # seven linked members where a solve holds six: members_full, and nothing is solved
    go, lk = [0] * 7 + [1] * 5, [1] * 7 + [0] * 5
    R = Rig(liw, synth, gg, group_of=go, linked=lk, fixed=[0] * 12)
    found, edge = np.zeros(12, np.uint8), np.zeros((12, 4), np.int32)
    found[:2], edge[0], edge[1] = 1, (0, 1, 0, 9), (0, 2, 0, 9)
    R.g.add_edges(dict(found=found, edge=edge, tf12=np.tile(gc.tf12_of(np.eye(4)), (12, 1))))
    T0 = R.T()
    R.g.solve()
    fl = R.g.flags(0)
    assert (fl["edges"], fl["members_full"], fl["solves"]) == (2, 1, 0) and R.T().tobytes() == T0.tobytes()
    R.close()
    R = Rig(liw, synth, gg, group_of=go, linked=lk, fixed=[0] * 12, max_members=7)
    R.g.add_edges(dict(found=found, edge=edge, tf12=np.tile(gc.tf12_of(np.eye(4)), (12, 1))))
    R.g.solve()
    fl = R.g.flags(0)
    assert (fl["members_full"], fl["solves"], fl["nodes"], fl["used"]) == (0, 1, 7, 2)
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 6b
@pytest.mark.parametrize("M", (21, 22))
def test_a_group_at_and_beyond_the_lds_limit(liw, synth, gg, M):
    """One group of M linked robots, a cycle with a ring of chords, noise-free, robot 0 the anchor.  M = 21: the triangle (8 001 doubles) is
    the largest that runs from LDS, and gives the bytes it gives from the work area.  M = 22 (8 778 doubles): a store whose groups can
    only run from the work area.  Bar against the truth: the parameter tolerance leaves at most 1e-8 |x| of the way (group_graph_cases),
    |x| < 50 here (21 free nodes within 4 m and 2.5 rad), so 1e-6."""
    import torch
    pose_of, mk = lbc._lie()
    rng = np.random.default_rng(M)
    W = [gc._frame(rng, 4.0) for _ in range(M)]
    P = [pose_of(gc._frame(rng, 3.0)) for _ in range(M)]
    T0 = [W[0]] + [W[r] @ gc._small(rng, gc.START_P, gc.START_Q) for r in range(1, M)]
    assert gg.layout(dict(B=M, G=1, max_members=M, max_edges=2 * M))["tri_doubles"] == (8001 if M == 21 else 8778)
    prm = synth.office_params()
    fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=M, max_keyframes=2, max_points=16, max_kf_corners=8))
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=M, max_keyframes=2, max_loops=1), solve_period=1e9)
    for r in range(M):
        fb.load_graph(r, dict(poses=np.array([P[r]]), seq_tf12=np.zeros((0, 12)), loop_idx=np.zeros((0, 2), np.int32), loop_tf12=np.zeros((0, 12))))
    al = liw.FleetGroupAligner(fl, [0] * M, {0: W[0]}, 9, xc.MAX_RMS)
    al.linked.fill_(1)
    al.via[1:] = 0
    g = gg.FleetGroupGraph(al, fb, M, 2 * M, guard=GUARD)
    for ring in (1, 2):
        edge, tf12 = np.zeros((M, 4), np.int32), np.zeros((M, 12))
        for a in range(M):
            b = (a + ring) % M
            edge[a], tf12[a] = (0, b, 0, 20), gc.tf12_of(ref.iso_inv(mk(P[a])) @ ref.iso_inv(W[a]) @ W[b] @ mk(P[b]))
        g.add_edges(dict(found=np.ones(M, np.uint8), edge=edge, tf12=tf12))
    start = torch.tensor(np.array([gc.tf12_of(T) for T in T0]), device="cuda")
    outs = []
    for lds in ((8192, 0) if M == 21 else (8192,)):
        al.T_g_w.copy_(start)
        g.set_lds_doubles(lds)
        g.solve()
        outs.append((al.T_g_w.cpu().numpy().copy(), g.summaries()[0]))
    T, sm = outs[0]
    fl0 = g.flags(0)
    dev = max(gc.deviation(gc.mat_of(T[r]), W[r]) for r in range(M))
    print("M = %d: %s, max |T_g_w - truth| %.3e" % (M, sm, dev))
    assert (fl0["nodes"], fl0["used"], fl0["skipped"], fl0["members_full"], fl0["solves"]) == (M, 2 * M, 0, 0, len(outs))
    assert sm["termination"] in (1, 2, 3) and sm["successful"] >= 2 and dev <= 1e-6
    assert T[0].tobytes() == gc.tf12_of(W[0]).tobytes()
    if M == 21:
        assert outs[1][0].tobytes() == T.tobytes() and outs[1][1] == sm
    assert bool((g._buf[:GUARD] == 0xA5).all()) and bool((g._buf[-GUARD:] == 0xA5).all())
    for o in (g, fb, fl):
        o.close()


def test_einval_writes_nothing(liw, synth, gg):
    import torch
    R = Rig(liw, synth, gg, guard=GUARD).feed()
    R.g.solve(max_iters=3)
    torch.cuda.synchronize()
    snap, Tsnap = R.g._buf.clone(), R.al.T_g_w.clone()
    L, h, vp = R.g.L, R.g.h, lambda t: C.c_void_p(t.data_ptr())
    st, odd, a = vp(R.g.store), C.c_void_p(R.g.store.data_ptr() + 4), vp(R.al.T_g_w)
    calls = [L.liw_ggraph_reset(h, odd, None, None), L.liw_ggraph_add_edges(h, odd, a, a, a, a, None, None), L.liw_ggraph_add_edges(h, st, a, None, a, a, None, None),
             L.liw_ggraph_partner(h, a, a, -1, a, None), L.liw_ggraph_solve(h, st, a, 6, a, a, a, a, None, a, 0, a, None),
             L.liw_ggraph_solve(h, odd, a, 6, a, a, a, a, a, a, 0, a, None), L.liw_ggraph_solve(h, st, a, -6, a, a, a, a, a, a, 0, a, None),
             L.liw_ggraph_get_edges(h, st, gc.G, 0, None, None), L.liw_ggraph_get_Z(h, st, -1, 0, None, None, None, None)]
    torch.cuda.synchronize()
    assert calls == [-22] * len(calls), calls
    assert torch.equal(R.g._buf, snap) and torch.equal(R.al.T_g_w, Tsnap)
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 7
def test_end_to_end_two_robots_one_room(liw, synth, gg):
    """The fixture of tests/test_gpu_loop_cross.py's end-to-end case through FleetLoopDetector.push -> FleetBackEnd.push ->
    FleetGroupGraph.push -> FleetGroupMap.render_all: robot 1 links to the anchor, both robots go on producing edges, the group is
    solved whenever it gains one, FleetGroupGraph.push copies nothing to the host, and the group grid equals the serial walk fed the
    read-back T_g_w * T_w_l."""
    import math
    import torch
    import loop_reference as lref
    prm = synth.office_params()
    rng = np.random.default_rng(5)
    pose_of, _ = lbc._lie()
    Tiw, Til = lbc.T_imu_to_wheel(), liw.loop.tf12_to_mat(mc.til12(liw, prm))
    Lm = tgl._landmarks(np.random.default_rng(900))
    room = mc._replay().replay_room()
    W = [xc._world(0, 21), xc._world(1, 21)]
    B, K, cap, n_rays = 2, 7, 8, 90          # two frames more than that case: both robots are linked by then and go on producing edges
    bases = [xc._line(-2.0, 0.0, 0.0, K), xc._line(-0.8, -1.2, math.pi / 2, K)]       # robot 1 crosses robot 0's path at its fifth key frame
    fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=cap, max_points=64, max_kf_corners=32))
    # solve_period beyond any stamp: the back-end never solves here, so the corrected poses stay the tracking poses and W_0 W_1^-1 stays the
    # truth of T_g_w[1] (T_g_w after a back-end correction is test_after_a_back_end_correction's subject)
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=cap, max_loops=4), solve_period=1e308)
    fm = mc.mapper(liw, synth, B, cap, cap * n_rays, 1 << 19, 2048, prm=prm)
    gm = liw.FleetGroupMap(fm, 1, 1 << 21)
    al = liw.FleetGroupAligner(fl, [0, 0], [0], 9, xc.MAX_RMS)
    gr = gg.FleetGroupGraph(al, fb, 2, 16)
    subs_of, frames = [[], []], []
    for t in range(K):
        items = []
        for r in range(B):
            Cn = tgl._seen(Lm, bases[r][t], r=2.5)
            Cn[:, :2] += rng.uniform(-xc.NOISE, xc.NOISE, (len(Cn), 2))
            items.append((pose_of(W[r] @ bases[r][t] @ lref.iso_inv(Tiw)), Cn @ W[r][:3, :3].T + W[r][:3, 3]))
            Tl = bases[r][t] @ lref.iso_inv(Tiw) @ Til                               # the laser in the room
            subs_of[r].append(mc.scan(room, Tl[0, 3], Tl[1, 3], math.atan2(Tl[1, 0], Tl[0, 0]), n_rays, rng))
        frames.append(tlb._upload(torch, B, 48, items))
    stamps = torch.zeros(B, dtype=torch.float64, device="cuda")
    reads = []
    for o, names in ((gm, ("_sync", "infos", "info_of", "grid", "members")), (fm, ("_sync", "infos", "tf", "info_of", "grid")), (fl, ("_sync",)),
                     (fb, ("_sync", "_read_n_due")), (gr, ("_sync", "summaries", "flags", "edges"))):
        for nm in names:
            setattr(o, nm, (lambda real, nm: lambda *a, **k: reads.append(nm) or real(*a, **k))(getattr(o, nm), nm))
    in_push = 0
    for t in range(K):
        loop_out = fl.push(frames[t])
        back_out = fb.push(dict(key=loop_out["added"], pose=frames[t]["pose"]), loop_out, stamps + t)
        fm.add_keyframes(*mc.frame(subs_of, t, n_rays))
        n = len(reads)
        gr.push(loop_out, back_out)
        in_push += len(reads) - n
    n = len(reads)
    gm.render_all(fb, al.group_linked, al.T_g_w)
    assert in_push == 0 and len(reads) == n and set(reads) <= {"_read_n_due"}          # the back-end's own 4-byte read is the only one of a frame
    assert al.linked.cpu().tolist() == [1, 1] and al.group_linked.cpu().tolist() == [0, 0] and int(al.via[1, 0]) == 0
    fl0 = gr.flags(0)
    edges, _ = gr.edges(0)
    print("end to end: group 0 holds %d edges %s, %d solves, last %s" % (fl0["edges"], edges[:, [0, 2]].tolist(), fl0["solves"], gr.last_summary(0)))
    # robot 1 links through its own edge, and from then on the linked robots 0 and 1 both go on producing edges, each gain followed by a solve
    assert fl0["edges"] >= 3 and fl0["solves"] >= 2 and fl0["bad_edge"] == 0 and fl0["used"] == fl0["edges"] and {0, 1} <= set(edges[:, 0].tolist())
    assert gr.last_summary(0)["termination"] in (1, 2, 3)
    Tg = al.T_g_w.cpu().numpy()
    assert np.array_equal(liw.loop.tf12_to_mat(Tg[0]), np.eye(4))
    dev, solved = float(np.abs(liw.loop.tf12_to_mat(Tg[1]) - W[0] @ lref.iso_inv(W[1])).max()), [fb.flags(b)["solves"] for b in range(B)]
    print("end to end: |T_g_w[1] - W_0 W_1^-1| %.3e, back-end solves %s" % (dev, solved))
    assert solved == [0, 0] and dev < 0.02
    status, rows = gm.gstatus.cpu().numpy(), gm.infos()
    assert status.tolist() == [0]
    T_g_l = [fm.tf(b) for b in range(B)]
    want = mref.render(*mgc.concat(T_g_l, subs_of, [0, 1]), mc.RES)
    mgc.assert_group(gm, 0, want, rows[0])
    for o in (fl, fb, fm, gm, gr):
        o.close()
