"""The group edge gate on the MI355X (include/liw_group_gate.h, FleetGroupGraph.gate / solve_gated / edge_states) on the cases of
tests/group_gate_cases.py: solve -> gate -> states -> solve(changed) driven by hand and compared with the restatement after every step
(state, rejected, changed, used, skipped equal; chi2 against the host's value from the device's own Z and T_g_w; T_g_w, iteration counts
and terminations against the oracle at the bars of tests/test_gpu_group_graph.py), a second gate after one solve, a NaN group, an
unselected group, duplicates of a rejected edge, reset, solve_gated on consistent edges and on the fleet of group_graph_cases, min_support
1, guard bytes on LIW_EINVAL, determinism / tiling / the work-area path, and push() without a read-back."""
import ctypes as C
import importlib

import numpy as np
import pytest

import group_gate_cases as cs
import group_graph_cases as gc
import loop_batch_cases as lbc
import loop_cross_cases as xc
import test_gpu_loop as tgl

pytestmark = pytest.mark.gpu
GUARD = 256
KCAP = 8           # max_keyframes of the back-end


@pytest.fixture(scope="module")
def gg(liw):
    return importlib.import_module(liw.__name__ + ".group_graph")


class Rig:
    """tests/test_gpu_group_graph.py's Rig over a cases module `cm` (group_gate_cases or group_graph_cases): detector (for its handle only),
    back-end holding the cases' poses, aligner in the cases' state, and the group graph; `tiles` copies of the fleet (robot r of tile t is
    r + B t, its group g + G t); kw goes to FleetGroupGraph"""

    def __init__(self, liw, synth, gg, cm=cs, tiles=1, guard=0, **kw):
        import torch
        F = cm.fleet()
        self.cm, self.tiles, self.B = cm, tiles, cm.B * tiles
        B = self.B
        prm = synth.office_params()
        self.fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=KCAP, max_points=64, max_kf_corners=32))
        self.fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=KCAP, max_loops=1), solve_period=1e9)
        for r in range(B):
            x = np.array(F["P"][r % cm.B])
            eye = np.tile(gc.tf12_of(np.eye(4)), (max(len(x) - 1, 1), 1))
            self.fb.load_graph(r, dict(poses=x, seq_tf12=eye[:len(x) - 1], loop_idx=np.zeros((0, 2), np.int32), loop_tf12=np.zeros((0, 12))))
        self.group_of = [g + cm.G * t if g >= 0 else -1 for t in range(tiles) for g in cm.GROUP_OF]
        self.linked, self.fixed = list(cm.LINKED) * tiles, list(cm.FIXED) * tiles
        self.al = liw.FleetGroupAligner(self.fl, self.group_of, {r: F["W"][r % cm.B] for r in range(B) if self.fixed[r]}, 9, xc.MAX_RMS)
        self.al.linked.copy_(torch.tensor(self.linked, dtype=torch.uint8))
        self.al.via[torch.tensor([bool(l and not f) for l, f in zip(self.linked, self.fixed)], device=self.al.dev)] = 0      # linked through an edge: no anchor
        self.set_T(F["T0"])
        self.g = gg.FleetGroupGraph(self.al, self.fb, cm.MAX_MEMBERS, cm.MAX_EDGES, groups=cm.G * tiles, guard=guard, **kw)

    def set_T(self, T):
        import torch
        self.al.T_g_w.copy_(torch.tensor(np.array([gc.tf12_of(T[r % self.cm.B]) for r in range(self.B)])))

    def call(self, c):
        """the arguments of add_edges for one call of the cases, tiled"""
        B0 = self.cm.B
        edge = np.tile(c["edge"], (self.tiles, 1))
        for t in range(self.tiles):
            b = edge[t * B0:(t + 1) * B0, 1]
            b[:] = np.where(b >= B0, self.B, np.where(b >= 0, b + B0 * t, b))
        return dict(found=np.tile(c["found"], self.tiles), edge=edge, tf12=np.tile(c["tf12"], (self.tiles, 1))), np.tile(c["mask"], self.tiles)

    def feed(self, calls=None):
        for c in (self.cm.fleet()["calls"] if calls is None else calls):
            out, mask = self.call(c)
            self.g.add_edges(out, mask=mask)
        return self

    def T(self):
        return self.al.T_g_w.cpu().numpy().copy()

    def close(self):
        for o in (self.g, self.fb, self.fl):
            o.close()


_CACHE = {}


def _orc(synth, pyoracle):
    return _CACHE.setdefault("orc", pyoracle.Oracle(synth.office_params()))


def _run(liw, synth, pyoracle, group, min_support=cs.MIN_SUPPORT):
    """the restated loop of a group, computed once"""
    if (group, min_support) not in _CACHE:
        _CACHE[group, min_support] = cs.run(pyoracle, _orc(synth, pyoracle), liw.posegraph.office_pg_params(), group, min_support=min_support)
    return _CACHE[group, min_support]


def _nodes(group):
    return [r for r in range(cs.B) if cs.GROUP_OF[r] == group]


def _check_solve(R, group, step, T, sm, n_solves):
    """a solve step against the oracle at the bars of test_solve_against_the_oracle_and_the_truth"""
    pose_of, _ = lbc._lie()
    xo, so = step["x"], step["summary"]
    x = np.array([pose_of(gc.mat_of(T[r])) for r in _nodes(group)])
    print("group %s solve %d: device %s\n%29s %s\n   |x - oracle| %.3e" % (cs.NAMES[group], n_solves, sm, "oracle", so, np.abs(x - xo).max()))
    assert (sm["iterations"], sm["successful"], sm["termination"]) == (so["iterations"], so["successful"], so["termination"]), (group, sm, so)
    assert abs(sm["initial_cost"] - so["initial_cost"]) <= 1e-9 * so["initial_cost"], group
    assert abs(sm["final_cost"] - so["final_cost"]) <= 1e-6 * max(1.0, so["final_cost"]), group
    assert np.abs(x - xo).max() <= 1e-6 * max(1.0, np.abs(xo).max()), group
    fl = R.g.flags(group)
    assert (fl["used"], fl["skipped"], fl["solves"]) == (sum(step["used"]), step["skipped"], n_solves), (group, fl)
    assert R.g.get_Z(group)["used"].tolist() == step["used"], group


def _check_gate(R, liw, synth, pyoracle, group, step, changed, T, before):
    """a gate step against the restatement; chi2 of the edges of the last solve against the host's value from the device's Z and T_g_w"""
    pose_of, _ = lbc._lie()
    st, z = R.g.edge_states(group), R.g.get_Z(group)
    assert st["state"].tolist() == step["state"] and st["rejected"] == step["rejected"] and int(changed[group]) == step["changed"], (group, st, step)
    assert st["gated_solves"] == R.g.flags(group)["solves"]
    nodes = _nodes(group)
    idx, _ = R.g.edges(group)
    worst = 0.0
    for e, (a, q, b, i, size) in enumerate(idx.tolist()):
        if z["used"][e]:
            want = cs.chi2_of(pyoracle, _orc(synth, pyoracle), liw.posegraph.office_pg_params(), pose_of(gc.mat_of(T[a])), pose_of(gc.mat_of(T[b])), gc.mat_of(z["Z"][e]))
            worst = max(worst, abs(st["chi2"][e] - want) / want)
        else:
            assert st["chi2"][e] == before["chi2"][e], (group, e)                                              # not part of the solve: as it was
    print("group %s gate: rejected %s, chi2 %s, worst relative distance from the host's %.2e" % (cs.NAMES[group], step["reject"], ["%.4g" % c for c in st["chi2"]], worst))
    assert worst <= 1e-9, (group, worst)
    assert nodes == sorted(nodes)


# --------------------------------------------------------------------------------------------------------------------- 1
def test_the_loop_by_hand_equals_the_restatement(liw, synth, gg, pyoracle):
    import torch
    F = cs.fleet()
    R = Rig(liw, synth, gg, guard=GUARD, chi2_max=cs.CHI2_MAX, min_support=cs.MIN_SUPPORT).feed()
    runs = [_run(liw, synth, pyoracle, g) for g in range(cs.G)]
    for g in range(cs.G):
        st = R.g.edge_states(g)
        assert not st["state"].any() and not st["chi2"].any() and (st["rejected"], st["gated_solves"]) == (0, 0)
    n_solves = [0] * cs.G
    sel = None
    for k in range(1 + cs.GATE_ROUNDS):
        R.g.solve(sel)
        T, sm = R.T(), R.g.summaries()
        for g in range(cs.G):
            step = runs[g][2 * k]
            if step is not None:
                n_solves[g] += 1
                _check_solve(R, g, step, T, sm[g], n_solves[g])
            else:
                assert R.g.flags(g)["solves"] == n_solves[g]
        if k == cs.GATE_ROUNDS:
            break
        before = [R.g.edge_states(g) for g in range(cs.G)]
        sel = R.g.gate(sel).clone()
        changed = sel.cpu().numpy()
        for g in range(cs.G):
            _check_gate(R, liw, synth, pyoracle, g, runs[g][2 * k + 1], changed, T, before[g])
        # a second gate after the same solve: changed = 0 and not a byte of the store moves
        torch.cuda.synchronize()
        snap = R.g._buf.clone()
        again = R.g.gate().cpu().numpy()
        torch.cuda.synchronize()
        assert not again.any() and torch.equal(R.g._buf, snap)
    assert [R.g.edge_states(g)["state"].nonzero()[0].tolist() for g in range(cs.G)] == [sorted(cs.EXPECT[g]) for g in range(cs.G)]
    for g in (0, 1):      # the worth of it: the groups with wrong edges end at the truth up to the edge noise
        dev = max(gc.deviation(gc.mat_of(T[r]), F["W"][r]) for r in _nodes(g))
        print("group %s: max |T_g_w - truth| %.3e" % (cs.NAMES[g], dev))
        assert dev < 5e-3, (g, dev)
    assert bool((R.g._buf[:GUARD] == 0xA5).all()) and bool((R.g._buf[-GUARD:] == 0xA5).all())
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 2
def test_groups_the_gate_leaves_alone_duplicates_and_reset(liw, synth, gg):
    import torch
    calls = [dict(c, tf12=c["tf12"].copy()) for c in cs.fleet()["calls"]]
    calls[0]["tf12"][7, 4] = np.nan                              # the edge 7 -> 8 of group D: robot 9 keeps a finite gradient, so the solve goes on
    R = Rig(liw, synth, gg, chi2_max=cs.CHI2_MAX).feed(calls=calls)
    R.g.solve()
    assert R.g.summaries()[3]["termination"] == 6
    torch.cuda.synchronize()
    before = R.g.group_regions().clone()
    changed = R.g.gate([1, 0, 1, 1]).cpu().numpy()
    torch.cuda.synchronize()
    after = R.g.group_regions()
    assert changed.tolist() == [1, 0, 1, 0]
    assert torch.equal(after[1], before[1]) and torch.equal(after[3], before[3])          # the unselected group and the failed one: byte-identical
    assert not torch.equal(after[0], before[0]) and R.g.edge_states(3)["gated_solves"] == 0
    stA = R.g.edge_states(0)
    assert stA["state"].tolist() == [1, 0, 0, 0] and stA["rejected"] == 1
    # the rejected edge comes again: still a duplicate
    out, mask = R.call(calls[0])
    R.g.add_edges(out, mask=mask)
    assert [R.g.flags(g)["edges"] for g in range(cs.G)] == [4, 5, 7, 8] and R.g.edge_states(0)["state"].tolist() == [1, 0, 0, 0]
    # group B was not gated: it still can be; group A was
    changed = R.g.gate().cpu().numpy()
    assert changed.tolist() == [0, 1, 0, 0] and R.g.edge_states(1)["state"].tolist() == [1, 0, 0, 0, 0]
    # reset clears the states and the counts
    R.g.reset(gmask=[1, 0, 0, 0])
    torch.cuda.synchronize()
    assert not bool(R.g.group_regions()[0].any())
    st = R.g.edge_states(0)
    assert len(st["state"]) == 0 and (st["rejected"], st["gated_solves"]) == (0, 0) and R.g.edge_states(1)["rejected"] == 1
    R.g.add_edges(out, mask=mask)
    st = R.g.edge_states(0)
    assert st["state"].tolist() == [0] and st["chi2"].tolist() == [0.0]                     # the first edge again, active
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 3
def test_solve_gated(liw, synth, gg, pyoracle):
    import torch
    # by hand, as the reference of solve_gated
    R = Rig(liw, synth, gg, chi2_max=cs.CHI2_MAX).feed()
    R.g.solve()
    T_plain = R.T()
    sel = None
    for _ in range(cs.GATE_ROUNDS):
        sel = R.g.gate(sel)
        R.g.solve(sel)
    torch.cuda.synchronize()
    want_T, want_regions = R.T(), R.g.group_regions().clone().cpu()
    R.close()
    outs = {}
    for name, kw, lds, tiles in (("run 1", {}, None, 1), ("run 2", {}, None, 1), ("work area", {}, 0, 1), ("one round", dict(gate_rounds=1), None, 1),
                                 ("tiled", {}, None, 32)):
        R = Rig(liw, synth, gg, tiles=tiles, chi2_max=cs.CHI2_MAX, **kw).feed()
        if lds is not None:
            R.g.set_lds_doubles(lds)
        R.g.solve_gated()
        torch.cuda.synchronize()
        outs[name] = (R.T(), R.g.group_regions().clone().cpu(), [R.g.edge_states(g)["state"].tolist() for g in range(cs.G)])
        R.close()
    for name in ("run 1", "run 2", "work area"):
        assert outs[name][0].tobytes() == want_T.tobytes() and torch.equal(outs[name][1], want_regions), name
    assert [np.flatnonzero(s).tolist() for s in outs["run 1"][2]] == [sorted(cs.EXPECT[g]) for g in range(cs.G)]
    # group D, all consistent: the bytes of the plain solve
    for r in (7, 8, 9):
        assert outs["run 1"][0][r].tobytes() == T_plain[r].tobytes(), r
    # gate_rounds = 1: one of group B's two wrong edges
    assert [np.flatnonzero(s).tolist() for s in outs["one round"][2]] == [[0], [0], [3], []]
    # 32 tiled copies: every tile gives what the ten give, at other group and robot indices
    Tt, Rt = outs["tiled"][0].reshape(32, cs.B, 12), outs["tiled"][1].reshape(32, cs.G, -1)
    assert tuple(Rt.shape[1:]) == tuple(want_regions.shape)
    for t in range(32):
        assert Tt[t].tobytes() == want_T.tobytes(), t
    # the regions hold robot indices (a and b of every record), which move with the tile; everything else is equal
    held = np.array([[e < n for e in range(cs.MAX_EDGES)] for n in (4, 5, 7, 8)], dtype=np.int32)
    lo, hi = 256, 256 + 128 * cs.MAX_EDGES
    for t in range(32):
        reg = Rt[t].numpy().copy()
        recs = reg[:, lo:hi].reshape(cs.G, cs.MAX_EDGES, 128).copy()
        words = recs[:, :, :16].copy().view(np.int32)                      # a, q, b, i
        words[:, :, 0] -= cs.B * t * held
        words[:, :, 2] -= cs.B * t * held
        recs[:, :, :16] = words.view(np.uint8)
        reg[:, lo:hi] = recs.reshape(cs.G, -1)
        assert reg.tobytes() == want_regions.numpy().tobytes(), t


def test_min_support_one_on_group_a_alone(liw, synth, gg):
    R = Rig(liw, synth, gg, chi2_max=cs.CHI2_MAX, min_support=1).feed()
    R.g.solve_gated([1, 0, 0, 0])
    assert [R.g.edge_states(g)["state"].tolist() for g in range(cs.G)] == [[1, 0, 0, 0], [0] * 5, [0] * 7, [0] * 8]
    assert [R.g.flags(g)["solves"] for g in range(cs.G)] == [2, 0, 0, 0] and R.g.edge_states(0)["rejected"] == 1
    R.close()


def test_the_fleet_of_the_group_graph_cases_is_untouched(liw, synth, gg):
    """nothing there is inconsistent: under chi2_max T_g_w has the bytes of the run without it"""
    outs = []
    for kw in ({}, dict(chi2_max=cs.CHI2_MAX)):
        R = Rig(liw, synth, gg, cm=gc, **kw).feed()
        if kw:
            R.g.solve_gated(max_iters=20)
            assert not any(R.g.edge_states(g)["state"].any() or R.g.edge_states(g)["rejected"] for g in range(gc.G))
            assert [R.g.flags(g)["solves"] for g in range(gc.G)] == [1, 1, 1]
        else:
            R.g.solve(max_iters=20)
        outs.append(R.T())
        R.close()
    assert outs[0].tobytes() == outs[1].tobytes()


# --------------------------------------------------------------------------------------------------------------------- 4
def test_einval_writes_nothing(liw, synth, gg):
    import torch
    R = Rig(liw, synth, gg, guard=GUARD, chi2_max=cs.CHI2_MAX).feed()
    R.g.solve()
    torch.cuda.synchronize()
    ch = torch.full((cs.G,), 7, dtype=torch.uint8, device="cuda")
    snap = R.g._buf.clone()
    L, h, vp = R.g.Lg, R.g.h, lambda t: C.c_void_p(t.data_ptr())
    st, odd, a, c = vp(R.g.store), C.c_void_p(R.g.store.data_ptr() + 4), vp(R.g.gsel), vp(ch)
    d, i = C.c_double, C.c_int
    calls = [L.liw_ggate_gate(None, st, a, d(12.0), i(2), c, None), L.liw_ggate_gate(h, None, a, d(12.0), i(2), c, None), L.liw_ggate_gate(h, odd, a, d(12.0), i(2), c, None),
             L.liw_ggate_gate(h, st, None, d(12.0), i(2), c, None), L.liw_ggate_gate(h, st, a, d(12.0), i(2), None, None)]
    calls += [L.liw_ggate_gate(h, st, a, d(v), i(2), c, None) for v in (0.0, -12.0, float("inf"), float("nan"))]
    calls += [L.liw_ggate_gate(h, st, a, d(12.0), i(0), c, None), L.liw_ggate_get(h, st, cs.G, 0, None, None, None), L.liw_ggate_get(h, st, -1, 0, None, None, None),
              L.liw_ggate_get(h, odd, 0, 0, None, None, None), L.liw_ggate_get(h, st, 0, -1, None, None, None)]
    torch.cuda.synchronize()
    assert calls == [-22] * len(calls), calls
    assert torch.equal(R.g._buf, snap) and ch.cpu().tolist() == [7] * cs.G
    assert bool((R.g._buf[:GUARD] == 0xA5).all()) and bool((R.g._buf[-GUARD:] == 0xA5).all())
    R.g.chi2_max = None
    with pytest.raises(ValueError):
        R.g.gate()                                   # no threshold, here or in the constructor
    R.close()


# --------------------------------------------------------------------------------------------------------------------- 5
def test_push_reads_nothing_back(liw, synth, gg):
    """FleetGroupGraph.push with chi2_max set: the aligner's detect_cross is replaced by the cases' hand-made outputs (device tensors), so
    push runs partner choice, add_edges and solve_gated; the synchronous methods are wrapped as test_end_to_end_two_robots_one_room wraps
    them and none may be called"""
    import torch
    R = Rig(liw, synth, gg, chi2_max=cs.CHI2_MAX)
    dev = R.al.dev
    outs = []
    for c in cs.fleet()["calls"]:
        o, _ = R.call(c)
        outs.append(dict(found=torch.tensor(o["found"], device=dev), edge=torch.tensor(o["edge"], device=dev), tf12=torch.tensor(o["tf12"], device=dev)))
    feed = iter(outs)
    R.al.detect_cross = lambda key, partner: dict(next(feed))
    R.al.link = lambda partner=None: {}
    added = torch.ones(cs.B, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    reads = []
    for o, names in ((R.g, ("_sync", "summaries", "flags", "edges", "edge_states", "get_Z", "last_summary")), (R.fb, ("_sync", "_read_n_due")), (R.fl, ("_sync",))):
        for nm in names:
            setattr(o, nm, (lambda real, nm: lambda *a, **k: reads.append(nm) or real(*a, **k))(getattr(o, nm), nm))
    res = [R.g.push(dict(added=added)) for _ in outs]
    assert reads == [] and all(r["gsel"].is_cuda and r["summary"].is_cuda for r in res)
    torch.cuda.synchronize()
    states = [np.flatnonzero(R.g.edge_states(g)["state"]).tolist() for g in range(cs.G)]
    print("after three pushes the rejected edges are", states, "solves", [R.g.flags(g)["solves"] for g in range(cs.G)])
    # every rejected edge is one of the wrong ones, group A's first edge among them, and the consistent group keeps everything
    wrong = [[0], [0, 3], [3], []]
    assert all(set(s) <= set(w) for s, w in zip(states, wrong)) and states[0] == [0] and states[3] == []
    R.close()
