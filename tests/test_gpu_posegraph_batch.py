"""The fleet pose-graph back-end on the device (include/liw_posegraph_batch.h, posegraph_batch.FleetBackEnd): the bookkeeping of B
keyframe_manager instances against the host restatement (tests/fleet_backend_reference.py), the lock-step solve against the oracle
(pyoracle.posegraph_solve) and one PoseGraph.solve per robot at the bars of tests/test_gpu_posegraph.py, independence of B / robot
index / check_every, a NaN robot among healthy ones, the commit after a solve, and the chain step -> loop detector -> back-end."""
import ctypes as C

import numpy as np
import pytest

import fleet_backend_reference as fbr

pytestmark = pytest.mark.gpu

GUARD = 256
BOOK_BAR = 1e-12   # tf and pose entries of the bookkeeping: magnitudes <= 100 m, a handful of fp64 operations


# ------------------------------------------------------------------------------------------------------------------ graphs
def _rec12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def _truth_loop(synth, G, j, i, rng, sp=0.002, sq=0.0008):
    """a loop edge (j, i) measured from the truth poses, with the noise of make_pose_graph's loops"""
    def T(x):
        M = np.eye(4)
        M[:3, :3] = synth.exp_so3(x[3:6])
        M[:3, 3] = x[:3]
        return M
    D = np.eye(4)
    D[:3, :3] = synth.exp_so3(rng.normal(0, sq, 3))
    D[:3, 3] = rng.normal(0, sp, 3)
    return (j, i), _rec12(synth.inv_se3(T(G["truth"][j])) @ T(G["truth"][i]) @ D)


def _with_loops(G, loops):
    G = dict(G)
    G["loop_idx"] = np.vstack([G["loop_idx"].reshape(-1, 2)] + [np.asarray([l[0]], dtype=np.int32) for l in loops]).astype(np.int32)
    G["loop_tf12"] = np.vstack([G["loop_tf12"].reshape(-1, 12)] + [l[1][None] for l in loops])
    return G


_CACHE = {}


def _graphs(liw, synth):
    """name -> graph: the graphs tests/test_gpu_posegraph.py solves, and the fleet solver's own edge cases"""
    if "graphs" in _CACHE:
        return _CACHE["graphs"]
    prm = synth.office_params()
    mp = liw.posegraph.make_pose_graph
    out = {}
    for N, n_loop, seed in ((12, 0, 1), (60, 5, 2), (150, 8, 3), (30, 3, 7)):
        out["mp_%d_%d_%d" % (N, n_loop, seed)] = mp(prm, N=N, seed=seed, n_loop=n_loop)
    # five loop edges between one pair of key frames, three one way and two the other (test_many_parallel_loop_edges...)
    G = mp(prm, N=50, seed=9, n_loop=4)
    const = int(G["seq_idx"][0, 0])
    e0 = next(k for k in range(len(G["loop_idx"])) if const not in G["loop_idx"][k])
    a, b = int(G["loop_idx"][e0, 0]), int(G["loop_idx"][e0, 1])
    rng = np.random.default_rng(3)
    extra = []
    for k in range(4):
        tf = G["loop_tf12"][e0].copy()
        tf[9:12] += rng.normal(0.0, 0.01, 3)
        if k % 2 == 0:
            extra.append(((a, b), tf))
        else:
            R = tf[:9].reshape(3, 3)
            extra.append(((b, a), np.concatenate([R.T.reshape(9), -R.T @ tf[9:12]])))
    out["dup_pair"] = _with_loops(G, extra)
    rng = np.random.default_rng(21)
    out["n2"] = mp(prm, N=2, seed=11, n_loop=0)
    out["n3"] = mp(prm, N=3, seed=12, n_loop=0)
    G4 = mp(prm, N=4, seed=13, n_loop=0)
    out["n4_loop"] = _with_loops(G4, [_truth_loop(synth, G4, 3, 1, rng)])
    out["n49"] = mp(prm, N=49, seed=14, n_loop=3)                  # one frame past a stride separator
    G0 = mp(prm, N=40, seed=5, n_loop=0)
    out["loop_on_0"] = _with_loops(G0, [_truth_loop(synth, G0, 39, 0, rng)])
    out["adjacent_seps"] = _with_loops(G0, [_truth_loop(synth, G0, 21, 20, rng), _truth_loop(synth, G0, 35, 3, rng)])
    # 23 separators (frames 0, 48, 59 and twenty distinct loop end points): 138 unknowns, a triangle of 9 591 doubles, more than the
    # 8 192 of LDS the solver asks for at the most, so this robot's separator system is factorised in its work area
    G6 = mp(prm, N=60, seed=6, n_loop=0)
    out["many_seps"] = _with_loops(G6, [_truth_loop(synth, G6, 31 + 2 * k, 2 + 2 * k, rng) for k in range(10)])
    _CACHE["graphs"] = out
    return out


def _separators(G):
    N = len(G["poses"])
    return len({0, N - 1} | set(range(0, N, 48)) | set(int(v) for v in np.asarray(G["loop_idx"]).reshape(-1)))


def _args(G):
    return (G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"] if len(G["loop_idx"]) else None, G["loop_tf12"] if len(G["loop_idx"]) else None)


CONFIGS = (("office_5", {}, 5), ("office_20", {}, 20), ("no_ground_q", dict(use_ground_q_factor=False), 0))


def _references(liw, synth, pyoracle):
    """(config, graph) -> (oracle poses, summary, PoseGraph.solve poses, summary), computed once"""
    if "refs" in _CACHE:
        return _CACHE["refs"]
    prm = synth.office_params()
    orc, pgs = pyoracle.Oracle(prm), liw.posegraph.PoseGraph(prm)
    refs = {}
    for cname, upd, cap in CONFIGS:
        cfg = dict(liw.posegraph.office_pg_params(), **upd)
        for gname, G in _graphs(liw, synth).items():
            xo, so = pyoracle.posegraph_solve(orc, cfg, *_args(G), max_iters=cap)
            xg, sg = pgs.solve(cfg, *_args(G), max_iters=cap)
            refs[cname, gname] = (xo, so, xg, sg)
    _CACHE["refs"] = refs
    return refs


def _backend(liw, synth, pg, B, K, ML, **kw):
    return liw.FleetBackEnd(synth.office_params(), pg, dict(B=B, max_keyframes=K, max_loops=ML), **kw)


def _solve_all(fb, graphs, cap, check_every, sel=None):
    import torch
    for b, G in enumerate(graphs):
        if G is not None:
            fb.load_graph(b, G)
    sel = np.array([G is not None for G in graphs], dtype=np.uint8) if sel is None else sel
    fb.solve(torch.as_tensor(sel), torch.full((fb.B,), 100.0, dtype=torch.float64), max_iters=cap, check_every=check_every)
    sm = fb.summaries()
    return [fb.keyframes(b)["poses"] if G is not None else None for b, G in enumerate(graphs)], sm


# ------------------------------------------------------------------------------------------------------------------ 1
def test_bookkeeping_case_by_case(liw, synth):
    """Six robots fed frame by frame: r0 fills max_keyframes, r1 is masked out, r2 is offered more loops than max_loops, r3 an edge
    outside its key frames and one with equal ends, r4 no loop, r5 one loop.  After every call the store equals the restatement."""
    import torch
    B, K, ML, F = 6, 5, 2, 9
    fb = _backend(liw, synth, liw.posegraph.office_pg_params(), B, K, ML, solve_period=1.0, guard=GUARD)
    lie = fbr.Lie(liw)
    ref = [fbr.RobotBackEnd(lie, K, ML, 1.0) for _ in range(B)]
    rng = np.random.default_rng(5)
    mask = np.array([1, 0, 1, 1, 1, 1], dtype=np.uint8)
    masked0 = fb.robot_regions()[1].clone()
    yaws = np.linspace(-np.pi + 1e-3, np.pi - 1e-3, F * B).reshape(F, B)       # planar, no closer to +-pi than 1e-3
    worst = 0.0

    def compare(due=None, key=None, stamps=None):
        nonlocal worst
        for b in range(B):
            if not mask[b]:
                continue
            r, fl, kf = ref[b], fb.flags(b), fb.keyframes(b)
            assert fb.num_keyframes(b) == len(r.tfs)
            assert (fl["loops"], fl["full"], fl["loops_full"], fl["bad_edge"], fl["pending"], fl["solves"]) == \
                (len(r.loop_idx), int(r.full), int(r.loops_full), int(r.bad_edge), int(r.pending), r.solves), (b, fl)
            assert fl["last_solve_time"] == r.last_solve_time and np.array_equal(kf["stamps"], np.array(r.stamps))
            if r.tfs:
                worst = max(worst, float(np.abs(kf["tf12"] - np.array(r.tfs)).max()), float(np.abs(kf["poses"] - np.array(r.poses)).max()))
            se = fb.seq_edges(b)
            assert se.shape == (max(len(r.tfs) - 1, 0), 12)
            if len(se):
                worst = max(worst, float(np.abs(se - np.array(r.seq)).max()))
            li, lt = fb.loop_edges(b)
            assert li.tolist() == [list(e) for e in r.loop_idx] and np.array_equal(lt, np.array(r.loop_tf).reshape(-1, 12))
            if due is not None:
                assert bool(due[b]) == r.due(key[b], stamps[b]), b
        assert worst <= BOOK_BAR, worst

    for k in range(F):
        key = np.array([1, 1, k % 2 == 0, k % 2 == 1 or k == 0, k % 3 == 0, 1], dtype=np.uint8)
        pose = np.zeros((B, 6))
        pose[:, :2] = rng.uniform(-100, 100, (B, 2))
        pose[:, 5] = yaws[k]
        stamps = 0.7 * k + 0.01 * np.arange(B)
        added = fb.add_keyframes(torch.as_tensor(key), torch.as_tensor(pose), torch.as_tensor(stamps), mask=torch.as_tensor(mask)).cpu().numpy()
        for b in range(B):
            if mask[b] and key[b]:
                assert bool(added[b]) == ref[b].add_keyframe(pose[b], stamps[b]), (k, b)
            elif mask[b]:
                assert added[b] == 0
        compare()
        found = np.zeros(B, dtype=np.uint8)
        edge = np.full((B, 3), -1, dtype=np.int32)
        tf12 = np.zeros((B, 12))
        n = [len(r.tfs) for r in ref]
        found[1], edge[1] = 1, (0, 0, 1)                                           # masked out: never looked at
        if key[2] and n[2] >= 2:
            found[2], edge[2] = 1, (n[2] - 1, 0, 7)
        if k == 2:
            found[3], edge[3] = 1, (n[3] - 1, 7, 3)                                # index2 outside the key frames
        if k == 4:
            found[3], edge[3] = 1, (1, 1, 3)                                       # equal ends
        if k == 5:
            found[3], edge[3] = 1, (n[3] - 1, 0, 3)
        if k == 4:
            found[5], edge[5] = 1, (n[5] - 1, 1, 9)
        for b in range(B):
            tf12[b] = lie.make_tf(rng.uniform(-1, 1, 3), [0, 0, rng.uniform(-1, 1)])
        fb.add_loops(torch.as_tensor(found), torch.as_tensor(edge), torch.as_tensor(tf12), mask=torch.as_tensor(mask))
        for b in range(B):
            if mask[b] and found[b]:
                ref[b].add_loop(edge[b], tf12[b])
        due, n_due = fb.due(torch.as_tensor(key), torch.as_tensor(stamps), mask=torch.as_tensor(mask))
        due = due.cpu().numpy()
        compare(due, key, stamps)
        assert int(n_due.item()) == int(due[mask != 0].sum())
    assert ref[0].full and ref[2].loops_full and ref[3].bad_edge and len(ref[3].loop_idx) == 1 and not ref[4].loop_idx and len(ref[5].loop_idx) == 1
    # correct() with the identity, the masked-out robot, the guard, LIW_EINVAL
    pose = np.concatenate([rng.uniform(-50, 50, (B, 2)), np.zeros((B, 3)), rng.uniform(-3, 3, (B, 1))], axis=1)
    got = fb.correct(torch.as_tensor(pose), mask=torch.as_tensor(mask)).cpu().numpy()
    for b in range(B):
        if mask[b]:
            assert np.abs(got[b] - ref[b].correct(pose[b])).max() <= BOOK_BAR
    assert torch.equal(fb.robot_regions()[1], masked0)
    before = fb._buf.clone()
    p = fb._ptr(fb.store)
    L = fb.L
    assert L.liw_fpg_add_keyframes(fb.h, p, None, p, p, None, None, None) == -22
    assert L.liw_fpg_add_keyframes(fb.h, C.c_void_p(fb.store.data_ptr() + 4), p, p, p, None, None, None) == -22
    assert L.liw_fpg_add_loops(fb.h, p, p, None, p, None, None) == -22
    assert L.liw_fpg_due(fb.h, p, p, p, None, None, None, None) == -22
    assert L.liw_fpg_solve(fb.h, p, None, p, 3, 0, p, None) == -22
    assert L.liw_fpg_correct(fb.h, p, None, p, None, None) == -22
    assert L.liw_fpg_reset(fb.h, None, None, None) == -22
    torch.cuda.synchronize()
    assert torch.equal(fb._buf, before)
    assert bool((fb._buf[:GUARD] == 0xA5).all()) and bool((fb._buf[-GUARD:] == 0xA5).all())
    print("fleet back-end bookkeeping: worst tf / pose entry difference %.3e" % worst)
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cname,upd,cap", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_solve_parity_every_robot(liw, synth, pyoracle, cname, upd, cap):
    """All graphs in one fleet, every robot compared with the oracle and with its own PoseGraph.solve at the standing bars."""
    graphs = _graphs(liw, synth)
    refs = _references(liw, synth, pyoracle)
    names = list(graphs)
    cfg = dict(liw.posegraph.office_pg_params(), **upd)
    ns = {n: _separators(graphs[n]) for n in names}
    assert ns["many_seps"] == 23 and 3 * 23 * (6 * 23 + 1) > 8192 >= 3 * ns["mp_150_8_3"] * (6 * ns["mp_150_8_3"] + 1)   # both branches of k_fpg_reduced
    fb = _backend(liw, synth, cfg, len(names), 150, 10, guard=GUARD)
    poses, sm = _solve_all(fb, [graphs[n] for n in names], cap, 4)
    torch_regions = fb.robot_regions().clone()
    for b, name in enumerate(names):
        G, (xo, so, xg, sg), s, x = graphs[name], refs[cname, name], sm[b], poses[b]
        print("%-12s %-14s fleet %s" % (cname, name, s))
        for what, xr, sr in (("oracle", xo, so), ("PoseGraph.solve", xg, sg)):
            assert (s["iterations"], s["successful"], s["termination"]) == (sr["iterations"], sr["successful"], sr["termination"]), (name, what, s, sr)
            assert abs(s["initial_cost"] - sr["initial_cost"]) <= 1e-9 * sr["initial_cost"], (name, what)
            assert abs(s["final_cost"] - sr["final_cost"]) <= 1e-6 * max(1.0, sr["final_cost"]), (name, what)
            assert np.abs(x - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max()), (name, what)
        assert np.array_equal(x[0], G["poses"][0])                                   # key frame 0 is held constant: bit-unchanged
        assert fb.last_summary(b) == s and fb.flags(b)["solves"] == 1 and fb.flags(b)["pending"] == 0
    quick, long_ = sm[names.index("mp_12_0_1")], sm[names.index("mp_150_8_3")]
    if cname == "office_20":     # with the cone-shaped ground_factor_q every robot runs to the cap
        assert long_["iterations"] == 20 and long_["termination"] == 4
    if cname == "no_ground_q":   # smooth problem: the loop-free robot is done within a few iterations, long before the 150-frame robot
        assert quick["termination"] == 2 and quick["iterations"] < 10 and quick["iterations"] < long_["iterations"]
    # every separator system from the work area (no LDS): the same instructions on another pointer, the same bytes for every robot
    import torch
    fb.set_lds_doubles(0)
    fb.reset()
    _solve_all(fb, [graphs[n] for n in names], cap, 4)
    torch.cuda.synchronize()
    assert torch.equal(fb.robot_regions(), torch_regions)
    assert bool((fb._buf[:GUARD] == 0xA5).all()) and bool((fb._buf[-GUARD:] == 0xA5).all())
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("upd,cap", [({}, 12), (dict(use_ground_q_factor=False), 0)], ids=["office_12", "no_ground_q"])
def test_independence_and_determinism(liw, synth, upd, cap):
    """A robot's region (poses, summary, modify_delta_tf) is bit-identical solved alone, at another index among other graphs, with
    check_every 0 / 1 / 4, with the separator system in LDS or in the work area, in 256 tiled copies and in two runs."""
    import torch
    graphs = _graphs(liw, synth)
    G, cfg = graphs["mp_60_5_2"], dict(liw.posegraph.office_pg_params(), **upd)

    def region(fb, b, nbytes):
        torch.cuda.synchronize()
        return fb.robot_regions()[b, :nbytes].cpu().numpy().tobytes()
    fb = _backend(liw, synth, cfg, 1, 60, 5)
    x0, s0 = _solve_all(fb, [G], cap, 4)
    want = region(fb, 0, fb.lay["robot_bytes"])
    assert s0[0]["iterations"] >= 4 and s0[0]["successful"] >= 3
    for ce in (0, 1, 4):
        _solve_all(fb, [G], cap, ce)
        assert region(fb, 0, fb.lay["robot_bytes"]) == want, ce
    fb.close()
    others = [graphs["mp_30_3_7"], graphs["n3"], G, graphs["n49"]]
    fb = _backend(liw, synth, cfg, 4, 60, 5)
    for ce in (0, 4):
        xs, ss = _solve_all(fb, others, cap, ce)
        assert region(fb, 2, fb.lay["robot_bytes"]) == want and ss[2] == s0[0]
        if upd:          # the smooth configuration: robots leave the lock-step at different iterations
            assert len({s["iterations"] for s in ss}) > 1 and all(s["termination"] in (2, 3) for s in ss)
    fb.close()
    fb = _backend(liw, synth, cfg, 3, 60, 5)
    fb.set_lds_doubles(0)                              # the separator system in the work area instead of LDS
    xs, ss = _solve_all(fb, [graphs["n4_loop"], G, None], cap, 4)
    assert np.array_equal(xs[1], x0[0]) and ss[1] == s0[0] and region(fb, 1, fb.lay["robot_bytes"]) == want
    with pytest.raises(liw.LiwError):
        fb.set_lds_doubles(8193)
    fb.close()
    B = 256
    fb = _backend(liw, synth, cfg, B, 60, 5)
    runs = []
    for _ in range(2):
        _solve_all(fb, [G] * B, cap, 0)
        torch.cuda.synchronize()
        runs.append(fb.robot_regions().clone())
    assert torch.equal(runs[0], runs[1])
    assert bool((runs[0] == runs[0][0:1]).all()) and runs[0][0].cpu().numpy().tobytes() == want
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def test_nan_robot_among_healthy_ones(liw, synth):
    """A NaN in one loop tf12: that robot ends as PoseGraph.solve ends on the graph (same termination, poses unchanged) and its
    neighbours' bytes are those of a run without it."""
    import torch
    graphs = _graphs(liw, synth)
    cfg, cap = liw.posegraph.office_pg_params(), 10
    bad = dict(graphs["mp_30_3_7"])
    bad["loop_tf12"] = bad["loop_tf12"].copy()
    bad["loop_tf12"][1, 4] = np.nan
    xs_ref, s_ref = liw.posegraph.PoseGraph(synth.office_params()).solve(cfg, *_args(bad), max_iters=cap)
    fb = _backend(liw, synth, cfg, 3, 60, 5)
    fleet = [graphs["mp_60_5_2"], bad, graphs["n49"]]
    xs, ss = _solve_all(fb, fleet, cap, 4)
    torch.cuda.synchronize()
    with_bad = fb.robot_regions().clone()
    assert (ss[1]["termination"], ss[1]["iterations"], ss[1]["successful"]) == (s_ref["termination"], s_ref["iterations"], s_ref["successful"]), (ss[1], s_ref)
    assert np.array_equal(xs[1], bad["poses"]) and np.array_equal(xs_ref, bad["poses"])
    assert np.isfinite(xs[0]).all() and np.isfinite(xs[2]).all() and ss[0]["successful"] > 0 and ss[2]["successful"] > 0
    # one fleet, both ends of the lock-step: the NaN robot leaves after its invalid steps, its neighbours run to the cap
    assert ss[1]["iterations"] < cap and all((ss[b]["iterations"], ss[b]["termination"]) == (cap, 4) for b in (0, 2)), ss
    fb.reset()
    _solve_all(fb, [fleet[0], None, fleet[2]], cap, 4)
    torch.cuda.synchronize()
    without = fb.robot_regions()
    assert torch.equal(with_bad[0], without[0]) and torch.equal(with_bad[2], without[2])
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_after_the_solve_and_the_solve_period(liw, synth):
    """push() frame by frame: the first loop is solved at once, a loop that arrives before solve_period has passed waits, one after it
    is solved; modify_delta_tf, solves, the pending flag, the key frames added afterwards and correct() follow the restatement, whose
    solve is handed the device's poses."""
    import torch
    G = _graphs(liw, synth)["mp_30_3_7"]
    N, period, B = 30, 1.2, 2
    fb = _backend(liw, synth, liw.posegraph.office_pg_params(), B, 32, 4, solve_period=period, max_iters=8)
    lie = fbr.Lie(liw)
    rb = fbr.RobotBackEnd(lie, 32, 4, period)
    trig = {int(j): (int(i), G["loop_tf12"][e]) for e, (j, i) in enumerate(G["loop_idx"])}
    assert len(trig) == 3
    untouched = fb.robot_regions()[1].clone()
    solved_at, waited = [], 0
    for k in range(N):
        stamps = np.array([0.5 * k, 0.5 * k])
        key = np.array([1, 0], dtype=np.uint8)
        pose = np.stack([G["poses"][k], np.zeros(6)])
        found, edge, tf12 = np.zeros(B, dtype=np.uint8), np.full((B, 3), -1, dtype=np.int32), np.zeros((B, 12))
        if k in trig:
            found[0], edge[0], tf12[0] = 1, (k, trig[k][0], 5), trig[k][1]
        out = fb.push(dict(key=torch.as_tensor(key), pose=torch.as_tensor(pose)),
                      dict(added=torch.as_tensor(key), found=torch.as_tensor(found), edge=torch.as_tensor(edge), tf12=torch.as_tensor(tf12)),
                      torch.as_tensor(stamps))
        assert rb.add_keyframe(pose[0], stamps[0])
        if k in trig:
            rb.add_loop(edge[0], tf12[0])
        want_due = rb.due(True, stamps[0])
        assert out["n_due"] == int(want_due) and bool(out["due"].cpu().numpy()[0]) == want_due
        kf = fb.keyframes(0)
        if want_due:
            s = fb.last_summary(0)
            assert s["iterations"] >= 1 and fb.summaries()[0] == s
            rb.commit(kf["poses"], stamps[0])
            solved_at.append(k)
        elif rb.pending:
            waited += 1
        fl = fb.flags(0)
        assert (fl["solves"], fl["pending"], fl["last_solve_time"], fl["loops"]) == (rb.solves, int(rb.pending), rb.last_solve_time, len(rb.loop_idx))
        assert np.abs(kf["poses"] - np.array(rb.poses)).max() <= BOOK_BAR and np.abs(fb.get_modify_delta_tf(0) - rb.modify).max() <= BOOK_BAR
        assert np.abs(out["modify_delta_tf"][0].cpu().numpy() - rb.modify).max() <= BOOK_BAR
        got = fb.correct(torch.as_tensor(pose)).cpu().numpy()[0]
        assert np.abs(got - rb.correct(pose[0])).max() <= BOOK_BAR
    first = min(trig)
    assert solved_at[0] == first and len(solved_at) == 2 and waited >= 1 and solved_at[1] - first > period / 0.5
    assert np.abs(rb.modify - fbr.IDENTITY12).max() > 1e-4
    assert torch.equal(fb.robot_regions()[1], untouched)
    fb.close()


def test_push_never_solves_a_masked_out_robot(liw, synth):
    """Robot 0 is due and solved in one frame; in the next it is masked out (its row of `due` still says 1 from before) while robot 1
    becomes due: only robot 1 is solved, and no byte of robot 0's region or summary row changes."""
    import torch
    G = _graphs(liw, synth)["mp_12_0_1"]
    B, N = 2, 12
    fb = _backend(liw, synth, liw.posegraph.office_pg_params(), B, 16, 2, solve_period=0.1, max_iters=4)
    lie = fbr.Lie(liw)
    loop_tf = lie.mul(lie.inverse(lie.make_tf(G["poses"][N - 1, :3], G["poses"][N - 1, 3:])), lie.make_tf(G["poses"][2, :3], G["poses"][2, 3:]))

    def frame(k, found, mask):
        key = torch.ones(B, dtype=torch.uint8)
        pose = torch.as_tensor(np.stack([G["poses"][k], G["poses"][k]]))
        edge = torch.as_tensor(np.array([[k, 2, 5], [k, 2, 5]], dtype=np.int32))
        tf12 = torch.as_tensor(np.stack([loop_tf, loop_tf]))
        return fb.push(dict(key=key, pose=pose), dict(added=key, found=torch.as_tensor(np.array(found, dtype=np.uint8)), edge=edge, tf12=tf12),
                       torch.full((B,), 0.5 * k, dtype=torch.float64), mask=None if mask is None else torch.as_tensor(np.array(mask, dtype=np.uint8)))
    for k in range(N - 1):
        assert frame(k, [0, 0], None)["n_due"] == 0
    out = frame(N - 1, [1, 0], None)                   # robot 0 closes a loop and is solved
    assert out["n_due"] == 1 and out["due"].cpu().numpy().tolist() == [1, 0]
    assert (fb.flags(0)["solves"], fb.flags(1)["solves"]) == (1, 0)
    torch.cuda.synchronize()
    region0, row0 = fb.robot_regions()[0].clone(), fb.summary[0].clone()
    assert int(fb.due_flags[0]) == 1                   # what a masked-out frame leaves in place
    # the next frame: robot 0 masked out, robot 1 offered a loop between the key frames it holds
    key = torch.ones(B, dtype=torch.uint8)
    out = fb.push(dict(key=key, pose=torch.as_tensor(np.stack([G["poses"][N - 1], G["poses"][N - 1]]) + 0.01)),
                  dict(added=key, found=torch.as_tensor(np.array([1, 1], dtype=np.uint8)), edge=torch.as_tensor(np.array([[N, 2, 5], [N, 2, 5]], dtype=np.int32)),
                       tf12=torch.as_tensor(np.stack([loop_tf, loop_tf]))),
                  torch.full((B,), 0.5 * N, dtype=torch.float64), mask=torch.as_tensor(np.array([0, 1], dtype=np.uint8)))
    assert out["n_due"] == 1 and out["due"].cpu().numpy().tolist() == [0, 1]
    torch.cuda.synchronize()
    assert torch.equal(fb.robot_regions()[0], region0) and torch.equal(fb.summary[0], row0)
    assert (fb.flags(0)["solves"], fb.flags(1)["solves"], fb.num_keyframes(0), fb.num_keyframes(1)) == (1, 1, N, N + 1)
    mod = out["modify_delta_tf"]
    assert mod.data_ptr() == fb.store.data_ptr() + 40 and np.array_equal(mod[1].cpu().numpy(), fb.get_modify_delta_tf(1))   # a view of the store
    fb.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_behind_the_tracker(liw, synth):
    """step -> FleetLoopDetector.push -> FleetBackEnd.push for the fleet of tests/test_gpu_loop_batch.py::test_behind_the_tracker: both
    stores hold the same key frames, every stored loop edge is the detector's output of its frame, and a frame without a solve reads
    back nothing but the n_due word."""
    import torch
    import test_gpu_laser_track as tlt
    import test_gpu_loop as tgl
    import test_gpu_loop_batch as tglb
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
    tp = dict(liw.laser_batch.office_track_params(prm), key_frame_p_motion_threshold=0.1)
    nb, F, B = 8, 6, 16
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=F + 1, L=0) for j in range(nb)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(F + 1, 15) for t in trajs])
    ranges = np.stack([[tlt._cast(liw, synth, lp, 3000 + j, truth[j, k, 0:6], seed=j * 10 + k) for k in range(F + 1)] for j in range(nb)])
    sc = dict(prm=prm, lp=lp, tp=tp, nb=nb, F=F, trajs=trajs, truth=truth, ranges=ranges, times=np.stack([t["times"] for t in trajs]))
    rob = np.arange(B) % nb
    ft = tlt._fleet(liw, sc, B)
    tlt._seed(torch, sc, ft.fe, rob)
    ft.start(truth[rob, 0])
    K = 16
    fl = tglb._fleet(liw, synth, tgl._params(min_interval=2, submap_count=3), B, K, 256, 256)
    fb = _backend(liw, synth, liw.posegraph.office_pg_params(), B, K, 4, solve_period=1e9, max_iters=5)
    reads = []
    real_read = fb._read_n_due
    fb._read_n_due = lambda: reads.append(1) or real_read()
    stored = [[] for _ in range(B)]
    frames_without_solve = 0
    for k in range(1, F + 1):
        r, st = tlt._frame(torch, sc, rob, k)
        o = ft.step(r, st, tlt._interval(torch, sc, rob, k))
        lo = fl.push(o)
        before = len(reads)
        out = fb.push(o, lo, torch.as_tensor(sc["times"][rob, k]))
        assert len(reads) == before + 1
        found, edge, tf12, added = [lo[x].cpu().numpy() for x in ("found", "edge", "tf12", "added")]
        assert np.array_equal(out["added"].cpu().numpy(), added)
        for b in range(B):
            if found[b]:
                stored[b].append((edge[b, :2].tolist(), tf12[b].copy()))
        frames_without_solve += out["n_due"] == 0
    edges = 0
    for b in range(B):
        assert fb.num_keyframes(b) == fl.num_keyframes(b) >= 3
        li, lt = fb.loop_edges(b)
        assert li.tolist() == [e[0] for e in stored[b]][:4] and all(np.array_equal(lt[i], stored[b][i][1]) for i in range(len(li)))
        assert fb.flags(b)["bad_edge"] == 0
        edges += len(li)
    assert len(reads) == F and frames_without_solve >= 1
    print("behind the tracker: %d loop edges stored, %d of %d frames without a solve" % (edges, frames_without_solve, F))
    fb.close()
    fl.close()
    ft.close()
