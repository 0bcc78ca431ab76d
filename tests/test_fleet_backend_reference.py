"""tests/fleet_backend_reference.py (the host restatement the GPU tests of the fleet pose-graph back-end compare with) against the
oracle's keyframe_manager (pyoracle.backend_run): the same key frames and loop schedule, the solve delegated to
pyoracle.posegraph_solve, give the same counts, modify_delta_tf and poses.  Runs anywhere: the oracle is host code."""
import numpy as np

import fleet_backend_reference as fbr


def _schedule(liw, synth, N, n_loop, seed):
    prm = synth.office_params()
    G = liw.posegraph.make_pose_graph(prm, N=N, seed=seed, n_loop=n_loop)
    times = 0.5 * np.arange(N)
    loops = [(int(j), int(i), G["loop_tf12"][e]) for e, (j, i) in enumerate(G["loop_idx"])]
    assert len({l[0] for l in loops}) == len(loops) and all(l[0] > l[1] for l in loops)   # one loop per trigger, to an older key frame
    return prm, G, times, loops


def test_restatement_equals_the_oracle_back_end(liw, synth, pyoracle):
    """LM capped at 8 iterations, before the round-off amplification of the pose-graph LM path sets in (tests/test_gpu_replay.py): the two
    differ only by the libm calls of liw_lie_* against the oracle's lie.h, so the bar is 1e-9 of the pose scale."""
    pg = liw.posegraph.office_pg_params()
    for N, n_loop, seed, period in ((40, 3, 7, 1.0), (60, 5, 2, 0.4), (25, 0, 4, 1.0)):
        prm, G, times, loops = _schedule(liw, synth, N, n_loop, seed)
        orc = pyoracle.Oracle(prm)

        def solve(g):
            x, s = pyoracle.posegraph_solve(orc, pg, g["poses"], g["seq_idx"], g["seq_tf12"], g["loop_idx"], g["loop_tf12"], max_iters=8)
            return x, s["iterations"]
        rb, its = fbr.run_schedule(liw, solve, times, G["poses"], loops, period)
        ref = pyoracle.backend_run(orc, pg, times, G["poses"], loops, solve_period=period, max_iterations=8)
        assert (len(rb.tfs), len(rb.loop_idx), rb.solves, its) == (ref["keyframes"], ref["loops"], ref["solves"], ref["iterations"])
        assert rb.solves >= (2 if n_loop >= 3 else 0) and not (rb.full or rb.loops_full or rb.bad_edge)
        scale = max(1.0, np.abs(ref["poses"]).max())
        assert np.abs(np.array(rb.poses) - ref["poses"]).max() <= 1e-9 * scale
        assert np.abs(rb.modify - ref["modify_delta_tf"]).max() <= 1e-9 * scale
        if n_loop:
            assert np.abs(rb.modify - fbr.IDENTITY12).max() > 1e-4      # the loop closures moved the map frame
            assert np.abs(rb.correct(G["poses"][-1]) - np.array(rb.poses)[-1]).max() <= 1e-9 * scale or rb.pending


def test_capacity_and_bad_edge_rules(liw):
    lie = fbr.Lie(liw)
    rb = fbr.RobotBackEnd(lie, max_keyframes=3, max_loops=1, solve_period=1.0)
    poses = [[0.1 * k, 0.0, 0.0, 0.0, 0.0, 0.2 * k] for k in range(5)]
    assert [rb.add_keyframe(x, k) for k, x in enumerate(poses)] == [True, True, True, False, False]
    assert rb.full and len(rb.tfs) == 3 and len(rb.seq) == 2 and not rb.pending
    for edge in ((2, 3), (-1, 0), (1, 1)):
        rb.add_loop(edge, fbr.IDENTITY12)
    assert rb.bad_edge and not rb.loop_idx and not rb.pending and not rb.due(True, 100.0)
    rb.add_loop((2, 0), fbr.IDENTITY12)
    rb.add_loop((2, 1), fbr.IDENTITY12)
    assert rb.loops_full and rb.loop_idx == [(2, 0)] and rb.pending and rb.due(True, 0.0) and not rb.due(False, 0.0)
    rb.commit(np.array(rb.poses), 5.0)
    assert rb.solves == 1 and not rb.pending and np.abs(rb.modify - fbr.IDENTITY12).max() <= 1e-15
    rb.add_loop((1, 0), fbr.IDENTITY12)          # still full: nothing stored, nothing pending
    assert not rb.pending and not rb.due(True, 100.0)
    assert np.abs(lie.mul(lie.inverse(rb.tfs[0]), rb.tfs[1]) - rb.seq[0]).max() == 0.0
