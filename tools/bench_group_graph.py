"""Group pose graph timing on the MI355X (include/liw_group_graph.h): liw_ggraph_solve for G groups of M linked robots, each group a
cycle with two rings of chords (3 M edges, noisy measurements, the start 2 cm / 5 mrad off), one launch per solve.  Beside it, as the
yardstick for the lock-step alternative, FleetBackEnd.solve (about ten launches per iteration) for G robots whose graphs have the
same node and edge counts: M key frames, M - 1 sequential edges and 2 M + 1 loops, ground factors off.  Median of --reps calls after
two warm-ups, wall time around torch.cuda.synchronize(); the time per LM iteration divides by the most iterations any group (robot)
took.  The edge gate (include/liw_group_gate.h) on the same, all-consistent edges: liw_ggate_gate alone after a solve (gate_ms; every
edge is evaluated and its pair's support counted, none is retired), and FleetGroupGraph.solve_gated, which adds to the solve two gates
and two solve launches that return at once (solve_gated_ms, against solve_ms).  One JSON line per (G, M), also written to --out.
  python tools/bench_group_graph.py [--groups 64,1024] [--members 4,16] [--reps 12] [--no-backend] [--out profiles/group_graph_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + K if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _tf(rng, span, yaw, tilt=0.01):
    T = np.eye(4)
    T[:3, :3] = _exp(np.array([rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-yaw, yaw)]))
    T[:3, 3] = rng.uniform(-span, span, 3) * (1.0, 1.0, 0.05)
    return T


def _inv(T):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3])
    return out


def _t12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def timed(torch, reps, before, call):
    ts = []
    for k in range(reps + 2):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def group_graph_leg(liw, synth, gg, G, M, reps):
    import torch
    lp = liw.loop
    rng = np.random.default_rng(1)
    B, K = G * M, 2
    prm = synth.office_params()
    # the detector only lends the aligner its handle: a small store
    fl = liw.FleetLoopDetector(prm, dict(lp.office_loop_params(), submap_count=1, min_interval=2), dict(B=B, max_keyframes=K, max_points=16, max_kf_corners=8))
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=K, max_loops=1))
    al = liw.FleetGroupAligner(fl, np.repeat(np.arange(G), M), list(range(0, B, M)), 9, 0.01)       # the first robot of a group is its anchor
    al.linked.fill_(1)
    gr = gg.FleetGroupGraph(al, fb, M, 3 * M, chi2_max=12.0, min_support=2, gate_rounds=2)
    # one group's data, tiled: truth W, poses P, start T0
    W = [np.eye(4)] + [_tf(rng, 4.0, 2.5) for _ in range(M - 1)]
    P = [[_tf(rng, 3.0, 2.5) for _ in range(K)] for _ in range(M)]
    T0 = [W[0]] + [W[r] @ _tf(rng, 0.02, 0.005, 0.005) for r in range(1, M)]
    lib = liw.lib()
    import ctypes as C
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def pose_of(T):
        t, p, q = np.ascontiguousarray(_t12(T)), np.zeros(3), np.zeros(3)
        lib.liw_lie_log_SE3(pd(t), pd(p), pd(q))
        return np.concatenate([p, q])
    poses = np.array([[pose_of(T) for T in P[r]] for r in range(M)])
    fb.poses()[:, :K, :] = torch.tensor(np.tile(poses, (G, 1, 1)), device=fb.dev)
    start = torch.tensor(np.tile(np.array([_t12(T) for T in T0]), (G, 1)), device=fb.dev)
    nkf = torch.full((B,), K, dtype=torch.int32, device=fb.dev)
    fixed = torch.zeros(B, dtype=torch.uint8, device=fb.dev)
    fixed[::M] = 1
    for ring in (1, 2, 3):
        if ring >= M:
            break
        edge, tf12 = np.zeros((M, 4), np.int32), np.zeros((M, 12))
        for a in range(M):
            b = (a + ring) % M
            noise = _tf(rng, 1e-3, 2e-4, 2e-4)
            edge[a] = (1, b, 0, 20)
            tf12[a] = _t12(_inv(P[a][1]) @ _inv(W[a]) @ W[b] @ P[b][0] @ noise)
        et = np.tile(edge, (G, 1))
        et[:, 1] += np.repeat(np.arange(G) * M, M)
        gr.add_edges(dict(found=np.ones(B, np.uint8), edge=et, tf12=np.tile(tf12, (G, 1))))
    ms = timed(torch, reps, lambda: al.T_g_w.copy_(start), lambda: gr.solve(fixed=fixed, n_keyframes=nkf))
    sm = gr.summaries()
    fl0 = gr.flags(0)
    gated_word = gr.group_regions()[:, 68:72]      # gated_solves: cleared, the group is eligible for a gate again

    def ungate():
        gated_word.zero_()
    gate_ms = timed(torch, reps, ungate, lambda: gr.gate())
    both_ms = timed(torch, reps, lambda: al.T_g_w.copy_(start), lambda: gr.solve_gated(fixed=fixed, n_keyframes=nkf))
    rejected = sum(gr.edge_states(g)["rejected"] for g in range(0, G, max(G // 8, 1)))
    its = max(s["iterations"] for s in sm)
    out = dict(solve_ms=ms[0], solve_ms_min=ms[1], solve_ms_max=ms[2], gate_ms=gate_ms[0], gate_ms_min=gate_ms[1], gate_ms_max=gate_ms[2],
               solve_gated_ms=both_ms[0], solve_gated_ms_min=both_ms[1], solve_gated_ms_max=both_ms[2], rejected=rejected, iterations=its, ms_per_iteration=ms[0] / max(its, 1), edges=fl0["used"],
               terminations=sorted(set(s["termination"] for s in sm)), lds_triangle=bool(3 * M * (6 * M + 1) <= 8192))
    for o in (gr, fb, fl):
        o.close()
    return out


def backend_leg(liw, synth, G, M, reps):
    """G robots, each a graph of M key frames, M - 1 sequential edges and 2 M + 1 loops measured from the truth"""
    import torch
    prm = synth.office_params()
    pg = dict(liw.posegraph.office_pg_params(), use_ground_p_factor=False, use_ground_q_factor=False)
    Gr = liw.posegraph.make_pose_graph(prm, N=M, seed=4, n_loop=0)
    rng = np.random.default_rng(2)

    def T(x):
        Mx = np.eye(4)
        Mx[:3, :3], Mx[:3, 3] = _exp(np.asarray(x[3:6])), x[:3]
        return Mx
    idx, tfs = [], []
    while len(idx) < 2 * M + 1:
        j, i = rng.choice(M, 2, replace=False)
        idx.append((int(j), int(i)))
        tfs.append(_t12(_inv(T(Gr["truth"][j])) @ T(Gr["truth"][i]) @ _tf(rng, 1e-3, 2e-4, 2e-4)))
    Gr = dict(Gr, loop_idx=np.array(idx, np.int32), loop_tf12=np.array(tfs))
    fb = liw.FleetBackEnd(prm, pg, dict(B=G, max_keyframes=M, max_loops=2 * M + 1))
    sel, stamps = torch.ones(G, dtype=torch.uint8, device=fb.dev), torch.full((G,), 100.0, dtype=torch.float64, device=fb.dev)
    fb.load_graph(0, Gr)
    region = fb.robot_regions()[0].clone()

    def restore():
        fb.robot_regions()[:] = region
    ms = timed(torch, reps, restore, lambda: fb.solve(sel, stamps))
    sm = fb.summaries()
    its = max(s["iterations"] for s in sm)
    fb.close()
    return dict(solve_ms=ms[0], solve_ms_min=ms[1], solve_ms_max=ms[2], iterations=its, ms_per_iteration=ms[0] / max(its, 1), edges=M - 1 + len(idx),
                terminations=sorted(set(s["termination"] for s in sm)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="64,1024")
    ap.add_argument("--members", default="4,16")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-backend", action="store_true", help="leave the FleetBackEnd yardstick out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_graph_bench.json"))
    a = ap.parse_args()
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    gg = importlib.import_module("2dliw-slam_amd.group_graph")
    import torch
    lines = []
    for G in (int(v) for v in a.groups.split(",")):
        for M in (int(v) for v in a.members.split(",")):
            row = dict(bench="group_graph", device=torch.cuda.get_device_name(0), groups=G, members=M, reps=a.reps,
                       ggraph=group_graph_leg(liw, synth, gg, G, M, a.reps))
            if not a.no_backend:
                row["fleet_backend"] = backend_leg(liw, synth, G, M, a.reps)
            print(json.dumps(row), flush=True)
            lines.append(row)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
