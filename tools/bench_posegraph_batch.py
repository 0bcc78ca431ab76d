"""Fleet pose-graph solve timing on the MI355X (include/liw_posegraph_batch.h): FleetBackEnd.solve for B robots that are all due,
each holding a graph of --keyframes key frames and --loops loop edges (posegraph.make_pose_graph, a different seed per robot up
to 16 distinct graphs), against the only way to do it without it: a host loop of B PoseGraph.solve calls on the same graphs.

The host loop is linear in the robots by construction (serial, synchronising calls), so it is measured on at most
--baseline-robots graphs and scaled to B; the JSON says which.  Wall times around torch.cuda.synchronize(); the graphs are loaded
again before every repetition (not timed).  One JSON line per B with the time per call, per LM iteration (the largest iteration
count of the fleet: the lock-step runs that many) and per robot.
  python tools/bench_posegraph_batch.py --fleet 1,64,1024 [--keyframes 200] [--loops 5] [--iters 20] [--check-every 4] [--reps 3]
Under rocprofv3 --kernel-trace --stats: --fleet 1024 --no-baseline --reps 1."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleet", default="1,64,1024")
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check-every", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-robots", type=int, default=64)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-ground-q", action="store_true", help="the smooth configuration, in which robots converge before the cap")
    a = ap.parse_args()
    import torch
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    prm = synth.office_params()
    pg = liw.posegraph.office_pg_params()
    if a.no_ground_q:
        pg["use_ground_q_factor"] = False
    K, L = a.keyframes, a.loops
    distinct = [liw.posegraph.make_pose_graph(prm, N=K, seed=200 + s, n_loop=L, laps=2.2) for s in range(16)]
    pgs = liw.posegraph.PoseGraph(prm)
    for B in [int(v) for v in a.fleet.split(",")]:
        graphs = [distinct[b % len(distinct)] for b in range(B)]
        fb = liw.FleetBackEnd(prm, pg, dict(B=B, max_keyframes=K, max_loops=L), max_iters=a.iters, check_every=a.check_every)
        sel, stamps = torch.ones(B, dtype=torch.uint8), torch.zeros(B, dtype=torch.float64)
        ts = []
        for rep in range(a.reps + 1):          # the first one warms up
            for b, G in enumerate(graphs):
                fb.load_graph(b, G)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fb.solve(sel, stamps)
            torch.cuda.synchronize()
            if rep:
                ts.append(time.perf_counter() - t0)
        sm = fb.summaries()
        its = max(s["iterations"] for s in sm)
        t_fleet = float(np.median(ts)) if ts else float("nan")
        row = dict(bench="fleet_posegraph", B=B, keyframes=K, loops=L, max_iters=a.iters, check_every=a.check_every, ground_q=not a.no_ground_q,
                   store_MB=round(fb.lay["bytes"] / 1e6, 1), fleet_ms_per_call=round(t_fleet * 1e3, 3), lm_iterations=its,
                   fleet_ms_per_iteration=round(t_fleet * 1e3 / max(its, 1), 3), fleet_us_per_robot=round(t_fleet * 1e6 / B, 2),
                   iterations_min=min(s["iterations"] for s in sm))
        if not a.no_baseline:
            nb = min(B, a.baseline_robots)
            args = [(G["poses"], G["seq_idx"], G["seq_tf12"], G["loop_idx"], G["loop_tf12"]) for G in graphs[:nb]]
            pgs.solve(pg, *args[0], max_iters=a.iters)
            tb = []
            for _ in range(max(1, a.reps)):
                t0 = time.perf_counter()
                for g in args:
                    pgs.solve(pg, *g, max_iters=a.iters)
                tb.append(time.perf_counter() - t0)
            t_host = float(np.median(tb)) * B / nb
            row.update(host_loop_ms_per_call=round(t_host * 1e3, 3), host_loop_robots_measured=nb, host_loop_scaled=bool(nb < B),
                       speedup=round(t_host / t_fleet, 2))
        print(json.dumps(row), flush=True)
        fb.close()
        del fb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
