"""Joint group pose graph timing on the MI355X (include/liw_group_joint.h): FleetGroupJoint.solve for G groups of M robots with N key
frames each (drifting chains), two own loops per robot and 3 M cross edges between key frames, office configuration.  Median of --reps
calls after two warm-ups, wall time around torch.cuda.synchronize(); the time per LM iteration divides by the most iterations any group
took.  Beside it the baseline, what the tree offers without this module: a host loop over the groups that reads the back-end store, the
group graph's edge list and T_g_w back, concatenates the chains and calls liw_posegraph_solve (PoseGraph.solve; a list that is not one
chain takes its dense factorisation, with the trust region on the host).  The baseline is timed on min(G, --baseline-groups) groups and
scaled to G ("baseline_scaled": true).  One JSON line per (G, M, N), also written to --out.
  python tools/bench_group_joint.py [--groups 1,64,1024] [--members 2,4] [--keyframes 50,200] [--reps 12] [--baseline-groups 64]
                                    [--baseline-reps 12] [--no-baseline] [--check-every 0] [--out profiles/group_joint_bench.json]"""
import argparse
import ctypes as C
import importlib
import json
import math
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


def _small(rng, sp, sq):
    T = np.eye(4)
    T[:3, :3] = _exp(rng.uniform(-sq, sq, 3))
    T[:3, 3] = rng.uniform(-sp, sp, 3)
    return T


def _planar(x, y, yaw):
    T = np.eye(4)
    T[:3, :3] = _exp(np.array([0.0, 0.0, yaw]))
    T[:3, 3] = (x, y, 0.0)
    return T


def _inv(T):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3])
    return out


def _t12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def _mat(t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.asarray(t[:9]).reshape(3, 3), t[9:12]
    return M


def timed(torch, reps, call, warm=2):
    ts = []
    for k in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def one_group(liw, synth, M, N, rng):
    """one group's data: per robot the graph FleetBackEnd.load_graph takes, the starting T_g_w, and the 3 M cross edges (a, q, b, i, tf12)"""
    lib = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def pose_of(T):
        t, p, q = np.ascontiguousarray(_t12(T)), np.zeros(3), np.zeros(3)
        lib.liw_lie_log_SE3(pd(t), pd(p), pd(q))
        return np.concatenate([p, q])
    Tio_inv = _inv(synth.normalize_extrinsic(synth.office_params()["T_imu_to_wheel"]))
    graphs, X, T0 = [], [], []
    for r in range(M):
        W = _planar(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.5, 0.5))
        x, y, yaw, rate = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), 1.8 / N * (1 if r % 2 else -1)
        Xr = []
        for k in range(N):
            Xr.append(_planar(x, y, yaw) @ Tio_inv)
            x, y, yaw = x + 0.2 * math.cos(yaw), y + 0.2 * math.sin(yaw), yaw + rate
        S = [_inv(Xr[k - 1]) @ Xr[k] @ _small(rng, 2e-3, 1e-3) for k in range(1, N)]
        Pr = [_inv(W) @ Xr[0]]
        for s in S:
            Pr.append(Pr[-1] @ s)
        loops = [(N - 1, N // 10), (N // 2, N // 5)]
        graphs.append(dict(poses=np.array([pose_of(T) for T in Pr]), seq_tf12=np.array([_t12(s) for s in S]), loop_idx=np.array(loops, np.int32),
                           loop_tf12=np.array([_t12(_inv(Xr[i1]) @ Xr[i2] @ _small(rng, 1e-3, 2e-4)) for i1, i2 in loops])))
        X.append(Xr)
        T0.append(W if r == 0 else W @ _small(rng, 0.02, 0.005))
    cross = []
    for ring in (1, 2, 3):
        for a in range(M):
            b = (a + ring) % M
            if b == a:
                b = (a + 1) % M
            q, i = (7 * ring + 3 * a) % N, (11 * ring + 5 * a + 1) % N
            cross.append((ring, a, q, b, i, _t12(_inv(X[a][q]) @ X[b][i] @ _small(rng, 1e-3, 2e-4))))
    return graphs, T0, cross


def build(liw, synth, gg, gj, G, M, N):
    import torch
    rng = np.random.default_rng(7)
    B = G * M
    prm, pg = synth.office_params(), liw.posegraph.office_pg_params()
    graphs, T0, cross = one_group(liw, synth, M, N, rng)
    # the detector only lends the aligner its handle: a small store
    fl = liw.FleetLoopDetector(prm, dict(liw.loop.office_loop_params(), submap_count=1, min_interval=2), dict(B=B, max_keyframes=2, max_points=16, max_kf_corners=8))
    fb = liw.FleetBackEnd(prm, pg, dict(B=B, max_keyframes=N, max_loops=2), solve_period=1e9)
    for r in range(M):
        fb.load_graph(r, graphs[r])
    regions = fb.robot_regions()
    regions.view(G, M, -1)[1:] = regions[:M].clone()          # every group holds the first group's graphs
    al = liw.FleetGroupAligner(fl, np.repeat(np.arange(G), M), list(range(0, B, M)), 9, 0.01)       # the first robot of a group is its anchor
    al.linked.fill_(1)
    al.T_g_w.copy_(torch.tensor(np.tile(np.array([_t12(T) for T in T0]), (G, 1)), device=fb.dev))
    gr = gg.FleetGroupGraph(al, fb, M, 3 * M)
    for ring in (1, 2, 3):
        found, edge, tf12 = np.zeros(M, np.uint8), np.zeros((M, 4), np.int32), np.zeros((M, 12))
        for rg, a, q, b, i, t in cross:
            if rg == ring:
                found[a], edge[a], tf12[a] = 1, (q, b, i, 20), t
        et = np.tile(edge, (G, 1))
        et[:, 1] += np.repeat(np.arange(G) * M, M)
        gr.add_edges(dict(found=np.tile(found, G), edge=et, tf12=np.tile(tf12, (G, 1))))
    fixed = torch.zeros(B, dtype=torch.uint8, device=fb.dev)
    fixed[::M] = 1
    jt = gj.FleetGroupJoint(gr, fb, M * N, 2 * M + 3 * M)
    return fl, fb, al, gr, jt, fixed, pg


def baseline_solve(liw, pgraph, pg, fb, al, gr, g, M):
    """what the tree offers without the module: read everything back, concatenate, liw_posegraph_solve on the edge list"""
    lib = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    T = al.T_g_w[g * M:(g + 1) * M].cpu().numpy()
    x0, seq_idx, seq_tf, loop_idx, loop_tf, off = [], [], [], [], [], {}
    n = 0
    for m in range(M):
        r = g * M + m
        kf, st = fb.keyframes(r), fb.seq_edges(r)
        li, lt = fb.loop_edges(r)
        off[r] = n
        for p in kf["poses"]:
            tf, prod, pp, qq = np.zeros(12), np.zeros(12), np.zeros(3), np.zeros(3)
            lib.liw_lie_make_tf(pd(np.ascontiguousarray(p[:3])), pd(np.ascontiguousarray(p[3:])), pd(tf))
            lib.liw_lie_mul(pd(np.ascontiguousarray(T[m])), pd(tf), pd(prod))
            lib.liw_lie_log_SE3(pd(prod), pd(pp), pd(qq))
            x0.append(np.concatenate([pp, qq]))
        seq_idx += [(n + k, n + k + 1) for k in range(len(st))]
        seq_tf += list(st)
        loop_idx += [(n + int(a), n + int(b)) for a, b in li]
        loop_tf += list(lt)
        n += len(kf["poses"])
    idx, tf = gr.edges(g)
    for (a, q, b, i, size), t in zip(idx.tolist(), tf):
        loop_idx.append((off[a] + q, off[b] + i))
        loop_tf.append(t)
    return pgraph.solve(pg, np.array(x0), np.array(seq_idx, np.int32), np.array(seq_tf), np.array(loop_idx, np.int32), np.array(loop_tf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,64,1024")
    ap.add_argument("--members", default="2,4")
    ap.add_argument("--keyframes", default="50,200")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--baseline-groups", type=int, default=64)
    ap.add_argument("--baseline-reps", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--check-every", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_joint_bench.json"))
    a = ap.parse_args()
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    gg = importlib.import_module("2dliw-slam_amd.group_graph")
    gj = importlib.import_module("2dliw-slam_amd.group_joint")
    import torch
    lines = []
    for N in (int(v) for v in a.keyframes.split(",")):
        for M in (int(v) for v in a.members.split(",")):
            for G in (int(v) for v in a.groups.split(",")):
                fl, fb, al, gr, jt, fixed, pg = build(liw, synth, gg, gj, G, M, N)
                gsel = torch.ones(G, dtype=torch.uint8, device=fb.dev)
                ms = timed(torch, a.reps, lambda: jt.solve(gsel=gsel, fixed=fixed, check_every=a.check_every))
                sm, fl0 = jt.summaries(), jt.flags(0)
                its = max(s["iterations"] for s in sm)
                row = dict(bench="group_joint", device=torch.cuda.get_device_name(0), groups=G, members=M, keyframes=N, reps=a.reps, check_every=a.check_every,
                           joint=dict(solve_ms=ms[0], solve_ms_min=ms[1], solve_ms_max=ms[2], iterations=its, ms_per_iteration=ms[0] / max(its, 1),
                                      nodes=fl0["nodes"], loops=fl0["own_loops"] + fl0["used"], separators=fl0["separators"], solved=fl0["solved"],
                                      terminations=sorted(set(s["termination"] for s in sm)), final_cost=sm[0]["final_cost"],
                                      lds_triangle=bool(3 * fl0["separators"] * (6 * fl0["separators"] + 1) <= 8192), store_mib=jt.lay["bytes"] / 2 ** 20))
                if not a.no_baseline:
                    nb = min(G, a.baseline_groups)
                    pgraph = liw.posegraph.PoseGraph(synth.office_params())
                    out = []

                    def host_loop():
                        out[:] = [baseline_solve(liw, pgraph, pg, fb, al, gr, g, M)[1] for g in range(nb)]
                    bs = timed(torch, a.baseline_reps, host_loop, warm=1)
                    bits = max(s["iterations"] for s in out)
                    row["baseline"] = dict(groups_timed=nb, reps=a.baseline_reps, timed_ms=bs[0], solve_ms=bs[0] * G / nb, baseline_scaled=bool(nb < G), iterations=bits,
                                           ms_per_iteration=bs[0] * G / nb / max(bits, 1), terminations=sorted(set(s["termination"] for s in out)),
                                           final_cost=out[0]["final_cost"])
                    row["speedup"] = row["baseline"]["solve_ms"] / ms[0]
                print(json.dumps(row), flush=True)
                lines.append(row)
                for o in (jt, gr, fb, fl):
                    o.close()
                del fl, fb, al, gr, jt
                torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
