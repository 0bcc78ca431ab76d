"""Loop detector timing on the MI355X (include/liw_loop.h): add_keyframe and detect against the number of stored key frames and the
points per sub-map.

Every key frame sees a slice of one static scene of P points (config/office.yaml values, submap_count = 30), so each sub-map holds
exactly P points after de-duplication and every candidate passes the origin-distance gate: the worst case, in which all
(K - min_interval) / 11 candidates run on the device.  The calls are synchronous (they read their results back), so wall time is
device-synchronised.  Prints one JSON line per (K, P) with the task count and the fraction of tasks the quick filter removed.
  python tools/bench_loop.py [--keyframes 500,2000,5000] [--points 50,150,300] [--reps 5]
Under rocprofv3 --kernel-trace --stats, run a small case: --keyframes 500 --points 150."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(P, seed=0):
    """P points at least 0.2 m apart (no de-duplication), jittered on a 0.5 m grid"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(P)))
    g = np.arange(side) * 0.5
    X, Y = np.meshgrid(g, g)
    pts = np.stack([X.ravel(), Y.ravel()], axis=1)[:P] + rng.uniform(-0.15, 0.15, (P, 2))
    return np.concatenate([pts, np.zeros((P, 1))], axis=1)


def run(liw, synth, K, P, reps):
    lp = liw.loop
    p = lp.office_loop_params()
    det = lp.LoopDetector(synth.office_params(), p, dict(max_keyframes=K, max_points=P))
    S = scene(P)
    sc = p["submap_count"]
    slices = np.array_split(np.arange(P), sc)
    pose = np.eye(4)
    add_t = []
    for k in range(K):
        t0 = time.perf_counter()
        det.add_keyframe(pose, S[slices[k % sc]])
        if k >= K - 50:
            add_t.append(time.perf_counter() - t0)
    assert det.status(K - 1)["n_points"] == P
    det.detect()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        e = det.detect()
        ts.append(time.perf_counter() - t0)
    st = det.last_stats()
    return dict(keyframes=K, points=P, add_keyframe_ms=1e3 * float(np.median(add_t)), detect_ms=1e3 * float(np.median(ts)),
                detect_ms_min=1e3 * float(np.min(ts)), candidates=st["candidates"], launched=st["launched"], tasks=st["tasks"],
                quick_filtered=1.0 - st["quick_pass"] / max(1, st["tasks"]), accepted=st["accepted"], loop=None if e is None else [e["index1"], e["index2"], e["size"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="500,2000,5000")
    ap.add_argument("--points", default="50,150,300")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    for K in [int(v) for v in a.keyframes.split(",")]:
        for P in [int(v) for v in a.points.split(",")]:
            print(json.dumps(run(liw, synth, K, P, a.reps)), flush=True)


if __name__ == "__main__":
    main()
