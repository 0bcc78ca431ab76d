"""Loop detector timing on the MI355X (include/liw_loop.h): add_keyframe and detect against the number of stored key frames and the
points per sub-map.

Every key frame sees a slice of one static scene of P points (config/office.yaml values, submap_count = 30), so each sub-map holds
exactly P points after de-duplication and every candidate passes the origin-distance gate: the worst case, in which all
(K - min_interval) / 11 candidates run on the device.  The calls are synchronous (they read their results back), so wall time is
device-synchronised.  Prints one JSON line per (K, P) with the task count and the fraction of tasks the quick filter removed.
  python tools/bench_loop.py [--keyframes 500,2000,5000] [--points 50,150,300] [--reps 5]
Under rocprofv3 --kernel-trace --stats, run a small case: --keyframes 500 --points 150.

--fleet B[,B...] times the fleet detector instead (include/liw_loop_batch.h): FleetLoopDetector.push (add_keyframes + detect) per
frame for B robots against the only way to do it without it, one LoopDetector per robot driven from a host loop on the same key
frames.  Every robot holds --preload key frames (default 120: two candidates at the office min_interval of 100), then --frames frames
are timed in which a fraction --key-fraction of the robots (staggered) has a key frame.  The host loop is linear in the robots by
construction (serial, a synchronising read-back per call), so it is measured on at most --baseline-robots detectors and scaled to
B; the JSON says which.  Wall times around torch.cuda.synchronize().  One JSON line per (B, P, fraction).
  python tools/bench_loop.py --fleet 1,64,1024,4096 [--points 10,150] [--key-fraction 1.0,0.25] [--frames 12] [--no-baseline]
--fleet B[,B...] --cross times liw_xloop_detect (include/liw_loop_cross.h; robots paired 2j <-> 2j + 1, every odd robot queries its even
partner) beside FleetLoopDetector.detect for the same robots of the same store, and writes the lines to profiles/fleet_cross_loop_bench.json.
Under rocprofv3 --kernel-trace --stats: --fleet 1024 --points 150 --key-fraction 1.0 --no-baseline."""
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
    return dict(keyframes=K, points=P, add_keyframe_ms=1e3 * float(np.median(add_t)), add_keyframe_ms_min=1e3 * float(np.min(add_t)),
                add_keyframe_ms_max=1e3 * float(np.max(add_t)), detect_ms=1e3 * float(np.median(ts)),
                detect_ms_min=1e3 * float(np.min(ts)), detect_ms_max=1e3 * float(np.max(ts)), candidates=st["candidates"], launched=st["launched"], tasks=st["tasks"],
                quick_filtered=1.0 - st["quick_pass"] / max(1, st["tasks"]), accepted=st["accepted"], loop=None if e is None else [e["index1"], e["index2"], e["size"]])


def run_fleet(liw, synth, B, P, frac, preload, frames, baseline_robots):
    import torch
    lp = liw.loop
    p = lp.office_loop_params()
    sc = p["submap_count"]
    K = preload + frames + 2                      # the two warm-up frames add key frames too
    S = scene(P)
    slices = np.array_split(np.arange(P), sc)
    stride = max(len(s) for s in slices)
    fl = liw.FleetLoopDetector(synth.office_params(), p, dict(B=B, max_keyframes=K, max_points=P, max_kf_corners=stride))
    pose = torch.zeros(B, 6, dtype=torch.float64, device="cuda")

    def corners(k):
        c = S[slices[k % sc]]
        a = np.zeros((stride, 3))
        a[:len(c)] = c
        return torch.from_numpy(a).cuda().expand(B, stride, 3).contiguous(), torch.full((B,), len(c), dtype=torch.int32, device="cuda")

    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    for k in range(preload):
        acc, n = corners(k)
        fl.add_keyframes(ones, pose, acc, n)
    period = max(1, int(round(1.0 / frac)))
    nk = np.full(B, preload)                      # key frames per robot
    keys, ts, found = [], [], 0
    for f in range(frames + 2):                   # two warm-up frames
        key = ((np.arange(B) + f) % period == 0)
        # every keyed robot is at the same key-frame count only when period == 1; the corner slice follows the robot's own count
        acc = np.zeros((B, stride, 3))
        n = np.zeros(B, np.int32)
        for b in np.nonzero(key)[0]:
            c = S[slices[nk[b] % sc]]
            acc[b, :len(c)], n[b] = c, len(c)
        inp = dict(key=torch.from_numpy(key.astype(np.uint8)).cuda(), pose=pose, acc=torch.from_numpy(acc).cuda(), n_acc=torch.from_numpy(n).cuda())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fl.push(inp)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        nk[key] += 1
        if f >= 2:
            ts.append(dt)
            keys.append(int(key.sum()))
            found += int(out["found"].sum())
    stats = out["stats"].cpu().numpy()
    lay = fl.lay
    r = dict(fleet=B, points=P, key_fraction=frac, preload=preload, frames=frames, keyed_per_frame=float(np.mean(keys)),
             fleet_ms=1e3 * float(np.median(ts)), fleet_ms_min=1e3 * float(np.min(ts)), fleet_ms_max=1e3 * float(np.max(ts)), found=found,
             candidates_per_robot=int(stats[:, 0].max()), tasks_per_robot=int(stats[:, 2].max()), robot_bytes=lay["robot_bytes"],
             scratch_bytes_per_robot=lay["scratch_bytes"] // B, single_store_bytes=lp.store_bytes(p, dict(max_keyframes=K, max_points=P)))
    fl.close()
    if baseline_robots > 0:
        nb = min(B, baseline_robots)
        dets = [lp.LoopDetector(synth.office_params(), p, dict(max_keyframes=K, max_points=P)) for _ in range(nb)]
        for d in dets:
            for k in range(preload):
                d.add_keyframe(np.eye(4), S[slices[k % sc]])
        per = []                                   # seconds per keyed robot: add_keyframe + detect, as the host loop runs them
        nkb = np.full(nb, preload)
        for f in range(frames + 2):
            key = ((np.arange(nb) + f) % period == 0)
            t0 = time.perf_counter()
            for b in np.nonzero(key)[0]:
                dets[b].add_keyframe(np.eye(4), S[slices[nkb[b] % sc]])
                dets[b].detect()
            dt = time.perf_counter() - t0
            nkb[key] += 1
            if f >= 2 and key.any():
                per.append(dt / int(key.sum()))
        base = float(np.median(per)) * r["keyed_per_frame"]
        r.update(baseline_robots_measured=nb, baseline_scaled=nb < B, baseline_ms_per_keyed_robot=1e3 * float(np.median(per)),
                 baseline_ms_per_keyed_robot_min=1e3 * float(np.min(per)), baseline_ms_per_keyed_robot_max=1e3 * float(np.max(per)),
                 baseline_ms=1e3 * base, ratio=1e3 * base / r["fleet_ms"])
    return r


def run_cross(liw, synth, B, P, preload, frames):
    """liw_xloop_detect (robots paired 2j <-> 2j + 1, every odd robot queries its even partner) beside FleetLoopDetector.detect for the
    same odd robots of the same store, in one process.  min_interval = 1, so that own detection walks the same candidate slots but
    the newest one: the same match bodies over (nearly) the same task counts."""
    import torch
    lp = liw.loop
    p = dict(lp.office_loop_params(), min_interval=1)
    sc = p["submap_count"]
    S = scene(P)
    slices = np.array_split(np.arange(P), sc)
    stride = max(len(s) for s in slices)
    fl = liw.FleetLoopDetector(synth.office_params(), p, dict(B=B, max_keyframes=preload, max_points=P, max_kf_corners=stride))
    pose = torch.zeros(B, 6, dtype=torch.float64, device="cuda")
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    for k in range(preload):
        c = S[slices[k % sc]]
        a = np.zeros((stride, 3))
        a[:len(c)] = c
        fl.add_keyframes(ones, pose, torch.from_numpy(a).cuda().expand(B, stride, 3).contiguous(), torch.full((B,), len(c), dtype=torch.int32, device="cuda"))
    odd = (np.arange(B) % 2 == 1) & (np.arange(B) < B - B % 2 + 1)
    key = torch.from_numpy(odd.astype(np.uint8)).cuda()
    partner = torch.from_numpy(np.where(odd, np.arange(B) - 1, -1).astype(np.int32)).cuda()
    al = liw.FleetGroupAligner(fl, np.zeros(B, np.int32), [0], p["min_match_threshold"], 0.05)
    res = {}
    for name, fn in (("cross", lambda: al.detect_cross(key, partner)), ("detect", lambda: fl.detect(key))):
        ts = []
        for f in range(frames + 2):               # two warm-up calls
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if f >= 2:
                ts.append(time.perf_counter() - t0)
        st = out["stats"].cpu().numpy()[odd] if odd.any() else np.zeros((1, 6), np.int64)
        res[name] = dict(ms=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), ms_max=1e3 * float(np.max(ts)), found=int(out["found"].sum()),
                         candidates_per_robot=int(st[:, 0].max()), launched_per_robot=int(st[:, 1].max()), tasks_per_robot=int(st[:, 2].max()))
    fl.close()
    return dict(fleet=B, points=P, preload=preload, frames=frames, queries=int(odd.sum()), cross=res["cross"], detect=res["detect"],
                ratio=res["cross"]["ms"] / res["detect"]["ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="500,2000,5000")
    ap.add_argument("--points", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fleet", default=None, help="robots, comma separated: time the fleet detector against a host loop of single detectors")
    ap.add_argument("--key-fraction", default="1.0,0.25")
    ap.add_argument("--preload", type=int, default=120)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--baseline-robots", type=int, default=64)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--cross", action="store_true", help="with --fleet: time liw_xloop_detect (2j <-> 2j + 1, odd robots query) beside detect")
    a = ap.parse_args()
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    if a.fleet and a.cross:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "fleet_cross_loop_bench.json"), "w") as f:
            for B in [int(v) for v in a.fleet.split(",")]:
                for P in [int(v) for v in (a.points or "10,150").split(",")]:
                    line = json.dumps(run_cross(liw, synth, B, P, a.preload, a.frames))
                    print(line, flush=True)
                    f.write(line + "\n")
        return
    if a.fleet:
        for B in [int(v) for v in a.fleet.split(",")]:
            for P in [int(v) for v in (a.points or "10,150").split(",")]:
                for frac in [float(v) for v in a.key_fraction.split(",")]:
                    print(json.dumps(run_fleet(liw, synth, B, P, frac, a.preload, a.frames, 0 if a.no_baseline else a.baseline_robots)), flush=True)
        return
    a.points = a.points or "50,150,300"
    for K in [int(v) for v in a.keyframes.split(",")]:
        for P in [int(v) for v in a.points.split(",")]:
            print(json.dumps(run(liw, synth, K, P, a.reps)), flush=True)


if __name__ == "__main__":
    main()
