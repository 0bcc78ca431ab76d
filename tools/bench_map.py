"""Occupancy-grid map render time on the MI355X (include/liw_map.h): K key frames x 1 080 rays for a room (8 x 6 m) and a long
corridor (60 x 3 m), K in {200, 2 000}.

The robot drives a loop inside the room / up and down the corridor; every key frame's scan is cast from its true pose and
rendered at that pose plus a few millimetres of noise and a small roll / pitch, as corrected back-end poses would be.  The
points are uploaded once; a render is one synchronous call (it reads the counters back), so wall time is device-synchronised.
Prints one JSON line per shape: render time (median / min of --reps after a warm-up), samples and samples/s, the cell visits
left after the repeat filter and the SAMPLED / HIT atomics actually issued (counted by k_map_rays itself), and with --serial the
1-core time of the literal serial walk (tests/cpp/map_serial.cpp, built with the host compiler) on the same input, that time / 16
(the best a threaded host version could do on the 16 CPUs of a job) and whether the two grids are identical.
  python tools/bench_map.py [--keyframes 200,2000] [--rays 1080] [--shapes room,corridor] [--reps 10] [--serial]
Under rocprofv3 --kernel-trace --stats run one shape: --keyframes 2000 --shapes room --reps 5 (without --serial)."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box(x0, y0, x1, y1):
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [(np.array(c[k], dtype=np.float64), np.array(c[(k + 1) % 4], dtype=np.float64)) for k in range(4)]


def shape(name):
    """wall segments and the path pose(u), u in [0, 1)"""
    if name == "room":
        segs = box(-4.0, -3.0, 4.0, 3.0) + box(-0.6, -0.4, 0.6, 0.4)
        return segs, lambda u: (2.6 * np.cos(2 * np.pi * u), 1.8 * np.sin(2 * np.pi * u), 2 * np.pi * u + np.pi / 2)
    if name == "corridor":
        segs = box(0.0, -1.5, 60.0, 1.5) + [s for x in range(5, 60, 10) for s in box(x, 1.0, x + 0.4, 1.5)]

        def pose(u):
            v = 2 * u if u < 0.5 else 2 - 2 * u
            return 1.0 + 58.0 * v, 0.3 * np.sin(40 * u), 0.0 if u < 0.5 else np.pi
        return segs, pose
    raise ValueError(name)


def make_input(replay, name, K, n_rays, seed=0):
    rng = np.random.default_rng(seed)
    segs, pose = shape(name)
    tfs, subs = [], []
    for k in range(K):
        x, y, yaw = pose(k / K)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        T[:2, 3] = (x, y)
        rg, amin, inc = replay.cast_scan_moving(segs, lambda t: T, 0.0, n_rays, 2 * np.pi * 0.75, 0.0, 0.004, rng, max_range=80.0)
        a = float(amin) + float(inc) * np.arange(n_rays)
        ok = np.isfinite(rg) & (rg > 0.1)
        r = rg[ok].astype(np.float64)
        subs.append(np.stack([r * np.cos(a[ok]), r * np.sin(a[ok]), np.zeros(r.size)], axis=1))
        yaw += rng.normal(0, 0.002)
        roll, pitch = rng.normal(0, 0.003, 2)
        Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
        Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        tfs.append(np.concatenate([(Rz @ Ry @ Rx).reshape(9), [x + rng.normal(0, 0.005), y + rng.normal(0, 0.005), rng.normal(0, 0.005)]]))
    return np.array(tfs), subs


def run(liw, synth, replay, name, K, n_rays, reps, serial):
    tfs, subs = make_input(replay, name, K, n_rays)
    npts = sum(s.shape[0] for s in subs)
    m = liw.gridmap.GridMap(synth.office_params(), dict(resolution=0.05), dict(max_submaps=K, max_points=npts, max_cells=1 << 23))
    t0 = time.perf_counter()
    for s in subs:
        m.add_submap(s)
    upload = time.perf_counter() - t0
    info = m.render_tf(tfs)   # warm-up (also uploads the step table)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.render_tf(tfs)
        ts.append(time.perf_counter() - t0)
    pc = m.probe_counts()
    med = float(np.median(ts))
    out = dict(shape=name, keyframes=K, rays=info["rays"], width=info["width"], height=info["height"], samples=info["samples"],
               samples_per_ray=info["samples"] / max(1, info["rays"]), upload_ms=1e3 * upload, render_ms=1e3 * med, render_ms_min=1e3 * float(np.min(ts)),
               samples_per_s=info["samples"] / med, cell_visits=pc["visits"], atomics=pc["atomics"], hit_atomics=pc["hit_atomics"],
               atomics_per_visit=pc["atomics"] / max(1, pc["visits"]), visits_per_s=pc["visits"] / med,
               cells=dict(unknown=info["unknown"], free=info["free_cells"], hit_once=info["hit_once"], hit_more=info["hit_more"]))
    if serial:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import map_reference as ref
        with tempfile.TemporaryDirectory() as d:
            L = ref.build_serial(d)
            t0 = time.perf_counter()
            want = ref.render_serial(L, tfs, subs, 0.05)
            st = time.perf_counter() - t0
        out.update(serial_1core_ms=1e3 * st, serial_over_16_ms=1e3 * st / 16, speedup_vs_1core=st / med, speedup_vs_16=st / 16 / med,
                   identical=bool(np.array_equal(want["grid"], m.grid()) and want["samples"] == info["samples"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="200,2000")
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--shapes", default="room,corridor")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--serial", action="store_true")
    a = ap.parse_args()
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    replay = importlib.import_module("2dliw-slam_amd.replay")
    for name in a.shapes.split(","):
        for K in [int(v) for v in a.keyframes.split(",")]:
            print(json.dumps(run(liw, synth, replay, name, K, a.rays, a.reps, a.serial)), flush=True)


if __name__ == "__main__":
    main()
