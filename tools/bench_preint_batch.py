"""Fleet pre-integration timing on the MI355X (include/liw_preint_batch.h): one frame of FleetPreint (push + commit) for B robots, each
with --imu IMU and --wheel wheel-odometry messages since its last scan (streams of 16 distinct trajectories, tiled over the fleet),
against the loop a caller of FleetTracker.step runs without it: read back bias(), a pair of ImuPreintegration / WheelPreintegration
handles per robot (add the messages, update_only_t, result, reset), upload the seven row arrays.

The host loop is linear in the robots by construction, so it is measured on at most --baseline-robots robots and scaled to B; the
JSON says which.  Wall times around torch.cuda.synchronize(), the median of --reps frames after one warm-up frame; the messages are
device tensors before the clock starts, as they are behind a device-side message queue (their upload is timed separately as
`upload_ms`).  The rows are printed as JSON lines and written to --out (profiles/fleet_preint_bench.json).
  python tools/bench_preint_batch.py --fleet 1,64,1024,16384 [--imu 20] [--wheel 2] [--reps 5]
Under rocprofv3 --kernel-trace --stats: --fleet 1024 --no-baseline --out ''."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def streams(synth, prm, n_traj, frames, n_imu, n_wheel, seed=11):
    """per trajectory and frame the message rows: imu [frames][n_imu, 7], wheel [frames][about n_wheel, 13]; stamps [frames].  The wheel
    messages come every 0.101 / n_wheel s (50.5 ms at two a frame, as the reference's odometry: just above the 0.05 s gate), so a
    frame holds n_wheel of them or one fewer; every trajectory has the same count in a frame"""
    import preint_batch_cases as pc
    rng = np.random.default_rng(seed)
    stamps = 1.0 + 0.1 * (1 + np.arange(frames))
    imu, wheel = [], []
    for j in range(n_traj):
        tr = synth._Truth(prm, yaw_rate=0.2 + 0.02 * j, radius=4.0 + 0.25 * j)
        imu.append([pc.imu_rows(tr, rng, t - 0.1, t, n_imu) for t in stamps])
        tw = 0.95 + 0.101 / max(n_wheel, 1) * np.arange(int(frames * n_wheel * 1.2) + 8) if n_wheel else np.zeros(0)
        wheel.append([pc.wheel_rows(tr, rng, tw[(tw > (t - 0.1 if k else 0.0)) & (tw <= t)]) for k, t in enumerate(stamps)])
    return stamps, imu, wheel


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleet", default="1,64,1024,16384")
    ap.add_argument("--imu", type=int, default=20)
    ap.add_argument("--wheel", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trajectories", type=int, default=16)
    ap.add_argument("--baseline-robots", type=int, default=64)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_preint_bench.json"))
    a = ap.parse_args()
    import torch
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    prm = synth.office_params()
    frames = a.reps + 1
    stamps, imu, wheel = streams(synth, prm, a.trajectories, frames, a.imu, a.wheel)
    rows = []
    for B in [int(v) for v in a.fleet.split(",")]:
        rob = np.arange(B) % a.trajectories
        fp = liw.FleetPreint(prm, B)
        bias = torch.zeros(B, 6, dtype=torch.float64, device="cuda")
        taken = torch.ones(B, dtype=torch.uint8, device="cuda")
        io = torch.as_tensor((a.imu * np.arange(B + 1)).astype(np.int32)).cuda()
        t_fleet, t_up, ready = [], [], 0
        for k in range(frames):
            im = np.stack([imu[j][k] for j in range(a.trajectories)])[rob].reshape(-1, 7)
            wm = np.stack([wheel[j][k] for j in range(a.trajectories)])[rob].reshape(-1, 13)
            wo = torch.as_tensor((len(wheel[0][k]) * np.arange(B + 1)).astype(np.int32)).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_im, d_wm, d_st = torch.as_tensor(im).cuda(), torch.as_tensor(wm).cuda(), torch.full((B,), float(stamps[k]), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            o = fp.push(io, d_im, wo, d_wm, d_st, bias)
            fp.commit(taken)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k:   # frame 0 is the warm-up (and seeds the accumulators)
                t_up.append((t1 - t0) * 1e3)
                t_fleet.append((t2 - t1) * 1e3)
            ready = int(o["ready"].sum())
        row = dict(bench="fleet_preint", B=B, imu=a.imu, wheel=a.wheel, trajectories=int(min(B, a.trajectories)), ready=ready,
                   store_MB=round(fp.lay["bytes"] / 1e6, 2), fleet_ms_per_frame=round(median(t_fleet), 4), upload_ms=round(median(t_up), 4),
                   fleet_us_per_robot=round(1e3 * median(t_fleet) / B, 3))
        if not a.no_baseline:
            nb = min(B, a.baseline_robots)
            acc = [(liw.ImuPreintegration(prm), liw.WheelPreintegration(prm)) for _ in range(nb)]
            x = torch.zeros(nb, 2, 15, dtype=torch.float64, device="cuda")   # stands for FleetTracker.x: bias() is a view of it
            t_host = []
            for k in range(frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bs = x[:, 1, 9:15].cpu().numpy()
                out = {key: np.zeros((nb, w)) for key, w in liw.preint_batch.ROW_WIDTH.items()}
                for b in range(nb):
                    pi, pw = acc[b]
                    for r in imu[rob[b]][k]:
                        pi.add_imu_measure(r[0], r[1:4], r[4:7])
                    for r in wheel[rob[b]][k]:
                        pw.add_wheel_odom_measure(r[0], r[1:10], r[10:13])
                    pw.update_only_t(stamps[k])
                    pi.update_only_t(stamps[k])
                    X, J, S, Dt = pi.get_preintegraption_result()
                    T, Sw, Dtw = pw.get_preintegraption_result()
                    out["imu_X"][b], out["imu_J"][b], out["imu_sqrtP"][b], out["imu_Dt"][b] = X, J.reshape(-1), S.reshape(-1), Dt
                    out["wheel_T"][b], out["wheel_sqrtP"][b], out["wheel_Dt"][b] = T, Sw.reshape(-1), Dtw
                    pw.reset_wheel_odom_measure(stamps[k])
                    pi.reset_imu_measure(stamps[k], bs[b, 0:3], bs[b, 3:6])
                dev = {key: torch.as_tensor(v).cuda() for key, v in out.items()}
                torch.cuda.synchronize()
                if k:
                    t_host.append((time.perf_counter() - t0) * 1e3)
            # the two sides got the same messages and resets: the last frame's rows agree
            agree = max(float((fp.rows[key].view(B, -1)[:nb] - dev[key].view(nb, -1)).abs().max() / dev[key].abs().max().clamp_min(1e-300))
                        for key in ("imu_X", "imu_J", "wheel_T"))
            host = median(t_host) * B / nb
            row.update(host_loop_ms_per_frame=round(host, 3), host_loop_robots_measured=nb, host_loop_scaled=bool(nb < B),
                       speedup=round(host / median(t_fleet), 1), rows_max_rel_diff=agree)
        fp.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
