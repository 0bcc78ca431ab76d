"""Localisation timing on the MI355X (include/liw_map_locate.h): FleetLocalizer.build of the fields of 16 rooms and FleetLocalizer.match
of Q queries against them, against what a user had without it: read the grid back and search on the host (the numpy restatement
of tests/map_locate_cases.py, which is vectorised over the points and the column shifts of a row).

Fixed settings: scans of --rays (1 080) rays cast in the 16 rooms of map_batch_cases.rooms(), tiled over the queries; each room's map
is --keyframes scans rendered by a FleetMapper; 41 angles (half a degree apart) and W = 20, so a query has 41 * 41 * 41 = 68 921
candidates; the priors are off by up to 0.5 m and 8 degrees.  Wall times around torch.cuda.synchronize(): the median, minimum and
maximum of --reps runs after one warm-up.  The host search is linear in the queries by construction, so it is measured on
--baseline-queries queries and scaled to Q; the JSON says so.  The rows are printed as JSON lines and written to --out
(profiles/map_locate_bench.json).
  python tools/bench_map_locate.py --queries 256,4096 [--reps 7]
Under rocprofv3 --kernel-trace --stats: --queries 4096 --no-baseline --reps 1 --out ''."""
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

N_THETA, STEP_DEG, W = 41, 0.5, 20


def scenes(n_rooms, K, n_rays, per_room, seed=5):
    """per room: K mapping scans with flat poses on the circle, and per_room query scans with their true poses"""
    import map_batch_cases as mc
    rng = np.random.default_rng(seed)
    tfs, pts, cnt = np.zeros((n_rooms, K, 12)), np.zeros((n_rooms, K, n_rays, 3)), np.zeros((n_rooms, K), np.int32)
    qpts, qcnt, qtrue = np.zeros((n_rooms, per_room, n_rays, 3)), np.zeros((n_rooms, per_room), np.int32), np.zeros((n_rooms, per_room, 3))
    for r, room in enumerate(mc.rooms(n_rooms)):
        for k in range(K):
            a = 2 * np.pi * k / K + 0.3 * r
            x, y, yaw = 5.0 * np.cos(a), 5.0 + 5.0 * np.sin(a), a + np.pi / 2
            s = mc.scan(room, x, y, yaw, n_rays, rng)
            cnt[r, k] = len(s)
            pts[r, k, :len(s)] = s
            tfs[r, k] = mc.tf12(x, y, yaw)
        for k in range(per_room):
            a = rng.uniform(-np.pi, np.pi)
            x, y, yaw = 4.0 * np.cos(a), 5.0 + 4.0 * np.sin(a), rng.uniform(-np.pi, np.pi)
            s = mc.scan(room, x, y, yaw, n_rays, rng)
            qcnt[r, k] = len(s)
            qpts[r, k, :len(s)] = s
            qtrue[r, k] = (x, y, yaw)
    return tfs, pts, cnt, qpts, qcnt, qtrue


def timed(fn, reps, torch):
    ts = []
    for rep in range(reps + 1):          # the first one warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="256,4096")
    ap.add_argument("--keyframes", type=int, default=12)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rooms", type=int, default=16)
    ap.add_argument("--per-room", type=int, default=4, help="distinct query scans per room")
    ap.add_argument("--baseline-queries", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_locate_bench.json"))
    a = ap.parse_args()
    if a.reps < 5 and not a.no_baseline:
        ap.error("--reps must be at least 5 for a timing that is kept")
    import torch
    import map_batch_cases as mc
    import map_locate_cases as lc
    liw = importlib.import_module("2dliw-slam_amd")
    synth = importlib.import_module("2dliw-slam_amd.synth")
    prm = synth.office_params()
    M, K, R = a.rooms, a.keyframes, a.rays
    tfs, pts, cnt, qpts, qcnt, qtrue = scenes(M, K, R, a.per_room)
    cells = 1 << 17                        # a 16 m room at 5 cm is 321 x 321 cells
    fm = liw.FleetMapper(prm, dict(resolution=0.05), dict(B=M, max_submaps=K, max_points=K * R, max_cells=cells, max_steps=1024))
    key = torch.ones(M, dtype=torch.uint8, device="cuda")
    d_pts, d_cnt = torch.as_tensor(pts).cuda(), torch.as_tensor(cnt).cuda()
    for k in range(K):
        fm.add_keyframes(key, d_pts[:, k], d_cnt[:, k])
    fm.render_tf(torch.as_tensor(tfs).cuda())
    assert fm.status.cpu().tolist() == [0] * M
    a0 = (np.arange(N_THETA) - (N_THETA - 1) // 2) * np.radians(STEP_DEG)
    table = np.ascontiguousarray(np.stack([np.cos(a0), np.sin(a0)], axis=1))
    rows = []
    for Q in [int(v) for v in a.queries.split(",")]:
        rng = np.random.default_rng(100 + Q)
        room_of, scan_of = np.arange(Q) % M, (np.arange(Q) // M) % a.per_room
        off = np.stack([rng.uniform(-0.5, 0.5, Q), rng.uniform(-0.5, 0.5, Q), np.radians(rng.uniform(-8.0, 8.0, Q))], axis=1)
        true = qtrue[room_of, scan_of]
        T0 = np.array([mc.tf12(t[0] + o[0], t[1] + o[1], t[2] + o[2]) for t, o in zip(true, off)])
        loc = liw.FleetLocalizer(fm, Q, max_theta=N_THETA, prm=prm)
        args = [torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (room_of.astype(np.int32), qpts[room_of, scan_of], qcnt[room_of, scan_of], T0, table)]
        t_build = timed(lambda: loc.build(), a.reps, torch)
        t_match = timed(lambda: loc.match(*args, W), a.reps, torch)
        best, stats, found = loc.best.cpu().numpy(), loc.stats.cpu().numpy(), loc.found.cpu().numpy()
        # the best candidate against the truth: whole cells and table steps
        ex = np.abs(best[:, 1] * 0.05 + off[:, 0]) / 0.05
        ey = np.abs(best[:, 2] * 0.05 + off[:, 1]) / 0.05
        et = np.abs((best[:, 0] - (N_THETA - 1) // 2) * np.radians(STEP_DEG) + off[:, 2]) / np.radians(STEP_DEG)
        near = (ex <= 1.0) & (ey <= 1.0) & (et <= 1.0)
        lookups = float(stats[:, 1].astype(np.int64).sum()) * N_THETA * (2 * W + 1) ** 2
        info = loc.field_info(0)
        row = dict(bench="map_locate", Q=Q, maps=M, rays=R, n_theta=N_THETA, W=W, candidates_per_query=N_THETA * (2 * W + 1) ** 2,
                   mean_valid_points=round(float(stats[:, 1].mean()), 1), grid="%d x %d" % (info["width"], info["height"]),
                   status_ok=bool((stats[:, 0] == 0).all()), found=int(found.sum()), unique_maximum=int((stats[:, 2] == 1).sum()),
                   within_one_cell_and_step=int(near.sum()), store_MB=round(loc.lay["bytes"] / 1e6, 2), reps=a.reps,
                   build_ms=round(t_build[0] * 1e3, 3), build_ms_min=round(t_build[1] * 1e3, 3), build_ms_max=round(t_build[2] * 1e3, 3),
                   build_us_per_map=round(t_build[0] * 1e6 / M, 2),
                   match_ms=round(t_match[0] * 1e3, 3), match_ms_min=round(t_match[1] * 1e3, 3), match_ms_max=round(t_match[2] * 1e3, 3),
                   match_us_per_query=round(t_match[0] * 1e6 / Q, 2), field_lookups_G=round(lookups / 1e9, 2),
                   field_lookups_G_per_s=round(lookups / 1e9 / t_match[0], 1))
        if not a.no_baseline:
            nq = min(Q, a.baseline_queries)
            t0 = time.perf_counter()
            same = True
            for q in range(nq):
                m = int(room_of[q])
                grid, gi = fm.grid(m), fm.info_of(m)                                   # the read-back is part of it
                r = lc.match_one(lc.field_of(grid), gi, qpts[m, scan_of[q], :qcnt[m, scan_of[q]]], T0[q], table, W)
                same &= bool(np.array_equal(r["best"], best[q]) and np.array_equal(r["stats"], stats[q]))
            t_host = (time.perf_counter() - t0) / nq
            row.update(host_ms_per_query=round(t_host * 1e3, 1), host_queries_measured=nq, host_s_scaled_to_Q=round(t_host * Q, 1), host_scaled=bool(nq < Q),
                       device_equals_host_on_measured=same, speedup_scaled=round(t_host * Q / t_match[0], 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        loc.close()
        del loc, args
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
