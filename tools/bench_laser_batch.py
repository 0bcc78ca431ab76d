"""Device time of the batched laser front-end (laser_batch.BatchFrontEnd) per stage, one JSON line.

B robots (default 4 096 and 49 152) with 1 080-ray scans tiled from 64 distinct rooms / poses.  Per B: ranges -> points, spawn
(spawn_ms: the default wave-per-scan kernel, with min / max of the repetitions; spawn_lane_ms: the lane-per-scan kernel selected
by LIW_LFE_SPAWN=lane; spawn_corners_ms: the default kernel also writing the corners, corners_per_robot of them),
match against the reference sub-map, add_scan (the accumulating call: the reference exists; add_scan_ms: the default
wave-per-robot kernel, add_scan_lane_ms: the lane-per-robot kernel selected by LIW_LFE_ADD_SCAN=lane, both with min / max, and
add_scan_path: what the default dispatch ran, 1 = wave) and pack_track, each timed with
HIP events on the current stream (median of --reps after one warm-up); scans/s = B / ms.  For comparison the same line carries
the host front-end (liw.laser through ctypes) per scan over 256 robots: laser_to_points, Scan.spawn, match_with_ref, add_scan.

--init N adds the initialisation of a fleet (key "init", per B of --init-B): N scans per robot in N scan slots, then
match_front_ms (F = N - 1 frames against slot 0 in one launch of the wave-per-(robot, frame) kernel), lane_match_ms (the same
work as N - 1 calls of the lane-per-robot match, outputs reused), pack_init_ms (incl. the Ltot read-back), rebuild_ms (the default:
one launch of the wave-per-robot add_scan kernel) and rebuild_lane_ms (LIW_LFE_ADD_SCAN=lane: the reset and N launches), each
with min / max, the ratios lane / wave, and whether the two paths' counts and rebuilt stores' headers agree.  --B "" runs that leg alone.

--track K adds the tracking frame of a fleet (key "track", per B of --track-B): K fleet.FleetTracker.step frames (track_begin ->
ranges_to_points -> deskew -> spawn_corners -> match -> pack_track -> solve(TRACK) -> marginalize -> track_end -> corners_to_world
-> add_scan) on --track-distinct trajectories of synth.make_window with scans cast from their truth poses in the tool's rooms.
frame_ms: the median over the K frames of a host clock around step + synchronise, per repetition; its median / min / max over
--reps repetitions after one warm-up run.  track_begin_ms / track_end_ms: the two glue kernels alone (HIP events).  host_glue: the
baseline without them, the same stages with the glue done on the host from read-backs (tests/track_glue_reference.py
HostGlueTracker: a loop over the robots through liw_lie_*), frame_ms over --track-host-frames frames of one run, and whether the
two sides' key / skip decisions agree on those frames.

--cold-start N adds the cold start of a fleet (key "cold_start", per B of --cold-B): fleet.FleetTrajectory from reset(), windows of N
frames, robot b starting to move b % 4 frames late (until then it is dropped by the motion gate).  cold: the N + 3 frames until the
last robot tracks, frame_ms per frame (median over --reps runs after one warm-up, host clock around step + synchronise), their sum
first_scan_to_tracking_ms with min / max over the runs, and per frame with an INIT solve the ready robots R and the bucket.
all_tracking: the --cold-frames frames after that through FleetTrajectory.step and, from a copy of the same state and on the same
inputs, through FleetTracker.step (median / min / max over --reps of the per-run median frame).  mixed: the same frames after a
quarter of the robots was put back to INITIALIZING and kept at rest: frame_ms, and the LM iterations of the tracking solve per
group of rows (robots that track / robots that do not).  host_glue: the baseline with every piece of glue on the host from
read-backs (tests/fleet_init_reference.py HostGlueTrajectory: a Python loop over the robots), the same N + 3 frames from reset in one
run (--cold-host-frames fewer), per frame and in total, beside the device's total over the same frames; at the first B only.

  python tools/bench_laser_batch.py [--B 4096,49152] [--reps 5] [--init 30 [--init-B 4096]] [--track 8 [--track-B 4096,49152]]
                                    [--cold-start 4 [--cold-B 4096,49152] [--cold-frames 4] [--cold-host-frames -1]]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_RAYS = 1080
ANG_MIN = np.float32(-2.0 * np.pi * 0.75 / 2)
ANG_INC = np.float32(2.0 * np.pi * 0.75 / (N_RAYS - 1))
T_INC = np.float32(1.0 / (40.0 * N_RAYS))


def _T(p, q):
    th = np.linalg.norm(q)
    R = np.eye(3)
    if th > 1e-15:
        k = q / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, p
    return T


def scenes(liw, lp, nd, seed=4242):
    """nd distinct (ranges at pose a, ranges at pose b, pose a, pose b)"""
    rng = np.random.default_rng(seed)
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    ra, rb, pa, pb = [], [], [], []
    for j in range(nd):
        segs = liw.laser.room_segments(5000 + j)
        a = np.concatenate([rng.uniform(-1, 1, 2), [0.0, 0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
        b = a.copy()
        b[:2] += rng.uniform(-0.15, 0.15, 2)
        b[5] += rng.uniform(-0.07, 0.07)
        ra.append(liw.laser.cast_scan(segs, _T(a[:3], a[3:]) @ Til, n_rays=N_RAYS, seed=2 * j)[0])
        rb.append(liw.laser.cast_scan(segs, _T(b[:3], b[3:]) @ Til, n_rays=N_RAYS, seed=2 * j + 1)[0])
        pa.append(a)
        pb.append(b)
    return np.stack(ra), np.stack(rb), np.stack(pa), np.stack(pb)


def timed(torch, fn, reps, spread=None):
    """median of reps (after one warm-up); spread: a list that receives (min, max)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    if spread is not None:
        spread[:] = [float(min(ts)), float(max(ts))]
    return float(np.median(ts))


def with_env(name, value, fn):
    """fn() with the environment variable set (the library reads its A/B knobs per call)"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def device_run(liw, torch, lp, B, sc, reps, cap=256, max_corners=64):
    ra, rb, pa, pb = sc
    nd = ra.shape[0]
    rob = np.arange(B) % nd
    fe = liw.laser_batch.BatchFrontEnd(lp, dict(B=B, slots=2, max_points=N_RAYS, max_lines=256, max_cell_entries=8192))
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    RA = torch.from_numpy(ra).cuda()[torch.from_numpy(rob).cuda()].contiguous()
    RB = torch.from_numpy(rb).cuda()[torch.from_numpy(rob).cuda()].contiguous()
    PA, PB = torch.from_numpy(pa[rob]).cuda(), torch.from_numpy(pb[rob]).cuda()
    stamps = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = {}
    a = fe.ranges_to_points(RA, stamps)
    b = fe.ranges_to_points(RB, stamps)
    out["ranges_to_points_ms"] = timed(torch, lambda: fe.ranges_to_points(RB, stamps, out=b), reps)
    # spawn: the default (wave-per-scan) kernel, the lane-per-scan kernel behind the knob, and the default kernel with corners
    sp = []
    out["spawn_ms"] = timed(torch, lambda: fe.spawn(1, b[0], b[2]), reps, sp)
    out["spawn_min_ms"], out["spawn_max_ms"] = sp
    out["spawn_lane_ms"] = with_env("LIW_LFE_SPAWN", "lane", lambda: timed(torch, lambda: fe.spawn(1, b[0], b[2]), reps, sp))
    out["spawn_lane_min_ms"], out["spawn_lane_max_ms"] = sp
    cbuf = fe.spawn(1, b[0], b[2], corners=max_corners)
    out["spawn_corners_ms"] = timed(torch, lambda: fe.spawn(1, b[0], b[2], corners=max_corners, out=cbuf), reps, sp)
    out["spawn_corners_min_ms"], out["spawn_corners_max_ms"] = sp
    out["corners_per_robot"] = float(cbuf[1].clamp(max=max_corners).sum().item()) / B

    def fresh():   # reset, both scans spawned, the first scan added (the reference sub-map exists)
        fe.reset()
        fe.spawn(0, a[0], a[2])
        fe.spawn(1, b[0], b[2])
        fe.add_scan(0, PA)

    def add_b():   # the accumulating add_scan; the first-scan call is not part of the timing
        fresh()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fe.add_scan(1, PB)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    def add_timed(key):
        add_b()
        ts = [add_b() for _ in range(reps)]
        out[key + "_ms"], out[key + "_min_ms"], out[key + "_max_ms"] = float(np.median(ts)), float(min(ts)), float(max(ts))
    add_timed("add_scan")
    out["add_scan_path"] = fe.add_scan_path()
    with_env("LIW_LFE_ADD_SCAN", "lane", lambda: add_timed("add_scan_lane"))
    out["add_scan_lane_over_default"] = out["add_scan_lane_ms"] / out["add_scan_ms"]
    fresh()
    m = fe.match_with_ref(1, PB, cap=cap)
    mbufs = {k: m[k] for k in ("count", "recs", "idx1", "idx2", "match_pose")}   # outputs allocated outside the timed region
    out["match_with_ref_ms"] = timed(torch, lambda: fe.match(liw.laser_batch.REF, 1, None, PB, 0, cap, out=mbufs), reps)
    pk, Ltot = fe.pack_track(m)
    bufs = dict(laser_off=pk["laser_off"], laser_frame=torch.empty(B * cap, dtype=torch.int32, device="cuda"),
                laser_pts=torch.empty(12 * B * cap, dtype=torch.float64, device="cuda"))
    mo = dict(match_pose=pk["match_pose"], has_match=pk["has_match"])
    out["pack_track_ms"] = timed(torch, lambda: fe.pack_track(m, out=mo, bufs=bufs), reps)   # includes the Ltot read-back
    out["frame_ms"] = out["ranges_to_points_ms"] + out["spawn_ms"] + out["match_with_ref_ms"] + out["add_scan_ms"] + out["pack_track_ms"]
    for k in ("ranges_to_points", "spawn", "match_with_ref", "add_scan", "pack_track", "frame"):
        out[k + "_scans_per_s"] = B / (out[k + "_ms"] * 1e-3)
    out["Ltot"] = int(Ltot)
    out["pairs_per_robot"] = Ltot / B
    del fe
    torch.cuda.empty_cache()
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def init_scenes(liw, lp, nd, N, seed=4343):
    """nd distinct windows of N scans: (ranges [nd, N, n_rays], poses [nd, N, 6]), frame 0 the front key frame"""
    rng = np.random.default_rng(seed)
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    R, Pq = np.zeros((nd, N, N_RAYS), dtype=np.float32), np.zeros((nd, N, 6))
    for j in range(nd):
        segs = liw.laser.room_segments(6000 + j)
        a = np.concatenate([rng.uniform(-1, 1, 2), [0.0, 0.0, 0.0], rng.uniform(-np.pi, np.pi, 1)])
        for k in range(N):
            if k:   # a walk away from the front pose, a few centimetres and degrees per frame
                a = a.copy()
                a[:2] += rng.uniform(-0.03, 0.03, 2)
                a[5] += rng.uniform(-0.02, 0.02)
            R[j, k] = liw.laser.cast_scan(segs, _T(a[:3], a[3:]) @ Til, n_rays=N_RAYS, seed=100 * j + k)[0]
            Pq[j, k] = a
    return R, Pq


def init_run(liw, torch, lp, B, N, nd, reps, cap=256):
    R, Pq = init_scenes(liw, lp, nd, N)
    rob = torch.from_numpy(np.arange(B) % nd).cuda()
    dims = dict(B=B, slots=N, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)
    fe = liw.laser_batch.BatchFrontEnd(lp, dims)
    fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    stamps = torch.zeros(B, dtype=torch.float64, device="cuda")
    Rd = torch.from_numpy(R).cuda()
    buf = None
    for k in range(N):
        buf = fe.ranges_to_points(Rd[:, k][rob].contiguous(), stamps, out=buf)
        fe.spawn(k, buf[0], buf[2])
    poses = torch.from_numpy(Pq).cuda()[rob].contiguous()           # [B, N, 6]
    pf, pk = poses[:, 0].contiguous(), [poses[:, k].contiguous() for k in range(N)]
    F = N - 1
    out = dict(dims=dims, N=N, cap=cap, store_GB=round(fe.store.numel() / 1e9, 3))
    sp = []
    m = fe.match_front(0, 1, F, pf, poses[:, 1:], cap=cap)
    mb = {k: m[k] for k in ("count", "recs", "idx1", "idx2", "match_pose")}
    out["match_front_ms"] = timed(torch, lambda: fe.match_front(0, 1, F, pf, poses[:, 1:], cap=cap, out=mb), reps, sp)
    out["match_front_min_ms"], out["match_front_max_ms"] = sp
    l = fe.match(0, 1, pf, pk[1], cap=cap)
    lb_ = {k: l[k] for k in ("count", "recs", "idx1", "idx2", "match_pose")}
    counts = []
    for k in range(1, N):                                           # the lane path's counts, for the agreement flag
        counts.append(fe.match(0, k, pf, pk[k], cap=cap, out=lb_)["count"].clone())

    def lane_all():
        for k in range(1, N):
            fe.match(0, k, pf, pk[k], 0, cap, out=lb_)
    out["lane_match_ms"] = timed(torch, lane_all, reps, sp)
    out["lane_match_min_ms"], out["lane_match_max_ms"] = sp
    out["lane_over_wave"] = out["lane_match_ms"] / out["match_front_ms"]
    out["counts_agree"] = bool(torch.equal(torch.stack(counts, 1), m["count"].view(B, F)))
    pack, Ltot, ok = fe.pack_init(m, N, pf)
    bufs = dict(laser_off=pack["laser_off"], laser_frame=torch.empty(max(Ltot, 1), dtype=torch.int32, device="cuda"),
                laser_pts=torch.empty(12 * max(Ltot, 1), dtype=torch.float64, device="cuda"))
    po = dict(match_pose=pack["match_pose"], has_match=pack["has_match"], init_ok=ok)
    out["pack_init_ms"] = timed(torch, lambda: fe.pack_init(m, N, pf, out=po, L_cap=Ltot, bufs=bufs), reps, sp)
    out["pack_init_min_ms"], out["pack_init_max_ms"] = sp
    out["rebuild_ms"] = timed(torch, lambda: fe.rebuild(0, N, poses), reps, sp)
    out["rebuild_min_ms"], out["rebuild_max_ms"] = sp
    out["rebuild_path"] = fe.add_scan_path()
    torch.cuda.synchronize()
    mgr_default = fe.store.view(B, -1)[:, :256].clone()
    out["rebuild_lane_ms"] = with_env("LIW_LFE_ADD_SCAN", "lane", lambda: timed(torch, lambda: fe.rebuild(0, N, poses), reps, sp))
    out["rebuild_lane_min_ms"], out["rebuild_lane_max_ms"] = sp
    out["rebuild_lane_over_default"] = out["rebuild_lane_ms"] / out["rebuild_ms"]
    torch.cuda.synchronize()
    out["rebuild_managers_agree"] = bool(torch.equal(mgr_default, fe.store.view(B, -1)[:, :256]))
    out["Ltot"], out["pairs_per_frame"], out["init_ok"] = int(Ltot), Ltot / (B * F), int(ok.sum().item())
    del fe
    torch.cuda.empty_cache()
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def track_scenes(liw, synth, prm, lp, nd, K):
    """nd trajectories of K frames after the start frame: truth states, stamps, the intervals' arrays, scans cast from the truth"""
    hp = liw.HostPreint(prm)
    Til = synth.normalize_extrinsic(lp["T_imu_to_laser"])
    trajs = [synth.make_window(hp, prm, seed=8100 + j, n=K + 1, L=0) for j in range(nd)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(K + 1, 15) for t in trajs])
    R = np.zeros((nd, K + 1, N_RAYS), dtype=np.float32)
    for j in range(nd):
        segs = liw.laser.room_segments(5000 + j)
        for k in range(K + 1):
            R[j, k] = liw.laser.cast_scan(segs, _T(truth[j, k, 0:3], truth[j, k, 3:6]) @ Til, n_rays=N_RAYS, seed=100 * j + k)[0]
    iv = {key: np.stack([np.asarray(t[key]).reshape(K, -1) for t in trajs]) for key in liw.fleet.INTERVAL_KEYS}
    return dict(truth=truth, ranges=R, times=np.stack([t["times"] for t in trajs]), iv=iv)


def track_run(liw, torch, prm, lp, tp, B, K, sc, reps, host_frames):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_glue_reference as ref
    nd = sc["truth"].shape[0]
    rob = np.arange(B) % nd
    robd = torch.from_numpy(rob).cuda()
    dims = dict(B=B, slots=1, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)
    Rd, Td = torch.from_numpy(sc["ranges"]).cuda(), torch.from_numpy(sc["times"]).cuda()
    ivd = {k: torch.from_numpy(v).cuda() for k, v in sc["iv"].items()}
    frames = [(Rd[:, k][robd].contiguous(), Td[:, k][robd].contiguous(), {kk: v[:, k - 1][robd].contiguous() for kk, v in ivd.items()}) for k in range(1, K + 1)]
    r0, t0, x0 = Rd[:, 0][robd].contiguous(), Td[:, 0][robd].contiguous(), sc["truth"][rob, 0]

    def begin(tr):
        tr.fe.reset()
        tr.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
        pts, _, n = tr.fe.ranges_to_points(r0, t0)
        tr.fe.spawn(0, pts, n)
        tr.fe.add_scan(0, x0[:, 0:6])
        tr.start(x0)

    def run(tr, nf):
        begin(tr)
        torch.cuda.synchronize()
        ts, dec = [], []
        for r, st, iv in frames[:nf]:
            t_a = time.perf_counter()
            o = tr.step(r, st, iv)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t_a) * 1e3)
            dec.append((np.asarray(o["key"].cpu() if torch.is_tensor(o["key"]) else o["key"]).copy(),
                        np.asarray(o["skip"].cpu() if torch.is_tensor(o["skip"]) else o["skip"]).copy(), int(o["Ltot"])))
        return ts, dec

    out = dict(K=K, distinct=nd)
    ft = liw.FleetTracker(prm, lp, tp, dims)
    run(ft, K)   # warm-up
    meds, dec_d = [], None
    for _ in range(reps):
        ts, dec_d = run(ft, K)
        meds.append(float(np.median(ts)))
    out["frame_ms"], out["frame_min_ms"], out["frame_max_ms"] = float(np.median(meds)), float(min(meds)), float(max(meds))
    out["robot_frames_per_s"] = B / (out["frame_ms"] * 1e-3)
    out["key_frames"], out["skipped"], out["Ltot_last"] = int(sum(d[0].sum() for d in dec_d)), int(sum(d[1].sum() for d in dec_d)), dec_d[-1][2]
    # the two glue kernels alone, on the state the last run left
    r, st, iv = frames[-1]
    x = ft.x.clone()
    sp = []
    out["track_begin_ms"] = timed(torch, lambda: ft.fe.track_begin(ft.tp, ft.track, x, iv["imu_X"], iv["imu_Dt"], iv["wheel_T"], st, out=ft._tb), reps, sp)
    out["track_begin_min_ms"], out["track_begin_max_ms"] = sp
    eo = dict(key=torch.zeros_like(ft.key), pose=torch.zeros_like(ft.pose))
    out["track_end_ms"] = timed(torch, lambda: ft.fe.track_end(ft.tp, ft.track, 0, x, ft._m["count"], out=eo), reps, sp)
    out["track_end_min_ms"], out["track_end_max_ms"] = sp
    ft.close()
    del ft
    torch.cuda.empty_cache()
    if host_frames > 0:
        ht = ref.HostGlueTracker(liw, prm, lp, tp, dims)
        ts, dec_h = run(ht, min(host_frames, K))
        out["host_glue"] = dict(frames=len(ts), frame_ms=float(np.median(ts)), frame_min_ms=float(min(ts)), frame_max_ms=float(max(ts)),
                                decisions_agree=bool(all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
                                                         for a, b in zip(dec_d, dec_h))))
        out["host_glue_over_device"] = out["host_glue"]["frame_ms"] / out["frame_ms"]
        ht.fe.close()
        ht.bs.close()
        del ht
        torch.cuda.empty_cache()
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def cold_run(liw, torch, prm, lp, tp, ip, B, K, sc, reps, host_frames):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fleet_init_reference as ref
    N = int(ip["slide_window_size"])
    Tc = N + 3                                   # the last robot (three frames late) tracks after this many frames
    nd = sc["truth"].shape[0]
    assert sc["truth"].shape[1] - 1 >= Tc + K
    robd = torch.from_numpy(np.arange(B) % nd).cuda()
    lag = torch.arange(B, device="cuda") % 4
    dims = dict(B=B, slots=N + 1, max_points=N_RAYS, max_lines=256, max_cell_entries=8192)
    Rd, Td = torch.from_numpy(sc["ranges"]).cuda(), torch.from_numpy(sc["times"]).cuda()
    ivd = {k: torch.from_numpy(v).cuda() for k, v in sc["iv"].items()}
    eye = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device="cuda")

    def frame(t, rest=None):
        """the inputs of frame t: robot b is at trajectory frame t - lag[b]; before its first frame, and where rest[b], it stands still"""
        kf = (t - lag).clamp(0, Tc + K)
        if rest is not None:
            kf = torch.where(rest, torch.zeros_like(kf), kf)
        mv, kc = kf >= 1, kf.clamp(min=1)
        iv = {}
        for k, v in ivd.items():
            a = v[robd, kc - 1]
            iv[k] = (torch.where(mv[:, None], a, eye[None, :]) if k == "wheel_T" else a).contiguous()
        return Rd[robd, kc].contiguous(), Td[robd, kc].contiguous(), iv

    def clock(tr, args):
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        o = tr.step(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t_a) * 1e3, o

    stat = lambda v: dict(ms=round(float(np.median(v)), 4), min_ms=round(float(min(v)), 4), max_ms=round(float(max(v)), 4))
    out = dict(N=N, K=K, distinct=nd)
    ft = liw.FleetTrajectory(prm, lp, tp, ip, dims)
    ft.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    cold_frames = [frame(t) for t in range(1, Tc + 1)]
    runs, inits = [], []
    for rep in range(reps + 1):                  # the first run is the warm-up: it also makes the INIT solvers
        ft.reset()
        ts, inits = [], []
        for t, args in enumerate(cold_frames, 1):
            ms, o = clock(ft, args)
            ts.append(ms)
            if bool(o["ready"].any()):
                inits.append(dict(frame=t, bucket=ft.last_init[0], R=ft.last_init[1], blocks=ft.last_init[2], committed=int(o["init_ok"].sum())))
        if rep:
            runs.append(ts)
    per = np.median(np.array(runs), axis=0)
    for d in inits:
        d["frame_ms"] = round(float(per[d["frame"] - 1]), 4)
    out["cold"] = dict(frames=Tc, frame_ms=[round(float(v), 4) for v in per], inits=inits, tracking_after=int((ft.status() == 1).sum()),
                       first_scan_to_tracking=stat([sum(r) for r in runs]))
    # ---- every robot tracks: the same frames through FleetTrajectory.step and FleetTracker.step, from the same state
    state = [ft.fe.store, ft.init, ft.track, ft.x, ft.match_pose, ft.has_match, ft.acc, ft.n_acc, ft.key, ft.pose, ft.flags] + [ft.bs.t[k] for k in liw.fleet.PRIOR_KEYS]
    snap = [t.clone() for t in state]
    track_frames = [frame(t) for t in range(Tc + 1, Tc + K + 1)]

    def restore():
        for t, s_ in zip(state, snap):
            t.copy_(s_)

    def frames_ms(tr, frames, prepare):
        meds = []
        for rep in range(reps + 1):
            prepare()
            ts = [clock(tr, args)[0] for args in frames]
            if rep:
                meds.append(float(np.median(ts)))
        return meds

    all_t = dict(trajectory=stat(frames_ms(ft, track_frames, restore)))
    tk = liw.FleetTracker(prm, lp, tp, dims)
    tk.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
    pairs = [(tk.fe.store, 0), (tk.track, 2), (tk.x, 3), (tk.match_pose, 4), (tk.has_match, 5), (tk.acc, 6), (tk.n_acc, 7), (tk.key, 8), (tk.pose, 9), (tk.flags, 10)]
    pairs += [(tk.bs.t[k], 11 + i) for i, k in enumerate(liw.fleet.PRIOR_KEYS)]

    def restore_tk():
        for t, i in pairs:
            t.copy_(snap[i])

    all_t["tracker"] = stat(frames_ms(tk, track_frames, restore_tk))
    all_t["trajectory_over_tracker"] = round(all_t["trajectory"]["ms"] / all_t["tracker"]["ms"], 4)
    out["all_tracking"] = all_t
    tk.close()
    del tk
    torch.cuda.empty_cache()
    # ---- a quarter of the fleet INITIALIZING and at rest
    quarter = (torch.arange(B, device="cuda") % 4) == 1
    qm = quarter.to(torch.uint8)
    mixed_frames = [frame(t, rest=quarter) for t in range(Tc + 1, Tc + K + 1)]
    its = []

    def to_mixed():
        restore()
        ft.fe.reset(mask=qm)
        ft.fe.init_reset(ft.tp, ft.init, mask=qm)

    out["mixed"] = dict(initializing=int(quarter.sum()), **stat(frames_ms(ft, mixed_frames, to_mixed)))
    to_mixed()
    qh = quarter.cpu().numpy()
    for args in mixed_frames:
        ft.step(*args)
        it = np.array([s_["iterations"] for s_ in ft.bs.summaries()])
        its.append(dict(tracking_max=int(it[~qh].max()), tracking_mean=round(float(it[~qh].mean()), 3), other_max=int(it[qh].max()),
                        other_mean=round(float(it[qh].mean()), 3)))
    out["mixed"]["iterations"] = its
    out["mixed"]["over_all_tracking"] = round(out["mixed"]["ms"] / all_t["trajectory"]["ms"], 4)
    ft.close()
    del ft, snap, state
    torch.cuda.empty_cache()
    if host_frames:
        host_frames = Tc if host_frames < 0 else min(host_frames, Tc)
        ht = ref.HostGlueTrajectory(liw, prm, lp, tp, ip, dims)
        ht.fe.set_geometry(N_RAYS, ANG_MIN, ANG_INC, T_INC)
        ts = [clock(ht, args)[0] for args in cold_frames[:host_frames]]
        dev_ms = float(sum(per[:len(ts)]))
        out["host_glue"] = dict(frames=len(ts), label="Python loop over the robots, one run", frame_ms=[round(float(v), 4) for v in ts],
                                total_ms=round(float(sum(ts)), 4), device_total_ms=round(dev_ms, 4), tracking_after=int((ht.status == 1).sum()))
        out["host_glue_over_device"] = round(float(sum(ts)) / dev_ms, 2)
        ht.close()
        del ht
        torch.cuda.empty_cache()
    return out


def host_run(liw, lp, sc, n=256):
    ra, rb, pa, pb = sc
    nd = ra.shape[0]
    t = dict(ranges_to_points=0.0, spawn=0.0, match_with_ref=0.0, add_scan=0.0)
    for i in range(n):
        j = i % nd
        m = liw.laser.LaserManager(lp)
        pts, _ = liw.laser.laser_to_points(ra[j], ANG_MIN, ANG_INC, T_INC, 0.0)
        m.add_scan(liw.laser.Scan.spawn(lp, pts), pa[j, :3], pa[j, 3:])
        t0 = time.perf_counter()
        pts, _ = liw.laser.laser_to_points(rb[j], ANG_MIN, ANG_INC, T_INC, 0.0)
        t1 = time.perf_counter()
        s = liw.laser.Scan.spawn(lp, pts)
        t2 = time.perf_counter()
        m.match_with_ref(s, pb[j, :3], pb[j, 3:])
        t3 = time.perf_counter()
        m.add_scan(s, pb[j, :3], pb[j, 3:])
        t4 = time.perf_counter()
        for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[k] += v
    out = {k + "_us": round(v / n * 1e6, 2) for k, v in t.items()}
    out["frame_us"] = round(sum(t.values()) / n * 1e6, 2)
    out["robots"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="4096,49152")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--init", type=int, default=0, help="frames per INIT window (0: no initialisation leg)")
    ap.add_argument("--init-B", default="4096")
    ap.add_argument("--track", type=int, default=0, help="frames of the fleet tracking leg (0: none)")
    ap.add_argument("--track-B", default="4096,49152")
    ap.add_argument("--track-distinct", type=int, default=16)
    ap.add_argument("--track-host-frames", type=int, default=2, help="frames of the host-glue baseline (0: none)")
    ap.add_argument("--cold-start", type=int, default=0, help="frames per INIT window of the cold-start leg (0: none)")
    ap.add_argument("--cold-B", default="4096,49152")
    ap.add_argument("--cold-frames", type=int, default=4, help="tracking frames timed after the cold start")
    ap.add_argument("--cold-host-frames", type=int, default=-1, help="frames of the host-glue baseline (-1: the whole cold start, 0: none)")
    a = ap.parse_args()
    import torch
    liw = importlib.import_module("2dliw-slam_amd")
    lp = liw.laser.office_laser_params()
    res = dict(tool="bench_laser_batch", n_rays=N_RAYS, distinct=a.distinct, device=torch.cuda.get_device_name(0), batch={})
    Bs = [int(x) for x in a.B.split(",") if x]
    if Bs:
        sc = scenes(liw, lp, a.distinct)
        for B in Bs:
            res["batch"][str(B)] = device_run(liw, torch, lp, B, sc, a.reps)
        res["host_per_scan"] = host_run(liw, lp, sc)
    if a.init:
        assert a.init >= 2, "--init N: at least two frames"
        res["init"] = {str(B): init_run(liw, torch, lp, B, a.init, a.distinct, a.reps) for B in [int(x) for x in a.init_B.split(",") if x]}
    if a.track:
        synth = importlib.import_module("2dliw-slam_amd.synth")
        prm = synth.office_params()
        lpt = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)   # the reference sub-map exists at every frame
        tp = liw.laser_batch.office_track_params(prm)
        tsc = track_scenes(liw, synth, prm, lpt, a.track_distinct, a.track)
        res["track"] = {str(B): track_run(liw, torch, prm, lpt, tp, B, a.track, tsc, a.reps, a.track_host_frames)
                        for B in [int(x) for x in a.track_B.split(",") if x]}
    if a.cold_start:
        synth = importlib.import_module("2dliw-slam_amd.synth")
        prm = synth.office_params()
        lpt = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
        tp = liw.laser_batch.office_track_params(prm)
        ip = dict(slide_window_size=a.cold_start, p_motion_threshold=0.1, q_motion_threshold=0.1)
        csc = track_scenes(liw, synth, prm, lpt, a.track_distinct, a.cold_start + 3 + a.cold_frames)
        res["cold_start"] = {}
        for B in [int(x) for x in a.cold_B.split(",") if x]:   # the host-glue baseline at the first B only: a Python loop over the robots
            res["cold_start"][str(B)] = cold_run(liw, torch, prm, lpt, tp, ip, B, a.cold_frames, csc, a.reps, a.cold_host_frames if not res["cold_start"] else 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
