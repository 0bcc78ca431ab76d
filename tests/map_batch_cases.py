"""Rooms, scans and fleet plumbing for the fleet map tests (tests/test_gpu_map_batch.py) and tools/bench_map_batch.py: small room
cases under SE(3) transforms, loading per-robot sub-map lists into a FleetMapper frame by frame, and the exact comparison of a
robot's grid and info with a reference render (tests/map_reference.py, imported as it is)."""
import ctypes as C
import importlib

import numpy as np

RES = 0.05


def _replay():
    return importlib.import_module("2dliw-slam_amd.replay")


def tf12(x, y, yaw, z=0.0, roll=0.0, pitch=0.0):
    """world <- laser as R (row-major 9) then t"""
    Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
    Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    return np.concatenate([(Rz @ Ry @ Rx).reshape(9), [x, y, z]])


def rooms(n=16):
    """n distinct rooms: replay_room and pillar_room, each with one more wall stub at a place of its own"""
    rp = _replay()
    out = []
    for i in range(n):
        segs = list(rp.pillar_room() if i % 2 else rp.replay_room())
        a = 2 * np.pi * i / n
        c = np.array([6.2 * np.cos(a), 5.0 + 6.2 * np.sin(a)])
        d = 0.6 * np.array([np.cos(a + 0.7 * i), np.sin(a + 0.7 * i)])
        segs.append((c - d, c + d))
        out.append(segs)
    return out


def scan(room, x, y, yaw, n_rays, rng, noise=0.004):
    """laser-frame points [m][3] of a scan cast from (x, y, yaw) in the world (misses dropped)"""
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = (x, y)
    rg, amin, inc = _replay().cast_scan_moving(room, lambda t: T, 0.0, n_rays, 2 * np.pi * 0.75, 0.0, noise, rng)
    a = float(amin) + float(inc) * np.arange(n_rays)
    ok = np.isfinite(rg) & (rg > 0.1)
    r = rg[ok].astype(np.float64)
    return np.stack([r * np.cos(a[ok]), r * np.sin(a[ok]), np.zeros(r.size)], axis=1)


def room_case(rng, K, n_rays, tilt=0.03, room=None):
    """K scans of the room from random poses on the circle, each with its world <- laser transform (small roll / pitch: dz != 0);
    n_rays may be a pair (lo, hi): every scan draws its own ray count"""
    room = _replay().replay_room() if room is None else room
    tfs, subs = [], []
    for _ in range(K):
        a = rng.uniform(-np.pi, np.pi)
        x, y, yaw = 5.0 * np.cos(a), 5.0 + 5.0 * np.sin(a), rng.uniform(-np.pi, np.pi)
        nr = int(rng.integers(n_rays[0], n_rays[1] + 1)) if isinstance(n_rays, tuple) else n_rays
        subs.append(scan(room, x, y, yaw, nr, rng))
        tfs.append(tf12(x, y, yaw, rng.uniform(-0.05, 0.05), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)))
    return np.array(tfs).reshape(K, 12), subs


def mapper(liw, synth, B, K, P, cells, steps, res=RES, guard=64, prm=None):
    return liw.FleetMapper(synth.office_params() if prm is None else prm, dict(resolution=res),
                           dict(B=B, max_submaps=K, max_points=P, max_cells=cells, max_steps=steps), guard=guard)


def frame(subs_of, f, stride):
    """frame f of the per-robot sub-map lists: key [B] uint8, points [B, stride, 3], n [B] int32"""
    B = len(subs_of)
    key, pts, n = np.zeros(B, np.uint8), np.zeros((B, stride, 3)), np.zeros(B, np.int32)
    for b, subs in enumerate(subs_of):
        if f < len(subs):
            s = np.asarray(subs[f], dtype=np.float64).reshape(-1, 3)
            key[b], n[b] = 1, len(s)
            pts[b, :len(s)] = s
    return key, pts, n


def load(fm, subs_of, stride=None):
    """push every robot's sub-maps, one per frame (robots with fewer sub-maps have their key clear in the later frames)"""
    stride = max([1] + [len(s) for subs in subs_of for s in subs]) if stride is None else stride
    for f in range(max([0] + [len(subs) for subs in subs_of])):
        fm.add_keyframes(*frame(subs_of, f, stride))


def pad_tfs(tfs_of, n, width=12):
    """per-robot [K_b, width] arrays -> [B, n, width] (zeros behind)"""
    out = np.zeros((len(tfs_of), n, width))
    for b, t in enumerate(tfs_of):
        t = np.asarray(t, dtype=np.float64).reshape(-1, width)
        out[b, :len(t)] = t
    return out


def assert_info(info, want):
    assert (info["width"], info["height"]) == (want["width"], want["height"])
    assert (info["origin_x"], info["origin_y"]) == (want["origin_x"], want["origin_y"])
    assert info["resolution"] == want["resolution"]
    assert (info["rays"], info["samples"]) == (want["rays"], want["samples"])
    assert {-1: info["unknown"], 0: info["free_cells"], 50: info["hit_once"], 100: info["hit_more"]} == want["counts"]


def assert_robot(fm, b, want, row=None):
    """robot b's held grid and info equal the reference render `want` exactly; row: its info row of the render, equal too"""
    info = fm.info_of(b)
    assert info.pop("status") == (1 if want["rays"] == 0 else 0)
    assert_info(info, want)
    if row is not None:
        assert row == info
    g = fm.grid(b)
    assert g.shape == want["grid"].shape
    assert int((g != want["grid"]).sum()) == 0


def regions(fm):
    """[B, robot_bytes] uint8 host copy of the robot regions"""
    fm._sync()
    return fm.robot_regions().cpu().numpy().copy()


def host_tf(liw, poses, Til12):
    """liw_lie_make_tf(p, q) * T_imu_to_laser for poses [n, 6] -> [n, 12]"""
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)
    out = np.zeros((len(poses), 12))
    Til12 = np.ascontiguousarray(Til12, dtype=np.float64)
    for k, ps in enumerate(poses):
        A = np.zeros(12)
        p, q = np.ascontiguousarray(ps[:3]), np.ascontiguousarray(ps[3:])
        L.liw_lie_make_tf(pd(p), pd(q), pd(A))
        L.liw_lie_mul(pd(A), pd(Til12), pd(out[k]))
    return out


def til12(liw, prm):
    """T_imu_to_laser as the library loads it (liw_lie_from_matrix16 with the parameters' normalize_extrinsics)"""
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    M = np.ascontiguousarray(np.asarray(prm["T_imu_to_laser"], dtype=np.float64).reshape(16))
    out = np.zeros(12)
    L.liw_lie_from_matrix16(pd(M), C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), pd(out))
    return out


def ulps(a, b):
    """largest |a - b| in units of the spacing at the larger magnitude, over all entries"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))
