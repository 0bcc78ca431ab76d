"""The eight key-frame sequences of the fleet loop detector's tests (tests/test_gpu_loop_batch.py), one per robot, built from the
scene helpers of tests/test_gpu_loop.py, and their host restatement: loop_reference.Detector with every gate quantity recorded, so
that "the fleet decides what the single detector decides" is a statement about decisions that are not within round-off of a
threshold.  Poses go through (p, rotation vector), as the fleet takes them: T -> liw_lie_log_SE3 -> liw_lie_make_tf."""
import ctypes as C
import functools
import importlib

import numpy as np

import loop_reference as ref
import second_config as sc
import test_gpu_loop as tgl

FRAMES = 40            # fleet frames; robot r gets its 30 key frames in frames OFFSET[r] .. OFFSET[r] + 29
KEYFRAMES = 30
# (submap_count, seed, landmark kwargs, sequence kwargs, first frame)
ROBOTS = [
    (3, 5, {}, dict(drift=(0.2, -0.1, 0.05)), 0),                                               # two passing candidates: the earlier wins
    (3, 7, {}, dict(revisit=False), 3),                                                         # no revisit
    (3, 44, dict(extent=14.0, spacing=0.6, jitter=0.18), dict(drift=(0.2, -0.1, 0.05), r=5.0), 7),   # sub-maps of 215 ... 446 points
    (3, 10, {}, dict(drift=(0.1, 0.1, 0.02)), 10),
    (1, 6, {}, dict(spin0=0.8), 0),                                                             # candidate 0 rejected by the tf gate
    (1, 8, {}, dict(drift=(-0.15, 0.1, -0.04)), 5),
    (1, 21, {}, dict(drift=(0.05, 0.05, -0.02)), 2),
    (1, 22, {}, dict(revisit=False), 9),
]
# the sequences at the second sets (second_config.LOOP_SETS "fine" and "coarse", detectors created from skewed_params): robot 2 comes
# back 0.9 m beside its first leg, so origin distances lie between max_tf_p and max_dis on candidates that give edges; robots 3 and
# 6 drift by half a metre, so |dp| of the tf gate lies between max_tf_q and max_tf_p on accepted edges
ROBOTS_SECOND = [
    (3, 5, {}, dict(drift=(0.2, -0.1, 0.05)), 0),
    (3, 7, {}, dict(revisit=False), 3),
    (3, 10, {}, dict(drift=(0.2, 0.0, 0.02), offset=(0.9, -0.03, 0.03)), 7),
    (3, 11, {}, dict(drift=(0.45, -0.2, 0.05)), 10),
    (1, 6, {}, dict(spin0=0.8), 0),
    (1, 8, {}, dict(drift=(-0.15, 0.1, -0.04)), 5),
    (1, 21, {}, dict(drift=(0.45, -0.2, 0.05)), 2),
    (1, 22, {}, dict(revisit=False), 9),
]
SETS = {3: [0, 1, 2, 3], 1: [4, 5, 6, 7]}     # robots by parameter set (submap_count): one fleet detector per set
MAX_POINTS = {3: 512, 1: 128}
REL = 1e-6


def _lie():
    L = importlib.import_module("2dliw-slam_amd").lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def pose_of(T):
        T12 = np.ascontiguousarray(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]))
        p, q = np.zeros(3), np.zeros(3)
        L.liw_lie_log_SE3(pd(T12), pd(p), pd(q))
        return np.concatenate([p, q])

    def make_tf(pose):
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        p, q, T12 = pose[:3].copy(), pose[3:].copy(), np.zeros(12)
        L.liw_lie_make_tf(pd(p), pd(q), pd(T12))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = T12[:9].reshape(3, 3), T12[9:]
        return M
    return pose_of, make_tf


def make_tf(pose):
    return _lie()[1](pose)


def robots(cfg="office"):
    return ROBOTS if cfg == "office" else ROBOTS_SECOND


def params(submap_count, cfg="office", **kw):
    return tgl._set_params(cfg, submap_count=submap_count, **kw)


def prm(cfg="office"):
    """the parameters the detectors of a set are created from"""
    return tgl._set_prm(importlib.import_module("2dliw-slam_amd.synth"), cfg)


def T_imu_to_wheel(cfg="office"):
    """the extrinsic as the detectors load it (liw_get_extrinsics of a ctx made from the set's parameters)"""
    liw = importlib.import_module("2dliw-slam_amd")
    L = liw.lib()
    ps = liw.params_struct(prm(cfg))
    ctx = C.c_void_p(L.liw_create(C.byref(ps)))
    M = np.zeros(16)
    L.liw_get_extrinsics(ctx, M.ctypes.data_as(C.POINTER(C.c_double)), None)
    L.liw_destroy(ctx)
    return M.reshape(4, 4)


@functools.lru_cache(maxsize=None)
def sequences(cfg="office"):
    """per robot: list of KEYFRAMES (pose6, T = make_tf(pose6), corners [n][3])"""
    pose_of, mk = _lie()
    Tiw = T_imu_to_wheel(cfg)
    out = []
    for S, seed, lkw, skw, _ in robots(cfg):
        rng = np.random.default_rng(seed)
        skw = dict(skw)
        if "drift" in skw:
            skw["drift"] = tgl._pose(*skw["drift"])
        frames, _ = tgl._loop_sequence(rng, tgl._landmarks(rng, **lkw), Tiw, **skw)
        seq = []
        for T, Cn, laser in frames:
            assert laser
            pose = pose_of(T)
            seq.append((pose, mk(pose), np.ascontiguousarray(Cn, dtype=np.float64).reshape(-1, 3)))
        out.append(seq)
    return out


class GateRecorder(ref.Detector):
    """loop_reference.Detector that records (kind, value, threshold) of every gate it evaluates"""

    def __init__(self, p, max_points, T_iw):
        super().__init__(p, max_points, T_iw)
        self.gates = []

    def try_candidate(self, q, i):
        p, F = self.p, self.features
        f1, f2 = F[q], F[i]
        if f1 is not None and f2 is not None and f1.valid and f2.valid:
            rel = ref.iso_inv(f1.origin) @ f2.origin
            self.gates.append(("dis", float(np.linalg.norm(rel[:3, 3])), p["max_dis"]))
        m = ref.match_map(f1, f2, q, i, p, self.margins)
        if m["gate"] in (0, 4):
            self.gates.append(("size", m["size"], p["min_match_threshold"]))
        if m["gate"] != 0:
            return None
        A1, A2 = ref.iso_inv(self.tfs[q] @ self.T_iw), ref.iso_inv(self.tfs[i] @ self.T_iw)
        P1 = np.array([A1[:3, :3] @ F[q].points[k] + A1[:3, 3] for k in m["p1"]])
        P2 = np.array([A2[:3, :3] @ F[i].points[k] + A2[:3, 3] for k in m["p2"]])
        P1[:, 2] = 0
        P2[:, 2] = 0
        w = ref.icp_closed_form(P1, P2)
        it12 = self.T_iw @ w @ ref.iso_inv(self.T_iw)
        err = ref.iso_inv(it12) @ (ref.iso_inv(self.tfs[q]) @ self.tfs[i])
        dp, dq = float(np.linalg.norm(err[:3, 3])), float(np.linalg.norm(ref.log_so3(err[:3, :3])))
        self.gates.append(("tf_p", dp, p["max_tf_p"]))
        self.gates.append(("tf_q", dq, p["max_tf_q"]))
        if dp > p["max_tf_p"] or dq > p["max_tf_q"]:
            return None
        return dict(index1=q, index2=i, size=m["size"], tf12=it12)


@functools.lru_cache(maxsize=None)
def restatement(cfg="office", T_iw=None):
    """per robot: dict(edges [KEYFRAMES] (None or the edge after key frame k), gates, n_points, later_passes, per_candidate: the gate
    values grouped by evaluated candidate).  T_iw (a tuple of 16) replaces the extrinsic of the restatement alone: the CPU guards
    show with it that a wrong T_imu_to_wheel in the tf gate's conjugation moves the edges."""
    Tiw = T_imu_to_wheel(cfg) if T_iw is None else np.array(T_iw).reshape(4, 4)
    out = []
    for r, (S, *_rest) in enumerate(robots(cfg)):
        rd = GateRecorder(params(S, cfg), MAX_POINTS[S], Tiw)
        edges = []
        for pose, T, Cn in sequences(cfg)[r]:
            rd.add_keyframe(T, Cn, True)
            edges.append(rd.detect())
        later = False
        if r == 0:   # a later candidate passes every gate too, so the ascending walk is what picked the earlier one
            e, n0 = edges[-1], len(rd.gates)
            s = S // 3 + 1
            later = any(rd.try_candidate(e["index1"], c) is not None for c in range(e["index2"] + s, e["index1"] - rd.p["min_interval"], s))
            del rd.gates[n0:]
        out.append(dict(edges=edges, gates=list(rd.gates), n_points=[len(f.points) for f in rd.features], later_passes=later,
                        per_candidate=per_candidate(rd.gates), min_margin=min(rd.margins) if rd.margins else np.inf))
    return out


def per_candidate(gates):
    """the recorded gates grouped by evaluated candidate: every candidate starts with its "dis" record -> list of dicts kind -> value"""
    out = []
    for k, v, _ in gates:
        if k == "dis" or not out:
            out.append({})
        out[-1][k] = v
    return out


def near_threshold(gates, rel=REL):
    """the recorded gate quantities within `rel` (relative) of their threshold; sizes are integers and compare exactly"""
    return [(k, v, t) for k, v, t in gates if k != "size" and abs(v - t) <= rel * abs(t)]
