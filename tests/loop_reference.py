"""Literal serial restatement of the reference's laser loop detection (src/trajectory/keyframe_manager.cpp: the sub-map
feature :898-1032, match_des :1034-1123, match_map :1125-1184, laser_loop_detect :642-712) in plain Python / numpy, with the
deliberate substitutes of include/liw_loop.h: splitmix64 row draws instead of rand(), no shuffle, the first bin of the tie
list, descriptors sorted by (dij, j), and the closed-form planar ICP.  A numpy Levenberg-Marquardt over point_factor
(src/factor/point_factor.h:17-35) is here only to check that closed form.  Every angle-bin decision records its distance to the
nearest bin boundary (`margins`), so that a comparison with the device (whose acos may differ by an ulp) is a real statement."""
import math

import numpy as np

M64 = 0xFFFFFFFFFFFFFFFF
DRAWS = 5
QUICK_COUNTS = set()   # every quick-filter popcount match_des has seen (tests check that the edge cases occur)


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_row(seed, q, c, d, n1):
    return splitmix64((seed ^ (q << 40) ^ (c << 8) ^ d) & M64) % n1


def sizes(p):
    n_angle = int(math.pi * 2 / p["a_res"] + 2)
    W = int((100.0 / p["d_res"] + 1) / 64 + 1)
    return W, n_angle


def dedup(corner_lists, d_res):
    """laser_map_feature constructor :955-980: corner lists newest key frame first"""
    pts = []
    for cs in corner_lists:
        for c in cs:
            c = [float(c[0]), float(c[1]), float(c[2])]
            dup = False
            for k in range(len(pts)):
                dx, dy = c[0] - pts[k][0], c[1] - pts[k][1]
                nrm = math.sqrt(dx * dx + dy * dy)
                if nrm < d_res / 2:
                    pts[k] = [(pts[k][e] * 3 + c[e]) / 4 for e in range(3)]
                if nrm < d_res * 5:
                    dup = True
                    break
            if not dup:
                pts.append(c)
    return pts


def describe(pts, d_res, W):
    """-> rows: per point i dict(i, dij, j, aij (lists in (dij, j) order), quick (W python ints))"""
    rows = []
    n = len(pts)
    for i in range(n):
        ent = []
        for j in range(n):
            if j == i:
                continue
            vx, vy = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
            nrm = math.sqrt(vx * vx + vy * vy)
            a = math.acos(vx / nrm) if vy > 0 else math.pi * 2 - math.acos(vx / nrm)
            ent.append((int(nrm / d_res + 0.5), j, a))
        ent.sort(key=lambda e: (e[0], e[1]))
        quick = [0] * W
        for e in ent:
            if e[0] // 64 < W:
                quick[e[0] // 64] |= 1 << (e[0] % 64)
        rows.append(dict(i=i, dij=[e[0] for e in ent], j=[e[1] for e in ent], aij=[e[2] for e in ent], quick=quick))
    return rows


def _bin(a1, a2, a_res, orign, margins):
    d0 = a1 - a2
    d = d0
    if d >= math.pi:
        d -= math.pi * 2
    elif d < -math.pi:
        d += math.pi * 2
    q = d / a_res
    if margins is not None:   # int() truncates toward zero: the boundaries are the non-zero integers, and the wrap at +-pi
        aq = abs(q)
        margins.append((1.0 - aq if aq < 1.0 else min(aq - math.floor(aq), math.ceil(aq) - aq)) * a_res)
        margins.append(min(abs(d0 - math.pi), abs(d0 + math.pi)))
    return int(q) + orign


def match_des(d1, d2, p, margins=None):
    """the serial walk of :1034-1123 -> None (quick filter) or dict(size, bin, p1, p2) or the reference's match_all[maxIndex]"""
    total = sum(bin(a & b).count("1") for a, b in zip(d1["quick"], d2["quick"]))
    QUICK_COUNTS.add(total)
    if total < p["min_match_threshold"]:
        return None
    M, N = len(d1["dij"]), len(d2["dij"])
    n_angle = int(math.pi * 2 / p["a_res"] + 2)
    orign = n_angle // 2
    match_all = [None] * (n_angle + 1)
    m = n = 0
    max_size, max_index = 0, 0
    ties = []
    while m < M and n < N:
        if d1["dij"][m] == d2["dij"][n]:
            tn = 0
            while n + tn < N and d1["dij"][m] == d2["dij"][n + tn]:
                b = _bin(d1["aij"][m], d2["aij"][n + tn], p["a_res"], orign, margins)
                if match_all[b] is None:
                    match_all[b] = dict(bin=b, p1=[d1["i"]], p2=[d2["i"]])
                has_use = d1["j"][m] in match_all[b]["p1"]
                if not has_use:
                    match_all[b]["p1"].append(d1["j"][m])
                    match_all[b]["p2"].append(d2["j"][n + tn])
                    sz = len(match_all[b]["p1"])
                    if sz > max_size:
                        max_size, max_index, ties = sz, b, [b]
                    elif sz == max_size:
                        ties.append(b)
                tn += 1
            m += 1
        elif d1["dij"][m] > d2["dij"][n]:
            n += 1
        else:
            m += 1
    r = match_all[max_index] if not ties else match_all[ties[0]]
    if r is None:
        return None
    return dict(size=len(r["p1"]), bin=r["bin"], p1=list(r["p1"]), p2=list(r["p2"]))


class Feature:
    def __init__(self, pts, origin, p, max_points):
        self.points = pts
        self.origin = origin
        self.valid = len(pts) <= max_points
        W, _ = sizes(p)
        self.rows = describe(pts, p["d_res"], W) if self.valid else None


def match_map(f1, f2, q, c, p, margins=None):
    """:1125-1184 with the splitmix64 draws -> dict(gate, size, draw, row, query_row, bin, p1, p2)"""
    out = dict(gate=0, size=0, draw=-1, row=-1, query_row=-1, bin=-1, p1=[], p2=[])
    if f1 is None or f2 is None or not f1.valid or not f2.valid:
        out["gate"] = 1
        return out
    n1, n2, thr = len(f1.points), len(f2.points), p["min_match_threshold"]
    if n1 < thr or n2 < thr or n1 == 0 or n2 == 0:
        out["gate"] = 2
        return out
    rel = iso_inv(f1.origin) @ f2.origin
    if np.linalg.norm(rel[:3, 3]) > p["max_dis"]:
        out["gate"] = 3
        return out
    best = None
    has = [0] * n1
    for d in range(DRAWS):
        ri = draw_row(int(p.get("seed", 0)), q, c, d, n1)
        if has[ri]:
            continue
        has[ri] = 1
        for i in range(n2):
            t = match_des(f1.rows[ri], f2.rows[i], p, margins)
            if t is not None and t["size"] > out["size"]:
                out.update(size=t["size"], draw=d, row=i, query_row=ri, bin=t["bin"])
                best = t
    if out["size"] > thr:
        out["p1"], out["p2"] = best["p1"], best["p2"]
    else:
        out["gate"] = 4
    return out


def iso_inv(T):
    """Eigen's Isometry3d::inverse(): R^T, -R^T t (the extrinsics need not be exactly orthonormal)"""
    R = T[:3, :3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -(R.T @ T[:3, 3])
    return out


def icp_closed_form(P1, P2):
    """planar Procrustes: T (4x4) with P1 ~ T P2"""
    P1, P2 = np.asarray(P1, dtype=np.float64), np.asarray(P2, dtype=np.float64)
    c1, c2 = P1[:, :2].mean(axis=0), P2[:, :2].mean(axis=0)
    a, b = P1[:, :2] - c1, P2[:, :2] - c2
    yaw = math.atan2(float(np.sum(b[:, 0] * a[:, 1] - b[:, 1] * a[:, 0])), float(np.sum(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1])))
    c, s = math.cos(yaw), math.sin(yaw)
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:2, 3] = c1 - T[:2, :2] @ c2
    return T


def _exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def log_so3(R):
    c = max(-1.0, min(1.0, (np.trace(R) - 1) / 2))
    th = math.acos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v / 2 if th < 1e-12 else th / (2 * math.sin(th)) * v


def icp_lm(P1, P2, iters=100):
    """Levenberg-Marquardt over point_factor (residual 100 (p1 - T p2), all three components) from identity, 6 dof."""
    P1, P2 = np.asarray(P1, dtype=np.float64), np.asarray(P2, dtype=np.float64)
    R, t, lam = np.eye(3), np.zeros(3), 1e-4

    def cost(R, t):
        r = 100 * (P1 - (P2 @ R.T + t))
        return float(np.sum(r * r)), r
    c0, r = cost(R, t)
    for _ in range(iters):
        RP = P2 @ R.T
        J = np.zeros((3 * len(P1), 6))
        for k in range(len(P1)):
            v = RP[k]
            J[3 * k:3 * k + 3, :3] = -100 * np.eye(3)
            J[3 * k:3 * k + 3, 3:] = 100 * np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        H, g = J.T @ J, J.T @ r.reshape(-1)
        step = np.linalg.solve(H + lam * np.diag(np.diag(H) + 1e-12), -g)
        Rn, tn = _exp_so3(step[3:]) @ R, step[:3] + t
        cn, rn = cost(Rn, tn)
        if cn <= c0:
            R, t, c0, r, lam = Rn, tn, cn, rn, lam * 0.1
            if np.abs(step).max() < 1e-15:
                break
        else:
            lam *= 10
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


class Detector:
    """add_keyframe / detect of the C ABI, restated serially.  Poses are 4x4 world <- IMU; T_iw = T_imu_to_wheel (4x4)."""

    def __init__(self, p, max_points, T_iw):
        self.p, self.max_points, self.T_iw = dict(p), max_points, np.asarray(T_iw, dtype=np.float64)
        self.tfs, self.laser, self.corners, self.features = [], [], [], []
        self.margins = []

    def add_keyframe(self, T, corners, is_laser=True):
        self.tfs.append(np.asarray(T, dtype=np.float64))
        self.laser.append(bool(is_laser))
        self.corners.append([] if corners is None else [list(map(float, c)) for c in np.asarray(corners).reshape(-1, 3)])
        if not is_laser:
            self.features.append(None)
            return len(self.tfs) - 1
        lists, count, index, origin = [], 0, -1, np.eye(4)
        for i in range(len(self.tfs) - 1, -1, -1):
            if self.laser[i]:
                count += 1
                lists.append(self.corners[i])
                if count == self.p["submap_count"]:
                    break
                if index == -1:
                    index, origin = i, self.tfs[i]
        self.features.append(Feature(dedup(lists, self.p["d_res"]), origin, self.p, self.max_points))
        return len(self.tfs) - 1

    def try_candidate(self, q, i):
        """match_map of candidate i for query q, then the ICP and the tf gate -> the edge, or None"""
        p, F = self.p, self.features
        m = match_map(F[q], F[i], q, i, p, self.margins)
        if m["gate"] != 0:
            return None
        A1, A2 = iso_inv(self.tfs[q] @ self.T_iw), iso_inv(self.tfs[i] @ self.T_iw)
        P1 = np.array([A1[:3, :3] @ F[q].points[k] + A1[:3, 3] for k in m["p1"]])
        P2 = np.array([A2[:3, :3] @ F[i].points[k] + A2[:3, 3] for k in m["p2"]])
        P1[:, 2] = 0
        P2[:, 2] = 0
        w = icp_closed_form(P1, P2)
        it12 = self.T_iw @ w @ iso_inv(self.T_iw)
        err = iso_inv(it12) @ (iso_inv(self.tfs[q]) @ self.tfs[i])
        if np.linalg.norm(err[:3, 3]) > p["max_tf_p"] or np.linalg.norm(log_so3(err[:3, :3])) > p["max_tf_q"]:
            return None
        return dict(index1=q, index2=i, size=m["size"], tf12=it12)

    def detect(self):
        p, F = self.p, self.features
        K = len(F)
        if K < p["min_interval"] or F[-1] is None or not F[-1].valid:
            return None
        q, s = K - 1, p["submap_count"] // 3 + 1
        for i in range(0, K - p["min_interval"], s):
            if F[i] is None:
                continue
            e = self.try_candidate(q, i)
            if e is not None:
                return e
        return None
