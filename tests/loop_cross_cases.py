"""Cases of the cross-robot loop detection and group alignment (include/liw_loop_cross.h; tests/test_gpu_loop_cross.py runs them on
the device, tests/test_loop_cross_cases.py guards them on the host alone) and their host restatement, built on
tests/loop_reference.py: match_map with max_dis = inf, icp_closed_form, iso_inv, then the residual, the best-size choice and the
link rules.  The scenes come from the helpers of tests/test_gpu_loop.py.  Robots of one building see the same landmark set; each
robot has a world frame of its own, a known W_r (yaw, translation, a small tilt) applied to its poses and corners, so the truth
T_w1_w2 = W_a W_b^-1 is known.  Corner noise is uniform in +-1 mm per planar axis, so that a hard bound follows from it.

Fleets (max_points 64, max_kf_corners 32):
  "s3"    B = 8, submap_count 3 (candidate stride 2), K <= 14
  "s1"    B = 8, submap_count 1 (stride 1), K <= 14
  "long"  B = 2, submap_count 1: robot 0 has 70 key frames of about 10-point sub-maps, so robot 1 has more than 64 candidates
Robots of "s3" / "s1" (K0 = 11 / 12, S = submap_count):
  0  building 0, along x from (-2, 0); the anchor
  1  building 0, K0 + S key frames, ends on robot 0's path 1.5 m before its end: several passing candidates of different size
  2  building 0, K0 + S key frames, runs back along robot 0's path to (-1, 0.2): covers the newest key frames of robots 0 and 1
  3  building 0, stands still at (0.1, -0.2) and sees the same corners in every key frame, but in key frame 4 half of them are
     rotated about the robot by SPIN: equal candidates (a size tie, settled by index) and one accepted by size, rejected by rms
  4  building 1
  5  building 0, ends at robot 3's place
  6  no key frames
  7  building 0; its newest sub-map is invalid (s3: over max_points, s1: a key frame over max_kf_corners)
"""
import functools
import math

import numpy as np

import loop_batch_cases as lbc
import loop_reference as ref
import test_gpu_loop as tgl

MAX_POINTS, MAX_KF_CORNERS = 64, 32
NOISE = 1e-3            # uniform, per planar axis
SPIN = 0.012            # rad: moves a corner 2 m from the robot by 2.4 cm, inside the descriptor's bins often enough
MIN_MATCH = {"s3": 9, "s1": 9, "long": 5}
MAX_RMS = 0.006         # clean candidates have a residual of about 1 mm, the spun one about 1 cm
REL = lbc.REL
FLEETS = ("s3", "s1", "long")
SUBMAP = {"s3": 3, "s1": 1, "long": 1}
GROUP_OF = [0, 0, 0, 0, 1, 0, 0, -1]
T_ANCHOR4 = (1.5, -2.0, 0.4)     # the second anchor (robot 4, group 1) starts with a transform of its own (x, y, yaw)
SEED = {"s3": 0, "s1": 4, "long": 5}   # of the paths' jitter and the noise: the first seeds at which check() has nothing to report


def params(name):
    return tgl._params(submap_count=SUBMAP[name], min_interval=2)


def dims(name):
    return dict(B=2 if name == "long" else 8, max_keyframes=72 if name == "long" else 14, max_points=MAX_POINTS, max_kf_corners=MAX_KF_CORNERS)


def _world(r, seed):
    """W_r: yaw, translation, a tilt of up to 0.01 rad about x and y"""
    rng = np.random.default_rng(seed * 100 + r)
    yaw, tx, ty = rng.uniform(-math.pi, math.pi), rng.uniform(-4, 4), rng.uniform(-4, 4)
    ax, ay = rng.uniform(-0.01, 0.01, 2)
    W = np.eye(4)
    W[:3, :3] = ref._exp_so3(np.array([ax, ay, 0.0])) @ ref._exp_so3(np.array([0.0, 0.0, yaw]))
    W[:3, 3] = (tx, ty, rng.uniform(-0.2, 0.2))
    return W


STEP = {"s3": 0.3, "s1": 0.5}     # metres between key frames: at stride 1 a longer step, or neighbouring candidates tie in size


def _line(x0, y0, yaw, K, step=0.3, jit=None):
    if jit is not None:     # the whole path is shifted by up to 0.15 m and turned by up to 0.05 rad
        x0, y0, yaw = x0 + jit.uniform(-0.15, 0.15), y0 + jit.uniform(-0.15, 0.15), yaw + jit.uniform(-0.05, 0.05)
    return [tgl._pose(x0 + step * k * math.cos(yaw), y0 + step * k * math.sin(yaw), yaw + 0.02 * k) for k in range(K)]


@functools.lru_cache(maxsize=None)
def fleet(name):
    """-> dict(name, params, dims, W [B] 4x4, building [B], K [B], frames [B][K] of (pose6, T 4x4, corners [n][3]), T_iw)"""
    pose_of, mk = lbc._lie()
    Tiw = lbc.T_imu_to_wheel()
    S = SUBMAP[name]
    rng = np.random.default_rng({"s3": 31, "s1": 11, "long": 71}[name] + 1000 * SEED[name])
    jit = np.random.default_rng({"s3": 32, "s1": 12, "long": 72}[name] + 1000 * SEED[name])
    Ls = [tgl._landmarks(np.random.default_rng(900)), tgl._landmarks(np.random.default_rng(901))]
    B = dims(name)["B"]
    W = [_world(r, 7 if name != "long" else 8) for r in range(B)]
    bases, building, radius = [], [0] * B, [2.5] * B
    if name == "long":
        bases = [_line(-9.0, 1.0, 0.0, 70, step=0.25, jit=jit), _line(1.0, -2.0, math.pi / 2, 13, step=0.25, jit=jit)]
        radius = [1.8, 1.8]
    else:
        K0 = 11 if S == 3 else 12
        K1 = K0 + S
        st = STEP[name]
        end0 = -2.0 + st * (K0 - 1)        # robot 0 ends here; robot 1 ends 1.5 m before it, robot 2 starts 1.9 m behind it and ends at -1
        bases = [_line(-2.0, 0.0, 0.0, K0, step=st, jit=jit),
                 _line(end0 - 1.5, -st * (K1 - 1), math.pi / 2, K1, step=st, jit=jit),
                 _line(-1.0 + st * (K1 - 1), 0.2, math.pi, K1, step=st, jit=jit),
                 [tgl._pose(0.1, -0.2, 0.3)] * 9,
                 _line(-2.0, 0.5, 0.1, 10, step=st, jit=jit),
                 _line(0.1 - st * 7, -0.2, 0.0, 8, step=st),
                 [],
                 _line(-4.0, -4.0, 0.5, 3, step=5.5) if S == 3 else _line(-4.0, -4.0, 0.5, 5)]
        building[4] = 1
        radius[7] = 2.9 if S == 3 else 2.5    # s3: about 27 corners a key frame, 5.5 m apart: three of them pass 64 points
    frames = []
    for r in range(B):
        seq, still = [], None
        for k, Bk in enumerate(bases[r]):
            L = Ls[building[r]]
            C = tgl._seen(L, Bk, r=radius[r])
            C[:, :2] += rng.uniform(-NOISE, NOISE, (len(C), 2))
            if name != "long" and r == 3:
                if still is None:
                    still = C.copy()
                C = still.copy()
                if k == 4:          # half of the corners (every second one) rotated about the robot
                    Cs = C.copy()
                    c = Bk[:2, 3]
                    Cs[:, :2] = (C[:, :2] - c) @ tgl._rot(SPIN).T + c
                    C[1::2] = Cs[1::2]
            if name == "s1" and r == 7 and k == len(bases[r]) - 1:    # the newest key frame has more than max_kf_corners corners
                extra = np.stack([np.arange(20) * 0.7 + 30.0, np.full(20, 25.0), np.zeros(20)], axis=1)
                C = np.concatenate([C, extra])
                assert len(C) > MAX_KF_CORNERS
            else:
                assert len(C) <= MAX_KF_CORNERS, (name, r, k, len(C))
            Cw = C @ W[r][:3, :3].T + W[r][:3, 3]
            pose = pose_of(W[r] @ Bk @ ref.iso_inv(Tiw))
            seq.append((pose, mk(pose), np.ascontiguousarray(Cw)))
        frames.append(seq)
    return dict(name=name, params=params(name), dims=dims(name), W=W, building=building, K=[len(s) for s in frames], frames=frames, T_iw=Tiw,
                bases=bases)


def truth(name, a, b):
    F = fleet(name)
    return F["W"][a] @ ref.iso_inv(F["W"][b])


# ---------------------------------------------------------------------------------------------------------------- restatement
@functools.lru_cache(maxsize=None)
def features(name):
    """per robot a loop_reference.Detector fed its key frames; a sub-map that contains a key frame over max_kf_corners is invalid, as
    in the fleet's store (LIW_FLOOP_OVER_CORNERS)"""
    F = fleet(name)
    out = []
    for r in range(F["dims"]["B"]):
        rd = ref.Detector(F["params"], MAX_POINTS, F["T_iw"])
        over = []
        for k, (pose, T, C) in enumerate(F["frames"][r]):
            big = len(C) > MAX_KF_CORNERS
            over.append(big)
            rd.add_keyframe(T, np.zeros((0, 3)) if big else C, True)
            if any(over[max(0, k - SUBMAP[name] + 1):k + 1]):
                rd.features[k].valid = False
                rd.features[k].rows = None
        out.append(rd)
    return out


def _popcount_tasks(f1, f2, q, c, p):
    """(tasks, quick_pass) of a launched pair: a task per distinct drawn query row and candidate row"""
    n1, n2 = len(f1.points), len(f2.points)
    seen, tasks, quick = set(), 0, 0
    for d in range(ref.DRAWS):
        ri = ref.draw_row(int(p.get("seed", 0)), q, c, d, n1)
        if ri in seen:
            continue
        seen.add(ri)
        tasks += n2
        for i in range(n2):
            if sum(bin(x & y).count("1") for x, y in zip(f1.rows[ri]["quick"], f2.rows[i]["quick"])) >= p["min_match_threshold"]:
                quick += 1
    return tasks, quick


def candidate(name, a, b, i, min_match):
    """the walk over one candidate -> dict(gate: 1 null / 2 points / 0 launched, match (match_map's result), and for size >
    min_match: tf12 (it12 4x4), T (T_w1_w2 4x4), rms, P2w (the matched candidate points in b's world), spread, margins)"""
    F, D = fleet(name), features(name)
    p = dict(F["params"], max_dis=float("inf"))
    q = F["K"][a] - 1
    f1, f2 = D[a].features[q], D[b].features[i]
    margins = []
    m = ref.match_map(f1, f2, q, i, p, margins)
    out = dict(gate=m["gate"] if m["gate"] in (1, 2) else 0, match=m, margins=margins)
    if out["gate"]:
        return out
    out["tasks"], out["quick"] = _popcount_tasks(f1, f2, q, i, p)
    if m["size"] <= min_match:
        return out
    Tiw = F["T_iw"]
    tfa, tfb = D[a].tfs[q], D[b].tfs[i]
    A1, A2 = ref.iso_inv(tfa @ Tiw), ref.iso_inv(tfb @ Tiw)
    P2w = np.array([f2.points[k] for k in m["p2"]])
    P1 = np.array([A1[:3, :3] @ np.asarray(f1.points[k]) + A1[:3, 3] for k in m["p1"]])
    P2 = np.array([A2[:3, :3] @ np.asarray(f2.points[k]) + A2[:3, 3] for k in m["p2"]])
    P1[:, 2] = 0
    P2[:, 2] = 0
    w = ref.icp_closed_form(P1, P2)
    d = P1[:, :2] - (P2[:, :2] @ w[:2, :2].T + w[:2, 3])
    ss = 0.0
    for e in d:
        ss += e[0] * e[0] + e[1] * e[1]
    it12 = Tiw @ w @ ref.iso_inv(Tiw)
    c2 = P2[:, :2] - P2[:, :2].mean(axis=0)
    out.update(tf12=it12, T=(tfa @ it12) @ ref.iso_inv(tfb), rms=math.sqrt(ss / len(P1)), P2w=P2w,
               spread=math.sqrt(float(np.sum(c2 * c2)) / len(P2)))
    return out


def detect(name, key, partner, mask=None, min_match=None, max_rms=MAX_RMS):
    """liw_xloop_detect restated -> per robot None (masked out), dict(found=0) alone (key clear), or dict(found, edge, tf12, T, rms,
    stats, cands: {i: candidate(...)})"""
    F = fleet(name)
    B, s = F["dims"]["B"], SUBMAP[name] // 3 + 1
    mm = MIN_MATCH[name] if min_match is None else min_match
    D = features(name)
    out = []
    for a in range(B):
        if mask is not None and not mask[a]:
            out.append(None)
            continue
        if not key[a]:
            out.append(dict(found=0, key=0))
            continue
        b = int(partner[a])
        res = dict(found=0, key=1, edge=[-1, -1, -1, 0], stats=[0] * 6, cands={})
        out.append(res)
        Ka = F["K"][a]
        if not (0 <= b < B) or b == a or Ka == 0 or F["K"][b] == 0 or not D[a].features[Ka - 1].valid:
            continue
        st, best = res["stats"], None
        for i in range(0, F["K"][b], s):
            st[0] += 1
            c = candidate(name, a, b, i, mm)
            res["cands"][i] = c
            if c["gate"]:
                continue
            st[1] += 1
            st[2] += c["tasks"]
            st[3] += c["quick"]
            if c["match"]["size"] <= mm:
                continue
            st[4] += 1
            st[5] += 1
            if not (c["rms"] > max_rms) and (best is None or c["match"]["size"] > res["cands"][best]["match"]["size"]):
                best = i
        if best is not None:
            c = res["cands"][best]
            res.update(found=1, edge=[Ka - 1, b, best, c["match"]["size"]], tf12=c["tf12"], T=c["T"], rms=c["rms"])
    return out


def choose_partners(group_of, linked, rnd):
    """liw_xloop_partner restated"""
    B = len(group_of)
    out = []
    for a in range(B):
        members = [m for m in range(B) if linked[m] and group_of[m] == group_of[a]]
        out.append(members[rnd % len(members)] if group_of[a] >= 0 and not linked[a] and members else -1)
    return out


def link(group_of, partner, found, edge, T, linked, T_g_w, via):
    """liw_xloop_link restated: edge / T per robot as detect() gives them (T 4x4 or None); linked, T_g_w (list of 4x4) and via are
    updated in place -> group_linked"""
    B = len(group_of)
    before = list(linked)
    for r in range(B):
        if before[r] or group_of[r] < 0:
            continue
        p = partner[r]
        if found[r] and 0 <= p < B and p != r and before[p] and group_of[p] == group_of[r]:
            T_g_w[r] = T_g_w[p] @ ref.iso_inv(T[r])
            via[r] = [p, edge[r][0], edge[r][2], edge[r][3]]
            linked[r] = 1
            continue
        for a in range(B):
            if a != r and partner[a] == r and found[a] and before[a] and group_of[a] == group_of[r]:
                T_g_w[r] = T_g_w[a] @ T[a]
                via[r] = [a, edge[a][2], edge[a][0], edge[a][3]]
                linked[r] = 1
                break
    return [group_of[r] if linked[r] else -1 for r in range(B)]


# ---------------------------------------------------------------------------------------------------------------------- the calls
# detect calls of the eight-robot fleets: (key, partner, mask)
CALLS = {
    "main": ([1, 1, 1, 1, 1, 1, 0, 1], [1, 0, 0, 0, 0, 3, 0, 0], None),          # mutual 0 <-> 1; 2, 3 -> 0; 4 (other building) -> 0; 5 -> 3; 7 invalid
    "odd": ([1, 1, 1, 1, 1, 1, 0, 1], [-1, 1, 8, 6, -7, 3, 0, 6], [1, 1, 1, 1, 1, 0, 1, 1]),   # -1, self, out of range, empty partner; 5 masked out
    "claim": ([1, 1, 0, 0, 0, 0, 0, 0], [2, 2, -1, -1, -1, -1, -1, -1], None),   # two linked robots query the unlinked robot 2
}
LONG_CALL = ([0, 1], [-1, 0], None)
KA_KB_PAIRS = [(1, 0), (2, 0)]       # K_a = K_b + submap_count


@functools.lru_cache(maxsize=None)
def restated(name, call):
    key, partner, mask = LONG_CALL if name == "long" else CALLS[call]
    return detect(name, key, partner, mask)


def anchor_T(r):
    return np.eye(4) if r != 4 else tgl._pose(*T_ANCHOR4)


def link_scenarios(name):
    """the link calls -> list of dict(anchors, steps: [(call, partner, expected linked after, via after, group_linked after)], T_g_w)"""
    out = []
    for anchors, calls in (((0, 4), ("main", "main")), ((0, 1, 4), ("claim",))):
        linked = [int(r in anchors) for r in range(8)]
        Tg = [anchor_T(r) for r in range(8)]
        via = [[-1] * 4 for _ in range(8)]
        steps = []
        for call in calls:
            res = restated(name, call)
            partner = CALLS[call][1]
            found = [int(bool(x and x["found"])) for x in res]
            edge = [x["edge"] if x and x.get("key") else [-1, -1, -1, 0] for x in res]
            T = [x.get("T") if x else None for x in res]
            gl = link(GROUP_OF, partner, found, edge, T, linked, Tg, via)
            steps.append(dict(call=call, linked=list(linked), via=[list(v) for v in via], group_linked=gl, T_g_w=[t.copy() for t in Tg]))
        out.append(dict(anchors=anchors, steps=steps))
    return out


def deviation_bound(c):
    """Hard bound on max |T_w1_w2 - truth| of an accepted candidate whose correspondences are all true pairs.  Every corner is within
    NOISE per planar axis of its landmark, and a blended point is a convex combination of such corners, so in the wheel frames a pair
    obeys p1 = R p2 + t + e with |e| <= eps = 2 sqrt(2) NOISE.  For the planar Procrustes solution tan(dtheta) = sum(b x e) / sum(b .
    (b + e)) with b the centred p2, so |dtheta| <= eps / (spread - eps) (Cauchy-Schwarz; spread = rms |b|), and the centroid is mapped
    with an error of at most eps.  Conjugating with isometries keeps both; the translation of T_w1_w2 is the image of b's world origin,
    which lies |c_b| from the centroid: |dt| <= eps + dtheta |c_b|."""
    eps = 2 * math.sqrt(2) * NOISE
    dth = eps / (c["spread"] - eps)
    return eps + dth * max(1.0, float(np.linalg.norm(c["P2w"].mean(axis=0))))


def check(name):
    """what is wrong with the cases of a fleet (the guards of tests/test_loop_cross_cases.py, in one place so that SEED can be found by
    a search): a list of strings, empty when the cases are decided away from every threshold"""
    bad = []
    mm = MIN_MATCH[name]
    margins = []
    for call in (["long"] if name == "long" else list(CALLS)):
        for a, r in enumerate(restated(name, call)):
            if not r or not r.get("key"):
                continue
            sizes = {i: c["match"]["size"] for i, c in r["cands"].items() if not c["gate"]}
            for c in r["cands"].values():
                margins += c["margins"]
                if "rms" in c and abs(c["rms"] - MAX_RMS) <= REL * MAX_RMS:
                    bad.append("%s %s %d: rms at max_rms" % (name, call, a))
            if r["found"]:
                win = r["edge"][3]
                if win - mm < 2:
                    bad.append("%s %s %d: chosen size %d within 1 of min_match" % (name, call, a, win))
                ties = [i for i, c in r["cands"].items() if "rms" in c and not c["rms"] > MAX_RMS and c["match"]["size"] == win]
                tie_case = name != "long" and call == "main" and a == 5
                if (len(ties) > 1) != tie_case:
                    bad.append("%s %s %d: chosen size ties %s" % (name, call, a, ties))
                dev = float(np.abs(r["T"] - truth(name, a, r["edge"][1])).max())
                if not dev < deviation_bound(r["cands"][r["edge"][2]]):
                    bad.append("%s %s %d: deviation %g" % (name, call, a, dev))
            elif sizes and max(sizes.values()) > mm - 2:
                bad.append("%s %s %d: not found with size %d within 1 of min_match" % (name, call, a, max(sizes.values())))
    if margins and min(margins) <= tgl.MARGIN:
        bad.append("%s: an angle within %g of a bin boundary" % (name, tgl.MARGIN))
    return bad
