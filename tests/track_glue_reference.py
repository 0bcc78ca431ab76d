"""The glue of a tracking frame, restated on the host: what lvio_2d::trajectory::add_sensor_data(laser) does between the heavy
stages while status == TRACKING (include/lvio_2d_trajectory.hpp:94-127 and :153-173), over the exported liw_lie_* routines through
ctypes — the reference of tests/test_gpu_laser_track.py — next to an independent plain-numpy restatement (4 x 4 matrices,
synth.exp_so3, an arccos / skew logarithm) that tests/test_laser_track_abi.py compares it with, the case generator of those tests,
and a frame loop whose glue is this restatement fed from read-backs (HostGlueTracker: the other side of the free-running
comparison and the baseline of tools/bench_laser_batch.py --track).

A helper module, not a conftest."""
import ctypes as C

import numpy as np

FACTORS = (0.5, 0.98, 1.02, 2.0)          # of min_delta_t, of the key-frame translation and of the rotation threshold
COUNT_CASES = ("fewer", "equal", "more", "empty")   # n_match < n_no_match, ==, >, and count = 0 with an empty scan
N_COMBOS = len(FACTORS) ** 3 * len(COUNT_CASES)
MAX_ANGLE = 3.0


def param_sets(liw, synth, projected=False):
    """(name, track params, laser params) of the office set and of a second one (second_config.skewed_params: a wheel extrinsic with
    a 0.48 rad turn and a lever arm, a laser extrinsic off the office value; other thresholds).  The office extrinsics are the 7-digit
    values of the configuration file, which the loader's quaternion round trip leaves 1e-7 off orthonormal; projected = True projects
    the rotations of both sets onto SO3 first (synth.normalize_extrinsic), the second set's always are."""
    import second_config
    out = []
    for name, prm in (("office", synth.office_params()), ("second", second_config.skewed_params(synth))):
        if projected or name == "second":
            prm = dict(prm, **{k: [float(v) for v in synth.normalize_extrinsic(prm[k]).reshape(16)] for k in ("T_imu_to_wheel", "T_imu_to_laser")})
        tp = dict(liw.laser_batch.office_track_params(prm), min_delta_t=0.01)
        if name == "second":
            tp.update(key_frame_p_motion_threshold=0.07, key_frame_q_motion_threshold=0.03)
        out.append((name, tp, liw.laser.office_laser_params(prm)))
    return out


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _v(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Lie:
    """liw_lie.h on numpy arrays; a transform is T12 = R (9, row-major) then t (3)"""

    def __init__(self, liw):
        self.L = liw.lib()

    def from_matrix16(self, M16, normalize):
        T = np.zeros(12)
        self.L.liw_lie_from_matrix16(_pd(_v(M16).reshape(16)), C.c_int(int(bool(normalize))), _pd(T))
        return T

    def make_tf(self, p, q):
        T = np.zeros(12)
        self.L.liw_lie_make_tf(_pd(_v(p)), _pd(_v(q)), _pd(T))
        return T

    def mul(self, A, B):
        out = np.zeros(12)
        self.L.liw_lie_mul(_pd(_v(A)), _pd(_v(B)), _pd(out))
        return out

    def inverse(self, A):
        out = np.zeros(12)
        self.L.liw_lie_inverse(_pd(_v(A)), _pd(out))
        return out

    def exp_so3(self, a):
        R = np.zeros(9)
        self.L.liw_lie_exp_so3(_pd(_v(a)), _pd(R))
        return R

    def log_SO3(self, R9):
        a = np.zeros(3)
        self.L.liw_lie_log_SO3(_pd(_v(R9)), _pd(a))
        return a

    def log_SE3(self, T):
        p, q = np.zeros(3), np.zeros(3)
        self.L.liw_lie_log_SE3(_pd(_v(T)), _pd(p), _pd(q))
        return p, q


class Glue:
    """the restatement for one parameter set: tp a liw_lfe_track_params dict, T_imu_to_laser16 / normalize as the laser parameters
    hold them.  Statements in the order of the reference, one robot at a time."""

    def __init__(self, liw, tp, T_imu_to_laser16, normalize_laser):
        self.lie = Lie(liw)
        self.tp = dict(tp)
        self.Tiw = self.lie.from_matrix16(tp["T_imu_to_wheel"], tp["normalize_extrinsics"])
        self.Til = self.lie.from_matrix16(T_imu_to_laser16, normalize_laser)

    def twist(self, state, angular_local):   # :94-109
        lie = self.lie
        T_w_laser = lie.mul(lie.make_tf(state[0:3], state[3:6]), self.Til)
        v = state[6:9]
        Rt_v = np.array([T_w_laser[0 * 3 + i] * v[0] + T_w_laser[1 * 3 + i] * v[1] + T_w_laser[2 * 3 + i] * v[2] for i in range(3)])
        A, B = np.zeros(12), np.zeros(12)
        A[:9], B[:9] = lie.exp_so3(angular_local), self.Til[:9]
        Cm = lie.mul(lie.inverse(B), A)
        return Rt_v, lie.log_SO3(lie.mul(Cm, B)[:9])

    def skip(self, imu_Dt):   # :115
        return bool(imu_Dt < self.tp["min_delta_t"])

    def predict(self, state, wheel_T):   # :125-127, :204-209, :228-234
        lie = self.lie
        delta = lie.mul(lie.mul(self.Tiw, wheel_T), lie.inverse(self.Tiw))
        p, q = lie.log_SE3(lie.mul(lie.make_tf(state[0:3], state[3:6]), delta))
        return np.concatenate([p, q])

    def angular_local(self, imu_X, imu_Dt):   # :124
        return np.array([imu_X[6 + k] / imu_Dt for k in range(3)])

    def tf_w_l(self, pose):   # :154-155
        return self.lie.mul(self.lie.make_tf(pose[0:3], pose[3:6]), self.Til)

    def delta(self, last_keyframe_tf, pose):   # :161-163 and is_static's log_SE3: (|dp|, |dq|)
        lie = self.lie
        dp, dq = lie.log_SE3(lie.mul(lie.inverse(last_keyframe_tf), self.tf_w_l(pose)))
        return float(np.sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2])), float(np.sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2]))

    def key(self, last_keyframe_tf, pose, n_match, n_lines):   # :164-167
        dp, dq = self.delta(last_keyframe_tf, pose)
        static = dp < self.tp["key_frame_p_motion_threshold"] and dq < self.tp["key_frame_q_motion_threshold"]
        return bool((not static) or int(n_match) < int(n_lines) - int(n_match))


# ------------------------------------------------------------------------------------------- the independent numpy restatement
def _log_np(R):
    """arccos / skew logarithm of a rotation matrix (angles up to pi - 1e-3: the generator stays below MAX_ANGLE)"""
    c = max(-1.0, min(1.0, (np.trace(R) - 1.0) * 0.5))
    th = float(np.arccos(c))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-6:   # arccos loses half the digits near 0: the skew part is exact to second order there
        return 0.5 * v
    s = float(np.linalg.norm(v)) * 0.5          # sin(th), better conditioned than arccos below pi / 4 and above 3 pi / 4
    if c > 0.7:
        th = float(np.arcsin(min(1.0, s)))
    elif c < -0.7:
        th = float(np.pi - np.arcsin(min(1.0, s)))
    return v * (th / (2.0 * s))


class GlueNumpy:
    """the same statements on 4 x 4 matrices with synth.exp_so3 and _log_np.  T12_wheel / T12_laser: the extrinsics as the loader
    holds them (Glue.Tiw / .Til), so that the comparison is about the glue; without them the given matrices, projected onto SO3 when
    normalisation is asked for.  The two logarithms agree to round-off only on rotations: compare at param_sets(projected=True)."""

    def __init__(self, synth, tp, T_imu_to_laser16, normalize_laser, T12_wheel=None, T12_laser=None):
        self.s, self.tp = synth, dict(tp)
        load = lambda M, nrm: synth.normalize_extrinsic(M) if nrm else np.asarray(M, dtype=np.float64).reshape(4, 4).copy()
        self.Tiw = load(tp["T_imu_to_wheel"], tp["normalize_extrinsics"]) if T12_wheel is None else self.m4(T12_wheel)
        self.Til = load(T_imu_to_laser16, normalize_laser) if T12_laser is None else self.m4(T12_laser)

    @staticmethod
    def m4(T12):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = np.asarray(T12[:9]).reshape(3, 3), T12[9:12]
        return T

    def tf(self, pose):
        return self.s.se3(self.s.exp_so3(np.asarray(pose[3:6], dtype=np.float64)), np.asarray(pose[0:3], dtype=np.float64))

    def twist(self, state, angular_local):
        Rwl = (self.tf(state) @ self.Til)[:3, :3]
        Ril = self.Til[:3, :3]
        return Rwl.T @ np.asarray(state[6:9]), _log_np(Ril.T @ self.s.exp_so3(np.asarray(angular_local, dtype=np.float64)) @ Ril)

    def predict(self, state, wheel_T):
        N = self.tf(state) @ self.Tiw @ self.m4(wheel_T) @ self.s.inv_se3(self.Tiw)
        return np.concatenate([N[:3, 3], _log_np(N[:3, :3])])

    def tf_w_l(self, pose):
        T = self.tf(pose) @ self.Til
        return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])

    def delta(self, last_keyframe_tf, pose):
        D = self.s.inv_se3(self.m4(last_keyframe_tf)) @ self.tf(pose) @ self.Til
        return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(_log_np(D[:3, :3])))


# ------------------------------------------------------------------------------------------------------------ the generator
def _unit(rng):
    v = rng.normal(0.0, 1.0, 3)
    return v / np.linalg.norm(v)


def make_cases(glue, synth, B, pool_lines, seed=0, page=0):
    """B robots for liw_lfe_track_begin / _end.  Robot b takes combination 101 (page * B + b) % N_COMBOS of FACTORS^3 x COUNT_CASES:
    imu_Dt = f * min_delta_t; the key-frame delta (last_keyframe_tf^-1 * tf_w_l at the pose the frame ends with: the predicted one,
    or the unchanged one when the gate skips) has translation norm f * p threshold and rotation angle f * q threshold; count sits on
    the asked side of n_lines - count.  pool_lines: the line counts of the scans the test can put in slot 0 — it must hold a 0 (the
    empty scan) and a positive even count (the equality).  Every rotation angle of a pose is at most MAX_ANGLE.
    -> dict of arrays: x [B, 2, 15], kf_pose [B, 6] (last_keyframe_tf = make_tf of it), angular_local [B, 3], imu_X [B, 15],
    imu_Dt [B], wheel_T [B, 12], stamps [B], scan [B] (index into the pool), count [B] int32, combo [B, 4]"""
    rng = np.random.default_rng(seed)
    lie, tp = glue.lie, glue.tp
    pool_lines = [int(v) for v in pool_lines]
    empties = [i for i, n in enumerate(pool_lines) if n == 0]
    evens = [i for i, n in enumerate(pool_lines) if n > 0 and n % 2 == 0]
    full = [i for i, n in enumerate(pool_lines) if n >= 4]
    assert empties and evens and full
    o = dict(x=np.zeros((B, 2, 15)), kf_pose=np.zeros((B, 6)), angular_local=np.zeros((B, 3)), imu_X=np.zeros((B, 15)), imu_Dt=np.zeros(B),
             wheel_T=np.zeros((B, 12)), stamps=np.zeros(B), scan=np.zeros(B, dtype=np.int64), count=np.zeros(B, dtype=np.int32),
             combo=np.zeros((B, 4), dtype=np.int64))
    nf = len(FACTORS)
    for b in range(B):
        ci = ((page * B + b) * 101) % N_COMBOS   # 101 is coprime with N_COMBOS: N_COMBOS robots in a row take every combination, mixed
        i_dt, i_p, i_q, i_c = np.unravel_index(ci, (nf, nf, nf, len(COUNT_CASES)))
        o["combo"][b] = (i_dt, i_p, i_q, i_c)
        while True:
            x = np.zeros((2, 15))
            for r in range(2):
                x[r, 0:3] = rng.uniform(-8.0, 8.0, 3)
                x[r, 3:6] = _unit(rng) * rng.uniform(0.05, 2.6)
                x[r, 6:9] = rng.uniform(-1.5, 1.5, 3)
                x[r, 9:15] = rng.normal(0.0, 1e-2, 6)
            wheel = lie.make_tf(rng.uniform(-0.2, 0.2, 3), _unit(rng) * rng.uniform(0.01, 0.25))
            Dt = FACTORS[i_dt] * tp["min_delta_t"]
            pose_end = x[1, 0:6].copy() if glue.skip(Dt) else glue.predict(x[1], wheel)
            # last_keyframe_tf = tf_w_l * D^-1 with |D.t| and the angle of D.R at the asked multiples of the thresholds
            D = lie.make_tf(_unit(rng) * FACTORS[i_p] * tp["key_frame_p_motion_threshold"], _unit(rng) * FACTORS[i_q] * tp["key_frame_q_motion_threshold"])
            kp, kq = lie.log_SE3(lie.mul(glue.tf_w_l(pose_end), lie.inverse(D)))
            if max(np.linalg.norm(pose_end[3:6]), np.linalg.norm(kq)) <= MAX_ANGLE - 0.05:
                break
        o["x"][b], o["kf_pose"][b], o["wheel_T"][b], o["imu_Dt"][b] = x, np.concatenate([kp, kq]), wheel, Dt
        o["angular_local"][b] = _unit(rng) * rng.uniform(0.05, 1.5)
        o["imu_X"][b] = rng.normal(0.0, 0.05, 15)
        o["stamps"][b] = 100.0 + 0.1 * b
        o["scan"][b], o["count"][b] = _scan_and_count(COUNT_CASES[i_c], b, pool_lines)
    return o


def _scan_and_count(case, b, pool_lines):
    """the scan of the pool and the match count that put robot b on the asked side of n_match < n_lines - n_match"""
    empties = [i for i, n in enumerate(pool_lines) if n == 0]
    evens = [i for i, n in enumerate(pool_lines) if n > 0 and n % 2 == 0]
    full = [i for i, n in enumerate(pool_lines) if n >= 4]
    if case == "empty":
        return empties[b % len(empties)], 0
    if case == "equal":
        s = evens[b % len(evens)]
        return s, pool_lines[s] // 2
    s = full[b % len(full)]
    return s, ((pool_lines[s] - 1) // 2 if case == "fewer" else pool_lines[s] // 2 + 1)


PLANAR_MAX_ANGLE = np.pi - 1e-3   # the range the restatements state


def planar_yaws():
    """+-pi/2, +-3 pi/4, +-(pi - 2e-3) and the two neighbouring doubles of each: 18 angles.  The half angle exp_so3 takes of the first
    is the double nearest pi/4, the arguments of the third sit next to pi/2: where a sine or a cosine reduced without enough words of
    pi is wrong"""
    out = []
    for base in (np.pi / 2, 3 * np.pi / 4, np.pi - 2e-3):
        for sgn in (1.0, -1.0):
            out += [sgn * np.nextafter(base, 0.0), sgn * base, sgn * np.nextafter(base, 4.0)]
    return out


def make_planar_cases(glue, synth, B, pool_lines, seed=0, page=0):
    """make_cases for the workload's own geometry, a robot that turns about z only: the state rotation vectors are (0, 0, yaw) with
    the yaws of planar_yaws() (robot b takes number b % 18 in its current row), positions and velocities lie in the plane, the wheel
    increment is a pure yaw with a planar translation and current_angular_local is along z.  The combinations of FACTORS^3 x
    COUNT_CASES, the key-frame delta and the counts are make_cases's.  Every rotation angle a logarithm returns (the predicted pose,
    the key-frame pose) is at most PLANAR_MAX_ANGLE."""
    rng = np.random.default_rng(seed)
    lie, tp = glue.lie, glue.tp
    pool_lines = [int(v) for v in pool_lines]
    yaws = planar_yaws()
    o = dict(x=np.zeros((B, 2, 15)), kf_pose=np.zeros((B, 6)), angular_local=np.zeros((B, 3)), imu_X=np.zeros((B, 15)), imu_Dt=np.zeros(B),
             wheel_T=np.zeros((B, 12)), stamps=np.zeros(B), scan=np.zeros(B, dtype=np.int64), count=np.zeros(B, dtype=np.int32),
             combo=np.zeros((B, 4), dtype=np.int64))
    nf = len(FACTORS)
    for b in range(B):
        ci = ((page * B + b) * 101) % N_COMBOS
        i_dt, i_p, i_q, i_c = np.unravel_index(ci, (nf, nf, nf, len(COUNT_CASES)))
        o["combo"][b] = (i_dt, i_p, i_q, i_c)
        x = np.zeros((2, 15))
        for r in range(2):
            x[r, 0:2] = rng.uniform(-8.0, 8.0, 2)
            x[r, 5] = yaws[(b + 7 * (1 - r)) % len(yaws)]
            x[r, 6:8] = rng.uniform(-1.5, 1.5, 2)
            x[r, 9:15] = rng.normal(0.0, 1e-2, 6)
        Dt = FACTORS[i_dt] * tp["min_delta_t"]
        for attempt in range(200):
            turn = rng.uniform(0.01, 0.25) * (-np.sign(x[1, 5]) if attempt % 4 < 3 else np.sign(x[1, 5]))   # mostly away from pi
            wheel = lie.make_tf(np.concatenate([rng.uniform(-0.2, 0.2, 2), [0.0]]), np.array([0.0, 0.0, turn]))
            pose_end = x[1, 0:6].copy() if glue.skip(Dt) else glue.predict(x[1], wheel)
            D = lie.make_tf(_unit(rng) * FACTORS[i_p] * tp["key_frame_p_motion_threshold"], _unit(rng) * FACTORS[i_q] * tp["key_frame_q_motion_threshold"])
            kp, kq = lie.log_SE3(lie.mul(glue.tf_w_l(pose_end), lie.inverse(D)))
            if max(np.linalg.norm(pose_end[3:6]), np.linalg.norm(kq)) <= PLANAR_MAX_ANGLE:
                break
        else:
            raise AssertionError("no planar case within the restatement's range for robot %d" % b)
        o["x"][b], o["kf_pose"][b], o["wheel_T"][b], o["imu_Dt"][b] = x, np.concatenate([kp, kq]), wheel, Dt
        o["angular_local"][b] = np.array([0.0, 0.0, rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 1.5)])
        o["imu_X"][b] = rng.normal(0.0, 0.05, 15)
        o["stamps"][b] = 100.0 + 0.1 * b
        o["scan"][b], o["count"][b] = _scan_and_count(COUNT_CASES[i_c], b, pool_lines)
    return o


def expected(glue, cases, pool_lines, mask=None, end_mask=None):
    """what track_init (from kf_pose / angular_local) -> track_begin -> track_end leave, by the restatement and a plain state machine:
    dict(linear, angular, skip, x, pose_new, key, pose, kf [B, 12], ang [B, 3], stamp [B], counters [B, 3] = tracked, keys, skipped,
    dp, dq [B] the key-frame delta norms).  Rows of robots with mask[b] == 0 are NaN / -1 (nothing is written for them); end_mask is
    track_end's (default: mask)."""
    B = cases["x"].shape[0]
    mask = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    end_mask = mask if end_mask is None else np.asarray(end_mask, dtype=bool)
    nan = lambda *s: np.full(s, np.nan)
    e = dict(linear=nan(B, 3), angular=nan(B, 3), skip=np.full(B, -1), x=cases["x"].copy(), pose_new=nan(B, 6), key=np.full(B, -1), pose=nan(B, 6),
             kf=nan(B, 12), ang=nan(B, 3), stamp=nan(B), counters=np.full((B, 3), -1), dp=nan(B), dq=nan(B))
    for b in range(B):
        if not mask[b]:
            continue
        kf = glue.lie.make_tf(cases["kf_pose"][b, 0:3], cases["kf_pose"][b, 3:6])
        ang, stamp, cnt = cases["angular_local"][b].copy(), 0.0, [0, 0, 0]
        x = e["x"][b]
        e["linear"][b], e["angular"][b] = glue.twist(x[1], ang)
        sk = glue.skip(cases["imu_Dt"][b])
        e["skip"][b] = int(sk)
        if sk:
            cnt[2] += 1
        else:
            x[0] = x[1]
            x[1, 0:6] = glue.predict(x[1], cases["wheel_T"][b])
            ang = glue.angular_local(cases["imu_X"][b], cases["imu_Dt"][b])
            stamp = cases["stamps"][b]
            e["pose_new"][b] = x[1, 0:6]
        if end_mask[b]:
            pose = x[1, 0:6].copy()
            e["pose"][b] = pose
            e["dp"][b], e["dq"][b] = glue.delta(kf, pose)
            k = glue.key(kf, pose, cases["count"][b], pool_lines[cases["scan"][b]])
            e["key"][b] = int(k)
            cnt[0] += 1
            if k:
                cnt[1] += 1
                kf = glue.tf_w_l(pose)
        e["kf"][b], e["ang"][b], e["stamp"][b], e["counters"][b] = kf, ang, stamp, cnt
    return e


# ------------------------------------------------------------------------------------- a frame loop with the glue on the host
class HostGlueTracker:
    """FleetTracker.step with the same device stages (a front-end and a two-frame solver of its own) and the glue done on the host
    by `Glue`, robot by robot, from read-backs: the twist, the gate, the roll and the prediction before the scan, the key-frame
    decision after the solve, the restore of skipped robots.  State on the host: x [B, 2, 15], kf [B, 12], ang [B, 3],
    counters [B, 3]."""

    def __init__(self, liw, prm, laser_prm, track_prm, dims, device="cuda:0", cap=256, max_corners=64, acc_cap=1024):
        import torch
        self.liw, self.torch = liw, torch
        self.glue = Glue(liw, track_prm, laser_prm["T_imu_to_laser"], laser_prm.get("normalize_extrinsics", True))
        self.fe = fe = liw.laser_batch.BatchFrontEnd(laser_prm, dims, device)
        self.B = B = fe.B
        self.cap, self.max_corners = int(cap), int(max_corners)
        self.bs = liw.BatchSolver(prm, [liw.fleet.placeholder_window()], device=device,
                                  tile=dict(B=B, states=np.zeros((B, 2, 15)), match_pose=np.zeros((B, 2, 12))))
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=fe.dev)
        self.x_d, self.match_pose, self.has_match = z(B * 30), z(B * 24), z(B * 2, dt=torch.uint8)
        self.acc, self.n_acc = z(B, int(acc_cap), 3), z(B, dt=torch.int32)
        self.key = np.zeros(B, dtype=np.uint8)
        self.pose = np.zeros((B, 6))

    def start(self, x0, angular_local=None):
        B = self.B
        x0 = np.asarray(x0, dtype=np.float64).reshape(B, 15)
        self.x = np.stack([x0, x0], axis=1).copy()
        self.kf = np.stack([self.glue.lie.make_tf(x0[b, 0:3], x0[b, 3:6]) for b in range(B)])
        self.ang = np.zeros((B, 3)) if angular_local is None else np.asarray(angular_local, dtype=np.float64).reshape(B, 3).copy()
        self.counters = np.zeros((B, 3), dtype=np.int64)
        for k in ("prior_X", "prior_J", "prior_R", "has_prior"):
            self.bs.t[k].zero_()
        self.match_pose.zero_()
        self.has_match.zero_()
        self.n_acc.zero_()
        self.key[:] = 0

    def step(self, ranges, stamps, interval):
        liw, torch, fe, bs, g, B = self.liw, self.torch, self.fe, self.bs, self.glue, self.B
        dev = fe.dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        st = fe._t(stamps, torch.float64, (B,))
        iv = {k: fe._t(interval[k], torch.float64) for k in liw.fleet.INTERVAL_KEYS}
        imu_X, imu_Dt, wheel_T = (iv[k].cpu().numpy().reshape(B, -1) for k in ("imu_X", "imu_Dt", "wheel_T"))
        st_h = st.cpu().numpy()
        lin, ang, skip = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B, dtype=np.uint8)
        for b in range(B):
            lin[b], ang[b] = g.twist(self.x[b, 1], self.ang[b])
            skip[b] = g.skip(imu_Dt[b, 0])
            if skip[b]:
                self.counters[b, 2] += 1
                continue
            self.x[b, 0] = self.x[b, 1]
            self.x[b, 1, 0:6] = g.predict(self.x[b, 1], wheel_T[b])
            self.ang[b] = g.angular_local(imu_X[b], imu_Dt[b, 0])
        keep = (1 - skip).astype(np.uint8)
        robot_bytes = fe.store.numel() // B
        head_v = fe.store.view(B, robot_bytes)[:, :256 + 32]
        head = head_v.clone()
        self.x_d.copy_(up(self.x.reshape(-1)))
        pts, times, n = fe.ranges_to_points(ranges, st)
        fe.deskew(pts, times, n, st, up(lin), up(ang))
        sk_d = up(skip).bool()
        n_sp = torch.where(sk_d, torch.full_like(n, -1), n)
        corners, n_corners = fe.spawn(0, pts, n_sp, times=torch.where(n > 0, times[:, 0], st), corners=self.max_corners)
        m = fe.match(liw.laser_batch.REF, 0, None, up(self.x[:, 1, 0:6]), 0, self.cap)
        pk, Ltot = fe.pack_track(m, n=2, frame=1, out=dict(match_pose=self.match_pose, has_match=self.has_match))
        bs.rebind(dict(iv, x=self.x_d, **pk), Ltot)
        snap = [(bs.t[k], bs.t[k].clone()) for k in ("prior_X", "prior_J", "prior_R", "has_prior")]
        bs.solve(liw.LIW_MODE_TRACK)
        bs.marginalize()
        xs = self.x_d.cpu().numpy().reshape(B, 2, 15)
        count = m["count"].cpu().numpy()
        n_lines = self._n_lines()
        for t, old in snap:
            tv, ov = t.view(B, -1), old.view(B, -1)
            tv.copy_(torch.where(sk_d[:, None], ov, tv))
        prev_key = self.key.copy()
        for b in range(B):
            if skip[b]:
                continue
            self.x[b] = xs[b]
            self.pose[b] = xs[b, 1, 0:6]
            k = g.key(self.kf[b], self.pose[b], count[b], n_lines[b])
            self.key[b] = int(k)
            self.counters[b, 0] += 1
            if k:
                self.counters[b, 1] += 1
                self.kf[b] = g.tf_w_l(self.pose[b])
        self.x_d.copy_(up(self.x.reshape(-1)))
        pose_d = up(self.pose)
        fe.corners_to_world(corners, n_corners, pose_d, self.acc, self.n_acc, mask=keep, clear=prev_key & keep)
        flags = fe.add_scan(0, pose_d, mask=keep, flags=True)
        head_v.copy_(torch.where(sk_d[:, None], head, head_v))
        return dict(skip=skip, key=self.key & keep, flags=flags, pose=self.pose, Ltot=Ltot, acc=self.acc, n_acc=self.n_acc, count=count,
                    laser_off=pk["laser_off"], n_lines=n_lines, n_corners=n_corners)

    def _n_lines(self):
        """the clamped n_lines of scan slot 0 of every robot, read from the slot headers in one copy"""
        fe, B = self.fe, self.B
        robot_bytes = fe.store.numel() // B
        h = fe.store.view(B, robot_bytes)[:, 256:256 + 32].contiguous().view(self.torch.int32).cpu().numpy().reshape(B, 8)
        return np.clip(h[:, 1], 0, fe.dims.max_lines)
