"""Cases and the per-robot checker of the fleet pre-integration (include/liw_preint_batch.h, preint_batch.FleetPreint), shared by
tests/test_preint_batch_abi.py and tests/test_gpu_preint_batch.py.

Message streams come from synth._Truth.imu / T_w_o, seeded.  The checker is the host accumulators (liw.ImuPreintegration,
liw.WheelPreintegration).  They cannot be copied, and update_only_t changes them, so what a push is expected to emit is a REPLAY: the
robot's whole history (messages, and update_only_t + reset at every committed scan) goes into a fresh pair of accumulators, which is
then aligned with the scan stamp.  test_preint_batch_abi.py checks that replay against accumulators that really were carried across a
skipped scan."""
import numpy as np

B_BASE, F_BASE = 7, 6
FRAME_DT = 0.1
# where in a frame's interval its wheel messages lie: three messages are 0.03 s apart, so the middle one fails the 0.05 s gate
WHEEL_AT = {0: [], 1: [0.6], 2: [0.25, 0.85], 3: [0.2, 0.5, 0.8]}


def imu_rows(tr, rng, t0, t1, n):
    """n IMU messages (t, acc, gyro) in (t0, t1], the last one a little before t1"""
    out = np.zeros((n, 7))
    for i in range(n):
        t = t0 + (t1 - t0) * (i + 0.9) / n
        acc, gyro = tr.imu(t)
        out[i, 0], out[i, 1:4], out[i, 4:7] = t, acc + rng.normal(0.0, 0.01, 3), gyro + rng.normal(0.0, 0.001, 3)
    return out


def wheel_rows(tr, rng, times):
    out = np.zeros((len(times), 13))
    for i, t in enumerate(times):
        T = tr.T_w_o(t)
        out[i, 0], out[i, 1:10], out[i, 10:13] = t, T[:3, :3].reshape(9), T[:3, 3] + rng.normal(0.0, 2e-4, 3)
    return out


def base_case(synth, seed=4100):
    """B = 7 robots x 6 frames in which every arm of a push occurs (test_gpu_preint_batch.py asserts that each did):
      robot 0  17 IMU messages a frame          robot 1  2 a frame          robot 2  1 a frame
      robot 3  its first IMU messages arrive in frame 3 and its first wheel messages in frame 4 (1-based): the latch
      robot 4  not taken in frame 3 (one merged interval)      robot 5  not taken in frames 3 and 4 (two)
      robot 6  no IMU message at all (never ready); its stamps jump by 10.6 s before frame 4: update_by_v returns
    wheel counts cycle through 0 .. 3; with three messages in a frame the middle one comes less than 0.05 s after the last add.
    -> dict(prm, B, F, stamps [F, B], bias [F, B, 6], taken [F, B] uint8, imu [F][B] rows, wheel [F][B] rows)"""
    prm = synth.office_params()
    rng = np.random.default_rng(seed)
    B, F = B_BASE, F_BASE
    trs = [synth._Truth(prm, yaw_rate=0.25 + 0.05 * b, radius=4.0 + 0.5 * b) for b in range(B)]
    stamps = np.zeros((F, B))
    for b in range(B):
        stamps[:, b] = 1.0 + 0.013 * b + FRAME_DT * (1 + np.arange(F))
    stamps[3:, 6] += 10.6
    imu_n = np.array([[17, 2, 1, 0, 5, 4, 0]] * F)
    imu_n[2:, 3] = 3
    wheel_n = np.array([[(b + k) % 4 for b in range(B)] for k in range(F)])
    wheel_n[:, 3] = [0, 0, 0, 3, 2, 2]
    wheel_n[:, 6] = [2, 1, 2, 2, 2, 3]
    taken = np.ones((F, B), dtype=np.uint8)
    taken[2, 4] = 0
    taken[2:4, 5] = 0
    imu, wheel = [], []
    for k in range(F):
        imu.append([])
        wheel.append([])
        for b in range(B):
            t1 = stamps[k, b]
            t0 = t1 - FRAME_DT
            imu[k].append(imu_rows(trs[b], rng, t0, t1, int(imu_n[k, b])))
            wheel[k].append(wheel_rows(trs[b], rng, [t0 + FRAME_DT * f for f in WHEEL_AT[int(wheel_n[k, b])]]))
    return dict(prm=prm, B=B, F=F, stamps=stamps, bias=rng.normal(0.0, 1e-2, (F, B, 6)), taken=taken, imu=imu, wheel=wheel)


def closed_case(synth, seed=4200):
    """7 robots x 5 frames, every frame taken, every robot with IMU messages (17, 2, 1, 5, 4, 3, 8 a frame) and two wheel messages in
    every frame: once a robot is ready its intervals are the closed ones BatchPreint integrates"""
    prm = synth.office_params()
    rng = np.random.default_rng(seed)
    B, F = 7, 5
    trs = [synth._Truth(prm, yaw_rate=0.2 + 0.04 * b) for b in range(B)]
    stamps = np.stack([1.0 + 0.007 * np.arange(B) + FRAME_DT * (1 + k) for k in range(F)])
    counts = [17, 2, 1, 5, 4, 3, 8]
    imu = [[imu_rows(trs[b], rng, stamps[k, b] - FRAME_DT, stamps[k, b], counts[b]) for b in range(B)] for k in range(F)]
    wheel = [[wheel_rows(trs[b], rng, [stamps[k, b] - FRAME_DT + FRAME_DT * f for f in WHEEL_AT[2]]) for b in range(B)] for k in range(F)]
    return dict(prm=prm, B=B, F=F, stamps=stamps, bias=rng.normal(0.0, 1e-2, (F, B, 6)), taken=np.ones((F, B), dtype=np.uint8), imu=imu, wheel=wheel)


def pack(case, k, robots=None, imu_part=None, wheel_part=None):
    """the ragged arrays of frame k for the robots `robots` (indices into the case; None: all): imu_off [n + 1] int32, imu [., 7],
    wheel_off, wheel [., 13], stamps [n], bias [n, 6], taken [n].  imu_part / wheel_part: a function rows -> rows applied per robot
    (to push a part of a frame's messages)"""
    robots = list(range(case["B"])) if robots is None else list(robots)
    ip = imu_part or (lambda r: r)
    wp = wheel_part or (lambda r: r)
    im = [ip(case["imu"][k][b]) for b in robots]
    wm = [wp(case["wheel"][k][b]) for b in robots]
    off = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    cat = lambda rows, w: np.ascontiguousarray(np.concatenate([r.reshape(-1, w) for r in rows], axis=0)) if rows else np.zeros((0, w))
    return dict(imu_off=off(im), imu=cat(im, 7), wheel_off=off(wm), wheel=cat(wm, 13), stamps=np.ascontiguousarray(case["stamps"][k, robots]),
                bias=np.ascontiguousarray(case["bias"][k, robots]), taken=np.ascontiguousarray(case["taken"][k, robots]))


class Replay:
    """a robot's history replayed into fresh host accumulators, with the members the host handles do not show mirrored in Python"""

    def __init__(self, liw, prm, events):
        self.imu, self.wheel = liw.ImuPreintegration(prm), liw.WheelPreintegration(prm)
        self.imu_inited = self.wheel_odom_inited = False
        self.last_add_imu_time, self.last_acc, self.last_gyro = -1.0, np.zeros(3), np.zeros(3)
        self.last_update_time, self.last_add_time = -1.0, 0.0
        self.arms = set()
        for e in events:
            getattr(self, e[0])(*e[1:])

    def add_imu(self, row):
        if self.imu.add_imu_measure(row[0], row[1:4], row[4:7]):
            self.imu_inited = True
        self.last_add_imu_time, self.last_acc, self.last_gyro = float(row[0]), row[1:4].copy(), row[4:7].copy()

    def add_wheel(self, row):
        t = float(row[0])
        seeded = self.last_update_time >= 0
        done = self.wheel.add_wheel_odom_measure(t, row[1:10], row[10:13])
        if not seeded:
            assert not done
            self.arms.add("seed")
        elif done:
            self.arms.add("gap" if t - self.last_update_time >= 10 else "integrated")
            self.wheel_odom_inited = True
        else:
            assert t - self.last_add_time < 0.05
            self.arms.add("gated")
        if done or not seeded:
            self.last_add_time = self.last_update_time = t

    def align(self, stamp):
        """update_only_t of both accumulators, as the reference does before it takes the result (:118-119)"""
        self.wheel.update_only_t(stamp)
        self.imu.update_only_t(stamp)
        if self.last_update_time >= 0:
            if stamp - self.last_update_time >= 10:
                self.arms.add("gap")
            self.last_update_time = float(stamp)
        if self.last_add_imu_time != -1:
            self.last_add_imu_time = float(stamp)

    def reset(self, stamp, bias):
        """a committed scan: align, then reset_wheel_odom_measure / reset_imu_measure (:118-123)"""
        self.align(stamp)
        self.wheel.reset_wheel_odom_measure(stamp)
        self.imu.reset_imu_measure(stamp, bias[0:3], bias[3:6])
        self.last_update_time = self.last_add_imu_time = float(stamp)

    def result(self):
        X, J, S, Dt = self.imu.get_preintegraption_result()
        T, Sw, Dtw = self.wheel.get_preintegraption_result()
        return dict(imu_X=X, imu_J=np.asarray(J).reshape(225), imu_sqrtP=np.asarray(S).reshape(225), imu_Dt=Dt, wheel_T=np.asarray(T),
                    wheel_sqrtP=np.asarray(Sw).reshape(9), wheel_Dt=Dtw)


class HostFleet:
    """the expected side of a run: an event log per robot.  push() logs a frame's messages and returns, per robot, what the device is
    expected to hold (`persisted`: the un-aligned accumulators) and to emit (`rows`: after update_only_t(stamp) on a copy) and
    `ready`; commit() logs the reset of the robots that are taken and ready."""

    def __init__(self, liw, prm, B):
        self.liw, self.prm, self.B = liw, prm, B
        self.events = [[] for _ in range(B)]
        self.pending = [None] * B
        self.ready = np.zeros(B, dtype=np.uint8)
        self.arms = set()

    def push(self, imu, wheel, stamps, bias):
        out = []
        for b in range(self.B):
            self.events[b] += [("add_imu", r) for r in imu[b]] + [("add_wheel", r) for r in wheel[b]]
            self.pending[b] = (float(stamps[b]), np.array(bias[b]))
            rp = Replay(self.liw, self.prm, self.events[b])
            persisted = dict(rp.result(), last_add_imu_time=rp.last_add_imu_time, last_acc=rp.last_acc, last_gyro=rp.last_gyro,
                             last_update_time=rp.last_update_time, last_add_time=rp.last_add_time, imu_inited=int(rp.imu_inited),
                             wheel_odom_inited=int(rp.wheel_odom_inited), pending_stamp=float(stamps[b]), pending_bias=np.array(bias[b]))
            rp.align(float(stamps[b]))
            self.arms |= rp.arms
            self.ready[b] = int(rp.imu_inited and rp.wheel_odom_inited)
            out.append(dict(persisted=persisted, rows=rp.result(), ready=int(self.ready[b])))
        return out

    def commit(self, taken):
        done = np.zeros(self.B, dtype=np.uint8)
        for b in range(self.B):
            if taken[b] and self.ready[b]:
                self.events[b].append(("reset",) + self.pending[b])
                done[b] = 1
        return done


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))
