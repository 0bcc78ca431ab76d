"""The glue of an initialising robot, restated on the host: what lvio_2d::trajectory::add_sensor_data(laser) does between the heavy
stages while status == INITIALIZING (include/lvio_2d_trajectory.hpp:111-127: the is_static gate on the wheel increment,
update_current_status, the frame pushed into the window) and init_current_status (:218-227), per robot over the exported liw_lie_*
routines, in the style of tests/track_glue_reference.py whose Lie / Glue / GlueNumpy it builds on; an independent plain-numpy
restatement that tests/test_fleet_init_abi.py compares it with; the raw layout of the 256-byte initialisation record; and the case
generator of tests/test_gpu_fleet_init.py.

A helper module, not a conftest."""
import numpy as np

import track_glue_reference as tg

FACTORS = tg.FACTORS                      # of p_motion_threshold and of q_motion_threshold
INITIALIZING, TRACKING = 0, 1
REC_BYTES = 256
MAX_ANGLE = tg.MAX_ANGLE
INTERVAL = (("imu_X", 15), ("imu_J", 225), ("imu_sqrtP", 225), ("imu_Dt", 1), ("wheel_T", 12), ("wheel_sqrtP", 9))


def init_param_sets(liw, synth, projected=False):
    """(name, track params, laser params, init params) at the office set and at the second one (other thresholds, N = 4 and 6)"""
    out = []
    for name, tp, lp in tg.param_sets(liw, synth, projected=projected):
        ip = dict(slide_window_size=4, p_motion_threshold=0.1, q_motion_threshold=0.1)
        if name == "second":
            ip = dict(slide_window_size=6, p_motion_threshold=0.06, q_motion_threshold=0.13)
        out.append((name, tp, lp, ip))
    return out


class InitGlue(tg.Glue):
    """the restatement for one parameter set: tg.Glue (extrinsics, predict, angular_local) plus the INITIALIZING statements"""

    def __init__(self, liw, tp, T_imu_to_laser16, normalize_laser, ip):
        super().__init__(liw, tp, T_imu_to_laser16, normalize_laser)
        self.ip = dict(ip)

    def laser_delta(self, wheel_T):   # wheel_delta_to(T_imu_to_laser, delta) :210-217
        lie = self.lie
        T_x_to_wheel = lie.mul(lie.inverse(self.Til), self.Tiw)
        return lie.mul(lie.mul(T_x_to_wheel, wheel_T), lie.inverse(T_x_to_wheel))

    def motion(self, wheel_T):   # is_static's log_SE3 :199-203: (|dp|, |dq|)
        dp, dq = self.lie.log_SE3(self.laser_delta(wheel_T))
        return float(np.sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2])), float(np.sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2]))

    def drop(self, wheel_T):   # :114
        dp, dq = self.motion(wheel_T)
        return bool(dp < self.ip["p_motion_threshold"] and dq < self.ip["q_motion_threshold"])

    def init_state(self):   # init_current_status :218-227 -> state [15]
        p, q = self.lie.log_SE3(self.lie.inverse(self.Tiw))
        return np.concatenate([p, q, np.zeros(9)])

    def wheel_for(self, laser_delta):
        """the wheel increment whose laser_delta is the given transform (the generator's inverse of laser_delta)"""
        lie = self.lie
        T_x_to_wheel = lie.mul(lie.inverse(self.Til), self.Tiw)
        return lie.mul(lie.mul(lie.inverse(T_x_to_wheel), laser_delta), T_x_to_wheel)


class InitGlueNumpy(tg.GlueNumpy):
    """the same statements on 4 x 4 matrices (compare at projected extrinsics, as tg.GlueNumpy says)"""

    def motion(self, wheel_T):
        Tlw = self.s.inv_se3(self.Til) @ self.Tiw
        D = Tlw @ self.m4(wheel_T) @ self.s.inv_se3(Tlw)
        return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(tg._log_np(D[:3, :3])))

    def init_state(self):
        T = self.s.inv_se3(self.Tiw)
        return np.concatenate([T[:3, 3], tg._log_np(T[:3, :3]), np.zeros(9)])


# ------------------------------------------------------------------------------------------------------------ the record
def pack_records(state, ang, status, n_frames, counters):
    """raw initialisation records [B, 256] uint8 as include/liw_laser_batch.h lays them out: p q v bs [15 doubles],
    current_angular_local [3], then the ints status, n_frames, initialisations, failed windows, dropped frames; padding zero"""
    B = np.asarray(state).shape[0]
    raw = np.zeros((B, REC_BYTES), dtype=np.uint8)
    d, i = raw.view(np.float64).reshape(B, 32), raw.view(np.int32).reshape(B, 64)
    d[:, 0:15], d[:, 15:18] = state, ang
    i[:, 36], i[:, 37], i[:, 38:41] = status, n_frames, counters
    return raw


def unpack_records(raw, B):
    raw = np.ascontiguousarray(raw).reshape(B, REC_BYTES)
    d, i = raw.view(np.float64).reshape(B, 32), raw.view(np.int32).reshape(B, 64)
    return dict(state=d[:, 0:15], ang=d[:, 15:18], status=i[:, 36], n_frames=i[:, 37], counters=i[:, 38:41], raw=raw)


# ------------------------------------------------------------------------------------------------------------ the generator
N_FRAME_CASES = 4   # n_frames 0, 1, N - 1, and a robot that is already TRACKING
N_COMBOS = len(FACTORS) ** 2 * N_FRAME_CASES


def make_cases(glue, B, seed=0, page=0):
    """B robots for liw_lfe_init_begin.  Robot b takes combination 37 (page * B + b) % N_COMBOS of FACTORS^2 x {n_frames 0, 1, N - 1,
    TRACKING}: the laser-frame increment of its wheel_T has translation norm f_p * p_motion_threshold and rotation angle f_q *
    q_motion_threshold.  States, rates, counters and the interval arrays are random.
    -> dict: state [B, 15], ang [B, 3], status, n_frames [B], counters [B, 3], the six interval arrays [B, w], combo [B, 3]"""
    rng = np.random.default_rng(seed)
    lie, ip = glue.lie, glue.ip
    N = ip["slide_window_size"]
    nf = len(FACTORS)
    o = dict(state=np.zeros((B, 15)), ang=np.zeros((B, 3)), status=np.zeros(B, dtype=np.int32), n_frames=np.zeros(B, dtype=np.int32),
             counters=np.zeros((B, 3), dtype=np.int32), combo=np.zeros((B, 3), dtype=np.int64))
    for k, w in INTERVAL:
        o[k] = rng.normal(0.0, 0.05, (B, w))
    o["imu_Dt"] = rng.uniform(0.02, 0.2, (B, 1))
    for b in range(B):
        ci = ((page * B + b) * 37) % N_COMBOS   # 37 is coprime with N_COMBOS
        i_p, i_q, i_n = np.unravel_index(ci, (nf, nf, N_FRAME_CASES))
        o["combo"][b] = (i_p, i_q, i_n)
        o["status"][b] = TRACKING if i_n == 3 else INITIALIZING
        o["n_frames"][b] = (0, 1, N - 1, 2)[i_n]
        o["counters"][b] = rng.integers(0, 50, 3)
        while True:
            st = np.concatenate([rng.uniform(-8.0, 8.0, 3), tg._unit(rng) * rng.uniform(0.05, 2.6), rng.uniform(-1.5, 1.5, 3), rng.normal(0.0, 1e-2, 6)])
            D = lie.make_tf(tg._unit(rng) * FACTORS[i_p] * ip["p_motion_threshold"], tg._unit(rng) * FACTORS[i_q] * ip["q_motion_threshold"])
            wheel = glue.wheel_for(D)
            if np.linalg.norm(glue.predict(st, wheel)[3:6]) <= MAX_ANGLE - 0.05:
                break
        o["state"][b], o["wheel_T"][b] = st, wheel
        o["ang"][b] = tg._unit(rng) * rng.uniform(0.05, 1.5)
    return o


def expected(glue, c, mask=None):
    """what liw_lfe_init_begin leaves: dict(drop, slot_of [B] (-1: not written), state, ang, status, n_frames, counters (the record),
    row [B] (the x_init row written, -1 none), x_row [B, 15], dp, dq [B])"""
    B = c["state"].shape[0]
    N = glue.ip["slide_window_size"]
    mask = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    e = dict(drop=np.full(B, -1), slot_of=np.full(B, -1), state=c["state"].copy(), ang=c["ang"].copy(), status=c["status"].copy(),
             n_frames=c["n_frames"].copy(), counters=c["counters"].copy(), row=np.full(B, -1), x_row=np.full((B, 15), np.nan),
             dp=np.full(B, np.nan), dq=np.full(B, np.nan))
    for b in range(B):
        if not mask[b] or c["status"][b] != INITIALIZING or c["n_frames"][b] >= N:
            continue
        e["dp"][b], e["dq"][b] = glue.motion(c["wheel_T"][b])
        d = glue.drop(c["wheel_T"][b])
        e["drop"][b] = int(d)
        if d:
            e["counters"][b, 2] += 1
            continue
        k = int(c["n_frames"][b])
        e["state"][b, 0:6] = glue.predict(c["state"][b], c["wheel_T"][b])
        e["ang"][b] = glue.angular_local(c["imu_X"][b], c["imu_Dt"][b, 0])
        e["row"][b], e["x_row"][b] = k, e["state"][b]
        e["slot_of"][b] = 1 + k
        e["n_frames"][b] = k + 1
    return e


# ------------------------------------------------------------------------------------- a frame loop with the glue on the host
class HostGlueTrajectory:
    """FleetTrajectory.step with the stages that were there before it (a front-end, a two-frame solver and INIT solvers of its own)
    and every piece of glue done on the host by `InitGlue`, robot by robot, from read-backs: the gates, the predictions, the window
    bookkeeping, the ready list, the commit, the key-frame decision, the restore of robots that do not track.  The device only does
    what the host tells it for groups of robots: a scan slot is filled by a plain byte copy of slot 0 for the robots of one slot
    index at a time, the compact INIT batch is gathered with index operations and packed by liw_lfe_pack_init on a front-end of the
    bucket's size.  The other side of the cold-start comparison and the Python-loop baseline of tools/bench_laser_batch.py
    --cold-start.  State on the host: status, n_frames, state [B, 15], ang [B, 3], counters [B, 3] (initialisations, failed windows,
    dropped frames), x_init [B, N, 15]; x [B, 2, 15], kf [B, 12], ang_t [B, 3], tcount [B, 3] (tracked, key, skipped frames).
    margin: the smallest |quantity / threshold - 1| any decision saw; min_track / min_front: the fewest matches of a robot that
    tracked a frame / of a frame of a window that was committed."""

    def __init__(self, liw, prm, laser_prm, track_prm, init_prm, dims, device="cuda:0", cap=256, max_corners=64, acc_cap=1024):
        import torch
        self.liw, self.torch, self.prm, self.lp, self.device = liw, torch, prm, laser_prm, device
        self.g = InitGlue(liw, track_prm, laser_prm["T_imu_to_laser"], laser_prm.get("normalize_extrinsics", True), init_prm)
        self.N = N = int(init_prm["slide_window_size"])
        self.fe = fe = liw.laser_batch.BatchFrontEnd(laser_prm, dims, device)
        self.B = B = fe.B
        self.cap, self.max_corners = int(cap), int(max_corners)
        self.bs = liw.BatchSolver(prm, [liw.fleet.placeholder_window()], device=device,
                                  tile=dict(B=B, states=np.zeros((B, 2, 15)), match_pose=np.zeros((B, 2, 12))))
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=fe.dev)
        self.x_d, self.match_pose, self.has_match = z(B * 30), z(B * 24), z(B * 2, dt=torch.uint8)
        self.acc, self.n_acc = z(B, int(acc_cap), 3), z(B, dt=torch.int32)
        self.win = {k: z(B, N - 1, w) for k, w in INTERVAL}
        self.status, self.n_frames, self.counters = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64)
        self.state, self.ang, self.x_init = np.tile(self.g.init_state(), (B, 1)), np.zeros((B, 3)), np.zeros((B, N, 15))
        self.x, self.kf, self.ang_t, self.tcount = np.zeros((B, 2, 15)), np.zeros((B, 12)), np.zeros((B, 3)), np.zeros((B, 3), dtype=np.int64)
        self.key, self.pose = np.zeros(B, dtype=np.uint8), np.zeros((B, 6))
        self.init_bs, self.packers = {}, {}
        self.margin, self.min_track, self.min_front = np.inf, np.inf, np.inf

    def close(self):
        for o in [self.bs, self.fe, *self.init_bs.values(), *self.packers.values()]:
            o.close()

    def _near(self, value, thr):
        self.margin = min(self.margin, abs(value / thr - 1.0))

    def _bucket(self, R):
        b = 1
        while b < R:
            b *= 2
        b, N, liw = min(b, self.B), self.N, self.liw
        if b not in self.init_bs:
            self.init_bs[b] = liw.BatchSolver(self.prm, [liw.fleet.placeholder_init_window(N)], device=self.device,
                                              tile=dict(B=b, states=np.zeros((b, N, 15)), match_pose=np.zeros((b, N, 12))))
            self.packers[b] = liw.laser_batch.BatchFrontEnd(self.lp, dict(B=b, slots=1, max_points=8, max_lines=8, max_cell_entries=8), self.device)
        return b, self.init_bs[b], self.packers[b]

    def step(self, ranges, stamps, interval):
        liw, torch, fe, bs, g, B, N = self.liw, self.torch, self.fe, self.bs, self.g, self.B, self.N
        dev, tp, ip = fe.dev, self.g.tp, self.g.ip
        keys, priors = liw.fleet.INTERVAL_KEYS, liw.fleet.PRIOR_KEYS
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        st = fe._t(stamps, torch.float64, (B,))
        iv = {k: fe._t(interval[k], torch.float64) for k in keys}
        imu_X, imu_Dt, wheel_T = (iv[k].cpu().numpy().reshape(B, -1) for k in ("imu_X", "imu_Dt", "wheel_T"))
        trk = self.status == TRACKING
        lin, ang = np.zeros((B, 3)), np.zeros((B, 3))
        skip, drop, slot_of = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64)
        for b in range(B):
            if trk[b]:
                lin[b], ang[b] = g.twist(self.x[b, 1], self.ang_t[b])
                self._near(imu_Dt[b, 0], tp["min_delta_t"])
                skip[b] = g.skip(imu_Dt[b, 0])
                if skip[b]:
                    self.tcount[b, 2] += 1
                    continue
                self.x[b, 0] = self.x[b, 1]
                self.x[b, 1, 0:6] = g.predict(self.x[b, 1], wheel_T[b])
                self.ang_t[b] = g.angular_local(imu_X[b], imu_Dt[b, 0])
                continue
            dp, dq = g.motion(wheel_T[b])
            self._near(dp, ip["p_motion_threshold"])
            self._near(dq, ip["q_motion_threshold"])
            drop[b] = g.drop(wheel_T[b])
            if drop[b]:
                self.counters[b, 2] += 1
                continue
            k = int(self.n_frames[b])
            self.state[b, 0:6] = g.predict(self.state[b], wheel_T[b])
            self.x_init[b, k] = self.state[b]
            if k >= 1:
                for key, w in INTERVAL:
                    self.win[key][b, k - 1] = iv[key].view(B, w)[b]
            self.ang[b] = g.angular_local(imu_X[b], imu_Dt[b, 0])
            slot_of[b], self.n_frames[b] = 1 + k, k + 1
        keep, taken = trk & ~skip, ~trk & ~drop
        off_d, trk_d, keep_u8 = up(~keep), up(trk), keep.astype(np.uint8)
        rb = fe.store.numel() // B
        sb = (rb - 256) // (fe.slots + 2)
        v = fe.store.view(B, rb)
        head = v[:, :256 + 32].clone()
        self.x_d.copy_(up(self.x.reshape(-1)))
        pts, times, n = fe.ranges_to_points(ranges, st)
        fe.deskew(pts, times, torch.where(trk_d, n, torch.zeros_like(n)), st, up(lin), up(ang))
        n_sp = torch.where(up(keep | taken), n, torch.full_like(n, -1))
        corners, n_corners = fe.spawn(0, pts, n_sp, times=torch.where(n > 0, times[:, 0], st), corners=self.max_corners)
        for s in range(1, N + 1):   # the robots whose frame belongs in slot s: the whole of slot 0, byte for byte
            idx = np.nonzero(taken & (slot_of == s))[0]
            if idx.size:
                i = up(idx)
                v[i, 256 + s * sb:256 + (s + 1) * sb] = v[i, 256:256 + sb]
        m = fe.match(liw.laser_batch.REF, 0, None, up(self.x[:, 1, 0:6]), 0, self.cap)
        m["count"].copy_(torch.where(trk_d, m["count"], torch.zeros_like(m["count"])))
        pk, Ltot = fe.pack_track(m, n=2, frame=1, out=dict(match_pose=self.match_pose, has_match=self.has_match))
        bs.rebind(dict(iv, x=self.x_d, **pk), Ltot)
        snap = [(bs.t[k], bs.t[k].clone()) for k in priors]
        bs.solve(liw.LIW_MODE_TRACK)
        bs.marginalize()
        its = [(s["iterations"], s["termination"]) for s in bs.summaries()]
        xs = self.x_d.cpu().numpy().reshape(B, 2, 15)
        count = m["count"].cpu().numpy()
        n_lines = np.clip(v[:, 256:256 + 32].contiguous().view(torch.int32).cpu().numpy().reshape(B, 8)[:, 1], 0, fe.dims.max_lines)
        for t, old in snap:
            tv, ov = t.view(B, -1), old.view(B, -1)
            tv.copy_(torch.where(off_d[:, None], ov, tv))
        prev_key = self.key.copy()
        for b in np.nonzero(keep)[0]:
            self.x[b] = xs[b]
            self.pose[b] = xs[b, 1, 0:6]
            self.min_track = min(self.min_track, int(count[b]))
            dp, dq = g.delta(self.kf[b], self.pose[b])
            self._near(dp, tp["key_frame_p_motion_threshold"])
            self._near(dq, tp["key_frame_q_motion_threshold"])
            k = g.key(self.kf[b], self.pose[b], count[b], n_lines[b])
            self.key[b] = int(k)
            self.tcount[b, 0] += 1
            if k:
                self.tcount[b, 1] += 1
                self.kf[b] = g.tf_w_l(self.pose[b])
        pose_d = up(self.pose)
        fe.corners_to_world(corners, n_corners, pose_d, self.acc, self.n_acc, mask=keep_u8, clear=prev_key & keep_u8)
        flags = fe.add_scan(0, pose_d, mask=keep_u8, flags=True)
        v[:, :256 + 32] = torch.where(off_d[:, None], head, v[:, :256 + 32])
        # ---- the windows that filled in this frame
        ready = ~trk & (self.n_frames == N)
        init_ok, info, init_its = np.zeros(B, dtype=np.uint8), None, None
        sel = np.nonzero(ready)[0]
        if sel.size:
            R = int(sel.size)
            bucket, ibs, packer = self._bucket(R)
            xi = up(self.x_init)
            words = v[:, :4].clone()
            mf = fe.match_front(1, 2, N - 1, xi[:, 0, :6].contiguous(), xi[:, 1:, :6], 0, self.cap)
            v[:, :4] = torch.where(up(ready)[:, None], v[:, :4], words)
            pd = up(sel[np.arange(bucket) % R])
            cm = dict(count=mf["count"][pd].contiguous(), recs=mf["recs"][pd].contiguous(), match_pose=mf["match_pose"][pd].contiguous(), cap=self.cap, F=N - 1)
            pki, Li, ok = packer.pack_init(cm, N, xi[pd, 0, :6].contiguous())
            gt = {k: self.win[k][pd].reshape(-1) for k in keys}
            gt["x"] = xi[pd].reshape(-1).contiguous()
            for k in priors:
                ibs.t[k].zero_()
            ibs.rebind(dict(gt, **pki), Li)
            ibs.solve(liw.LIW_MODE_INIT)
            ibs.marginalize()
            init_its = [(s["iterations"], s["termination"]) for s in ibs.summaries()][:R]
            okh, xs, fc = ok.cpu().numpy()[:R], gt["x"].cpu().numpy().reshape(bucket, N, 15), mf["count"].cpu().numpy()
            for r, b in enumerate(sel):
                if not okh[r]:
                    self.state[b], self.ang[b], self.n_frames[b] = g.init_state(), 0.0, 0
                    self.counters[b, 1] += 1
                    continue
                self.min_front = min(self.min_front, int(fc[b].min()))
                last = xs[r, N - 1]
                self.x_init[b], self.state[b], self.x[b, 0], self.x[b, 1] = xs[r], last, last, last
                self.kf[b], self.ang_t[b], self.tcount[b] = g.lie.make_tf(last[0:3], last[3:6]), self.ang[b], 0
                self.status[b], init_ok[b] = TRACKING, 1
                self.counters[b, 0] += 1
            good = np.nonzero(okh)[0]
            if good.size:
                for k in priors:
                    bs.t[k].view(B, -1)[up(sel[good])] = ibs.t[k].view(bucket, -1)[up(good)]
            fe.rebuild(1, N, up(self.x_init), mask=init_ok)
            fe.reset(mask=(ready & (init_ok == 0)).astype(np.uint8))
            info = (bucket, R, Li)
        self.x_d.copy_(up(self.x.reshape(-1)))
        return dict(status=self.status.copy(), drop=drop.astype(np.uint8), ready=ready.astype(np.uint8), init_ok=init_ok, skip=(skip & trk).astype(np.uint8),
                    key=self.key & keep_u8, flags=flags, pose=self.pose.copy(), Ltot=Ltot, laser_off=pk["laser_off"], its=its, init_its=init_its,
                    last_init=info, tracking=trk, keep=keep)
