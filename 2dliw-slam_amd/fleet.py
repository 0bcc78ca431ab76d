"""A fleet of B robots tracked free-running on the device: `FleetTracker` chains the stages of one tracking frame of
lvio_2d::trajectory::add_sensor_data(laser) — the de-skew twist, the min_delta_t gate, the pose prediction from the wheel
increment, the roll of the two-frame window (liw_lfe_track_begin), ranges -> points -> de-skew -> lines and corners -> matches
against the reference sub-map -> the laser arrays of the batch -> solve(TRACK) -> marginalisation, the key-frame decision
(liw_lfe_track_end), the corner accumulation and add_scan — on torch's current stream.  The block count of pack_track is the only
read-back of a frame.  `FleetTracker` tracks robots that were initialised elsewhere (the front-end's entry points match_front ->
pack_init -> INIT solve -> rebuild, or a known state) and handed to start(); `FleetTrajectory` is the whole trajectory from the first
scan on: the per-robot INITIALIZING state machine (the is_static gate, each robot's own window, the INIT solve of the robots whose
window is full, the restart of a failed window) in the same step as the tracking frame.  The key frames a step returns (key, pose, acc,
n_acc) are what loop_batch.FleetLoopDetector.push takes: the fleet's key-frame store and laser loop detector; its result and the
step's go to posegraph_batch.FleetBackEnd.push, the pose-graph back-end of the fleet (queue, edges, solve, map-frame correction).
The occupancy map per robot is map_batch.FleetMapper's: it stores scan_points() of the key frames and renders from the back-end's poses.
The intervals a step takes come from preint_batch.FleetPreint, the front door of a frame: persistent per-robot IMU / wheel accumulators
fed raw messages, with the sensor-inited latch and the merge of the intervals of skipped and dropped scans (FleetPreint.step drives
either class).  Non-laser key frames stay with the caller.  There is no CPU fallback."""
import numpy as np

from .laser_batch import REF, BatchFrontEnd, track_params_struct

INTERVAL_KEYS = ("imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP")
PRIOR_KEYS = ("prior_X", "prior_J", "prior_R", "has_prior")


def placeholder_window():
    """a two-frame window with one laser block, all zeros: what BatchSolver sizes its workspace from before the first rebind"""
    z = np.zeros
    return dict(n=2, states=z((2, 15)), laser_frame=np.ones(1, np.int32), laser_pts=z((1, 12)), match_pose=z((2, 12)), has_match=z(2, np.uint8),
                imu_X=z((1, 15)), imu_J=z((1, 225)), imu_sqrtP=z((1, 225)), imu_Dt=z(1), wheel_T=z((1, 12)), wheel_sqrtP=z((1, 9)), wheel_Dt=z(1))


class FleetTracker:
    """prm: solver parameters (synth.office_params layout); laser_prm: laser parameters; track_prm: liw_lfe_track_params as a dict
    (laser_batch.office_track_params); dims: the front-end's dims.  cap: pairs per match; max_corners: corners per scan; acc_cap:
    accumulated corners per robot between key frames.

    Owns `fe` (BatchFrontEnd), `bs` (a two-frame BatchSolver), `track` (the tracking record), `x` [B * 30] (the states of the
    windows) and the corner accumulator `acc` [B, acc_cap, 3] / `n_acc` [B].  The sub-maps of `fe` are the caller's to seed before
    start(): fe.rebuild after an INIT solve, or spawn + add_scan at a known pose."""

    def __init__(self, prm, laser_prm, track_prm, dims, device="cuda:0", cap=256, max_corners=64, acc_cap=1024):
        import torch
        from .batch import BatchSolver
        self.torch = torch
        self.fe = fe = BatchFrontEnd(laser_prm, dims, device)
        self.dev, self.B = fe.dev, fe.B
        B = self.B
        self.tp = track_params_struct(track_prm)
        self.cap, self.max_corners, self.acc_cap = int(cap), int(max_corners), int(acc_cap)
        self.bs = BatchSolver(prm, [placeholder_window()], device=device, tile=dict(B=B, states=np.zeros((B, 2, 15)), match_pose=np.zeros((B, 2, 12))))
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=self.dev)
        self.track = z(fe.track_layout(), dt=torch.uint8)
        self.x = z(B * 30)
        self.match_pose, self.has_match = z(B * 24), z(B * 2, dt=torch.uint8)
        self.acc, self.n_acc = z(B, self.acc_cap, 3), z(B, dt=torch.int32)
        self.key, self.pose, self.flags = z(B, dt=torch.uint8), z(B, 6), z(B, dt=torch.uint8)
        self._tb = dict(linear=z(B, 3), angular=z(B, 3), pose_new=z(B, 6), skip=z(B, dt=torch.uint8))
        self._pts = (z(B, fe.max_points, 3), z(B, fe.max_points), z(B, dt=torch.int32))
        self._corners = (z(B, self.max_corners, 3), z(B, dt=torch.int32))
        self._m = dict(count=z(B, dt=torch.int32), recs=z(B, self.cap, 12), idx1=z(B, self.cap, dt=torch.int32), idx2=z(B, self.cap, dt=torch.int32),
                       match_pose=z(B, 12))
        L_cap = B * self.cap
        self._bufs = dict(laser_off=z(B + 1, dt=torch.int32), laser_frame=z(L_cap, dt=torch.int32), laser_pts=z(12 * L_cap))
        # the bytes of a robot's store region that a frame writes before add_scan: its manager record and the header of scan slot 0
        robot_bytes = fe.store.numel() // B
        self._head = fe.store.view(B, robot_bytes)[:, :256 + 32]
        self.frames = 0

    def close(self):
        self.bs.close()
        self.fe.close()

    def start(self, x0, angular_local=None, prior=None):
        """begin tracking from the known states x0 [B, 15] (p q v ba bw): both rows of every window, last_keyframe_tf and the
        counters (liw_lfe_track_init); angular_local [B, 3] is the body rate of the last interval (zero when None); prior: dict of
        prior_X [B, 15], prior_J [B, 225], prior_R [B, 15], has_prior [B] as a marginalisation left them (none when None).  The
        corner accumulator starts empty."""
        torch, fe, B = self.torch, self.fe, self.B
        x0 = fe._t(x0, torch.float64, (B, 15))
        xv = self.x.view(B, 2, 15)
        xv[:, 0], xv[:, 1] = x0, x0
        fe.track_init(self.tp, self.track, xv[:, 1], angular_local)
        for k in PRIOR_KEYS:
            t = self.bs.t[k]
            if prior is None:
                t.zero_()
            else:
                t.copy_(fe._t(prior[k], t.dtype).reshape(-1))
        self.match_pose.zero_()
        self.has_match.zero_()
        self.n_acc.zero_()
        self.key.zero_()
        self.frames = 0

    def scan_points(self):
        """(pts [B, max_points, 3], n [B] int32): views of the de-skewed laser-frame points of the last step's scans, valid until the
        next step: what map_batch.FleetMapper.add_keyframes stores for the robots whose key frame was kept"""
        return self._pts[0], self._pts[2]

    def bias(self):
        """[B, 6] view of the newest frame's ba, bw: what the next interval's pre-integration is reset with"""
        return self.x.view(self.B, 2, 15)[:, 1, 9:15]

    def _tracking_stages(self, iv, pose_new, corners, n_corners, head, off, keep, tracking=None):
        """the stages of a tracking frame after spawn, shared with FleetTrajectory: match against the reference sub-map -> pack_track
        -> solve(TRACK) -> marginalize -> track_end -> corners_to_world -> add_scan.  All B windows are solved; the rows and the
        head bytes of the robots with off[b] (bool: skipped, or not tracking) are put back from the snapshot / from `head`; keep
        [B] uint8 masks the stages after the solve.  tracking: bool [B], the counts of the other robots are zeroed before the pack
        (None: every robot tracks).  -> Ltot"""
        from . import LIW_MODE_TRACK
        torch, fe, bs, B = self.torch, self.fe, self.bs, self.B
        m = fe.match(REF, 0, None, pose_new, 0, self.cap, out=self._m)
        if tracking is not None:
            m["count"].copy_(torch.where(tracking, m["count"], torch.zeros_like(m["count"])))
        dev, Ltot = fe.pack_track(m, n=2, frame=1, out=dict(match_pose=self.match_pose, has_match=self.has_match), bufs=self._bufs)
        bs.rebind(dict(iv, x=self.x, **dev), Ltot)
        snap = [(self.x, self.x.clone())] + [(bs.t[k], bs.t[k].clone()) for k in PRIOR_KEYS]
        bs.solve(LIW_MODE_TRACK)
        bs.marginalize()
        for t, old in snap:   # the windows of skipped robots are solved with the rest and put back
            tv, ov = t.view(B, -1), old.view(B, -1)
            tv.copy_(torch.where(off[:, None], ov, tv))
        clear = self.key & keep
        fe.track_end(self.tp, self.track, 0, self.x, m["count"], mask=keep, out=dict(key=self.key, pose=self.pose))
        fe.corners_to_world(corners, n_corners, self.pose, self.acc, self.n_acc, mask=keep, clear=clear)
        fe.add_scan(0, self.pose, mask=keep, flags=self.flags)
        self._head.copy_(torch.where(off[:, None], head, self._head))
        return Ltot

    def step(self, ranges, stamps, interval):
        """one tracking frame of every robot.  ranges [B, n_rays] float32 (geometry: fe.set_geometry), stamps [B], interval: the six
        device tensors imu_X [B, 15], imu_J [B, 225], imu_sqrtP [B, 225], imu_Dt [B], wheel_T [B, 12], wheel_sqrtP [B, 9] of the
        interval that ends at the scan (FleetPreint.push makes them from the messages; BatchPreint from the closed intervals of a log).  A
        robot whose imu_Dt is below min_delta_t is skipped: apart from its skip counter it is left byte for byte as it was (its interval
        merges into the next one: FleetPreint.step does not commit it; a caller with intervals of its own has to merge them).
        -> dict(skip, key [B] uint8, flags [B] uint8 of ADD_* bits, pose [B, 6], Ltot, acc [B, acc_cap, 3], n_acc [B]): views of
        the tracker's buffers, valid until the next step; pose of a skipped robot is the one of its last accepted frame."""
        torch, fe, B = self.torch, self.fe, self.B
        st = fe._t(stamps, torch.float64, (B,))
        iv = {k: fe._t(interval[k], torch.float64) for k in INTERVAL_KEYS}
        head = self._head.clone()
        tb = fe.track_begin(self.tp, self.track, self.x, iv["imu_X"], iv["imu_Dt"], iv["wheel_T"], st, out=self._tb)
        sk = tb["skip"].bool()
        keep = tb["skip"] ^ 1
        pts, times, n = fe.ranges_to_points(ranges, st, out=self._pts)
        fe.deskew(pts, times, n, st, tb["linear"], tb["angular"])
        # a skipped robot's scan is not spawned: n_pts = -1 makes the call write nothing of it but the slot header, put back below
        n_sp = torch.where(sk, torch.full_like(n, -1), n)
        t_scan = torch.where(n > 0, times[:, 0], st)   # laser_data.times.front(), the stamp for an empty scan
        corners, n_corners = fe.spawn(0, pts, n_sp, times=t_scan, corners=self.max_corners, out=self._corners)
        Ltot = self._tracking_stages(iv, tb["pose_new"], corners, n_corners, head, sk, keep)
        self.frames += 1
        return dict(skip=tb["skip"], key=self.key & keep, flags=self.flags, pose=self.pose, Ltot=Ltot, acc=self.acc, n_acc=self.n_acc)


def placeholder_init_window(n):
    """placeholder_window for an n-frame INIT batch"""
    z = np.zeros
    return dict(n=n, states=z((n, 15)), laser_frame=np.ones(1, np.int32), laser_pts=z((1, 12)), match_pose=z((n, 12)), has_match=z(n, np.uint8),
                imu_X=z((n - 1, 15)), imu_J=z((n - 1, 225)), imu_sqrtP=z((n - 1, 225)), imu_Dt=z(n - 1), wheel_T=z((n - 1, 12)),
                wheel_sqrtP=z((n - 1, 9)), wheel_Dt=z(n - 1))


class FleetTrajectory(FleetTracker):
    """B instances of lvio_2d::trajectory (laser + IMU + odometry, keep_window_size = 1) from the first scan on: every robot starts
    INITIALIZING (reset()), fills its own window of init_prm["slide_window_size"] = N frames behind the is_static gate, is initialised
    by an INIT solve and tracks from the next frame, and robots in different states share one step().  init_prm: liw_lfe_init_params
    as a dict (laser_batch.office_init_params); dims["slots"] must be at least N + 1: slot 0 is where every scan is spawned, slots
    1 .. N hold the window (frame k in slot 1 + k).  init_iters: iteration cap of the INIT solve (0: the solver's).

    On top of FleetTracker's state it owns the initialisation record `init`, the window arrays `win` (x_init [B, N, 15] and the six
    interval arrays [B, N - 1, w]) and one INIT BatchSolver per bucket of ready robots (powers of two, capped at B, made on first
    use): rows R .. bucket-1 of a bucket repeat ready windows (sel[r mod R]) and their results are discarded, so the INIT solver never
    sees a window of made-up or partly filled data and its cost follows the ready robots.  liw_lfe_match_front has no robot list: it
    runs over the whole fleet in a frame with a ready robot, and the robot words it may set in robots that are not ready are put back.

    Device memory besides FleetTracker's (store, match and pack buffers): the match_front outputs for the whole fleet, B (N - 1) cap
    records of 104 bytes, held for the driver's life (3.9 GB at 49 152 robots, N = 4, cap 256), the window arrays (3.9 KB per robot
    and interval), and per bucket that was ever used an INIT solver plus its laser arrays of bucket (N - 1) cap blocks of 100 bytes
    (1.26 GB at a bucket of 16 384), kept for reuse.

    The tracking batch is solved for all B robots every frame.  The rows of a robot that is not TRACKING hold, while the batch is
    solved: x as reset() or its last frame left it (zeros until the robot is committed), the robot's interval of this frame, no laser
    block, has_match 1 with the pose record of an empty match, and its prior rows (none).  They are put back from a snapshot after
    the marginalisation, as the rows of a skipped robot are.

    The key frames and their loop edges are loop_batch.FleetLoopDetector's, the pose-graph solve around them
    posegraph_batch.FleetBackEnd's, the occupancy map per robot map_batch.FleetMapper's.  The imu_inited / wheel_odom_inited latch is preint_batch.FleetPreint's: its step() hands a robot whose
    latch is off the identity increment, which the gates here drop.  Out of scope: non-laser key frames, keep_window_size > 1, a C++
    mirror of this driver."""

    def __init__(self, prm, laser_prm, track_prm, init_prm, dims, device="cuda:0", cap=256, max_corners=64, acc_cap=1024, init_iters=0):
        super().__init__(prm, laser_prm, track_prm, dims, device=device, cap=cap, max_corners=max_corners, acc_cap=acc_cap)
        from .laser_batch import init_params_struct
        torch, fe, B = self.torch, self.fe, self.B
        self.prm, self.device = prm, device
        self.ip = init_params_struct(init_prm)
        self.N = N = int(self.ip.slide_window_size)
        assert 2 <= N <= fe.slots - 1, "dims['slots'] must be at least slide_window_size + 1"
        self.init_iters = int(init_iters)
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=self.dev)
        self.init = z(fe.init_layout(), dt=torch.uint8)
        self.win = fe.init_window(N)
        self._ib = dict(drop=z(B, dt=torch.uint8), slot_of=z(B, dt=torch.int32))
        self._sel = dict(ready=z(B, dt=torch.uint8), sel=z(B, dt=torch.int32), n_sel=z(1, dt=torch.int32))
        self._R = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._status = self.init.view(torch.int32).view(B, 64)[:, 36]   # the records' status words
        self._word = fe.store.view(B, fe.store.numel() // B)[:, :4]     # the robot words of the store
        self.init_ok = z(B, dt=torch.uint8)
        self._front = dict(count=z(B, N - 1, dt=torch.int32), recs=z(B, N - 1, self.cap, 12), match_pose=z(B, N - 1, 12),
                           idx1=z(B, N - 1, self.cap, dt=torch.int32), idx2=z(B, N - 1, self.cap, dt=torch.int32))
        self._init_bs, self._init_buf = {}, {}
        self.last_init = None   # (bucket, R, Ltot) of the last frame that ran an INIT solve
        self.reset()

    def close(self):
        for bs in self._init_bs.values():
            bs.close()
        self._init_bs, self._init_buf = {}, {}
        super().close()

    def reset(self):
        """every robot INITIALIZING with an empty window (init_current_status), an empty store, no prior, zero states"""
        fe = self.fe
        fe.reset()
        fe.init_reset(self.tp, self.init)
        for t in [self.track, self.x, self.match_pose, self.has_match, self.acc, self.n_acc, self.key, self.pose, self.flags, self.init_ok,
                  *self.win.values(), *self._tb.values(), *[self.bs.t[k] for k in PRIOR_KEYS]]:
            t.zero_()
        self.frames = 0

    def status(self):
        """[B] int32 view of the records' status words (laser_batch.INITIALIZING / TRACKING)"""
        return self._status

    def _bucket(self, R):
        from .batch import BatchSolver
        b = 1
        while b < R:
            b *= 2
        b = min(b, self.B)
        if b not in self._init_bs:
            torch, N = self.torch, self.N
            self._init_bs[b] = BatchSolver(self.prm, [placeholder_init_window(N)], device=self.device,
                                           tile=dict(B=b, states=np.zeros((b, N, 15)), match_pose=np.zeros((b, N, 12))))
            e = lambda n, dt: torch.empty(n, dtype=dt, device=self.dev)
            L_cap = b * (N - 1) * self.cap   # every pair of every frame: 100 bytes a block
            self._init_buf[b] = (dict(laser_off=e(b + 1, torch.int32), laser_frame=e(L_cap, torch.int32), laser_pts=e(12 * L_cap, torch.float64)),
                                 dict(match_pose=e(b * N * 12, torch.float64), has_match=e(b * N, torch.uint8), init_ok=e(b, torch.uint8)))
        return b, self._init_bs[b], self._init_buf[b]

    def step(self, ranges, stamps, interval):
        """one frame of every robot, whatever its state; arguments as FleetTracker.step.  An INITIALIZING robot whose wheel increment
        is below both motion thresholds is dropped: apart from its counter it is left byte for byte as it was (its interval merges into
        the next one, as FleetPreint.step does by not committing it), as a TRACKING robot below min_delta_t is skipped.  A robot committed in this frame tracks from
        the next one.
        -> FleetTracker.step's dict (skip, key, flags 0 for robots that are not TRACKING) plus status [B] int32 after the frame,
        drop [B] uint8, ready [B] uint8 (the window was full and went into the INIT solve), init_ok [B] uint8 (it was committed)."""
        from . import LIW_MODE_INIT
        torch, fe, bs, B, N = self.torch, self.fe, self.bs, self.B, self.N
        st = fe._t(stamps, torch.float64, (B,))
        iv = {k: fe._t(interval[k], torch.float64) for k in INTERVAL_KEYS}
        head = self._head.clone()
        trk = self._status == 1                      # the states of this frame: a commit below shows from the next frame on
        trk_u8 = trk.to(torch.uint8)
        self._ib["drop"].zero_()
        self._ib["slot_of"].zero_()
        ib = fe.init_begin(self.tp, self.ip, self.init, iv, self.win, out=self._ib)
        sel = fe.init_select(self.ip, self.init, out=self._sel, R_host=self._R)   # R arrives with pack_track's read-back
        tb = fe.track_begin(self.tp, self.track, self.x, iv["imu_X"], iv["imu_Dt"], iv["wheel_T"], st, mask=trk_u8, out=self._tb)
        keep_b = trk & (tb["skip"] == 0)
        off = ~keep_b                                # not TRACKING, or skipped: solved with the rest and put back
        keep = keep_b.to(torch.uint8)
        taken = ~trk & (ib["drop"] == 0)             # INITIALIZING robots whose frame goes into their window
        pts, times, n = fe.ranges_to_points(ranges, st, out=self._pts)
        fe.deskew(pts, times, torch.where(trk, n, torch.zeros_like(n)), st, tb["linear"], tb["angular"])   # no de-skew while INITIALIZING
        n_sp = torch.where(keep_b | taken, n, torch.full_like(n, -1))
        t_scan = torch.where(n > 0, times[:, 0], st)
        corners, n_corners = fe.spawn(0, pts, n_sp, times=t_scan, corners=self.max_corners, out=self._corners)
        fe.slot_copy(ib["slot_of"], mask=taken.to(torch.uint8))
        Ltot = self._tracking_stages(iv, tb["pose_new"], corners, n_corners, head, off, keep, tracking=trk)
        R = int(self._R[0])                          # valid since the read-back of Ltot
        # ---- the windows that filled in this frame
        self.init_ok.zero_()
        if R > 0:
            x_init = self.win["x_init"]
            words = self._word.clone()
            mf = fe.match_front(1, 2, N - 1, x_init[:, 0, :6].contiguous(), x_init[:, 1:, :6], 0, self.cap, out=self._front)
            self._word.copy_(torch.where(sel["ready"].bool()[:, None], self._word, words))
            bucket, ibs, (bufs, outs) = self._bucket(R)
            rsel = sel["sel"][:R]
            psel = rsel[torch.arange(bucket, device=self.dev) % R].contiguous()   # rows R .. bucket-1 repeat ready windows
            pk, Li, ok = fe.pack_init_sel(bucket, psel, mf, N, x_init[:, 0], out=outs, bufs=bufs)
            g = {k: self.win[k].index_select(0, psel.long()).reshape(-1) for k in INTERVAL_KEYS}
            g["x"] = x_init.index_select(0, psel.long()).reshape(-1)
            for k in PRIOR_KEYS:
                ibs.t[k].zero_()
            ibs.rebind(dict(g, **pk), Li)
            ibs.solve(LIW_MODE_INIT, self.init_iters)
            ibs.marginalize()
            fe.init_commit(self.tp, self.ip, self.init, self.track, R, rsel, ok, g["x"], x_init, self.x)
            okb = ok[:R].bool()
            for k in PRIOR_KEYS:   # the prior the marginalisation left, into the committed robots' rows of the tracking batch
                dst, src = bs.t[k].view(B, -1), ibs.t[k].view(bucket, -1)[:R]
                dst.index_copy_(0, rsel.long(), torch.where(okb[:, None], src, dst.index_select(0, rsel.long())))
            self.init_ok.index_copy_(0, rsel.long(), ok[:R])
            fe.rebuild(1, N, x_init, mask=self.init_ok)
            fe.reset(mask=sel["ready"] & (self.init_ok ^ 1))
            self.last_init = (bucket, R, Li)
        self.frames += 1
        return dict(skip=tb["skip"] & trk_u8, key=self.key & keep, flags=self.flags, pose=self.pose, Ltot=Ltot, acc=self.acc, n_acc=self.n_acc,
                    status=self._status, drop=ib["drop"], ready=sel["ready"], init_ok=self.init_ok)
