"""A fleet of B robots tracked free-running on the device: `FleetTracker` chains the stages of one tracking frame of
lvio_2d::trajectory::add_sensor_data(laser) — the de-skew twist, the min_delta_t gate, the pose prediction from the wheel
increment, the roll of the two-frame window (liw_lfe_track_begin), ranges -> points -> de-skew -> lines and corners -> matches
against the reference sub-map -> the laser arrays of the batch -> solve(TRACK) -> marginalisation, the key-frame decision
(liw_lfe_track_end), the corner accumulation and add_scan — on torch's current stream.  The block count of pack_track is the only
read-back of a frame.  The key-frame deque and the INITIALIZING state machine stay with the caller: robots are initialised with
the front-end's entry points (match_front -> pack_init -> INIT solve -> rebuild) or from a known state, then handed to start().
There is no CPU fallback."""
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

    def bias(self):
        """[B, 6] view of the newest frame's ba, bw: what the next interval's pre-integration is reset with"""
        return self.x.view(self.B, 2, 15)[:, 1, 9:15]

    def step(self, ranges, stamps, interval):
        """one tracking frame of every robot.  ranges [B, n_rays] float32 (geometry: fe.set_geometry), stamps [B], interval: the six
        device tensors imu_X [B, 15], imu_J [B, 225], imu_sqrtP [B, 225], imu_Dt [B], wheel_T [B, 12], wheel_sqrtP [B, 9] of the
        interval that ends at the scan (BatchPreint makes them).  A robot whose imu_Dt is below min_delta_t is skipped: apart from its
        skip counter it is left byte for byte as it was (the caller merges that interval into the next one).
        -> dict(skip, key [B] uint8, flags [B] uint8 of ADD_* bits, pose [B, 6], Ltot, acc [B, acc_cap, 3], n_acc [B]): views of
        the tracker's buffers, valid until the next step; pose of a skipped robot is the one of its last accepted frame."""
        from . import LIW_MODE_TRACK
        torch, fe, bs, B = self.torch, self.fe, self.bs, self.B
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
        m = fe.match(REF, 0, None, tb["pose_new"], 0, self.cap, out=self._m)
        dev, Ltot = fe.pack_track(m, n=2, frame=1, out=dict(match_pose=self.match_pose, has_match=self.has_match), bufs=self._bufs)
        bs.rebind(dict(iv, x=self.x, **dev), Ltot)
        snap = [(self.x, self.x.clone())] + [(bs.t[k], bs.t[k].clone()) for k in PRIOR_KEYS]
        bs.solve(LIW_MODE_TRACK)
        bs.marginalize()
        for t, old in snap:   # the windows of skipped robots are solved with the rest and put back
            tv, ov = t.view(B, -1), old.view(B, -1)
            tv.copy_(torch.where(sk[:, None], ov, tv))
        clear = self.key & keep
        fe.track_end(self.tp, self.track, 0, self.x, m["count"], mask=keep, out=dict(key=self.key, pose=self.pose))
        fe.corners_to_world(corners, n_corners, self.pose, self.acc, self.n_acc, mask=keep, clear=clear)
        fe.add_scan(0, self.pose, mask=keep, flags=self.flags)
        self._head.copy_(torch.where(sk[:, None], head, self._head))
        self.frames += 1
        return dict(skip=tb["skip"], key=self.key & keep, flags=self.flags, pose=self.pose, Ltot=Ltot, acc=self.acc, n_acc=self.n_acc)
