"""Batched laser front-end on the device (C ABI include/liw_laser_batch.h): `BatchFrontEnd` runs the tracking-time work of
`laser.LaserManager` for B robots at once on torch device tensors — ranges -> points -> de-skew -> lines -> matches against
the reference sub-map -> sub-map update -> the laser arrays `BatchSolver.rebind` takes — and a fleet's initialisation: the
matches of a whole INIT window against the front key frame (`match_front`), its laser arrays (`pack_init`) and the sub-map
rebuild at the solved poses (`rebuild`).  The host front-end (`laser`) is its parity reference.  There is no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from .laser import LaserParamsC, laser_params_struct

# every symbol include/liw_laser_batch.h declares (checked by tests/test_laser_batch_abi.py)
LFE_EXPORTS = [
    "liw_lfe_store_layout", "liw_lfe_create", "liw_lfe_destroy", "liw_lfe_last_error", "liw_lfe_set_geometry", "liw_lfe_store_reset",
    "liw_lfe_ranges_to_points", "liw_lfe_deskew", "liw_lfe_spawn", "liw_lfe_match", "liw_lfe_add_scan", "liw_lfe_pack_track",
    "liw_lfe_status", "liw_lfe_num_lines", "liw_lfe_get_lines", "liw_lfe_cell_lines", "liw_lfe_submap_pose",
    "liw_lfe_spawn_corners", "liw_lfe_corners_to_world", "liw_lfe_match_front", "liw_lfe_pack_init", "liw_lfe_rebuild",
    "liw_lfe_add_scan_flags", "liw_lfe_add_scan_path",
    "liw_lfe_track_layout", "liw_lfe_track_init", "liw_lfe_track_begin", "liw_lfe_track_end", "liw_lfe_track_get",
    "liw_lfe_crmath_eval",
    "liw_lfe_init_layout", "liw_lfe_init_reset", "liw_lfe_init_get", "liw_lfe_init_begin", "liw_lfe_slot_copy", "liw_lfe_init_select",
    "liw_lfe_pack_init_sel", "liw_lfe_init_commit",
]

ST_POINTS, ST_LINES, ST_CELLS, ST_MATCH, ST_INVALID, ST_CORNERS = 1, 2, 4, 8, 16, 32
ADD_ADDED, ADD_FIRST, ADD_SPAWNED, ADD_SWAPPED = 1, 2, 4, 8   # LIW_LFE_ADD_*: what an add_scan did for a robot
REF, SPAWNING, ROBOT = -1, -2, -3
INITIALIZING, TRACKING = 0, 1   # LIW_LFE_INITIALIZING / LIW_LFE_TRACKING: the status of an initialisation record
NONE = -61   # LIW_LFE_NONE: a getter's "no such sub-map / outside the grid" (the Python getters turn it into -1 / None)


class DimsC(C.Structure):
    _fields_ = [("B", C.c_int), ("slots", C.c_int), ("max_points", C.c_int), ("max_lines", C.c_int), ("max_cell_entries", C.c_int)]


class TrackParamsC(C.Structure):
    _fields_ = [("T_imu_to_wheel", C.c_double * 16), ("normalize_extrinsics", C.c_int), ("min_delta_t", C.c_double),
                ("key_frame_p_motion_threshold", C.c_double), ("key_frame_q_motion_threshold", C.c_double)]


def office_track_params(prm=None):
    """liw_lfe_track_params with the trajectory values of reference config/office.yaml and the extrinsic of prm (synth.office_params)"""
    from .synth import office_params
    prm = prm or office_params()
    return dict(T_imu_to_wheel=list(prm["T_imu_to_wheel"]), normalize_extrinsics=bool(prm.get("normalize_extrinsics", True)), min_delta_t=0.001,
                key_frame_p_motion_threshold=0.05, key_frame_q_motion_threshold=0.05)


def track_params_struct(tp):
    if isinstance(tp, TrackParamsC):
        return tp
    s = TrackParamsC()
    s.T_imu_to_wheel = (C.c_double * 16)(*[float(v) for v in np.asarray(tp["T_imu_to_wheel"], dtype=np.float64).reshape(16)])
    s.normalize_extrinsics = int(bool(tp["normalize_extrinsics"]))
    for k in ("min_delta_t", "key_frame_p_motion_threshold", "key_frame_q_motion_threshold"):
        setattr(s, k, float(tp[k]))
    return s


class InitParamsC(C.Structure):
    _fields_ = [("slide_window_size", C.c_int), ("p_motion_threshold", C.c_double), ("q_motion_threshold", C.c_double)]


def office_init_params():
    """liw_lfe_init_params with the trajectory values of reference config/office.yaml"""
    return dict(slide_window_size=10, p_motion_threshold=0.1, q_motion_threshold=0.1)


def init_params_struct(ip):
    if isinstance(ip, InitParamsC):
        return ip
    s = InitParamsC()
    s.slide_window_size = int(ip["slide_window_size"])
    s.p_motion_threshold, s.q_motion_threshold = float(ip["p_motion_threshold"]), float(ip["q_motion_threshold"])
    return s


def dims_struct(dims):
    if isinstance(dims, DimsC):
        return dims
    s = DimsC()
    for k, _ in DimsC._fields_:
        setattr(s, k, int(dims[k]))
    return s


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_lfe_ready", False):
        vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.liw_lfe_store_layout.argtypes = [C.POINTER(DimsC), C.POINTER(C.c_size_t)]
        L.liw_lfe_create.restype = vp
        L.liw_lfe_create.argtypes = [C.POINTER(LaserParamsC), C.POINTER(DimsC), C.c_int]
        L.liw_lfe_destroy.argtypes = [vp]
        L.liw_lfe_last_error.restype = C.c_char_p
        L.liw_lfe_last_error.argtypes = [vp]
        L.liw_lfe_set_geometry.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
        L.liw_lfe_store_reset.argtypes = [vp, vp, vp, vp]
        L.liw_lfe_ranges_to_points.argtypes = [vp] * 8
        L.liw_lfe_deskew.argtypes = [vp] * 8
        L.liw_lfe_spawn.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
        L.liw_lfe_spawn_corners.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
        L.liw_lfe_corners_to_world.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
        L.liw_lfe_match.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_add_scan.argtypes = [vp, vp, C.c_int, vp, vp, vp]
        L.liw_lfe_add_scan_flags.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
        L.liw_lfe_add_scan_path.argtypes = [vp]
        L.liw_lfe_pack_track.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        ll = C.c_longlong
        L.liw_lfe_match_front.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, ll, ll, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_pack_init.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_rebuild.argtypes = [vp, vp, C.c_int, C.c_int, vp, ll, ll, vp, vp]
        L.liw_lfe_track_layout.argtypes = [C.POINTER(DimsC), C.POINTER(C.c_size_t)]
        tpp = C.POINTER(TrackParamsC)
        L.liw_lfe_track_init.argtypes = [vp, tpp, vp, vp, ll, vp, vp, vp]
        L.liw_lfe_track_begin.argtypes = [vp, tpp] + [vp] * 12
        L.liw_lfe_track_end.argtypes = [vp, tpp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_track_get.argtypes = [vp, vp, C.c_int, dp, dp, dp, ip]
        L.liw_lfe_crmath_eval.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
        ipp = C.POINTER(InitParamsC)
        L.liw_lfe_init_layout.argtypes = [C.POINTER(DimsC), C.POINTER(C.c_size_t)]
        L.liw_lfe_init_reset.argtypes = [vp, tpp, vp, vp, vp]
        L.liw_lfe_init_get.argtypes = [vp, vp, C.c_int, ip, ip, dp, dp, ip]
        L.liw_lfe_init_begin.argtypes = [vp, tpp, ipp] + [vp] * 18
        L.liw_lfe_slot_copy.argtypes = [vp, vp, vp, vp, vp]
        L.liw_lfe_init_select.argtypes = [vp, ipp, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_pack_init_sel.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, ll, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_init_commit.argtypes = [vp, tpp, ipp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.liw_lfe_status.argtypes = [vp, vp, C.c_int, C.c_int]
        L.liw_lfe_num_lines.argtypes = [vp, vp, C.c_int, C.c_int]
        L.liw_lfe_get_lines.argtypes = [vp, vp, C.c_int, C.c_int, dp, C.c_int]
        L.liw_lfe_cell_lines.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, ip, C.c_int]
        L.liw_lfe_submap_pose.argtypes = [vp, vp, C.c_int, C.c_int, dp, dp]
        L._lfe_ready = True
    return L


def _layout_bytes(fn, dims):
    """what the C layout function `fn` answers for dims (host-only; LiwError(LIW_EINVAL) for a non-positive dimension)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = getattr(_lib(), fn)(C.byref(dims_struct(dims)), C.byref(n))
    if r < 0:
        raise LiwError(r, fn)
    return int(n.value)


def store_bytes(dims):
    """bytes of the store for dims (host-only; LiwError(LIW_EINVAL) for a non-positive dimension)"""
    return _layout_bytes("liw_lfe_store_layout", dims)


def track_bytes(dims):
    """bytes of the tracking record for dims, 256 per robot (host-only; LiwError(LIW_EINVAL) for a non-positive dimension)"""
    return _layout_bytes("liw_lfe_track_layout", dims)


def init_bytes(dims):
    """bytes of the initialisation record for dims, 256 per robot (host-only; LiwError(LIW_EINVAL) for a non-positive dimension)"""
    return _layout_bytes("liw_lfe_init_layout", dims)


WINDOW_KEYS = (("imu_X", 15), ("imu_J", 225), ("imu_sqrtP", 225), ("imu_Dt", 1), ("wheel_T", 12), ("wheel_sqrtP", 9))


def pad_points(point_lists, max_points):
    """variable-length host point lists ([m_b, 3]) -> (pts [B, max_points, 3], n_pts [B]) in the device layout"""
    B = len(point_lists)
    pts = np.zeros((B, max_points, 3))
    n = np.zeros(B, dtype=np.int32)
    for b, p in enumerate(point_lists):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        m = min(p.shape[0], max_points)
        pts[b, :m] = p[:m]
        n[b] = p.shape[0]
    return pts, n


def pad_times(time_lists, max_points):
    B = len(time_lists)
    out = np.zeros((B, max_points))
    for b, t in enumerate(time_lists):
        t = np.asarray(t, dtype=np.float64).reshape(-1)[:max_points]
        out[b, :t.size] = t
    return out


class BatchFrontEnd:
    """laser_manager's tracking-time front-end for B robots, resident on one GPU.

    prm_laser: laser parameters (laser.office_laser_params layout); dims: dict(B, slots, max_points, max_lines, max_cell_entries).
    The store is a torch uint8 tensor; every method takes / returns torch tensors on `device` and launches on torch's current
    stream.  Slots are 0 .. slots-1; REF names the manager's reference sub-map."""

    def __init__(self, prm_laser, dims, device="cuda:0"):
        import torch
        from . import LiwError
        self.torch, self.LiwError = torch, LiwError
        self.L = _lib()
        self.dev = torch.device(device)
        self.dims = dims_struct(dims)
        self.B, self.slots, self.max_points = self.dims.B, self.dims.slots, self.dims.max_points
        self._ps = laser_params_struct(prm_laser)
        nbytes = store_bytes(self.dims)
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_lfe_create(C.byref(self._ps), C.byref(self.dims), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_lfe_create")
        self.store = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        self.n_rays = None
        self.reset()

    def close(self):
        if getattr(self, "h", None):
            self.L.liw_lfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r < 0:
            raise self.LiwError(r, self.L.liw_lfe_last_error(self.h).decode())
        return r

    def _s(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _t(self, a, dtype, shape=None):
        t = self.torch.as_tensor(a, dtype=dtype, device=self.dev)
        t = t.contiguous()
        if shape is not None:
            t = t.view(*shape)
        return t

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _mask(self, mask):
        return None if mask is None else self._t(mask, self.torch.uint8, (self.B,))

    # -------------------------------------------------------------------------------------------------------- compute
    def set_geometry(self, n_rays, angle_min, angle_increment, time_increment):
        self._chk(self.L.liw_lfe_set_geometry(self.h, int(n_rays), float(angle_min), float(angle_increment), float(time_increment)))
        self.n_rays = int(n_rays)

    def reset(self, mask=None):
        """laser_manager::clear_all_scan for the masked robots (all when mask is None)"""
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_store_reset(self.h, self._p(self.store), self._p(m), self._s()))

    def ranges_to_points(self, ranges, stamps, angle_min=None, angle_increment=None, time_increment=None, out=None):
        """ranges [B, n_rays] float32, stamps [B] -> (pts [B, max_points, 3], times [B, max_points], n_pts [B] int32); `out` may be
        such a tuple to write into (entries past n_pts are left as they are)"""
        torch = self.torch
        r = self._t(ranges, torch.float32)
        if angle_min is not None:
            self.set_geometry(r.shape[-1], angle_min, angle_increment, time_increment)
        assert self.n_rays is not None and r.numel() == self.B * self.n_rays, "ranges must be [B, n_rays] of the geometry"
        st = self._t(stamps, torch.float64, (self.B,))
        if out is None:
            pts = torch.zeros(self.B, self.max_points, 3, dtype=torch.float64, device=self.dev)
            times = torch.zeros(self.B, self.max_points, dtype=torch.float64, device=self.dev)
            n = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        else:
            pts, times, n = out
            assert pts.is_contiguous() and times.is_contiguous() and n.is_contiguous()
            assert pts.dtype == times.dtype == torch.float64 and n.dtype == torch.int32
            assert pts.numel() >= self.B * self.max_points * 3 and times.numel() >= self.B * self.max_points and n.numel() >= self.B
        self._chk(self.L.liw_lfe_ranges_to_points(self.h, self._p(self.store), self._p(r), self._p(st), self._p(pts), self._p(times), self._p(n), self._s()))
        return pts, times, n

    def deskew(self, pts, times, n_pts, stamps, linear, angular):
        """in place on pts [B, max_points, 3]; linear / angular [B, 3]"""
        torch = self.torch
        assert pts.is_contiguous() and pts.dtype == torch.float64 and pts.numel() == self.B * self.max_points * 3
        tm, n = self._t(times, torch.float64), self._t(n_pts, torch.int32)
        st, li, an = self._t(stamps, torch.float64, (self.B,)), self._t(linear, torch.float64, (self.B, 3)), self._t(angular, torch.float64, (self.B, 3))
        self._chk(self.L.liw_lfe_deskew(self.h, self._p(pts), self._p(tm), self._p(n), self._p(st), self._p(li), self._p(an), self._s()))
        return pts

    def spawn(self, slot, pts, n_pts, times=None, corners=None, out=None):
        """laser_manager::spawn_scan into `slot`: pts [B, max_points, 3], n_pts [B], times [B] (scan time) or None.
        corners=max_corners also computes scan::concers and returns (corners [B, max_corners, 3] in the laser frame, n_corners [B]
        int32; max_corners + 1 marks an overflow); `out` may be such a pair to write into.  The environment's LIW_LFE_SPAWN=lane
        selects the lane-per-scan kernel (no corners) for the call."""
        torch = self.torch
        p = self._t(pts, torch.float64, (self.B, self.max_points, 3))
        n = self._t(n_pts, torch.int32, (self.B,))
        t = None if times is None else self._t(times, torch.float64, (self.B,))
        if corners is None:
            self._chk(self.L.liw_lfe_spawn(self.h, self._p(self.store), int(slot), self._p(p), self._p(n), self._p(t), self._s()))
            return None
        mc = int(corners)
        if out is None:
            cz = torch.zeros(self.B, max(mc, 1), 3, dtype=torch.float64, device=self.dev)
            cn = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        else:
            cz, cn = out
            assert cz.is_contiguous() and cn.is_contiguous() and cz.dtype == torch.float64 and cn.dtype == torch.int32
            assert cz.numel() >= self.B * mc * 3 and cn.numel() >= self.B
        self._chk(self.L.liw_lfe_spawn_corners(self.h, self._p(self.store), int(slot), self._p(p), self._p(n), self._p(t), mc, self._p(cz), self._p(cn),
                                               self._s()))
        return cz, cn

    def corners_to_world(self, corners, n_corners, pose, acc, n_acc, mask=None, clear=None):
        """lvio_2d::trajectory's corner accumulation: robots with clear[b] restart from n_acc[b] = 0, then the masked robots (all
        when None) append make_tf(pose[b]) * T_imu_to_laser * corners[b, :n_corners[b]] to acc [B, acc_cap, 3] at n_acc [B] int32,
        both updated in place.  An append that does not fit leaves n_acc[b] = acc_cap + 1 and sets ST_CORNERS."""
        torch = self.torch
        assert corners.is_contiguous() and corners.dtype == torch.float64 and corners.dim() == 3 and corners.shape[0] == self.B
        assert acc.is_contiguous() and acc.dtype == torch.float64 and acc.dim() == 3 and acc.shape[0] == self.B and acc.shape[2] == 3
        assert n_acc.is_contiguous() and n_acc.dtype == torch.int32 and n_acc.numel() >= self.B
        nc = self._t(n_corners, torch.int32, (self.B,))
        p = self._t(pose, torch.float64, (self.B, 6))
        m, c = self._mask(mask), self._mask(clear)
        self._chk(self.L.liw_lfe_corners_to_world(self.h, self._p(self.store), int(corners.shape[1]), self._p(corners), self._p(nc), self._p(p),
                                                  self._p(m), self._p(c), int(acc.shape[1]), self._p(acc), self._p(n_acc), self._s()))
        return acc, n_acc

    def match(self, slot1, slot2, pose1, pose2, kk=0, cap=256, out=None):
        """laser_manager::do_match per robot -> dict(count [B], recs [B, cap, 12], idx1 / idx2 [B, cap], match_pose [B, 12]);
        `out` may supply any of those (contiguous device tensors of at least that size)"""
        torch = self.torch
        p1 = None if pose1 is None else self._t(pose1, torch.float64, (self.B, 6))
        p2 = self._t(pose2, torch.float64, (self.B, 6))
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=self.dev)
        o = dict(count=z(self.B, dt=torch.int32), recs=z(self.B, cap, 12), idx1=z(self.B, cap, dt=torch.int32), idx2=z(self.B, cap, dt=torch.int32),
                 match_pose=z(self.B, 12)) if out is None else dict(out)
        for k, shape, dt in (("count", (self.B,), torch.int32), ("recs", (self.B, cap, 12), torch.float64), ("idx1", (self.B, cap), torch.int32),
                             ("idx2", (self.B, cap), torch.int32), ("match_pose", (self.B, 12), torch.float64)):
            if k not in o:
                o[k] = z(*shape, dt=dt)
            assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() >= int(np.prod(shape)), k
        o["cap"] = int(cap)
        self._chk(self.L.liw_lfe_match(self.h, self._p(self.store), int(slot1), int(slot2), self._p(p1), self._p(p2), int(kk), int(cap),
                                       self._p(o["count"]), self._p(o["recs"]), self._p(o["idx1"]), self._p(o["idx2"]), self._p(o["match_pose"]), self._s()))
        return o

    def match_with_ref(self, slot, pose, cap=256):
        """laser_manager::match_with_ref of scan `slot` at pose [B, 6]"""
        return self.match(REF, slot, None, pose, 0, cap)

    def add_scan(self, slot, pose, mask=None, flags=False):
        """laser_manager::add_scan of scan `slot` at pose [B, 6] (the key-frame deque stays with the caller).  flags=True returns
        what the call did per robot, a [B] uint8 tensor of ADD_* bits (0: masked out or dropped by the motion filter); flags may
        also be such a tensor to write into.  The environment's LIW_LFE_ADD_SCAN=lane selects the lane-per-robot kernel for the
        call (add_scan_path() tells which one ran)."""
        torch = self.torch
        p = self._t(pose, torch.float64, (self.B, 6))
        m = self._mask(mask)
        if flags is False or flags is None:
            self._chk(self.L.liw_lfe_add_scan(self.h, self._p(self.store), int(slot), self._p(p), self._p(m), self._s()))
            return None
        if flags is True:
            flags = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        assert torch.is_tensor(flags) and flags.dtype == torch.uint8 and flags.is_contiguous() and flags.device == self.dev and flags.numel() >= self.B
        self._chk(self.L.liw_lfe_add_scan_flags(self.h, self._p(self.store), int(slot), self._p(p), self._p(m), self._p(flags), self._s()))
        return flags

    def add_scan_path(self):
        """the kernel the last add_scan / rebuild launched: 0 lane-per-robot, 1 wave-per-robot (LiwError before any)"""
        return self._chk(self.L.liw_lfe_add_scan_path(self.h))

    def pack_track(self, m, n=2, frame=1, out=None, L_cap=None, bufs=None):
        """the laser arrays of B n-frame windows whose laser frame is `frame`, from a match() result.  out: dict with `match_pose`
        [B * n * 12] and `has_match` [B * n] to write the frame's rows into (fresh zero tensors when None); bufs: laser_off [B + 1],
        laser_frame [L_cap], laser_pts [12 * L_cap] to reuse (a double buffer across frames).  -> (dict of
        laser_off, laser_frame, laser_pts, match_pose, has_match, Ltot); the dict can go into BatchSolver.rebind with the other inputs."""
        torch = self.torch
        cap = int(m["cap"])
        L_cap = self.B * cap if L_cap is None else int(L_cap)
        out = dict(out or {})
        if "match_pose" not in out:
            out["match_pose"] = torch.zeros(self.B * n * 12, dtype=torch.float64, device=self.dev)
        if "has_match" not in out:
            out["has_match"] = torch.zeros(self.B * n, dtype=torch.uint8, device=self.dev)
        fresh = bufs is None
        if fresh:   # every entry the result exposes is written by the call, but for the one padding entry of an empty pack
            bufs = dict(laser_off=torch.empty(self.B + 1, dtype=torch.int32, device=self.dev),
                        laser_frame=torch.empty(max(L_cap, 1), dtype=torch.int32, device=self.dev),
                        laser_pts=torch.empty(12 * max(L_cap, 1), dtype=torch.float64, device=self.dev))
        off, lf, lp = bufs["laser_off"], bufs["laser_frame"], bufs["laser_pts"]
        assert off.numel() >= self.B + 1 and lf.numel() >= max(L_cap, 1) and lp.numel() >= 12 * max(L_cap, 1)
        Ltot = self._chk(self.L.liw_lfe_pack_track(self.h, int(n), int(frame), cap, self._p(m["count"]), self._p(m["recs"]), self._p(m["match_pose"]),
                                                   L_cap, self._p(off), self._p(lf), self._p(lp), self._p(out["match_pose"]), self._p(out["has_match"]), self._s()))
        if fresh and Ltot == 0:   # no record: the entry kept so that no array is empty was never written
            lf[:1].zero_()
            lp[:12].zero_()
        res = dict(laser_off=off, laser_frame=lf[:max(Ltot, 1)], laser_pts=lp[:12 * max(Ltot, 1)], match_pose=out["match_pose"], has_match=out["has_match"])
        return res, Ltot

    # ------------------------------------------------------------------------------------------------- initialisation
    def _strided_poses(self, poses, F):
        """poses of F frames per robot -> (tensor kept alive, robot stride, frame stride) in doubles: a [B, F, k >= 6] float64 device
        tensor whose last stride is 1 (a view of x [B, n, 15] included) is passed as it is, anything else is packed to [B, F, 6]"""
        torch = self.torch
        if (torch.is_tensor(poses) and poses.dim() == 3 and poses.dtype == torch.float64 and poses.device == self.dev and poses.shape[0] == self.B
                and poses.shape[1] == F and poses.shape[2] >= 6 and poses.stride(2) == 1 and poses.stride(0) >= 0 and poses.stride(1) >= 0):
            return poses, int(poses.stride(0)), int(poses.stride(1))
        t = self._t(poses, torch.float64, (self.B, F, 6))
        return t, 6 * F, 6

    def match_front(self, front_slot, first_slot, F, pose_front, poses, kk=0, cap=256, out=None):
        """laser_manager::match_with_front of a whole INIT window in one launch: scan slots first_slot .. first_slot + F - 1 against
        `front_slot`, task (b, k) = match(front_slot, first_slot + k, pose_front, poses[:, k], kk) bit for bit.  pose_front [B, 6];
        poses [B, F, 6], or a strided view such as x.view(B, n, 15)[:, 1:, :6].  -> dict(count [B, F], recs [B, F, cap, 12],
        idx1 / idx2 [B, F, cap], match_pose [B, F, 12], cap, F); `out` may supply any of the tensors."""
        torch = self.torch
        F = int(F)
        pf = self._t(pose_front, torch.float64, (self.B, 6))
        ps, rs, fs = self._strided_poses(poses, F)
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=self.dev)
        o = {} if out is None else dict(out)
        for k, shape, dt in (("count", (self.B, F), torch.int32), ("recs", (self.B, F, cap, 12), torch.float64), ("idx1", (self.B, F, cap), torch.int32),
                             ("idx2", (self.B, F, cap), torch.int32), ("match_pose", (self.B, F, 12), torch.float64)):
            if k not in o:
                o[k] = z(*[max(int(v), 0) for v in shape], dt=dt)
            assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() >= int(np.prod(shape)), k
        o["cap"], o["F"] = int(cap), F
        self._chk(self.L.liw_lfe_match_front(self.h, self._p(self.store), int(front_slot), int(first_slot), F, self._p(pf), self._p(ps), rs, fs, int(kk),
                                             int(cap), self._p(o["count"]), self._p(o["recs"]), self._p(o["idx1"]), self._p(o["idx2"]),
                                             self._p(o["match_pose"]), self._s()))
        return o

    def pack_init(self, m, n, pose_front, out=None, L_cap=None, bufs=None):
        """the laser arrays of B n-frame INIT windows from a match_front() result with F = n - 1 (frame 0: the empty match at
        pose_front [B, 6]).  out: dict with `match_pose` [B * n * 12], `has_match` [B * n], `init_ok` [B] to write into; bufs:
        laser_off [B + 1], laser_frame [L_cap], laser_pts [12 * L_cap] to reuse.  -> (dict of laser_off, laser_frame, laser_pts,
        match_pose, has_match for BatchSolver.rebind, Ltot, init_ok [B] uint8: 1 iff every frame 1 .. n-1 has at least 2 pairs)."""
        torch = self.torch
        n, cap = int(n), int(m["cap"])
        assert int(m["F"]) == n - 1, "pack_init needs a match_front result with F = n - 1"
        L_cap = self.B * (n - 1) * cap if L_cap is None else int(L_cap)
        pf = self._t(pose_front, torch.float64, (self.B, 6))
        out = dict(out or {})
        for k, size, dt in (("match_pose", self.B * n * 12, torch.float64), ("has_match", self.B * n, torch.uint8), ("init_ok", self.B, torch.uint8)):
            if k not in out:
                out[k] = torch.zeros(max(size, 1), dtype=dt, device=self.dev)
            assert out[k].dtype == dt and out[k].is_contiguous() and out[k].numel() >= size, k
        fresh = bufs is None
        if fresh:
            bufs = dict(laser_off=torch.empty(self.B + 1, dtype=torch.int32, device=self.dev),
                        laser_frame=torch.empty(max(L_cap, 1), dtype=torch.int32, device=self.dev),
                        laser_pts=torch.empty(12 * max(L_cap, 1), dtype=torch.float64, device=self.dev))
        off, lf, lp = bufs["laser_off"], bufs["laser_frame"], bufs["laser_pts"]
        assert off.numel() >= self.B + 1 and lf.numel() >= max(L_cap, 1) and lp.numel() >= 12 * max(L_cap, 1)
        Ltot = self._chk(self.L.liw_lfe_pack_init(self.h, n, cap, self._p(m["count"]), self._p(m["recs"]), self._p(m["match_pose"]), self._p(pf), L_cap,
                                                  self._p(off), self._p(lf), self._p(lp), self._p(out["match_pose"]), self._p(out["has_match"]),
                                                  self._p(out["init_ok"]), self._s()))
        if fresh and Ltot == 0:   # no record: the entry kept so that no array is empty was never written
            lf[:1].zero_()
            lp[:12].zero_()
        res = dict(laser_off=off, laser_frame=lf[:max(Ltot, 1)], laser_pts=lp[:12 * max(Ltot, 1)], match_pose=out["match_pose"], has_match=out["has_match"])
        return res, Ltot, out["init_ok"]

    def rebuild(self, first_slot, F, poses, mask=None):
        """the sub-map rebuild after the INIT solve: clear_all_scan on the masked robots' managers (their scan slots are kept), then
        add_scan of slot first_slot + k at poses[:, k], k = 0 .. F - 1.  poses as in match_front (x.view(B, n, 15) is one)."""
        F = int(F)
        ps, rs, fs = self._strided_poses(poses, F)
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_rebuild(self.h, self._p(self.store), int(first_slot), F, self._p(ps), rs, fs, self._p(m), self._s()))

    # ------------------------------------------------------------------------------------------------ tracking glue
    def track_layout(self):
        """bytes of the tracking record of this front-end's dims (host-only)"""
        return track_bytes(self.dims)

    def _track(self, track):
        torch = self.torch
        assert torch.is_tensor(track) and track.dtype == torch.uint8 and track.is_contiguous() and track.device == self.dev
        assert track.numel() >= self.track_layout()
        return track

    def _out(self, t, dtype, numel):
        assert self.torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous() and t.device == self.dev and t.numel() >= numel
        return t

    def track_init(self, tp, track, x, angular_local=None, mask=None):
        """the tracking record (a uint8 device tensor of track_layout() bytes) of the masked robots (all when None) from the state
        rows x: [B, 15] or any float64 device view [B, k >= 6] whose last stride is 1 (x.view(B, n, 15)[:, n - 1] is one):
        last_keyframe_tf = make_tf(p, q), current_angular_local = angular_local [B, 3] (zero when None), counters 0."""
        torch = self.torch
        tps = track_params_struct(tp)
        if not (torch.is_tensor(x) and x.dim() == 2 and x.dtype == torch.float64 and x.device == self.dev and x.shape[0] == self.B and x.shape[1] >= 6
                and x.stride(1) == 1 and x.stride(0) >= 1):
            x = self._t(x, torch.float64, (self.B, -1))
        a = None if angular_local is None else self._t(angular_local, torch.float64, (self.B, 3))
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_track_init(self.h, C.byref(tps), self._p(self._track(track)), self._p(x), int(x.stride(0)), self._p(a), self._p(m), self._s()))
        return track

    def track_begin(self, tp, track, x, imu_X, imu_Dt, wheel_T, stamps, mask=None, out=None):
        """before the scan is processed: the de-skew twist from the current state, the min_delta_t gate, the roll of the two-frame
        window x [B, 2, 15] (float64, contiguous, updated in place) and the new frame's pose from the wheel increment.
        -> dict(linear [B, 3], angular [B, 3], pose_new [B, 6], skip [B] uint8); `out` may supply any of them."""
        torch = self.torch
        tps = track_params_struct(tp)
        self._out(x, torch.float64, self.B * 30)
        iX, iD = self._t(imu_X, torch.float64, (self.B, 15)), self._t(imu_Dt, torch.float64, (self.B,))
        wT, st = self._t(wheel_T, torch.float64, (self.B, 12)), self._t(stamps, torch.float64, (self.B,))
        o = dict(out or {})
        for k, w, dt in (("linear", 3, torch.float64), ("angular", 3, torch.float64), ("pose_new", 6, torch.float64), ("skip", 1, torch.uint8)):
            if k not in o:
                o[k] = torch.zeros((self.B, w) if w > 1 else (self.B,), dtype=dt, device=self.dev)
            self._out(o[k], dt, self.B * w)
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_track_begin(self.h, C.byref(tps), self._p(self._track(track)), self._p(x), self._p(iX), self._p(iD), self._p(wT), self._p(st),
                                             self._p(m), self._p(o["linear"]), self._p(o["angular"]), self._p(o["pose_new"]), self._p(o["skip"]), self._s()))
        return o

    def track_end(self, tp, track, slot, x, count, mask=None, out=None):
        """after the solve: the key-frame decision of the masked robots (all when None; mask out the skipped ones) from the solved
        x [B, 2, 15], the match count [B] int32 and the lines of scan `slot`.  -> dict(key [B] uint8, pose [B, 6]); key of frame t
        is corners_to_world's `clear` of frame t + 1."""
        torch = self.torch
        tps = track_params_struct(tp)
        self._out(x, torch.float64, self.B * 30)
        cnt = self._t(count, torch.int32, (self.B,))
        o = dict(out or {})
        if "key" not in o:
            o["key"] = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        if "pose" not in o:
            o["pose"] = torch.zeros(self.B, 6, dtype=torch.float64, device=self.dev)
        self._out(o["key"], torch.uint8, self.B)
        self._out(o["pose"], torch.float64, self.B * 6)
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_track_end(self.h, C.byref(tps), self._p(self._track(track)), self._p(self.store), int(slot), self._p(x), self._p(cnt),
                                           self._p(m), self._p(o["key"]), self._p(o["pose"]), self._s()))
        return o

    def track_get(self, track, robot):
        """-> dict(last_keyframe_tf [12], angular_local [3], stamp, tracked, keys, skipped) of one robot (synchronous)"""
        tf, a, st, cn = np.zeros(12), np.zeros(3), C.c_double(0), np.zeros(3, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        self._chk_get(self.L.liw_lfe_track_get(self.h, self._p(self._track(track)), int(robot), tf.ctypes.data_as(dp), a.ctypes.data_as(dp), C.byref(st),
                                               cn.ctypes.data_as(C.POINTER(C.c_int))))
        return dict(last_keyframe_tf=tf, angular_local=a, stamp=float(st.value), tracked=int(cn[0]), keys=int(cn[1]), skipped=int(cn[2]))

    # ------------------------------------------------------------------------------------------- initialisation glue
    def init_layout(self):
        """bytes of the initialisation record of this front-end's dims (host-only)"""
        return init_bytes(self.dims)

    def _init(self, init):
        torch = self.torch
        assert torch.is_tensor(init) and init.dtype == torch.uint8 and init.is_contiguous() and init.device == self.dev
        assert init.numel() >= self.init_layout()
        return init

    def init_reset(self, tp, init, mask=None):
        """init_current_status for the masked robots (all when None) of the initialisation record `init` (a uint8 device tensor of
        init_layout() bytes): p, q = log_SE3(T_imu_to_wheel^-1), the rest 0, INITIALIZING, an empty window, counters 0"""
        tps = track_params_struct(tp)
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_init_reset(self.h, C.byref(tps), self._p(self._init(init)), self._p(m), self._s()))
        return init

    def init_get(self, init, robot):
        """-> dict(status, n_frames, state [15] = p q v bs, angular_local [3], inits, failed, dropped) of one robot (synchronous)"""
        st, nf, x, a, cn = C.c_int(0), C.c_int(0), np.zeros(15), np.zeros(3), np.zeros(3, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        self._chk_get(self.L.liw_lfe_init_get(self.h, self._p(self._init(init)), int(robot), C.byref(st), C.byref(nf), x.ctypes.data_as(dp),
                                              a.ctypes.data_as(dp), cn.ctypes.data_as(C.POINTER(C.c_int))))
        return dict(status=int(st.value), n_frames=int(nf.value), state=x, angular_local=a, inits=int(cn[0]), failed=int(cn[1]), dropped=int(cn[2]))

    def init_window(self, N):
        """zeroed window arrays of B N-frame INIT windows: dict(x_init [B, N, 15] and the six interval arrays [B, N - 1, w])"""
        z = lambda *s: self.torch.zeros(*s, dtype=self.torch.float64, device=self.dev)
        return dict(x_init=z(self.B, N, 15), **{k: z(self.B, N - 1, w) for k, w in WINDOW_KEYS})

    def init_begin(self, tp, ip, init, interval, window, mask=None, out=None):
        """before the scan is processed, for the INITIALIZING robots of the mask (all when None): the is_static gate on the wheel
        increment, the pose prediction, the frame's state into row n_frames of window["x_init"] and its interval (dict of the six
        liw_batch arrays, [B, w]) into row n_frames - 1 of the window arrays (init_window), updated in place.
        -> dict(drop [B] uint8, slot_of [B] int32); `out` may supply them.  Rows of robots that are not INITIALIZING are not written."""
        torch = self.torch
        tps, ips = track_params_struct(tp), init_params_struct(ip)
        N = ips.slide_window_size
        iv = [self._t(interval[k], torch.float64, (self.B, w)) for k, w in WINDOW_KEYS]
        self._out(window["x_init"], torch.float64, self.B * N * 15)
        wv = [self._out(window[k], torch.float64, self.B * (N - 1) * w) for k, w in WINDOW_KEYS]
        o = dict(out or {})
        if "drop" not in o:
            o["drop"] = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        if "slot_of" not in o:
            o["slot_of"] = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self._out(o["drop"], torch.uint8, self.B)
        self._out(o["slot_of"], torch.int32, self.B)
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_init_begin(self.h, C.byref(tps), C.byref(ips), self._p(self._init(init)), *[self._p(t) for t in iv], self._p(m),
                                            self._p(window["x_init"]), *[self._p(t) for t in wv], self._p(o["drop"]), self._p(o["slot_of"]), self._s()))
        return o

    def slot_copy(self, dst_slot, mask=None):
        """scan slot 0 of the masked robots (all when None) -> slot dst_slot[b] [B] int32 of the same robot: header, status word,
        lines and line_map entries.  A dst_slot outside 1 .. slots-1 sets ST_INVALID in the robot word and copies nothing."""
        d = self._t(dst_slot, self.torch.int32, (self.B,))
        m = self._mask(mask)
        self._chk(self.L.liw_lfe_slot_copy(self.h, self._p(self.store), self._p(d), self._p(m), self._s()))

    def init_select(self, ip, init, out=None, R_host=None):
        """-> dict(ready [B] uint8, sel [B] int32 with the ready robots ascending in sel[:R], n_sel [1] int32 = R), all on the device
        and without a synchronisation; `out` may supply them.  R_host: a pinned int32 host tensor of one element that R is also
        copied into asynchronously (valid after the stream's next synchronisation)."""
        torch = self.torch
        ips = init_params_struct(ip)
        o = dict(out or {})
        for k, n, dt in (("ready", self.B, torch.uint8), ("sel", self.B, torch.int32), ("n_sel", 1, torch.int32)):
            if k not in o:
                o[k] = torch.zeros(n, dtype=dt, device=self.dev)
            self._out(o[k], dt, n)
        rh = None
        if R_host is not None:
            assert torch.is_tensor(R_host) and R_host.dtype == torch.int32 and R_host.device.type == "cpu" and R_host.numel() >= 1
            rh = C.c_void_p(R_host.data_ptr())
        self._chk(self.L.liw_lfe_init_select(self.h, C.byref(ips), self._p(self._init(init)), self._p(o["ready"]), self._p(o["sel"]), self._p(o["n_sel"]),
                                             rh, self._s()))
        return o

    def pack_init_sel(self, R, sel, m, n, pose_front, out=None, L_cap=None, bufs=None):
        """pack_init for the R robots sel[:R] (int32 device tensor) of a match_front() result over all B robots: window r of the
        output is robot sel[r].  pose_front: [B, 6], or a float64 device view [B, k >= 6] with last stride 1 (x_init[:, 0] is one).
        out / bufs as pack_init, sized for R windows.  -> (dict for BatchSolver.rebind, Ltot, init_ok [R] uint8)."""
        torch = self.torch
        R, n, cap = int(R), int(n), int(m["cap"])
        assert int(m["F"]) == n - 1, "pack_init_sel needs a match_front result with F = n - 1"
        L_cap = R * (n - 1) * cap if L_cap is None else int(L_cap)
        sel = self._out(sel, torch.int32, R)
        pf = pose_front
        if not (torch.is_tensor(pf) and pf.dim() == 2 and pf.dtype == torch.float64 and pf.device == self.dev and pf.shape[0] == self.B
                and pf.shape[1] >= 6 and pf.stride(1) == 1 and pf.stride(0) >= 6):
            pf = self._t(pf, torch.float64, (self.B, 6))
        out = dict(out or {})
        for k, size, dt in (("match_pose", R * n * 12, torch.float64), ("has_match", R * n, torch.uint8), ("init_ok", R, torch.uint8)):
            if k not in out:
                out[k] = torch.zeros(max(size, 1), dtype=dt, device=self.dev)
            assert out[k].dtype == dt and out[k].is_contiguous() and out[k].numel() >= size, k
        fresh = bufs is None
        if fresh:
            bufs = dict(laser_off=torch.empty(R + 1, dtype=torch.int32, device=self.dev),
                        laser_frame=torch.empty(max(L_cap, 1), dtype=torch.int32, device=self.dev),
                        laser_pts=torch.empty(12 * max(L_cap, 1), dtype=torch.float64, device=self.dev))
        off, lf, lp = bufs["laser_off"], bufs["laser_frame"], bufs["laser_pts"]
        assert off.numel() >= R + 1 and lf.numel() >= max(L_cap, 1) and lp.numel() >= 12 * max(L_cap, 1)
        Ltot = self._chk(self.L.liw_lfe_pack_init_sel(self.h, R, self._p(sel), n, cap, self._p(m["count"]), self._p(m["recs"]), self._p(m["match_pose"]),
                                                      self._p(pf), int(pf.stride(0)), L_cap, self._p(off), self._p(lf), self._p(lp),
                                                      self._p(out["match_pose"]), self._p(out["has_match"]), self._p(out["init_ok"]), self._s()))
        if fresh and Ltot == 0:   # no record: the entry kept so that no array is empty was never written
            lf[:1].zero_()
            lp[:12].zero_()
        res = dict(laser_off=off, laser_frame=lf[:max(Ltot, 1)], laser_pts=lp[:12 * max(Ltot, 1)], match_pose=out["match_pose"], has_match=out["has_match"])
        return res, Ltot, out["init_ok"]

    def init_commit(self, tp, ip, init, track, R, sel, init_ok, x_sol, x_init, x_track):
        """after the INIT solve of the compact batch (window r = robot sel[r]): for the robots with init_ok[r] the solved window
        x_sol[r] [N, 15] goes back into x_init [B, N, 15], both rows of x_track [B, 2, 15] and the records become the last solved
        frame, status TRACKING; the others restart (init_current_status, failed-window counter).  All tensors are updated in place."""
        torch = self.torch
        tps, ips = track_params_struct(tp), init_params_struct(ip)
        R, N = int(R), ips.slide_window_size
        self._out(sel, torch.int32, R)
        self._out(init_ok, torch.uint8, R)
        self._out(x_sol, torch.float64, R * N * 15)
        self._out(x_init, torch.float64, self.B * N * 15)
        self._out(x_track, torch.float64, self.B * 30)
        self._chk(self.L.liw_lfe_init_commit(self.h, C.byref(tps), C.byref(ips), self._p(self._init(init)), self._p(self._track(track)), R, self._p(sel),
                                             self._p(init_ok), self._p(x_sol), self._p(x_init), self._p(x_track), self._s()))

    # ----------------------------------------------------------------------------------------------------- diagnostics
    CR_SIN, CR_COS, CR_ATAN2 = 0, 1, 2

    def crmath_eval(self, op, a, b=None, out=None):
        """the sin (op 0), cos (op 1) or atan2(a, b) (op 2) of csrc/liw_crmath.hpp as track_begin evaluates them on the device, element
        by element in one launch: a, b float64 device tensors of n elements (b only for op 2), out such a tensor to write into (a
        itself is allowed) or None for a fresh one.  A diagnostic entry for the tests, on no tracking path."""
        torch = self.torch
        a = self._out(a, torch.float64, 0)
        n = a.numel()
        if b is not None:
            self._out(b, torch.float64, n)
        out = torch.empty_like(a) if out is None else self._out(out, torch.float64, n)
        self._chk(self.L.liw_lfe_crmath_eval(self.h, int(op), int(n), self._p(a), self._p(b), self._p(out), self._s()))
        return out

    # -------------------------------------------------------------------------------------------------------- getters
    def status(self, robot, slot=ROBOT):
        """status word (-1 for a missing sub-map)"""
        return self._chk_get(self.L.liw_lfe_status(self.h, self._p(self.store), int(robot), int(slot)), allow_missing=True)

    def _chk_get(self, r, allow_missing=False):
        if allow_missing and r == NONE:
            return -1
        if r < 0:
            raise self.LiwError(r, self.L.liw_lfe_last_error(self.h).decode())
        return r

    def num_lines(self, robot, slot):
        """number of lines (-1 for a missing sub-map)"""
        return self._chk_get(self.L.liw_lfe_num_lines(self.h, self._p(self.store), int(robot), int(slot)), allow_missing=True)

    def get_lines(self, robot, slot):
        """[num_lines, 10] = p1 p2 abc len in scan::lines order (None for a missing sub-map)"""
        n = self.num_lines(robot, slot)
        if n < 0:
            return None
        out = np.zeros((max(n, 1), 10))
        k = self._chk_get(self.L.liw_lfe_get_lines(self.h, self._p(self.store), int(robot), int(slot), out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return out[:k].copy()

    def cell_lines(self, robot, slot, x, y, cap=64):
        """(cell size, ids) as laser.Scan.cell_lines: size -1 outside the grid or for a missing sub-map"""
        ids = np.zeros(cap, dtype=np.int32)
        k = self._chk_get(self.L.liw_lfe_cell_lines(self.h, self._p(self.store), int(robot), int(slot), float(x), float(y),
                                                    ids.ctypes.data_as(C.POINTER(C.c_int)), int(cap)), allow_missing=True)
        return k, ids[:max(0, min(k, cap))].copy()

    def submap_pose(self, robot, slot=REF):
        p, q = np.zeros(3), np.zeros(3)
        r = self._chk_get(self.L.liw_lfe_submap_pose(self.h, self._p(self.store), int(robot), int(slot), p.ctypes.data_as(C.POINTER(C.c_double)),
                                                     q.ctypes.data_as(C.POINTER(C.c_double))), allow_missing=True)
        return None if r < 0 else (p, q)
