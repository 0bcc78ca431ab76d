"""The fleet's key-frame sink and laser loop detector on the device (C ABI include/liw_loop_batch.h): `FleetLoopDetector` takes
the key / pose / acc / n_acc tensors `FleetTracker.step` / `FleetTrajectory.step` return, appends the key frames of the robots
whose key is set to a per-robot store with their sub-map features, and runs laser_loop_detect for each of them, on torch's
current stream and without a host loop over robots.  `loop.LoopDetector` (one robot, host glue) is its parity reference.  There is
no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950 device.  What `push` returns goes on to
posegraph_batch.FleetBackEnd.push, the fleet's pose-graph back-end, and the occupancy map per robot is map_batch.FleetMapper's; non-laser key frames stay with the caller."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore, _pd, _pi
from .loop import LoopParamsC, params_struct, sizes, tf12_to_mat

# every symbol include/liw_loop_batch.h declares (checked by tests/test_loop_batch_abi.py)
FLOOP_EXPORTS = ["liw_floop_store_bytes", "liw_floop_layout", "liw_floop_create", "liw_floop_destroy", "liw_floop_last_error", "liw_floop_reset",
                 "liw_floop_add_keyframes", "liw_floop_detect", "liw_floop_num_keyframes", "liw_floop_full", "liw_floop_status",
                 "liw_floop_get_points", "liw_floop_get_row"]

OVER_CORNERS = 4   # LIW_FLOOP_OVER_CORNERS, besides loop.NULL / VALID / OVER_CAP / DIJ_OVERFLOW
STATS = ("candidates", "launched", "tasks", "quick_pass", "accepted", "icp_checked")


class FloopDimsC(C.Structure):
    _fields_ = [("B", C.c_int), ("max_keyframes", C.c_int), ("max_points", C.c_int), ("max_kf_corners", C.c_int)]


class FloopLayoutC(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("robot_bytes", C.c_size_t), ("scratch_off", C.c_size_t), ("scratch_bytes", C.c_size_t),
                ("feature_bytes", C.c_size_t), ("feature_slots", C.c_int), ("stride", C.c_int), ("quick_words", C.c_int)]


def dims_struct(d):
    if isinstance(d, FloopDimsC):
        return d
    return FloopDimsC(int(d["B"]), int(d["max_keyframes"]), int(d["max_points"]), int(d["max_kf_corners"]))


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_floop_ready", False):
        vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
        pp, dd = C.POINTER(LoopParamsC), C.POINTER(FloopDimsC)
        L.liw_floop_store_bytes.argtypes = [pp, dd, C.POINTER(C.c_size_t)]
        L.liw_floop_layout.argtypes = [pp, dd, C.POINTER(FloopLayoutC)]
        L.liw_floop_create.restype = vp
        L.liw_floop_create.argtypes = [pp, dd, dp, C.c_int, C.c_int]
        L.liw_floop_destroy.argtypes = [vp]
        L.liw_floop_last_error.restype = C.c_char_p
        L.liw_floop_last_error.argtypes = [vp]
        L.liw_floop_reset.argtypes = [vp, vp, vp, vp]
        L.liw_floop_add_keyframes.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.liw_floop_detect.argtypes = [vp] * 9
        L.liw_floop_num_keyframes.argtypes = [vp, vp, C.c_int]
        L.liw_floop_full.argtypes = [vp, vp, C.c_int]
        L.liw_floop_status.argtypes = [vp, vp, C.c_int, C.c_int, ip, dp, dp]
        L.liw_floop_get_points.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, dp]
        L.liw_floop_get_row.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, C.POINTER(C.c_ulonglong)]
        L._floop_ready = True
    return L


def layout(params, dims):
    """dict of liw_floop_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad params / dims"""
    from . import LiwError
    out = FloopLayoutC()
    r = _lib().liw_floop_layout(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_floop_layout: bad params or dims")
    return {k: getattr(out, k) for k, _ in FloopLayoutC._fields_}


def store_bytes(params, dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_floop_store_bytes(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_floop_store_bytes: bad params or dims")
    return n.value


class FleetLoopDetector(FleetStore):
    """prm: solver parameters (synth.office_params layout; T_imu_to_wheel and normalize_extrinsics are used); loop_params: dict as
    loop.office_loop_params; dims: dict(B, max_keyframes, max_points, max_kf_corners).  Owns the store (a torch uint8 tensor, with
    `guard` bytes of 0xA5 on either side for tests) and the outputs added [B] uint8, found [B] uint8, edge [B, 3] int32, tf12 [B, 12], stats [B, 6]
    int64: views valid until the next call.  Every call runs on torch's current stream; add_keyframes, detect and push neither
    synchronise nor read back."""

    _destroy, _last_error = "liw_floop_destroy", "liw_floop_last_error"

    def __init__(self, prm, loop_params, dims, device="cuda:0", guard=0):
        import torch
        from . import LiwError
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.params, self.dims = dict(loop_params), {k: int(dims[k]) for k in ("B", "max_keyframes", "max_points", "max_kf_corners")}
        self.B = self.dims["B"]
        self.dev = torch.device(device)
        self.lay = layout(self.params, self.dims)
        self.W, self.n_angle = sizes(self.params)
        Tiw = np.ascontiguousarray(np.asarray(prm["T_imu_to_wheel"], dtype=np.float64).reshape(16))
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_floop_create(C.byref(params_struct(self.params)), C.byref(dims_struct(self.dims)), _pd(Tiw),
                                                     C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_floop_create: bad params or dims")
        self._alloc_store(guard)
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        B = self.B
        self.found, self.edge, self.tf12, self.stats = z(B, dt=torch.uint8), z(B, 3, dt=torch.int32), z(B, 12, dt=torch.float64), z(B, 6, dt=torch.int64)
        self.added = z(B, dt=torch.uint8)
        self.reset()

    def reset(self, mask=None):
        m = self._mask(mask)
        self._chk(self.L.liw_floop_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def add_keyframes(self, key, pose, corners, n_corners, mask=None):
        """key [B] uint8, pose [B, 6] (p, rotation vector), corners [B, stride, 3] world frame, n_corners [B] int32
        -> added [B] uint8: 1 where the key frame was stored (0: key clear, or the robot is full)"""
        torch = self.torch
        k, p = self._t(key, torch.uint8, (self.B,)), self._t(pose, torch.float64, (self.B, 6))
        c, n, m = self._t(corners, torch.float64), self._t(n_corners, torch.int32, (self.B,)), self._mask(mask)
        if c.dim() != 3 or c.shape[0] != self.B or c.shape[2] != 3 or c.shape[1] < 1:
            raise ValueError("corners must be [B, stride, 3]")
        self._chk(self.L.liw_floop_add_keyframes(self.h, self._ptr(self.store), self._ptr(k), self._ptr(p), self._ptr(c), C.c_int(int(c.shape[1])),
                                                 self._ptr(n), self._ptr(m), self._ptr(self.added), self._stream()))
        return self.added

    def detect(self, key, mask=None):
        """-> dict(found [B] uint8, edge [B, 3] int32 (index1, index2, size), tf12 [B, 12], stats [B, 6] int64)"""
        k, m = self._t(key, self.torch.uint8, (self.B,)), self._mask(mask)
        self._chk(self.L.liw_floop_detect(self.h, self._ptr(self.store), self._ptr(k), self._ptr(m), self._ptr(self.found), self._ptr(self.edge),
                                          self._ptr(self.tf12), self._ptr(self.stats), self._stream()))
        return dict(found=self.found, edge=self.edge, tf12=self.tf12, stats=self.stats)

    def full(self):
        """[B] bool: robots that were offered a key frame while holding max_keyframes"""
        return self.robot_regions()[:, 4:8].contiguous().view(self.torch.int32)[:, 0] != 0

    def push(self, step_out, mask=None):
        """add + detect for the key frames of a FleetTracker.step / FleetTrajectory.step result.  A robot that is full gets no
        detection for the key frame that was not stored.  The result also carries `added`, which posegraph_batch.FleetBackEnd.push
        takes as its key so that both stores hold the same key frames."""
        added = self.add_keyframes(step_out["key"], step_out["pose"], step_out["acc"], step_out["n_acc"], mask=mask)
        return dict(self.detect(added, mask=mask), added=added)

    # ---- inspection (synchronous)
    def num_keyframes(self, robot):
        self._sync()
        return self._chk(self.L.liw_floop_num_keyframes(self.h, self._ptr(self.store), C.c_int(robot)))

    def is_full(self, robot):
        self._sync()
        return bool(self._chk(self.L.liw_floop_full(self.h, self._ptr(self.store), C.c_int(robot))))

    def status(self, robot, k):
        self._sync()
        n, o, t = C.c_int(0), np.zeros(12), np.zeros(12)
        st = self._chk(self.L.liw_floop_status(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.byref(n), _pd(o), _pd(t)))
        return dict(state=st, n_points=n.value, origin=tf12_to_mat(o), tf=tf12_to_mat(t))

    def get_points(self, robot, k):
        self._sync()
        n = self._chk(self.L.liw_floop_get_points(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.c_int(0), None))
        out = np.zeros((max(n, 1), 3))
        self._chk(self.L.liw_floop_get_points(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.c_int(n), _pd(out)))
        return out[:n]

    def get_row(self, robot, k, i):
        self._sync()
        cap = self.dims["max_points"]
        dij, j, aij = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap)
        q = np.zeros(self.W, dtype=np.uint64)
        m = self._chk(self.L.liw_floop_get_row(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.c_int(i), C.c_int(cap), _pi(dij), _pi(j),
                                               _pd(aij), q.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return dict(dij=dij[:m].copy(), j=j[:m].copy(), aij=aij[:m].copy(), quick=q)
