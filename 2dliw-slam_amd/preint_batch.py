"""The fleet's pre-integration on the device (C ABI include/liw_preint_batch.h): `FleetPreint` keeps the IMU and wheel-odometry
accumulators of B robots in one store, is fed the raw messages that arrived before each robot's scan and emits the interval arrays
`FleetTracker.step` / `FleetTrajectory.step` take, on torch's current stream, without a host loop over robots and without a
read-back.  It is the front door of `FleetPreint.step -> FleetTrajectory.step -> FleetLoopDetector.push -> FleetBackEnd.push ->
FleetMapper.push`.  Unlike `BatchPreint` (closed, independent intervals of a log) the accumulators persist: the interval of a scan
that the gates threw away merges into the next one, the accumulator is reset with the bias at the scan's arrival, and the
imu_inited / wheel_odom_inited latch is part of a robot's state.  `ImuPreintegration` / `WheelPreintegration` (one robot, host) are
its parity reference.  There is no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore

# every symbol include/liw_preint_batch.h declares (checked by tests/test_preint_batch_abi.py)
FPRE_EXPORTS = ["liw_fpre_store_bytes", "liw_fpre_layout", "liw_fpre_create", "liw_fpre_destroy", "liw_fpre_last_error", "liw_fpre_reset",
                "liw_fpre_push", "liw_fpre_commit", "liw_fpre_get"]

DIM_KEYS = ("B",)
ROW_KEYS = ("imu_X", "imu_J", "imu_sqrtP", "imu_Dt", "wheel_T", "wheel_sqrtP", "wheel_Dt")   # the liw_batch rows of a push
ROW_WIDTH = dict(imu_X=15, imu_J=225, imu_sqrtP=225, imu_Dt=1, wheel_T=12, wheel_sqrtP=9, wheel_Dt=1)
LAYOUT_PARTS = ("X_off", "J_off", "P_off", "imu_last_off", "wheel_off", "pending_off", "latch_off")


class FpreDimsC(C.Structure):
    _fields_ = [(k, C.c_int) for k in DIM_KEYS]


class FpreLayoutC(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("bytes", "robot_bytes", "shared_off", "shared_bytes") + LAYOUT_PARTS] + [("mat_pitch", C.c_int)]


class FpreStateC(C.Structure):
    _d = C.c_double
    _fields_ = [("X", _d * 15), ("J", _d * 225), ("P", _d * 225), ("last_acc", _d * 3), ("last_gyro", _d * 3), ("last_add_imu_time", _d), ("imu_Dt", _d),
                ("delta_Tij", _d * 12), ("last_pose", _d * 12), ("v", _d * 3), ("omega", _d * 3), ("last_update_time", _d), ("last_add_time", _d),
                ("wheel_Dt", _d), ("pending_stamp", _d), ("pending_bias", _d * 6), ("imu_inited", C.c_ubyte), ("wheel_odom_inited", C.c_ubyte)]


def dims_struct(d):
    if isinstance(d, FpreDimsC):
        return d
    return FpreDimsC(*[int(d[k]) for k in DIM_KEYS])


def _lib():
    from . import ParamsC, lib
    L = lib()
    if not getattr(L, "_fpre_ready", False):
        vp, ci = C.c_void_p, C.c_int
        dd = C.POINTER(FpreDimsC)
        L.liw_fpre_store_bytes.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_fpre_layout.argtypes = [dd, C.POINTER(FpreLayoutC)]
        L.liw_fpre_create.restype = vp
        L.liw_fpre_create.argtypes = [C.POINTER(ParamsC), dd]
        L.liw_fpre_destroy.argtypes = [vp]
        L.liw_fpre_last_error.restype = C.c_char_p
        L.liw_fpre_last_error.argtypes = [vp]
        L.liw_fpre_reset.argtypes = [vp, vp, vp, vp]
        L.liw_fpre_push.argtypes = [vp] * 18
        L.liw_fpre_commit.argtypes = [vp, vp, vp, vp, vp]
        L.liw_fpre_get.argtypes = [vp, vp, ci, C.POINTER(FpreStateC)]
        L._fpre_ready = True
    return L


def layout(dims):
    """dict of liw_fpre_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = FpreLayoutC()
    r = _lib().liw_fpre_layout(C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_fpre_layout: bad dims")
    return {k: getattr(out, k) for k, _ in FpreLayoutC._fields_}


def store_bytes(dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_fpre_store_bytes(C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_fpre_store_bytes: bad dims")
    return n.value


class FleetPreint(FleetStore):
    """prm: solver parameters (synth.office_params layout; the noise sigmas are used); B: robots.  Owns the store (a torch uint8
    tensor, with `guard` bytes of 0xA5 on either side for tests) and the rows of the last push: imu_X [B, 15], imu_J [B, 225],
    imu_sqrtP [B, 225], imu_Dt [B], wheel_T [B, 12], wheel_sqrtP [B, 9], wheel_Dt [B] (the liw_batch layout) and ready [B] uint8:
    device tensors, valid until the next push.  Every call runs on torch's current stream; reset, push, commit and step's own work
    neither synchronise nor read back.  Messages come as torch tensors or numpy arrays: imu_off / wheel_off [B + 1] int32 offsets
    into imu [n, 7] (t, acc, gyro) and wheel [m, 13] (t, R row-major, t), per robot in time order and stamped at or before the
    robot's scan; a robot whose offsets do not grow has no messages."""

    _destroy, _last_error = "liw_fpre_destroy", "liw_fpre_last_error"

    def __init__(self, prm, B, device="cuda:0", guard=0):
        import torch
        from . import LiwError, params_struct
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.dims = dict(B=int(B))
        self.B = B = self.dims["B"]
        self.dev = torch.device(device)
        self.lay = layout(self.dims)
        self._ps = params_struct(prm, self.dev.index if self.dev.index is not None else 0)
        self.h = C.c_void_p(self.L.liw_fpre_create(C.byref(self._ps), C.byref(dims_struct(self.dims))))
        if not self.h:
            raise LiwError(-22, "liw_fpre_create: bad params or dims")
        self._alloc_store(guard)
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=self.dev)
        self.rows = {k: (z(B, w) if w > 1 else z(B)) for k, w in ROW_WIDTH.items()}
        self.ready = z(B, dt=torch.uint8)
        self._eye12 = z(12)
        self._eye12[0] = self._eye12[4] = self._eye12[8] = 1.0
        self._keep = None
        self.reset()

    def reset(self, mask=None):
        """the accumulators as ImuPreintegration(prm) / WheelPreintegration(prm) start, latches off"""
        m = self._mask(mask)
        self._chk(self.L.liw_fpre_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def _msgs(self, off, rows, width):
        torch = self.torch
        o = self._t(off, torch.int32, (self.B + 1,))
        r = self._t(rows, torch.float64)
        if r.numel() == 0:
            r = torch.zeros(1, width, dtype=torch.float64, device=self.dev)   # the entry wants a pointer even when nobody has a message
        if r.dim() != 2 or r.shape[1] != width:
            raise ValueError("messages must be [n, %d]" % width)
        return o, r

    def push(self, imu_off, imu, wheel_off, wheel, stamps, bias, mask=None, out=None):
        """one scan of every robot: its messages into the persisted accumulators, (stamps [B], bias [B, 6] = ba bw at the scan's
        arrival) stored as pending, and the accumulators aligned with the stamp on a copy -> dict of the seven rows plus ready [B]
        uint8 (both latches set).  out: dict of tensors to write instead of the owned ones (tests).  Of a masked-out robot nothing is
        written."""
        torch, B = self.torch, self.B
        io, im = self._msgs(imu_off, imu, 7)
        wo, wm = self._msgs(wheel_off, wheel, 13)
        st, bi, m = self._t(stamps, torch.float64, (B,)), self._t(bias, torch.float64, (B, 6)), self._mask(mask)
        o = dict(self.rows, ready=self.ready) if out is None else out
        self._keep = (io, im, wo, wm, st, bi, m)   # kept: the kernels read them after this call has returned
        p = self._ptr
        self._chk(self.L.liw_fpre_push(self.h, p(self.store), p(io), p(im), p(wo), p(wm), p(st), p(bi), p(m), *[p(o[k]) for k in ROW_KEYS],
                                       p(o["ready"]), self._stream()))
        return o

    def commit(self, taken, mask=None):
        """after the frame: reset_imu_measure(stamp, bias) / reset_wheel_odom_measure(stamp) with the pending stamp and bias for the
        robots with taken[b] whose two latches are set; every other robot keeps its accumulators un-aligned, so that its next
        interval merges with this one"""
        t, m = self._t(taken, self.torch.uint8, (self.B,)), self._mask(mask)
        self._keep_commit = (t, m)
        self._chk(self.L.liw_fpre_commit(self.h, self._ptr(self.store), self._ptr(t), self._ptr(m), self._stream()))

    def step(self, fleet, ranges, stamps, imu_off, imu, wheel_off, wheel):
        """one frame of a FleetTracker or FleetTrajectory behind its sensors: push with current_bs at the scan's arrival (fleet.bias()
        read BEFORE fleet.step, which is what lvio_2d_trajectory.hpp:123 resets with; for an INITIALIZING robot of a FleetTrajectory
        current_bs of its initialisation record), fleet.step on the rows, commit of the robots whose frame was taken.  A robot that is
        not ready (a latch is off) is handed wheel_T = identity and imu_Dt = 0, so the gate that applies to it (min_delta_t or
        is_static) leaves it untouched; such frames count in the fleet's skipped / dropped counters.  The gates read the ALIGNED
        interval, as liw_lfe_track_begin / liw_lfe_init_begin define; the reference reads the un-aligned accumulator there.
        -> fleet.step's dict plus ready [B] uint8 and taken [B] uint8 = ready and not skipped and not dropped."""
        torch, B = self.torch, self.B
        bias = fleet.bias()
        if hasattr(fleet, "init"):   # FleetTrajectory: doubles 9 .. 14 of a 256-byte initialisation record are current_bs
            rec = fleet.init.view(torch.float64).view(B, 32)[:, 9:15]
            bias = torch.where((fleet.status() == 1)[:, None], bias, rec)
        o = self.push(imu_off, imu, wheel_off, wheel, stamps, bias)
        rd = o["ready"].bool()
        iv = {k: o[k] for k in ROW_KEYS if k != "wheel_Dt"}
        iv["wheel_T"] = torch.where(rd[:, None], o["wheel_T"], self._eye12[None, :])
        iv["imu_Dt"] = torch.where(rd, o["imu_Dt"], torch.zeros_like(o["imu_Dt"]))
        self._iv = iv
        res = fleet.step(ranges, stamps, iv)
        taken = o["ready"] & (res["skip"] ^ 1)
        if "drop" in res:
            taken = taken & (res["drop"] ^ 1)
        self.commit(taken)
        return dict(res, ready=o["ready"], taken=taken)

    # ---- inspection (synchronous)
    def get(self, robot):
        """the robot's persisted accumulators as a dict of numpy arrays / floats (J, P [15, 15]; delta_Tij, last_pose [12])"""
        self._sync()
        s = FpreStateC()
        self._chk(self.L.liw_fpre_get(self.h, self._ptr(self.store), C.c_int(robot), C.byref(s)))
        out = {}
        for k, t in FpreStateC._fields_:
            v = getattr(s, k)
            out[k] = np.array(v[:]) if hasattr(v, "__len__") else v
        out["J"], out["P"] = out["J"].reshape(15, 15), out["P"].reshape(15, 15)
        return out
