"""The fleet's occupancy-grid maps on the device (C ABI include/liw_map_batch.h): `FleetMapper` keeps the laser-frame scan of every
key frame of B robots in one store and renders the reference's 5 cm occupancy grid of the selected robots from the back-end's
corrected poses, on torch's current stream, without a host loop over robots and without a read-back.  It is the last stage of
`FleetTrajectory.step -> FleetLoopDetector.push -> FleetBackEnd.push -> FleetMapper.push`.  `gridmap.GridMap` (one robot, host
glue) is its parity reference.  `FleetGroupMap` (C ABI include/liw_map_group.h) renders one shared grid per group of a FleetMapper's
robots from the same store.  There is no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore, _pd
from .gridmap import MapInfoC, MapParamsC, _info_dict, _palette, office_map_params, params_struct

# every symbol include/liw_map_batch.h declares (checked by tests/test_map_batch_abi.py)
FMAP_EXPORTS = ["liw_fmap_store_bytes", "liw_fmap_layout", "liw_fmap_create", "liw_fmap_destroy", "liw_fmap_last_error", "liw_fmap_reset",
                "liw_fmap_add_keyframes", "liw_fmap_render_tf", "liw_fmap_render", "liw_fmap_num_submaps", "liw_fmap_full", "liw_fmap_get_submap",
                "liw_fmap_get_tf", "liw_fmap_last_info", "liw_fmap_get", "liw_fmap_device_data", "liw_fmap_write_pgm"]

# every symbol include/liw_map_group.h declares (checked by tests/test_map_group_abi.py)
GMAP_EXPORTS = ["liw_gmap_store_bytes", "liw_gmap_layout", "liw_gmap_create", "liw_gmap_destroy", "liw_gmap_last_error", "liw_gmap_reset",
                "liw_gmap_render_tf", "liw_gmap_render", "liw_gmap_last_info", "liw_gmap_members", "liw_gmap_get", "liw_gmap_device_data",
                "liw_gmap_write_pgm"]

OK, EMPTY, OVER_CELLS, RAY_TOO_LONG = 0, 1, 2, 3   # LIW_FMAP_*
INFO_BYTES = C.sizeof(MapInfoC)                    # sizeof(liw_map_info)
DIM_KEYS = ("B", "max_submaps", "max_points", "max_cells", "max_steps")


class FmapDimsC(C.Structure):
    _fields_ = [(k, C.c_int) for k in DIM_KEYS]


class FmapLayoutC(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("bytes", "robot_bytes", "shared_off", "shared_bytes", "cell_bytes", "offsets_off", "points_off", "index_off",
                                          "tf_off", "partial_off", "bits_off", "grid_off")] + [("partials", C.c_int)]


class GmapDimsC(C.Structure):
    _fields_ = [("G", C.c_int), ("max_cells", C.c_int)]


class GmapLayoutC(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("bytes", "group_bytes", "cell_bytes", "bits_off", "grid_off")] + [("cell_chunks", C.c_int)]


def dims_struct(d):
    if isinstance(d, FmapDimsC):
        return d
    return FmapDimsC(*[int(d[k]) for k in DIM_KEYS])


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_fmap_ready", False):
        vp, dp, ci, ll = C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_longlong
        pp, dd = C.POINTER(MapParamsC), C.POINTER(FmapDimsC)
        L.liw_fmap_store_bytes.argtypes = [pp, dd, C.POINTER(C.c_size_t)]
        L.liw_fmap_layout.argtypes = [pp, dd, C.POINTER(FmapLayoutC)]
        L.liw_fmap_create.restype = vp
        L.liw_fmap_create.argtypes = [pp, dd, dp, ci, ci]
        L.liw_fmap_destroy.argtypes = [vp]
        L.liw_fmap_last_error.restype = C.c_char_p
        L.liw_fmap_last_error.argtypes = [vp]
        L.liw_fmap_reset.argtypes = [vp, vp, vp, vp]
        L.liw_fmap_add_keyframes.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp]
        L.liw_fmap_render_tf.argtypes = [vp, vp, vp, ll, vp, vp, vp, vp]
        L.liw_fmap_render.argtypes = [vp, vp, vp, ll, vp, vp, vp, vp]
        L.liw_fmap_num_submaps.argtypes = [vp, vp, ci]
        L.liw_fmap_full.argtypes = [vp, vp, ci]
        L.liw_fmap_get_submap.argtypes = [vp, vp, ci, ci, ci, dp]
        L.liw_fmap_get_tf.argtypes = [vp, vp, ci, ci, dp]
        L.liw_fmap_last_info.argtypes = [vp, vp, ci, C.POINTER(MapInfoC), C.POINTER(ci)]
        L.liw_fmap_get.restype = ll
        L.liw_fmap_get.argtypes = [vp, vp, ci, C.POINTER(C.c_byte), ll]
        L.liw_fmap_device_data.restype = vp
        L.liw_fmap_device_data.argtypes = [vp, vp, ci]
        L.liw_fmap_write_pgm.argtypes = [vp, vp, ci, C.c_char_p, C.POINTER(C.c_ubyte)]
        gd = C.POINTER(GmapDimsC)
        L.liw_gmap_store_bytes.argtypes = [gd, C.POINTER(C.c_size_t)]
        L.liw_gmap_layout.argtypes = [gd, C.POINTER(GmapLayoutC)]
        L.liw_gmap_create.restype = vp
        L.liw_gmap_create.argtypes = [vp, gd]
        L.liw_gmap_destroy.argtypes = [vp]
        L.liw_gmap_last_error.restype = C.c_char_p
        L.liw_gmap_last_error.argtypes = [vp]
        L.liw_gmap_reset.argtypes = [vp, vp, vp, vp]
        L.liw_gmap_render_tf.argtypes = [vp, vp, vp, vp, ll, vp, vp, vp, vp, vp, vp]
        L.liw_gmap_render.argtypes = [vp, vp, vp, vp, ll, vp, vp, vp, vp, vp, vp]
        L.liw_gmap_last_info.argtypes = [vp, vp, ci, C.POINTER(MapInfoC), C.POINTER(ci)]
        L.liw_gmap_members.argtypes = [vp, vp, ci, C.POINTER(ci), C.POINTER(ci)]
        L.liw_gmap_get.restype = ll
        L.liw_gmap_get.argtypes = [vp, vp, ci, C.POINTER(C.c_byte), ll]
        L.liw_gmap_device_data.restype = vp
        L.liw_gmap_device_data.argtypes = [vp, vp, ci]
        L.liw_gmap_write_pgm.argtypes = [vp, vp, ci, C.c_char_p, C.POINTER(C.c_ubyte)]
        L._fmap_ready = True
    return L


def layout(params, dims):
    """dict of liw_fmap_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad params / dims"""
    from . import LiwError
    out = FmapLayoutC()
    r = _lib().liw_fmap_layout(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_fmap_layout: bad params or dims")
    return {k: getattr(out, k) for k, _ in FmapLayoutC._fields_}


def store_bytes(params, dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_fmap_store_bytes(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_fmap_store_bytes: bad params or dims")
    return n.value


def group_layout(G, max_cells):
    """dict of liw_gmap_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = GmapLayoutC()
    r = _lib().liw_gmap_layout(C.byref(GmapDimsC(int(G), int(max_cells))), C.byref(out))
    if r:
        raise LiwError(r, "liw_gmap_layout: bad dims")
    return {k: getattr(out, k) for k, _ in GmapLayoutC._fields_}


def group_store_bytes(G, max_cells):
    """bytes of the group store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_gmap_store_bytes(C.byref(GmapDimsC(int(G), int(max_cells))), C.byref(n))
    if r:
        raise LiwError(r, "liw_gmap_store_bytes: bad dims")
    return n.value


def info_rows(raw):
    """[B, INFO_BYTES] uint8 host array of liw_map_info rows -> list of dicts as GridMap.render_tf returns"""
    raw = np.ascontiguousarray(raw)
    return [_info_dict(MapInfoC.from_buffer_copy(r.tobytes())) for r in raw]


class FleetMapper(FleetStore):
    """prm: solver parameters (synth.office_params layout; T_imu_to_laser and normalize_extrinsics are used); map_params: dict as
    gridmap.office_map_params (None: those); dims: dict(B, max_submaps, max_points, max_cells, max_steps).  Owns the store (a torch
    uint8 tensor, with `guard` bytes of 0xA5 on either side for tests) and the outputs added [B] uint8, status [B] int32 and info
    [B, INFO_BYTES] uint8 (liw_map_info rows; infos() decodes them): device tensors, valid until the next call.  Every call runs on
    torch's current stream; reset, add_keyframes, render_tf, render, push and render_all neither synchronise nor read back.  Behind a
    FleetBackEnd give both the same number of key frames: push() stores a scan exactly when the back-end stored the key frame."""

    _destroy, _last_error = "liw_fmap_destroy", "liw_fmap_last_error"

    def __init__(self, prm, map_params=None, dims=None, device="cuda:0", guard=0):
        import torch
        from . import LiwError
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.params = dict(office_map_params() if map_params is None else map_params)
        self.dims = {k: int(dims[k]) for k in DIM_KEYS}
        self.B = self.dims["B"]
        self.dev = torch.device(device)
        self.lay = layout(self.params, self.dims)
        Til = np.ascontiguousarray(np.asarray(prm["T_imu_to_laser"], dtype=np.float64).reshape(16))
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_fmap_create(C.byref(params_struct(self.params)), C.byref(dims_struct(self.dims)), _pd(Til),
                                                    C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_fmap_create: bad params or dims")
        self._alloc_store(guard)
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        B = self.B
        self.added, self.status, self.info = z(B, dt=torch.uint8), z(B, dt=torch.int32), z(B, INFO_BYTES, dt=torch.uint8)
        self.reset()

    def reset(self, mask=None):
        m = self._mask(mask)
        self._chk(self.L.liw_fmap_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def add_keyframes(self, key, points, n_points, mask=None):
        """key [B] uint8, points [B, stride, 3] laser frame, n_points [B] int32 -> added [B] uint8: 1 where the scan was stored as the
        robot's next sub-map (0: key clear, or the robot is full)"""
        torch = self.torch
        k, p, n, m = self._t(key, torch.uint8, (self.B,)), self._t(points, torch.float64), self._t(n_points, torch.int32, (self.B,)), self._mask(mask)
        if p.dim() != 3 or p.shape[0] != self.B or p.shape[2] != 3 or p.shape[1] < 1:
            raise ValueError("points must be [B, stride, 3]")
        self._chk(self.L.liw_fmap_add_keyframes(self.h, self._ptr(self.store), self._ptr(k), self._ptr(p), C.c_int(int(p.shape[1])), self._ptr(n),
                                                self._ptr(m), self._ptr(self.added), self._stream()))
        return self.added

    def _strided(self, a, width):
        """a [B, n, width] float64 whose rows of a robot are contiguous (any stride between robots) -> (tensor kept alive, robot stride)"""
        torch = self.torch
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
        t = t.to(device=self.dev, dtype=torch.float64)
        if t.dim() != 3 or t.shape[0] != self.B or t.shape[2] != width:
            raise ValueError("expected [B, n, %d]" % width)
        if t.shape[1] and (t.stride(2) != 1 or t.stride(1) != width or (self.B > 1 and t.stride(0) < 0)):
            t = t.contiguous()
        return t, (int(t.stride(0)) if self.B > 1 else 0)

    def _render(self, fn, a, width, sel):
        t, stride = self._strided(a, width)
        s = self._mask(sel)
        self._src, self._sel = t, s   # kept: the kernels read them after this call has returned
        self._chk(fn(self.h, self._ptr(self.store), self._ptr(t), C.c_longlong(stride), self._ptr(s), self._ptr(self.status), self._ptr(self.info),
                     self._stream()))
        return dict(status=self.status, info=self.info)

    def render_tf(self, T_w_l, sel=None):
        """T_w_l [B, n, 12] world <- laser (R row-major, t), n at least the sub-maps of every selected robot; sel [B] uint8 (None: all)
        -> dict(status [B] int32, info [B, INFO_BYTES] uint8): rows of the selected robots"""
        return self._render(self.L.liw_fmap_render_tf, T_w_l, 12, sel)

    def render(self, poses, sel=None):
        """the same from IMU poses [B, n, 6] (p, rotation vector), e.g. FleetBackEnd.poses(): T_w_l is composed on the device"""
        return self._render(self.L.liw_fmap_render, poses, 6, sel)

    def push(self, step_out, scan, back_out, backend, mask=None):
        """One frame behind FleetBackEnd.push: store the scan (scan = FleetTracker.scan_points() of this step) of every robot in
        back_out["added"], and when back_out["n_due"] (already a host integer) is non-zero render the robots in back_out["due"], which
        were solved this frame, from backend.poses().  Adds no read-back.  -> dict(added, status, info, rendered (bool))"""
        pts, n = scan
        added = self.add_keyframes(back_out["added"], pts, n, mask=mask)
        rendered = bool(back_out["n_due"])
        if rendered:
            due = back_out["due"]
            if mask is not None:
                due = due & (self._mask(mask) != 0).to(self.torch.uint8)
            self.render(backend.poses(), sel=due)
        return dict(added=added, status=self.status, info=self.info, rendered=rendered)

    def render_all(self, backend, sel=None):
        """the end of a log: every (selected) robot's map from the back-end's corrected poses"""
        return self.render(backend.poses(), sel=sel)

    # ---- inspection (synchronous)
    def infos(self):
        """the info rows of the last render as dicts"""
        self._sync()
        return info_rows(self.info.cpu().numpy())

    def num_submaps(self, robot):
        self._sync()
        return self._chk(self.L.liw_fmap_num_submaps(self.h, self._ptr(self.store), C.c_int(robot)))

    def is_full(self, robot):
        self._sync()
        return bool(self._chk(self.L.liw_fmap_full(self.h, self._ptr(self.store), C.c_int(robot))))

    def submap(self, robot, k):
        """[n, 3] laser-frame points of sub-map k"""
        self._sync()
        n = self._chk(self.L.liw_fmap_get_submap(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.c_int(0), None))
        out = np.zeros((max(n, 1), 3))
        self._chk(self.L.liw_fmap_get_submap(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(k), C.c_int(n), _pd(out)))
        return out[:n]

    def tf(self, robot):
        """[n, 12]: the transforms the last render() composed for the robot"""
        self._sync()
        n = self._chk(self.L.liw_fmap_get_tf(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(0), None))
        out = np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_fmap_get_tf(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(n), _pd(out)))
        return out[:n]

    def info_of(self, robot):
        """info dict of the grid the robot holds, with `status` of its last render"""
        self._sync()
        i, st = MapInfoC(), C.c_int(0)
        self._chk(self.L.liw_fmap_last_info(self.h, self._ptr(self.store), C.c_int(robot), C.byref(i), C.byref(st)))
        return dict(_info_dict(i), status=st.value)

    def grid(self, robot):
        """the grid the robot holds, int8 [height][width]"""
        i = self.info_of(robot)
        n = i["width"] * i["height"]
        out = np.zeros(max(n, 1), dtype=np.int8)
        self._chk(self.L.liw_fmap_get(self.h, self._ptr(self.store), C.c_int(robot), out.ctypes.data_as(C.POINTER(C.c_byte)), C.c_longlong(n)))
        return out[:n].reshape(i["height"], i["width"])

    def device_data(self, robot):
        return self.L.liw_fmap_device_data(self.h, self._ptr(self.store), C.c_int(robot))

    def write_pgm(self, robot, path_stem, palette=None):
        self._sync()
        self._chk(self.L.liw_fmap_write_pgm(self.h, self._ptr(self.store), C.c_int(robot), str(path_stem).encode(), _palette(palette)))


class FleetGroupMap(FleetStore):
    """One shared occupancy grid per group of a FleetMapper's robots (C ABI include/liw_map_group.h): the grid of the concatenation
    of the members' sub-maps, robot b's moved into its group's frame by T_g_w[b].  mapper: the FleetMapper that holds the sub-maps
    (its store is read in place; a render overwrites its robots' tf scratch, so mapper.tf(b) returns T_g_l afterwards); G groups
    of at most max_cells cells each.  Owns the group store (`guard` bytes of 0xA5 on either side for tests) and the outputs gstatus
    [G] int32 and ginfo [G, INFO_BYTES] uint8: device tensors, valid until the next call.  Every call runs on torch's current
    stream; reset, render_tf, render and render_all neither synchronise nor read back."""

    _destroy, _last_error = "liw_gmap_destroy", "liw_gmap_last_error"

    def __init__(self, mapper, G, max_cells, guard=0):
        torch = mapper.torch
        self.torch, self.LiwError, self.L = torch, mapper.LiwError, _lib()
        self.mapper, self.G, self.max_cells, self.dev = mapper, int(G), int(max_cells), mapper.dev
        self.B = mapper.B
        self.lay = group_layout(self.G, self.max_cells)
        self.h = C.c_void_p(self.L.liw_gmap_create(mapper.h, C.byref(GmapDimsC(self.G, self.max_cells))))
        if not self.h:
            raise self.LiwError(-22, "liw_gmap_create: bad dims")
        self._alloc_store(guard)
        self.gstatus = torch.zeros(self.G, dtype=torch.int32, device=self.dev)
        self.ginfo = torch.zeros(self.G, INFO_BYTES, dtype=torch.uint8, device=self.dev)
        self.reset()

    def _gmask(self, m):
        return None if m is None else self._t(m, self.torch.uint8, (self.G,))

    def reset(self, gmask=None):
        m = self._gmask(gmask)
        self._chk(self.L.liw_gmap_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def _render(self, fn, a, width, group_of, T_g_w, gsel):
        torch = self.torch
        t, stride = self.mapper._strided(a, width)
        go = self._t(group_of, torch.int32, (self.B,))
        tg = None if T_g_w is None else self._t(T_g_w, torch.float64, (self.B, 12))
        s = self._gmask(gsel)
        self._keep = (t, go, tg, s)   # the kernels read them after this call has returned
        self._chk(fn(self.h, self._ptr(self.mapper.store), self._ptr(self.store), self._ptr(t), C.c_longlong(stride), self._ptr(go), self._ptr(tg),
                     self._ptr(s), self._ptr(self.gstatus), self._ptr(self.ginfo), self._stream()))
        return dict(status=self.gstatus, info=self.ginfo)

    def render_tf(self, T_w_l, group_of, T_g_w=None, gsel=None):
        """T_w_l [B, n, 12] as FleetMapper.render_tf takes it; group_of [B] int32 (outside 0 .. G-1: in no group); T_g_w [B, 12] group
        <- robot world (None: T_w_l is used bit for bit); gsel [G] uint8 (None: all) -> dict(status [G] int32, info [G, INFO_BYTES])"""
        return self._render(self.L.liw_gmap_render_tf, T_w_l, 12, group_of, T_g_w, gsel)

    def render(self, poses, group_of, T_g_w=None, gsel=None):
        """the same from IMU poses [B, n, 6] (p, rotation vector), e.g. FleetBackEnd.poses()"""
        return self._render(self.L.liw_gmap_render, poses, 6, group_of, T_g_w, gsel)

    def render_all(self, backend, group_of, T_g_w=None, gsel=None):
        """the end of a log: every (selected) group's map from the back-end's corrected poses"""
        return self.render(backend.poses(), group_of, T_g_w=T_g_w, gsel=gsel)

    def group_regions(self):
        """[G, group_bytes] uint8 view of the group regions"""
        return self.store.view(self.G, self.lay["group_bytes"])

    # ---- inspection (synchronous)
    def infos(self):
        """the info rows of the last render as dicts"""
        self._sync()
        return info_rows(self.ginfo.cpu().numpy())

    def info_of(self, g):
        """info dict of the grid the group holds, with `status` of its last render"""
        self._sync()
        i, st = MapInfoC(), C.c_int(0)
        self._chk(self.L.liw_gmap_last_info(self.h, self._ptr(self.store), C.c_int(g), C.byref(i), C.byref(st)))
        return dict(_info_dict(i), status=st.value)

    def members(self, g):
        """(member robots, sub-maps used) of the group's last render"""
        self._sync()
        r, k = C.c_int(0), C.c_int(0)
        self._chk(self.L.liw_gmap_members(self.h, self._ptr(self.store), C.c_int(g), C.byref(r), C.byref(k)))
        return r.value, k.value

    def grid(self, g):
        """the grid the group holds, int8 [height][width]"""
        i = self.info_of(g)
        n = i["width"] * i["height"]
        out = np.zeros(max(n, 1), dtype=np.int8)
        self._chk(self.L.liw_gmap_get(self.h, self._ptr(self.store), C.c_int(g), out.ctypes.data_as(C.POINTER(C.c_byte)), C.c_longlong(n)))
        return out[:n].reshape(i["height"], i["width"])

    def device_data(self, g):
        return self.L.liw_gmap_device_data(self.h, self._ptr(self.store), C.c_int(g))

    def write_pgm(self, g, path_stem, palette=None):
        self._sync()
        self._chk(self.L.liw_gmap_write_pgm(self.h, self._ptr(self.store), C.c_int(g), str(path_stem).encode(), _palette(palette)))
