"""Localisation of fleet robots in a held occupancy grid on the device (C ABI include/liw_map_locate.h): `FleetLocalizer` turns the
grids a `FleetMapper` (one per robot) or a `FleetGroupMap` (one per group) holds into dilated fields once, and then gives each of Q
query rows (a laser-frame scan, e.g. `FleetTracker.scan_points()`, and a rough prior pose in the map) the best whole-cell, whole
table-step pose by the exhaustive correlative scan match, on torch's current stream and without a read-back.  `link_tf` turns a
found pose into the T_g_w row `FleetGroupMap.render` takes for that robot.  There is no CPU fallback: compute calls raise
LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore, _pd
from .gridmap import MapInfoC, _info_dict

# every symbol include/liw_map_locate.h declares (checked by tests/test_map_locate_abi.py)
FLOC_EXPORTS = ["liw_floc_store_bytes", "liw_floc_layout", "liw_floc_create", "liw_floc_destroy", "liw_floc_last_error", "liw_floc_build",
                "liw_floc_match", "liw_floc_link_tf", "liw_floc_field_info", "liw_floc_get_field", "liw_floc_device_field"]

FIELD_OK, FIELD_EMPTY, FIELD_OVER = 0, 1, 2          # LIW_FLOC_FIELD_*
OK, NO_MAP, NO_POINTS, BAD_PRIOR = 0, 1, 2, 3        # LIW_FLOC_*
MAX_W, MAX_THETA, MAX_STRIDE = 31, 256, 1 << 20
DIM_KEYS = ("Q", "M", "max_cells", "max_theta")


class FlocDimsC(C.Structure):
    _fields_ = [(k, C.c_int) for k in DIM_KEYS]


class FlocLayoutC(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("bytes", "map_bytes", "field_bytes", "field_off", "partial_off", "row_bytes")] + [("cell_chunks", C.c_int)]


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_floc_ready", False):
        vp, dp, ci, ll, sz = C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_longlong, C.c_size_t
        dd = C.POINTER(FlocDimsC)
        L.liw_floc_store_bytes.argtypes = [dd, C.POINTER(sz)]
        L.liw_floc_layout.argtypes = [dd, C.POINTER(FlocLayoutC)]
        L.liw_floc_create.restype = vp
        L.liw_floc_create.argtypes = [dd, dp, ci, ci]
        L.liw_floc_destroy.argtypes = [vp]
        L.liw_floc_last_error.restype = C.c_char_p
        L.liw_floc_last_error.argtypes = [vp]
        L.liw_floc_build.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.liw_floc_match.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.liw_floc_link_tf.argtypes = [vp, vp, vp, ll, vp, vp, vp, vp, vp]
        L.liw_floc_field_info.argtypes = [vp, vp, ci, C.POINTER(MapInfoC), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.liw_floc_get_field.restype = ll
        L.liw_floc_get_field.argtypes = [vp, vp, ci, C.POINTER(C.c_ubyte), ll]
        L.liw_floc_device_field.restype = vp
        L.liw_floc_device_field.argtypes = [vp, vp, ci]
        L._floc_ready = True
    return L


def layout(Q, M, max_cells, max_theta):
    """dict of liw_floc_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = FlocLayoutC()
    r = _lib().liw_floc_layout(C.byref(FlocDimsC(int(Q), int(M), int(max_cells), int(max_theta))), C.byref(out))
    if r:
        raise LiwError(r, "liw_floc_layout: bad dims")
    return {k: getattr(out, k) for k, _ in FlocLayoutC._fields_}


def store_bytes(Q, M, max_cells, max_theta):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_floc_store_bytes(C.byref(FlocDimsC(int(Q), int(M), int(max_cells), int(max_theta))), C.byref(n))
    if r:
        raise LiwError(r, "liw_floc_store_bytes: bad dims")
    return n.value


def angle_table(half_width_rad, step_rad):
    """[n, 2] float64 (cos, sin) of the angles k * step for k = -n_half .. n_half, n_half = floor(half_width / step + 1e-9): numpy on
    the host, as the laser front-end's table; the middle row is the angle 0, (1, 0) exactly"""
    n_half = int(np.floor(float(half_width_rad) / float(step_rad) + 1e-9))
    a = np.arange(-n_half, n_half + 1, dtype=np.float64) * float(step_rad)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


class FleetLocalizer(FleetStore):
    """source: the FleetMapper or FleetGroupMap whose grids are matched against (map m = robot / group m), or a dict(store (a torch
    uint8 device tensor of M regions), M, region_bytes, grid_off, max_cells) for a hand-made source: each region holds a liw_map_info
    at byte 32 and an int8 grid at grid_off.  Q query rows; tables of at most max_theta angles; prm: solver parameters (T_imu_to_laser
    and normalize_extrinsics are used by link_tf; None: synth.office_params()).  Owns the store (`guard` bytes of 0xA5 on either side
    for tests) and the outputs found [Q] uint8, best [Q, 4] int32 (j, ix, iy, score), stats [Q, 4] int32 (status, n_valid, ties, 0),
    T_m_l, T_w_l, T_g_w [Q, 12] float64: device tensors, valid until the next call.  Every compute call runs on torch's current stream;
    build, match and link_tf neither synchronise nor read back.  A fresh localiser holds M EMPTY fields: call build()."""

    _destroy, _last_error = "liw_floc_destroy", "liw_floc_last_error"

    def __init__(self, source, Q, max_theta=64, prm=None, guard=0):
        import torch
        from . import LiwError
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        if isinstance(source, dict):
            self.src_store, self.M = source["store"], int(source["M"])
            self.region_bytes, self.grid_off, self.max_cells = int(source["region_bytes"]), int(source["grid_off"]), int(source["max_cells"])
        else:
            self.src_store = source.store
            if hasattr(source, "G"):      # a FleetGroupMap
                self.M, self.region_bytes, self.max_cells = source.G, source.lay["group_bytes"], source.max_cells
            else:                         # a FleetMapper
                self.M, self.region_bytes, self.max_cells = source.B, source.lay["robot_bytes"], source.dims["max_cells"]
            self.grid_off = source.lay["grid_off"]
        self.source = source              # kept alive: build() reads its store
        self.dev = self.src_store.device
        self.Q, self.B, self.max_theta = int(Q), int(Q), int(max_theta)
        self.lay = layout(self.Q, self.M, self.max_cells, self.max_theta)
        if prm is None:
            from . import synth
            prm = synth.office_params()
        Til = np.ascontiguousarray(np.asarray(prm["T_imu_to_laser"], dtype=np.float64).reshape(16))
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_floc_create(C.byref(FlocDimsC(self.Q, self.M, self.max_cells, self.max_theta)), _pd(Til),
                                                    C.c_int(int(bool(prm.get("normalize_extrinsics", True)))), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_floc_create: bad dims")
        self._alloc_store(guard)
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        Q = self.Q
        self.found, self.best, self.stats = z(Q, dt=torch.uint8), z(Q, 4, dt=torch.int32), z(Q, 4, dt=torch.int32)
        self.T_m_l, self.T_w_l, self.T_g_w = z(Q, 12, dt=torch.float64), z(Q, 12, dt=torch.float64), z(Q, 12, dt=torch.float64)
        self.build(src_of=np.full(self.M, -1, np.int32))      # EMPTY headers

    def build(self, src_of=None, msel=None):
        """grid -> field for every map with msel[m] != 0 (None: all); src_of [M] int32: the source region of map m (None: m itself;
        negative: the map becomes EMPTY)"""
        torch = self.torch
        so = torch.arange(self.M, dtype=torch.int32, device=self.dev) if src_of is None else self._t(src_of, torch.int32, (self.M,))
        ms = None if msel is None else self._t(msel, torch.uint8, (self.M,))
        self._keep_build = (so, ms)       # the kernels read them after this call has returned
        self._chk(self.L.liw_floc_build(self.h, self._ptr(self.store), self._ptr(self.src_store), C.c_size_t(self.region_bytes), C.c_size_t(self.grid_off),
                                        self._ptr(so), self._ptr(ms), self._stream()))

    def match(self, map_of, points, n_points, T0, table, W, min_permille=0, mask=None):
        """map_of [Q] int32; points [Q, stride, 3] laser frame; n_points [Q] int32; T0 [Q, 12] the prior map <- laser (R row-major 9,
        then t); table [n_theta, 2] (cos, sin), e.g. angle_table(); W the window half-width in cells (0 .. 31); mask [Q] uint8
        (None: all) -> dict(found, best, stats, T_m_l): rows of the selected queries"""
        torch = self.torch
        Q = self.Q
        mo, p, n = self._t(map_of, torch.int32, (Q,)), self._t(points, torch.float64), self._t(n_points, torch.int32, (Q,))
        if p.dim() != 3 or p.shape[0] != Q or p.shape[2] != 3 or p.shape[1] < 1:
            raise ValueError("points must be [Q, stride, 3]")
        t0, tab, m = self._t(T0, torch.float64, (Q, 12)), self._t(table, torch.float64), self._mask(mask)
        if tab.dim() != 2 or tab.shape[1] != 2:
            raise ValueError("table must be [n_theta, 2]")
        if t0.data_ptr() == self.T_m_l.data_ptr():      # the last match's own output as the prior: the kernels must not read what they write
            t0 = t0.clone()
        self._keep_match = (mo, p, n, t0, tab, m)
        self._chk(self.L.liw_floc_match(self.h, self._ptr(self.store), self._ptr(mo), self._ptr(p), C.c_int(int(p.shape[1])), self._ptr(n), self._ptr(t0),
                                        self._ptr(tab), C.c_int(int(tab.shape[0])), C.c_int(int(W)), C.c_int(int(min_permille)), self._ptr(m),
                                        self._ptr(self.found), self._ptr(self.best), self._ptr(self.stats), self._ptr(self.T_m_l), self._stream()))
        return dict(found=self.found, best=self.best, stats=self.stats, T_m_l=self.T_m_l)

    def link_tf(self, poses, mask=None):
        """poses [Q, 6] IMU poses (p, rotation vector) of the query rows in their own world frames -> dict(T_w_l, T_g_w) [Q, 12]: of the
        rows the last match found (and mask selects), T_w_l = make_tf(p, q) * T_imu_to_laser and T_g_w = T_m_l * inverse(T_w_l), the row
        FleetGroupMap.render takes for that robot; other rows keep their bytes"""
        torch = self.torch
        ps, m = self._t(poses, torch.float64, (self.Q, 6)), self._mask(mask)
        self._keep_link = (ps, m)
        self._chk(self.L.liw_floc_link_tf(self.h, self._ptr(self.T_m_l), self._ptr(ps), C.c_longlong(6), self._ptr(self.found), self._ptr(m),
                                          self._ptr(self.T_w_l), self._ptr(self.T_g_w), self._stream()))
        return dict(T_w_l=self.T_w_l, T_g_w=self.T_g_w)

    angle_table = staticmethod(angle_table)

    def map_regions(self):
        """[M, map_bytes] uint8 view of the map regions"""
        return self.store[:self.M * self.lay["map_bytes"]].view(self.M, self.lay["map_bytes"])

    # ---- inspection (synchronous)
    def field_info(self, m):
        """info dict of the grid the field of map m was built from, with `status` of the build and the `occupied` / `near` counts"""
        self._sync()
        i, st, occ, near = MapInfoC(), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.liw_floc_field_info(self.h, self._ptr(self.store), C.c_int(m), C.byref(i), C.byref(st), C.byref(occ), C.byref(near)))
        return dict(_info_dict(i), status=st.value, occupied=occ.value, near=near.value)

    def field(self, m):
        """the field of map m, uint8 [height][width] (0 x 0 unless its status is FIELD_OK)"""
        i = self.field_info(m)
        h, w = (i["height"], i["width"]) if i["status"] == FIELD_OK else (0, 0)
        out = np.zeros(max(h * w, 1), dtype=np.uint8)
        self._chk(self.L.liw_floc_get_field(self.h, self._ptr(self.store), C.c_int(m), out.ctypes.data_as(C.POINTER(C.c_ubyte)), C.c_longlong(h * w)))
        return out[:h * w].reshape(h, w)

    def device_field(self, m):
        return self.L.liw_floc_device_field(self.h, self._ptr(self.store), C.c_int(m))
