"""Occupancy-grid map of the back-end's laser key frames over the C ABI of include/liw_map.h: `GridMap` keeps every key
frame's laser-frame points on the device and renders the reference's 5 cm nav_msgs/OccupancyGrid from the current poses
(reference src/trajectory/keyframe_manager.cpp:483-511, src/utilies/visualization.cpp:33-75 and :369-451)."""
import ctypes as C

import numpy as np

MAP_EXPORTS = ["liw_map_store_bytes", "liw_map_create", "liw_map_destroy", "liw_map_last_error", "liw_map_add_submap", "liw_map_num_submaps",
               "liw_map_clear", "liw_map_render_tf", "liw_map_render", "liw_map_last_info", "liw_map_get", "liw_map_device_data",
               "liw_map_probe_counts", "liw_map_step_table", "liw_map_write_pgm", "liw_map_write_pgm_grid"]

UNKNOWN, FREE, HIT_ONCE, HIT_MORE = -1, 0, 50, 100
DEFAULT_PALETTE = (205, 254, 0, 0)


class MapParamsC(C.Structure):
    _fields_ = [("resolution", C.c_double)]


class MapDimsC(C.Structure):
    _fields_ = [("max_submaps", C.c_int), ("max_points", C.c_longlong), ("max_cells", C.c_longlong)]


class MapInfoC(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("resolution", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double),
                ("rays", C.c_longlong), ("samples", C.c_longlong), ("unknown", C.c_longlong), ("free_cells", C.c_longlong),
                ("hit_once", C.c_longlong), ("hit_more", C.c_longlong)]


def office_map_params():
    """visualization.cpp:389"""
    return dict(resolution=0.05)


def params_struct(p):
    return MapParamsC(float(p["resolution"]))


def dims_struct(d):
    return MapDimsC(int(d["max_submaps"]), int(d["max_points"]), int(d["max_cells"]))


def _info_dict(i):
    return {k: getattr(i, k) for k, _ in MapInfoC._fields_}


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_map_typed", False):
        L.liw_map_create.restype = C.c_void_p
        L.liw_map_create.argtypes = [C.c_void_p, C.POINTER(MapParamsC), C.POINTER(MapDimsC)]
        L.liw_map_destroy.argtypes = [C.c_void_p]
        L.liw_map_last_error.restype = C.c_char_p
        L.liw_map_last_error.argtypes = [C.c_void_p]
        L.liw_map_add_submap.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.liw_map_num_submaps.argtypes = [C.c_void_p]
        L.liw_map_clear.argtypes = [C.c_void_p]
        L.liw_map_render_tf.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(MapInfoC)]
        L.liw_map_render.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(MapInfoC)]
        L.liw_map_last_info.argtypes = [C.c_void_p, C.POINTER(MapInfoC)]
        L.liw_map_get.restype = C.c_longlong
        L.liw_map_get.argtypes = [C.c_void_p, C.POINTER(C.c_byte), C.c_longlong]
        L.liw_map_device_data.restype = C.c_void_p
        L.liw_map_device_data.argtypes = [C.c_void_p]
        L.liw_map_probe_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.liw_map_step_table.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_double)]
        L.liw_map_write_pgm.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_ubyte)]
        L.liw_map_write_pgm_grid.argtypes = [C.c_char_p, C.POINTER(C.c_byte), C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                             C.POINTER(C.c_ubyte)]
        for name in MAP_EXPORTS:
            if name not in ("liw_map_create", "liw_map_destroy", "liw_map_last_error", "liw_map_get", "liw_map_device_data"):
                getattr(L, name).restype = C.c_int
        L._map_typed = True
    return L


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _palette(palette):
    return None if palette is None else (C.c_ubyte * 4)(*[int(v) for v in palette])


def store_bytes(params, dims):
    """bytes of the device store; raises ValueError on bad params / dims (host-only)"""
    n = C.c_size_t(0)
    r = _lib().liw_map_store_bytes(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise ValueError("liw_map_store_bytes: %d" % r)
    return n.value


def step_table(resolution, n):
    """T[0 .. n): the accumulated tr values of the reference's `for (tr = 0; tr <= len; tr += res / 2)` (host-only)"""
    T = np.zeros(max(int(n), 1))
    r = _lib().liw_map_step_table(float(resolution), int(n), _pd(T))
    if r:
        raise ValueError("liw_map_step_table: %d" % r)
    return T[:int(n)]


def write_pgm_grid(path_stem, grid, resolution, origin_x, origin_y, palette=None):
    """stem.pgm + stem.yaml of a [height][width] int8 array of -1 / 0 / 50 / 100 (host-only)"""
    g = np.ascontiguousarray(grid, dtype=np.int8)
    if g.ndim != 2:
        raise ValueError("grid must be [height][width]")
    r = _lib().liw_map_write_pgm_grid(str(path_stem).encode(), g.ctypes.data_as(C.POINTER(C.c_byte)), g.shape[1], g.shape[0],
                                      float(resolution), float(origin_x), float(origin_y), _palette(palette))
    if r:
        raise ValueError("liw_map_write_pgm_grid: %d" % r)


class GridMap:
    """One map on its own liw_ctx (device and T_imu_to_laser come from `prm`).  Sub-maps are [n][3] laser-frame points."""

    def __init__(self, prm, params=None, dims=None, device=0):
        from . import params_struct as liw_params_struct, LiwError
        self.L, self.LiwError = _lib(), LiwError
        self.params = dict(office_map_params() if params is None else params)
        self.dims = dict(dict(max_submaps=4096, max_points=1 << 22, max_cells=1 << 24) if dims is None else dims)
        self._ps = liw_params_struct(prm, device)
        self.ctx = C.c_void_p(self.L.liw_create(C.byref(self._ps)))
        self.h = C.c_void_p(self.L.liw_map_create(self.ctx, C.byref(params_struct(self.params)), C.byref(dims_struct(self.dims))))
        if not self.h:
            raise ValueError("liw_map_create: bad params or dims")
        M = np.zeros(16)
        self.L.liw_get_extrinsics(self.ctx, None, _pd(M))
        self.T_imu_to_laser = M.reshape(4, 4)

    def _chk(self, r):
        if r < 0:
            raise self.LiwError(r, self.L.liw_map_last_error(self.h).decode())
        return r

    def add_submap(self, points):
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        return self._chk(self.L.liw_map_add_submap(self.h, p.shape[0], _pd(p)))

    def num_submaps(self):
        return self._chk(self.L.liw_map_num_submaps(self.h))

    def clear(self):
        self._chk(self.L.liw_map_clear(self.h))

    def render_tf(self, T_w_l):
        """T_w_l: [K][12] (R row-major, then t) or [K][4][4]; returns the info dict"""
        T = np.asarray(T_w_l, dtype=np.float64)
        if T.ndim == 3:
            T = np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], axis=1)
        T = np.ascontiguousarray(T.reshape(-1, 12))
        i = MapInfoC()
        self._chk(self.L.liw_map_render_tf(self.h, T.shape[0], _pd(T), C.byref(i)))
        return _info_dict(i)

    def render(self, poses):
        """poses: [K][6] p, q of the IMU (the key frames' corrected poses)"""
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 6))
        i = MapInfoC()
        self._chk(self.L.liw_map_render(self.h, P.shape[0], _pd(P), C.byref(i)))
        return _info_dict(i)

    @property
    def info(self):
        i = MapInfoC()
        self._chk(self.L.liw_map_last_info(self.h, C.byref(i)))
        return _info_dict(i)

    def grid(self):
        """the rendered grid, int8 [height][width]"""
        i = self.info
        out = np.zeros(max(i["width"] * i["height"], 1), dtype=np.int8)
        n = self._chk(self.L.liw_map_get(self.h, out.ctypes.data_as(C.POINTER(C.c_byte)), i["width"] * i["height"]))
        return out[:n].reshape(i["height"], i["width"])

    def device_data(self):
        return self.L.liw_map_device_data(self.h)

    def probe_counts(self):
        a, v, t = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._chk(self.L.liw_map_probe_counts(self.h, C.byref(a), C.byref(v), C.byref(t)))
        return dict(atomics=a.value, visits=v.value, hit_atomics=t.value)

    def write_pgm(self, path_stem, palette=None):
        self._chk(self.L.liw_map_write_pgm(self.h, str(path_stem).encode(), _palette(palette)))

    def __del__(self):
        try:
            if self.h:
                self.L.liw_map_destroy(self.h)
            if self.ctx:
                self.L.liw_destroy(self.ctx)
        except Exception:
            pass
