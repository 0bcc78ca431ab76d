"""Laser loop-closure detection over the C ABI of include/liw_loop.h: `LoopDetector` holds the key frames' sub-map features
(host de-duplication, device descriptors) and runs laser_loop_detect for the newest key frame on the device (reference
src/trajectory/keyframe_manager.cpp:642-712, :898-1184).  `office_loop_params` are the values of config/office.yaml:98-108."""
import ctypes as C

import numpy as np

LOOP_EXPORTS = ["liw_loop_store_bytes", "liw_loop_sizes", "liw_loop_create", "liw_loop_destroy", "liw_loop_last_error", "liw_loop_num_keyframes",
                "liw_loop_add_keyframe", "liw_loop_detect", "liw_loop_last_stats", "liw_loop_match", "liw_loop_get_points", "liw_loop_get_row",
                "liw_loop_status", "liw_loop_icp"]

ACCEPTED, GATE_NULL, GATE_POINTS, GATE_DIS, GATE_SIZE = 0, 1, 2, 3, 4
NULL, VALID, OVER_CAP, DIJ_OVERFLOW = 0, 1, 2, 3


class LoopParamsC(C.Structure):
    _fields_ = [("a_res", C.c_double), ("d_res", C.c_double), ("submap_count", C.c_int), ("min_match_threshold", C.c_int),
                ("min_interval", C.c_int), ("max_dis", C.c_double), ("max_tf_p", C.c_double), ("max_tf_q", C.c_double),
                ("seed", C.c_ulonglong)]


class LoopDimsC(C.Structure):
    _fields_ = [("max_keyframes", C.c_int), ("max_points", C.c_int)]


class LoopEdgeC(C.Structure):
    _fields_ = [("index1", C.c_int), ("index2", C.c_int), ("size", C.c_int), ("tf12", C.c_double * 12)]


class LoopMatchInfoC(C.Structure):
    _fields_ = [("size", C.c_int), ("draw", C.c_int), ("row", C.c_int), ("bin", C.c_int), ("query_row", C.c_int), ("gate", C.c_int),
                ("tasks", C.c_int), ("quick_pass", C.c_int)]


class LoopStatsC(C.Structure):
    _fields_ = [("candidates", C.c_int), ("launched", C.c_int), ("tasks", C.c_longlong), ("quick_pass", C.c_longlong), ("accepted", C.c_int),
                ("icp_checked", C.c_int)]


def office_loop_params(seed=0):
    """config/office.yaml:98-108"""
    return dict(a_res=0.03, d_res=0.03, submap_count=30, min_match_threshold=5, min_interval=100, max_dis=1.0, max_tf_p=1.0, max_tf_q=0.5,
                seed=seed)


def params_struct(p):
    s = LoopParamsC()
    for k in ("a_res", "d_res", "max_dis", "max_tf_p", "max_tf_q"):
        setattr(s, k, float(p[k]))
    for k in ("submap_count", "min_match_threshold", "min_interval"):
        setattr(s, k, int(p[k]))
    s.seed = int(p.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
    return s


def dims_struct(d):
    return LoopDimsC(int(d["max_keyframes"]), int(d["max_points"]))


def _lib():
    from . import lib
    L = lib()
    if not getattr(L, "_loop_typed", False):
        L.liw_loop_create.restype = C.c_void_p
        L.liw_loop_create.argtypes = [C.c_void_p, C.POINTER(LoopParamsC), C.POINTER(LoopDimsC)]
        L.liw_loop_destroy.argtypes = [C.c_void_p]
        L.liw_loop_last_error.restype = C.c_char_p
        L.liw_loop_last_error.argtypes = [C.c_void_p]
        for name in ("liw_loop_num_keyframes", "liw_loop_add_keyframe", "liw_loop_detect", "liw_loop_last_stats", "liw_loop_match",
                     "liw_loop_get_points", "liw_loop_get_row", "liw_loop_status"):
            getattr(L, name).restype = C.c_int
        L._loop_typed = True
    return L


def store_bytes(params, dims):
    """bytes of the device store; raises ValueError on bad params / dims (host-only)"""
    n = C.c_size_t(0)
    r = _lib().liw_loop_store_bytes(C.byref(params_struct(params)), C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise ValueError("liw_loop_store_bytes: %d" % r)
    return n.value


def sizes(params):
    """(quick_des words W, nAngle)"""
    w, na = C.c_int(0), C.c_int(0)
    if _lib().liw_loop_sizes(C.byref(params_struct(params)), C.byref(w), C.byref(na)):
        raise ValueError("bad loop params")
    return w.value, na.value


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def icp(p1, p2):
    """closed-form planar ICP: T (4x4) with p1 ~ T p2 (host-only)"""
    a = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
    T = np.zeros(12)
    r = _lib().liw_loop_icp(C.c_int(a.shape[0]), _pd(a), _pd(b), _pd(T))
    if r:
        raise ValueError("liw_loop_icp: %d" % r)
    return tf12_to_mat(T)


def tf12_to_mat(T):
    M = np.eye(4)
    M[:3, :3] = np.asarray(T[:9]).reshape(3, 3)
    M[:3, 3] = T[9:12]
    return M


def mat_to_tf12(M):
    M = np.asarray(M, dtype=np.float64)
    return np.concatenate([M[:3, :3].reshape(9), M[:3, 3]])


class LoopDetector:
    """One detector on its own liw_ctx (device and T_imu_to_wheel come from `prm`).  Poses are 4x4 world <- IMU matrices or
    T12 arrays; corners [k][3] in the world frame."""

    def __init__(self, prm, params, dims, device=0):
        from . import params_struct as liw_params_struct, LiwError
        self.L, self.LiwError = _lib(), LiwError
        self.params, self.dims = dict(params), dict(dims)
        self._ps = liw_params_struct(prm, device)
        self.ctx = C.c_void_p(self.L.liw_create(C.byref(self._ps)))
        self.h = C.c_void_p(self.L.liw_loop_create(self.ctx, C.byref(params_struct(params)), C.byref(dims_struct(dims))))
        if not self.h:
            raise ValueError("liw_loop_create: bad params or dims")
        self.W, self.n_angle = sizes(params)
        M = np.zeros(16)
        self.L.liw_get_extrinsics(self.ctx, _pd(M), None)
        self.T_imu_to_wheel = M.reshape(4, 4)

    def _chk(self, r):
        if r < 0:
            raise self.LiwError(r, self.L.liw_loop_last_error(self.h).decode())
        return r

    def add_keyframe(self, pose, corners=None, is_laser=True):
        T = np.asarray(pose, dtype=np.float64)
        tf = np.ascontiguousarray(mat_to_tf12(T) if T.shape == (4, 4) else T.reshape(12))
        c = np.ascontiguousarray(np.zeros((0, 3)) if corners is None else corners, dtype=np.float64).reshape(-1, 3)
        return self._chk(self.L.liw_loop_add_keyframe(self.h, C.c_int(int(bool(is_laser))), _pd(tf), C.c_int(c.shape[0]), _pd(c)))

    def detect(self):
        """None or dict(index1, index2, size, tf12 (4x4))"""
        e = LoopEdgeC()
        if not self._chk(self.L.liw_loop_detect(self.h, C.byref(e))):
            return None
        return dict(index1=e.index1, index2=e.index2, size=e.size, tf12=tf12_to_mat(list(e.tf12)))

    def last_stats(self):
        s = LoopStatsC()
        self._chk(self.L.liw_loop_last_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LoopStatsC._fields_}

    def match(self, query, candidate, cap=4096):
        p1, p2, info = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), LoopMatchInfoC()
        n = self._chk(self.L.liw_loop_match(self.h, C.c_int(query), C.c_int(candidate), C.c_int(cap), _pi(p1), _pi(p2), C.byref(info)))
        d = {k: getattr(info, k) for k, _ in LoopMatchInfoC._fields_}
        d["p1"], d["p2"] = p1[:n].copy(), p2[:n].copy()
        return d

    def num_keyframes(self):
        return self._chk(self.L.liw_loop_num_keyframes(self.h))

    def get_points(self, k):
        n = self._chk(self.L.liw_loop_get_points(self.h, C.c_int(k), C.c_int(0), None))
        out = np.zeros((max(n, 1), 3))
        self._chk(self.L.liw_loop_get_points(self.h, C.c_int(k), C.c_int(n), _pd(out)))
        return out[:n]

    def get_row(self, k, i):
        cap = int(self.dims["max_points"])
        dij, j, aij = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap)
        q = np.zeros(self.W, dtype=np.uint64)
        m = self._chk(self.L.liw_loop_get_row(self.h, C.c_int(k), C.c_int(i), C.c_int(cap), _pi(dij), _pi(j), _pd(aij),
                                              q.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return dict(dij=dij[:m].copy(), j=j[:m].copy(), aij=aij[:m].copy(), quick=q)

    def status(self, k):
        n, o = C.c_int(0), np.zeros(12)
        st = self._chk(self.L.liw_loop_status(self.h, C.c_int(k), C.byref(n), _pd(o)))
        return dict(state=st, n_points=n.value, origin=tf12_to_mat(o))

    def __del__(self):
        try:
            if self.h:
                self.L.liw_loop_destroy(self.h)
            if self.ctx:
                self.L.liw_destroy(self.ctx)
        except Exception:
            pass
