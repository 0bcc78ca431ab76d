"""The edge gate of the group pose graph (C ABI include/liw_group_gate.h): inconsistent cross edges are retired on the device, one per
call and group, from what the group's last solve left behind.  The calls take the handle and the store of a
`group_graph.FleetGroupGraph`, whose gate(), solve_gated() and edge_states() are the public face; this module holds the prototypes.
There is no CPU fallback."""
import ctypes as C

import numpy as np

from ._fleet import _pd, _pi

# every symbol include/liw_group_gate.h declares (checked by tests/test_group_gate_abi.py)
EXPORTS = ["liw_ggate_gate", "liw_ggate_get"]


def _lib():
    from .group_graph import _lib as graph_lib
    L = graph_lib()
    if not getattr(L, "_ggate_ready", False):
        vp, ip, dp, ci = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int
        L.liw_ggate_gate.argtypes = [vp, vp, vp, C.c_double, ci, vp, vp]
        L.liw_ggate_get.argtypes = [vp, vp, ci, ci, ip, dp, ip]
        L._ggate_ready = True
    return L


def gate(L, h, store, gsel, chi2_max, min_support, changed, stream):
    """liw_ggate_gate on device pointers (ctypes c_void_p); -> its return code"""
    return L.liw_ggate_gate(h, store, gsel, C.c_double(float(chi2_max)), C.c_int(int(min_support)), changed, stream)


def get(L, h, store, group):
    """-> the return code (< 0) or dict(state [n] int32, chi2 [n], rejected, gated_solves) over the held edges; synchronous"""
    n = L.liw_ggate_get(h, store, C.c_int(group), C.c_int(0), None, None, None)
    if n < 0:
        return n
    s, c, k = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1)), np.zeros(2, dtype=np.int32)
    r = L.liw_ggate_get(h, store, C.c_int(group), C.c_int(n), _pi(s), _pd(c), _pi(k))
    if r < 0:
        return r
    return dict(state=s[:n], chi2=c[:n], rejected=int(k[0]), gated_solves=int(k[1]))
