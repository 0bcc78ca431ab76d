"""The joint pose graph of a group of fleet robots on the device (C ABI include/liw_group_joint.h): `FleetGroupJoint` sits behind a
`FleetGroupGraph` and a `FleetBackEnd` and solves, per group, ONE graph over the key frames of all members: every member's sequential
and own loop edges (read in place from the back-end's store) and the group's held cross edges (read in place from the group graph's
store) as direct edges between key frames, from the start T_g_w * P.  Where the group graph can only move a robot's trajectory as one
rigid body, here a member's drift is corrected by what its team-mates saw.  The result is a pose part of its own, which
`FleetGroupMap.render(joint.poses(), group_linked, T_g_w=None)` draws with no change to the map code; the back-end store, the group
graph's store and T_g_w are only read.  Everything runs on torch's current stream, with no read-back unless check_every > 0.  There
is no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore, _pi
from .posegraph import PgParamsC, pg_struct
from .posegraph_batch import SUMMARY_BYTES, summary_rows

# every symbol include/liw_group_joint.h declares (checked by tests/test_group_joint_abi.py)
EXPORTS = ["liw_gjoint_store_bytes", "liw_gjoint_layout", "liw_gjoint_pose_offset", "liw_gjoint_create", "liw_gjoint_destroy", "liw_gjoint_last_error",
           "liw_gjoint_solve", "liw_gjoint_set_lds_doubles", "liw_gjoint_get_header", "liw_gjoint_get_summary", "liw_gjoint_get_members",
           "liw_gjoint_get_nodes", "liw_gjoint_get_separators"]

FLAGS = ("reserved", "members_full", "nodes_full", "loops_full", "members", "nodes", "seq_edges", "own_loops", "used", "skipped", "separators", "solved",
         "const_node")


class GjointDimsC(C.Structure):
    _fields_ = [("B", C.c_int), ("G", C.c_int), ("max_keyframes", C.c_int), ("max_robot_loops", C.c_int), ("max_edges", C.c_int),
                ("max_members", C.c_int), ("max_nodes", C.c_int), ("max_loops", C.c_int)]


class GjointLayoutC(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("pose_off", C.c_size_t), ("header_off", C.c_size_t), ("work_off", C.c_size_t), ("work_group_bytes", C.c_size_t),
                ("max_separators", C.c_int), ("tri_doubles", C.c_int)]


def dims_struct(d):
    if isinstance(d, GjointDimsC):
        return d
    return GjointDimsC(*(int(d[k]) for k, _ in GjointDimsC._fields_))


def _lib():
    from . import ParamsC, SummaryC, lib
    L = lib()
    if not getattr(L, "_gjoint_ready", False):
        vp, ip, ci = C.c_void_p, C.POINTER(C.c_int), C.c_int
        dd = C.POINTER(GjointDimsC)
        L.liw_gjoint_store_bytes.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_gjoint_layout.argtypes = [dd, C.POINTER(GjointLayoutC)]
        L.liw_gjoint_pose_offset.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_gjoint_create.restype = vp
        L.liw_gjoint_create.argtypes = [C.POINTER(ParamsC), C.POINTER(PgParamsC), dd, ci]
        L.liw_gjoint_destroy.argtypes = [vp]
        L.liw_gjoint_last_error.restype = C.c_char_p
        L.liw_gjoint_last_error.argtypes = [vp]
        L.liw_gjoint_solve.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp]
        L.liw_gjoint_set_lds_doubles.argtypes = [vp, ci]
        L.liw_gjoint_get_header.argtypes = [vp, vp, ci, ip]
        L.liw_gjoint_get_summary.argtypes = [vp, vp, ci, C.POINTER(SummaryC)]
        L.liw_gjoint_get_members.argtypes = [vp, vp, ci, ci, ip, ip]
        L.liw_gjoint_get_nodes.argtypes = [vp, vp, ci, ci, ip, ip]
        L.liw_gjoint_get_separators.argtypes = [vp, vp, ci, ci, ip]
        L._gjoint_ready = True
    return L


def layout(dims):
    """dict of liw_gjoint_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = GjointLayoutC()
    r = _lib().liw_gjoint_layout(C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_gjoint_layout: bad dims")
    return {k: getattr(out, k) for k, _ in GjointLayoutC._fields_}


def store_bytes(dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_gjoint_store_bytes(C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_gjoint_store_bytes: bad dims")
    return n.value


class FleetGroupJoint(FleetStore):
    """graph: the FleetGroupGraph whose held cross edges, aligner (group_of, linked, T_g_w) and anchors are read; backend: the FleetBackEnd
    whose key frames and edges are read in place; max_nodes: key frames of all members of a group; max_loops: own loop edges plus used
    cross edges of a group; max_members: members a solve can hold (default: the graph's); pg: dict as posegraph.office_pg_params (default: the back-end's); max_iters
    (<= 0: 50) is the default of solve().  Owns the store (a torch uint8 tensor, with `guard` bytes of 0xA5 on either side for tests) and
    summary [G, 32] uint8 (liw_summary rows; summaries() decodes them): valid until the next call."""

    _destroy, _last_error = "liw_gjoint_destroy", "liw_gjoint_last_error"

    def __init__(self, graph, backend, max_nodes, max_loops, pg=None, max_iters=0, guard=0, max_members=None):
        from . import LiwError
        torch = graph.torch
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.gr, self.fb, self.al, self.dev, self.B, self.G = graph, backend, graph.al, graph.dev, graph.B, graph.G
        if backend.B != self.B:
            raise ValueError("the group graph has %d robots, the back-end %d" % (self.B, backend.B))
        self.K = backend.dims["max_keyframes"]
        self.dims = dict(B=self.B, G=self.G, max_keyframes=self.K, max_robot_loops=backend.dims["max_loops"], max_edges=graph.dims["max_edges"],
                         max_members=int(graph.dims["max_members"] if max_members is None else max_members), max_nodes=int(max_nodes), max_loops=int(max_loops))
        self.lay = layout(self.dims)
        self.max_iters = int(max_iters)
        self.pg = dict(backend.pg if pg is None else pg)
        self._pgs = pg_struct(self.pg)
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_gjoint_create(C.byref(backend._ps), C.byref(self._pgs), C.byref(dims_struct(self.dims)), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_gjoint_create: bad params or dims")
        self._alloc_store(guard)
        self.summary = torch.zeros(self.G, SUMMARY_BYTES, dtype=torch.uint8, device=self.dev)
        self.gsel = torch.zeros(self.G, dtype=torch.uint8, device=self.dev)

    def set_lds_doubles(self, doubles):
        """test hook: separator triangles of more than `doubles` entries run from the work area (0: all of them; default 8192)"""
        self._chk(self.L.liw_gjoint_set_lds_doubles(self.h, C.c_int(int(doubles))))

    def poses(self):
        """[B, max_keyframes, 6] float64 strided view of the pose part (no copy: it shows what later solves write); FleetGroupMap.render
        and FleetMapper.render take it as it is"""
        o, n = self.lay["pose_off"], self.B * self.K * 48
        return self.store[o:o + n].view(self.torch.float64).view(self.B, self.K, 6)

    def solve(self, gsel=None, fixed=None, check_every=0, max_iters=None):
        """the joint solve of the groups in gsel [G] uint8 (default: every group that holds an edge), anchors fixed [B] uint8 (default:
        graph.fixed()) -> summary [G, 32] uint8; the rows of poses() of every member of a selected group are written"""
        torch, a = self.torch, self.al
        gs = (self.gr.edge_counts() > 0).to(torch.uint8) if gsel is None else self._t(gsel, torch.uint8, (self.G,))
        fx = self.gr.fixed() if fixed is None else self._t(fixed, torch.uint8, (self.B,))
        mi = self.max_iters if max_iters is None else int(max_iters)
        self._keep = (gs, fx)   # the kernels read them after this call has returned
        self.gsel = gs
        self._chk(self.L.liw_gjoint_solve(self.h, self._ptr(self.store), self._ptr(self.fb.store), self._ptr(self.gr.store), self._ptr(a.group_of),
                                          self._ptr(a.linked), self._ptr(fx), self._ptr(a.T_g_w), self._ptr(gs), C.c_int(mi), C.c_int(int(check_every)),
                                          self._ptr(self.summary), self._stream()))
        return self.summary

    def push(self, graph_out):
        """behind FleetGroupGraph.push: the joint solve of the groups that call solved (graph_out["gsel"], a device tensor; nothing is
        read back) -> summary"""
        return self.solve(gsel=graph_out["gsel"])

    # ---- inspection (synchronous)
    def summaries(self):
        self._sync()
        return summary_rows(self.summary.cpu().numpy())

    def flags(self, group):
        """dict of the header words of the group's last solve (FLAGS)"""
        self._sync()
        f = np.zeros(16, dtype=np.int32)
        self._chk(self.L.liw_gjoint_get_header(self.h, self._ptr(self.store), C.c_int(group), _pi(f)))
        return {k: int(v) for k, v in zip(FLAGS, f)}

    def last_summary(self, group):
        from . import SummaryC
        self._sync()
        sm = SummaryC()
        self._chk(self.L.liw_gjoint_get_summary(self.h, self._ptr(self.store), C.c_int(group), C.byref(sm)))
        return dict(iterations=sm.iterations, successful=sm.successful_steps, termination=sm.termination, initial_cost=sm.initial_cost,
                    final_cost=sm.final_cost)

    def members(self, group):
        """(member robots, node offsets) of the group's last solve"""
        self._sync()
        n = self._chk(self.L.liw_gjoint_get_members(self.h, self._ptr(self.store), C.c_int(group), C.c_int(0), None, None))
        r, o = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.liw_gjoint_get_members(self.h, self._ptr(self.store), C.c_int(group), C.c_int(n), _pi(r), _pi(o)))
        return r[:n].tolist(), o[:n].tolist()

    def nodes(self, group):
        """(row [n] = robot * max_keyframes + key frame, sepidx [n]) of the group's last solve"""
        self._sync()
        n = self._chk(self.L.liw_gjoint_get_nodes(self.h, self._ptr(self.store), C.c_int(group), C.c_int(0), None, None))
        r, s = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.liw_gjoint_get_nodes(self.h, self._ptr(self.store), C.c_int(group), C.c_int(n), _pi(r), _pi(s)))
        return r[:n].tolist(), s[:n].tolist()

    def separators(self, group):
        """the separator list (node indices) of the group's last solve"""
        self._sync()
        n = self._chk(self.L.liw_gjoint_get_separators(self.h, self._ptr(self.store), C.c_int(group), C.c_int(0), None))
        s = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.liw_gjoint_get_separators(self.h, self._ptr(self.store), C.c_int(group), C.c_int(n), _pi(s)))
        return s[:n].tolist()

    def header_bytes(self):
        """[G, 256] uint8 view of the group headers"""
        o = self.lay["header_off"]
        return self.store[o:o + 256 * self.G].view(self.G, 256)
