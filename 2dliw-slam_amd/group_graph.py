"""The group pose graph of the fleet on the device (C ABI include/liw_group_graph.h): `FleetGroupGraph` sits behind a
`FleetGroupAligner` and a `FleetBackEnd`, keeps every accepted cross edge of a group, lets linked robots go on producing edges, and
refines the aligner's T_g_w from all edges and from the back-end's current corrected poses, one Levenberg-Marquardt solve per group
in a single launch.  `FleetGroupMap.render_all(backend, aligner.group_linked, aligner.T_g_w)` needs no change.  Everything runs on
torch's current stream, with no read-back.  There is no CPU fallback: compute calls raise LiwError(LIW_ENODEV) without a gfx950
device."""
import ctypes as C

import numpy as np

from . import group_gate
from ._fleet import FleetStore, _pd, _pi
from .posegraph import PgParamsC, pg_struct
from .posegraph_batch import SUMMARY_BYTES, summary_rows

# every symbol include/liw_group_graph.h declares (checked by tests/test_group_graph_abi.py)
EXPORTS = ["liw_ggraph_store_bytes", "liw_ggraph_layout", "liw_ggraph_create", "liw_ggraph_destroy", "liw_ggraph_last_error", "liw_ggraph_reset",
           "liw_ggraph_add_edges", "liw_ggraph_partner", "liw_ggraph_solve", "liw_ggraph_set_lds_doubles", "liw_ggraph_get_edges", "liw_ggraph_get_flags",
           "liw_ggraph_get_summary", "liw_ggraph_get_Z"]

FLAGS = ("edges", "edges_full", "members_full", "bad_edge", "solves", "skipped", "nodes", "used")


class GgraphDimsC(C.Structure):
    _fields_ = [("B", C.c_int), ("G", C.c_int), ("max_members", C.c_int), ("max_edges", C.c_int)]


class GgraphLayoutC(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("group_bytes", C.c_size_t), ("work_off", C.c_size_t), ("work_bytes", C.c_size_t),
                ("work_group_bytes", C.c_size_t), ("tri_doubles", C.c_int)]


def dims_struct(d):
    if isinstance(d, GgraphDimsC):
        return d
    return GgraphDimsC(int(d["B"]), int(d["G"]), int(d["max_members"]), int(d["max_edges"]))


def _lib():
    from . import SummaryC, lib
    L = lib()
    if not getattr(L, "_ggraph_ready", False):
        vp, ip, dp, ci = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int
        dd = C.POINTER(GgraphDimsC)
        L.liw_ggraph_store_bytes.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_ggraph_layout.argtypes = [dd, C.POINTER(GgraphLayoutC)]
        L.liw_ggraph_create.restype = vp
        L.liw_ggraph_create.argtypes = [C.POINTER(PgParamsC), dd, ci]
        L.liw_ggraph_destroy.argtypes = [vp]
        L.liw_ggraph_last_error.restype = C.c_char_p
        L.liw_ggraph_last_error.argtypes = [vp]
        L.liw_ggraph_reset.argtypes = [vp, vp, vp, vp]
        L.liw_ggraph_add_edges.argtypes = [vp] * 8
        L.liw_ggraph_partner.argtypes = [vp, vp, vp, ci, vp, vp]
        L.liw_ggraph_solve.argtypes = [vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp, vp, ci, vp, vp]
        L.liw_ggraph_set_lds_doubles.argtypes = [vp, ci]
        L.liw_ggraph_get_edges.argtypes = [vp, vp, ci, ci, ip, dp]
        L.liw_ggraph_get_flags.argtypes = [vp, vp, ci, ip]
        L.liw_ggraph_get_summary.argtypes = [vp, vp, ci, C.POINTER(SummaryC)]
        L.liw_ggraph_get_Z.argtypes = [vp, vp, ci, ci, ip, dp, dp, dp]
        L._ggraph_ready = True
    return L


def layout(dims):
    """dict of liw_ggraph_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = GgraphLayoutC()
    r = _lib().liw_ggraph_layout(C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_ggraph_layout: bad dims")
    return {k: getattr(out, k) for k, _ in GgraphLayoutC._fields_}


def store_bytes(dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_ggraph_store_bytes(C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_ggraph_store_bytes: bad dims")
    return n.value


class FleetGroupGraph(FleetStore):
    """aligner: the FleetGroupAligner whose T_g_w, linked, via and group_of are worked on in place (its anchors, the linked robots that
    no edge linked, are the fixed nodes); backend: the FleetBackEnd whose corrected poses are read in place; max_members: linked robots
    a group's solve can hold; max_edges: cross edges kept per group; groups: G (default: the highest group index + 1); pg: dict as
    posegraph.office_pg_params (default: the back-end's), of which the loop sigmas are used; max_iters (<= 0: 50) is the default of
    solve().  chi2_max (None: no gate), min_support and gate_rounds are the edge gate's (include/liw_group_gate.h): with chi2_max set,
    push() follows its solve with gate_rounds rounds of gate and re-solve.  Owns the store (a torch uint8 tensor, with `guard` bytes of
    0xA5 on either side for tests) and the outputs partner [B] int32, gsel [G] uint8, changed [G] uint8, summary [G, 32] uint8
    (liw_summary rows; summaries() decodes them): views valid until the next call."""

    _destroy, _last_error = "liw_ggraph_destroy", "liw_ggraph_last_error"

    def __init__(self, aligner, backend, max_members, max_edges, groups=None, pg=None, guard=0, max_iters=0, chi2_max=None, min_support=2, gate_rounds=2):
        from . import LiwError
        torch = aligner.torch
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.al, self.fb, self.dev, self.B = aligner, backend, aligner.dev, aligner.B
        if backend.B != self.B:
            raise ValueError("the aligner has %d robots, the back-end %d" % (self.B, backend.B))
        go = np.asarray(aligner.group_of.cpu())
        G = int(max(int(go.max()) + 1, 1)) if groups is None else int(groups)
        if int(go.max()) >= G:
            raise ValueError("group_of names group %d, there are %d groups" % (int(go.max()), G))
        self.G = G
        self.dims = dict(B=self.B, G=G, max_members=int(max_members), max_edges=int(max_edges))
        self.lay = layout(self.dims)
        self.max_iters = int(max_iters)
        self.chi2_max, self.min_support, self.gate_rounds = (None if chi2_max is None else float(chi2_max)), int(min_support), int(gate_rounds)
        self.Lg = group_gate._lib()
        self._pgs = pg_struct(dict(backend.pg if pg is None else pg))
        index = self.dev.index if self.dev.index is not None else 0
        self.h = C.c_void_p(self.L.liw_ggraph_create(C.byref(self._pgs), C.byref(dims_struct(self.dims)), C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_ggraph_create: bad params or dims")
        self._alloc_store(guard)
        self.partner = torch.full((self.B,), -1, dtype=torch.int32, device=self.dev)
        self.gsel = torch.zeros(G, dtype=torch.uint8, device=self.dev)
        self.summary = torch.zeros(G, SUMMARY_BYTES, dtype=torch.uint8, device=self.dev)
        self._changed = [torch.zeros(G, dtype=torch.uint8, device=self.dev) for _ in range(2)]   # a gate reads one and writes the other
        self.changed, self._ci = self._changed[0], 0
        self._group_index = aligner.group_of.clamp(min=0).long()
        self.round = 0
        self.reset()

    def set_lds_doubles(self, doubles):
        """test hook: triangles of more than `doubles` entries run from the work area (0: all of them; default 8192)"""
        self._chk(self.L.liw_ggraph_set_lds_doubles(self.h, C.c_int(int(doubles))))

    def _gmask(self, m):
        return None if m is None else self._t(m, self.torch.uint8, (self.G,))

    def reset(self, gmask=None):
        m = self._gmask(gmask)
        self._chk(self.L.liw_ggraph_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def group_regions(self):
        """[G, group_bytes] uint8 view of the store's group regions (the work area behind them is not part of it)"""
        return self.store[:self.G * self.lay["group_bytes"]].view(self.G, self.lay["group_bytes"])

    def edge_counts(self):
        """[G] int32: the edges every group holds, a copy made on the device (a clone: with one group the slice is contiguous as it is)"""
        return self.group_regions()[:, :4].clone().view(self.torch.int32).view(self.G)

    def choose_partners(self, round=None):
        """-> partner [B] int32: for a robot of a group the (round mod n)-th of the n OTHER linked members of its group, -1 when there is
        none; for an unlinked robot this is FleetGroupAligner.choose_partners"""
        a = self.al
        r = self.round if round is None else int(round)
        self._chk(self.L.liw_ggraph_partner(self.h, self._ptr(a.group_of), self._ptr(a.linked), C.c_int(r), self._ptr(self.partner), self._stream()))
        return self.partner

    def add_edges(self, cross_out, mask=None):
        """the found, edge [B, 4], tf12 of one FleetGroupAligner.detect_cross call are appended to their groups' lists"""
        torch, B = self.torch, self.B
        f, e, t = self._t(cross_out["found"], torch.uint8, (B,)), self._t(cross_out["edge"], torch.int32, (B, 4)), self._t(cross_out["tf12"], torch.float64, (B, 12))
        m = self._mask(mask)
        self._keep_add = (f, e, t, m)   # the kernel reads them after this call has returned
        self._chk(self.L.liw_ggraph_add_edges(self.h, self._ptr(self.store), self._ptr(self.al.group_of), self._ptr(f), self._ptr(e), self._ptr(t), self._ptr(m),
                                              self._stream()))

    def fixed(self):
        """[B] uint8 on the device: the anchors, the linked robots that no edge linked (via is -1)"""
        a = self.al
        return ((a.linked != 0) & (a.via[:, 0] < 0)).to(self.torch.uint8)

    def n_keyframes(self):
        """[B] int32 on the device: the key frames every robot of the back-end holds (word 0 of its region)"""
        return self.fb.robot_regions()[:, :4].contiguous().view(self.torch.int32).view(self.B)

    def solve(self, gsel=None, max_iters=None, fixed=None, n_keyframes=None):
        """refines aligner.T_g_w of the groups in gsel [G] uint8 (default: all) from the held edges and backend.poses() in place ->
        summary [G, 32] uint8; rows of groups that were not solved keep what they held"""
        torch, a, fb = self.torch, self.al, self.fb
        gs = torch.ones(self.G, dtype=torch.uint8, device=self.dev) if gsel is None else self._gmask(gsel)
        fx = self.fixed() if fixed is None else self._t(fixed, torch.uint8, (self.B,))
        nk = self.n_keyframes() if n_keyframes is None else self._t(n_keyframes, torch.int32, (self.B,))
        mi = self.max_iters if max_iters is None else int(max_iters)
        self._keep_solve = (gs, fx, nk)
        poses = C.c_void_p(fb.store.data_ptr() + fb.pose_offset())
        self._chk(self.L.liw_ggraph_solve(self.h, self._ptr(self.store), poses, C.c_longlong(fb.lay["robot_bytes"] // 8), self._ptr(nk), self._ptr(a.group_of),
                                          self._ptr(a.linked), self._ptr(fx), self._ptr(a.T_g_w), self._ptr(gs), C.c_int(mi), self._ptr(self.summary),
                                          self._stream()))
        return self.summary

    def gate(self, gsel=None, chi2_max=None, min_support=None):
        """one gate step (liw_ggate_gate) on the groups in gsel [G] uint8 (default: all), on what their last solve left: the used edge
        with the largest squared residual above chi2_max whose robot pair holds at least min_support other used edges is retired
        (defaults: the constructor's) -> changed [G] uint8, 1 where an edge was retired: the gsel of the next solve"""
        torch = self.torch
        c2 = self.chi2_max if chi2_max is None else float(chi2_max)
        if c2 is None:
            raise ValueError("gate() needs chi2_max, here or in the constructor")
        ms = self.min_support if min_support is None else int(min_support)
        gs = torch.ones(self.G, dtype=torch.uint8, device=self.dev) if gsel is None else self._gmask(gsel)
        self._ci ^= 1                                 # the two outputs take turns, so that one gate's changed can be the next one's gsel
        if gs.data_ptr() == self._changed[self._ci].data_ptr():
            self._ci ^= 1
        out = self._changed[self._ci]
        self._keep_gate = gs
        self._chk(group_gate.gate(self.Lg, self.h, self._ptr(self.store), self._ptr(gs), c2, ms, self._ptr(out), self._stream()))
        self.changed = out
        return out

    def solve_gated(self, gsel=None, max_iters=None, fixed=None, n_keyframes=None):
        """solve(gsel), then gate_rounds times: changed = gate(the groups just solved); solve(changed).  Everything is enqueued, nothing is
        read back; a group whose edges are consistent costs one gate and launches that return at once.  -> summary"""
        self.solve(gsel, max_iters, fixed, n_keyframes)
        current = gsel
        for _ in range(self.gate_rounds):
            current = self.gate(current)
            self.solve(current, max_iters, fixed, n_keyframes)
        return self.summary

    def push(self, loop_out, back_out=None, mask=None):
        """behind FleetLoopDetector.push and FleetBackEnd.push: partner choice of this round (linked robots included), cross detection for
        the robots whose key frame was stored, link for the still unlinked robots, the edges appended, and a solve of the groups that gained
        an edge in this call or have a linked member in back_out["due"] (solve_gated when chi2_max is set).  That group set is computed
        on the device; nothing is read back.
        -> the views of detect_cross and link, partner, gsel and summary"""
        torch, a = self.torch, self.al
        key = loop_out["added"]
        if mask is not None:
            key = key * self._mask(mask)
        partner = self.choose_partners()
        self.round += 1
        out = a.detect_cross(key, partner)
        out.update(a.link(partner=partner))
        before = self.edge_counts()
        self.add_edges(out, mask=mask)
        gsel = (self.edge_counts() != before).to(torch.uint8)
        if back_out is not None and back_out.get("due") is not None:
            member = ((self._t(back_out["due"], torch.uint8, (self.B,)) != 0) & (a.linked != 0) & (a.group_of >= 0)).to(torch.uint8)
            gsel = torch.maximum(gsel, torch.zeros_like(gsel).scatter_reduce(0, self._group_index, member, "amax"))
        self.gsel = gsel
        if self.chi2_max is None:
            self.solve(gsel)
        else:
            self.solve_gated(gsel)
        out.update(partner=partner, gsel=gsel, summary=self.summary)
        return out

    # ---- inspection (synchronous)
    def summaries(self):
        self._sync()
        return summary_rows(self.summary.cpu().numpy())

    def flags(self, group):
        """dict(edges, edges_full, members_full, bad_edge, solves, and of the last solve skipped, nodes, used)"""
        self._sync()
        f = np.zeros(8, dtype=np.int32)
        self._chk(self.L.liw_ggraph_get_flags(self.h, self._ptr(self.store), C.c_int(group), _pi(f)))
        return {k: int(v) for k, v in zip(FLAGS, f)}

    def edges(self, group):
        """idx [n, 5] int32 (a, q, b, i, size), tf12 [n, 12]"""
        self._sync()
        n = self._chk(self.L.liw_ggraph_get_edges(self.h, self._ptr(self.store), C.c_int(group), C.c_int(0), None, None))
        i, t = np.zeros((max(n, 1), 5), dtype=np.int32), np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_ggraph_get_edges(self.h, self._ptr(self.store), C.c_int(group), C.c_int(n), _pi(i), _pd(t)))
        return i[:n], t[:n]

    def edge_states(self, group):
        """dict(state [n] int32 (0 active, 1 rejected), chi2 [n] (of the last gate that saw the edge in a solve), rejected, gated_solves)"""
        self._sync()
        out = group_gate.get(self.Lg, self.h, self._ptr(self.store), group)
        return out if isinstance(out, dict) else self._chk(out)

    def last_summary(self, group):
        from . import SummaryC
        self._sync()
        sm = SummaryC()
        self._chk(self.L.liw_ggraph_get_summary(self.h, self._ptr(self.store), C.c_int(group), C.byref(sm)))
        return dict(iterations=sm.iterations, successful=sm.successful_steps, termination=sm.termination, initial_cost=sm.initial_cost,
                    final_cost=sm.final_cost)

    def get_Z(self, group):
        """of the group's last solve -> dict(used [n] int32, Z, Ta, Tb [n, 12]) over the held edges"""
        self._sync()
        n = self._chk(self.L.liw_ggraph_get_Z(self.h, self._ptr(self.store), C.c_int(group), C.c_int(0), None, None, None, None))
        u, z, ta, tb = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 12)), np.zeros((max(n, 1), 12)), np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_ggraph_get_Z(self.h, self._ptr(self.store), C.c_int(group), C.c_int(n), _pi(u), _pd(z), _pd(ta), _pd(tb)))
        return dict(used=u[:n], Z=z[:n], Ta=ta[:n], Tb=tb[:n])
