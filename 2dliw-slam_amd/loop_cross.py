"""Inter-robot loop closure and group alignment of the fleet on the device (C ABI include/liw_loop_cross.h): `FleetGroupAligner`
sits behind `FleetLoopDetector.push`, matches the newest key frame of every unlinked robot against the candidate slots of a linked
robot of its group, and chains the accepted edges into T_g_w [B, 12] (robot world -> group frame), which together with
`group_linked` is what `FleetGroupMap.render_all(backend, aligner.group_linked, aligner.T_g_w)` takes: an unlinked robot is in no
group.  Everything runs on torch's current stream, with no read-back.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from .loop import mat_to_tf12

# every symbol include/liw_loop_cross.h declares (checked by tests/test_loop_cross_abi.py)
XLOOP_EXPORTS = ["liw_xloop_detect", "liw_xloop_partner", "liw_xloop_link", "liw_xloop_get_pair"]


class XloopParamsC(C.Structure):
    _fields_ = [("min_match", C.c_int), ("max_rms", C.c_double)]


def _lib():
    from .loop_batch import _lib as floop_lib
    L = floop_lib()
    if not getattr(L, "_xloop_ready", False):
        vp, ip = C.c_void_p, C.POINTER(C.c_int)
        L.liw_xloop_detect.argtypes = [vp, vp, vp, vp, C.POINTER(XloopParamsC)] + [vp] * 8
        L.liw_xloop_partner.argtypes = [vp, vp, vp, C.c_int, vp, vp]
        L.liw_xloop_link.argtypes = [vp] * 11
        L.liw_xloop_get_pair.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, ip]
        L._xloop_ready = True
    return L


class FleetGroupAligner:
    """detector: the FleetLoopDetector whose store is read; group_of [B] int32 (negative: in no group); anchors: robots that start
    linked, an iterable (identity) or a dict robot -> 4x4 / T12 (group <- robot world); a candidate is accepted when its size is
    above min_match (>= the detector's min_match_threshold) and its planar residual is not above max_rms (metres).  Owns linked [B]
    uint8, T_g_w [B, 12], via [B, 4] int32 (source robot, own key frame, source key frame, size; -1 until linked), group_linked
    [B] int32, partner [B] int32, the cross outputs found, edge [B, 4], tf12, T_w1_w2 [B, 12], rms [B], stats [B, 6] and a round
    counter: device tensors, views valid until the next call."""

    def __init__(self, detector, group_of, anchors, min_match, max_rms):
        torch = detector.torch
        self.torch, self.det, self.L, self.B, self.dev = torch, detector, _lib(), detector.B, detector.dev
        self.params = XloopParamsC(int(min_match), float(max_rms))
        B = self.B
        self.group_of = detector._t(group_of, torch.int32, (B,))
        linked, T = np.zeros(B, np.uint8), np.tile(mat_to_tf12(np.eye(4)), (B, 1))
        items = anchors.items() if hasattr(anchors, "items") else [(a, None) for a in anchors]
        for a, M in items:
            a = int(a)
            if not 0 <= a < B:
                raise ValueError("anchor %d is outside 0 .. B-1" % a)
            linked[a] = 1
            if M is not None:
                M = np.asarray(M, dtype=np.float64)
                T[a] = mat_to_tf12(M) if M.shape == (4, 4) else M.reshape(12)
        go = np.asarray(self.group_of.cpu())
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        self.linked, self.T_g_w = detector._t(linked, torch.uint8, (B,)), detector._t(T, torch.float64, (B, 12))
        self.group_linked = detector._t(np.where(linked != 0, go, -1), torch.int32, (B,))
        self.via, self.partner = torch.full((B, 4), -1, dtype=torch.int32, device=self.dev), torch.full((B,), -1, dtype=torch.int32, device=self.dev)
        self.found, self.edge, self.stats = z(B, dt=torch.uint8), z(B, 4, dt=torch.int32), z(B, 6, dt=torch.int64)
        self.tf12, self.T_w1_w2, self.rms = z(B, 12, dt=torch.float64), z(B, 12, dt=torch.float64), z(B, dt=torch.float64)
        self.round = 0

    def _chk(self, r):
        return self.det._chk(r)

    def choose_partners(self, round=None):
        """-> partner [B] int32: for an unlinked robot the (round mod n)-th of the n linked members of its group, else -1"""
        d = self.det
        r = self.round if round is None else int(round)
        self._chk(self.L.liw_xloop_partner(d.h, d._ptr(self.group_of), d._ptr(self.linked), C.c_int(r), d._ptr(self.partner), d._stream()))
        return self.partner

    def detect_cross(self, key, partner, mask=None):
        """key [B] uint8, partner [B] int32 -> dict(found, edge [B, 4] (q, partner, i, size), tf12, T_w1_w2, rms, stats)"""
        d, torch = self.det, self.torch
        k, p, m = d._t(key, torch.uint8, (self.B,)), d._t(partner, torch.int32, (self.B,)), d._mask(mask)
        self._keep = (k, p, m)   # the kernels read them after this call has returned
        self._chk(self.L.liw_xloop_detect(d.h, d._ptr(d.store), d._ptr(k), d._ptr(p), C.byref(self.params), d._ptr(m), d._ptr(self.found),
                                          d._ptr(self.edge), d._ptr(self.tf12), d._ptr(self.T_w1_w2), d._ptr(self.rms), d._ptr(self.stats), d._stream()))
        return dict(found=self.found, edge=self.edge, tf12=self.tf12, T_w1_w2=self.T_w1_w2, rms=self.rms, stats=self.stats)

    def link(self, partner=None, found=None, edge=None, T_w1_w2=None):
        """chains the edges of one detect_cross call (default: the last one's outputs) -> dict(linked, T_g_w, via, group_linked)"""
        d, torch, B = self.det, self.torch, self.B
        p = self.partner if partner is None else d._t(partner, torch.int32, (B,))
        f = self.found if found is None else d._t(found, torch.uint8, (B,))
        e = self.edge if edge is None else d._t(edge, torch.int32, (B, 4))
        T = self.T_w1_w2 if T_w1_w2 is None else d._t(T_w1_w2, torch.float64, (B, 12))
        self._keep_link = (p, f, e, T)
        self._chk(self.L.liw_xloop_link(d.h, d._ptr(self.group_of), d._ptr(p), d._ptr(f), d._ptr(e), d._ptr(T), d._ptr(self.linked),
                                        d._ptr(self.T_g_w), d._ptr(self.via), d._ptr(self.group_linked), d._stream()))
        return dict(linked=self.linked, T_g_w=self.T_g_w, via=self.via, group_linked=self.group_linked)

    def push(self, loop_out, mask=None):
        """behind FleetLoopDetector.push: partner choice of this round, cross detection for the robots whose key frame was stored
        (loop_out["added"]), link.  -> the views of detect_cross and link, and partner"""
        key = loop_out["added"]
        if mask is not None:
            key = key * self.det._mask(mask)
        partner = self.choose_partners()
        self.round += 1
        out = self.detect_cross(key, partner)
        out.update(self.link())
        out["partner"] = partner
        return out

    def get_pair(self, robot, cand):
        """test hook (synchronous): the pair (robot, candidate key frame of its partner) of the last detect_cross ->
        dict(size, draw, row, bin, quick_pass, query_row, n2, p1, p2)"""
        d = self.det
        d._sync()
        cap = d.dims["max_points"]
        info, p1, p2 = np.zeros(8, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        n = self._chk(self.L.liw_xloop_get_pair(d.h, d._ptr(d.store), C.c_int(robot), C.c_int(cand), C.c_int(cap), ip(info), ip(p1), ip(p2)))
        return dict(size=int(info[0]), draw=int(info[1]), row=int(info[2]), bin=int(info[3]), quick_pass=int(info[4]), query_row=int(info[6]),
                    n2=int(info[7]), p1=p1[:n].copy(), p2=p2[:n].copy())
