"""The fleet's pose-graph back-end on the device (C ABI include/liw_posegraph_batch.h): `FleetBackEnd` keeps B instances of
keyframe_manager (key-frame queue, sequential and loop edges, solve, map-frame correction) in one store and consumes what
`FleetTrajectory.step` and `FleetLoopDetector.push` return, on torch's current stream and without a host loop over robots.
`posegraph.PoseGraph.solve` (one graph per call, LM bookkeeping on the host) is its parity reference.  There is no CPU fallback:
compute calls raise LiwError(LIW_ENODEV) without a gfx950 device."""
import ctypes as C

import numpy as np

from ._fleet import FleetStore, _pd, _pi
from .posegraph import PgParamsC, pg_struct

# every symbol include/liw_posegraph_batch.h declares (checked by tests/test_posegraph_batch_abi.py)
FPG_EXPORTS = ["liw_fpg_store_bytes", "liw_fpg_layout", "liw_fpg_create", "liw_fpg_destroy", "liw_fpg_last_error", "liw_fpg_reset",
               "liw_fpg_add_keyframes", "liw_fpg_add_loops", "liw_fpg_due", "liw_fpg_solve", "liw_fpg_correct", "liw_fpg_num_keyframes",
               "liw_fpg_flags", "liw_fpg_get_keyframes", "liw_fpg_get_seq_edges", "liw_fpg_get_loop_edges", "liw_fpg_get_modify_delta_tf",
               "liw_fpg_get_summary", "liw_fpg_load_graph", "liw_fpg_set_lds_doubles", "liw_fpg_pose_offset"]

FLAGS = ("loops", "full", "loops_full", "bad_edge", "pending", "solves")
SUMMARY_BYTES = 32   # sizeof(liw_summary)


class FpgDimsC(C.Structure):
    _fields_ = [("B", C.c_int), ("max_keyframes", C.c_int), ("max_loops", C.c_int)]


class FpgLayoutC(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("robot_bytes", C.c_size_t), ("work_off", C.c_size_t), ("work_bytes", C.c_size_t),
                ("work_robot_bytes", C.c_size_t), ("max_separators", C.c_int), ("edge_slots", C.c_int)]


def dims_struct(d):
    if isinstance(d, FpgDimsC):
        return d
    return FpgDimsC(int(d["B"]), int(d["max_keyframes"]), int(d["max_loops"]))


def _lib():
    from . import ParamsC, SummaryC, lib
    L = lib()
    if not getattr(L, "_fpg_ready", False):
        vp, ip, dp, ci = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int
        dd = C.POINTER(FpgDimsC)
        L.liw_fpg_store_bytes.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_fpg_layout.argtypes = [dd, C.POINTER(FpgLayoutC)]
        L.liw_fpg_pose_offset.argtypes = [dd, C.POINTER(C.c_size_t)]
        L.liw_fpg_create.restype = vp
        L.liw_fpg_create.argtypes = [C.POINTER(ParamsC), C.POINTER(PgParamsC), dd, C.c_double, ci]
        L.liw_fpg_destroy.argtypes = [vp]
        L.liw_fpg_last_error.restype = C.c_char_p
        L.liw_fpg_last_error.argtypes = [vp]
        L.liw_fpg_reset.argtypes = [vp, vp, vp, vp]
        L.liw_fpg_add_keyframes.argtypes = [vp] * 8
        L.liw_fpg_add_loops.argtypes = [vp] * 7
        L.liw_fpg_due.argtypes = [vp] * 8
        L.liw_fpg_solve.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp]
        L.liw_fpg_correct.argtypes = [vp] * 6
        L.liw_fpg_num_keyframes.argtypes = [vp, vp, ci]
        L.liw_fpg_flags.argtypes = [vp, vp, ci, ip, dp]
        L.liw_fpg_get_keyframes.argtypes = [vp, vp, ci, ci, dp, dp, dp]
        L.liw_fpg_get_seq_edges.argtypes = [vp, vp, ci, ci, dp]
        L.liw_fpg_get_loop_edges.argtypes = [vp, vp, ci, ci, ip, dp]
        L.liw_fpg_get_modify_delta_tf.argtypes = [vp, vp, ci, dp]
        L.liw_fpg_get_summary.argtypes = [vp, vp, ci, C.POINTER(SummaryC)]
        L.liw_fpg_set_lds_doubles.argtypes = [vp, ci]
        L.liw_fpg_load_graph.argtypes = [vp, vp, ci, ci, dp, dp, dp, ci, ip, dp]
        L._fpg_ready = True
    return L


def layout(dims):
    """dict of liw_fpg_layout_info (host-only); raises LiwError(LIW_EINVAL) on bad dims"""
    from . import LiwError
    out = FpgLayoutC()
    r = _lib().liw_fpg_layout(C.byref(dims_struct(dims)), C.byref(out))
    if r:
        raise LiwError(r, "liw_fpg_layout: bad dims")
    return {k: getattr(out, k) for k, _ in FpgLayoutC._fields_}


def store_bytes(dims):
    """bytes of the store (host-only)"""
    from . import LiwError
    n = C.c_size_t(0)
    r = _lib().liw_fpg_store_bytes(C.byref(dims_struct(dims)), C.byref(n))
    if r:
        raise LiwError(r, "liw_fpg_store_bytes: bad dims")
    return n.value


def summary_rows(raw):
    """[B, 32] uint8 host array of liw_summary rows -> list of dicts as PoseGraph.solve returns"""
    raw = np.ascontiguousarray(raw)
    ints, dbl = raw.view(np.int32).reshape(len(raw), 8), raw.view(np.float64).reshape(len(raw), 4)
    return [dict(iterations=int(i[0]), successful=int(i[1]), termination=int(i[2]), initial_cost=float(d[2]), final_cost=float(d[3]))
            for i, d in zip(ints, dbl)]


class FleetBackEnd(FleetStore):
    """prm: solver parameters (synth.office_params layout; the extrinsics and ground sigmas are used); pg: dict as
    posegraph.office_pg_params; dims: dict(B, max_keyframes, max_loops); solve_period: seconds of key-frame time between two solves of
    a robot; max_iters (<= 0: 50) and check_every are the defaults of solve().  Owns the store (a torch uint8 tensor, with `guard`
    bytes of 0xA5 on either side for tests) and the outputs added [B] uint8, due [B] uint8, n_due [1] int32, summary [B, 32] uint8
    (liw_summary rows; summaries() decodes them), corrected [B, 6]: views valid until the next call.  Every call runs on torch's
    current stream.  Behind a FleetLoopDetector give both the same max_keyframes: push() stores a key frame exactly when the loop
    detector stored it, so the edge indices of its loops are the indices of this queue.
    The occupancy map per robot is map_batch.FleetMapper's, which reads poses() in place.  What stays with the caller: non-laser key
    frames, a C++ mirror of this class."""

    _destroy, _last_error = "liw_fpg_destroy", "liw_fpg_last_error"

    def __init__(self, prm, pg, dims, solve_period=10.0, device="cuda:0", guard=0, max_iters=0, check_every=4):
        import torch
        from . import LiwError, params_struct
        self.torch, self.LiwError, self.L = torch, LiwError, _lib()
        self.pg, self.dims = dict(pg), {k: int(dims[k]) for k in ("B", "max_keyframes", "max_loops")}
        self.B = self.dims["B"]
        self.dev = torch.device(device)
        self.lay = layout(self.dims)
        self.solve_period, self.max_iters, self.check_every = float(solve_period), int(max_iters), int(check_every)
        index = self.dev.index if self.dev.index is not None else 0
        self._ps, self._pgs = params_struct(prm, index), pg_struct(self.pg)
        self.h = C.c_void_p(self.L.liw_fpg_create(C.byref(self._ps), C.byref(self._pgs), C.byref(dims_struct(self.dims)), C.c_double(self.solve_period),
                                                   C.c_int(index)))
        if not self.h:
            raise LiwError(-22, "liw_fpg_create: bad params or dims")
        self._alloc_store(guard)
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        B = self.B
        self.added, self.due_flags, self.n_due = z(B, dt=torch.uint8), z(B, dt=torch.uint8), z(1, dt=torch.int32)
        self.summary, self.corrected = z(B, SUMMARY_BYTES, dt=torch.uint8), z(B, 6, dt=torch.float64)
        self.reset()

    def modify_delta_tf(self):
        """[B, 12] float64 strided view of every robot's modify_delta_tf in the store (no copy: it shows what later solves write)"""
        rb = self.lay["robot_bytes"]
        return self.store[:self.B * rb].view(self.torch.float64).view(self.B, rb // 8)[:, 5:17]

    def pose_offset(self):
        """byte offset of the corrected poses within a robot region (liw_fpg_pose_offset)"""
        off = C.c_size_t(0)
        self._chk(self.L.liw_fpg_pose_offset(C.byref(dims_struct(self.dims)), C.byref(off)))
        return off.value

    def poses(self):
        """[B, max_keyframes, 6] float64 strided view of every robot's corrected poses (p, rotation vector) in the store (no copy: it
        shows what later solves write); robot b holds num_keyframes(b) of them.  map_batch.FleetMapper.render takes it as it is."""
        rb, K = self.lay["robot_bytes"], self.dims["max_keyframes"]
        o = self.pose_offset() // 8
        return self.store[:self.B * rb].view(self.torch.float64).view(self.B, rb // 8)[:, o:o + 6 * K].unflatten(1, (K, 6))

    def set_lds_doubles(self, doubles):
        """test hook: separator systems of more than `doubles` entries run from the work area (0: all of them; default 8192)"""
        self._chk(self.L.liw_fpg_set_lds_doubles(self.h, C.c_int(int(doubles))))

    def reset(self, mask=None):
        m = self._mask(mask)
        self._chk(self.L.liw_fpg_reset(self.h, self._ptr(self.store), self._ptr(m), self._stream()))

    def add_keyframes(self, key, pose, stamps, mask=None):
        """key [B] uint8, pose [B, 6] (p, rotation vector), stamps [B] -> added [B] uint8: 1 where the key frame was stored"""
        torch = self.torch
        k, p, t, m = self._t(key, torch.uint8, (self.B,)), self._t(pose, torch.float64, (self.B, 6)), self._t(stamps, torch.float64, (self.B,)), self._mask(mask)
        self._chk(self.L.liw_fpg_add_keyframes(self.h, self._ptr(self.store), self._ptr(k), self._ptr(p), self._ptr(t), self._ptr(m), self._ptr(self.added),
                                               self._stream()))
        return self.added

    def add_loops(self, found, edge, tf12, mask=None):
        """the found [B] uint8, edge [B, 3] int32, tf12 [B, 12] of FleetLoopDetector.detect"""
        torch = self.torch
        f, e, t, m = self._t(found, torch.uint8, (self.B,)), self._t(edge, torch.int32, (self.B, 3)), self._t(tf12, torch.float64, (self.B, 12)), self._mask(mask)
        self._chk(self.L.liw_fpg_add_loops(self.h, self._ptr(self.store), self._ptr(f), self._ptr(e), self._ptr(t), self._ptr(m), self._stream()))

    def due(self, key, stamps, mask=None):
        """-> due [B] uint8 (is_time_to_solve for the robots with key set) and n_due [1] int32, both on the device"""
        torch = self.torch
        k, t, m = self._t(key, torch.uint8, (self.B,)), self._t(stamps, torch.float64, (self.B,)), self._mask(mask)
        self._chk(self.L.liw_fpg_due(self.h, self._ptr(self.store), self._ptr(k), self._ptr(t), self._ptr(m), self._ptr(self.due_flags), self._ptr(self.n_due),
                                     self._stream()))
        return self.due_flags, self.n_due

    def solve(self, sel, stamps, max_iters=None, check_every=None):
        """keyframe_manager::solve for the robots in sel [B] uint8 (with at least two key frames) -> summary [B, 32] uint8.  With
        check_every > 0 the call synchronises every check_every iterations; with check_every <= 0 never."""
        torch = self.torch
        s = self._t(sel, torch.uint8, (self.B,))
        self._stamps = self._t(stamps, torch.float64, (self.B,))   # kept: the kernels read it after this call has returned
        self._sel = s
        mi = self.max_iters if max_iters is None else int(max_iters)
        ce = self.check_every if check_every is None else int(check_every)
        self._chk(self.L.liw_fpg_solve(self.h, self._ptr(self.store), self._ptr(s), self._ptr(self._stamps), C.c_int(mi), C.c_int(ce), self._ptr(self.summary),
                                       self._stream()))
        return self.summary

    def correct(self, pose, mask=None):
        """update_other_frame: pose [B, 6] of the front-end -> [B, 6] in the corrected map frame"""
        p, m = self._t(pose, self.torch.float64, (self.B, 6)), self._mask(mask)
        self._chk(self.L.liw_fpg_correct(self.h, self._ptr(self.store), self._ptr(p), self._ptr(self.corrected), self._ptr(m), self._stream()))
        return self.corrected

    def _read_n_due(self):
        """the one 4-byte device -> host read of a frame"""
        return int(self.n_due.item())

    def push(self, step_out, loop_out, stamps, mask=None):
        """One frame of the back-end for a FleetTracker.step / FleetTrajectory.step result and, when given, the FleetLoopDetector.push
        result of the same frame: add the key frames (those the loop detector stored, `added`, when loop_out is given, so that both stores
        hold the same key frames and the edge indices agree; step_out["key"] otherwise), add the loops found, evaluate due, and solve the due
        robots.  The read of the n_due word (4 bytes) is the only synchronisation of a frame without a solve; solve() is called only when
        it is non-zero; a masked-out robot is never solved.  -> dict(added, due (zero for masked-out robots), n_due (int), summary,
        modify_delta_tf (the view of modify_delta_tf()))"""
        key = step_out["key"] if loop_out is None else loop_out["added"]
        added = self.add_keyframes(key, step_out["pose"], stamps, mask=mask)
        if loop_out is not None:
            self.add_loops(loop_out["found"], loop_out["edge"], loop_out["tf12"], mask=mask)
        due, _ = self.due(added, stamps, mask=mask)
        if mask is not None:      # due() leaves the rows of masked-out robots as an earlier frame wrote them: they are not selected
            due = due & (self._mask(mask) != 0).to(self.torch.uint8)
        n = self._read_n_due()
        if n:
            self.solve(due, stamps)
        return dict(added=added, due=due, n_due=n, summary=self.summary, modify_delta_tf=self.modify_delta_tf())

    # ---- inspection (synchronous)
    def summaries(self):
        self._sync()
        return summary_rows(self.summary.cpu().numpy())

    def num_keyframes(self, robot):
        self._sync()
        return self._chk(self.L.liw_fpg_num_keyframes(self.h, self._ptr(self.store), C.c_int(robot)))

    def flags(self, robot):
        """dict(loops, full, loops_full, bad_edge, pending, solves, last_solve_time)"""
        self._sync()
        f, t = np.zeros(6, dtype=np.int32), C.c_double(0)
        self._chk(self.L.liw_fpg_flags(self.h, self._ptr(self.store), C.c_int(robot), _pi(f), C.byref(t)))
        out = {k: int(v) for k, v in zip(FLAGS, f)}
        out["last_solve_time"] = t.value
        return out

    def keyframes(self, robot):
        """dict(poses [n, 6], stamps [n], tf12 [n, 12])"""
        self._sync()
        n = self._chk(self.L.liw_fpg_get_keyframes(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(0), None, None, None))
        p, s, t = np.zeros((max(n, 1), 6)), np.zeros(max(n, 1)), np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_fpg_get_keyframes(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(n), _pd(p), _pd(s), _pd(t)))
        return dict(poses=p[:n], stamps=s[:n], tf12=t[:n])

    def seq_edges(self, robot):
        """[n - 1, 12]: edge k is (k, k + 1)"""
        self._sync()
        n = self._chk(self.L.liw_fpg_get_seq_edges(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(0), None))
        t = np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_fpg_get_seq_edges(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(n), _pd(t)))
        return t[:n]

    def loop_edges(self, robot):
        """idx [n, 2] int32, tf12 [n, 12]"""
        self._sync()
        n = self._chk(self.L.liw_fpg_get_loop_edges(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(0), None, None))
        i, t = np.zeros((max(n, 1), 2), dtype=np.int32), np.zeros((max(n, 1), 12))
        self._chk(self.L.liw_fpg_get_loop_edges(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(n), _pi(i), _pd(t)))
        return i[:n], t[:n]

    def get_modify_delta_tf(self, robot):
        self._sync()
        t = np.zeros(12)
        self._chk(self.L.liw_fpg_get_modify_delta_tf(self.h, self._ptr(self.store), C.c_int(robot), _pd(t)))
        return t

    def last_summary(self, robot):
        from . import SummaryC
        self._sync()
        sm = SummaryC()
        self._chk(self.L.liw_fpg_get_summary(self.h, self._ptr(self.store), C.c_int(robot), C.byref(sm)))
        return dict(iterations=sm.iterations, successful=sm.successful_steps, termination=sm.termination, initial_cost=sm.initial_cost,
                    final_cost=sm.final_cost)

    def load_graph(self, robot, G, stamps=None):
        """replace a robot's graph by a posegraph.make_pose_graph dict (tests and tools)"""
        self._sync()
        x = np.ascontiguousarray(G["poses"], dtype=np.float64).reshape(-1, 6)
        st = np.ascontiguousarray(G["seq_tf12"], dtype=np.float64).reshape(-1, 12) if len(x) > 1 else None
        li = np.ascontiguousarray(G["loop_idx"], dtype=np.int32).reshape(-1, 2)
        lt = np.ascontiguousarray(G["loop_tf12"], dtype=np.float64).reshape(-1, 12)
        ts = None if stamps is None else np.ascontiguousarray(stamps, dtype=np.float64)
        self._chk(self.L.liw_fpg_load_graph(self.h, self._ptr(self.store), C.c_int(robot), C.c_int(len(x)), _pd(x), _pd(ts), _pd(st), C.c_int(len(li)),
                                            _pi(li) if len(li) else None, _pd(lt) if len(li) else None))
