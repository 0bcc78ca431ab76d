"""What the fleet modules that own a per-robot store share (loop_batch.FleetLoopDetector, posegraph_batch.FleetBackEnd): the store
tensor with its guard bytes, the handle's life cycle and error check, and the tensor / pointer conversions of a call."""
import ctypes as C

import numpy as np


def _pd(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _pi(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class FleetStore:
    """Base of a class that owns a fleet store.  The subclass names the C functions `_destroy` and `_last_error` (attributes of
    the library), sets L, B, dev, lay and the handle h, and then calls `_alloc_store`."""

    _destroy = _last_error = None

    def _alloc_store(self, guard):
        """the zeroed store (a torch uint8 tensor) with `guard` bytes of 0xA5 on either side"""
        torch = self.torch
        self.guard = int(guard)
        if self.guard % 8:
            raise ValueError("guard must be a multiple of 8 (the store is 8-byte aligned)")
        self._buf = torch.zeros(self.lay["bytes"] + 2 * self.guard, dtype=torch.uint8, device=self.dev)   # zeroed: the bytes are reproducible
        if self.guard:
            self._buf[:self.guard] = 0xA5
            self._buf[self.guard + self.lay["bytes"]:] = 0xA5
        self.store = self._buf[self.guard:self.guard + self.lay["bytes"]]

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r < 0:
            raise self.LiwError(r, getattr(self.L, self._last_error)(self.h).decode())
        return r

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _t(self, a, dt, shape=None):
        torch = self.torch
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
        t = t.to(device=self.dev, dtype=dt).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def _mask(self, mask):
        return None if mask is None else self._t(mask, self.torch.uint8, (self.B,))

    def robot_regions(self):
        """[B, robot_bytes] uint8 view of the store's robot regions (the work area behind them is not part of it)"""
        return self.store[:self.B * self.lay["robot_bytes"]].view(self.B, self.lay["robot_bytes"])

    def _sync(self):
        self.torch.cuda.synchronize(self.dev)
