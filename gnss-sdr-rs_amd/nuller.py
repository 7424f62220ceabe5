"""Adaptive spatial nulling of an antenna array over the C ABI (gm_nuller, include/gnss_mi355x.h): A coherent antennas, interleaved time
sample by time sample in one complex64 or int8-IQ stream, combined into one complex64 stream at the same rate.  Per block of B time
samples the weights come from the block's own covariance, w = Rl^-1 s / (s^H Rl^-1 s): a null on whatever dominates the block, the
response held at 1 towards s (None: antenna 0 as the reference, power inversion).  Every output is defined by absolute indices, so the
words do not depend on how the stream is cut into calls.  All counts are TIME samples."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NullerCfg, check, lib
from .resample import _p


def _cfg(n_antennas, block=0, loading=0.0, steering=None):
    """-> (cfg, the array it points at: keep it alive as long as the cfg)"""
    keep = None
    if steering is not None:
        keep = np.ascontiguousarray(np.asarray(steering).astype(np.complex64))
        if keep.shape != (int(n_antennas),):
            raise ValueError("steering: n_antennas complex words")
    return NullerCfg(int(n_antennas), int(block), float(loading), 0, keep.ctypes.data if keep is not None else None), keep


def plan(n_antennas, block=0, loading=0.0, steering=None, inputs_so_far=0, n_in=0):
    """gm_nuller_plan (host only, no device): the argument rules, the defaults and the number of outputs that n_in more time samples
    deliver to a stream that has taken inputs_so_far."""
    c, keep = _cfg(n_antennas, block, loading, steering)
    b, ld, n = C.c_uint32(0), C.c_float(0), C.c_uint64(0)
    check(lib().gm_nuller_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(b), C.byref(ld), C.byref(n)), "gm_nuller_plan")
    return dict(block=b.value, loading=ld.value, n_out=n.value)


def _array(x, A):
    """[n, A] complex64 or [n, A, 2] int8 -> (contiguous array, time samples, format)"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.int8 and x.ndim == 3 and x.shape[1:] == (A, 2):
        return x, x.shape[0], _lib.FMT_I8_IQ
    if x.dtype == np.complex64 and x.ndim == 2 and x.shape[1] == A:
        return x, x.shape[0], _lib.FMT_C32
    raise ValueError("x: [n, %d] complex64 or [n, %d, 2] int8" % (A, A))


class Nuller:
    def __init__(self, n_antennas, block=0, loading=0.0, steering=None, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, block, loading, steering)
        c, keep = _cfg(n_antennas, block, loading, steering)
        self.n_antennas, self.block, self.loading = int(n_antennas), p["block"], p["loading"]
        h = C.c_void_p()
        check(lib().gm_nuller_create(C.byref(c), C.byref(h)), "gm_nuller_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gm_nuller_destroy(self._h)
            self._h = None

    def __del__(self):      # (at interpreter shutdown the module globals close() uses may be gone already)
        try:
            self.close()
        except Exception:
            pass

    def process(self, x, want_blocks=False):
        """x: [n, A] complex64 or [n, A, 2] int8 -> complex64 [n_out]: this call's outputs (synchronous); with want_blocks
        (y, R [blocks, A, A], w [blocks, A]): the words each of the call's blocks was combined with (R is zeros in static mode)"""
        A = self.n_antennas
        x, n, fmt = _array(x, A)
        cap = n + self.block
        out = np.zeros(cap, np.complex64)
        got = C.c_size_t(0)
        if not want_blocks:
            check(lib().gm_nuller_process(self._h, _p(x), fmt, n, _p(out), cap, C.byref(got), None, None, 0), "gm_nuller_process")
            return out[:got.value].copy()
        nb = cap // self.block
        R, w = np.zeros((nb, A, A), np.complex64), np.zeros((nb, A), np.complex64)
        check(lib().gm_nuller_process(self._h, _p(x), fmt, n, _p(out), cap, C.byref(got), _p(R), _p(w), nb), "gm_nuller_process")
        nb = got.value // self.block
        return out[:got.value].copy(), R[:nb].copy(), w[:nb].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_cap, stream=None):
        """device pointers, n_in time samples; asynchronous on `stream` (None: the handle's own); returns the outputs written"""
        got = C.c_size_t(0)
        check(lib().gm_nuller_process_dev(self._h, d_in, fmt, n_in, d_out, out_cap, C.byref(got), stream), "gm_nuller_process_dev")
        return got.value

    def set_weights(self, w=None):
        """A fixed complex weights for every later block (static mode); None: back to the adaptive rule"""
        if w is None:
            check(lib().gm_nuller_set_weights(self._h, None), "gm_nuller_set_weights")
            return
        w = np.ascontiguousarray(np.asarray(w).astype(np.complex64))
        if w.shape != (self.n_antennas,):
            raise ValueError("w: n_antennas complex words")
        check(lib().gm_nuller_set_weights(self._h, _p(w)), "gm_nuller_set_weights")

    def capture(self, d_R=None, d_w=None, cap_blocks=0):
        """device buffers [cap_blocks][A][A] and [cap_blocks][A] complex64 that every later process_dev fills from word 0"""
        check(lib().gm_nuller_capture(self._h, d_R, d_w, int(cap_blocks)), "gm_nuller_capture")

    def reset(self, input_index=0):
        check(lib().gm_nuller_reset(self._h, int(input_index)), "gm_nuller_reset")

    def stats(self):
        """time samples taken, outputs delivered, blocks finished since the creation or the last reset (synchronises)"""
        i, o, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().gm_nuller_stats(self._h, C.byref(i), C.byref(o), C.byref(b)), "gm_nuller_stats")
        return dict(inputs=i.value, outputs=o.value, blocks=b.value)

    def synchronize(self):
        check(lib().gm_nuller_synchronize(self._h), "gm_nuller_synchronize")
