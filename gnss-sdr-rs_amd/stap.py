"""Space-time adaptive nulling of an antenna array over the C ABI (gm_stap, include/gnss_mi355x.h): the nuller's interleaved stream of A
coherent antennas, with L taps in time behind each.  Per block of B time samples the M = A L weights come from the exact Gram matrix of
the block's stacked samples z[t][l A + a] = x_a[t - l], w = Rl^-1 s / (s^H Rl^-1 s), and y[t] = sum_l sum_a conj(w[l A + a]) x_a[t - l]:
a narrowband interferer costs a temporal degree of freedom, not one of the A - 1 spatial ones.  s is [L][A] (None: antenna 0 at tap 0).
Every output is defined by absolute indices, so the words do not depend on how the stream is cut into calls.  All counts are TIME
samples."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import StapCfg, check, lib
from .nuller import _array
from .resample import _p


def _cfg(n_antennas, taps, block=0, loading=0.0, steering=None):
    """-> (cfg, the array it points at: keep it alive as long as the cfg)"""
    keep = None
    if steering is not None:
        keep = np.ascontiguousarray(np.asarray(steering).astype(np.complex64)).reshape(-1)
        if keep.shape != (int(n_antennas) * int(taps),):
            raise ValueError("steering: taps * n_antennas complex words")
    return StapCfg(int(n_antennas), int(taps), int(block), float(loading), keep.ctypes.data if keep is not None else None, 0), keep


def plan(n_antennas, taps, block=0, loading=0.0, steering=None, inputs_so_far=0, n_in=0):
    """gm_stap_plan (host only, no device): the argument rules, the defaults and the number of outputs that n_in more time samples
    deliver to a stream that has taken inputs_so_far."""
    c, keep = _cfg(n_antennas, taps, block, loading, steering)
    b, ld, n = C.c_uint32(0), C.c_float(0), C.c_uint64(0)
    check(lib().gm_stap_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(b), C.byref(ld), C.byref(n)), "gm_stap_plan")
    return dict(block=b.value, loading=ld.value, n_out=n.value)


class Stap:
    def __init__(self, n_antennas, taps, block=0, loading=0.0, steering=None, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, taps, block, loading, steering)
        c, keep = _cfg(n_antennas, taps, block, loading, steering)
        self.n_antennas, self.taps, self.block, self.loading = int(n_antennas), int(taps), p["block"], p["loading"]
        self.n_weights = self.n_antennas * self.taps
        h = C.c_void_p()
        check(lib().gm_stap_create(C.byref(c), C.byref(h)), "gm_stap_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gm_stap_destroy(self._h)
            self._h = None

    def __del__(self):      # (at interpreter shutdown the module globals close() uses may be gone already)
        try:
            self.close()
        except Exception:
            pass

    def process(self, x, want_blocks=False):
        """x: [n, A] complex64 or [n, A, 2] int8 -> complex64 [n_out]: this call's outputs (synchronous); with want_blocks
        (y, R [blocks, M, M], w [blocks, M]): the words each of the call's blocks was combined with (R is zeros in static mode)"""
        M = self.n_weights
        x, n, fmt = _array(x, self.n_antennas)
        cap = n + self.block
        out = np.zeros(cap, np.complex64)
        got = C.c_size_t(0)
        if not want_blocks:
            check(lib().gm_stap_process(self._h, _p(x), fmt, n, _p(out), cap, C.byref(got), None, None, 0), "gm_stap_process")
            return out[:got.value].copy()
        nb = cap // self.block
        R, w = np.zeros((nb, M, M), np.complex64), np.zeros((nb, M), np.complex64)
        check(lib().gm_stap_process(self._h, _p(x), fmt, n, _p(out), cap, C.byref(got), _p(R), _p(w), nb), "gm_stap_process")
        nb = got.value // self.block
        return out[:got.value].copy(), R[:nb].copy(), w[:nb].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_cap, stream=None):
        """device pointers, n_in time samples; asynchronous on `stream` (None: the handle's own); returns the outputs written"""
        got = C.c_size_t(0)
        check(lib().gm_stap_process_dev(self._h, d_in, fmt, n_in, d_out, out_cap, C.byref(got), stream), "gm_stap_process_dev")
        return got.value

    def set_weights(self, w=None):
        """M = taps * n_antennas fixed complex weights [taps][n_antennas] for every later block (static mode); None: back to the
        adaptive rule"""
        if w is None:
            check(lib().gm_stap_set_weights(self._h, None), "gm_stap_set_weights")
            return
        w = np.ascontiguousarray(np.asarray(w).astype(np.complex64)).reshape(-1)
        if w.shape != (self.n_weights,):
            raise ValueError("w: taps * n_antennas complex words")
        check(lib().gm_stap_set_weights(self._h, _p(w)), "gm_stap_set_weights")

    def capture(self, d_R=None, d_w=None, cap_blocks=0):
        """device buffers [cap_blocks][M][M] and [cap_blocks][M] complex64 that every later process_dev fills from word 0"""
        check(lib().gm_stap_capture(self._h, d_R, d_w, int(cap_blocks)), "gm_stap_capture")

    def reset(self, input_index=0):
        check(lib().gm_stap_reset(self._h, int(input_index)), "gm_stap_reset")

    def stats(self):
        """time samples taken, outputs delivered, blocks finished and blocks that took the fallback weights since the creation or the
        last reset (synchronises)"""
        i, o, b, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().gm_stap_stats(self._h, C.byref(i), C.byref(o), C.byref(b), C.byref(f)), "gm_stap_stats")
        return dict(inputs=i.value, outputs=o.value, blocks=b.value, fallback_blocks=f.value)

    def synchronize(self):
        check(lib().gm_stap_synchronize(self._h), "gm_stap_synchronize")
