"""What the wrappers of the streaming stages share.  Stage holds a handle of the C ABI's gm_<name>_* entries and its life cycle
(Resampler, Excisor, Ddc, Channelizer); ArrayStage adds what the antenna-array stages have in common (Nuller, Stap, Beamformer): the plan
outputs, the capture, process_dev and the body of process.  A class keeps what differs in more than the prefix of the entry's name."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _array(x, A):
    """[n, A] complex64 or [n, A, 2] int8 -> (contiguous array, time samples, format)"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.int8 and x.ndim == 3 and x.shape[1:] == (A, 2):
        return x, x.shape[0], _lib.FMT_I8_IQ
    if x.dtype == np.complex64 and x.ndim == 2 and x.shape[1] == A:
        return x, x.shape[0], _lib.FMT_C32
    raise ValueError("x: [n, %d] complex64 or [n, %d, 2] int8" % (A, A))


class Stage:
    _NAME = None            # the entries are gm_<_NAME>_*

    def _open(self, cfg):
        """gm_<name>_create on the initialised device"""
        h = C.c_void_p()
        entry = "gm_%s_create" % self._NAME
        check(getattr(lib(), entry)(C.byref(cfg), C.byref(h)), entry)
        self._h = h

    def _call(self, entry, *args):
        entry = "gm_%s_%s" % (self._NAME, entry)
        check(getattr(lib(), entry)(self._h, *args), entry)

    def _counters(self, *keys):
        """gm_<name>_stats where it is that many uint64 counters (synchronises)"""
        v = [C.c_uint64(0) for _ in keys]
        self._call("stats", *[C.byref(c) for c in v])
        return dict(zip(keys, (c.value for c in v)))

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), "gm_%s_destroy" % self._NAME)(self._h)
            self._h = None

    def __del__(self):      # (at interpreter shutdown the module globals close() uses may be gone already)
        try:
            self.close()
        except Exception:
            pass

    def reset(self, input_index=0):
        self._call("reset", int(input_index))

    def synchronize(self):
        self._call("synchronize")


def array_plan(name, cfg, inputs_so_far, n_in):
    """gm_<name>_plan of an array stage -> dict(block, loading, n_out)"""
    b, ld, n = C.c_uint32(0), C.c_float(0), C.c_uint64(0)
    entry = "gm_%s_plan" % name
    check(getattr(lib(), entry)(C.byref(cfg), int(inputs_so_far), int(n_in), C.byref(b), C.byref(ld), C.byref(n)), entry)
    return dict(block=b.value, loading=ld.value, n_out=n.value)


class ArrayStage(Stage):
    """A class sets n_antennas and block, and _M and _P: per block R is [_M, _M] and w is [_M], or [_P, _M] where the stage has _P
    output planes (None: one stream, no plane axis)."""
    _M, _P = 0, None

    def process(self, x, want_blocks=False):
        x, n, fmt = _array(x, self.n_antennas)
        cap = n + self.block
        rows = () if self._P is None else (self._P,)
        out = np.zeros(rows + (cap,), np.complex64)
        got = C.c_size_t(0)
        if not want_blocks:
            self._call("process", _p(x), fmt, n, _p(out), cap, C.byref(got), None, None, 0)
            return out[..., :got.value].copy()
        nb = cap // self.block
        R, w = np.zeros((nb, self._M, self._M), np.complex64), np.zeros((nb,) + rows + (self._M,), np.complex64)
        self._call("process", _p(x), fmt, n, _p(out), cap, C.byref(got), _p(R), _p(w), nb)
        nb = got.value // self.block
        return out[..., :got.value].copy(), R[:nb].copy(), w[:nb].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_cap, stream=None):
        """device pointers, n_in time samples; asynchronous on `stream` (None: the handle's own); returns the outputs written"""
        got = C.c_size_t(0)
        self._call("process_dev", d_in, fmt, n_in, d_out, out_cap, C.byref(got), stream)
        return got.value

    def _set_flat_weights(self, w, words, refusal):
        if w is None:
            self._call("set_weights", None)
            return
        w = np.ascontiguousarray(np.asarray(w).astype(np.complex64)).reshape(-1)
        if w.shape != (words,):
            raise ValueError(refusal)
        self._call("set_weights", _p(w))

    def capture(self, d_R=None, d_w=None, cap_blocks=0):
        """device buffers [cap_blocks] x the block's R words and [cap_blocks] x the block's w words, complex64, that every later
        process_dev fills from word 0"""
        self._call("capture", d_R, d_w, int(cap_blocks))
