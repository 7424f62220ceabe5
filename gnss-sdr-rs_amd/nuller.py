"""Adaptive spatial nulling of an antenna array over the C ABI (gm_nuller, include/gnss_mi355x.h): A coherent antennas, interleaved time
sample by time sample in one complex64 or int8-IQ stream, combined into one complex64 stream at the same rate.  Per block of B time
samples the weights come from the block's own covariance, w = Rl^-1 s / (s^H Rl^-1 s): a null on whatever dominates the block, the
response held at 1 towards s (None: antenna 0 as the reference, power inversion).  Every output is defined by absolute indices, so the
words do not depend on how the stream is cut into calls.  All counts are TIME samples."""
import numpy as np

from . import _lib
from ._lib import NullerCfg
from ._stage import ArrayStage, _array, _p, array_plan


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
    return array_plan("nuller", c, inputs_so_far, n_in)


class Nuller(ArrayStage):
    """process(x, want_blocks=False): x [n, A] complex64 or [n, A, 2] int8 -> complex64 [n_out]: this call's outputs (synchronous);
    with want_blocks (y, R [blocks, A, A], w [blocks, A]): the words each of the call's blocks was combined with (R is zeros in static
    mode).  capture(d_R, d_w, cap_blocks): device buffers [cap_blocks][A][A] and [cap_blocks][A]."""
    _NAME = "nuller"

    def __init__(self, n_antennas, block=0, loading=0.0, steering=None, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, block, loading, steering)
        c, keep = _cfg(n_antennas, block, loading, steering)
        self.n_antennas, self.block, self.loading = int(n_antennas), p["block"], p["loading"]
        self._M = self.n_antennas
        self._open(c)

    def set_weights(self, w=None):
        """A fixed complex weights for every later block (static mode); None: back to the adaptive rule"""
        if w is None:
            self._call("set_weights", None)
            return
        w = np.ascontiguousarray(np.asarray(w).astype(np.complex64))
        if w.shape != (self.n_antennas,):
            raise ValueError("w: n_antennas complex words")
        self._call("set_weights", _p(w))

    def stats(self):
        """time samples taken, outputs delivered, blocks finished since the creation or the last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blocks")
