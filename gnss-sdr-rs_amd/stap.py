"""Space-time adaptive nulling of an antenna array over the C ABI (gm_stap, include/gnss_mi355x.h): the nuller's interleaved stream of A
coherent antennas, with L taps in time behind each.  Per block of B time samples the M = A L weights come from the exact Gram matrix of
the block's stacked samples z[t][l A + a] = x_a[t - l], w = Rl^-1 s / (s^H Rl^-1 s), and y[t] = sum_l sum_a conj(w[l A + a]) x_a[t - l]:
a narrowband interferer costs a temporal degree of freedom, not one of the A - 1 spatial ones.  s is [L][A] (None: antenna 0 at tap 0).
Every output is defined by absolute indices, so the words do not depend on how the stream is cut into calls.  All counts are TIME
samples."""
import numpy as np

from . import _lib
from ._lib import StapCfg
from ._stage import ArrayStage, array_plan


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
    return array_plan("stap", c, inputs_so_far, n_in)


class Stap(ArrayStage):
    """process(x, want_blocks=False): x [n, A] complex64 or [n, A, 2] int8 -> complex64 [n_out]: this call's outputs (synchronous);
    with want_blocks (y, R [blocks, M, M], w [blocks, M]): the words each of the call's blocks was combined with (R is zeros in static
    mode).  capture(d_R, d_w, cap_blocks): device buffers [cap_blocks][M][M] and [cap_blocks][M]."""
    _NAME = "stap"

    def __init__(self, n_antennas, taps, block=0, loading=0.0, steering=None, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, taps, block, loading, steering)
        c, keep = _cfg(n_antennas, taps, block, loading, steering)
        self.n_antennas, self.taps, self.block, self.loading = int(n_antennas), int(taps), p["block"], p["loading"]
        self.n_weights = self._M = self.n_antennas * self.taps
        self._open(c)

    def set_weights(self, w=None):
        """M = taps * n_antennas fixed complex weights [taps][n_antennas] for every later block (static mode); None: back to the
        adaptive rule"""
        self._set_flat_weights(w, self.n_weights, "w: taps * n_antennas complex words")

    def stats(self):
        """time samples taken, outputs delivered, blocks finished and blocks that took the fallback weights since the creation or the
        last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blocks", "fallback_blocks")
