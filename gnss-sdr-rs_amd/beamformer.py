"""One beam per satellite from a shared covariance over the C ABI (gm_beamformer, include/gnss_mi355x.h): gm_stap's interleaved stream
of A coherent antennas with L taps in time behind each, and P constraint rows s_p of M = A L words in place of one.  Per block of B time
samples ONE Gram matrix and ONE Cholesky factor serve every beam; beam p then has w_p = Rl^-1 s_p / (s_p^H Rl^-1 s_p) and its own output
plane y_p[t] = sum_l sum_a conj(w_p[l A + a]) x_a[t - l].  Beam p's words are, word for word, those of a Stap created with steering = s_p
on the same stream, whatever P, the other rows and the cuts of the stream.  steering is [P][L][A] and is required (power inversion: e_0
as a row).  All counts are TIME samples, per beam."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BeamformerCfg
from ._stage import ArrayStage, _p, array_plan


def _rows(n_antennas, taps, steering):
    M = int(n_antennas) * int(taps)
    if steering is None:
        raise ValueError("steering is required: [beams][taps][n_antennas]")
    s = np.ascontiguousarray(np.asarray(steering).astype(np.complex64))
    if M <= 0 or s.size == 0 or s.size % M or (s.ndim > 1 and s.shape[0] * M != s.size):
        raise ValueError("steering: [beams][taps][n_antennas] complex words")
    return s.reshape(-1, M)


def _cfg(n_antennas, taps, steering, block=0, loading=0.0):
    """-> (cfg, the array it points at: keep it alive as long as the cfg)"""
    keep = _rows(n_antennas, taps, steering)
    return BeamformerCfg(int(n_antennas), int(taps), int(block), float(loading), keep.shape[0], 0, keep.ctypes.data, 0), keep


def plan(n_antennas, taps, steering, block=0, loading=0.0, inputs_so_far=0, n_in=0):
    """gm_beamformer_plan (host only, no device): the argument rules, the defaults and the number of outputs PER BEAM that n_in more
    time samples deliver to a stream that has taken inputs_so_far."""
    c, keep = _cfg(n_antennas, taps, steering, block, loading)
    return array_plan("beamformer", c, inputs_so_far, n_in)


class Beamformer(ArrayStage):
    """process(x, want_blocks=False): x [n, A] complex64 or [n, A, 2] int8 -> complex64 [P, n_out]: this call's outputs, a row a beam
    (synchronous); with want_blocks (y, R [blocks, M, M], w [blocks, P, M]): the words each of the call's blocks was combined with (R is
    zeros in static mode).  capture(d_R, d_w, cap_blocks): device buffers [cap_blocks][M][M] and [cap_blocks][P][M]."""
    _NAME = "beamformer"

    def __init__(self, n_antennas, taps, steering, block=0, loading=0.0, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, taps, steering, block, loading)
        c, keep = _cfg(n_antennas, taps, steering, block, loading)
        self.n_antennas, self.taps, self.block, self.loading = int(n_antennas), int(taps), p["block"], p["loading"]
        self.n_weights = self._M = self.n_antennas * self.taps
        self.n_beams = self._P = keep.shape[0]
        self._open(c)

    def process_dev(self, d_in, fmt, n_in, d_out, out_stride, stream=None):
        """device pointers, n_in time samples; beam p's outputs at d_out + p * out_stride complex64 words; asynchronous on `stream`
        (None: the handle's own); returns the outputs written per beam"""
        return super().process_dev(d_in, fmt, n_in, d_out, out_stride, stream)

    def set_steering(self, beam, s):
        """beam `beam`'s new row of M = taps * n_antennas words [taps][n_antennas], for every block a later call finishes; waits for
        the handle's calls in flight (synchronous)"""
        s = np.ascontiguousarray(np.asarray(s).astype(np.complex64)).reshape(-1)
        if s.shape != (self.n_weights,):
            raise ValueError("s: taps * n_antennas complex words")
        self._call("set_steering", int(beam), _p(s))

    def set_steering_dev(self, first_beam, n_rows, d_rows, d_info=None, min_ratio=0.0, d_installed=None, stream=None):
        """gm_beamformer_set_steering_dev: rows [n_rows][M] complex64 in DEVICE memory (solve_rows_dev's d_rows) into beams first_beam
        .. first_beam + n_rows - 1 by a kernel on `stream` (None: the handle's own), ordered like a process_dev call, no host wait.
        A row is installed where it is finite and not all zero and, with d_info (solve_rows_dev's), its status is 0 and lambda1 >=
        min_ratio * lambda2; d_installed: device uint8 [n_rows], 1 where installed."""
        self._call("set_steering_dev", int(first_beam), int(n_rows), C.c_void_p(d_rows), C.c_void_p(d_info), float(min_ratio),
                   C.c_void_p(d_installed), C.c_void_p(stream))

    def set_weights(self, w=None):
        """[P][M] fixed complex weights for every later block (static mode, synchronous); None: back to the adaptive rule"""
        self._set_flat_weights(w, self.n_beams * self.n_weights, "w: beams * taps * n_antennas complex words")

    def stats(self):
        """time samples taken, outputs delivered per beam, blocks finished and, per beam, the blocks that took the fallback weights
        since the creation or the last reset (synchronises)"""
        i, o, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = (C.c_uint64 * self.n_beams)()
        self._call("stats", C.byref(i), C.byref(o), C.byref(b), f)
        return dict(inputs=i.value, outputs=o.value, blocks=b.value, fallbacks=list(f))
