"""Several constraints on one beam over the C ABI (gm_lcmv, include/gnss_mi355x.h): the beamformer's interleaved stream of A coherent
antennas with L taps in time behind each, where beam p carries Q_p constraint rows c_q of M = A L words and Q_p responses f_q in place of
one row.  Per block of B time samples ONE Gram matrix and ONE Cholesky factor serve every beam; beam p then has
w_p = Rl^-1 C (C^H Rl^-1 C)^-1 f, so that C^H w_p = f, and its own output plane y_p[t] = sum_l sum_a conj(w_p[l A + a]) x_a[t - l]: a
signal whose stacked vector is c_q comes out with the gain conj(f_q).  `constraints` is a list of (rows [Q_p][L][A], f [Q_p]) per beam.
All counts are TIME samples, per beam."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LcmvCfg
from ._stage import ArrayStage, _p, array_plan


def _beam(M, rows, f):
    """one beam's (rows, f) -> (complex64 [Q, M], complex64 [Q])"""
    f = np.ascontiguousarray(np.asarray(f).astype(np.complex64)).reshape(-1)
    r = np.ascontiguousarray(np.asarray(rows).astype(np.complex64))
    if M <= 0 or f.size == 0 or r.size != f.size * M:
        raise ValueError("a beam: (rows [Q][taps][n_antennas], f [Q]) complex words")
    return r.reshape(f.size, M), f


def _pack(n_antennas, taps, constraints, response=None):
    """constraints: a list of (rows, f) per beam; or a list of rows per beam with `response` a list of f per beam
    -> (Q uint32 [P], rows complex64 [sum Q, M], f complex64 [sum Q])"""
    M = int(n_antennas) * int(taps)
    if constraints is None or len(constraints) == 0:
        raise ValueError("constraints are required: a list of (rows, f) per beam")
    if response is not None:
        if len(response) != len(constraints):
            raise ValueError("response: one list of responses per beam")
        constraints = list(zip(constraints, response))
    beams = [_beam(M, rows, f) for rows, f in constraints]
    q = np.array([b[1].size for b in beams], np.uint32)
    return q, np.ascontiguousarray(np.concatenate([b[0] for b in beams])), np.ascontiguousarray(np.concatenate([b[1] for b in beams]))


def _cfg(n_antennas, taps, constraints, response=None, block=0, loading=0.0):
    """-> (cfg, the arrays it points at: keep them alive as long as the cfg)"""
    keep = _pack(n_antennas, taps, constraints, response)
    q, rows, f = keep
    return LcmvCfg(int(n_antennas), int(taps), int(block), float(loading), q.size, 0, q.ctypes.data, rows.ctypes.data, f.ctypes.data, 0), keep


def plan(n_antennas, taps, constraints, response=None, block=0, loading=0.0, inputs_so_far=0, n_in=0):
    """gm_lcmv_plan (host only, no device): the argument rules, the defaults and the number of outputs PER BEAM that n_in more time
    samples deliver to a stream that has taken inputs_so_far."""
    c, keep = _cfg(n_antennas, taps, constraints, response, block, loading)
    return array_plan("lcmv", c, inputs_so_far, n_in)


class Lcmv(ArrayStage):
    """Lcmv(n_antennas, taps, constraints, response=None, block=0, loading=0.0): constraints is a list of (rows, f) per beam (or a list
    of rows per beam, with response a list of f per beam).
    process(x, want_blocks=False): x [n, A] complex64 or [n, A, 2] int8 -> complex64 [P, n_out]: this call's outputs, a row a beam
    (synchronous); with want_blocks (y, R [blocks, M, M], w [blocks, P, M]): the words each of the call's blocks was combined with (R is
    zeros in static mode).  capture(d_R, d_w, cap_blocks): device buffers [cap_blocks][M][M] and [cap_blocks][P][M]."""
    _NAME = "lcmv"

    def __init__(self, n_antennas, taps, constraints, response=None, block=0, loading=0.0, device=None):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_antennas, taps, constraints, response, block, loading)
        c, keep = _cfg(n_antennas, taps, constraints, response, block, loading)
        self.n_antennas, self.taps, self.block, self.loading = int(n_antennas), int(taps), p["block"], p["loading"]
        self.n_weights = self._M = self.n_antennas * self.taps
        self.n_beams = self._P = int(keep[0].size)
        self.n_constraints = [int(q) for q in keep[0]]
        self._open(c)

    @staticmethod
    def plan(n_antennas, taps, constraints, response=None, block=0, loading=0.0, inputs_so_far=0, n_in=0):
        """the module's plan(): gm_lcmv_plan, host only"""
        return plan(n_antennas, taps, constraints, response, block, loading, inputs_so_far, n_in)

    def want_blocks(self, x):
        """process(x, want_blocks=True): (y [P, n_out], R [blocks, M, M], w [blocks, P, M])"""
        return self.process(x, want_blocks=True)

    def process_dev(self, d_in, fmt, n_in, d_out, out_stride, stream=None):
        """device pointers, n_in time samples; beam p's outputs at d_out + p * out_stride complex64 words; asynchronous on `stream`
        (None: the handle's own); returns the outputs written per beam"""
        return super().process_dev(d_in, fmt, n_in, d_out, out_stride, stream)

    def set_constraints(self, beam, rows, f):
        """beam `beam`'s new rows [Q][taps][n_antennas] and responses [Q], for every block a later call finishes (Q may differ from
        the beam's old count as long as the rows of all beams stay <= 16); waits for the handle's calls in flight (synchronous)"""
        r, f = _beam(self.n_weights, rows, f)
        self._call("set_constraints", int(beam), int(f.size), _p(r), _p(f))
        self.n_constraints[int(beam)] = int(f.size)

    def set_weights(self, w=None):
        """[P][M] fixed complex weights for every later block (static mode, synchronous); None: back to the adaptive rule"""
        self._set_flat_weights(w, self.n_beams * self.n_weights, "w: beams * taps * n_antennas complex words")

    def stats(self):
        """time samples taken, outputs delivered per beam, blocks finished and, per beam, the blocks that took the quiescent weights
        since the creation or the last reset (synchronises)"""
        i, o, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = (C.c_uint64 * self.n_beams)()
        self._call("stats", C.byref(i), C.byref(o), C.byref(b), f)
        return dict(inputs=i.value, outputs=o.value, blocks=b.value, fallbacks=list(f))
