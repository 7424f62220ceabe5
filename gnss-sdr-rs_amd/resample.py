"""Rate conversion and pulse blanking over the C ABI (gm_resampler, include/gnss_mi355x.h): the two stages the reference's
DigitalFrontend::process_block names in comments and leaves out (src/rf/frontend.rs).  A Resampler turns a stream of complex64 or
int8-IQ samples at fs_in into complex64 samples at fs_in * up / down; every output is defined by absolute sample indices alone, so the
words do not depend on how the stream is cut into calls."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib
from ._lib import FMT_C32, FMT_I8_IQ, ResamplerCfg, check, lib
from ._stage import Stage, _p

_KEYS = ("taps", "n_phases", "cutoff", "kaiser_beta", "blank_threshold")


def _cfg(up, down, taps=0, n_phases=0, cutoff=0.0, kaiser_beta=0.0, blank_threshold=0.0):
    return ResamplerCfg(int(up), int(down), int(taps), int(n_phases), float(cutoff), float(kaiser_beta), float(blank_threshold), 0)


def plan(up, down, inputs_so_far=0, n_in=0, **cfg):
    """gm_resampler_plan (host only, no device): the argument rules, the reduced ratio, the defaults and the number of outputs that
    n_in more inputs deliver to a stream that has taken inputs_so_far."""
    c = _cfg(up, down, **cfg)
    u, d, t, ph, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    check(lib().gm_resampler_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(u), C.byref(d), C.byref(t), C.byref(ph),
                                  C.byref(n)), "gm_resampler_plan")
    return dict(up=u.value, down=d.value, taps=t.value, n_phases=ph.value, n_out=n.value)


def design(up, down, **cfg):
    """gm_resampler_design (host only, no device): the [n_phases + 1][taps] float32 table."""
    p = plan(up, down, **cfg)
    c = _cfg(up, down, **cfg)
    table = np.zeros((p["n_phases"] + 1, p["taps"]), np.float32)
    check(lib().gm_resampler_design(C.byref(c), _p(table)), "gm_resampler_design")
    return table


def _samples(samples):
    s = np.ascontiguousarray(samples)
    if s.dtype == np.int8:
        return s, s.size // 2, FMT_I8_IQ
    s = np.ascontiguousarray(s, np.complex64)
    return s, s.size, FMT_C32


class Resampler(Stage):
    _NAME = "resampler"

    def __init__(self, up, down, device=None, **cfg):
        unknown = set(cfg) - set(_KEYS)
        if unknown:
            raise TypeError("unknown resampler settings: %s" % sorted(unknown))
        _lib.init(device if device is not None else (_lib._initialised or 0))
        self._cfg = _cfg(up, down, **cfg)
        p = plan(up, down, **cfg)
        self.up, self.down, self.n_taps, self.n_phases = p["up"], p["down"], p["taps"], p["n_phases"]
        self._open(self._cfg)

    @classmethod
    def from_rates(cls, fs_in, fs_out, device=None, max_denominator=1 << 24, **cfg):
        """fs_out / fs_in as an exact fraction (fractions.Fraction of the two values as given: pass integers or Fractions for rates
        such as 16367600 -> 16368000; floats are taken at their binary value and limited to max_denominator)."""
        ratio = (Fraction(fs_out) / Fraction(fs_in)).limit_denominator(max_denominator)
        return cls(ratio.numerator, ratio.denominator, device=device, **cfg)

    def process(self, samples):
        """samples: complex64 array, or int8 array of interleaved I/Q -> complex64 array of this call's outputs (synchronous)."""
        s, n, fmt = _samples(samples)
        out = np.zeros(n * self.up // self.down + 2, np.complex64)      # a call never delivers more than n * up / down + 1
        got = C.c_size_t(0)
        self._call("process", _p(s), fmt, n, _p(out), out.size, C.byref(got))
        return out[:got.value].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_cap, stream=None):
        """device pointers; asynchronous on `stream` (None: the handle's own); returns the number of outputs written to d_out"""
        got = C.c_size_t(0)
        self._call("process_dev", d_in, fmt, n_in, d_out, out_cap, C.byref(got), stream)
        return got.value

    def taps(self):
        """the [n_phases + 1][taps] float32 words the device uses"""
        table = np.zeros((self.n_phases + 1, self.n_taps), np.float32)
        self._call("taps", _p(table))
        return table

    def stats(self):
        """inputs taken, outputs delivered, inputs blanked since the creation or the last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blanked")
