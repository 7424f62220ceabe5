"""Real-IF down-conversion over the C ABI (gm_ddc, include/gnss_mi355x.h): the first block of a receiver for IF-sampled data.  A Ddc
turns a stream of int8 REAL samples at fs_in, carrier at an intermediate frequency, into complex64 samples at complex baseband at
fs_in * up / down: blank, an exact integer NCO, then the resampler's centred polyphase filter.  Every output is defined by absolute
sample indices alone, so the words do not depend on how the stream is cut into calls."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib
from ._lib import DdcCfg, check, lib
from ._stage import Stage, _p

_KEYS = ("taps", "n_phases", "cutoff", "kaiser_beta", "blank_threshold")
TABLE_WORDS = 4096


def _cfg(mix_cycles_per_sample, up, down, taps=0, n_phases=0, cutoff=0.0, kaiser_beta=0.0, blank_threshold=0.0):
    return DdcCfg(float(mix_cycles_per_sample), int(up), int(down), int(taps), int(n_phases), float(cutoff), float(kaiser_beta),
                  float(blank_threshold), 0)


def plan(mix_cycles_per_sample, up, down, inputs_so_far=0, n_in=0, **cfg):
    """gm_ddc_plan (host only, no device): the argument rules, the reduced ratio, the defaults, the NCO's 64-bit phase increment and
    the number of outputs that n_in more inputs deliver to a stream that has taken inputs_so_far."""
    c = _cfg(mix_cycles_per_sample, up, down, **cfg)
    u, d, t, ph, inc, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().gm_ddc_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(u), C.byref(d), C.byref(t), C.byref(ph), C.byref(inc),
                            C.byref(n)), "gm_ddc_plan")
    return dict(up=u.value, down=d.value, taps=t.value, n_phases=ph.value, phase_inc=inc.value, n_out=n.value)


def phasor_tables():
    """the two 4096-word complex64 tables every handle uses (host only, no device): Whi[h] = exp(-j 2 pi h / 2^12) and
    Wlo[l] = exp(-j 2 pi l / 2^24)"""
    whi, wlo = np.zeros(TABLE_WORDS, np.complex64), np.zeros(TABLE_WORDS, np.complex64)
    check(lib().gm_ddc_tables(None, None, _p(whi), _p(wlo)), "gm_ddc_tables")
    return whi, wlo


class Ddc(Stage):
    _NAME = "ddc"

    def __init__(self, mix_cycles_per_sample, up, down, device=None, **cfg):
        unknown = set(cfg) - set(_KEYS)
        if unknown:
            raise TypeError("unknown down-converter settings: %s" % sorted(unknown))
        _lib.init(device if device is not None else (_lib._initialised or 0))
        self._cfg = _cfg(mix_cycles_per_sample, up, down, **cfg)
        p = plan(mix_cycles_per_sample, up, down, **cfg)
        self.up, self.down, self.n_taps, self.n_phases, self.phase_inc = p["up"], p["down"], p["taps"], p["n_phases"], p["phase_inc"]
        self.mix_cycles_per_sample = float(mix_cycles_per_sample)
        self._open(self._cfg)

    @classmethod
    def from_rates(cls, fs_in, fs_out, f_mix_hz, device=None, max_denominator=1 << 24, **cfg):
        """fs_out / fs_in as an exact fraction, as Resampler.from_rates takes it (pass integers or Fractions for rates such as
        16367600 -> 8184000); the mix frequency is f_mix_hz / fs_in, the exact fraction rounded once to float64."""
        ratio = (Fraction(fs_out) / Fraction(fs_in)).limit_denominator(max_denominator)
        return cls(float(Fraction(f_mix_hz) / Fraction(fs_in)), ratio.numerator, ratio.denominator, device=device, **cfg)

    def process(self, samples):
        """samples: int8 array of real samples -> complex64 array of this call's outputs (synchronous)."""
        s = np.ascontiguousarray(samples, np.int8).reshape(-1)
        out = np.zeros(s.size * self.up // self.down + 2, np.complex64)     # a call never delivers more than n * up / down + 1
        got = C.c_size_t(0)
        self._call("process", _p(s), s.size, _p(out), out.size, C.byref(got))
        return out[:got.value].copy()

    def process_dev(self, d_in, n_in, d_out, out_cap, stream=None):
        """device pointers (d_in at any byte address); asynchronous on `stream` (None: the handle's own); returns the number of outputs
        written to d_out"""
        got = C.c_size_t(0)
        self._call("process_dev", d_in, n_in, d_out, out_cap, C.byref(got), stream)
        return got.value

    def write_ring(self, ring, block, excisor=None, resampler=None):
        """block: int8 array of real samples.  Down-converter, then the excise.Excisor and the resample.Resampler if given, into the
        ring (gm_ddc_write_ring): ring indices count the last stage's outputs, and the outputs enqueued are returned."""
        s = np.ascontiguousarray(block, np.int8).reshape(-1)
        total = C.c_uint64(0)
        self._call("write_ring", excisor._h if excisor is not None else None, resampler._h if resampler is not None else None,
                   ring._h, _p(s), s.size, C.byref(total))
        return total.value

    def tables(self):
        """the words the device uses: the [n_phases + 1][taps] float32 filter table, and the complex64 phasor tables Whi and Wlo"""
        table = np.zeros((self.n_phases + 1, self.n_taps), np.float32)
        whi, wlo = np.zeros(TABLE_WORDS, np.complex64), np.zeros(TABLE_WORDS, np.complex64)
        self._call("tables", _p(table), _p(whi), _p(wlo))
        return table, whi, wlo

    def stats(self):
        """inputs taken, outputs delivered, inputs blanked since the creation or the last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blanked")
