"""The polyphase filter bank over the C ABI (gm_channelizer, include/gnss_mi355x.h): M sub-bands of one complex64 or int8-IQ stream,
each delivered as its own complex64 stream at fs / D.  Channel k is centred at k fs / M (k >= M/2: (k - M) fs / M); every output is
defined by absolute sample indices alone, so the words do not depend on how the stream is cut into calls.  With glonass_code() and
glonass_channels(M) it is the front of a GLONASS L1OF search: fourteen FDMA carriers of one capture, one plane each."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ChannelizerCfg, check, lib
from ._stage import Stage, _p
from .resample import _samples

_KEYS = ("taps_per_branch", "cutoff", "kaiser_beta", "blank_threshold")


def _cfg(n_channels, decim, channels=None, taps_per_branch=0, cutoff=0.0, kaiser_beta=0.0, blank_threshold=0.0):
    """-> (cfg, the list it points at: keep it alive as long as the cfg)"""
    c = ChannelizerCfg(int(n_channels), int(decim), int(taps_per_branch), float(cutoff), float(kaiser_beta), float(blank_threshold), 0, 0, None)
    keep = None
    if channels is not None:
        keep = (C.c_uint32 * max(len(channels), 1))(*[int(k) for k in channels])
        c.n_out_channels = len(channels)
        c.out_channels = C.cast(keep, C.POINTER(C.c_uint32))
    return c, keep


def plan(n_channels, decim, inputs_so_far=0, n_in=0, channels=None, **cfg):
    """gm_channelizer_plan (host only, no device): the argument rules, the defaults and the number of outputs per channel that n_in more
    inputs deliver to a stream that has taken inputs_so_far."""
    c, keep = _cfg(n_channels, decim, channels, **cfg)
    nc, p, taps, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    check(lib().gm_channelizer_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(nc), C.byref(p), C.byref(taps), C.byref(n)),
          "gm_channelizer_plan")
    return dict(n_out_channels=nc.value, taps_per_branch=p.value, n_taps=taps.value, n_out=n.value)


def design(n_channels, decim, **cfg):
    """gm_channelizer_design (host only, no device): the L = M P float32 words of the prototype filter."""
    p = plan(n_channels, decim, **cfg)
    c, keep = _cfg(n_channels, decim, None, **cfg)
    taps = np.zeros(p["n_taps"], np.float32)
    check(lib().gm_channelizer_design(C.byref(c), _p(taps)), "gm_channelizer_design")
    return taps


def glonass_channels(n_channels):
    """the channel indices of the L1OF carriers k = -7 .. 6, in that order, in a bank of n_channels whose channel spacing fs / M is the
    562.5 kHz of the carriers (fs = M * 562.5 kHz, centred on 1602 MHz)"""
    if n_channels < 16:
        raise ValueError("fourteen carriers need at least 16 channels")
    return [k % n_channels for k in range(-7, 7)]


def glonass_code():
    """the 511 chips (+-1, +1 for logic 0) of the L1OF ranging code, [1][511] int8: what AcquisitionEngine takes as `codes`"""
    chips = np.zeros((1, 511), np.int8)
    check(lib().gm_glonass_code(_p(chips)), "gm_glonass_code")
    return chips


class Channelizer(Stage):
    _NAME = "channelizer"

    def __init__(self, n_channels, decim, channels=None, device=None, **cfg):
        unknown = set(cfg) - set(_KEYS)
        if unknown:
            raise TypeError("unknown channelizer settings: %s" % sorted(unknown))
        _lib.init(device if device is not None else (_lib._initialised or 0))
        p = plan(n_channels, decim, channels=channels, **cfg)
        c, keep = _cfg(n_channels, decim, channels, **cfg)
        self.n_channels, self.decim = int(n_channels), int(decim)
        self.channels = [int(k) for k in channels] if channels is not None else list(range(self.n_channels))
        self.taps_per_branch, self.n_taps = p["taps_per_branch"], p["n_taps"]
        self._open(c)

    def process(self, samples):
        """samples: complex64 array, or int8 array of interleaved I/Q -> complex64 [C, n]: this call's outputs, a row per listed
        channel (synchronous)."""
        s, n, fmt = _samples(samples)
        cap = n // self.decim + 2                                      # a call never delivers more than n / D + 1
        out = np.zeros((len(self.channels), cap), np.complex64)
        got = C.c_size_t(0)
        self._call("process", _p(s), fmt, n, _p(out), cap, C.byref(got))
        return out[:, :got.value].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_stride, out_cap, stream=None):
        """device pointers; d_out is [C][out_stride] complex64; asynchronous on `stream` (None: the handle's own); returns the number
        of outputs written to every plane"""
        got = C.c_size_t(0)
        self._call("process_dev", d_in, fmt, n_in, d_out, out_stride, out_cap, C.byref(got), stream)
        return got.value

    def taps(self):
        """the L float32 words the device uses"""
        taps = np.zeros(self.n_taps, np.float32)
        self._call("taps", _p(taps))
        return taps

    def stats(self):
        """inputs taken, outputs delivered per channel, inputs blanked since the creation or the last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blanked")
