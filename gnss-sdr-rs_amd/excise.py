"""Narrowband interference excision over the C ABI (gm_excisor, include/gnss_mi355x.h): a 50 % overlap-add filter bank with sine
windows and a per-bin gain, and a device-side adaptive step that sets the gains from a Welch periodogram.  An Excisor turns a stream of
complex64 or int8-IQ samples into complex64 samples at the same rate and the same sample index; every output is defined by absolute
sample indices alone, so the words do not depend on how the stream is cut into calls."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FMT_C32, FMT_I8_IQ, ExcisorBlockCfg, ExcisorCfg, check, lib
from ._stage import Stage, _p

_KEYS = ("guard_bins", "threshold_factor", "blank_threshold")


_HIP = None


def _hip():
    """the HIP runtime the library already loaded: Excisor.adapt keeps one plain device buffer for its host samples"""
    global _HIP
    if _HIP is None:
        h = C.CDLL("libamdhip64.so.7")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        _HIP = h
    return _HIP


def _cfg(block=0, guard_bins=0, threshold_factor=0.0, blank_threshold=0.0):
    return ExcisorCfg(int(block), int(guard_bins), float(threshold_factor), float(blank_threshold), (C.c_uint32 * 4)(0, 0, 0, 0))


def plan(block=0, inputs_so_far=0, n_in=0, **cfg):
    """gm_excisor_plan (host only, no device): the argument rules, the resolved defaults and the number of outputs that n_in more
    inputs deliver to a stream that has taken inputs_so_far."""
    c = _cfg(block, **cfg)
    b, g, f, n = C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_uint64(0)
    check(lib().gm_excisor_plan(C.byref(c), int(inputs_so_far), int(n_in), C.byref(b), C.byref(g), C.byref(f), C.byref(n)),
          "gm_excisor_plan")
    return dict(block=b.value, guard_bins=g.value, threshold_factor=f.value, n_out=n.value)


def _block_cfg(threshold_factor=0.0, guard_bins=0):
    return ExcisorBlockCfg(float(threshold_factor), int(guard_bins), (C.c_uint32 * 6)(0, 0, 0, 0, 0, 0))


def block_plan(threshold_factor=0.0, guard_bins=0):
    """gm_excisor_block_plan (host only, no device): the block-adapt mode's argument rules and resolved defaults"""
    c = _block_cfg(threshold_factor, guard_bins)
    f, g = C.c_float(0), C.c_uint32(0)
    check(lib().gm_excisor_block_plan(C.byref(c), C.byref(f), C.byref(g)), "gm_excisor_block_plan")
    return dict(threshold_factor=f.value, guard_bins=g.value)


def windows(block=0, **cfg):
    """gm_excisor_windows (host only, no device): the float32 analysis and synthesis windows, [block] each."""
    c = _cfg(block, **cfg)
    B = plan(block, **cfg)["block"]
    wa, ws = np.zeros(B, np.float32), np.zeros(B, np.float32)
    check(lib().gm_excisor_windows(C.byref(c), _p(wa), _p(ws)), "gm_excisor_windows")
    return wa, ws


def _samples(samples):
    s = np.ascontiguousarray(samples)
    if s.dtype == np.int8:
        return s, s.size // 2, FMT_I8_IQ
    s = np.ascontiguousarray(s, np.complex64)
    return s, s.size, FMT_C32


class Excisor(Stage):
    _NAME = "excisor"

    def __init__(self, block=0, device=None, **cfg):
        unknown = set(cfg) - set(_KEYS)
        if unknown:
            raise TypeError("unknown excisor settings: %s" % sorted(unknown))
        _lib.init(device if device is not None else (_lib._initialised or 0))
        self._cfg = _cfg(block, **cfg)
        self._settings = dict(cfg)
        p = plan(block, **cfg)
        self.block, self.guard_bins, self.threshold_factor = p["block"], p["guard_bins"], p["threshold_factor"]
        self._d_adapt, self._adapt_cap, self._base = None, 0, 0
        self._open(self._cfg)

    def close(self):
        super().close()
        if getattr(self, "_d_adapt", None):
            _hip().hipFree(self._d_adapt)
            self._d_adapt = None

    def set_block_adapt(self, threshold_factor=0.0, guard_bins=0):
        """the block-adapt mode on (a mask per block, decided on the device between the two transforms; 0 -> factor 16) or, with
        set_block_adapt(None), off; returns self"""
        if threshold_factor is None:
            self._call("set_block_adapt", None)
        else:
            c = _block_cfg(threshold_factor, guard_bins)
            self._call("set_block_adapt", C.byref(c))
        return self

    def block_stats(self):
        """the block-adapt counters since the creation or the last reset (synchronises)"""
        v = [C.c_uint64(0) for _ in range(4)]
        self._call("block_stats", *[C.byref(c) for c in v])
        return dict(zip(("blocks", "blocks_flagged", "bins_flagged", "bins_zeroed"), (c.value for c in v)))

    def block_capture(self, d_power=None, d_mask=None, cap_blocks=0):
        """arms a capture of the power words (f32 [cap_blocks][block]) and masks (u8 [cap_blocks][block]) of every later process_dev
        into device buffers; both None disarms it"""
        self._call("block_capture", d_power, d_mask, int(cap_blocks))

    def _process_blocks(self, s, n, fmt):
        """process(want_blocks=True): process_dev with a capture armed on plain device buffers of this call's own"""
        hip = _hip()
        H = self.block // 2
        n_blocks = plan(self.block, self.stats()["inputs"] + self._base, n, **self._settings)["n_out"] // H + 1
        sizes = (max(s.nbytes, 1), (n + self.block) * 8, n_blocks * self.block * 4, n_blocks * self.block)
        bufs = []
        try:
            for size in sizes:
                p = C.c_void_p()
                if hip.hipMalloc(C.byref(p), size) != 0:
                    raise MemoryError("hipMalloc")
                bufs.append(p)
            d_in, d_out, d_p, d_m = bufs
            if hip.hipMemcpy(d_in, _p(s), s.nbytes, 1) != 0:
                raise RuntimeError("hipMemcpy")
            self.block_capture(d_p, d_m, n_blocks)
            try:
                got = self.process_dev(d_in, fmt, n, d_out, n + self.block)
                self.synchronize()
            finally:
                self.block_capture(None, None, 0)
            out = np.zeros(got, np.complex64)
            rows = got // H + 1 if got else 0
            power, mask = np.zeros((rows, self.block), np.float32), np.zeros((rows, self.block), np.uint8)
            for host, dev in ((out, d_out), (power, d_p), (mask, d_m)):
                if host.nbytes and hip.hipMemcpy(_p(host), dev, host.nbytes, 2) != 0:
                    raise RuntimeError("hipMemcpy")
            return out, power, mask
        finally:
            for p in bufs:
                hip.hipFree(p)

    def process(self, samples, want_blocks=False):
        """samples: complex64 array, or int8 array of interleaved I/Q -> complex64 array of this call's outputs (synchronous).
        want_blocks (block-adapt mode on): -> (outputs, power float32 [n_seg + 1][block], mask uint8 [n_seg + 1][block]) of the call's
        blocks, empty when the call delivers no segment."""
        s, n, fmt = _samples(samples)
        if want_blocks:
            return self._process_blocks(s, n, fmt)
        out = np.zeros(n + self.block, np.complex64)                    # a call never delivers more than n + H
        got = C.c_size_t(0)
        self._call("process", _p(s), fmt, n, _p(out), out.size, C.byref(got))
        return out[:got.value].copy()

    def process_dev(self, d_in, fmt, n_in, d_out, out_cap, stream=None):
        """device pointers; asynchronous on `stream` (None: the handle's own); returns the number of outputs written to d_out"""
        got = C.c_size_t(0)
        self._call("process_dev", d_in, fmt, n_in, d_out, out_cap, C.byref(got), stream)
        return got.value

    def adapt_dev(self, d_in, fmt, n, stream=None):
        """the adaptive step on n samples in device memory: periodogram, median, mask, gains; enqueued, no host wait"""
        self._call("adapt_dev", d_in, fmt, n, stream)

    def adapt(self, samples):
        """the adaptive step on host samples (copied to a device buffer the object keeps, then adapt_dev on the handle's stream)"""
        s, n, fmt = _samples(samples)
        hip = _hip()
        if self._adapt_cap < s.nbytes:
            self.synchronize()
            if self._d_adapt:
                hip.hipFree(self._d_adapt)
            p = C.c_void_p()
            if hip.hipMalloc(C.byref(p), max(s.nbytes, 1)) != 0:
                raise MemoryError("hipMalloc")
            self._d_adapt, self._adapt_cap = p, s.nbytes
        self.synchronize()                                              # the last adapt has read the buffer
        if hip.hipMemcpy(self._d_adapt, _p(s), s.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy")
        self.adapt_dev(self._d_adapt, fmt, n)

    def set_gains(self, gains):
        g = np.ascontiguousarray(gains, np.float32)
        if g.shape != (self.block,):
            raise ValueError("gains: %d values" % self.block)
        self._call("set_gains", _p(g))

    def gains(self):
        g = np.zeros(self.block, np.float32)
        self._call("gains", _p(g))
        return g

    def psd(self):
        """the last adapt's words: dict of P [block] float32, median, n_flagged, n_zeroed (synchronises)"""
        P = np.zeros(self.block, np.float32)
        med, nf, nz = C.c_float(0), C.c_uint32(0), C.c_uint32(0)
        self._call("psd", _p(P), C.byref(med), C.byref(nf), C.byref(nz))
        return dict(P=P, median=np.float32(med.value), n_flagged=nf.value, n_zeroed=nz.value)

    def reset(self, input_index=0):
        super().reset(input_index)
        self._base = int(input_index)

    def stats(self):
        """inputs taken, outputs delivered, inputs blanked since the creation or the last reset (synchronises)"""
        return self._counters("inputs", "outputs", "blanked")

    def windows(self):
        """the float32 analysis and synthesis window words the device uses"""
        return windows(self.block, **self._settings)
