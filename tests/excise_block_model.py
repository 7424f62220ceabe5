"""A numpy restatement of the excisor's block-adapt mode (gm_excisor_set_block_adapt, include/gnss_mi355x.h), on top of excise_model.py.

A helper module, not a test.  Shared by tests/test_excise_block_host.py (CPU) and tests/test_gpu_excise_block.py (GPU).

Per block b of the stream (excise_model's blocks: block b covers absolute inputs [(b - 1) H, (b + 1) H)):
    p[k]   = re*re + im*im of X_b = fft(wa xb)                 float32 on the words it is given: each product and the sum rounded
    med_b  = the element of rank (B - 1) div 2 of p, the low 16 bits of its float32 word cleared
    flag   = p > factor * med_b                                one float32 product, strictly greater
    m_b    = 0 within guard bins (circular) of a flag, 1 elsewhere
    Y_b    = (g m_b) X_b, then the inverse transform and the overlap-add of excise_model.Model
    counters: block b is counted once, when segment b - 1 is delivered; block 0 never
decide() is the float32 rule on given power words (a GPU test hands it the device's own); BlockModel is the float64 stream with a gain
row per block, which either decides the masks itself (from its float64 spectrum rounded to float32) or takes them as given."""
import numpy as np

import excise_model as EM

DEFAULT_FACTOR = 16.0
COUNTERS = ("blocks", "blocks_flagged", "bins_flagged", "bins_zeroed")


def resolve(threshold_factor=0.0, guard_bins=0, reserved=(0, 0, 0, 0, 0, 0)):
    """gm_excisor_block_plan's argument rules and defaults -> dict, or None where they say GM_ERR_INVALID_ARG"""
    if any(reserved) or not (0 <= guard_bins <= 16) or not (threshold_factor == 0.0 or threshold_factor > 1.0):
        return None
    return dict(factor=float(np.float32(threshold_factor)) or DEFAULT_FACTOR, guard=guard_bins)


def power(X):
    """float32 power words of a spectrum given as complex64 words"""
    X = np.asarray(X, np.complex64)
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def median_word(p):
    """med_b of float32 power words [..., B]: the rank-(B - 1) div 2 element by bit pattern, low 16 bits cleared"""
    w = np.ascontiguousarray(p, np.float32).view(np.uint32)
    B = w.shape[-1]
    s = np.sort(w, axis=-1)[..., (B - 1) // 2]
    return (s & np.uint32(0xFFFF0000)).view(np.float32)


def decide(p, factor, guard):
    """float32 power words [..., B] -> (med [...], flag bool [..., B], mask uint8 [..., B]: 1 kept, 0 zeroed)"""
    p = np.ascontiguousarray(p, np.float32)
    med = median_word(p)
    with np.errstate(invalid="ignore", over="ignore"):
        level = np.float32(factor) * med
        flag = p > level[..., None]
    zero = np.zeros(p.shape, bool)
    for d in range(-guard, guard + 1):
        zero |= np.roll(flag, d, axis=-1)
    return med, flag, np.where(zero, 0, 1).astype(np.uint8)


def count(flags, masks):
    """the counters of a run from the flags and masks [J][B] of its calls' blocks, the first block of every call left out: block j > 0
    of a call is the second block of segment j - 1, which that call delivers"""
    c = dict.fromkeys(COUNTERS, 0)
    for f, m in zip(flags, masks):
        f, m = np.asarray(f)[1:], np.asarray(m)[1:]
        c["blocks"] += len(f)
        c["blocks_flagged"] += int(f.any(axis=-1).sum()) if len(f) else 0
        c["bins_flagged"] += int(f.sum())
        c["bins_zeroed"] += int((m == 0).sum())
    return c


class BlockModel(EM.Model):
    """excise_model.Model with a mask per block.  process(x, masks=None): masks [n_seg + 1][B] (the device's own) or None, in which
    case the model decides them from its float64 spectrum rounded to float32 words.  -> (y, scale, power float64 [n_seg + 1][B],
    masks uint8 [n_seg + 1][B]); the counters run in self.counters."""

    def __init__(self, p, factor=DEFAULT_FACTOR, guard=0, **kw):
        self.factor, self.guard = factor, guard
        super().__init__(p, **kw)

    def reset(self, input_index=0):
        super().reset(input_index)
        self.counters = dict.fromkeys(COUNTERS, 0)

    def process(self, x, masks=None):
        B, H = self.B, self.B // 2
        xb, nb = EM.blank(EM.as_c128(x), self.p["thr"])
        A = self.base + self.inputs
        m0, m1 = EM.total_out(B, A), EM.total_out(B, A + xb.size)
        ext = np.concatenate([self.hist, xb])
        self.hist = ext[-3 * H:].copy()
        self.inputs += xb.size; self.outputs += m1 - m0; self.blanked += nb
        if m1 == m0:
            return np.zeros(0, np.complex128), np.zeros(0), np.zeros((0, B)), np.zeros((0, B), np.uint8)
        s0, s1 = m0 // H, m1 // H
        first = (s0 - 1) * H - (A - 3 * H)
        blocks = np.stack([ext[first + k * H:first + k * H + B] for k in range(s1 - s0 + 1)])
        X = np.fft.fft(self.wa[None, :] * blocks, axis=1)
        P = X.real * X.real + X.imag * X.imag
        if masks is None:
            _, flag, masks = decide(power(X.astype(np.complex64)), self.factor, self.guard)
            for k, v in count([flag], [masks]).items():
                self.counters[k] += v
        masks = np.asarray(masks, np.uint8)
        assert masks.shape == P.shape
        u = np.fft.ifft((self.g[None, :] * masks) * X, axis=1) * B
        y = self.ws[None, H:] * u[:-1, H:] + self.ws[None, :H] * u[1:, :H]
        mag = np.abs(ext[first:first + (s1 - s0 + 2) * H]).reshape(-1, H).max(axis=1)
        scale = np.maximum(np.maximum(mag[:-2], mag[1:-1]), mag[2:])
        return y.reshape(-1), np.repeat(scale, H), P, masks


def run(p, x, factor=DEFAULT_FACTOR, guard=0, masks=None, **kw):
    """the whole of x in one call through a fresh BlockModel -> (y, scale, power, masks, model)"""
    m = BlockModel(p, factor, guard, **kw)
    y, scale, P, masks = m.process(x, masks)
    return y, scale, P, masks, m


# ---- the scenes: a CW that moves -------------------------------------------------------------------------------------------------------
SWEEP_HZ = (-800e3, 800e3)
HOP_SAMPLES = 700


def _jam(x, cycles, jn_db):
    return (x + np.sqrt(2.0 * 10.0 ** (jn_db / 10.0)) * np.exp(2j * np.pi * (cycles - np.floor(cycles)) + 0.3j)).astype(np.complex64)


def sweep_scene(seed, jn_db=30.0):
    """excise_model's clean scene plus a CW that sweeps linearly from -800 kHz to +800 kHz over the N_IN samples"""
    n = np.arange(EM.N_IN, dtype=np.float64)
    f0, f1 = SWEEP_HZ
    cycles = (f0 * n + 0.5 * (f1 - f0) * n * n / EM.N_IN) / EM.FS
    return _jam(EM.scene(seed).astype(np.complex128), cycles, jn_db)


def hop_scene(seed, jn_db=30.0):
    """... plus a CW that takes a new frequency, uniform in +-800 kHz, every 700 samples (phase-continuous)"""
    rng = np.random.default_rng(1000 + seed)
    f = rng.uniform(SWEEP_HZ[0], SWEEP_HZ[1], EM.N_IN // HOP_SAMPLES + 1)
    cycles = np.cumsum(np.repeat(f, HOP_SAMPLES)[:EM.N_IN]) / EM.FS
    return _jam(EM.scene(seed).astype(np.complex128), cycles, jn_db)


def excise_blocks(x, block=1024, factor=DEFAULT_FACTOR, guard=2):
    """the per-block rule on the whole of x -> (the first DWELL outputs complex64, flags' masks [J][B], the model)"""
    y, _, _, masks, m = run(EM.resolve(block), x, factor, guard)
    assert y.size >= EM.DWELL
    return y[:EM.DWELL].astype(np.complex64), masks, m
