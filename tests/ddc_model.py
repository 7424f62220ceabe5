"""A numpy restatement of the real-IF down-conversion (gm_ddc, include/gnss_mi355x.h), and its scene.

A helper module like resample_model.py, not a test.  Shared by tests/test_ddc_host.py (CPU) and tests/test_gpu_ddc.py (GPU).

The model restates the definition, not the kernel.  Handed the library's filter table and phasor tables it forms, for the input with
absolute index n,
    Theta_n = (n * inc) mod 2^64 (numpy uint64, wrapping),  k = Theta_n >> 40,  w[n] = Whi[k >> 12] * Wlo[k & 4095]
    p[n] = (fl(xb[n] * re), fl(xb[n] * im))
in numpy float32 with every product and sum rounded on its own — bit for bit what the definition says — and hands p to
resample_model.Model, which forms the filter sum in float64 with the rate converter's positions and counts."""
import math

import numpy as np

import resample_model as RM

TABLE_WORDS = 4096


def phase_inc(mix):
    """inc = floor(frac(mix) * 2^64) in Python integers (the float64 scaling by 2^64 is exact); a frac that rounds to 1 wraps to 0"""
    frac = mix - math.floor(mix)
    return int(math.ldexp(frac, 64)) if frac < 1.0 else 0


def resolve(mix, up, down, **cfg):
    """gm_ddc_plan's argument rules and defaults -> dict (resample_model.resolve's, with mix and inc), or None where they refuse"""
    if not math.isfinite(mix):
        return None
    p = RM.resolve(up, down, **cfg)
    if p is None:
        return None
    p = dict(p)
    p["mix"], p["inc"] = float(mix), phase_inc(float(mix))
    return p


def phasor_tables():
    """(Whi, Wlo) complex64 [4096] as defined: the float64 value rounded once"""
    i = np.arange(TABLE_WORDS, dtype=np.float64)
    hi, lo = 2.0 * np.pi * i / 4096.0, 2.0 * np.pi * i / 16777216.0

    def mk(a):
        w = np.empty(TABLE_WORDS, np.complex64)
        w.real, w.imag = np.cos(a).astype(np.float32), (0.0 - np.sin(a)).astype(np.float32)
        return w
    return mk(hi), mk(lo)


def phase_words(n, inc):
    """k [len(n)] uint32 (24 bits) of the absolute indices n (uint64 array)"""
    with np.errstate(over="ignore"):
        theta = np.asarray(n, np.uint64) * np.uint64(inc)
    return (theta >> np.uint64(40)).astype(np.uint32)


def phasor_of_k(k, whi, wlo):
    """(re, im) float32 arrays of w = Whi[k >> 12] * Wlo[k & 4095]: no fused operation, every product and sum rounded on its own"""
    k = np.asarray(k, np.uint32)
    a, b = np.asarray(whi, np.complex64)[k >> 12], np.asarray(wlo, np.complex64)[k & 4095]
    ar, ai, br, bi = a.real.astype(np.float32), a.imag.astype(np.float32), b.real.astype(np.float32), b.imag.astype(np.float32)
    return (ar * br) - (ai * bi), (ar * bi) + (ai * br)


def indices(first, count):
    """uint64 [count]: first, first + 1, ... (first a Python integer up to 2^62)"""
    return np.uint64(first) + np.arange(count, dtype=np.uint64)


class Model:
    def __init__(self, p, g, whi, wlo, input_index=0):
        self.p, self.whi, self.wlo = p, np.asarray(whi, np.complex64), np.asarray(wlo, np.complex64)
        inner = dict(p)
        inner["thr"] = np.float32(0.0)               # the blanking is this model's: it acts on the real sample
        self.rs = RM.Model(inner, g, input_index)
        self.blanked = 0

    @property
    def inputs(self):
        return self.rs.inputs

    @property
    def outputs(self):
        return self.rs.outputs

    def product(self, x):
        """p[n] complex64 of this call's samples (int8, or float for a stream that is not quantised), and the blanked count"""
        xf = np.asarray(x).reshape(-1).astype(np.float32)
        thr = np.float32(self.p["thr"])
        nb = 0
        if thr > 0:
            hit = (xf * xf) > (thr * thr)
            xf = np.where(hit, np.float32(0.0), xf)
            nb = int(hit.sum())
        re, im = phasor_of_k(phase_words(indices(self.rs.base + self.rs.inputs, xf.size), self.p["inc"]), self.whi, self.wlo)
        return ((xf * re) + 1j * (xf * im)).astype(np.complex64), nb

    def process(self, x):
        """one call -> (y complex128 [n_out], weight float64 [n_out][2]): weight = sum_j |c_j| |p_j| per component"""
        prod, nb = self.product(x)
        self.blanked += nb
        return self.rs.process(prod)


def run(p, g, whi, wlo, x, blocks=None, input_index=0):
    """the whole stream x through a fresh Model, in one call or cut into `blocks` (a block length, repeated) -> (y, weight, model)"""
    m = Model(p, g, whi, wlo, input_index)
    x = np.asarray(x).reshape(-1)
    step = x.size if not blocks else blocks
    ys, ws = [], []
    for s in range(0, max(x.size, 1), max(step, 1)):
        y, w = m.process(x[s:s + step])
        ys.append(y); ws.append(w)
    return np.concatenate(ys), np.concatenate(ws), m


# ---- the tone: what the image rejection and the gain are measured on --------------------------------------------------------------------
FS_IN, F_MIX = 16367600.0, 4130400.0
MIX = 4130400.0 / 16367600.0
TONE_OFFSET, TONE_AMP, TONE_OUTPUTS, TONE_SKIP = 37.0e3, 100.0, 8000, 300


def tone_measure(p, g, whi, wlo):
    """A real carrier of amplitude 100 at f_mix + 37 kHz, not quantised, through the model -> (amplitude of the baseband tone, the
    strongest other line in dB relative to it).  Over 8000 outputs behind the filter's start: the tone is fitted at its known
    frequency under a Blackman window and removed; the strongest line is the largest word of the 8 x zero-padded windowed transform of
    what is left, on the same scale."""
    n_in = (TONE_OUTPUTS + TONE_SKIP + 8) * p["down"] // p["up"] + p["T"]
    n = np.arange(n_in, dtype=np.float64)
    cyc = (F_MIX + TONE_OFFSET) / FS_IN * n
    x = TONE_AMP * np.cos(2.0 * np.pi * (cyc - np.floor(cyc)))
    y, _, _ = run(p, g, whi, wlo, x, blocks=4000)
    y = y[TONE_SKIP:TONE_SKIP + TONE_OUTPUTS]
    assert y.size == TONE_OUTPUTS
    m = np.arange(TONE_SKIP, TONE_SKIP + TONE_OUTPUTS, dtype=np.float64)
    f_out = TONE_OFFSET / (FS_IN * p["up"] / p["down"])            # cycles per output sample
    win = np.blackman(TONE_OUTPUTS)
    e = np.exp(2j * np.pi * f_out * m)
    a = np.sum(win * y * np.conj(e)) / np.sum(win)
    rest = np.fft.fft(win * (y - a * e), 8 * TONE_OUTPUTS) / np.sum(win)
    return float(np.abs(a)), float(20.0 * np.log10(np.abs(rest).max() / np.abs(a)))


# ---- the scene: the capture's format — int8 real at 16.3676 Msps, IF 4.1304 MHz, a C/A period of 16367.6 samples --------------------------
UP, DOWN = 20460, 40919                      # 16367.6 * UP / DOWN = 8184 exactly
N, FS_OUT = 8184, 8184000.0
T_TRUE = 16367.6
PERIODS_IN, M = 12, 10
DOP = np.arange(-2000.0, 2001.0, 500.0)
SAT = dict(code_start=3000.3, doppler=1000.0, phase=0.7)
SIGMA = 30.0
N_IN = int(PERIODS_IN * T_TRUE)
EXPECTED_PHASE = SAT["code_start"] * UP / DOWN                   # 1500.19
TRUE_BIN = int(np.argmin(np.abs(DOP - SAT["doppler"])))


def scene_chips(seed=7):
    """[1][1023] random +-1 chips"""
    return np.where(np.random.default_rng(seed).integers(0, 2, (1, 1023)) > 0, 1, -1).astype(np.int8)


def scene(cn0, seed):
    """int8 real [N_IN]: the code with period T_TRUE input samples from code_start on, on a carrier at f_mix + doppler, in noise of
    sigma 30, rounded and clipped to int8.  A real stream at fs has a noise bandwidth of fs / 2: C / N0 = (A^2 / 2) (fs / 2) / sigma^2."""
    chips = scene_chips()[0]
    rng = np.random.default_rng(seed)
    n = np.arange(N_IN, dtype=np.float64)
    u = (n - SAT["code_start"]) / T_TRUE
    chip = chips[np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = SIGMA * np.sqrt(4.0 * 10.0 ** (cn0 / 10.0) / FS_IN)
    cyc = (F_MIX + SAT["doppler"]) * n / FS_IN
    x = amp * chip * np.cos(2.0 * np.pi * (cyc - np.floor(cyc)) + SAT["phase"]) + SIGMA * rng.standard_normal(N_IN)
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


def scene_tables(n=N, fs=FS_OUT, f_if=0.0):
    """[9][n] complex128 mix tables exp(-j 2 pi (f_if + f) i / fs) of the bins DOP, and their frequencies"""
    i = np.arange(n, dtype=np.float64)
    return np.exp(-2j * np.pi * (f_if + DOP)[:, None] * i[None, :] / fs), (f_if + DOP).astype(np.float32)


def best_cell(mx, am, sm, n=N):
    """(bin, arg-max, peak-to-mean) of the one worker's best cell of [1][1][D] blocks"""
    mx, am, sm = (np.asarray(a).reshape(-1) for a in (mx, am, sm))
    ratio = mx.astype(np.float64) * n / sm.astype(np.float64)
    d = int(np.argmax(ratio))
    return d, int(am[d]), float(ratio[d])
