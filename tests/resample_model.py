"""A float64 numpy restatement of the polyphase rate conversion and pulse blanking (gm_resampler, include/gnss_mi355x.h), and its scene.

A helper module like acq_cancel_model.py, not a test.  Shared by tests/test_resample_host.py (CPU: gm_resampler_plan and
gm_resampler_design against it, the filter's quality, the scene that motivates the entry) and tests/test_gpu_resample.py (GPU: the
device's words against it).

The model restates the definition, not the kernel.  With the settings resolved (resolve) and a table g [PHI + 1][T]:
    total_out(A) = max(0, ceil((A - T/2) up / down))                       outputs that exist after A inputs
    output m:  pos = m down,  i0 = pos div up,  r = pos mod up,  q = r PHI,  phi = q div up,  alpha = float32(q mod up / up)
               c_j = g[phi][j] + alpha (g[phi+1][j] - g[phi][j]),   y[m] = sum_j c_j xb[i0 - (T/2 - 1) + j]
    xb = the input after blanking (float32: re*re + im*im > thr*thr, each product and the sum rounded on its own), zero before the
    stream's first sample.
Positions are Python / int64 integers; everything else is float64.  Model.process takes the table as given: a GPU test hands it the
library's own words (gm_resampler_taps), so the table's rounding drops out of the comparison."""
import math

import numpy as np

DEFAULT_PHASES, DEFAULT_CUTOFF, DEFAULT_BETA = 256, 0.9, 8.0
INDEX_MAX = 1 << 62


# ---- the settings ------------------------------------------------------------------------------------------------------------------
def resolve(up, down, taps=0, n_phases=0, cutoff=0.0, kaiser_beta=0.0, blank_threshold=0.0, reserved=0):
    """gm_resampler_plan's argument rules and defaults -> dict, or None where they say GM_ERR_INVALID_ARG"""
    if reserved or not (1 <= up <= 1 << 24) or not (1 <= down <= 1 << 24):
        return None
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up > 16 * down or down > 16 * up:
        return None
    if taps:
        if taps % 8 or not (8 <= taps <= 256):
            return None
    else:
        taps = min(256, 32 * (-(-down // up) if down > up else 1))
    if n_phases:
        if not (16 <= n_phases <= 1024) or n_phases & (n_phases - 1):
            return None
    else:
        n_phases = DEFAULT_PHASES
    if not (0.0 <= cutoff <= 1.0) or not (0.0 <= kaiser_beta <= 20.0) or not (blank_threshold >= 0.0):
        return None
    return dict(up=up, down=down, T=taps, PHI=n_phases, cutoff=float(np.float32(cutoff)) or DEFAULT_CUTOFF,
                beta=float(np.float32(kaiser_beta)) or DEFAULT_BETA, thr=np.float32(blank_threshold))


def total_out(p, A):
    half = p["T"] // 2
    return 0 if A <= half else -(-(A - half) * p["up"] // p["down"])           # Python integers: exact at any size


def plan(p, inputs_so_far, n_in):
    """the number of outputs n_in more inputs deliver, or None where the sum exceeds 2^62"""
    if inputs_so_far > INDEX_MAX or n_in > INDEX_MAX or inputs_so_far + n_in > INDEX_MAX:
        return None
    return total_out(p, inputs_so_far + n_in) - total_out(p, inputs_so_far)


def tile_outputs(p):
    """the kernel's tile (gnss_mi355x.h states the rule): where the GPU tests put their block lengths"""
    n = (4096 - p["T"] - 1) * p["up"] // p["down"] + 1
    return 1024 if n >= 1024 else 512 if n >= 512 else 256 if n >= 256 else n


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _h(p, t):
    T = p["T"]
    fc = p["cutoff"] * min(1.0, p["up"] / p["down"])
    w = np.clip(1.0 - (2.0 * t / T) ** 2, 0.0, None)
    return np.where(np.abs(t) <= T / 2, fc * np.sinc(fc * t) * np.i0(p["beta"] * np.sqrt(w)) / np.i0(p["beta"]), 0.0)


def table(p):
    """[PHI + 1][T] float64, every row divided by its own sum (the library rounds each word once to float32)"""
    T, PHI = p["T"], p["PHI"]
    t = np.arange(T, dtype=np.float64)[None, :] - (T / 2 - 1) - np.arange(PHI + 1, dtype=np.float64)[:, None] / PHI
    g = _h(p, t)
    return g / g.sum(axis=1, keepdims=True)


def exact_coeffs(p, r):
    """[len(r)][T] float64: the filter evaluated AT the fractional position r / up of every output (no table, no blending), every row
    divided by its own sum"""
    T = p["T"]
    t = np.arange(T, dtype=np.float64)[None, :] - (T / 2 - 1) - (np.asarray(r, np.float64) / p["up"])[:, None]
    g = _h(p, t)
    return g / g.sum(axis=1, keepdims=True)


# ---- the stream --------------------------------------------------------------------------------------------------------------------
def as_c128(x):
    """complex samples, or int8 interleaved I/Q ([n][2] or flat), as complex128 — what the device's conversion to float32 holds"""
    x = np.asarray(x)
    if x.dtype == np.int8:
        v = x.reshape(-1, 2).astype(np.float64)
        return v[:, 0] + 1j * v[:, 1]
    return x.astype(np.complex64).astype(np.complex128)


def positions(p, m):
    """int64 arrays (i0, r, phi) and float64 alpha (the float32 value) of outputs m (int64 array); m = a up + m' keeps every product
    below 2^63"""
    up, down, PHI = p["up"], p["down"], p["PHI"]
    m = np.asarray(m, np.int64)
    a, mp = m // up, m % up
    pos = mp * down
    i0 = a * down + pos // up
    r = pos % up
    q = r * PHI
    alpha = ((q % up).astype(np.float64) / np.float64(up)).astype(np.float32).astype(np.float64)
    return i0, r, q // up, alpha


class Model:
    def __init__(self, p, g, input_index=0):
        self.p, self.g = p, np.asarray(g, np.float64)
        assert self.g.shape == (p["PHI"] + 1, p["T"])
        self.reset(input_index)

    def reset(self, input_index=0):
        self.base, self.inputs, self.outputs, self.blanked = int(input_index), 0, 0, 0
        self.hist = np.zeros(self.p["T"], np.complex128)

    def blank(self, x):
        """-> (xb, how many were blanked): float32 arithmetic, strictly greater"""
        thr = self.p["thr"]
        if not thr > 0:
            return x, 0
        re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
        hit = (re * re + im * im) > thr * thr
        return np.where(hit, 0.0, x), int(hit.sum())

    def process(self, x, exact=False):
        """one call -> (y complex128 [n_out], weight float64 [n_out][2]): weight = sum_j |c_j| |xb_j| per component, what the bound of
        the device's float32 sum is stated in.  exact: exact_coeffs in place of the blended table rows."""
        p, T = self.p, self.p["T"]
        xb, nb = self.blank(as_c128(x))
        A = self.base + self.inputs
        m0, m1 = total_out(p, A), total_out(p, A + xb.size)
        ext = np.concatenate([self.hist, xb])                    # ext[0] is absolute input A - T
        self.hist = ext[-T:].copy()
        self.inputs += xb.size; self.outputs += m1 - m0; self.blanked += nb
        if m1 == m0:
            return np.zeros(0, np.complex128), np.zeros((0, 2))
        i0, r, phi, alpha = positions(p, np.arange(m0, m1, dtype=np.int64))
        c = exact_coeffs(p, r) if exact else self.g[phi] + alpha[:, None] * (self.g[phi + 1] - self.g[phi])
        idx = (i0 - (T // 2 - 1) - (A - T))[:, None] + np.arange(T)[None, :]
        assert idx.min() >= 0 and idx.max() < ext.size
        X = ext[idx]
        y = (c * X).sum(axis=1)
        w = np.stack([(np.abs(c) * np.abs(X.real)).sum(axis=1), (np.abs(c) * np.abs(X.imag)).sum(axis=1)], axis=1)
        return y, w


def run(p, g, x, blocks=None, input_index=0, exact=False):
    """the whole stream x through a fresh Model, in one call or cut into `blocks` (a block length, repeated) -> (y, weight, model)"""
    m = Model(p, g, input_index)
    x = as_c128(x)
    step = x.size if not blocks else blocks
    ys, ws = [], []
    for s in range(0, max(x.size, 1), max(step, 1)):
        y, w = m.process(x[s:s + step], exact)
        ys.append(y); ws.append(w)
    return np.concatenate(ys), np.concatenate(ws), m


def tone_gain_db(p, g, f, n=None):
    """the rms gain, in dB, of a complex tone at f cycles per INPUT sample: over the outputs whose taps lie inside the tone (a tone in
    the stop band comes out as the phases' residues, whose rms is the aliased power)"""
    n = n or 40 * p["T"] + 4000
    x = np.exp(2j * np.pi * f * np.arange(n))
    y, _, _ = run(p, g, x)
    skip = -(-p["T"] * p["up"] // p["down"])
    y = y[skip:]
    return 10.0 * np.log10(np.mean(np.abs(y) ** 2))


# ---- the scene: a code period that is not a whole number of samples ------------------------------------------------------------------
N, FS = 2048, 2.048e6
T_TRUE = N - 0.4
UP, DOWN = 5120, 5119               # T_TRUE * UP / DOWN = N exactly
PERIODS = 40
DOP = np.array([-400.0, 0.0, 400.0])
SAT = dict(worker=0, code_start=700.3, doppler=60.0, phase=0.7)
N_IN = PERIODS * N + 64             # inputs: 40 whole periods of the resampled dwell need PERIODS * N * DOWN / UP + T / 2 of them


def scene_codes(seed=7):
    """[2][1023] random +-1 chips: worker 0 is in the scene, worker 1 is not"""
    return np.where(np.random.default_rng(seed).integers(0, 2, (2, 1023)) > 0, 1, -1).astype(np.int8)


def scene(cn0, seed):
    """complex64 [N_IN] at baseband: worker 0's code with period T_TRUE input samples from code_start on, + unit-variance-per-component
    noise"""
    chips = scene_codes()
    rng = np.random.default_rng(seed)
    n = np.arange(N_IN, dtype=np.float64)
    u = (n - SAT["code_start"]) / T_TRUE
    chip = chips[SAT["worker"]][np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = np.sqrt(2.0 * 10.0 ** (cn0 / 10.0) / FS)
    cyc = SAT["doppler"] * n / FS
    sig = amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * SAT["phase"])
    return (sig + rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN)).astype(np.complex64)


def scene_tables(fs=FS):
    """[3][N] complex128 mix tables exp(-j 2 pi f n / fs) of the bins DOP (f_if = 0), and their frequencies"""
    n = np.arange(N, dtype=np.float64)
    return np.exp(-2j * np.pi * DOP[:, None] * n[None, :] / fs), DOP.astype(np.float32)


def sampled_codes(chips):
    """[P][N] the replicas as the library samples them at N samples a period (acq_model.sample_codes with code_rate = 1023 fs / N)"""
    import acq_model as AM
    return AM.sample_codes(chips, 1023.0 * FS / N, FS, N)


def best_cell(mx, am, sm, w):
    """(bin, arg-max, peak-to-mean) of worker w's best cell of [P][1][D] (or [P][D]) blocks"""
    mx, am, sm = (np.asarray(a).reshape(2, -1) for a in (mx, am, sm))
    ratio = mx[w].astype(np.float64) * N / sm[w].astype(np.float64)
    d = int(np.argmax(ratio))
    return d, int(am[w][d]), float(ratio[d])


EXPECTED_PHASE = int(round(SAT["code_start"] * UP / DOWN))      # 700
