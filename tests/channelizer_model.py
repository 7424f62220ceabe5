"""A float64 numpy restatement of the polyphase filter bank (gm_channelizer, include/gnss_mi355x.h), and its scene.

A helper module like resample_model.py, not a test.  Shared by tests/test_channelizer_host.py (CPU: gm_channelizer_plan and
gm_channelizer_design against it, the two forms of the definition against each other, the filter's gain, the GLONASS scene) and
tests/test_gpu_channelizer.py (GPU: the device's words against it).

With the settings resolved (resolve) and the L = M P words g:
    total_out(A) = max(0, ceil((A - L/2) / D))                            outputs per channel that exist after A inputs
    output m:  n0 = m D - (L/2 - 1)
      direct:     y_k[m] = sum_{j<L} g[j] xb[n0 + j] exp(-j 2 pi k (n0 + j) / M)
      polyphase:  u[r] = sum_{p<P} g[r + pM] xb[n0 + r + pM];  y_k[m] = sum_{r<M} u[r] exp(-j 2 pi k ((n0 + r) mod M) / M)
    xb = the input after blanking (float32: re*re + im*im > thr*thr, each product and the sum rounded on its own), zero before the
    stream's first sample.
Positions are Python / int64 integers and every phase is taken from an integer reduced mod M; everything else is float64.
Model.process takes the words as given: a GPU test hands it the library's own (gm_channelizer_taps)."""
import math

import numpy as np

DEFAULT_P, DEFAULT_CUTOFF, DEFAULT_BETA = 16, 0.9, 8.0
INDEX_MAX = 1 << 62
SPAN_MAX = 4096


# ---- the settings ------------------------------------------------------------------------------------------------------------------
def resolve(n_channels, decim, channels=None, taps_per_branch=0, cutoff=0.0, kaiser_beta=0.0, blank_threshold=0.0, reserved=0):
    """gm_channelizer_plan's argument rules and defaults -> dict, or None where they say GM_ERR_INVALID_ARG"""
    M, D = n_channels, decim
    if reserved or M not in (4, 8, 16, 32, 64) or not (1 <= D <= M):
        return None
    if taps_per_branch and not (2 <= taps_per_branch <= 32):
        return None
    if not all(math.isfinite(v) for v in (cutoff, kaiser_beta, blank_threshold)):
        return None
    if not (0.0 <= cutoff <= 1.0) or not (0.0 <= kaiser_beta <= 20.0) or not (blank_threshold >= 0.0):
        return None
    if channels is None:
        channels = list(range(M))
    else:
        channels = [int(k) for k in channels]
        if not (1 <= len(channels) <= M) or len(set(channels)) != len(channels) or any(not (0 <= k < M) for k in channels):
            return None
    P = taps_per_branch or DEFAULT_P
    return dict(M=M, D=D, P=P, L=M * P, channels=channels, cutoff=float(np.float32(cutoff)) or DEFAULT_CUTOFF,
                beta=float(np.float32(kaiser_beta)) or DEFAULT_BETA, thr=np.float32(blank_threshold))


def total_out(p, A):
    half = p["L"] // 2
    return 0 if A <= half else -(-(A - half) // p["D"])                       # Python integers: exact at any size


def plan(p, inputs_so_far, n_in):
    """the number of outputs per channel n_in more inputs deliver, or None where the sum exceeds 2^62"""
    if inputs_so_far > INDEX_MAX or n_in > INDEX_MAX or inputs_so_far + n_in > INDEX_MAX:
        return None
    return total_out(p, inputs_so_far + n_in) - total_out(p, inputs_so_far)


def tile_outputs(p):
    """the kernel's tile (gnss_mi355x.h states the rule): where the GPU tests put their block lengths"""
    n = (SPAN_MAX - p["L"]) // p["D"] + 1
    return 1024 if n >= 1024 else 512 if n >= 512 else 256 if n >= 256 else n


# ---- the prototype filter ----------------------------------------------------------------------------------------------------------
def _i0(x):
    """sum_k ((x/2)^k / k!)^2, term by term as the library adds it"""
    h = 0.5 * x
    term = total = 1.0
    for k in range(1, 200):
        term *= (h / k) * (h / k)
        total += term
        if term < 1e-18 * total:
            break
    return total


def design(p):
    """[L] float64 values whose float32 roundings are the library's words: the definition evaluated with the same float64 operations
    in the same order (Python floats, libm's sin and sqrt), so that the comparison is bit for bit"""
    L = p["L"]
    fc = p["cutoff"] / float(p["D"])
    inv_i0 = 1.0 / _i0(p["beta"])
    half = 0.5 * L
    h = []
    total = 0.0
    for j in range(L):
        t = float(j) - (half - 1.0)
        u = t / half
        w = 1.0 - u * u
        x = fc * t
        sinc = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
        v = fc * sinc * _i0(p["beta"] * math.sqrt(w if w > 0.0 else 0.0)) * inv_i0
        h.append(v)
        total += v
    return np.array([v / total for v in h], np.float64)


def design_numpy(p):
    """the same definition through numpy's sinc and i0: an independent evaluation, equal within a few float64 ulps"""
    L = p["L"]
    fc = p["cutoff"] / p["D"]
    t = np.arange(L, dtype=np.float64) - (L / 2 - 1)
    w = np.clip(1.0 - (2.0 * t / L) ** 2, 0.0, None)
    h = np.where(np.abs(t) <= L / 2, fc * np.sinc(fc * t) * np.i0(p["beta"] * np.sqrt(w)) / np.i0(p["beta"]), 0.0)
    return h / h.sum()


# ---- the stream --------------------------------------------------------------------------------------------------------------------
def as_c128(x):
    """complex samples, or int8 interleaved I/Q ([n][2] or flat), as complex128 — what the device's conversion to float32 holds"""
    x = np.asarray(x)
    if x.dtype == np.int8:
        v = x.reshape(-1, 2).astype(np.float64)
        return v[:, 0] + 1j * v[:, 1]
    return x.astype(np.complex64).astype(np.complex128)


def _phasor(e, M):
    """exp(-j 2 pi e / M) for integer arrays e, reduced mod M first: exact at any index"""
    return np.exp(-2j * np.pi * (np.asarray(e, np.int64) % M).astype(np.float64) / M)


class Model:
    def __init__(self, p, g, input_index=0, form="polyphase"):
        self.p, self.g, self.form = p, np.asarray(g, np.float64), form
        assert self.g.shape == (p["L"],)
        self.reset(input_index)

    def reset(self, input_index=0):
        self.base, self.inputs, self.outputs, self.blanked = int(input_index), 0, 0, 0
        self.hist = np.zeros(self.p["L"], np.complex128)

    def blank(self, x):
        """-> (xb, how many were blanked): float32 arithmetic, strictly greater"""
        thr = self.p["thr"]
        if not thr > 0:
            return x, 0
        re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
        hit = (re * re + im * im) > thr * thr
        return np.where(hit, 0.0, x), int(hit.sum())

    def process(self, x):
        """one call -> (y complex128 [C][n_out], weight float64 [n_out]): weight = sum_j |g_j| |xb[n0 + j]|, what the bound of the
        device's float32 arithmetic is stated in"""
        p = self.p
        M, D, P, L, ch = p["M"], p["D"], p["P"], p["L"], np.asarray(p["channels"], np.int64)
        xb, nb = self.blank(as_c128(x))
        A = self.base + self.inputs
        m0, m1 = total_out(p, A), total_out(p, A + xb.size)
        ext = np.concatenate([self.hist, xb])                    # ext[0] is absolute input A - L
        self.hist = ext[-L:].copy()
        self.inputs += xb.size; self.outputs += m1 - m0; self.blanked += nb
        if m1 == m0:
            return np.zeros((ch.size, 0), np.complex128), np.zeros(0)
        n0 = np.array([m * D - (L // 2 - 1) for m in range(m0, m1)], dtype=object)       # Python integers
        rel = np.array([int(v) - (A - L) for v in n0], np.int64)
        q = np.array([int(v) % M for v in n0], np.int64)                                 # n0 mod M, n0 of either sign
        idx = rel[:, None] + np.arange(L)[None, :]
        assert idx.min() >= 0 and idx.max() < ext.size
        X = ext[idx]                                             # [n_out][L]
        weight = (np.abs(self.g)[None, :] * np.abs(X)).sum(axis=1)
        if self.form == "direct":
            e = ch[:, None, None] * (q[None, :, None] + np.arange(L)[None, None, :])     # k (n0 + j), below 2^63 after the reduction of n0
            y = (self.g[None, None, :] * X[None, :, :] * _phasor(e, M)).sum(axis=2)
        else:
            u = (self.g.reshape(P, M)[None, :, :] * X.reshape(-1, P, M)).sum(axis=1)     # [n_out][M]: u[r] = sum_p g[r + pM] x[n0 + r + pM]
            e = ch[:, None, None] * (q[None, :, None] + np.arange(M)[None, None, :])
            y = (u[None, :, :] * _phasor(e, M)).sum(axis=2)
        return y, weight


def run(p, g, x, blocks=None, input_index=0, form="polyphase"):
    """the whole stream x through a fresh Model, in one call or cut into `blocks` (a block length, repeated) -> (y [C][n], weight, model)"""
    m = Model(p, g, input_index, form)
    x = as_c128(x)
    step = x.size if not blocks else blocks
    ys, ws = [], []
    for s in range(0, max(x.size, 1), max(step, 1)):
        y, w = m.process(x[s:s + step])
        ys.append(y); ws.append(w)
    return np.concatenate(ys, axis=1), np.concatenate(ws), m


def tone_gain_db(p, g, f):
    """the gain, in dB, of channel 0 for a complex tone at f cycles per INPUT sample, from the filter's frequency response"""
    j = np.arange(p["L"], dtype=np.float64)
    return 20.0 * np.log10(max(abs(np.sum(np.asarray(g, np.float64) * np.exp(-2j * np.pi * f * j))), 1e-300))


# ---- the GLONASS L1OF code ---------------------------------------------------------------------------------------------------------
def glonass_logic():
    """[511] 0 / 1: nine stages, all ones; each clock the output is stage 7, then stage 5 xor stage 9 enters stage 1"""
    s = [1] * 9
    out = []
    for _ in range(511):
        out.append(s[6])
        s = [s[4] ^ s[8]] + s[:8]
    return np.array(out, np.int8)


def glonass_chips():
    return (1 - 2 * glonass_logic()).astype(np.int8)          # +1 stands for logic 0


# ---- the scene: three L1OF signals on three FDMA carriers of one capture -----------------------------------------------------------
FS, M, D, P = 18.0e6, 32, 9, 16                      # channel spacing fs / M = 562.5 kHz; each plane at 2 Msps
N = 2000                                             # samples of a code period (1 ms) in a plane
PERIODS = 12
SIGMA = 30.0
DOP = np.array([-1000.0, -500.0, 0.0, 500.0, 1000.0])
SIGNALS = [dict(channel=3, doppler=1000.0, code_start=6300, cn0=45.0), dict(channel=4, doppler=-500.0, code_start=900, cn0=60.0),
           dict(channel=27, doppler=0.0, code_start=12600, cn0=42.0)]
EMPTY = 10
K_SEARCH, M_SEARCH = 1, 10                           # a plain search: K = 1 coherent period, M = 10 non-coherent sums
N_IN = PERIODS * N * D                               # 216000 inputs: total_out = (216000 - 256) / 9 -> 23972 outputs, 11 whole periods + 1972
EXPECTED = {3: (700, 4), 4: (100, 1), 27: (1400, 2)}     # channel -> (code phase = code_start / D, Doppler bin)
DETECT = 7.0


def scene(seed):
    """int8 [N_IN][2]: noise of sigma 30 per component + the three signals, rounded and clipped"""
    rng = np.random.default_rng(seed)
    chips = glonass_chips().astype(np.float64)
    n = np.arange(N_IN, dtype=np.float64)
    x = SIGMA * (rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN))
    for s in SIGNALS:
        k = s["channel"] if s["channel"] < M // 2 else s["channel"] - M
        f = k * FS / M + s["doppler"]
        amp = SIGMA * np.sqrt(2.0 * 10.0 ** (s["cn0"] / 10.0) / FS)          # C/N0 against the noise density 2 sigma^2 / fs
        u = (n - s["code_start"]) / (N * D)
        chip = chips[np.minimum(510, np.floor((u - np.floor(u)) * 511.0).astype(np.int64))]
        cyc = f * n / FS
        x = x + amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)))
    out = np.stack([np.clip(np.rint(x.real), -128, 127), np.clip(np.rint(x.imag), -128, 127)], axis=1)
    return out.astype(np.int8)


def sampled_code():
    """[N] the replica at 2 Msps: chip floor(n * 511 / N)"""
    return glonass_chips()[(np.arange(N) * 511) // N].astype(np.float64)


def search(y, replica=None, tables=None):
    """a plain search of one plane y (complex, at least M_SEARCH * N samples): for each Doppler bin, the circular correlation of each
    of M_SEARCH periods with the replica, |.|^2 summed over the periods -> (bin, code phase, peak-to-mean) of the best cell.
    replica [N], tables [len(DOP)][N]: a handle's own sampled chips and mix tables in place of the model's"""
    y = np.asarray(y, np.complex128)[:M_SEARCH * N].reshape(M_SEARCH, N)
    cf = np.conj(np.fft.fft(sampled_code() if replica is None else np.asarray(replica, np.float64)))
    n = np.arange(N, dtype=np.float64)
    best = (0, 0, 0.0)
    for b, f in enumerate(DOP):
        mix = np.exp(-2j * np.pi * f * n / (FS / D)) if tables is None else np.asarray(tables[b], np.complex128)
        power = (np.abs(np.fft.ifft(np.fft.fft(y * mix[None, :], axis=1) * cf[None, :], axis=1)) ** 2).sum(axis=0)
        ratio = float(power.max() * N / power.sum())
        if ratio > best[2]:
            best = (b, int(np.argmax(power)), ratio)
    return best
