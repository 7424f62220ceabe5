"""A float64 numpy restatement of the fine Doppler from per-period prompts (gm_acq_refine_doppler), and the truth scenes.

A helper module like acq_model.py (which it imports and does not edit), not a test.  Shared by tests/test_acq_refine_host.py (CPU: the
argument rules of gm_acq_refine_plan, the model against the simulated Doppler) and tests/test_gpu_refine_doppler.py (GPU: the device's
prompts, spectrum and peak against the model; the truth scenes end to end).

The model restates the definition, not the kernels.  For a worker w, bin d, code phase cp and offset o:
    z[i]   = sum_n x[s[d][o + i] + n] tab[d][n] c_w[(n - cp) mod N]                                i < R_u = G J
    S[j]   = N^2 sum_g | sum_k sigma_k exp(-j 2 pi frac((f_c + delta_j)(s[d][o+gJ+k] - s[d][o+gJ]) / fs)) z[g J + k] |^2
    delta_j = (j - (Z - 1) / 2) step,  step = half_span / ((Z - 1) / 2)
Everything is float64; the only device words it takes are the mix tables (as acq_model.search_model)."""
import numpy as np

import acq_model as AM

N_FREQ_DEFAULT = 257
N_FREQ_MAX = 4097
K_MAX = 32


# ---- the argument rules (gm_acq_refine_plan) ---------------------------------------------------------------------------------------
def default_half_span(table_freq, b, fs, N, K):
    """half the distance from the bin's table_freq to the farther neighbouring bin's, at most fs / (2 N); one bin: fs / (2 N max(K, 1))"""
    tf = np.asarray(table_freq, np.float32).astype(np.float64)
    limit = float(fs) / (2.0 * N)
    if tf.size == 1:
        return float(fs) / (2.0 * N * max(int(K), 1))
    lo = abs(tf[b] - tf[b - 1]) if b > 0 else 0.0
    hi = abs(tf[b + 1] - tf[b]) if b + 1 < tf.size else 0.0
    return min(0.5 * max(lo, hi), limit)


def plan(K, M, fs, N, table_freq, b=0, span_periods=0, n_freq=0, half_span_hz=0.0):
    """dict(span_periods, n_groups, n_freq, half_span_hz, step_hz), or None where the rules say GM_ERR_INVALID_ARG"""
    tf = np.asarray(table_freq, np.float32).reshape(-1)
    fs = float(np.float32(fs))
    half_span_hz = float(np.float32(half_span_hz))
    K = max(int(K), 1)
    if K > K_MAX or M < 1 or N < 1 or tf.size < 1 or not fs > 0.0 or not 0 <= b < tf.size:
        return None
    if K >= 2:
        if span_periods not in (0, K):
            return None
        J, G = K, M
    else:
        J = span_periods or M
        G = M // J
    if J < 2 or G < 1:
        return None
    Z = n_freq or N_FREQ_DEFAULT
    if Z < 3 or Z > N_FREQ_MAX or Z % 2 == 0:
        return None
    limit = fs / (2.0 * N)
    hs = default_half_span(tf, b, fs, N, K) if half_span_hz == 0.0 else half_span_hz
    if not (hs > 0.0 and hs <= limit):
        return None
    return dict(span_periods=J, n_groups=G, n_freq=Z, half_span_hz=hs, step_hz=hs / ((Z - 1) // 2))


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def prompts(x, table_d, code_w, N, starts_d, o, R_u, cp):
    """[R_u] complex128: the circular correlation value at lag cp of each of the periods o .. o + R_u - 1 alone, each read from its
    start.  table_d: [N] the bin's mix table; code_w: [N] the worker's replica as sampled chips; starts_d: [R] the bin's period starts."""
    X = AM.as_c128(x)
    ref = np.asarray(table_d).astype(np.complex128) * np.roll(np.asarray(code_w, np.float64), int(cp))     # c[(n - cp) mod N]
    return np.array([np.sum(X[int(starts_d[o + i]):int(starts_d[o + i]) + N] * ref) for i in range(R_u)])


def grid(Z, half_span):
    step = half_span / ((Z - 1) // 2)
    return (np.arange(Z, dtype=np.float64) - (Z - 1) // 2) * step, step


def spectrum(z, starts_d, o, f_c, fs, N, J, G, Z, half_span, sec=None):
    """[Z] float64: S[j] of the definition on the prompts z [G J]"""
    delta, _ = grid(Z, half_span)
    s = np.asarray(starts_d)[o:o + G * J].astype(np.int64).reshape(G, J)
    dt = (s - s[:, :1]).astype(np.float64)                                         # samples since the group's first period
    sig = np.ones(J, np.float64) if sec is None else np.asarray(sec, np.float64)
    cyc = (np.float64(f_c) + delta)[:, None, None] * dt[None, :, :] / np.float64(fs)
    w = np.exp(-2j * np.pi * (cyc - np.floor(cyc)))                                # [Z][G][J]
    acc = np.sum(w * (sig[None, None, :] * np.asarray(z).reshape(G, J)[None, :, :]), axis=2)
    return np.float64(N) ** 2 * np.sum(acc.real ** 2 + acc.imag ** 2, axis=1)


def peak_interp(S, step):
    """(peak_index, delta_hz, at_edge): the first index of the maximum; a three-point parabola through it unless it is at an end"""
    S = np.asarray(S, np.float64)
    Z = S.size
    pk = int(np.argmax(S))
    delta = (pk - (Z - 1) // 2) * step
    if pk == 0 or pk == Z - 1:
        return pk, delta, 1
    y0, y1, y2 = S[pk - 1], S[pk], S[pk + 1]
    den = y0 - 2.0 * y1 + y2
    off = 0.5 * (y0 - y2) / den if den < 0.0 else 0.0
    return pk, delta + min(max(off, -0.5), 0.5) * step, 0


def refine(x, table_d, code_w, N, starts_d, o, cp, f_c, fs, J, G, Z, half_span, sec=None):
    """the whole estimator for one cell -> dict(z, S, peak_index, delta_hz, at_edge, step_hz, carrier_hz)"""
    z = prompts(x, table_d, code_w, N, starts_d, o, G * J, cp)
    S = spectrum(z, starts_d, o, f_c, fs, N, J, G, Z, half_span, sec)
    _, step = grid(Z, half_span)
    pk, delta, edge = peak_interp(S, step)
    return dict(z=z, S=S, peak_index=pk, delta_hz=delta, at_edge=edge, step_hz=step, carrier_hz=float(f_c) + delta)


# ---- the truth scenes --------------------------------------------------------------------------------------------------------------
# chips x secondary row x data bits x carrier + noise, rounded to int8 (synth.make_scene has neither a secondary row nor bits shorter
# than 20 periods).  One satellite; N = 2048 samples a period nominally (fs = 2.048 MHz, a 1 ms code), the true period T = N - 0.4
# samples, so the handle runs with the code-drift compensation.  f_if = fs / 4: the real-sample scene keeps its image 1 MHz away.
TRUTH_N = 2048
TRUTH_FS = 2.048e6
TRUTH_F_IF = 512.0e3
TRUTH_DOPPLER = 130.0                          # between the bins of AM.DOP (-300, 0, 300)
TRUTH_T = TRUTH_N - 0.4
TRUTH_PRN = 5
TRUTH_ROW = (1, 1, -1, -1)
# name -> K, M, span_periods, offsets, secondary row, true edge (periods), data bits of the groups from the edge on, sample format,
# code start (samples), C/N0 (dB-Hz), seed
# The row (1, 1, -1, -1) moved by two periods is its own negative, and a Doppler 130 Hz off the bin turns the phase by 187 degrees over
# one group of 4 ms, which a sign flip in the middle of a group undoes: the hypothesis two periods off the true edge, in the same bin,
# comes within +-6 % of the true cell's power whatever the noise is (bins 300 Hz apart are wider than the 1 / (2 K T_code) = 125 Hz the
# header recommends).  Which of the two is larger depends on where the code starts inside the period, on which group boundary carries
# the bit flip and on the noise: the scenes below (the flip between the second and the third group, the code start, the seed) are
# those of a small scan in which the true cell is the search's maximum by 5 % or more — test_acq_refine_host.py asserts 3 %.
TRUTH_SCENES = {
    "a": dict(K=4, M=3, span=0, offsets=(0, 1, 2, 3), sec=TRUTH_ROW, edge=1, bits=(1, 1, -1), fmt="i8", code_start=12.3, cn0=60.0, seed=11),
    "b": dict(K=4, M=3, span=0, offsets=(0, 1, 2, 3), sec=TRUTH_ROW, edge=1, bits=(1, 1, -1), fmt="real", code_start=TRUTH_N - 5.0, cn0=60.0, seed=11),
    "c": dict(K=1, M=6, span=6, offsets=None, sec=None, edge=0, bits=None, fmt="i8", code_start=700.3, cn0=60.0, seed=13),
}
TRUTH_MARGIN = 0.03


def truth_bound(R_u, T=TRUTH_T, fs=TRUTH_FS):
    """1 / (4 R_u T_code): a quarter of the dwell's own frequency resolution (20.8 Hz at 12 periods of 1 ms, 41.7 Hz at 6)"""
    return 1.0 / (4.0 * R_u * (T / fs))


def truth_scene(code_table, name):
    """-> dict(x, chips, code_rate, codes, starts [D][R], dwell, T, K, M, span, offsets, sec, edge, fmt, cp_window, f_true)"""
    c = dict(TRUTH_SCENES[name])
    N, fs, T = TRUTH_N, TRUTH_FS, TRUTH_T
    K, M = c["K"], c["M"]
    offs = list(c["offsets"]) if c["offsets"] else [0]
    R = K * M + offs[-1]
    Tb = np.full(AM.D, T, np.float64)
    starts = AM.drift_starts(Tb, R)
    dwell = int(starts[:, -1].max()) + N
    chips = np.ascontiguousarray(np.asarray(code_table, np.int8)[[TRUTH_PRN - 1], :])
    L = chips.shape[1]
    rate = fs * L / T
    rng = np.random.default_rng(c["seed"])
    n = np.arange(dwell, dtype=np.float64)
    u = (n - c["code_start"]) / T                       # code periods since the code start; period index floor(u)
    per = np.floor(u).astype(np.int64)
    chip = chips[0][np.floor((u - per) * L).astype(np.int64) % L].astype(np.float64)
    sign = np.ones(dwell, np.float64)
    # `edge` is the offset at which the handle's groups line up with the signal's.  The handle's period p is the N samples from s[p]
    # on; the lag-cp correlation takes its samples from cp on out of the signal's period p and the ones before cp out of period p - 1,
    # so a code start in the second half of the period makes period p - 1 the one that counts
    lead = 1 if c["code_start"] > N / 2 else 0
    q = per - (c["edge"] - lead)                        # periods since the signal's edge
    if c["sec"] is not None:
        sign *= np.asarray(c["sec"], np.float64)[q % K]
    if c["bits"] is not None:
        g = q // K                                      # the data bit (group) a period belongs to; before the edge: the bit before
        bits = np.asarray(c["bits"], np.float64)
        sign *= np.where(g < 0, -bits[0], bits[np.clip(g, 0, bits.size - 1)])
    sigma = 16.0
    amp = sigma * np.sqrt(2.0 * 10.0 ** (c["cn0"] / 10.0) / fs)
    f_true = TRUTH_F_IF + TRUTH_DOPPLER
    cyc = f_true * n / fs
    sig = amp * chip * sign * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 0.7j)
    noise = sigma * (rng.standard_normal(dwell) + 1j * rng.standard_normal(dwell))
    xi = np.clip(np.rint((sig + noise).real), -127, 127) + 1j * np.clip(np.rint((sig + noise).imag), -127, 127)
    c.update(x=AM.convert(xi, c["fmt"]), chips=chips, code_rate=rate, codes=AM.sample_codes(chips, rate, fs, N), starts=starts,
             dwell=dwell, T=Tb, offsets=c["offsets"] and offs, f_true=f_true, N=N, fs=fs, f_if=TRUTH_F_IF,
             cp_window=(int(np.floor(c["code_start"])) - 1, int(np.ceil(c["code_start"])) + 1))
    return c
