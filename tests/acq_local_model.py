"""A float64 numpy restatement of the lag window x fine Doppler at known cells (gm_acq_local_search), and its scenes.

A helper module like acq_refine_model.py (which it imports, with acq_model.py, and does not edit), not a test.  Shared by
tests/test_acq_local_host.py (CPU: the argument rules of gm_acq_local_plan, the model against the simulated code start) and
tests/test_gpu_local_search.py (GPU: the device's prompts, surface, peak, fine code phase and floor against the model).

The model restates the definition, not the kernels.  For a candidate (worker w, bin d, centre cp, offset o) and L = lag_half_window:
    lambda_l = (cp + l - L) mod N,  l < W = 2 L + 1
    z[l][i]  = sum_n x[s[d][o + i] + n] tab[d][n] c_w[(n - lambda_l) mod N]              acq_refine_model.prompts at lag lambda_l
    S[l][j]  = acq_refine_model.spectrum(z[l])                                           gm_acq_refine_doppler's statistic, per lag
    (l*, j*) = the first maximum of S in (l, j) order
    frac     = (a+ - a-) / (2 (a0 - min(a-, a+))),  a = sqrt(S[l* -1 / 0 / +1][j*]), clamped to +-0.5, 0 where the denominator is <= 0
    lambda   = lambda_{l*} + frac
    code_phase_fine = lambda mod N without the drift compensation, else (lambda + ebar - (lambda / N)(N - T_d)) mod N with
    ebar     = mean_i (s[d][o + i] - (o + i) T_d)
    floor    = mean of S[l][.] over the lags at a circular distance >= ceil(fs / code_rate) + 1 from l*
Everything is float64; the only device words it takes are the mix tables."""
import math

import numpy as np

import acq_model as AM
import acq_refine_model as RM

L_MAX = 64


# ---- the argument rules (gm_acq_local_plan) ----------------------------------------------------------------------------------------
def plan(K, M, fs, N, table_freq, b=0, lag_half_window=0, span_periods=0, n_freq=0, half_span_hz=0.0):
    """acq_refine_model.plan's dict plus n_lags, or None where the rules say GM_ERR_INVALID_ARG"""
    p = RM.plan(K, M, fs, N, table_freq, b, span_periods, n_freq, half_span_hz)
    L = int(lag_half_window)
    if p is None or L < 0 or L > L_MAX or 2 * L + 1 > N:
        return None
    return dict(p, n_lags=2 * L + 1)


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def lags(cp, L, N):
    return (int(cp) + np.arange(2 * L + 1, dtype=np.int64) - L) % N


def prompts(x, table_d, code_w, N, starts_d, o, R_u, cp, L):
    """[W][R_u] complex128: acq_refine_model.prompts at every lag of the window (one matrix product instead of W calls)"""
    X = AM.as_c128(x)
    prod = np.stack([X[int(starts_d[o + i]):int(starts_d[o + i]) + N] for i in range(R_u)]) * np.asarray(table_d).astype(np.complex128)
    code = np.asarray(code_w, np.float64)
    rot = np.stack([np.roll(code, int(lam)) for lam in lags(cp, L, N)])            # c[(n - lambda_l) mod N]
    return rot @ prod.T


def guard_lags(fs, code_rate):
    """ceil(fs / code_rate) + 1: one chip and a sample, in samples (f32 arguments as the handle holds them)"""
    return int(math.ceil(float(np.float32(fs)) / float(np.float32(code_rate)))) + 1


def triangle_frac(am, a0, ap):
    den = 2.0 * (a0 - min(am, ap))
    return min(max((ap - am) / den, -0.5), 0.5) if den > 0.0 else 0.0


def ebar(starts_d, o, R_u, T_d):
    """the mean rounding of the period starts used: mean_i (s[o + i] - (o + i) T_d)"""
    i = np.arange(o, o + R_u, dtype=np.float64)
    return float(np.mean(np.asarray(starts_d)[o:o + R_u].astype(np.float64) - i * float(T_d)))


def fine_phase(lam, N, starts_d=None, o=0, R_u=0, T_d=None, blend=True):
    """code_phase_fine from lambda = lambda_{l*} + frac; T_d None: no drift compensation.  blend=False leaves the second correction
    out (for the test that shows it is needed)."""
    if T_d is None:
        return lam % N
    corr = (lam / N) * (N - float(T_d)) if blend else 0.0
    return (lam + ebar(starts_d, o, R_u, T_d) - corr) % N


def floor_of(S, l_star, guard, N):
    """(floor_power, n_floor) of a surface [W][Z]"""
    W = S.shape[0]
    dl = np.abs(np.arange(W) - l_star)
    far = np.minimum(dl, N - dl) >= guard
    n = int(far.sum())
    return (float(np.mean(S[far])) if n else 0.0), n


def fine_from_surface(S, l, j, cp, L, N, starts_d=None, o=0, R_u=0, T_d=None, blend=True):
    """(code_phase_samples, lag_at_edge, frac, code_phase_fine) of a surface [W][Z] whose peak is taken to be (l, j)"""
    W = 2 * L + 1
    lam = int(lags(cp, L, N)[l])
    if l == 0 or l == W - 1:
        return lam, 1, 0.0, float(lam)
    frac = triangle_frac(*(math.sqrt(float(S[l + u][j])) for u in (-1, 0, 1)))
    return lam, 0, frac, fine_phase(lam + frac, N, starts_d, o, R_u, T_d, blend)


def local(x, table_d, code_w, N, starts_d, o, cp, L, f_c, fs, J, G, Z, half_span, sec=None, T_d=None, code_rate=None, blend=True):
    """the whole evaluation for one candidate -> dict(z [W][R_u], S [W][Z], l, j, lam, delta_hz, carrier_hz, freq_at_edge,
    lag_at_edge, frac, code_phase_samples, code_phase_fine, floor_power, n_floor, step_hz)"""
    R_u, W = G * J, 2 * L + 1
    z = prompts(x, table_d, code_w, N, starts_d, o, R_u, cp, L)
    S = np.stack([RM.spectrum(z[l], starts_d, o, f_c, fs, N, J, G, Z, half_span, sec) for l in range(W)])
    l, j = (int(v) for v in np.unravel_index(int(np.argmax(S)), S.shape))
    _, step = RM.grid(Z, half_span)
    _, delta, fedge = RM.peak_interp(S[l], step)                 # (row l*'s own first maximum is j*)
    lam, ledge, frac, fine = fine_from_surface(S, l, j, cp, L, N, starts_d, o, R_u, T_d, blend)
    fl, nf = floor_of(S, l, guard_lags(fs, code_rate), N) if code_rate else (0.0, 0)
    return dict(z=z, S=S, l=l, j=j, lam=lam, delta_hz=delta, carrier_hz=float(f_c) + delta, freq_at_edge=fedge, lag_at_edge=ledge,
                frac=frac, code_phase_samples=lam, code_phase_fine=fine, floor_power=fl, n_floor=nf, step_hz=step)


def circular_error(got, want, period):
    """got - want on a circle of `period`, in (-period / 2, period / 2]"""
    return (got - want + period / 2.0) % period - period / 2.0


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
def truth_scene(code_table, name, s0=0, seed_add=0):
    """acq_refine_model.truth_scene's signal from sample s0 on (s0 = 0, seed_add = 0: that scene's words, which test_acq_local_host.py asserts): a second,
    later dwell of the same satellite for the fresh-samples tests, with a noise realisation of its own.  The handle's period p of
    this dwell is the signal's period p + s0 / T; with s0 a whole number of secondary-row lengths (K periods) to within a sample the
    edge's offset is unchanged.  Adds code_start_here = (code_start - s0) mod T, the code phase this dwell should show."""
    c = RM.truth_scene(code_table, name)
    T = RM.TRUTH_T
    c["s0"] = int(s0)
    c["code_start_here"] = (c["code_start"] - s0) % T
    N, fs, K, dwell = c["N"], c["fs"], c["K"], c["dwell"]
    chips = c["chips"]
    Lc = chips.shape[1]
    rng = np.random.default_rng(c["seed"] + seed_add)
    n = np.arange(dwell, dtype=np.float64) + float(s0)
    u = (n - c["code_start"]) / T
    per = np.floor(u).astype(np.int64)
    chip = chips[0][np.floor((u - per) * Lc).astype(np.int64) % Lc].astype(np.float64)
    sign = np.ones(dwell, np.float64)
    lead = 1 if c["code_start"] > N / 2 else 0
    q = per - (c["edge"] - lead)
    if c["sec"] is not None:
        sign *= np.asarray(c["sec"], np.float64)[q % K]
    if c["bits"] is not None:
        g = q // K
        bits = np.asarray(c["bits"], np.float64)
        sign *= np.where(g < 0, -bits[0], bits[np.clip(g, 0, bits.size - 1)])
    sigma = 16.0
    amp = sigma * np.sqrt(2.0 * 10.0 ** (c["cn0"] / 10.0) / fs)
    cyc = c["f_true"] * n / fs
    sig = amp * chip * sign * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 0.7j)
    noise = sigma * (rng.standard_normal(dwell) + 1j * rng.standard_normal(dwell))
    xi = np.clip(np.rint((sig + noise).real), -127, 127) + 1j * np.clip(np.rint((sig + noise).imag), -127, 127)
    c["x"] = AM.convert(xi, c["fmt"])
    return c


def later_start(K, periods=3):
    """a start for the later dwell: `periods` secondary-row lengths on, rounded to a whole sample"""
    return int(round(periods * K * RM.TRUTH_T))
