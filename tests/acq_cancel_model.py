"""A float64 numpy restatement of subtracting found satellites from a dwell (gm_acq_cancel), and its scene.

A helper module like acq_local_model.py (which it imports, with acq_model.py, and does not edit), not a test.  Shared by
tests/test_acq_cancel_host.py (CPU: gm_acq_cancel_plan against the model's bounds, the model's self-checks, the two-satellite scene)
and tests/test_gpu_cancel.py (GPU: the device's output, amplitudes and bounds against the model, the chain on the GPU).

The model restates the definition, not the kernels.  For a candidate (worker w, carrier f, code phase cp, period T) on a dwell x of D
samples:
    q0 = -ceil(cp / T);  o_k = cp + (q0 + k) T;  b_k = clamp(ceil(o_k), 0, D), k = 0 .. Q with Q the least count with o_Q >= D, b_Q = D
    r[n] = c_w[min(L - 1, floor((n - o_k) L / T))] exp(j 2 pi frac(n f / fs))            for b_k <= n < b_{k+1}
    a_k  = sum_{b_k <= n < b_{k+1}} x[n] conj(r[n]) / (b_{k+1} - b_k)                    (0 for an empty segment)
    y[n] = x[n] - a_k r[n]        (the real format: x[n] - 2 Re(a_k r[n]))
For several candidates every amplitude comes from x and the terms are subtracted in index order.  Everything is float64."""
import numpy as np

import acq_local_model as LM
import acq_model as AM

MAX_CANDS = 64
T_SPAN = 8.0            # |T - N| <= 8


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def cancel(x, code, cp, f, T, fs, L, real):          # one candidate; x complex128 [D]
    D = x.size; q0 = -int(np.ceil(cp / T)); o = []; k = 0
    while True:
        o.append(cp + float(q0 + k) * T)
        if o[-1] >= D: break
        k += 1
    b = np.clip(np.ceil(o), 0, D).astype(np.int64); b[-1] = D; y = x.copy(); amps = []
    for k in range(len(b) - 1):
        lo, hi = b[k], b[k + 1]
        if hi <= lo: amps.append(0j); continue
        n = np.arange(lo, hi, dtype=np.float64)
        idx = np.minimum(L - 1, np.floor((n - o[k]) * (L / T)).astype(np.int64))
        cyc = n * (f / fs); r = code[idx] * np.exp(2j * np.pi * (cyc - np.floor(cyc)))
        a = np.sum(x[lo:hi] * np.conj(r)) / (hi - lo); amps.append(a)
        y[lo:hi] -= 2 * np.real(a * r) if real else a * r
    return y, np.array(amps), b


def plan(D, N, cp, T=0.0):
    """gm_acq_cancel_plan's rules -> dict(n_segments, bounds int64 [Q + 1]), or None where they say GM_ERR_INVALID_ARG"""
    if not (0.0 <= cp < N) or (T != 0.0 and not abs(T - N) <= T_SPAN) or D <= 0:
        return None
    _, amps, b = cancel(np.zeros(int(D), np.complex128), np.ones(1), float(cp), 0.0, float(T) if T != 0.0 else float(N), 1.0, 1, False)
    return dict(n_segments=len(amps), bounds=b)


def cancel_all(x, chips, cands, fs, N, real):
    """every candidate (dicts with worker, carrier_hz, code_phase, period_samples: cancel()'s of the engine) against the INPUT x, the
    terms subtracted in index order -> (y complex128 [D], [amps], [bounds]); the real format's y has a zero imaginary part"""
    X = AM.as_c128(x)
    y, amps, bounds = X.copy(), [], []
    for c in cands:
        T = float(c.get("period_samples", 0.0)) or float(N)
        code = np.asarray(chips[c["worker"]], np.float64)
        yc, a, b = cancel(X, code, float(c["code_phase"]), float(c["carrier_hz"]), T, float(fs), code.size, real)
        y -= X - yc
        amps.append(a)
        bounds.append(b)
    return y, amps, bounds


def out_fields(amps, bounds, D):
    """gm_acq_cancel_out's host formula on one candidate's amplitudes (the device's words, or the model's)"""
    n = np.diff(np.asarray(bounds, np.int64)).astype(np.float64)
    a = np.asarray(amps).astype(np.complex128)
    e = float(np.sum(n * (a.real * a.real + a.imag * a.imag)))
    return dict(n_segments=len(n), first_samples=int(n[0]), last_samples=int(n[-1]), removed_energy=e, amp_rms=float(np.sqrt(e / D)))


# ---- the scene: a strong and a weak satellite ------------------------------------------------------------------------------------
N, FS, F_IF = 2048, 2.048e6, 512.0e3
T_TRUE = N - 0.4
PERIODS = 12
SIGMA = 16.0
STRONG = dict(worker=0, cn0=66.0, code_start=700.3, doppler=130.0)           # PRN 5
WEAK = dict(worker=1, cn0=42.0, code_start=1200.7, doppler=-170.0)           # PRN 6
WEAK_PHASES = (1200, 1201)
BIT_PERIODS = 4         # data bits are constant within groups of four signal periods
LOCAL_L, LOCAL_SPAN = 3, 4


def scene(code_table, seed, strong_cn0=STRONG["cn0"], weak_cn0=WEAK["cn0"], fmt="i8", periods=PERIODS, drift=True):
    """-> dict: x (the dwell in format fmt), chips [2][1023] (PRN 5 and 6), codes (the replicas as the handle samples them), starts
    [3][periods] (AM.drift_starts of T_TRUE in every bin; drift False: a handle without the compensation, period p from p N — the
    signal's period is T_TRUE either way), dwell, code_rate, T [3]"""
    chips = np.ascontiguousarray(np.asarray(code_table, np.int8)[[p - 1 for p in AM.PRN_IDS], :1023])
    T = np.full(AM.D, T_TRUE)
    starts = AM.drift_starts(T, periods) if drift else AM.plain_starts(AM.D, periods, N)
    dwell = int(starts[:, -1].max()) + N
    rate = FS * chips.shape[1] / T_TRUE
    rng = np.random.default_rng(seed)
    n = np.arange(dwell, dtype=np.float64)
    sig = np.zeros(dwell, np.complex128)
    for s, cn0, phase in ((STRONG, strong_cn0, 0.7), (WEAK, weak_cn0, 2.1)):
        u = (n - s["code_start"]) / T_TRUE
        per = np.floor(u).astype(np.int64)
        chip = chips[s["worker"]][np.minimum(1022, np.floor((u - per) * 1023.0).astype(np.int64))].astype(np.float64)
        bits = rng.integers(0, 2, periods // BIT_PERIODS + 2) * 2.0 - 1.0
        sign = bits[(per + BIT_PERIODS) // BIT_PERIODS]                      # (per starts at -1)
        amp = SIGMA * np.sqrt(2.0 * 10.0 ** (cn0 / 10.0) / FS)
        cyc = (F_IF + s["doppler"]) * n / FS
        sig += amp * chip * sign * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * phase)
    noise = SIGMA * (rng.standard_normal(dwell) + 1j * rng.standard_normal(dwell))
    v = sig + noise
    xi = np.clip(np.rint(v.real), -127, 127) + 1j * np.clip(np.rint(v.imag), -127, 127)
    return dict(x=AM.convert(xi, fmt), fmt=fmt, chips=chips, codes=AM.sample_codes(chips, rate, FS, N), starts=starts, dwell=dwell,
                code_rate=rate, T=T, seed=seed)


def best_cell(mx, sm, w):
    """(bin, peak-to-mean) of worker w's best cell over the bins: the largest max / (sum / N) of search_model's [P][1][D] blocks (or
    the engine's [P][D] metrics)"""
    ratio = np.asarray(mx, np.float64).reshape(AM.P, -1)[w] * N / np.asarray(sm, np.float64).reshape(AM.P, -1)[w]
    d = int(np.argmax(ratio))
    return d, float(ratio[d])


def strong_candidate(c, tables, tf, d, cp):
    """the cancellation parameters of the strong satellite: what acq_local_model.local returns for its found cell (bin d, arg-max cp)
    with L = 3 and span_periods = 4, and the true period of that bin"""
    p = LM.plan(1, PERIODS, FS, N, tf, d, LOCAL_L, LOCAL_SPAN)
    r = LM.local(c["x"], tables[d], c["codes"][STRONG["worker"]], N, c["starts"][d], 0, int(cp), LOCAL_L, tf[d], FS, p["span_periods"],
                 p["n_groups"], p["n_freq"], p["half_span_hz"], None, T_d=c["T"][d], code_rate=c["code_rate"])
    return dict(worker=STRONG["worker"], carrier_hz=float(r["carrier_hz"]), code_phase=float(r["code_phase_fine"]),
                period_samples=float(c["T"][d]))
