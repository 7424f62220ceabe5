"""The correlator bank at tracked states (gm_trk_bank, include/gnss_mi355x.h) in numpy: the definition, and the argument rules of
gm_trk_bank_plan.

    f_f      = fl(carrier_freq + df_f)
    phase_i  = carrier_phase + fl(fl(fl(2 pi) * f_f) * i) / fs
    y_f[i]   = x[i] * (cos phase_i, -sin phase_i)                      num-complex order
    c[i]     = (code_phase + i * (code_rate / fs)) mod code_len
    out[f][t] = sum_{i < n} y_f[i] * chip(fl(c[i] + tau_t))

Every operation the definition rounds in f32 is done in float32 here — f_f, the phase expression, the products in num-complex
order, c[i] with np.fmod, the tap phase; sine and cosine are taken in float64 of the f32 phase and rounded once; the sum over i is
in float64."""
import math

import numpy as np

FAITHFUL, FIXED = 0, 1
OK, INVALID_ARG, OUT_OF_RANGE = 0, -1, -5
SLICE = 4096
F32 = np.float32


def samples_per_code(fs, code_rate, code_len):
    """round(fs / (code_rate / code_len)) in f32, roundf's halves away from zero; 0 where the tracker's own count is 0"""
    with np.errstate(all="ignore"):
        v = float(F32(fs) / (F32(code_rate) / F32(code_len)))
    if not v > 0.0:
        return 0
    return int(math.floor(v + 0.5)) if math.isfinite(v) else 1 << 64


def slices(n):
    """workgroup slices of a record's epoch: a function of n alone; 0 for an epoch the bank skips"""
    return (n + SLICE - 1) // SLICE if 0 < n < (1 << 31) else 0


def plan(fs, taps, offsets_hz=None, n_states=1, code_rate=1.023e6, code_len=1023):
    """gm_trk_bank_plan: the dict it fills in, or the status it refuses with"""
    taps = None if taps is None else np.atleast_1d(np.asarray(taps, F32))
    offs = np.zeros(0, F32) if offsets_hz is None else np.atleast_1d(np.asarray(offsets_hz, F32))
    if taps is None:
        return INVALID_ARG
    if code_len > 16384:                 # the chip row shares the workgroup's LDS with the slice's samples
        return OUT_OF_RANGE
    T, F = taps.size, max(offs.size, 1)
    if not 1 <= T <= 64 or F > 8 or F * T > 256 or not 1 <= n_states <= 1024:
        return OUT_OF_RANGE
    if not np.all(np.isfinite(taps)) or not np.all(np.isfinite(offs)):
        return INVALID_ARG
    if np.any(np.abs(taps) > 64) or np.any(np.abs(taps) >= F32(0.5) * F32(code_len)) or np.any(np.abs(offs) > F32(0.5) * F32(fs)):
        return OUT_OF_RANGE
    n = samples_per_code(fs, code_rate, code_len)
    return dict(n_taps=T, n_offsets=F, out_words=n_states * F * T, samples=n if slices(n) else 0, slices=slices(n),
                tap_groups=(T + 15) // 16)


def chip_index(phase, code_len, mode):
    """get_ca_chip's index (do_tracking.rs:275): FAITHFUL `(phase.floor() as usize) % len` — the cast saturates a negative phase to
    0 —, FIXED the floor wrapped into [0, len)"""
    f = np.floor(phase.astype(np.float64)).astype(np.int64)
    if mode == FAITHFUL:
        return np.where(f > 0, f, 0) % code_len
    return f % code_len


def bank(x, n, fs, row, carrier_freq, carrier_phase, code_phase, code_rate, taps, offsets_hz=(0.0,), mode=FIXED, boc11=False):
    """-> complex128 [F, T]: the definition on the first n samples of x, `row` the record's +-1 chips"""
    taps = np.atleast_1d(np.asarray(taps, F32))
    offs = np.atleast_1d(np.asarray(offsets_hz, F32))
    row = np.asarray(row, np.float64)
    L = row.size
    x = np.asarray(x[:n], np.complex64)
    re, im = x.real.astype(F32), x.imag.astype(F32)
    fi = np.arange(n).astype(F32)
    step = F32(code_rate) / F32(fs)
    c = np.fmod(F32(code_phase) + fi * step, F32(L)).astype(F32)
    chips = np.empty((taps.size, n), np.float64)
    for t, tau in enumerate(taps):
        p = (c + F32(tau)).astype(F32)
        chips[t] = row[chip_index(p, L, mode)]
        if boc11:
            chips[t] *= np.where((p - np.floor(p)).astype(F32) < F32(0.5), 1.0, -1.0)
    out = np.zeros((offs.size, taps.size), np.complex128)
    for f, df in enumerate(offs):
        f_f = F32(carrier_freq) + F32(df)
        w = ((F32(2.0) * F32(np.pi)) * f_f) * fi
        phase = (F32(carrier_phase) + w / F32(fs)).astype(F32)
        wc = np.cos(phase.astype(np.float64)).astype(F32)
        ws = -np.sin(phase.astype(np.float64)).astype(F32)
        yr = (re * wc - im * ws).astype(np.float64)              # num-complex Mul: each product and the difference rounded in f32
        yi = (re * ws + im * wc).astype(np.float64)
        out[f] = chips @ yr + 1j * (chips @ yi)
    return out


def bank_state(x, st, fs, row, taps, offsets_hz=(0.0,), mode=FIXED, boc11=False, n=None):
    """bank() at a gm_trk_state record; n None: the ring form's n = round(fs / (code_rate / code_len))"""
    if n is None:
        n = samples_per_code(fs, st.code_rate, len(row))
    return bank(x, n, fs, row, st.carrier_freq, st.carrier_phase, st.code_phase, st.code_rate, taps, offsets_hz, mode, boc11)
