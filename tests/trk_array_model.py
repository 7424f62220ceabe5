"""Per-antenna prompts at tracked states (gm_trk_array_prompts, include/gnss_mi355x.h) in numpy: the definition, the argument rules of
gm_trk_array_plan and the rules that skip a record.  Built on trk_bank_model's chip_index and samples_per_code.

    phase_i = carrier_phase + fl(fl(fl(2 pi) * carrier_freq) * i) / fs
    c[i]    = (code_phase + i * (code_rate / fs)) mod code_len
    ref[i]  = (cos phase_i, -sin phase_i) * chip(fl(c[i] + tau))
    z[l][a] = sum_{i < n} x_a[s + i - l] * ref[i]              a time index below 0 reads as zero

Every operation the definition rounds in f32 is done in float32 here — the phase expression, c[i] with np.fmod, the tap phase; sine and
cosine are taken in float64 of the f32 phase and rounded once; the products and the sum over i are in float64.

A helper module, not a test.  Shared by tests/test_trk_array_host.py (CPU) and tests/test_gpu_trk_array.py (GPU).  Run as a script it
prints the README's table.  x is always [n_time, A] complex128 (stap_model.as_c128 converts the device formats)."""
import numpy as np

import trk_bank_model as TB

FAITHFUL, FIXED = TB.FAITHFUL, TB.FIXED
OK, INVALID_ARG, OUT_OF_RANGE = TB.OK, TB.INVALID_ARG, TB.OUT_OF_RANGE
SLICE = 4096
A_MIN, A_MAX, L_MIN, L_MAX, M_MAX, STATES_MAX = 2, 8, 1, 8, 32, 1024
INDEX_MAX = 1 << 62
F32 = np.float32


# ---- the argument rules (gm_trk_array_plan) and the skips -------------------------------------------------------------------------------
def slices(n):
    """workgroup slices of a record: ceil(n / 4096), a function of n alone; 0 for a count the entry skips"""
    return (n + SLICE - 1) // SLICE if 0 < n < (1 << 31) else 0


def plan(fs, n_antennas, taps, tap_chips=0.0, n_states=1, code_rate=1.023e6, code_len=1023, reserved=(0, 0, 0, 0, 0)):
    """gm_trk_array_plan: the dict it fills in, or the status it refuses with"""
    if not (fs > 0 and np.isfinite(fs)) or any(reserved) or not np.isfinite(F32(tap_chips)):
        return INVALID_ARG
    if code_len > 16384:                 # the chip row shares the workgroup's LDS with the slice's ref image
        return OUT_OF_RANGE
    if not A_MIN <= n_antennas <= A_MAX or not L_MIN <= taps <= L_MAX or n_antennas * taps > M_MAX or not 1 <= n_states <= STATES_MAX:
        return OUT_OF_RANGE
    if abs(F32(tap_chips)) > 64 or not abs(F32(tap_chips)) < F32(0.5) * F32(code_len):
        return OUT_OF_RANGE
    n = TB.samples_per_code(fs, code_rate, code_len)
    return dict(words_per_record=taps * n_antennas, out_words=n_states * taps * n_antennas, samples=n if slices(n) else 0, slices=slices(n))


def runs(active, row, n_codes, n, s, L, first_index, n_time):
    """does a record run?  row: its code table row; n: its samples_per_code; s: next_sample_index"""
    if not active or not 0 <= row < n_codes or slices(n) == 0:
        return False
    if max(0, s - (L - 1)) < first_index:                # part of its halo lies in front of the buffer
        return False
    return s + n <= first_index + n_time


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def reference(n, fs, row, carrier_freq, carrier_phase, code_phase, code_rate, tau=0.0, mode=FIXED, boc11=False):
    """ref[i], i < n -> complex128 [n] whose parts are f32 values; `row` the record's +-1 chips"""
    row = np.asarray(row, np.float64)
    Lc = row.size
    fi = np.arange(n).astype(F32)
    step = F32(code_rate) / F32(fs)
    c = np.fmod(F32(code_phase) + fi * step, F32(Lc)).astype(F32)
    p = (c + F32(tau)).astype(F32)
    chip = row[TB.chip_index(p, Lc, mode)]
    if boc11:
        chip = chip * np.where((p - np.floor(p)).astype(F32) < F32(0.5), 1.0, -1.0)
    w = ((F32(2.0) * F32(np.pi)) * F32(carrier_freq)) * fi
    phase = (F32(carrier_phase) + w / F32(fs)).astype(F32)
    wc = np.cos(phase.astype(np.float64)).astype(F32).astype(np.float64)
    ws = (-np.sin(phase.astype(np.float64)).astype(F32)).astype(np.float64)
    return (wc + 1j * ws) * chip


def delayed(x, s, l, n, first_index=0):
    """x_a[s - l .. s - l + n) of [n_time, A] whose row 0 is time first_index; a time index below 0 reads as zero"""
    lo = int(s) - int(l)
    if lo >= 0:
        return x[lo - first_index:lo - first_index + n]
    assert first_index == 0
    return np.concatenate([np.zeros((-lo, x.shape[1]), x.dtype), x[:lo + n]])


def prompts(x, n, s, L, ref, first_index=0):
    """-> (z complex128 [L, A], envelope float64 [L, A] = sum_i |x_a[s + i - l]|: |ref| = 1, what the bars are a fraction of)"""
    A = x.shape[1]
    z = np.zeros((L, A), np.complex128)
    env = np.zeros((L, A), np.float64)
    for l in range(L):
        seg = delayed(x, s, l, n, first_index)
        z[l] = ref @ seg
        env[l] = np.abs(seg).sum(axis=0)
    return z, env


def prompts_state(x, st, fs, row, L, tau=0.0, mode=FIXED, boc11=False, first_index=0):
    """prompts() at a gm_trk_state record, n = round(fs / (code_rate / code_len))"""
    n = TB.samples_per_code(fs, st.code_rate, len(row))
    ref = reference(n, fs, row, st.carrier_freq, st.carrier_phase, st.code_phase, st.code_rate, tau, mode, boc11)
    return prompts(x, n, st.next_sample_index, L, ref, first_index)


# ---- the scenes: beam_model.scene's, the rows from tracker-form prompts ---------------------------------------------------------------
RECORDS = 9                       # next_sample_index = code_phase + p N, p = 0 .. 8: the last one ends inside the dwell of 10 N
CARRIER_PHASE = 0.3


def scene_records(worker):
    """the made-up records of satellite `worker`, from the scene's truth -> [(next_sample_index, carrier_freq, carrier_phase, code_phase,
    code_rate)]"""
    import beam_model as BM
    sat = BM.SATS[worker]
    return [(sat["code_phase"] + p * BM.N, float(sat["doppler"]), CARRIER_PHASE + 0.1 * p, 0.0, 1.023e6) for p in range(RECORDS)]


def scene_prompts(x, worker, L):
    """the RECORDS tracker-form prompt vectors of satellite `worker` on the scene x -> complex128 [RECORDS, L, A]"""
    import beam_model as BM
    import excise_model as EM
    row = EM.scene_codes()[worker]
    out = []
    for s, f, ph, cp, rate in scene_records(worker):
        n = TB.samples_per_code(BM.FS, rate, row.size)
        assert n == BM.N
        out.append(prompts(x, n, s, L, reference(n, BM.FS, row, f, ph, cp, rate))[0])
    return np.stack(out)


_CELLS = {}


def cells(name, seed, L):
    """the scene behind the two rows solved from the tracker-form prompts and the beamformer's own Gram matrix -> {(worker, "trk"):
    (bin, code phase, peak-to-mean), (worker, "quality"): lambda1 / lambda2}; computed once and shared"""
    import array_probe_model as PM
    import beam_model as BM
    key = (name, seed, L)
    if key not in _CELLS:
        x = BM.scene(name, seed)
        R = PM.gram(x, L)
        got = [PM.solve_row(scene_prompts(x, w, L), R, PM.LOADING) for w in (0, 1)]
        y = PM.beams(x, L, np.stack([g[0] for g in got]).astype(np.complex64), R)
        out = {}
        for w in (0, 1):
            out[(w, "trk")] = BM.search(y[w], w)
            info = got[w][1]
            out[(w, "quality")] = info["lambda1"] / info["lambda2"] if info["lambda2"] > 0.0 else float("inf")
        _CELLS[key] = out
    return _CELLS[key]


def table(out=print):
    """the README's table: per scene, L and satellite the peak-to-mean behind the acquisition-form row (array_probe_model) and behind the
    tracker-form row, seeds 1 / 2 / 3, their ratio and lambda1 / lambda2 of the tracker-form prompts"""
    import array_probe_model as PM
    import beam_model as BM
    for name, L in PM.CONFIGS:
        out("%s (A = %d), L = %d" % (name, BM.SCENES[name][0], L))
        for w in (0, 1):
            acq = [PM.cells(name, seed, L)[(w, "est")][2] for seed in PM.SEEDS]
            trk = [cells(name, seed, L)[(w, "trk")][2] for seed in PM.SEEDS]
            q = [cells(name, seed, L)[(w, "quality")] for seed in PM.SEEDS]
            out("  sat %d  acquisition-form %s   tracker-form %s   ratio %s   lambda1 / lambda2 %s"
                % (w, " / ".join("%.1f" % v for v in acq), " / ".join("%.1f" % v for v in trk),
                   " / ".join("%.3f" % (t / a) for t, a in zip(trk, acq)), " / ".join("%.1f" % v for v in q)))


if __name__ == "__main__":
    table()
