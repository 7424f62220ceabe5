"""Times of the fine Doppler from per-period prompts (gm_acq_refine_doppler) and, where it can run, of the legacy estimator
(gm_acq_finer_doppler) on the same handle after the same search, 8 found satellites of 32; writes profiles/refine_doppler_times.json.
  a   N = 8000,  K = 1,  M = 10, int8 IQ, 29 bins at 500 Hz, J = 10
  b   N = 16368, K = 10, M = 2,  int8 real, 21 bins at 50 Hz
  c   N = 16368, K = 20, M = 4,  int8 real, 21 bins at 25 Hz, edge offsets 0..19, code drift on (T = N - 0.4): the legacy estimator
      refuses that dwell (GM_ERR_OUT_OF_RANGE) when a found cell chose the last offset, and its cell then stays empty; where no cell
      did it runs (uncompensated, without the secondary row: its time is a cost, its result means nothing there)
Both calls are synchronous (host copies in, kernels, host copies out, one stream synchronisation), so the time is wall time around the
call, the mean of `iters` calls; one process, two warm-up calls of each, then five repeats with the two estimators alternating; the
median and `spread` = (max - min) / median of the five.  The samples are noise (the time does not depend on them); the eight results
name the middle bin and a code phase near N - 91, so the replica rotation wraps.
Usage: python tools/refine_doppler_time.py [--iters 10] [--out profiles/refine_doppler_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, N, fs, f_if, bin step, bins, K, M, sample format, bytes a sample, edge offsets, drift)
SHAPES = [("a", 8000, 8.0e6, 0.0, 500.0, 29, 1, 10, "i8", 2, None, False),
          ("b", 16368, 16.3676e6, 4.1304e6, 50.0, 21, 10, 2, "real", 1, None, False),
          ("c", 16368, 16.3676e6, 4.1304e6, 25.0, 21, 20, 4, "real", 1, list(range(20)), True)]
REPEATS, N_PRN, N_FOUND = 5, 32, 8


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def _timed(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_doppler_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, acquisition as A
    rng = np.random.default_rng(20)
    rows = []
    for name, N, fs, f_if, step, D, K, M, fmt, b_in, offsets, drift in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, N_PRN + 1), n_integrations=M, coherent_periods=K)
        if offsets:
            eng.set_edge_search(offsets)
        if drift:
            eng.set_code_drift(N - 0.4)
        n = eng.dwell_samples
        x = rng.integers(-40, 41, (n, 2) if fmt == "i8" else n).astype(np.int8)
        eng.search(x)
        results = [None] * N_PRN
        for w in range(0, N_PRN, N_PRN // N_FOUND):
            results[w] = dict(_lib.AcqResult().as_dict(), prn=w + 1, doppler_bin=D // 2, code_phase_samples=N - 91 + w, fs=fs)
        new = lambda: eng.refine_doppler(results)
        old = lambda: eng.finer_doppler(results)
        legacy_status, fft_size = 0, None
        try:
            fft_size = [r for r in old() if r][0]["fft_size"]
        except _lib.GmError as e:
            legacy_status = e.status
        plan = new()[0]
        new()
        if not legacy_status:
            old()
        t_new, t_old = [], []
        for _ in range(REPEATS):
            t_new.append(_timed(new, args.iters))
            if not legacy_status:
                t_old.append(_timed(old, args.iters))
        eng.close()
        R_u, Z = plan["span_periods"] * plan["n_groups"], plan["n_freq"]
        row = dict(shape=name, fft_size=N, fs=fs, n_prn=N_PRN, n_found=N_FOUND, n_bins=D, bin_hz=step, coherent_periods=K,
                   n_integrations=M, sample_format=fmt, edge_offsets=len(offsets) if offsets else 0, code_drift=drift, dwell_samples=n,
                   prompts_per_satellite=R_u, n_freq=Z, half_span_hz=plan["half_span_hz"],
                   refine_bytes_read_per_satellite=R_u * N * (b_in + 9),
                   refine_doppler=_stats(t_new), finer_doppler=_stats(t_old) if t_old else None,
                   finer_doppler_status=legacy_status, finer_doppler_fft_size=fft_size,
                   finer_doppler_bytes_per_pass_per_satellite=8 * fft_size if fft_size else None,
                   finer_over_refine=round(float(np.median(t_old)) / float(np.median(t_new)), 3) if t_old else None)
        print(json.dumps(row), flush=True)
        rows.append(row)
    meta = dict(tool="tools/refine_doppler_time.py", iters=args.iters, repeats=REPEATS,
                timing="wall time around the synchronous call (host copies, kernels, one stream synchronisation), mean of `iters` calls; "
                       "one process, two warm-up calls each, five repeats with the two estimators alternating; median and spread = "
                       "(max - min) / median; finer_doppler_status -5: the legacy estimator refuses the dwell (not compensated)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
