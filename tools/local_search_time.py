"""Times of the lag window x fine Doppler at known cells (gm_acq_local_search) and of the way to the same surface without it: W =
2 L + 1 calls of gm_acq_refine_doppler, one per lag, on the same handle after the same search; 8 candidates (8 found satellites of 32);
writes profiles/local_search_times.json.  Shapes (b) and (c) of tools/refine_doppler_time.py, at L = 8 and L = 64:
  b   N = 16368, K = 10, M = 2,  int8 real, 21 bins at 50 Hz
  c   N = 16368, K = 20, M = 4,  int8 real, 21 bins at 25 Hz, edge offsets 0..19, code drift on (T = N - 0.4)
Both are synchronous (host copies in, kernels, host copies out, one stream synchronisation per call), so the time is wall time around
the call (for the baseline: around all W calls), the mean of `iters` of them; one process, two warm-up rounds of each, then five
repeats with the two ways alternating; the median and `spread` = (max - min) / median of the five.  No surface is copied out on either
side.  The samples are noise (the time does not depend on them); the candidates name the middle bin and a code phase near N - 91, so the
window's replica wraps.
Usage: python tools/local_search_time.py [--iters 10] [--out profiles/local_search_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, N, fs, f_if, bin step, bins, K, M, sample format, edge offsets, drift)
SHAPES = [("b", 16368, 16.3676e6, 4.1304e6, 50.0, 21, 10, 2, "real", None, False),
          ("c", 16368, 16.3676e6, 4.1304e6, 25.0, 21, 20, 4, "real", list(range(20)), True)]
LAGS = (8, 64)
REPEATS, N_PRN, N_CANDS = 5, 32, 8


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_search_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, acquisition as A
    rng = np.random.default_rng(21)
    rows = []
    for name, N, fs, f_if, step, D, K, M, fmt, offsets, drift in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, N_PRN + 1), n_integrations=M, coherent_periods=K)
        if offsets:
            eng.set_edge_search(offsets)
        if drift:
            eng.set_code_drift(N - 0.4)
        n = eng.dwell_samples
        x = rng.integers(-40, 41, n).astype(np.int8)
        eng.search(x)
        workers = list(range(0, N_PRN, N_PRN // N_CANDS))
        choice = eng.edge_choice() if offsets else None
        for L in LAGS:
            W = 2 * L + 1
            cands = [dict(worker=w, doppler_bin=D // 2, code_phase_samples=N - 91 + w,
                          offset_periods=int(offsets[int(choice[w, D // 2])]) if offsets else 0) for w in workers]
            per_lag = []
            for l in range(W):
                results = [None] * N_PRN
                for w in workers:
                    results[w] = dict(_lib.AcqResult().as_dict(), prn=w + 1, doppler_bin=D // 2,
                                      code_phase_samples=(N - 91 + w + l - L) % N, fs=fs)
                per_lag.append(results)
            new = lambda: eng.local_search(cands, lag_half_window=L)
            old = lambda: [eng.refine_doppler(r) for r in per_lag]
            plan = new()[0]
            new()
            old()
            old()
            t_new, t_old = [], []
            for _ in range(REPEATS):
                t_new.append(_timed(new, args.iters))
                t_old.append(_timed(old, args.iters))
            R_u, Z = plan["span_periods"] * plan["n_groups"], plan["n_freq"]
            row = dict(shape=name, fft_size=N, fs=fs, n_prn=N_PRN, n_cands=N_CANDS, n_bins=D, bin_hz=step, coherent_periods=K,
                       n_integrations=M, sample_format=fmt, edge_offsets=len(offsets) if offsets else 0, code_drift=drift,
                       dwell_samples=n, lag_half_window=L, n_lags=W, prompts_per_lag=R_u, n_freq=Z,
                       local_search=_stats(t_new), refine_doppler_per_lag=_stats(t_old),
                       per_lag_calls_over_local_search=round(float(np.median(t_old)) / float(np.median(t_new)), 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
        eng.close()
    meta = dict(tool="tools/local_search_time.py", iters=args.iters, repeats=REPEATS,
                timing="wall time around the synchronous call (host copies, kernels, one stream synchronisation); the baseline is W = "
                       "2 L + 1 calls of gm_acq_refine_doppler, one per lag, timed as one; mean of `iters`; one process, two warm-up rounds "
                       "each, five repeats with the two ways alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
