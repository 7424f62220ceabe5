"""Wall times of the space-time prompts of an antenna array at known cells (gm_acq_array_prompts) and of the way to the same words
without it: A L calls of gm_acq_local_search at lag_half_window = 0 on de-interleaved and delayed single-antenna copies of the dwell,
which are prepared in device memory OUTSIDE the timed region (the de-interleave and the delays are not charged to the yardstick).
Writes profiles/array_probe_times.json.
Set-up: 8 candidates at N = 16368 (fs = 16.368 MHz), K = 1, n_integrations = 10 (R_u = 10), int8 IQ, (A, L) = (4, 1), (4, 2), (4, 4), (8, 4).
Both entries are synchronous, so each figure is the host's clock around `iters` back-to-back calls (each ends in a stream synchronise),
divided by `iters`; two warm-up rounds, then five repeats with the two alternating in one process; the median and `spread` =
(max - min) / median of the five.  The yardstick also runs local_search's scan and pick kernels (257 grid points a candidate), which a
caller who only wants the prompts cannot switch off: that is part of what the entry saves.
Usage: python tools/array_probe_time.py [--iters 10] [--out profiles/array_probe_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4, 1), (4, 2), (4, 4), (8, 4))
N, PERIODS, CANDS = 16368, 10, 8
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_probe_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, acquisition
    _lib.init(0)
    hip = C.CDLL("libamdhip64.so.7")            # the runtime the library already loaded: plain device buffers
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def upload(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    rng = np.random.default_rng(3)
    dop = np.arange(-2000.0, 2001.0, 500.0, dtype=np.float32)
    eng = acquisition.AcquisitionEngine(float(N) * 1000.0, 0.0, N, doppler_hz=dop, prn_ids=list(range(1, 9)), n_integrations=PERIODS)
    dwell = int(eng.dwell_samples)
    assert dwell == PERIODS * N
    cands = [dict(worker=w, doppler_bin=int(rng.integers(dop.size)), code_phase_samples=int(rng.integers(N)), offset_periods=0)
             for w in range(CANDS)]

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    rows = []
    for A, L in SHAPES:
        x = np.clip(np.rint(30.0 * rng.standard_normal((dwell, A, 2))), -128, 127).astype(np.int8)
        d_x = upload(x)
        # the yardstick's inputs: antenna a delayed by l time samples, zeros in front
        copies = [upload(np.concatenate([np.zeros((l, 2), np.int8), x[:dwell - l, a]])) for l in range(L) for a in range(A)]
        new = lambda: eng.array_prompts(cands, d_x.value, A, L, _lib.FMT_I8_IQ)

        def old():
            return [eng.local_search(cands, samples=p.value, lag_half_window=0, want_prompts=True, fmt=_lib.FMT_I8_IQ) for p in copies]

        # the two ways give the same words to the order of the sums
        z = new()
        ref = old()
        scale = float(np.abs(z).max())
        for l in range(L):
            for a in range(A):
                for c in range(CANDS):
                    assert np.abs(z[c, :, l, a] - ref[l * A + a][c]["prompts"][0]).max() <= 1e-4 * scale, (A, L, l, a, c)
        for _ in range(2):
            timed(new)
            timed(old)
        t_new, t_old = [], []
        for _ in range(REPEATS):
            t_new.append(timed(new))
            t_old.append(timed(old))
        med, med_old = float(np.median(t_new)), float(np.median(t_old))
        larger_spread = max((max(t_new) - min(t_new)) / med, (max(t_old) - min(t_old)) / med_old)
        row = dict(n_antennas=A, taps=L, fft_size=N, periods=PERIODS, candidates=CANDS, array_prompts=_stats(t_new),
                   al_local_search_calls=_stats(t_old), array_prompts_over_al_calls=round(med / med_old, 4),
                   under_the_al_calls_by_more_than_the_larger_spread=bool(med < med_old * (1.0 - larger_spread)))
        print(json.dumps(row), flush=True)
        rows.append(row)
        for p in [d_x] + copies:
            hip.hipFree(p)
    eng.close()
    meta = dict(tool="tools/array_probe_time.py", iters=args.iters, repeats=REPEATS,
                timing="host clock around `iters` back-to-back synchronous gm_acq_array_prompts calls (8 candidates, N = 16368, R_u = 10, "
                       "int8 IQ, A interleaved antennas, L taps), and around as many rounds of A L gm_acq_local_search calls at "
                       "lag_half_window = 0 with prompts on de-interleaved, delayed device copies made outside the timed region; one "
                       "process, two warm-up rounds each, five repeats with the two alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
