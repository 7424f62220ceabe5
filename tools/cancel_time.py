"""Times of subtracting found satellites from a dwell (gm_acq_cancel) for 1, 4 and 8 candidates, beside one plain search of the same
dwell on the same handle (gm_acq_search_dev + gm_acq_synchronize); writes profiles/cancel_times.json.  Shapes:
  a   N = 8000,  K = 1,  M = 20, int8 IQ,   21 bins at 50 Hz, 32 workers
  c   N = 16368, K = 20, M = 4,  int8 real, 21 bins at 25 Hz, 32 workers, code drift on (T = N - 0.4)
gm_acq_cancel is synchronous (small host copies in, two kernels, the amplitudes out, one stream synchronisation), so the time is wall
time around the call, the mean of `iters` of them; one process, two warm-up rounds of each, then five repeats with the cancellation
and the search alternating; the median and `spread` = (max - min) / median of the five.  The dwell sits in device memory on both sides
and the output goes to a second device buffer.  The samples are noise (the time does not depend on them); candidate i names worker
4 i, a carrier 100 i Hz above the IF, a code start 700.3 + 37 i and the period N - 0.4.
Usage: python tools/cancel_time.py [--iters 20] [--out profiles/cancel_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, N, fs, f_if, bin step, bins, K, M, sample format, drift)
SHAPES = [("a", 8000, 8.0e6, 2.0e6, 50.0, 21, 1, 20, "i8", False),
          ("c", 16368, 16.3676e6, 4.1304e6, 25.0, 21, 20, 4, "real", True)]
N_CANDS = (1, 4, 8)
REPEATS, N_PRN = 5, 32


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cancel_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _lib.init(0)
    hip = C.CDLL("libamdhip64.so.7")            # the runtime the library already loaded: plain device buffers for both sides
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    rng = np.random.default_rng(22)
    rows = []
    for name, N, fs, f_if, step, D, K, M, fmt, drift in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, N_PRN + 1), n_integrations=M, coherent_periods=K)
        if drift:
            eng.set_code_drift(N - 0.4)
        n = eng.dwell_samples
        x = rng.integers(-40, 41, (n, 2) if fmt == "i8" else n).astype(np.int8)
        code = _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_I8_REAL
        d_x, d_y = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_x), x.nbytes) == 0 and hip.hipMalloc(C.byref(d_y), n * 8) == 0
        assert hip.hipMemcpy(d_x, x.ctypes.data, x.nbytes, 1) == 0

        def search():
            eng.search_dev(d_x.value, code)
            eng.synchronize()

        for nc in N_CANDS:
            cands = [dict(worker=4 * i, carrier_hz=f_if + 100.0 * i, code_phase=700.3 + 37.0 * i, period_samples=N - 0.4) for i in range(nc)]
            cancel = lambda: eng.cancel(cands, d_y.value, samples=d_x.value, fmt=code)
            info = cancel()[0]
            cancel()
            search()
            search()
            t_cancel, t_search = [], []
            for _ in range(REPEATS):
                t_cancel.append(_timed(cancel, args.iters))
                t_search.append(_timed(search, args.iters))
            row = dict(shape=name, fft_size=N, fs=fs, n_prn=N_PRN, n_bins=D, bin_hz=step, coherent_periods=K, n_integrations=M,
                       sample_format=fmt, code_drift=drift, dwell_samples=n, n_cands=nc, n_segments=info["n_segments"],
                       cancel=_stats(t_cancel), search=_stats(t_search),
                       cancel_over_search=round(float(np.median(t_cancel)) / float(np.median(t_search)), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
        eng.close()
        hip.hipFree(d_x)
        hip.hipFree(d_y)
    meta = dict(tool="tools/cancel_time.py", iters=args.iters, repeats=REPEATS,
                timing="wall time around the synchronous gm_acq_cancel call (host copies, two kernels, one stream synchronisation) and "
                       "around gm_acq_search_dev + gm_acq_synchronize of the same dwell on the same handle; mean of `iters`; one process, "
                       "two warm-up rounds each, five repeats with the two alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
