"""Wall-clock time of the whole synchronous gm_trk_array_prompts call — 32 records at 25 Msps (n = 25000), int8 IQ, on a resident
interleaved array stream — at (A, L) = (4, 1), (4, 2), (4, 4), (8, 4), beside what a caller could do before: A L calls of gm_trk_bank
(T = 1 tap 0, F = 1) on A L rings that hold the de-interleaved antennas delayed by l = 0 .. L-1 samples (the rings are prepared outside
the timed region).  Writes profiles/trk_array_times.json.  Each figure is the host's perf_counter time around ten back-to-back calls
(for the bank: ten rounds of A L calls), divided by ten; two warm-up rounds, then five repeats with the two alternating in the same
process; the median and `spread` = (max - min) / median of the five.  Neither entry moves anything, so every call sees the same epoch.
Usage: python tools/trk_array_time.py [--out profiles/trk_array_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 1), (4, 2), (4, 4), (8, 4)]
CALLS, REPEATS, WARMUP = 10, 5, 2
FS, N, RECORDS = 25.0e6, 25000, 32
N_TIME = 2 * N + 8


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trk_array_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, tracking as T
    _lib.init(0)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    mgr = T.TrackingManager(FS, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    rng = np.random.default_rng(1)
    states = []
    for r in range(RECORDS):
        s = T.TrkState()
        s.prn, s.active, s.next_sample_index = 1 + r % 31, 1, 8 + int(rng.integers(0, N))
        s.carrier_freq, s.carrier_phase, s.code_phase, s.code_rate = float(rng.uniform(-5000, 5000)), 0.3, float(rng.uniform(0, 1023)), 1.023e6
        states.append(s)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    rows = []
    for A, L in SHAPES:
        x = np.clip(np.rint(20.0 * rng.standard_normal((N_TIME, A, 2))), -128, 127).astype(np.int8)
        d_x = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_x), x.nbytes) == 0 and hip.hipMemcpy(d_x, x.ctypes.data, x.nbytes, 1) == 0
        xc = x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)
        rings = []
        for l in range(L):
            for a in range(A):
                ring = T.MulticastRingBuffer(1 << 16)
                ring.write_samples(np.concatenate([np.zeros(l, np.complex64), xc[:N_TIME - l, a].astype(np.complex64)]))
                rings.append(ring)

        def array():
            z, done = mgr.array_prompts(d_x.value, N_TIME, A, L, states=states, fmt=_lib.FMT_I8_IQ)
            assert done.all()
            return z

        def banks():
            out = [mgr.bank(ring, [0.0], states=states)[0][:, 0, 0] for ring in rings]
            return np.stack(out, axis=1).reshape(RECORDS, L, A)

        za, zb = array(), banks()                   # the two compute the same words (to the tracking tolerance)
        assert np.max(np.abs(za - zb)) <= 1e-4 * np.max(np.abs(za)), (A, L)
        for _ in range(WARMUP):
            timed(array)
            timed(banks)
        t_new, t_old = [], []
        for _ in range(REPEATS):
            t_new.append(timed(array))
            t_old.append(timed(banks))
        new, old = _stats(t_new), _stats(t_old)
        gain = old["median_ms"] - new["median_ms"]
        row = dict(n_antennas=A, taps=L, records=RECORDS, samples_per_record=N, fmt="int8 IQ", array_prompts=new, bank_calls=A * L,
                   bank_calls_total=old, bank_over_array=round(old["median_ms"] / new["median_ms"], 3),
                   faster_by_more_than_the_larger_spread=bool(gain > max(new["spread"] * new["median_ms"], old["spread"] * old["median_ms"])))
        print(json.dumps(row), flush=True)
        rows.append(row)
        for ring in rings:
            ring.close()
        hip.hipFree(d_x)
    mgr.close()
    meta = dict(tool="tools/trk_array_time.py", calls=CALLS, repeats=REPEATS, warmup_rounds=WARMUP,
                timing="host perf_counter time around ten back-to-back synchronous calls, divided by ten: gm_trk_array_prompts on 32 records "
                       "at 25 Msps, int8 IQ (the record upload, two kernels, the copy back and the wait), and A L calls of gm_trk_bank (T = 1, "
                       "F = 1) on A L rings of de-interleaved, delayed copies prepared outside the timed region; one process, two warm-up "
                       "rounds each, five repeats with the two alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
