"""Event times of gm_lcmv_process_dev alone (the block kernel and gm_stap's state kernel) on 2^19 time samples of int8 IQ in device
memory, for (A, L) = (4, 2), (4, 4) and (8, 4) at B = 1024, with P = 4 and P = 12 beams of Q = 1 constraint each and P = 4 beams of Q = 2
(P = 12 with Q = 2 would be 24 rows, above the 16 a handle carries).  The yardstick, in the same process and alternating with it, is
gm_beamformer_process_dev at the same (A, L, B, P) on the same input, its rows the beams' first rows.  Writes profiles/lcmv_times.json.
Each figure is the HIP-event time around `iters` back-to-back calls on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the two alternating; the median and `spread` = (max - min) / median of the five.
Usage: python tools/lcmv_time.py [--iters 20] [--out profiles/lcmv_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = tuple((A, L, 1024, P, Q) for A, L in ((4, 2), (4, 4), (8, 4)) for P, Q in ((4, 1), (4, 2), (12, 1)))
BLOCK = 1 << 19
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lcmv_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, beamformer, lcmv
    _lib.init(0)
    hip = C.CDLL("libamdhip64.so.7")            # the runtime the library already loaded: plain device buffers, a stream and two events
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0            # hipStreamNonBlocking
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    rng = np.random.default_rng(3)
    a_max, p_max = max(s[0] for s in SHAPES), max(s[3] for s in SHAPES)
    x_iq = np.clip(np.rint(30.0 * rng.standard_normal((BLOCK, a_max, 2))), -128, 127).astype(np.int8)
    d_iq, d_y = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_iq), x_iq.nbytes) == 0 and hip.hipMalloc(C.byref(d_y), p_max * BLOCK * 8) == 0
    assert hip.hipMemcpy(d_iq, x_iq.ctypes.data, x_iq.nbytes, 1) == 0

    def timed(fn):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(args.iters):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / args.iters

    rows = []
    for A, L, B, P, Q in SHAPES:
        M = A * L
        c = (rng.standard_normal((P, Q, M)) + 1j * rng.standard_normal((P, Q, M))).astype(np.complex64)
        f = np.zeros((P, Q), np.complex64)
        f[:, 0] = 1.0                               # the first row answers 1, the second 0
        lc = lcmv.Lcmv(A, L, [(c[p], f[p]) for p in range(P)], block=B)
        bf = beamformer.Beamformer(A, L, c[:, 0], B)
        step_lc = lambda: lc.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, BLOCK, stream.value)
        step_bf = lambda: bf.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, BLOCK, stream.value)
        for _ in range(2):
            timed(step_lc)
            timed(step_bf)
        t_lc, t_bf = [], []
        for _ in range(REPEATS):
            t_lc.append(timed(step_lc))
            t_bf.append(timed(step_bf))
        for h in (lc, bf):
            got = h.stats()
            assert got["outputs"] == got["inputs"] and got["blocks"] * B == got["outputs"] and got["fallbacks"] == [0] * P
        med, med_bf = float(np.median(t_lc)), float(np.median(t_bf))
        larger_spread = max((max(t_lc) - min(t_lc)) / med, (max(t_bf) - min(t_bf)) / med_bf)
        row = dict(n_antennas=A, taps=L, block=B, n_beams=P, constraints_per_beam=Q, time_samples=BLOCK, lcmv=_stats(t_lc),
                   beamformer=_stats(t_bf), lcmv_over_beamformer=round(med / med_bf, 4),
                   inside_the_larger_spread=bool(abs(med - med_bf) <= larger_spread * med_bf))
        print(json.dumps(row), flush=True)
        rows.append(row)
        lc.close()
        bf.close()
    for p in (d_iq, d_y):
        hip.hipFree(p)
    meta = dict(tool="tools/lcmv_time.py", iters=args.iters, repeats=REPEATS,
                timing="HIP-event time around `iters` back-to-back gm_lcmv_process_dev calls (the block kernel and gm_stap's state kernel) "
                       "on 2^19 int8-IQ time samples of A antennas on one non-blocking stream, and around as many "
                       "gm_beamformer_process_dev calls at the same (A, L, B, P) with the beams' first rows, on the same stream; one "
                       "process, two warm-up rounds each, five repeats with the two alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
