"""Event times of the beamforming step alone (gm_beamformer_process_dev: the block kernel and gm_stap's state kernel) on 2^19 time samples
of int8 IQ in device memory, for (A, L, B, P) = (4, 1, 1024, 8), (4, 2, 1024, 8), (4, 4, 1024, 8), (8, 4, 1024, 12) and (4, 4, 1024, 1).
The yardstick, in the same process and alternating with it, is what a caller did before the entry existed: P gm_stap_process_dev calls
of P handles at the same (A, L, B) on the same input, one after the other on the same stream.  The floor is the time the call's bytes
(the input read once plus P output planes) take at the HBM rate, 6.29 TB/s: the float4 copy rate measured on an MI355X.  Writes
profiles/beam_times.json.
Each figure is the HIP-event time around `iters` back-to-back steps on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the two alternating; the median and `spread` = (max - min) / median of the five.
Usage: python tools/beam_time.py [--iters 20] [--out profiles/beam_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4, 1, 1024, 8), (4, 2, 1024, 8), (4, 4, 1024, 8), (8, 4, 1024, 12), (4, 4, 1024, 1))
BLOCK = 1 << 19
REPEATS = 5
HBM_BYTES_PER_S = 6.29e12


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, beamformer, stap
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
    for A, L, B, P in SHAPES:
        M = A * L
        s = (rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M))).astype(np.complex64)
        s[0] = 0
        s[0, 0] = 1.0                               # the power-inversion row
        bf = beamformer.Beamformer(A, L, s, B)
        sts = [stap.Stap(A, L, B, steering=s[p]) for p in range(P)]
        step = lambda: bf.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, BLOCK, stream.value)

        def staps():
            for p, st in enumerate(sts):
                st.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value + p * BLOCK * 8, BLOCK, stream.value)

        for _ in range(2):
            timed(step)
            timed(staps)
        t_bf, t_st = [], []
        for _ in range(REPEATS):
            t_bf.append(timed(step))
            t_st.append(timed(staps))
        got = bf.stats()
        assert got["outputs"] == got["inputs"] and got["blocks"] * B == got["outputs"] and got["fallbacks"] == [0] * P
        nbytes = BLOCK * A * 2 + P * BLOCK * 8
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        med, med_st = float(np.median(t_bf)), float(np.median(t_st))
        larger_spread = max((max(t_bf) - min(t_bf)) / med, (max(t_st) - min(t_st)) / med_st)
        row = dict(n_antennas=A, taps=L, block=B, n_beams=P, time_samples=BLOCK, bytes=nbytes, floor_ms=round(floor_ms, 5),
                   beamformer=_stats(t_bf), p_stap_calls=_stats(t_st), beamformer_over_p_stap_calls=round(med / med_st, 4),
                   under_the_stap_calls_by_more_than_the_larger_spread=bool(med < med_st * (1.0 - larger_spread)),
                   beamformer_over_floor=round(med / floor_ms, 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
        bf.close()
        for st in sts:
            st.close()
    for p in (d_iq, d_y):
        hip.hipFree(p)
    meta = dict(tool="tools/beam_time.py", iters=args.iters, repeats=REPEATS, hbm_bytes_per_s=HBM_BYTES_PER_S,
                timing="HIP-event time around `iters` back-to-back gm_beamformer_process_dev calls (the block kernel and gm_stap's state "
                       "kernel) on 2^19 int8-IQ time samples of A antennas on one non-blocking stream, and around as many rounds of P "
                       "gm_stap_process_dev calls of P handles at the same (A, L, B), each with one of the P rows, on the same stream; one "
                       "process, two warm-up rounds each, five repeats with the two alternating; median and spread = (max - min) / median; "
                       "floor = (input bytes + P planes of output bytes) / 6.29 TB/s; at P = 1 the ratio is to one gm_stap call")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
