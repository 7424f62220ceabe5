"""Event times of the down-conversion step alone (gm_ddc_process_dev: the output kernel and the state kernel) on a block of 2^20 int8
REAL samples in device memory, at 1/2 and at 20460/40919 (16.3676 Msps real at an IF of 4.1304 MHz -> 8.184 Msps complex), with
blanking off and on (threshold 100 on samples of sigma 40).  Two yardsticks run in the same process, alternating with it:
gm_resampler_process_dev on 2^20 int8-IQ samples at the same ratio and blanking (twice the input bytes, no phasor product), and the
digital front-end's kernel (gm_frontend_process_dev) on 2^20 int8-IQ samples.  Writes profiles/ddc_times.json.
Each figure is the HIP-event time around `iters` back-to-back calls on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the three alternating; the median and `spread` = (max - min) / median of the five.
Usage: python tools/ddc_time.py [--iters 20] [--out profiles/ddc_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = [(1, 2), (20460, 40919)]
MIX = 4130400.0 / 16367600.0
BLOCK = 1 << 20
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddc_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, ddc, frontend, resample
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
    x_real = np.clip(np.rint(40.0 * rng.standard_normal(BLOCK)), -128, 127).astype(np.int8)
    x_iq = np.clip(np.rint(40.0 * rng.standard_normal((BLOCK, 2))), -128, 127).astype(np.int8)
    d_real, d_iq, d_y, d_fe = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    cap = BLOCK + 2
    assert hip.hipMalloc(C.byref(d_real), x_real.nbytes) == 0 and hip.hipMalloc(C.byref(d_iq), x_iq.nbytes) == 0
    assert hip.hipMalloc(C.byref(d_y), cap * 8) == 0 and hip.hipMalloc(C.byref(d_fe), BLOCK * 8) == 0
    assert hip.hipMemcpy(d_real, x_real.ctypes.data, x_real.nbytes, 1) == 0
    assert hip.hipMemcpy(d_iq, x_iq.ctypes.data, x_iq.nbytes, 1) == 0

    def timed(fn):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(args.iters):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / args.iters

    fe = frontend.DigitalFrontend(2.0e6, 8.0e6, 8.0e6)
    front = lambda: fe.process_dev(d_iq.value, _lib.FMT_I8_IQ, d_fe.value, BLOCK, stream.value)
    rows = []
    for up, down in RATIOS:
        for thr in (0.0, 100.0):
            dc = ddc.Ddc(MIX, up, down, blank_threshold=thr)
            rs = resample.Resampler(up, down, blank_threshold=thr)
            step = lambda: dc.process_dev(d_real.value, BLOCK, d_y.value, cap, stream.value)
            yard = lambda: rs.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, cap, stream.value)
            for _ in range(2):
                timed(step)
                timed(yard)
                timed(front)
            t_dc, t_rs, t_fe = [], [], []
            for _ in range(REPEATS):
                t_dc.append(timed(step))
                t_rs.append(timed(yard))
                t_fe.append(timed(front))
            st = dc.stats()
            row = dict(up=dc.up, down=dc.down, taps=dc.n_taps, n_phases=dc.n_phases, blank_threshold=thr, block_samples=BLOCK,
                       outputs_per_block=round(st["outputs"] / (st["inputs"] / BLOCK), 1), blanked_share=round(st["blanked"] / st["inputs"], 4),
                       ddc=_stats(t_dc), resample=_stats(t_rs), frontend=_stats(t_fe),
                       ddc_over_resample=round(float(np.median(t_dc)) / float(np.median(t_rs)), 4),
                       ddc_over_frontend=round(float(np.median(t_dc)) / float(np.median(t_fe)), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
            dc.close()
            rs.close()
    fe.close()
    for p in (d_real, d_iq, d_y, d_fe):
        hip.hipFree(p)
    meta = dict(tool="tools/ddc_time.py", iters=args.iters, repeats=REPEATS, mix_cycles_per_sample=MIX,
                timing="HIP-event time around `iters` back-to-back gm_ddc_process_dev calls (the output kernel and the state kernel) on "
                       "2^20 int8 real samples on one non-blocking stream, and around as many gm_resampler_process_dev calls (same ratio "
                       "and blanking) and gm_frontend_process_dev calls on 2^20 int8-IQ samples on the same stream; one process, two "
                       "warm-up rounds each, five repeats with the three alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, ratios=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
