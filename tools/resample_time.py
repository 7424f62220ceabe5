"""Event times of the rate-conversion step alone (gm_resampler_process_dev: the output kernel and the state kernel) on a block of 2^19
int8-IQ samples in device memory, for three ratios, beside the digital front-end's own kernel (gm_frontend_process_dev) on the same
block in the same process as the yardstick; writes profiles/resample_times.json.  Ratios:
  4/25          50 Msps -> 8 Msps, 224 taps (the default), blend weight exactly 0 (4 divides 256: one table row per output)
  40920/40919   16.3676 Msps -> 16.368 Msps, 32 taps, blended rows
  2/1           32 taps, twice the outputs
Each figure is the HIP-event time around `iters` back-to-back calls on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the resampler and the front-end alternating; the median and `spread` = (max - min) / median of the five.  The
samples are noise (the time does not depend on them); blanking is off, and on (threshold 60) in a second row per ratio, which adds the
counting pass over the inputs.
Usage: python tools/resample_time.py [--iters 20] [--out profiles/resample_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = [(4, 25), (40920, 40919), (2, 1)]
BLOCK = 1 << 19
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, frontend, resample
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
    x = np.random.default_rng(3).integers(-40, 41, (BLOCK, 2)).astype(np.int8)
    d_x, d_y, d_fe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cap = 2 * BLOCK + 2
    assert hip.hipMalloc(C.byref(d_x), x.nbytes) == 0 and hip.hipMalloc(C.byref(d_y), cap * 8) == 0
    assert hip.hipMalloc(C.byref(d_fe), BLOCK * 8) == 0
    assert hip.hipMemcpy(d_x, x.ctypes.data, x.nbytes, 1) == 0

    def timed(fn):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(args.iters):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / args.iters

    fe = frontend.DigitalFrontend(2.0e6, 8.0e6, 8.0e6)
    front = lambda: fe.process_dev(d_x.value, _lib.FMT_I8_IQ, d_fe.value, BLOCK, stream.value)
    rows = []
    for up, down in RATIOS:
        for thr in (0.0, 60.0):
            rs = resample.Resampler(up, down, blank_threshold=thr)
            step = lambda: rs.process_dev(d_x.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, cap, stream.value)
            for _ in range(2):
                timed(step)
                timed(front)
            t_rs, t_fe = [], []
            for _ in range(REPEATS):
                t_rs.append(timed(step))
                t_fe.append(timed(front))
            st = rs.stats()
            row = dict(up=rs.up, down=rs.down, taps=rs.n_taps, n_phases=rs.n_phases, blank_threshold=thr, block_samples=BLOCK,
                       outputs_per_block=round(st["outputs"] / (st["inputs"] / BLOCK), 1), blanked_share=round(st["blanked"] / st["inputs"], 4),
                       resample=_stats(t_rs), frontend=_stats(t_fe),
                       resample_over_frontend=round(float(np.median(t_rs)) / float(np.median(t_fe)), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
            rs.close()
    fe.close()
    for p in (d_x, d_y, d_fe):
        hip.hipFree(p)
    meta = dict(tool="tools/resample_time.py", iters=args.iters, repeats=REPEATS, sample_format="int8 IQ",
                timing="HIP-event time around `iters` back-to-back gm_resampler_process_dev calls (the output kernel and the state kernel) "
                       "on one non-blocking stream, and around as many gm_frontend_process_dev calls on the same block and stream; one "
                       "process, two warm-up rounds each, five repeats with the two alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, ratios=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
