"""Event times of the filter bank step alone (gm_channelizer_process_dev: the output kernel and the state kernel) on a block of 2^19
int8-IQ samples in device memory, shape (M, D, P) = (32, 9, 16), with C = 14 (GLONASS's carriers) and C = 32 planes.  Two yardsticks run
in the same process, alternating with it: fourteen gm_resampler_process_dev calls at 1/9 with 256 taps on the same block (the tap work
of fourteen separate down-converters, without their mixers), and the digital front-end's kernel (gm_frontend_process_dev) on the same
block.  Writes profiles/channelizer_times.json.
Each figure is the HIP-event time around `iters` back-to-back steps on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the three alternating; the median and `spread` = (max - min) / median of the five.
Usage: python tools/channelizer_time.py [--iters 20] [--out profiles/channelizer_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, D, P = 32, 9, 16
BLOCK = 1 << 19
REPEATS = 5
N_CARRIERS = 14


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channelizer_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, channelizer, frontend, resample
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
    x_iq = np.clip(np.rint(30.0 * rng.standard_normal((BLOCK, 2))), -128, 127).astype(np.int8)
    cap = BLOCK // D + 2
    d_iq, d_y, d_fe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_iq), x_iq.nbytes) == 0 and hip.hipMalloc(C.byref(d_y), M * cap * 8) == 0
    assert hip.hipMalloc(C.byref(d_fe), BLOCK * 8) == 0
    assert hip.hipMemcpy(d_iq, x_iq.ctypes.data, x_iq.nbytes, 1) == 0

    def timed(fn):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(args.iters):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / args.iters

    fe = frontend.DigitalFrontend(2.0e6, 18.0e6, 18.0e6)
    front = lambda: fe.process_dev(d_iq.value, _lib.FMT_I8_IQ, d_fe.value, BLOCK, stream.value)
    banks = [resample.Resampler(1, D, taps=256) for _ in range(N_CARRIERS)]

    def fourteen():
        for i, rs in enumerate(banks):
            rs.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value + i * cap * 8, cap, stream.value)

    rows = []
    for channels in (channelizer.glonass_channels(M), None):
        ch = channelizer.Channelizer(M, D, channels=channels, taps_per_branch=P)
        step = lambda: ch.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, cap, cap, stream.value)
        for _ in range(2):
            timed(step)
            timed(fourteen)
            timed(front)
        t_ch, t_rs, t_fe = [], [], []
        for _ in range(REPEATS):
            t_ch.append(timed(step))
            t_rs.append(timed(fourteen))
            t_fe.append(timed(front))
        st = ch.stats()
        row = dict(n_channels=M, decim=D, taps_per_branch=P, planes=len(ch.channels), block_samples=BLOCK,
                   outputs_per_block=round(st["outputs"] / (st["inputs"] / BLOCK), 1),
                   channelizer=_stats(t_ch), fourteen_resamplers=_stats(t_rs), frontend=_stats(t_fe),
                   channelizer_over_fourteen=round(float(np.median(t_ch)) / float(np.median(t_rs)), 4),
                   channelizer_over_frontend=round(float(np.median(t_ch)) / float(np.median(t_fe)), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        ch.close()
    for rs in banks:
        rs.close()
    fe.close()
    for p in (d_iq, d_y, d_fe):
        hip.hipFree(p)
    meta = dict(tool="tools/channelizer_time.py", iters=args.iters, repeats=REPEATS,
                timing="HIP-event time around `iters` back-to-back gm_channelizer_process_dev calls (the output kernel and the state "
                       "kernel) on 2^19 int8-IQ samples on one non-blocking stream, around as many rounds of fourteen "
                       "gm_resampler_process_dev calls (1/9, 256 taps) and around as many gm_frontend_process_dev calls on the same block "
                       "and stream; one process, two warm-up rounds each, five repeats with the three alternating; median and spread = "
                       "(max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
