"""Event times of gm_excisor_process_dev with the block-adapt mode off and on (gm_excisor_set_block_adapt: a mask per block, decided
between the two transforms) on a block of 2^19 int8-IQ samples in device memory, at B = 1024 and 4096, beside the digital front-end's
own kernel (gm_frontend_process_dev) on the same block in the same process as the yardstick; writes profiles/excise_block_times.json.
tools/excise_time.py's method: each figure is the HIP-event time around `iters` back-to-back calls on one non-blocking stream, divided
by `iters`; two warm-up rounds, then five repeats with the three steps (off, on, front-end) alternating; the median and `spread` =
(max - min) / median of the five.  The samples are noise with a CW on top that sweeps over the band, so the mode has something to
flag in every block; factor 16, guard 2; the static gains are all ones; blanking is off.  `off_vs_static` compares the mode-off median
with profiles/excise_times.json's figure for the same block length, when that file is there.
Usage: python tools/excise_block_time.py [--iters 20] [--out profiles/excise_block_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = [1024, 4096]
BLOCK = 1 << 19
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def _static_figures():
    try:
        with open(os.path.join(ROOT, "profiles", "excise_times.json")) as f:
            rows = json.load(f)["blocks"]
        return {r["block"]: r["process"]["median_ms"] for r in rows if r["blank_threshold"] == 0.0}
    except (OSError, KeyError, ValueError):
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "excise_block_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, excise, frontend
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
    t = np.arange(BLOCK, dtype=np.float64)
    cycles = -0.4 * t + 0.5 * (0.8 / BLOCK) * t * t                          # -0.4 .. +0.4 cycles a sample over the block
    cw = 40.0 * np.exp(2j * np.pi * (cycles - np.floor(cycles)))
    x = np.stack([np.clip(np.round(rng.normal(0, 12, BLOCK) + cw.real), -127, 127),
                  np.clip(np.round(rng.normal(0, 12, BLOCK) + cw.imag), -127, 127)], axis=1).astype(np.int8)
    d_x, d_y, d_fe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cap = BLOCK + 4096
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
    static = _static_figures()
    rows = []
    for block in BLOCKS:
        off, on = excise.Excisor(block), excise.Excisor(block).set_block_adapt(guard_bins=2)
        step_off = lambda: off.process_dev(d_x.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, cap, stream.value)
        step_on = lambda: on.process_dev(d_x.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, cap, stream.value)
        for _ in range(2):
            timed(step_off)
            timed(step_on)
            timed(front)
        on.reset(0)
        t_off, t_on, t_fe = [], [], []
        for _ in range(REPEATS):
            t_off.append(timed(step_off))
            t_on.append(timed(step_on))
            t_fe.append(timed(front))
        st = on.block_stats()
        m_off, m_on, m_fe = (float(np.median(v)) for v in (t_off, t_on, t_fe))
        row = dict(block=block, threshold_factor=16.0, guard_bins=2, block_samples=BLOCK, blocks_counted=st["blocks"],
                   blocks_flagged_share=round(st["blocks_flagged"] / st["blocks"], 4), bins_zeroed_per_block=round(st["bins_zeroed"] / st["blocks"], 2),
                   off=_stats(t_off), on=_stats(t_on), frontend=_stats(t_fe),
                   on_over_off=round(m_on / m_off, 4), on_over_frontend=round(m_on / m_fe, 4), off_over_frontend=round(m_off / m_fe, 4))
        if block in static:
            row["static_median_ms"] = static[block]
            row["off_vs_static"] = round(m_off / static[block] - 1.0, 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        off.close(); on.close()
    fe.close()
    for p in (d_x, d_y, d_fe):
        hip.hipFree(p)
    meta = dict(tool="tools/excise_block_time.py", iters=args.iters, repeats=REPEATS, sample_format="int8 IQ",
                timing="HIP-event time around `iters` back-to-back gm_excisor_process_dev calls (the output kernel and the state kernel) of a "
                       "handle with the block-adapt mode off, of one with it on (factor 16, guard 2), and around as many "
                       "gm_frontend_process_dev calls on the same block and stream; one process, two warm-up rounds each, five repeats "
                       "with the three alternating; median and spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, blocks=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
