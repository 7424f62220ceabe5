"""Event times of the space-time nulling step alone (gm_stap_process_dev: the block kernel and the state kernel that carries the L - 1
samples in front of the next block) on 2^19 time samples of int8 IQ in device memory, for (A, L) = (2, 8), (4, 4), (4, 8) and (8, 4) at
B = 1024 and 4096.  Two yardsticks run in the same process, alternating with it: gm_nuller_process_dev at the same (A, B) — the stage
does L times its output work and about A L^2 / 2 times its covariance work, plus an M = A L solve per block — and the digital
front-end's kernel (gm_frontend_process_dev) A times on a block of 2^19 samples, what conditioning A antennas separately costs.  The
floor is the time the call's bytes (the input read once plus the output) take at the HBM rate, 6.29 TB/s: the float4 copy rate measured
on an MI355X.  Writes profiles/stap_times.json.
Each figure is the HIP-event time around `iters` back-to-back steps on one non-blocking stream, divided by `iters`; two warm-up rounds,
then five repeats with the three alternating; the median and `spread` = (max - min) / median of the five.
Usage: python tools/stap_time.py [--iters 20] [--out profiles/stap_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = tuple((A, L, B) for B in (1024, 4096) for A, L in ((2, 8), (4, 4), (4, 8), (8, 4)))
BLOCK = 1 << 19
REPEATS = 5
HBM_BYTES_PER_S = 6.29e12


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stap_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, frontend, nuller, stap
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
    a_max = max(a for a, _, _ in SHAPES)
    x_iq = np.clip(np.rint(30.0 * rng.standard_normal((BLOCK, a_max, 2))), -128, 127).astype(np.int8)
    d_iq, d_y, d_fe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_iq), x_iq.nbytes) == 0 and hip.hipMalloc(C.byref(d_y), BLOCK * 8) == 0
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
    rows = []
    for A, L, B in SHAPES:
        st, nl = stap.Stap(A, L, B), nuller.Nuller(A, B)
        step = lambda: st.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, BLOCK, stream.value)
        spatial = lambda: nl.process_dev(d_iq.value, _lib.FMT_I8_IQ, BLOCK, d_y.value, BLOCK, stream.value)

        def fronts():                           # antenna a's 2^19 samples are not contiguous here; the front-end's cost does not depend on which it reads
            for a in range(A):
                fe.process_dev(d_iq.value + a * BLOCK * 2, _lib.FMT_I8_IQ, d_fe.value, BLOCK, stream.value)

        for _ in range(2):
            timed(step)
            timed(spatial)
            timed(fronts)
        t_st, t_nl, t_fe = [], [], []
        for _ in range(REPEATS):
            t_st.append(timed(step))
            t_nl.append(timed(spatial))
            t_fe.append(timed(fronts))
        s = st.stats()
        assert s["outputs"] == s["inputs"] and s["blocks"] * B == s["outputs"] and s["fallback_blocks"] == 0
        nbytes = BLOCK * A * 2 + BLOCK * 8
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        med, med_nl, med_fe = float(np.median(t_st)), float(np.median(t_nl)), float(np.median(t_fe))
        larger_spread = max((max(t_st) - min(t_st)) / med, (max(t_fe) - min(t_fe)) / med_fe)
        row = dict(n_antennas=A, taps=L, block=B, time_samples=BLOCK, bytes=nbytes, floor_ms=round(floor_ms, 5),
                   stap=_stats(t_st), nuller=_stats(t_nl), frontend_a_times=_stats(t_fe),
                   stap_over_nuller=round(med / med_nl, 3), stap_over_frontends=round(med / med_fe, 4),
                   under_the_frontends_by_more_than_the_larger_spread=bool(med < med_fe * (1.0 - larger_spread)),
                   stap_over_floor=round(med / floor_ms, 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
        st.close()
        nl.close()
    fe.close()
    for p in (d_iq, d_y, d_fe):
        hip.hipFree(p)
    meta = dict(tool="tools/stap_time.py", iters=args.iters, repeats=REPEATS, hbm_bytes_per_s=HBM_BYTES_PER_S,
                timing="HIP-event time around `iters` back-to-back gm_stap_process_dev calls (the block kernel and the state kernel of "
                       "the L - 1 carried samples) on 2^19 int8-IQ time samples of A antennas on one non-blocking stream, around as "
                       "many gm_nuller_process_dev calls at the same (A, B), and around as many rounds of A gm_frontend_process_dev "
                       "calls on 2^19 samples, all on the same stream; one process, two warm-up rounds each, five repeats with the "
                       "three alternating; median and spread = (max - min) / median; floor = (input bytes + output bytes) / 6.29 TB/s")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
