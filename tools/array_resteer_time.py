"""Wall-clock time of one re-steering update, two ways, in one process (writes profiles/array_resteer_times.json):
  (a) the loop of the synchronous entries: gm_trk_array_prompts (P records), P times gm_array_row_solve, P times
      gm_beamformer_set_steering;
  (b) the device chain on one stream: gm_trk_array_prompts_dev into a slot of a device history, gm_array_rows_solve_dev,
      gm_beamformer_set_steering_dev, timed to the stream's completion (hipStreamSynchronize).
Shapes: P = 4 and 12 beams, (A, L) = (4, 2) and (8, 4), n = 10 vectors a row, 20 captured blocks; 25 Msps (25000 samples a record), int8 IQ.
Each figure is the host's perf_counter time around ten back-to-back updates divided by ten; two warm-up rounds, then five repeats with
the two alternating; the median and `spread` = (max - min) / median of the five.
A second figure: a stream of 40 gm_beamformer_process_dev calls of 25000 time samples each (block 1024), with one update of kind (a),
one of kind (b) or none behind call 20, timed from the first enqueue to the stream's completion: what the drain of (a) costs a stream.
Usage: python tools/array_resteer_time.py [--out profiles/array_resteer_times.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 4, 2), (12, 4, 2), (4, 8, 4), (12, 8, 4)]          # (P, A, L)
CALLS, REPEATS, WARMUP = 10, 5, 2
FS, N, VECTORS, BLOCKS = 25.0e6, 25000, 10, 20
N_TIME = 2 * N + 8
STREAM_CALLS = 40


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def _beats(new, old):
    gain = old["median_ms"] - new["median_ms"]
    return bool(gain > max(new["spread"] * new["median_ms"], old["spread"] * old["median_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_resteer_times.json"))
    args = ap.parse_args()
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, beamformer, tracking as T
    _lib.init(0)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    held = []

    def dev(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(int(nbytes), 1)) == 0
        if src is not None:
            assert hip.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
        else:
            assert hip.hipMemset(p, 0, max(int(nbytes), 1)) == 0
        assert hip.hipDeviceSynchronize() == 0
        held.append(p)
        return p.value

    def host(ptr, nbytes, dtype):
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
        return out

    s = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0
    stream = s.value
    sync = lambda: hip.hipStreamSynchronize(stream)
    rng = np.random.default_rng(1)
    mgr = T.TrackingManager(FS, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)

    def states(P):
        out = []
        for r in range(P):
            st = T.TrkState()
            st.prn, st.active, st.next_sample_index = 1 + r % 31, 1, 8 + int(rng.integers(0, N))
            st.carrier_freq, st.carrier_phase, st.code_phase, st.code_rate = float(rng.uniform(-5000, 5000)), 0.3, float(rng.uniform(0, 1023)), 1.023e6
            out.append(st)
        return out

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    rows, stream_row = [], None
    for P, A, L in SHAPES:
        M = A * L
        x = np.clip(np.rint(20.0 * rng.standard_normal((N_TIME, A, 2))), -128, 127).astype(np.int8)
        d_x = dev(x.nbytes, x)
        steer = np.ascontiguousarray(rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M)), np.complex64)
        bf = beamformer.Beamformer(A, L, steer, 1024, 1e-4)
        d_y, d_R, d_w = dev(P * N_TIME * 8), dev(BLOCKS * M * M * 8), dev(BLOCKS * P * M * 8)
        bf.capture(d_R, d_w, BLOCKS)
        assert bf.process_dev(d_x, _lib.FMT_I8_IQ, BLOCKS * 1024, d_y, N_TIME) == BLOCKS * 1024
        bf.synchronize()
        bf.capture(None, None, 0)
        R = host(d_R, BLOCKS * M * M * 8, np.complex64).reshape(BLOCKS, M, M)
        # a history of VECTORS epochs, the same on both sides
        hist = np.zeros((VECTORS, P, M), np.complex64)
        for e in range(VECTORS):
            z, done = mgr.array_prompts(d_x, N_TIME, A, L, states=states(P), fmt=_lib.FMT_I8_IQ)
            assert done.all()
            hist[e] = z.reshape(P, M)
        d_hist = dev(hist.nbytes, hist)
        d_done, d_rows, d_info, d_inst = dev(P), dev(P * M * 8), dev(P * 24), dev(P)
        st = states(P)

        def old():
            z, _ = mgr.array_prompts(d_x, N_TIME, A, L, states=st, fmt=_lib.FMT_I8_IQ)
            hist[0] = z.reshape(P, M)
            for p in range(P):
                row, _ = AQ.solve_row(hist[:, p], R, 1e-4)
                bf.set_steering(p, row)

        def new():
            mgr.array_prompts_dev(d_x, N_TIME, A, st, d_hist, d_done, taps=L, fmt=_lib.FMT_I8_IQ, stream=stream)
            AQ.solve_rows_dev(M, VECTORS, P, d_hist, d_rows, d_info, d_R=d_R, n_blocks=BLOCKS, row_stride=M, vec_stride=P * M, loading=1e-4,
                              stream=stream)
            bf.set_steering_dev(0, P, d_rows, d_info, 0.0, d_inst, stream=stream)
            sync()

        old(); new()
        assert host(d_inst, P, np.uint8).all()
        for _ in range(WARMUP):
            timed(old); timed(new)
        t_new, t_old = [], []
        for _ in range(REPEATS):
            t_new.append(timed(new)); t_old.append(timed(old))
        a, b = _stats(t_old), _stats(t_new)
        row = dict(beams=P, n_antennas=A, taps=L, vectors=VECTORS, blocks=BLOCKS, samples_per_record=N, fmt="int8 IQ", host_loop=a, device_chain=b,
                   host_over_device=round(a["median_ms"] / b["median_ms"], 3), device_beats_host_by_more_than_the_larger_spread=_beats(b, a))
        print(json.dumps(row), flush=True)
        rows.append(row)

        if (P, A, L) == (12, 4, 2):                          # the drain: 40 calls of one code period each with one update in the middle
            def run(kind):
                t0 = time.perf_counter()
                for k in range(STREAM_CALLS):
                    bf.process_dev(d_x, _lib.FMT_I8_IQ, N, d_y, N_TIME, stream=stream)
                    if k == STREAM_CALLS // 2 - 1:
                        if kind == "host":
                            z, _ = mgr.array_prompts(d_x, N_TIME, A, L, states=st, fmt=_lib.FMT_I8_IQ)
                            hist[0] = z.reshape(P, M)
                            for p in range(P):
                                bf.set_steering(p, AQ.solve_row(hist[:, p], R, 1e-4)[0])
                        elif kind == "device":
                            mgr.array_prompts_dev(d_x, N_TIME, A, st, d_hist, d_done, taps=L, fmt=_lib.FMT_I8_IQ, stream=stream)
                            AQ.solve_rows_dev(M, VECTORS, P, d_hist, d_rows, d_info, d_R=d_R, n_blocks=BLOCKS, row_stride=M, vec_stride=P * M,
                                              loading=1e-4, stream=stream)
                            bf.set_steering_dev(0, P, d_rows, d_info, 0.0, d_inst, stream=stream)
                sync()
                return (time.perf_counter() - t0) * 1e3
            kinds = ("none", "host", "device")
            for _ in range(WARMUP):
                for k in kinds:
                    run(k)
            t = {k: [] for k in kinds}
            for _ in range(REPEATS):
                for k in kinds:
                    t[k].append(run(k))
            st_ = {k: _stats(v) for k, v in t.items()}
            stream_row = dict(beams=P, n_antennas=A, taps=L, calls=STREAM_CALLS, samples_per_call=N, block=1024, fmt="int8 IQ", no_update=st_["none"],
                              host_update=st_["host"], device_update=st_["device"],
                              host_update_costs_ms=round(st_["host"]["median_ms"] - st_["none"]["median_ms"], 4),
                              device_update_costs_ms=round(st_["device"]["median_ms"] - st_["none"]["median_ms"], 4),
                              device_beats_host_by_more_than_the_larger_spread=_beats(st_["device"], st_["host"]))
            print(json.dumps(stream_row), flush=True)
        bf.close()
    mgr.close()
    hip.hipStreamDestroy(s)
    for p in held:
        hip.hipFree(p)
    meta = dict(tool="tools/array_resteer_time.py", calls=CALLS, repeats=REPEATS, warmup_rounds=WARMUP,
                timing="host perf_counter time around ten back-to-back updates, divided by ten: (host_loop) gm_trk_array_prompts on P records, P "
                       "calls of gm_array_row_solve on 10 vectors and 20 captured blocks, P calls of gm_beamformer_set_steering; (device_chain) "
                       "gm_trk_array_prompts_dev, gm_array_rows_solve_dev and gm_beamformer_set_steering_dev on one stream, to "
                       "hipStreamSynchronize; one process, two warm-up rounds each, five repeats with the two alternating; median and spread = "
                       "(max - min) / median.  stream: 40 gm_beamformer_process_dev calls of 25000 time samples on that stream with one "
                       "update, or none, behind call 20, first enqueue to hipStreamSynchronize, three kinds alternating")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows, stream=stream_row), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
