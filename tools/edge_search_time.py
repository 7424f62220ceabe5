"""Times of the edge search of coherent acquisition (gm_acq_set_edge_search) against what a caller did before it existed: H plain
coherent search_dev calls on the same buffer at pointers advanced by o_h periods.  Both run in this process on the same device, int8 IQ
samples resident; writes profiles/edge_search_times.json.
  a  N = 8000,  32 PRN, 21 bins at 25 Hz, K = 20, M = 2, H = 20 (offsets 0..19)
  b  the same at 4 PRN
  c  N = 16368, 32 PRN, 21 bins at 50 Hz, K = 10, M = 1, H = 10
  d  N = 50000, 32 PRN, 21 bins at 50 Hz, K = 5,  M = 2, H = 5   (any_length)
Per shape: stage F and stage C (the reduction included) from gm_acq_enable_timing (HIP events on the handle's stream), and the whole
dwell as wall time around `iters` back-to-back searches and one synchronisation, five repeats of each; `spread` is (max - min) / median
of the five, the run-to-run margin the comparison is read against.
Usage: python tools/edge_search_time.py [--iters 20] [--out profiles/edge_search_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, N, fs, f_if, bin step, bins, K, M, H, PRNs)
SHAPES = [("a", 8000, 8.0e6, 0.0, 25.0, 21, 20, 2, 20, 32), ("b", 8000, 8.0e6, 0.0, 25.0, 21, 20, 2, 20, 4),
          ("c", 16368, 16.3676e6, 4.1304e6, 50.0, 21, 10, 1, 10, 32), ("d", 50000, 50.0e6, 0.0, 50.0, 21, 5, 2, 5, 32)]
REPEATS = 5


def _wall_ms(run, sync, iters):
    """five repeats of `iters` back-to-back calls of run() and one sync(): ms per call of each repeat"""
    out = []
    for _ in range(REPEATS):
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_search_times.json"))
    args = ap.parse_args()
    import torch
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    table = O.ca_code_table()
    rows = []
    for name, N, fs, f_if, step, D, K, M, H, P in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        offsets = list(range(H))
        n = (K * M + offsets[-1]) * N
        sats = [dict(prn_row=4, cn0_dbhz=45.0, doppler_hz=120.0, code_start=N // 3)]
        x = synth.to_i8_iq(synth.make_scene(table, fs, f_if, n, sats, config_id=700))
        d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        base = d_x.data_ptr()
        kw = dict(doppler_hz=dop, prn_ids=np.arange(1, P + 1), n_integrations=M, coherent_periods=K, any_length=N == 50000)
        # what a caller does without the edge search: H plain coherent searches at pointers advanced by o_h periods (2 bytes a sample)
        plain = A.AcquisitionEngine(fs, f_if, N, **kw)

        def run_plain():
            for o in offsets:
                plain.search_dev(base + o * N * 2, A.FMT_I8_IQ)

        for _ in range(2):
            run_plain()
        before = _wall_ms(run_plain, plain.synchronize, args.iters)
        plain.enable_timing(True)
        for _ in range(args.iters):
            plain.search_dev(base, A.FMT_I8_IQ)
        plain.synchronize()
        tp = plain.timing_summary()
        plain.close()
        eng = A.AcquisitionEngine(fs, f_if, N, **kw)
        eng.set_edge_search(offsets)
        assert eng.dwell_samples == n

        def run_edge():
            eng.search_dev(base, A.FMT_I8_IQ)

        for _ in range(3):
            run_edge()
        after = _wall_ms(run_edge, eng.synchronize, args.iters)
        eng.enable_timing(True)
        for _ in range(args.iters):
            run_edge()
        eng.synchronize()
        te = eng.timing_summary()
        form = eng.plan_info()["form"]
        eng.close()
        sb, sa = _stats(before), _stats(after)
        row = dict(shape=name, fft_size=N, fs=fs, n_prn=P, n_bins=D, bin_hz=step, coherent_periods=K, n_integrations=M, hypotheses=H,
                   form=form, dwell_ms=n / fs * 1e3, forward_transforms=H * D * M, inverse_transforms=P * H * D * M,
                   stage_f_ms=round(te["avg_mix_fft_ms"], 4), stage_c_ms=round(te["avg_corr_ms"], 4),
                   plain_one_search_stage_f_ms=round(tp["avg_mix_fft_ms"], 4), plain_one_search_stage_c_ms=round(tp["avg_corr_ms"], 4),
                   edge_search=sa, h_plain_searches=sb, ratio_edge_over_plain=round(sa["median_ms"] / sb["median_ms"], 4),
                   margin=round(max(sa["spread"], sb["spread"]), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    meta = dict(tool="tools/edge_search_time.py", device=torch.cuda.get_device_name(0), iters=args.iters, repeats=REPEATS,
                timing="stage times: gm_acq_enable_timing averages; edge_search / h_plain_searches: wall time per dwell over back-to-back "
                       "device-resident searches (int8 IQ), five repeats; ratio = edge median / H-plain-calls median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
