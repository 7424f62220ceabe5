"""Times of acquisition with code-drift compensation (gm_acq_set_code_drift, T = fft_size - 0.4 in every bin) against the same handle
with the compensation off, in this process on the same device, int8 IQ samples resident; writes profiles/code_drift_times.json.  With
the compensation off the handle launches the kernels it launched before it existed, so the off-run is the baseline.
  a   N = 8000,  32 PRN, 21 bins at 25 Hz, K = 20, M = 2,  edge search H = 20 (offsets 0..19)     (README's edge-search row a)
  c   N = 16368, 32 PRN, 21 bins at 50 Hz, K = 10, M = 1,  edge search H = 10                     (row c)
  k1  N = 16368, 32 PRN, 21 bins at 50 Hz, K = 1,  M = 40, no edge search
Per shape and state: stage F from gm_acq_enable_timing (HIP events on the handle's stream) averaged over `iters` searches, and the
whole dwell as wall time around `iters` back-to-back searches and one synchronisation; five repeats of each, the median and
`spread` = (max - min) / median of the five, the run-to-run margin the ratio is read against.  The states alternate (off, on, off,
on, ...) so that a drift of the device's clocks falls on both.
Usage: python tools/code_drift_time.py [--iters 20] [--out profiles/code_drift_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, N, fs, f_if, bin step, bins, K, M, H, PRNs)
SHAPES = [("a", 8000, 8.0e6, 0.0, 25.0, 21, 20, 2, 20, 32), ("c", 16368, 16.3676e6, 4.1304e6, 50.0, 21, 10, 1, 10, 32),
          ("k1", 16368, 16.3676e6, 4.1304e6, 50.0, 21, 1, 40, 0, 32)]
REPEATS = 5


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_drift_times.json"))
    args = ap.parse_args()
    import torch
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    table = O.ca_code_table()
    rows = []
    for name, N, fs, f_if, step, D, K, M, H, P in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        T = N - 0.4
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, P + 1), n_integrations=M, coherent_periods=K)
        if H:
            eng.set_edge_search(list(range(H)))
        n_off = eng.dwell_samples
        eng.set_code_drift(T)
        n_on = eng.dwell_samples
        sats = [dict(prn_row=4, cn0_dbhz=45.0, doppler_hz=120.0, code_start=N // 3)]
        x = synth.to_i8_iq(synth.make_scene(table, fs, f_if, max(n_on, n_off), sats, config_id=710))
        d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        base = d_x.data_ptr()

        def run():
            eng.search_dev(base, A.FMT_I8_IQ)

        wall, stage_f, stage_c = {"off": [], "on": []}, {"off": [], "on": []}, {"off": [], "on": []}
        for rep in range(REPEATS + 1):                     # (the first round warms both states up and is dropped)
            for state in ("off", "on"):
                eng.set_code_drift(T if state == "on" else None)
                eng.enable_timing(False)
                for _ in range(3):
                    run()
                eng.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    run()
                eng.synchronize()
                w = (time.perf_counter() - t0) * 1e3 / args.iters
                eng.enable_timing(True)
                for _ in range(args.iters):
                    run()
                eng.synchronize()
                t = eng.timing_summary()
                if rep:
                    wall[state].append(w)
                    stage_f[state].append(t["avg_mix_fft_ms"])
                    stage_c[state].append(t["avg_corr_ms"])
        form = eng.plan_info()["form"]
        eng.close()
        f_on, f_off, w_on, w_off = _stats(stage_f["on"]), _stats(stage_f["off"]), _stats(wall["on"]), _stats(wall["off"])
        row = dict(shape=name, fft_size=N, fs=fs, n_prn=P, n_bins=D, bin_hz=step, coherent_periods=K, n_integrations=M, hypotheses=H,
                   form=form, period_samples=T, dwell_samples_on=n_on, dwell_samples_off=n_off, forward_transforms=max(H, 1) * D * M,
                   stage_f_on=f_on, stage_f_off=f_off, stage_c_on=_stats(stage_c["on"]), stage_c_off=_stats(stage_c["off"]),
                   dwell_on=w_on, dwell_off=w_off,
                   stage_f_ratio_on_over_off=round(f_on["median_ms"] / f_off["median_ms"], 4), stage_f_margin=round(f_off["spread"] + 0.10, 4),
                   dwell_ratio_on_over_off=round(w_on["median_ms"] / w_off["median_ms"], 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    meta = dict(tool="tools/code_drift_time.py", device=torch.cuda.get_device_name(0), iters=args.iters, repeats=REPEATS,
                timing="stage_f / stage_c: gm_acq_enable_timing averages over `iters` searches; dwell: wall time per dwell over back-to-back "
                       "device-resident searches (int8 IQ); five repeats each, states alternating; ratio = on median / off median; "
                       "stage_f_margin = the off-run's own spread + 0.10, what the ratio - 1 is read against")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
