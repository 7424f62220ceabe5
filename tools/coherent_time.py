"""Stage F and stage C times of coherent acquisition (gm_acq_cfg.coherent_periods) for four dwell shapes, measured with
gm_acq_enable_timing (HIP events on the handle's stream) over repeated device-resident searches; writes profiles/coherent_times.json.
  a  N = 8000,  32 PRN,  41 bins at 250 Hz, K = 1,  M = 20   today's form of a 20 ms dwell
  b  N = 8000,  32 PRN, 201 bins at  50 Hz, K = 10, M = 2
  c  N = 16368, 32 PRN, 201 bins at  50 Hz, K = 10, M = 1
  d  N = 50000, 32 PRN,  41 bins at 250 Hz, K = 5,  M = 2    (any_length)
Usage: python tools/coherent_time.py [--iters 30] [--out profiles/coherent_times.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("a", 8000, 8.0e6, 0.0, 250.0, 41, 1, 20), ("b", 8000, 8.0e6, 0.0, 50.0, 201, 10, 2),
          ("c", 16368, 16.3676e6, 4.1304e6, 50.0, 201, 10, 1), ("d", 50000, 50.0e6, 0.0, 250.0, 41, 5, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherent_times.json"))
    args = ap.parse_args()
    import torch
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    table = O.ca_code_table()
    rows = []
    for name, N, fs, f_if, step, D, K, M in SHAPES:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        sats = [dict(prn_row=4, cn0_dbhz=45.0, doppler_hz=120.0, code_start=N // 3)]
        x = synth.to_i8_iq(synth.make_scene(table, fs, f_if, K * M * N, sats, config_id=500))
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, 33), n_integrations=M, coherent_periods=K,
                                  any_length=N == 50000)
        d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        for _ in range(3):                                       # warm-up
            eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ)
        eng.synchronize()
        eng.enable_timing(True)
        for _ in range(args.iters):
            eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ)
        eng.synchronize()
        t = eng.timing_summary()
        fwd, inv = D * M, 32 * D * M
        row = dict(shape=name, fft_size=N, fs=fs, n_prn=32, n_bins=D, bin_hz=step, coherent_periods=K, n_integrations=M,
                   dwell_ms=K * M * N / fs * 1e3, forward_transforms=fwd, inverse_transforms=inv, launches=t["launches"],
                   stage_f_ms=round(t["avg_mix_fft_ms"], 4), stage_c_ms=round(t["avg_corr_ms"], 4),
                   form=eng.plan_info()["form"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        eng.close()
    meta = dict(tool="tools/coherent_time.py", device=torch.cuda.get_device_name(0), iters=args.iters,
                timing="gm_acq_enable_timing averages over the timed device-resident searches (int8 IQ samples)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
