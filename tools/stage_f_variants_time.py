"""Stage-F times of the coherent, the edge-search and the code-drift kernels (csrc/acq_stage_f_variants.h) of the library GM_LIB_PATH
selects (default: the product library), for an A/B of two builds of it: each run is one library in one fresh process.
Thirteen rows, 4 PRN (stage F does not depend on the PRN count) and 21 bins each, int8 IQ samples resident:
  N = 8000   in-LDS                  K = 20, M = 2, H = 20      N = 32000  composite, base 16000   K = 5, M = 2, H = 5
  N = 16368  in-LDS, permuted store  K = 10, M = 1, H = 10      N = 50000  long (any_length)       K = 5, M = 2, H = 5
each as coherent (no H), edge (offsets 0..H-1) and drift (the edge search on, T = N - 0.4), and drift at K = 1, M = 40, N = 16368.
Per row: stage F from gm_acq_enable_timing (HIP events on the handle's stream) averaged over `iters` searches, five repeats after a
warm-up.
  python tools/stage_f_variants_time.py --out run.json                      one run
  python tools/stage_f_variants_time.py --ab p1.json n1.json p2.json n2.json [...] --out profiles/stage_f_variants_ab.json
--ab pools each library's repeats over its runs (parent, new, parent, new, ...) per row.  margin = the parent's own spread, (max -
min) / median over its pooled repeats: what two runs of identical code differ by.  A row passes when the new median is at most the
parent's median * (1 + margin); the exit status is the number of rows that do not."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, fs, f_if, bin step, K, M, H)
SHAPES = [(8000, 8.0e6, 0.0, 25.0, 20, 2, 20), (16368, 16.3676e6, 4.1304e6, 50.0, 10, 1, 10), (32000, 32.0e6, 0.0, 50.0, 5, 2, 5),
          (50000, 50.0e6, 0.0, 50.0, 5, 2, 5)]
ROWS = [(v,) + s for v in ("coherent", "edge", "drift") for s in SHAPES] + [("drift", 16368, 16.3676e6, 4.1304e6, 50.0, 1, 40, 0)]
REPEATS, P, D = 5, 4, 21


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))


def measure(args):
    import torch
    from gnss_sdr_rs_amd import _lib, acquisition as A
    rng = np.random.default_rng(720)
    rows = []
    for variant, N, fs, f_if, step, K, M, H in ROWS:
        dop = (np.arange(D, dtype=np.float32) - (D - 1) / 2) * np.float32(step)
        eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=np.arange(1, P + 1), n_integrations=M, coherent_periods=K,
                                  any_length=N == 50000)
        if H and variant != "coherent":
            eng.set_edge_search(list(range(H)))
        if variant == "drift":
            eng.set_code_drift(N - 0.4)
        d_x = torch.from_numpy(rng.integers(-8, 8, size=(eng.dwell_samples, 2), dtype=np.int8)).cuda()   # (the values do not matter to the time)
        for _ in range(3):
            eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ)
        reps = []
        for _ in range(REPEATS):
            eng.enable_timing(True)
            for _ in range(args.iters):
                eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ)
            eng.synchronize()
            reps.append(round(eng.timing_summary()["avg_mix_fft_ms"], 5))
        info = eng.plan_info()
        eng.close()
        row = dict(variant=variant, fft_size=N, coherent_periods=K, n_integrations=M, hypotheses=H if variant != "coherent" else 0,
                   form=info["form"], base=info["base"], stage_f_ms=reps, **_stats(reps))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return dict(tool="tools/stage_f_variants_time.py", library=os.path.basename(_lib._LIB_PATH), device=torch.cuda.get_device_name(0),
                iters=args.iters, repeats=REPEATS, n_prn=P, n_bins=D, rows=rows)


def ab(args):
    runs = [json.load(open(p)) for p in args.ab]
    libs = [runs[0]["library"], runs[1]["library"]]
    assert all(r["library"] == libs[i % 2] for i, r in enumerate(runs)) and libs[0] != libs[1], "runs alternate: parent, new, parent, new"
    rows, fails = [], 0
    for i, r0 in enumerate(runs[0]["rows"]):
        pool = [sum((r["rows"][i]["stage_f_ms"] for r in runs[s::2]), []) for s in (0, 1)]
        par, new = _stats(pool[0]), _stats(pool[1])
        ok = new["median_ms"] <= par["median_ms"] * (1 + par["spread"])
        fails += not ok
        rows.append(dict({k: r0[k] for k in ("variant", "fft_size", "coherent_periods", "n_integrations", "hypotheses", "form", "base")},
                         parent=dict(par, stage_f_ms=pool[0]), new=dict(new, stage_f_ms=pool[1]),
                         ratio_new_over_parent=round(new["median_ms"] / par["median_ms"], 4), margin=par["spread"], passed=bool(ok)))
        print("%-8s N %5d K %2d M %2d H %2d  parent %.5f ms  new %.5f ms  ratio %.4f  margin %.4f  %s" % (
            r0["variant"], r0["fft_size"], r0["coherent_periods"], r0["n_integrations"], r0["hypotheses"], par["median_ms"], new["median_ms"],
            rows[-1]["ratio_new_over_parent"], par["spread"], "ok" if ok else "BEYOND THE MARGIN"))
    meta = {k: runs[0][k] for k in ("tool", "device", "iters", "repeats", "n_prn", "n_bins")}
    meta.update(parent_library=libs[0], new_library=libs[1], runs=len(runs), order="parent, new, parent, new, ... each a fresh process",
                rule="pass: new median <= parent median * (1 + margin), margin = the parent's (max - min) / median over its pooled repeats")
    return dict(meta=meta, rows=rows), fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ab", nargs="+")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res, fails = ab(args) if args.ab else (measure(args), 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    sys.exit(fails)
