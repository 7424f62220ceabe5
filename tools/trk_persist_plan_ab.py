"""The persistent tracking kernel's launch layout and speed, of the library GM_LIB_PATH names (default: the product library), for an
A/B of two builds of the library.

  --layout            one handle and one two-epoch launch per anchor configuration of tests/cpu/test_trk_persist_plan.cpp on a small
                      ring, then one handle per instantiation key.  Run it under `rocprofv3 --kernel-trace --stats` (a trace run of
                      its own, no counters); with GM_DIAGNOSTICS=1 GM_TRK_PLAN_PRINT=1 gm_trk_create prints what it asked the
                      device and what it decided on stderr (a library without trk_persist_plan.h prints nothing).
  --listing A.csv B.csv [--plans B.stderr] --out profiles/trk_persist_plan_ab.txt
                      the persistent launches of two such traces side by side: kernel name, workgroups, LDS; exit status = the
                      number of rows that differ.
  --time --out X.json bench.py's tracking legs (32 and 256 channels) and its cfg5 leg (what tools/cfg5_time.py runs), REPS times each.
  --ab p1.json n1.json p2.json n2.json ... --out profiles/trk_persist_plan_ab.json
                      pools each library's repeats over its runs (parent, new, parent, new, ...).  margin = the parent's own spread,
                      (max - min) / median over its pooled repeats; a line passes when the new median <= the parent's median *
                      (1 + margin) — the rule of tools/stage_f_variants_time.py --ab; exit status = the lines that do not."""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, arms, fs, code_len, share_device): the anchor rows
ANCHORS = [(32, 3, 25e6, 1023, 0), (32, 3, 4.092e6, 1023, 0), (36, 5, 25e6, 1023, 0), (36, 5, 25e6, 4092, 0), (36, 3, 25e6, 4092, 0),
           (32, 3, 100e6, 1023, 0), (32, 5, 100e6, 1023, 0), (8, 3, 4.092e6, 1023, 0), (8, 5, 100e6, 1023, 0), (64, 5, 25e6, 1023, 0),
           (36, 5, 25e6, 4092, 1)]
REPS = 3


def layout():
    from gnss_sdr_rs_amd import _lib, tracking as T
    _lib.init(0)
    rng = np.random.default_rng(11)
    ring = T.MulticastRingBuffer(1 << 19)
    ring.write_samples((rng.standard_normal(1 << 18) + 1j * rng.standard_normal(1 << 18)).astype(np.complex64))
    for C, arms, fs, L, share in ANCHORS:
        codes = None if L == 1023 else np.where(rng.integers(0, 2, (C, L)) > 0, 1, -1).astype(np.int8)
        mgr = T.TrackingManager(fs, n_channels=C, n_arms=arms, codes=codes, nominal_code_rate=1.023e6, share_device=bool(share))
        n = int(round(fs / (1.023e6 / L)))
        for j in range(C):
            mgr.channels[j].start(dict(prn=(j + 1) if codes is not None else j % 31 + 1, code_phase_samples=0, code_phase_chips=0.0, carrier_freq=0.0,
                                       fs=fs, mag_relative=1.0, sample_global_index=0, doppler_bin=0))
            mgr.channels[j].set_state(code_rate=1.023e6, num_samples_per_code=n)
        mgr.update_all_dev(ring, 2)
        mgr.synchronize()
        print("anchor C=%d arms=%d fs=%g len=%d share=%d ran" % (C, arms, fs, L, share), flush=True)
        mgr.close()
    for arms in (3, 5):      # the eight keys: what the device says of each (GM_TRK_PLAN_PRINT)
        for mode in (T.CODE_INDEX_FAITHFUL, T.CODE_INDEX_FIXED):
            for boc in (False, True):
                T.TrackingManager(25e6, n_channels=32, n_arms=arms, code_index_mode=mode, boc11=boc).close()
    ring.close()


def _launches(path):
    rows = []
    for r in csv.DictReader(open(path)):
        if "trk_persistent_kernel" not in r["Kernel_Name"]:
            continue
        wg = int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
        grid = int(r.get("Grid_Size_X") or r["Grid_Size"]) // max(1, wg)
        rows.append((re.search(r"trk_persistent_kernel<[^>]*>", r["Kernel_Name"]).group(0), grid, wg, int(r.get("LDS_Block_Size") or r.get("LDS_Block_Size_v") or 0)))
    return rows


def listing(args):
    a, b = _launches(args.listing[0]), _launches(args.listing[1])
    lines = ["persistent launches of tools/trk_persist_plan_ab.py --layout (rocprofv3 --kernel-trace --stats), in launch order: one per anchor row",
             "kernel, workgroups x lanes per workgroup, LDS bytes as the trace reports them (the kernel's static share, rounded up; the",
             "dynamic share, the chip tables, is `lds` in the plan lines below: trk_persist_lds_bytes, moved as it was)",
             "%-4s %-66s | %-66s | %s" % ("row", "parent", "new", "same")]
    diff = abs(len(a) - len(b))
    for i in range(max(len(a), len(b))):
        x, y = (a[i] if i < len(a) else None), (b[i] if i < len(b) else None)
        diff += x != y and x is not None and y is not None
        fmt = lambda r: "%s %d x %d lds %d" % r if r else "-"
        who = "C=%d arms=%d fs=%g len=%d share=%d" % ANCHORS[i] if i < len(ANCHORS) else "?"
        lines.append("%-4d %-66s | %-66s | %s   (%s)" % (i, fmt(x), fmt(y), "yes" if x == y else "NO", who))
    lines.append("%d launches each, %d rows differ" % (len(b), diff) if len(a) == len(b) else "launch counts differ: %d / %d" % (len(a), len(b)))
    if args.plans:
        lines += ["", "gm_trk_create of the new library (GM_TRK_PLAN_PRINT): the anchor rows, then the eight keys at 32 channels x 25 Msps"]
        lines += [l.rstrip() for l in open(args.plans) if l.startswith("gm_trk plan:")]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return diff


def _stats(v):
    med = float(np.median(v))
    return dict(median=round(med, 6), min=round(min(v), 6), max=round(max(v), 6), spread=round((max(v) - min(v)) / med, 4))


def measure():
    import torch
    import bench
    from gnss_sdr_rs_amd import _lib, acquisition as A, synth, tracking as T
    _lib.init(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ca = A.ca_code_table()
    lines = {"tracking_32ch_ms_per_epoch": [], "tracking_32ch_strict_libm_us_per_epoch": [], "tracking_256ch_ms_per_epoch": [],
             "cfg5_ms_per_code_period": [], "cfg5_kernel_ms_per_code_period": []}
    for _ in range(REPS):
        t = bench.tracking_leg(torch, dev, st.cuda_stream, ca, T, synth, 1, None)
        lines["tracking_32ch_ms_per_epoch"].append(t["ms_per_epoch"])
        lines["tracking_32ch_strict_libm_us_per_epoch"].append(t["strict_libm"]["us_per_epoch"])
        lines["tracking_256ch_ms_per_epoch"].append(bench.tracking_leg(torch, dev, st.cuda_stream, ca, T, synth, 1, None, 0.0, C=256)["ms_per_epoch"])
        c5 = bench.cfg5_leg(torch, st.cuda_stream, T)
        lines["cfg5_ms_per_code_period"].append(c5["ms_per_code_period"])
        lines["cfg5_kernel_ms_per_code_period"].append(c5["kernel_ms_per_code_period"])
        print(json.dumps({k: v[-1] for k, v in lines.items()}), flush=True)
    return dict(tool="tools/trk_persist_plan_ab.py", library=os.path.basename(_lib._LIB_PATH), device=torch.cuda.get_device_name(0), repeats=REPS, lines=lines)


def ab(args):
    runs = [json.load(open(p)) for p in args.ab]
    libs = [runs[0]["library"], runs[1]["library"]]
    assert all(r["library"] == libs[i % 2] for i, r in enumerate(runs)) and libs[0] != libs[1], "runs alternate: parent, new, parent, new"
    rows, fails = [], 0
    for name in runs[0]["lines"]:
        pool = [sum((r["lines"][name] for r in runs[s::2]), []) for s in (0, 1)]
        par, new = _stats(pool[0]), _stats(pool[1])
        ok = new["median"] <= par["median"] * (1 + par["spread"])
        fails += not ok
        rows.append(dict(line=name, parent=dict(par, repeats=pool[0]), new=dict(new, repeats=pool[1]),
                         ratio_new_over_parent=round(new["median"] / par["median"], 4), margin=par["spread"], passed=bool(ok)))
        print("%-42s parent %.6f  new %.6f  ratio %.4f  margin %.4f  %s" % (name, par["median"], new["median"], rows[-1]["ratio_new_over_parent"],
                                                                          par["spread"], "ok" if ok else "BEYOND THE MARGIN"))
    meta = dict(tool=runs[0]["tool"], device=runs[0]["device"], parent_library=libs[0], new_library=libs[1], runs=len(runs),
                order="parent, new, parent, new, ... each a fresh process; a repeat is one call of the bench.py leg (its own median)",
                rule="pass: new median <= parent median * (1 + margin), margin = the parent's (max - min) / median over its pooled repeats")
    return dict(meta=meta, rows=rows), fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", action="store_true")
    ap.add_argument("--listing", nargs=2)
    ap.add_argument("--plans")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--ab", nargs="+")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.layout:
        layout()
        sys.exit(0)
    if args.listing:
        sys.exit(listing(args))
    res, fails = ab(args) if args.ab else (measure(), 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    sys.exit(fails)
