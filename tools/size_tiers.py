"""README's table of transform sizes: which stage-C kernel serves each size the acquisition handle accepts, how many scratch_*
instructions that kernel carries (tools/so_kernel_stats.py, no GPU), and — with a GPU — its measured time at one common geometry
(32 codes x 9 bins x 2 integrations, complex int8 samples resident), as ns per transform-sample = t_corr / (P D M N).  The sizes come
from gm_acq_plan_info: every in-LDS and composite size, and a few any_length sizes (the long path, acq_long.hip: its stage C is
C1 + C2 per slab + C3; the per-sample figure is per code-period sample N, not per transform sample L for the padded form).
    python tools/size_tiers.py --measure out.json      (GPU box)      python tools/size_tiers.py --table out.json   (here: markdown)"""
import json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LONG = [50000, 200000, 61440, 38400, 262136]        # any_length sizes: native 5 x 10000, 20 x 10000, 15 x 4096; padded 38400, 262136


def _plans():
    """(N, any_length, plan) for every size the handle serves in the in-LDS and composite forms, plus the LONG sample sizes — read from
    gm_acq_plan_info (the rule gm_acq_create applies), not restated here"""
    from gnss_sdr_rs_amd import acquisition as A
    out = []
    for n in range(8, (1 << 18) + 1, 8):
        st, info = A.plan_info(n, False)
        if st == 0:
            out.append((n, False, info))
    for n in LONG:
        st, info = A.plan_info(n, True)
        if st == 0:
            out.append((n, True, info))
    return out


P, D, M = (int(v) for v in os.environ.get("TIERS_PDM", "32,9,2").split(","))     # TIERS_PDM=32,41,4 TIERS_ONLY=6000,18000: an A/B at another grid


def measure(path):
    import numpy as np, torch
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _lib.init(0)
    rng = np.random.default_rng(1)
    out = {}
    only = [int(v) for v in os.environ.get("TIERS_ONLY", "").split(",") if v]
    for N, any_length, info in _plans():
        q, base = info["q"], info["base"]
        if only and N not in only:
            continue
        fs = N * 1000.0
        dop = (np.arange(D, dtype=np.float32) - D // 2) * 250.0
        x = rng.integers(-60, 60, 2 * M * N, dtype=np.int8)
        try:
            eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, n_integrations=M, any_length=any_length)
        except Exception as e:
            out[str(N)] = {"error": repr(e)}
            continue
        d_x = torch.from_numpy(x).cuda()
        d_met = torch.zeros(3 * P * D, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream(); torch.cuda.set_stream(st)
        eng.set_stream(st.cuda_stream)
        for _ in range(3):
            eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr())
        torch.cuda.synchronize()
        eng.enable_timing(True)
        for _ in range(10):
            eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr())
        torch.cuda.synchronize()
        ts = eng.timing_summary()
        out[str(N)] = {"q": q, "base": base, "form": info["form"], "transform_len": info["transform_len"], "corr_ms": ts["avg_corr_ms"], "mix_fft_ms": ts["avg_mix_fft_ms"],
                       "ns_per_transform_sample": ts["avg_corr_ms"] * 1e6 / (P * D * M * N)}
        eng.close()
        print(N, out[str(N)], flush=True)
    json.dump(out, open(path, "w"), indent=1)


def table(path):
    from so_kernel_stats import kernel_stats, short
    st = kernel_stats(os.path.join(ROOT, "gnss-sdr-rs_amd", "lib", "libgnss_mi355x.so"))
    meas = json.load(open(path)) if path and os.path.exists(path) else {}
    by = {}
    for r in st.values():
        n = short(r["demangled"])
        m = re.match(r"void (long_corr_inv_kernel)<Plan<(\d+)[^>]*> ?>()$", n) or re.match(r"void (acq_corr_kernel|acq_corr_ws31_kernel|comp_corr_kernel|comp_corr_ws_kernel)<(?:Hybrid)?(?:Plan|CorrPlan\w*)?<?(\d+)[^>]*>+,? ?(.*)>$", n)
        if not m:
            continue
        kern, base, rest = m.group(1), int(m.group(2)), m.group(3)
        flags = [f.strip() for f in rest.split(",")] if rest else []
        if kern == "acq_corr_kernel" and flags[-2:] != ["false", "false"]:
            continue                                   # the reference_products variant
        if kern == "acq_corr_ws31_kernel" and flags[-1:] != ["false"]:
            continue
        if kern == "comp_corr_kernel" and (len(flags) > 1 and flags[1] == "true"):
            continue                                   # the strict_sum_order (planes) variant
        if kern == "comp_corr_ws_kernel" and flags[-1] == "true":
            continue
        if kern == "long_corr_inv_kernel":             # one kernel per base, Q at run time
            by[("long", base)] = (kern, r["scratch_insts"], r["vgpr"], r["lds_bytes"])
            continue
        q = int(flags[0].rstrip("u")) if kern.startswith("comp") else 1
        by[(q, base)] = (kern, r["scratch_insts"], r["vgpr"], r["lds_bytes"])
    rows = []
    for N, _, info in _plans():
        q, base, form = info["q"], info["base"], info["form"]
        if form.startswith("long"):
            k = by.get(("long", base))
            label = "%d x %d%s" % (q, base, " = %d, padded" % info["transform_len"] if form == "long_padded" else ", long")
        else:
            k = by.get((q, base))
            label = ("%d x %d" % (q, base)) if q > 1 else "in LDS"
        if not k and q == 1 and base == 16368:
            k = next((v for (qq, bb), v in by.items() if v[0] == "acq_corr_ws31_kernel"), None)
        me = meas.get(str(N), {})
        rows.append((N, label, k, me))
    print("| N | form | stage-C kernel | scratch_* instructions | VGPRs | LDS | stage C, ms (32 x 9 x 2) | ns per transform-sample |")
    print("|---|---|---|---|---|---|---|---|")
    for N, form, k, me in rows:
        kn, sc, vg, lds = k if k else ("?", "?", "?", "?")
        print("| %d | %s | `%s` | %s | %s | %s | %s | %s |" % (N, form, kn, sc, vg, lds, ("%.3f" % me["corr_ms"]) if "corr_ms" in me else "—",
                                                       ("%.3f" % me["ns_per_transform_sample"]) if "corr_ms" in me else "—"))


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure(sys.argv[sys.argv.index("--measure") + 1])
    else:
        table(sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else None)
