"""Per-antenna prompts at tracked states on the CPU: the additive entries in every layer (this test fails without the feature), the ABI
number they leave alone, gm_trk_array_plan (host only, no device) against trk_array_model.py with every refusal, the model at L = 1
against trk_bank_model's bank on the de-interleaved antenna, and the scenes that motivate the entry: beam_model.scene's two satellites
behind rows solved from TRACKER-FORM prompts, against the same scenes behind the acquisition-form rows of array_probe_model.py.

The L = 1 bar.  trk_bank_model.bank rounds x * w in f32 before the chip — two products and a difference per component, three roundings of
2^-24 relative each on terms of size at most |x| (the difference's on the result) — and this model multiplies in float64, so the two
differ by at most about 3 x 2^-24 = 1.8e-7 of the envelope sum_i |x_a[s + i]|; the test holds them to trk_bank_model's REL = 1e-5 of it
and prints what it measures.

The scenes' bar.  For every seed and satellite the peak-to-mean behind the tracker-form row is at least 0.9 times the one behind the
acquisition-form row of the same scene (array_probe_model.cells(..)[(w, "est")]): 0.9 is the margin test_array_probe_host.BARS gives an
estimated row, and the yardstick is the merged method, not the code under test.  The committed model's table (python
tests/trk_array_model.py; seeds 1 / 2 / 3) is in README.md, "Per-antenna prompts at tracked states"."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import array_probe_model as PM
import beam_model as BM
import trk_array_model as M
import trk_bank_model as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_trk_array_plan", "gm_trk_array_prompts"]
REL = 1e-5
QUALITY_BAR = 0.9


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- layers -----------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_in_every_layer(gm):
    import gnss_sdr_rs_amd
    from gnss_sdr_rs_amd import _lib, tracking
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    L = gm.lib()
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    with open(_lib.library_path(), "rb") as f:      # the dynamic symbols of the built library, read from its file
        blob = f.read()
    hpp = _read("gnss-sdr-rs_amd", "host", "gnss_sdr.hpp")
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "pub fn %s(" % name in rust, name
        assert re.fullmatch(pattern.replace("*", ".*"), name), (pattern, name)
        assert getattr(L, name) is not None
        assert name.encode() + b"\0" in blob, name
        assert name + "(" in hpp, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in _read(doc), (doc, name)
    assert hasattr(tracking.TrackingManager, "array_prompts") and callable(tracking.array_plan)
    assert gnss_sdr_rs_amd.TrackingManager is tracking.TrackingManager and gnss_sdr_rs_amd.trk_array_plan is tracking.array_plan
    assert "array_prompts(" in hpp and "array_plan(" in hpp
    assert "pub fn array_prompts(" in _read("rust", "src", "mi355x", "do_tracking.rs")
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_trk_array" in internal and "TrkArrayArgs" in internal
    kernel = _read("gnss-sdr-rs_amd", "csrc", "trk_array.hip")
    assert "trk_array_kernel" in kernel and "trk_array_sum_kernel" in kernel
    assert '#include "trk_array.hip"' in _read("gnss-sdr-rs_amd", "csrc", "trk_kernels.hip")
    assert "trk_array.hip" in _read("gnss-sdr-rs_amd", "build.py")
    # the definition, word for word where it is a formula
    for words in ("phase_i = carrier_phase + fl(fl(fl(2 pi) * carrier_freq) * i) / fs",
                  "c[i]    = (code_phase + i * (code_rate / fs)) mod code_len",
                  "ref[i]  = (cos phase_i, -sin phase_i) * chip(fl(c[i] + tau))",
                  "z[r][l][a] = sum_{i < n} x_a[s + i - l] * ref[i]",
                  "re = fma(xr, rr, re);  re = fma(-xi, ri, re);  im = fma(xr, ri, im);  im = fma(xi, rr, im)",
                  "strict_sum_order is IGNORED", "a function of n and L alone", "NOT bit for bit", "NOTHING IS ADVANCED",
                  "A time index below 0 reads as ZERO", "SKIPPED", "HAS FINISHED WRITING d_samples"):
        assert words in header, words
    assert "Per-antenna prompts at tracked states" in _read("README.md") and "4.3b" in _read("DESIGN.md")
    stats = _read("profiles", "trk_array_kernel_stats.txt")
    assert "trk_array_kernel" in stats and "trk_bank_kernel" in stats and "trk_persistent_kernel" in stats and "scratch" in stats
    # the struct layouts, in every layer
    assert C.sizeof(_lib.TrkArrayCfg) == 32 and _lib.TrkArrayCfg.tap_chips.offset == 8 and _lib.TrkArrayCfg.reserved.offset == 12
    P = _lib.TrkArrayPlanOut
    assert C.sizeof(P) == 32 and (P.out_words.offset, P.samples.offset, P.slices.offset) == (8, 16, 24)
    for cname, rname, cls in (("gm_trk_array_cfg", "GmTrkArrayCfg", _lib.TrkArrayCfg), ("gm_trk_array_plan_out", "GmTrkArrayPlanOut", P)):
        body = re.search(r"pub struct %s\s*\{([^}]*)\}" % rname, rust, re.S).group(1)
        assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in cls._fields_], rname
        cstruct = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, header, re.S).group(1)
        names = []
        for decl in re.sub(r"/\*.*?\*/", "", cstruct, flags=re.S).split(";"):
            names += [re.sub(r"\[\d+\]", "", w).strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if w.strip()]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert re.search(r"pub\s+reserved\s*:\s*\[u32;\s*5\]", rust)


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.TrkState) == 64 and C.sizeof(_lib.TrkOut) == 40 and C.sizeof(_lib.TrkBankCfg) == 40      # no existing struct changed


# ---- 1. gm_trk_array_plan ---------------------------------------------------------------------------------------------------------------
def test_plan_holds_every_rule(gm):
    """every (A, L) in 0 .. 10 squared, the record counts at and beyond their limits, through the C entry and the Python wrapper"""
    from gnss_sdr_rs_amd import _lib, tracking
    fs, pairs = 25.0e6, 0
    for A in range(0, 11):
        for L in range(0, 11):
            for n_states in (0, 1, 32, 1024, 1025):
                want = M.plan(fs, A, L, 0.0, n_states)
                if isinstance(want, dict):
                    assert tracking.array_plan(fs, A, L, n_states=n_states) == want, (A, L, n_states)
                    assert want["samples"] == 25000 and want["slices"] == 7 and want["words_per_record"] == A * L
                    pairs += n_states == 1
                else:
                    with pytest.raises(_lib.GmError) as e:
                        tracking.array_plan(fs, A, L, n_states=n_states)
                    assert e.value.status == want == M.OUT_OF_RANGE, (A, L, n_states)
    assert pairs == 43                                       # gm_stap's (A, L) pairs, all of them
    assert tracking.array_plan(2.048e6, 4) == dict(words_per_record=4, out_words=4, samples=2048, slices=1)      # taps defaults to 1


PLANS = [dict(fs=2.048e6, n_antennas=2), dict(fs=25.0e6, n_antennas=4, taps=4, n_states=32), dict(fs=25.0e6, n_antennas=8, taps=4, n_states=1024),
         dict(fs=4.097e6, n_antennas=4, taps=8, tap_chips=-2.25), dict(fs=9.0e6, n_antennas=3, taps=2, tap_chips=64.0),
         dict(fs=4.092e6, n_antennas=5, taps=6, tap_chips=0.5, code_rate=1.023e6, code_len=4092),
         dict(fs=2.048e6, n_antennas=4, code_rate=1.0235e6), dict(fs=2.048e6, n_antennas=4, code_rate=1.0225e6),
         dict(fs=50.0e6, n_antennas=4, code_len=16384, code_rate=1.023e6), dict(fs=2.048e6, n_antennas=4, tap_chips=49.5, code_len=100)]


@pytest.mark.parametrize("kw", PLANS)
def test_plan_against_the_model(gm, kw):
    from gnss_sdr_rs_amd import tracking
    m = dict(kw, taps=kw.get("taps", 1))
    want = M.plan(**m, **({} if "code_len" in kw else dict(code_len=1023)))
    assert isinstance(want, dict), want
    assert tracking.array_plan(**kw) == want


def test_the_slice_count_depends_on_n_alone(gm):
    from gnss_sdr_rs_amd import tracking
    for fs, n in ((2.048e6, 2048), (4.096e6, 4096), (4.097e6, 4097), (5.0e6, 5000), (8.192e6, 8192), (9.0e6, 9000), (25.0e6, 25000)):
        want = (n + 4095) // 4096
        assert M.slices(n) == want
        for A, L, r in ((2, 1, 1), (4, 8, 1024), (8, 4, 40)):
            p = tracking.array_plan(fs, A, L, n_states=r)
            assert (p["samples"], p["slices"]) == (n, want), (fs, p)
    assert M.slices(0) == 0 and M.slices(1 << 31) == 0 and M.slices((1 << 31) - 1) == 1 << 19


REFUSED = [
    (dict(n_antennas=4, tap_chips=64.5), M.OUT_OF_RANGE), (dict(n_antennas=4, tap_chips=-65.0), M.OUT_OF_RANGE),
    (dict(n_antennas=4, tap_chips=50.0, code_len=100), M.OUT_OF_RANGE), (dict(n_antennas=4, tap_chips=-50.0, code_len=100), M.OUT_OF_RANGE),
    (dict(n_antennas=4, tap_chips=math.nan), M.INVALID_ARG), (dict(n_antennas=4, tap_chips=math.inf), M.INVALID_ARG),
    (dict(n_antennas=4, tap_chips=-math.inf), M.INVALID_ARG), (dict(n_antennas=4, code_len=16385), M.OUT_OF_RANGE),
    (dict(n_antennas=1), M.OUT_OF_RANGE), (dict(n_antennas=9), M.OUT_OF_RANGE), (dict(n_antennas=4, taps=0), M.OUT_OF_RANGE),
    (dict(n_antennas=4, taps=9), M.OUT_OF_RANGE), (dict(n_antennas=5, taps=7), M.OUT_OF_RANGE), (dict(n_antennas=8, taps=5), M.OUT_OF_RANGE),
    (dict(n_antennas=4, n_states=0), M.OUT_OF_RANGE), (dict(n_antennas=4, n_states=1025), M.OUT_OF_RANGE),
]


@pytest.mark.parametrize("kw,status", REFUSED)
def test_plan_refuses(gm, kw, status):
    from gnss_sdr_rs_amd import _lib, tracking
    assert M.plan(2.048e6, kw["n_antennas"], kw.get("taps", 1), kw.get("tap_chips", 0.0), kw.get("n_states", 1),
                  code_len=kw.get("code_len", 1023)) == status, kw
    with pytest.raises(_lib.GmError) as e:
        tracking.array_plan(2.048e6, **kw)
    assert e.value.status == status, kw


def test_plan_refuses_nulls_and_reserved_words_and_leaves_the_output(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    trk = _lib.TrkCfg()
    trk.fs, trk.n_channels = 2.048e6, 1
    cfg = _lib.TrkArrayCfg()
    cfg.n_antennas, cfg.taps = 4, 2
    out = _lib.TrkArrayPlanOut()
    out.samples = 77
    assert L.gm_trk_array_plan(None, C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG
    assert L.gm_trk_array_plan(C.byref(trk), None, 1, C.byref(out)) == M.INVALID_ARG
    for k in range(5):
        cfg.reserved[k] = 1
        assert L.gm_trk_array_plan(C.byref(trk), C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG, k
        assert M.plan(2.048e6, 4, 2, reserved=[int(j == k) for j in range(5)]) == M.INVALID_ARG
        cfg.reserved[k] = 0
    trk.fs = 0.0
    assert L.gm_trk_array_plan(C.byref(trk), C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG and M.plan(0.0, 4, 2) == M.INVALID_ARG
    assert out.samples == 77                                       # a refusal leaves the output untouched
    trk.fs = 2.048e6
    assert L.gm_trk_array_plan(C.byref(trk), C.byref(cfg), 1, None) == 0          # the output may be NULL
    assert L.gm_trk_array_plan(C.byref(trk), C.byref(cfg), 5, C.byref(out)) == 0
    assert (out.words_per_record, out.out_words, out.samples, out.slices) == (8, 40, 2048, 1)
    # the device entry refuses a null handle before it touches a device
    assert L.gm_trk_array_prompts(None, None, 0, 0, 0, None, 1, C.byref(cfg), None, None) == M.INVALID_ARG


def test_the_skip_rules_of_the_model():
    n, L = 2048, 4
    ok = dict(active=1, row=3, n_codes=32, n=n, s=5000, L=L, first_index=0, n_time=20000)
    assert M.runs(**ok)
    for change in (dict(active=0), dict(row=-1), dict(row=32), dict(n=0), dict(n=1 << 31), dict(s=20000 - n + 1),
                   dict(first_index=4998), dict(first_index=5001), dict(first_index=1, s=2)):
        assert not M.runs(**dict(ok, **change)), change
    for change in (dict(s=20000 - n), dict(first_index=4997), dict(s=0), dict(s=2), dict(first_index=4997, n_time=5000 + n - 4997)):
        assert M.runs(**dict(ok, **change)), change


# ---- 2. L = 1 against the bank model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,boc,tau", [(M.FIXED, False, 0.0), (M.FAITHFUL, False, -2.25), (M.FIXED, True, 0.5)])
def test_tap_zero_is_the_bank_models_word_per_antenna(mode, boc, tau):
    fs, n, A = 2.048e6, 2048, 3
    rng = np.random.default_rng(17)
    row = np.where(rng.integers(0, 2, 1023) > 0, 1, -1).astype(np.int8)
    x = (8.0 * (rng.standard_normal((3 * n, A)) + 1j * rng.standard_normal((3 * n, A)))).astype(np.complex64)
    worst = 0.0
    for s, f, ph, cp, rate in ((0, 1830.0, 0.3, 0.0, 1.023e6), (777, -2500.0, -1.1, 511.25, 1.023e6), (n + 5, 40.0, 2.9, 1022.9, 1.0231e6)):
        m = TB.samples_per_code(fs, rate, 1023)
        z, env = M.prompts(x.astype(np.complex128), m, s, 1, M.reference(m, fs, row, f, ph, cp, rate, tau, mode, boc))
        for a in range(A):
            want = TB.bank(x[s:, a], m, fs, row, f, ph, cp, rate, [tau], [0.0], mode, boc)[0, 0]
            worst = max(worst, abs(z[0, a] - want) / env[0, a])
    print("mode %d, boc %s, tau %g: largest |z - bank model| / envelope %.2e (expected about 1.8e-7 at most, bar %.0e)" % (mode, boc, tau, worst, REL))
    assert worst <= REL


def test_the_models_halo_is_zero_and_its_taps_are_delays():
    fs, n, A, L = 2.048e6, 2048, 2, 4
    rng = np.random.default_rng(4)
    row = np.where(rng.integers(0, 2, 1023) > 0, 1, -1).astype(np.int8)
    x = (rng.standard_normal((2 * n, A)) + 1j * rng.standard_normal((2 * n, A)))
    ref = M.reference(n, fs, row, 500.0, 0.2, 10.5, 1.023e6)
    for s in (0, 2, 100):
        z, env = M.prompts(x, n, s, L, ref)
        for l in range(L):
            shifted = np.concatenate([np.zeros((l, A)), x])[:x.shape[0]]           # x_a[t - l], zero in front of the stream
            want, _ = M.prompts(shifted, n, s, 1, ref)
            assert np.abs(z[l] - want[0]).max() <= 1e-12 * env.max(), (s, l)
    # a buffer that begins at s - (L-1) with that first_index gives the same words
    z0, _ = M.prompts(x, n, 100, L, ref)
    z1, _ = M.prompts(x[97:], n, 100, L, ref, first_index=97)
    assert (z0 == z1).all()


# ---- 3. quality on the scenes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", PM.CONFIGS, ids=["%s-L%d" % c for c in PM.CONFIGS])
def test_every_tracker_form_row_finds_its_satellite(name, L):
    for seed in PM.SEEDS:
        acq = PM.cells(name, seed, L)
        trk = M.cells(name, seed, L)
        for w in (0, 1):
            a, t, q = acq[(w, "est")], trk[(w, "trk")], trk[(w, "quality")]
            print("%s L = %d seed %d sat %d: acquisition-form row %.1f, tracker-form row %.1f at (%d, %d) (%.3f of it, bar %.1f), "
                  "lambda1 / lambda2 %.1f" % (name, L, seed, w, a[2], t[2], t[0], t[1], t[2] / a[2], QUALITY_BAR, q))
            assert BM.found(t, w), (seed, w, t)                       # the best cell is the true one
            assert t[2] >= QUALITY_BAR * a[2], (seed, w, t[2] / a[2])
            assert q >= 2.0, (seed, w, q)


def test_the_scene_records_are_the_issues():
    for w in (0, 1):
        recs = M.scene_records(w)
        assert len(recs) == 9 and [r[0] for r in recs] == [BM.SATS[w]["code_phase"] + p * BM.N for p in range(9)]
        assert all(r[1] == BM.SATS[w]["doppler"] and r[3] == 0.0 for r in recs)
        assert recs[-1][0] + BM.N <= BM.DWELL
