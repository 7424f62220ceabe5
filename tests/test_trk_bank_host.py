"""The correlator bank at tracked states on the CPU: the additive entries in every layer (this test fails without the feature), the
ABI number they leave alone, gm_trk_bank_plan (host only, no device) against trk_bank_model.py with every refusal, and the model
itself against things that can be derived: the C/A code's triangle, the sinc of a carrier offset over one millisecond, and the
lopsided correlation function a second path leaves."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import trk_bank_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_trk_bank_plan", "gm_trk_bank", "gm_trk_bank_samples"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, tracking
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    L = gm.lib()
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    with open(_lib.library_path(), "rb") as f:
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
    assert hasattr(tracking.TrackingManager, "bank") and hasattr(tracking.TrackingChannel, "bank") and callable(tracking.bank_plan)
    assert "pub fn bank(" in _read("rust", "src", "mi355x", "do_tracking.rs")
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_trk_bank" in internal and "TrkBankArgs" in internal
    kernel = _read("gnss-sdr-rs_amd", "csrc", "trk_bank.hip")
    assert "trk_bank_kernel" in kernel and "trk_bank_sum_kernel" in kernel
    # the definition, word for word where it is a formula
    for words in ("f_f      = fl(carrier_freq + df_f)",
                  "phase_i  = carrier_phase + fl(fl(fl(2 pi) * f_f) * i) / fs",
                  "y_f[i]   = x[i] * (cos phase_i, -sin phase_i)",
                  "c[i]     = (code_phase + i * (code_rate / fs)) mod code_len",
                  "out[r][f][t] = sum_{i < n} y_f[i] * chip(fl(c[i] + tau_t))",
                  "strict_sum_order is IGNORED", "NOTHING IS ADVANCED", "a function of n alone", "SKIPPED"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "Correlator bank at tracked states" in _read("README.md")
    stats = _read("profiles", "trk_bank_kernel_stats.txt")
    assert "trk_bank_kernel" in stats and "trk_persistent_kernel" in stats and "trk_correlate_kernel" in stats
    # the struct layouts, in every layer
    assert C.sizeof(_lib.TrkBankCfg) == 40 and _lib.TrkBankCfg.taps_chips.offset == 8 and _lib.TrkBankCfg.reserved.offset == 24
    assert C.sizeof(_lib.TrkBankPlanOut) == 32 and _lib.TrkBankPlanOut.slices.offset == 24
    for cname, rname, cls in (("gm_trk_bank_cfg", "GmTrkBankCfg", _lib.TrkBankCfg), ("gm_trk_bank_plan_out", "GmTrkBankPlanOut", _lib.TrkBankPlanOut)):
        body = re.search(r"pub struct %s\s*\{([^}]*)\}" % rname, rust, re.S).group(1)
        assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in cls._fields_], rname
        cstruct = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, header, re.S).group(1)
        names = []
        for decl in re.sub(r"/\*.*?\*/", "", cstruct, flags=re.S).split(";"):
            names += [re.sub(r"\[\d+\]", "", w).strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if w.strip()]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert re.search(r"pub\s+reserved\s*:\s*\[u32;\s*4\]", rust)


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.TrkState) == 64 and C.sizeof(_lib.TrkOut) == 40                # no existing struct changed


# ---- gm_trk_bank_plan ----------------------------------------------------------------------------------------------------------------
PLANS = [dict(fs=2.048e6, taps=[0.0]), dict(fs=25.0e6, taps=[-0.5, 0.0, 0.5], n_states=32),
         dict(fs=25.0e6, taps=np.linspace(-2, 2, 64), n_states=1024), dict(fs=5.0e6, taps=np.linspace(-1, 1, 32), offsets_hz=np.linspace(-700, 700, 8)),
         dict(fs=9.0e6, taps=np.linspace(-64, 64, 17), offsets_hz=[0.0, 4.5e6, -4.5e6]),
         dict(fs=4.092e6, taps=[-1.25, 0.75], code_rate=1.023e6, code_len=4092), dict(fs=2.048e6, taps=[0.0], code_rate=1.0235e6),
         dict(fs=2.048e6, taps=[3.0], code_rate=1.0225e6), dict(fs=50.0e6, taps=[0.0], code_len=16384, code_rate=1.023e6)]


@pytest.mark.parametrize("kw", PLANS)
def test_plan_against_the_model(gm, kw):
    from gnss_sdr_rs_amd import tracking
    want = M.plan(**{k: v for k, v in kw.items()}, **({} if "code_len" in kw else dict(code_len=1023)))
    assert isinstance(want, dict), want
    assert tracking.bank_plan(**kw) == want


def test_plan_examples(gm):
    from gnss_sdr_rs_amd import tracking
    p = tracking.bank_plan(25.0e6, np.zeros(17), np.zeros(3), n_states=40)
    assert p == dict(n_taps=17, n_offsets=3, out_words=40 * 3 * 17, samples=25000, slices=7, tap_groups=2)
    assert tracking.bank_plan(2.048e6, [0.0], None)["n_offsets"] == 1                 # no offsets: the single offset 0
    assert tracking.bank_plan(2.048e6, [0.0], code_rate=1.0235e6)["samples"] == 2047
    assert tracking.bank_plan(2.048e6, [0.0], code_rate=1.0225e6)["samples"] == 2049


def test_the_slice_count_depends_on_n_alone(gm):
    from gnss_sdr_rs_amd import tracking
    for fs, n in ((2.048e6, 2048), (4.096e6, 4096), (4.097e6, 4097), (5.0e6, 5000), (8.192e6, 8192), (9.0e6, 9000), (25.0e6, 25000)):
        want = (n + 4095) // 4096
        assert M.slices(n) == want
        for taps, offs, r in (([0.0], None, 1), (np.zeros(64), None, 1024), (np.zeros(32), np.zeros(8), 40)):
            p = tracking.bank_plan(fs, taps, offs, n_states=r)
            assert (p["samples"], p["slices"]) == (n, want), (fs, p)
    assert M.slices(0) == 0 and M.slices(1 << 31) == 0 and M.slices((1 << 31) - 1) == 1 << 19


REFUSED = [
    (dict(taps=np.zeros(0)), M.OUT_OF_RANGE), (dict(taps=np.zeros(65)), M.OUT_OF_RANGE),
    (dict(taps=[0.0], offsets_hz=np.zeros(9)), M.OUT_OF_RANGE), (dict(taps=np.zeros(64), offsets_hz=np.zeros(5)), M.OUT_OF_RANGE),
    (dict(taps=np.zeros(33), offsets_hz=np.zeros(8)), M.OUT_OF_RANGE),
    (dict(taps=[0.0], n_states=0), M.OUT_OF_RANGE), (dict(taps=[0.0], n_states=1025), M.OUT_OF_RANGE),
    (dict(taps=[0.0, 64.5]), M.OUT_OF_RANGE), (dict(taps=[-65.0]), M.OUT_OF_RANGE),
    (dict(taps=[50.0], code_len=100), M.OUT_OF_RANGE), (dict(taps=[-50.0], code_len=100), M.OUT_OF_RANGE),
    (dict(taps=[0.0, math.nan]), M.INVALID_ARG), (dict(taps=[math.inf]), M.INVALID_ARG), (dict(taps=[-math.inf, 0.0]), M.INVALID_ARG),
    (dict(taps=[0.0], offsets_hz=[math.nan]), M.INVALID_ARG), (dict(taps=[0.0], offsets_hz=[0.0, math.inf]), M.INVALID_ARG),
    (dict(taps=[0.0], offsets_hz=[1.0241e6]), M.OUT_OF_RANGE), (dict(taps=[0.0], offsets_hz=[-1.0241e6]), M.OUT_OF_RANGE),
    (dict(taps=[0.0], code_len=16385), M.OUT_OF_RANGE),
]


@pytest.mark.parametrize("kw,status", REFUSED)
def test_plan_refuses(gm, kw, status):
    from gnss_sdr_rs_amd import _lib, tracking
    assert M.plan(2.048e6, kw["taps"], kw.get("offsets_hz"), kw.get("n_states", 1), code_len=kw.get("code_len", 1023)) == status, kw
    with pytest.raises(_lib.GmError) as e:
        tracking.bank_plan(2.048e6, **kw)
    assert e.value.status == status, kw


def test_plan_takes_the_limits_themselves(gm):
    from gnss_sdr_rs_amd import tracking
    tracking.bank_plan(2.048e6, [64.0, -64.0], [1.024e6, -1.024e6], n_states=1024)
    tracking.bank_plan(2.048e6, np.zeros(32), np.zeros(8))
    tracking.bank_plan(2.048e6, [49.5], code_len=100)


def test_plan_refuses_null_pointers_and_leaves_the_output(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    trk = _lib.TrkCfg()
    trk.fs, trk.n_channels = 2.048e6, 1
    taps = np.zeros(3, np.float32)
    offs = np.zeros(2, np.float32)
    cfg = _lib.TrkBankCfg()
    cfg.n_taps, cfg.taps_chips = 3, taps.ctypes.data
    out = _lib.TrkBankPlanOut()
    out.samples = 77
    assert L.gm_trk_bank_plan(None, C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG
    assert L.gm_trk_bank_plan(C.byref(trk), None, 1, C.byref(out)) == M.INVALID_ARG
    cfg.taps_chips = None
    assert L.gm_trk_bank_plan(C.byref(trk), C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG
    cfg.taps_chips, cfg.n_offsets, cfg.offsets_hz = taps.ctypes.data, 2, None
    assert L.gm_trk_bank_plan(C.byref(trk), C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG
    trk.fs = 0.0
    cfg.n_offsets = 0
    assert L.gm_trk_bank_plan(C.byref(trk), C.byref(cfg), 1, C.byref(out)) == M.INVALID_ARG
    assert out.samples == 77                                       # a refusal leaves the output untouched
    trk.fs = 2.048e6
    cfg.n_offsets, cfg.offsets_hz = 2, offs.ctypes.data
    assert L.gm_trk_bank_plan(C.byref(trk), C.byref(cfg), 1, None) == 0          # the output may be NULL
    assert L.gm_trk_bank_plan(C.byref(trk), C.byref(cfg), 5, C.byref(out)) == 0 and out.out_words == 30 and out.samples == 2048
    # the device entries refuse a null handle before they touch a device
    assert L.gm_trk_bank(None, None, None, 1, C.byref(cfg), None, None) == M.INVALID_ARG
    assert L.gm_trk_bank_samples(None, None, None, 0, C.byref(cfg), None) == M.INVALID_ARG


# ---- the model against things that can be derived ------------------------------------------------------------------------------------
# Noise-free scene: one C/A code at fs = 4.092 MHz (exactly four samples a chip, n = 4092), code phase 0, the Doppler on the NCO,
# FIXED indexing.  Checked in the model before the constants were fixed: PRN 7 is the one of the three whose autocorrelation has
# side values next to the peak (0.030 and 0.046 at +-1.25 and +-1.5 chips), PRN 1 and 20 have -1/1023 there.
FS, N, FD, AMP = 4.092e6, 4092, 1250.0, 100.0
TAPS = np.arange(-6, 7) * 0.25


@pytest.fixture(scope="module", params=[1, 7, 20])
def scene(request, oracle):
    row = oracle.ca_code_table()[request.param - 1]
    i = np.arange(N)
    c = np.fmod(i.astype(np.float32) * (np.float32(1.023e6) / np.float32(FS)), np.float32(1023))
    carrier = np.exp(2j * np.pi * FD * i / FS)
    x = (AMP * row[np.floor(c).astype(np.int64)] * carrier).astype(np.complex64)
    # a second path half a chip ahead in tap coordinates (its peak sits at tau = +0.5), 6 dB down, in phase
    x2 = (x + 0.5 * AMP * row[M.chip_index((c + np.float32(0.5)).astype(np.float32), 1023, M.FIXED)] * carrier).astype(np.complex64)
    return dict(row=row, x=x, x2=x2)


def _bank(sc, x, taps, offs=(0.0,)):
    return M.bank(x, N, FS, sc["row"], FD, 0.0, 0.0, 1.023e6, taps, offs, mode=M.FIXED)


def test_model_the_triangle(scene):
    assert M.samples_per_code(FS, 1.023e6, 1023) == N
    out = np.abs(_bank(scene, scene["x"], TAPS)[0])
    r = out / out[6]
    assert abs(out[6] - AMP * N) <= 1e-4 * AMP * N
    tri = np.maximum(1.0 - np.abs(TAPS), 0.0)
    inside = np.abs(TAPS) <= 1.0
    assert np.all(np.abs(r - tri)[inside] <= 1.0 / 4.0)             # within 1 / (samples per chip) of 1 - |tau|
    assert np.all(r[~inside] < 0.05)                               # C/A side values are <= 65/1023, and these taps see a part of them
    assert np.argmax(r) == 6 and np.all(np.diff(r[2:7]) > 0.2) and np.all(np.diff(r[6:11]) < -0.2)      # the flanks, a quarter a tap


def test_model_the_sinc_of_a_carrier_offset(scene):
    offs = [0.0, 500.0, -500.0, 1000.0, -1000.0]
    out = np.abs(_bank(scene, scene["x"], [0.0], offs)[:, 0])
    want = np.abs(np.sinc(np.array(offs) * 1e-3))                  # 1, 0.6366, 0.6366, 0, 0
    assert abs(want[1] - 0.6366) < 1e-4 and want[3] < 1e-12
    assert np.all(np.abs(out / out[0] - want) <= 0.01)


def test_model_a_second_path_leans_the_function(scene):
    one = np.abs(_bank(scene, scene["x"], [-0.5, 0.0, 0.5])[0])
    two = np.abs(_bank(scene, scene["x2"], [-0.5, 0.0, 0.5])[0])
    assert abs(one[2] - one[0]) <= 0.01 * one[1]
    assert two[2] - two[0] > 0.2 * two[1]


def test_model_chip_index_modes():
    p = np.array([-1.5, -0.25, 0.0, 0.75, 1022.5, 1023.0, 1024.25], np.float32)
    assert list(M.chip_index(p, 1023, M.FAITHFUL)) == [0, 0, 0, 0, 1022, 0, 1]          # a negative phase saturates to chip 0
    assert list(M.chip_index(p, 1023, M.FIXED)) == [1021, 1022, 0, 0, 1022, 0, 1]       # FIXED wraps
