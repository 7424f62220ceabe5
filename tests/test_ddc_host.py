"""Real-IF down-conversion on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number they
leave alone, gm_ddc_plan (host only, no device) with every refusal, the NCO's phasor words for all 2^24 phases, and the model of
ddc_model.py on a real tone (gain and image rejection) and on the scene that motivates the entry: the capture's format, int8 real at
16.3676 Msps with the carrier at 4.1304 MHz, down-converted by 20460/40919 and searched plainly at N = 8184."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import acq_model as AM
import ddc_model as DM
import resample_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_ddc_plan", "gm_ddc_create", "gm_ddc_destroy", "gm_ddc_reset", "gm_ddc_stats", "gm_ddc_synchronize", "gm_ddc_tables",
           "gm_ddc_process_dev", "gm_ddc_process", "gm_ddc_write_ring"]
INVALID = -1
MIX = DM.MIX


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, ddc
    import gnss_sdr_rs_amd
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
        assert name in hpp, name
    assert "class Ddc" in hpp
    assert "GmDdcCfg" in rust and "pub enum GmDdc" in rust
    assert "ddc_kernels.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_ddc" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert gnss_sdr_rs_amd.Ddc is ddc.Ddc
    for method in ("from_rates", "process", "process_dev", "reset", "tables", "stats", "synchronize", "write_ring"):
        assert hasattr(ddc.Ddc, method), method
    assert callable(ddc.plan)
    for words in ("gm_ddc_cfg", "Theta_n = (n * inc) mod 2^64", "Whi[k >> 12] * Wlo[k & 4095]", "j ASCENDING", "ANY byte address"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "Real-IF down-conversion" in _read("README.md") and "ddc_kernels.hip" in _read("README.md")
    assert "4.4c" in _read("DESIGN.md")
    stats = _read("profiles", "ddc_kernel_stats.txt")
    assert "ddc_kernel" in stats and "ddc_state_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: a double, then the resampler's eight 4-byte words
    assert C.sizeof(_lib.DdcCfg) == 40 and _lib.DdcCfg.up.offset == 8 and _lib.DdcCfg.reserved.offset == 36
    assert [f[0] for f in _lib.DdcCfg._fields_[1:]] == [f[0] for f in _lib.ResamplerCfg._fields_]
    body = re.search(r"pub struct GmDdcCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.DdcCfg._fields_]


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.ResamplerCfg) == 32 and C.sizeof(_lib.ExcisorCfg) == 32          # no existing struct changed


# ---- gm_ddc_plan -------------------------------------------------------------------------------------------------------------------
def _plan(mix, cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import ddc
    return ddc.plan(mix, cfg["up"], cfg["down"], so_far, n_in, **{k: v for k, v in cfg.items() if k not in ("up", "down")})


def test_plan_fills_in_the_defaults_and_the_phase_increment(gm):
    for up, down in ((1, 2), (20460, 40919)):
        got = _plan(MIX, dict(up=up, down=down))
        assert (got["up"], got["down"], got["taps"], got["n_phases"]) == (up, down, 64, 256)
    assert _plan(0.25, dict(up=1, down=2))["phase_inc"] == 1 << 62
    assert _plan(-0.25, dict(up=1, down=2))["phase_inc"] == 3 << 62
    assert _plan(0.0, dict(up=1, down=1))["phase_inc"] == 0 and _plan(7.0, dict(up=1, down=1))["phase_inc"] == 0
    assert _plan(3.5, dict(up=1, down=1))["phase_inc"] == 1 << 63
    # the definition in Python integers: the float64 fraction, scaled by 2^64 exactly
    from fractions import Fraction
    mix = 4130400 / 16367600
    want = int(Fraction(mix - math.floor(mix)) * (1 << 64))
    assert _plan(mix, dict(up=1, down=2))["phase_inc"] == want == DM.phase_inc(mix)
    assert abs(want / 2.0 ** 64 - 0.2523522080207239) < 1e-15
    for mix in (-0.37, 1e-9, 123456.789, -1e-30):
        assert _plan(mix, dict(up=1, down=1))["phase_inc"] == DM.phase_inc(mix), mix
    assert DM.phase_inc(-1e-30) == 0                                  # the fraction rounds to 1: the wrapped value


@pytest.mark.parametrize("cfg", [dict(up=1, down=1, taps=8), dict(up=1, down=2), dict(up=20460, down=40919), dict(up=3, down=8),
                                 dict(up=1, down=16, taps=256), dict(up=2, down=1)])
def test_plan_counts_what_the_resampler_plan_counts(gm, cfg):
    from gnss_sdr_rs_amd import resample
    rest = {k: v for k, v in cfg.items() if k not in ("up", "down")}
    p = RM.resolve(**cfg)
    half = p["T"] // 2
    for so_far in (0, half - 1, half, half + 1, (1 << 32) - 3, (1 << 40) + 12345):
        for n_in in (0, 1, half - 1, half, half + 1, p["T"] - 1, 4095, 4113, 40000):
            want = resample.plan(cfg["up"], cfg["down"], so_far, n_in, **rest)
            got = _plan(MIX, cfg, so_far, n_in)
            assert {k: got[k] for k in want} == want and want["n_out"] == RM.plan(p, so_far, n_in)


def test_plan_refuses(gm):
    from gnss_sdr_rs_amd import _lib
    import test_resample_host as TH
    L = gm.lib()
    for cfg in TH.REFUSED:                                           # the resampler's rules, field by field
        assert DM.resolve(MIX, **cfg) is None
        with pytest.raises(_lib.GmError) as e:
            _plan(MIX, cfg)
        assert e.value.status == INVALID, cfg
    for mix in (math.nan, math.inf, -math.inf):
        assert DM.resolve(mix, 1, 2) is None
        with pytest.raises(_lib.GmError) as e:
            _plan(mix, dict(up=1, down=2))
        assert e.value.status == INVALID, mix
    ok = _lib.DdcCfg(MIX, 1, 2, 0, 0, 0.0, 0.0, 0.0, 0)
    n = C.c_uint64(77)
    args = (None, None, None, None, None, C.byref(n))
    assert L.gm_ddc_plan(C.byref(_lib.DdcCfg(MIX, 1, 2, 0, 0, 0.0, 0.0, 0.0, 1)), 0, 10, *args) == INVALID
    assert L.gm_ddc_plan(None, 0, 10, *args) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert L.gm_ddc_plan(C.byref(ok), so_far, n_in, *args) == INVALID
    assert n.value == 77                                              # nothing written
    assert L.gm_ddc_plan(C.byref(ok), 0, 100, None, None, None, None, None, None) == 0
    assert L.gm_ddc_plan(C.byref(ok), 1 << 62, 0, *args) == 0 and n.value == 0
    # a null handle is refused without a device
    assert L.gm_ddc_process_dev(None, C.c_void_p(4096), 8, C.c_void_p(8192), 8, None, None) == INVALID
    assert L.gm_ddc_process(None, C.c_void_p(4096), 8, C.c_void_p(8192), 8, None) == INVALID
    assert L.gm_ddc_reset(None, 0) == INVALID and L.gm_ddc_stats(None, None, None, None) == INVALID
    assert L.gm_ddc_synchronize(None) == INVALID and L.gm_ddc_write_ring(None, None, None, None, None, 0, None) == INVALID
    table = np.zeros(8, np.float32)
    assert L.gm_ddc_tables(None, table.ctypes.data_as(C.c_void_p), None, None) == INVALID     # the filter table is a handle's
    assert L.gm_ddc_create(None, C.byref(C.c_void_p())) == INVALID and L.gm_ddc_create(C.byref(ok), None) == INVALID
    assert L.gm_ddc_destroy(None) == 0


# ---- the phasor words ----------------------------------------------------------------------------------------------------------------
def test_every_phasor_word_is_within_the_bound(gm):
    """All 2^24 values of k, from the library's own tables: |w - exp(-j 2 pi k / 2^24)| per component <= 2^-22.  Derived from five
    roundings of at most 2^-25 each (half a unit in the last place of a value <= 1): the rounding of the Whi word and of the Wlo word
    (each reaches a component through both of its products, with weights |cos| + |sin| <= sqrt 2: 2 sqrt 2 x 2^-25 together), the two
    products and the sum: at most (2 sqrt 2 + 3) 2^-25 = 5.83 x 2^-25, and 2^-22 = 8 x 2^-25 leaves room for the second-order terms.
    Measured: 2.26 x 2^-24."""
    from gnss_sdr_rs_amd import ddc
    whi, wlo = ddc.phasor_tables()
    mine = DM.phasor_tables()
    assert whi.dtype == np.complex64 and whi.shape == wlo.shape == (4096,)
    # the library's tables are the definition's words: the float64 value rounded once (two libms may differ in the last float64 bit,
    # which moves a float32 word only on a rounding tie: allow one unit in the last place, on no more than a handful of words)
    for got, want in ((whi, mine[0]), (wlo, mine[1])):
        diff = np.abs(got.view(np.float32).view(np.int32).astype(np.int64) - want.view(np.float32).view(np.int32).astype(np.int64))
        assert diff.max() <= 1 and int((diff != 0).sum()) <= 8
    assert whi[0] == 1 and wlo[0] == 1 and whi[1024].imag == -1.0
    worst = 0.0
    for k0 in range(0, 1 << 24, 1 << 20):
        k = np.arange(k0, k0 + (1 << 20), dtype=np.uint32)
        re, im = DM.phasor_of_k(k, whi, wlo)
        ang = 2.0 * np.pi * k.astype(np.float64) / 16777216.0
        worst = max(worst, float(np.abs(re.astype(np.float64) - np.cos(ang)).max()), float(np.abs(im.astype(np.float64) + np.sin(ang)).max()))
    print("largest phasor error %.3f x 2^-24" % (worst * 2.0 ** 24))
    assert worst <= 2.0 ** -22


def test_the_phase_is_a_wrapping_64_bit_product():
    """numpy's uint64 product against Python integers, at indices where a 32-bit or a float product goes wrong"""
    inc = DM.phase_inc(MIX)
    for first in (0, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5):
        k = DM.phase_words(DM.indices(first, 7), inc)
        assert [int(v) for v in k] == [((first + i) * inc % (1 << 64)) >> 40 for i in range(7)]


# ---- a real tone in the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(1, 2), (20460, 40919)])
def test_a_real_tone_comes_out_at_half_its_amplitude_without_its_image(gm, ratio):
    """Amplitude 100, not quantised, at f_mix + 37 kHz; fs_in = 16.3676 MHz, f_mix = 4.1304 MHz, defaults.  The baseband tone's
    amplitude is 50 within 1e-4 relative, and the strongest other line (the image, aliased to about -113.5 kHz) is below -85 dB
    relative to it under a Blackman window over 8000 outputs.  Measured here: 1/2: 50.00016, -93.2 dB; 20460/40919: 50.00015,
    -91.7 dB."""
    from gnss_sdr_rs_amd import ddc, resample
    up, down = ratio
    p = DM.resolve(MIX, up, down)
    g = resample.design(up, down)
    whi, wlo = ddc.phasor_tables()
    amp, other = DM.tone_measure(p, g, whi, wlo)
    print("%d/%d: amplitude %.5f, strongest other line %.1f dB" % (up, down, amp, other))
    assert abs(amp - 50.0) <= 1e-4 * 50.0
    assert other < -85.0


def test_the_model_does_not_care_how_the_stream_is_cut():
    p = DM.resolve(MIX, 3, 8, blank_threshold=100.0)
    g = RM.table(p)
    whi, wlo = DM.phasor_tables()
    rng = np.random.default_rng(2)
    x = rng.integers(-128, 128, 3000).astype(np.int8)
    y, w, m = DM.run(p, g, whi, wlo, x)
    assert m.blanked == int((np.abs(x.astype(np.int64)) > 100).sum()) > 100
    assert (m.inputs, m.outputs) == (3000, y.size) and y.size == RM.total_out(p, 3000)
    for blocks in (1, 7, p["T"] - 1, 1000):
        y2, w2, m2 = DM.run(p, g, whi, wlo, x, blocks=blocks)
        assert (y2 == y).all() and (w2 == w).all() and (m2.blanked, m2.outputs) == (m.blanked, m.outputs)


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
_SCENES = {}
SCENE_SEED = 3


def scene_run(cn0, seed=SCENE_SEED):
    """The scene at one level through the model and a plain K = 1, M = 10 model search at N = 8184: computed once, shared
    (tests/test_gpu_ddc.py takes 50 dB-Hz) and left unchanged.  -> dict of x (int8 real), y (the down-converted dwell, complex64),
    chips, p and `ddc` = (bin, arg-max, peak-to-mean) of the best cell."""
    key = (cn0, seed)
    if key in _SCENES:
        return _SCENES[key]
    chips = DM.scene_chips()
    codes = AM.sample_codes(chips, 1023.0 * DM.FS_OUT / DM.N, DM.FS_OUT, DM.N)
    tabs, tf = DM.scene_tables()
    p = DM.resolve(MIX, DM.UP, DM.DOWN)
    whi, wlo = DM.phasor_tables()
    x = DM.scene(cn0, seed)
    y, _, _ = DM.run(p, RM.table(p).astype(np.float32), whi, wlo, x, blocks=20000)
    y = y[:DM.M * DM.N].astype(np.complex64)
    assert y.size == DM.M * DM.N
    found = DM.best_cell(*AM.search_model(y, tabs, codes, DM.N, 1, DM.M, tf, DM.FS_OUT))
    _SCENES[key] = dict(x=x, y=y, chips=chips, p=p, ddc=found)
    return _SCENES[key]


def test_a_plain_search_of_the_down_converted_capture_finds_the_satellite():
    """Random 1023-chip code, true period 16367.6 samples, code start 3000.3, Doppler +1 kHz, 45 dB-Hz, int8 real at sigma 30, 12
    periods, seed 3; 20460/40919 at the defaults; K = 1, M = 10 at N = 8184 over -2000 .. 2000 Hz in 500 Hz steps.  The best cell is
    the +1 kHz bin with the code phase within 1 of 3000.3 * 20460 / 40919 = 1500.19.  The carrier's amplitude is
    sigma sqrt(4 C/N0 / fs): a real stream's noise fills fs / 2.  Measured: arg-max 1501, peak-to-mean 32.3."""
    r = scene_run(45.0)
    print("45 dB-Hz, seed %d: (bin, arg-max, peak-to-mean) = %s" % (SCENE_SEED, r["ddc"]))
    assert DM.T_TRUE * DM.UP / DM.DOWN == DM.N and abs(DM.EXPECTED_PHASE - 1500.19) < 0.01
    assert DM.DOP[DM.TRUE_BIN] == 1000.0
    assert r["ddc"][0] == DM.TRUE_BIN
    assert abs(r["ddc"][1] - DM.EXPECTED_PHASE) <= 1
