"""Rate conversion and pulse blanking on the CPU: the additive entries in every layer (this test fails without the feature), the ABI
number they leave alone, gm_resampler_plan and gm_resampler_design (host only, no device) against the float64 model of
resample_model.py with every refusal, the model filter's quality, and the scene that motivates the entry: a code period of 2047.6
samples that a plain search smears and a search of the dwell resampled by 5120/5119 does not."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import acq_model as AM
import resample_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_resampler_plan", "gm_resampler_design", "gm_resampler_create", "gm_resampler_destroy", "gm_resampler_reset",
           "gm_resampler_taps", "gm_resampler_stats", "gm_resampler_process_dev", "gm_resampler_process", "gm_resampler_synchronize",
           "gm_frontend_write_ring_resampled"]
INVALID = -1
RATIOS = [(1, 1), (3, 2), (2, 3), (4, 25), (5120, 5119), (40920, 40919)]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, frontend, resample
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
        assert name in hpp or name in ("gm_resampler_plan", "gm_resampler_design"), name
    assert "class Resampler" in hpp and "Resampler& resampler" in hpp
    assert "GmResamplerCfg" in rust and "pub enum GmResampler" in rust
    assert "resample_kernels.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_resample" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert gnss_sdr_rs_amd.Resampler is resample.Resampler
    for method in ("from_rates", "process", "process_dev", "reset", "taps", "stats"):
        assert hasattr(resample.Resampler, method), method
    assert callable(resample.plan) and callable(resample.design)
    assert "resampler" in frontend.DigitalFrontend.write_ring.__code__.co_varnames
    for words in ("gm_resampler_cfg", "total_out(A) = max(0, ceil((A - T/2) * up / down))", "input time m * down / up",
                  "fs_out is stored only, as in the reference", "j ASCENDING", "two buffers used alternately"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "Rate conversion and pulse blanking" in _read("README.md") and "resample_kernels.hip" in _read("README.md")
    assert "4.4a" in _read("DESIGN.md")
    stats = _read("profiles", "resample_kernel_stats.txt")
    assert "resample_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: eight 4-byte words
    assert C.sizeof(_lib.ResamplerCfg) == 32 and _lib.ResamplerCfg.blank_threshold.offset == 24 and _lib.ResamplerCfg.reserved.offset == 28
    body = re.search(r"pub struct GmResamplerCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.ResamplerCfg._fields_]


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"
    assert C.sizeof(_lib.AcqLocalOut) == 88 and C.sizeof(_lib.AcqCand) == 16 and C.sizeof(_lib.AcqCancelCand) == 32   # no existing struct changed


# ---- gm_resampler_plan -------------------------------------------------------------------------------------------------------------
def _lib_plan(gm, cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import resample
    return resample.plan(cfg["up"], cfg["down"], so_far, n_in, **{k: v for k, v in cfg.items() if k not in ("up", "down")})


def test_plan_reduces_the_ratio_and_fills_in_the_defaults(gm):
    for up, down, taps in ((1, 1, 32), (3, 2, 32), (2, 3, 64), (4, 25, 224), (25, 4, 32), (5120, 5119, 32), (40920, 40919, 32),
                           (1, 16, 256), (16, 1, 32), (8, 50, 224), (48000, 44100, 32), (1 << 24, 1 << 24, 32), (1 << 20, 1 << 24, 256)):
        got = _lib_plan(gm, dict(up=up, down=down))
        p = RM.resolve(up, down)
        g = math.gcd(up, down)
        assert (got["up"], got["down"], got["taps"], got["n_phases"]) == (up // g, down // g, taps, 256) == (p["up"], p["down"], p["T"], p["PHI"])
    got = _lib_plan(gm, dict(up=6, down=4, taps=8, n_phases=16, cutoff=1.0, kaiser_beta=20.0, blank_threshold=3.5))
    assert (got["up"], got["down"], got["taps"], got["n_phases"]) == (3, 2, 8, 16)
    assert RM.resolve(1, 1)["cutoff"] == 0.9 and RM.resolve(1, 1)["beta"] == 8.0
    # the defaults are what a zero means: the same table words (0.9 is no float32, so the cutoff is left at its zero)
    from gnss_sdr_rs_amd import resample
    assert (resample.design(2, 3) == resample.design(4, 6, taps=64, n_phases=256, kaiser_beta=8.0)).all()


@pytest.mark.parametrize("ratio", RATIOS)
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, ratio):
    up, down = ratio
    cfg = dict(up=up, down=down)
    p = RM.resolve(up, down)
    half = p["T"] // 2
    rng = np.random.default_rng(up * 7 + down)
    for so_far in (0, half - 1, half, half + 1, (1 << 32) - 3, (1 << 40) + 12345):
        for n_in in (0, 1, half - 1, half, half + 1, p["T"] - 1, 1000, 20011):
            want = RM.plan(p, so_far, n_in)
            assert _lib_plan(gm, cfg, so_far, n_in)["n_out"] == want
            assert want == RM.total_out(p, so_far + n_in) - RM.total_out(p, so_far)
            cuts = np.sort(rng.integers(0, n_in + 1, 6))
            parts = np.diff(np.concatenate([[0], cuts, [n_in]]))
            done, total = so_far, 0
            for part in parts:
                total += _lib_plan(gm, cfg, done, int(part))["n_out"]
                done += int(part)
            assert total == want, (so_far, n_in, parts)
    # the count is the number of outputs whose last tap exists: i0(m) + T/2 <= A - 1 exactly for m < total_out(A)
    for A in (half + 1, half + 2, 1000, (1 << 32) + 5):
        n = RM.total_out(p, A)
        i0 = lambda m: m * down // up
        assert n >= 1 and i0(n - 1) + half <= A - 1 < i0(n) + half


REFUSED = [dict(up=0, down=1), dict(up=1, down=0), dict(up=(1 << 24) + 1, down=1 << 24), dict(up=1 << 24, down=(1 << 24) + 1),
           dict(up=17, down=1), dict(up=1, down=17), dict(up=3, down=50),
           dict(up=1, down=1, taps=4), dict(up=1, down=1, taps=12), dict(up=1, down=1, taps=264),
           dict(up=1, down=1, n_phases=8), dict(up=1, down=1, n_phases=48), dict(up=1, down=1, n_phases=2048),
           dict(up=1, down=1, cutoff=-0.1), dict(up=1, down=1, cutoff=1.01), dict(up=1, down=1, cutoff=math.nan),
           dict(up=1, down=1, kaiser_beta=-1.0), dict(up=1, down=1, kaiser_beta=20.5), dict(up=1, down=1, kaiser_beta=math.nan),
           dict(up=1, down=1, blank_threshold=-1.0), dict(up=1, down=1, blank_threshold=math.nan)]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_and_design_refuse(gm, cfg):
    from gnss_sdr_rs_amd import _lib, resample
    assert RM.resolve(**cfg) is None, cfg
    for call in (lambda: _lib_plan(gm, cfg), lambda: resample.design(**cfg)):
        with pytest.raises(_lib.GmError) as e:
            call()
        assert e.value.status == INVALID, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    ok = _lib.ResamplerCfg(3, 2, 0, 0, 0.0, 0.0, 0.0, 0)
    n = C.c_uint64(77)
    assert L.gm_resampler_plan(C.byref(_lib.ResamplerCfg(3, 2, 0, 0, 0.0, 0.0, 0.0, 1)), 0, 10, None, None, None, None, C.byref(n)) == INVALID
    assert L.gm_resampler_plan(None, 0, 10, None, None, None, None, C.byref(n)) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert RM.plan(RM.resolve(3, 2), so_far, n_in) is None
        assert L.gm_resampler_plan(C.byref(ok), so_far, n_in, None, None, None, None, C.byref(n)) == INVALID
    assert n.value == 77                                                                      # nothing written
    assert L.gm_resampler_plan(C.byref(ok), 0, 100, None, None, None, None, None) == 0
    assert L.gm_resampler_plan(C.byref(ok), 1 << 62, 0, None, None, None, None, C.byref(n)) == 0 and n.value == 0
    assert L.gm_resampler_design(C.byref(ok), None) == INVALID
    # a null handle is refused without a device
    assert L.gm_resampler_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(8192), 8, None, None) == INVALID
    assert L.gm_resampler_reset(None, 0) == INVALID and L.gm_resampler_stats(None, None, None, None) == INVALID
    assert L.gm_resampler_taps(None, None) == INVALID and L.gm_resampler_synchronize(None) == INVALID
    assert L.gm_frontend_write_ring_resampled(None, None, None, None, 0, 0, None) == INVALID
    assert L.gm_resampler_destroy(None) == 0


# ---- gm_resampler_design -----------------------------------------------------------------------------------------------------------
DESIGNS = [dict(up=1, down=1), dict(up=3, down=2, taps=8, n_phases=16), dict(up=2, down=3), dict(up=4, down=25),
           dict(up=5120, down=5119, taps=32), dict(up=40920, down=40919, taps=256, n_phases=1024),
           dict(up=1, down=16, cutoff=1.0, kaiser_beta=20.0), dict(up=16, down=1, taps=16, cutoff=0.5, kaiser_beta=0.5)]


@pytest.mark.parametrize("cfg", DESIGNS)
def test_design_gives_the_models_table(gm, cfg):
    """every word within 2^-23 of the model's float64 value: all |g| <= 1, and two correct float64 evaluations rounded to float32
    differ by at most one ulp there; every row sums to 1 within T 2^-24 (T roundings of half an ulp of words below 1)"""
    from gnss_sdr_rs_amd import resample
    p = RM.resolve(**cfg)
    want = RM.table(p)
    got = resample.design(**cfg)
    assert got.shape == want.shape == (p["PHI"] + 1, p["T"]) and got.dtype == np.float32
    assert np.abs(want).max() <= 1.0
    err = np.abs(got.astype(np.float64) - want).max()
    rows = np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max()
    print("%s: largest word error %.3g, largest row-sum error %.3g" % (cfg, err, rows))
    assert err <= 2.0 ** -23
    assert rows <= p["T"] * 2.0 ** -24


# ---- the model filter's quality ----------------------------------------------------------------------------------------------------
def test_the_decimating_filter_passes_and_stops():
    """4/25 at the default 224 taps: within 0.1 dB up to half the output Nyquist band, at or below -60 dB from 1.2 x the output
    Nyquist frequency on.  Frequencies in cycles per input sample; the output Nyquist frequency is 0.08.  Measured: pass band within
    0.0006 dB; -90.8, -100.3, -112.5, -109.6, -124.4 dB at 0.096, 0.12, 0.2, 0.35, 0.5."""
    p = RM.resolve(4, 25)
    assert p["T"] == 224
    g = RM.table(p).astype(np.float32)
    for f in (0.0, 0.01, 0.02, 0.03, 0.04):
        db = RM.tone_gain_db(p, g, f)
        print("pass %.3f: %+.4f dB" % (f, db))
        assert abs(db) <= 0.1, (f, db)
    for f in (0.096, 0.12, 0.2, 0.35, 0.5):
        db = RM.tone_gain_db(p, g, f)
        print("stop %.3f: %+.1f dB" % (f, db))
        assert db <= -60.0, (f, db)


def test_the_near_unity_filter_is_flat():
    """5120/5119 at 32 taps: within 0.1 dB at half Nyquist, within 0.5 dB at 0.8 Nyquist (measured -0.0001 and -0.28 dB)"""
    p = RM.resolve(5120, 5119, taps=32)
    g = RM.table(p).astype(np.float32)
    half, most = RM.tone_gain_db(p, g, 0.25), RM.tone_gain_db(p, g, 0.4)
    print("0.25: %+.4f dB, 0.4: %+.3f dB" % (half, most))
    assert abs(half) <= 0.1 and abs(most) <= 0.5


def test_blending_256_phases_is_as_good_as_evaluating_the_filter():
    """PHI = 256 linear blending of neighbouring rows against coefficients evaluated at every output's exact position, on noise:
    relative rms error at or below 1e-5 (measured 4.8e-6)"""
    p = RM.resolve(5120, 5119, taps=32)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(6000) + 1j * rng.standard_normal(6000)
    yb, _, _ = RM.run(p, RM.table(p), x)
    ye, _, _ = RM.run(p, RM.table(p), x, exact=True)
    rel = float(np.sqrt(np.mean(np.abs(yb - ye) ** 2) / np.mean(np.abs(ye) ** 2)))
    print("relative rms error %.3g" % rel)
    assert yb.size == ye.size > 5900 and rel <= 1e-5


def test_the_model_does_not_care_how_the_stream_is_cut():
    p = RM.resolve(2, 3, blank_threshold=2.0)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(3000) + 1j * rng.standard_normal(3000)
    y, w, m = RM.run(p, RM.table(p), x)
    assert m.blanked > 100 and (m.inputs, m.outputs) == (3000, y.size) and y.size == RM.total_out(p, 3000)
    for blocks in (1, 7, p["T"] - 1, 1000):
        y2, w2, m2 = RM.run(p, RM.table(p), x, blocks=blocks)
        assert (y2 == y).all() and (w2 == w).all() and (m2.blanked, m2.outputs) == (m.blanked, m.outputs)
    # absolute indices: a stream that starts at input_index is the stream with that many zeros in front
    k = 100 * p["down"] + 1
    y3, _, _ = RM.run(p, RM.table(p), x, input_index=k)
    y4, _, _ = RM.run(p, RM.table(p), np.concatenate([np.zeros(k), x]))
    assert y4.size > y3.size and np.abs(y4[-y3.size:] - y3).max() == 0.0 and np.abs(y4[:-y3.size]).max() == 0.0


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
_SCENES = {}
SCENE_SEED = 12


def scene_run(cn0, seed=SCENE_SEED):
    """The scene at one level through the three model searches: computed once, shared (tests/test_gpu_resample.py takes 50 dB-Hz) and
    left unchanged.  -> dict of x, y (the resampled dwell, complex64) and (bin, arg-max, peak-to-mean) of worker 0's best cell for
    plain (the original, period p from p N), drift (the original, AM.drift_starts of the true period) and resampled."""
    key = (cn0, seed)
    if key in _SCENES:
        return _SCENES[key]
    chips = RM.scene_codes()
    codes = RM.sampled_codes(chips)
    tabs, tf = RM.scene_tables()
    p = RM.resolve(RM.UP, RM.DOWN)
    x = RM.scene(cn0, seed)
    search = lambda s, **kw: RM.best_cell(*AM.search_model(s, tabs, codes, RM.N, 1, RM.PERIODS, tf, RM.FS, **kw), RM.SAT["worker"])
    y, _, _ = RM.run(p, RM.table(p).astype(np.float32), x)
    y = y[:RM.PERIODS * RM.N].astype(np.complex64)
    assert y.size == RM.PERIODS * RM.N
    _SCENES[key] = dict(x=x, y=y, chips=chips, p=p, plain=search(x), resampled=search(y),
                        drift=search(x, starts=AM.drift_starts(np.full(AM.D, RM.T_TRUE), RM.PERIODS)))
    return _SCENES[key]


@pytest.mark.parametrize("cn0", [40.0, 37.0])
def test_a_plain_search_of_the_resampled_dwell_matches_the_drift_search(cn0):
    """N = 2048, true period N - 0.4, K = 1, M = 40, 5120/5119 at the defaults, seed 12.  Peak-to-mean of the true worker's best cell,
    measured: at 40 dB-Hz plain 2.19 (arg-max 686), drift starts 7.75 (700), resampled 7.54 (700): ratio 0.97; at 37 dB-Hz 1.95
    (wrong bin), 4.41 (700), 4.30 (700): ratio 0.97.  (Seeds 11 and 13: ratios 0.94 and 1.01 at 40, 0.98 and 1.03 at 37 dB-Hz.)"""
    r = scene_run(cn0)
    print("%.0f dB-Hz: plain %s, drift starts %s, resampled %s" % (cn0, r["plain"], r["drift"], r["resampled"]))
    assert RM.T_TRUE * RM.UP / RM.DOWN == RM.N
    assert abs(r["resampled"][1] - RM.EXPECTED_PHASE) <= 1 and r["resampled"][0] == 1
    assert abs(r["drift"][1] - RM.EXPECTED_PHASE) <= 1
    assert r["resampled"][2] >= 0.8 * r["drift"][2]
    assert r["plain"][2] < r["drift"][2] and r["plain"][2] < r["resampled"][2]
