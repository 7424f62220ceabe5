"""Lag window x fine Doppler at known cells on the CPU: the two additive entries in every layer (this test fails without the feature),
the ABI number they leave alone, gm_acq_local_plan (host only, no device) against the numpy rules of acq_local_model.py with every
GM_ERR_INVALID_ARG case — its own lag rules and every rule it inherits from gm_acq_refine_plan — and the float64 model's fine code phase
against the simulated code start of the truth scenes.

The 0.25 sample of the truth test comes from a CPU run of exactly this estimator on these scenes with random 1023-chip codes, five code
starts (N - 5 among them) and three seeds: 0.03 to 0.12 sample at 60 dB-Hz, up to 0.17 at 45 dB-Hz; 0.25 is about twice the worst
60 dB-Hz value.  Without the blend term scene (b), whose code starts at N - 5, is 0.35 off: that scene is the test that the term is
there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import acq_local_model as LM
import acq_model as AM
import acq_refine_model as RM
from test_acq_refine_host import EVEN, INVALID_CASES as REFINE_INVALID, VALID as REFINE_VALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_local_search", "gm_acq_local_plan"]
INVALID = -1
FINE_BOUND = 0.25          # samples


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, acquisition as A
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
    assert "gm_acq_local_search" in hpp and "local_search(" in hpp
    assert "pub fn local_search" in _read("rust", "src", "mi355x", "do_acquisition.rs")
    build_py = _read("gnss-sdr-rs_amd", "build.py")
    assert "acq_local.hip" in build_py and "acq_load8.h" in build_py
    assert hasattr(A.AcquisitionEngine, "local_search") and hasattr(A, "local_plan")
    for words in ("gm_acq_cand", "gm_acq_local_cfg", "gm_acq_local_out", "88 bytes", "NO detection decision", "unobservable"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    # the ctypes structs have the header's layout: 16, 16 and 88 bytes, the doubles first
    assert C.sizeof(_lib.AcqCand) == 16 and C.sizeof(_lib.AcqLocalCfg) == 16 and C.sizeof(_lib.AcqLocalOut) == 88
    assert _lib.AcqLocalOut.carrier_hz.offset == 0 and _lib.AcqLocalOut.code_phase_fine.offset == 8
    assert _lib.AcqLocalOut.n_lags.offset == 80


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"
    assert C.sizeof(_lib.AcqRefineCfg) == 12 and C.sizeof(_lib.AcqRefineOut) == 56      # no existing struct changed


# (K, M, fs, N, table_freq, bin, lag_half_window, span_periods, n_freq, half_span_hz)
def _with_lag(case, L):
    return case[:6] + (L,) + case[6:]


# every valid case of gm_acq_refine_plan's table at L = 0, 3 and 64, and windows that just fit into the period
VALID = [_with_lag(c, L) for c in REFINE_VALID for L in (0, 3, 64)] + [
    (4, 3, 128.0e3, 128, EVEN, 1, 63, 0, 0, 0.0),               # 2 L + 1 = 127 <= N = 128
    (1, 2, 8.0e3, 8, [0.0], 0, 3, 0, 0, 0.0),                   # 2 L + 1 = 7 <= N = 8
]
# every invalid case of gm_acq_refine_plan's table stays invalid whatever the window is, and the lag rules of this entry's own
INVALID_CASES = [_with_lag(c, L) for c in REFINE_INVALID for L in (0, 64)] + [
    (4, 3, 2.048e6, 2048, EVEN, 1, 65, 0, 0, 0.0),              # L above 64
    (4, 3, 2.048e6, 2048, EVEN, 1, 1000, 0, 0, 0.0),
    (4, 3, 128.0e3, 128, EVEN, 1, 64, 0, 0, 0.0),               # L = 64 is in range, but 2 L + 1 = 129 > N = 128
    (1, 2, 8.0e3, 8, [0.0], 0, 4, 0, 0, 0.0),                   # 2 L + 1 = 9 > N = 8
    (4, 3, 2.048e6, 2048, EVEN, 1, 65, 0, 256, 0.0),            # both wrong
]
KEYS = ("n_lags", "span_periods", "n_groups", "n_freq")


@pytest.mark.parametrize("case", VALID)
def test_local_plan_follows_the_numpy_rules(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    K, M, fs, N, tf, b, L, span, Z, hs = case
    want = LM.plan(K, M, fs, N, tf, b, L, span, Z, hs)
    assert want is not None and want["n_lags"] == 2 * L + 1, case
    got = A.local_plan(K, M, fs, N, tf, b, L, span, Z, hs)
    assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}, (got, want)
    assert got["half_span_hz"] == pytest.approx(want["half_span_hz"], rel=1e-12) and got["step_hz"] == pytest.approx(want["step_hz"], rel=1e-12)
    # the same host code as gm_acq_refine_plan: its words
    ref = A.refine_plan(K, M, fs, N, tf, b, span, Z, hs)
    assert all(got[k] == ref[k] for k in ref), (got, ref)


@pytest.mark.parametrize("case", INVALID_CASES)
def test_local_plan_refuses(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    assert LM.plan(*case) is None, case
    with pytest.raises(GmError) as e:
        A.local_plan(*case)
    assert e.value.status == INVALID, case


def test_local_plan_takes_null_outputs_and_a_null_cfg(gm):
    tf = np.array(EVEN, np.float32)
    L = gm.lib()
    w, z = C.c_uint32(0), C.c_uint32(0)
    tfp = tf.ctypes.data_as(C.c_void_p)
    assert L.gm_acq_local_plan(4, 3, None, 2.048e6, 2048, 3, tfp, 1, C.byref(w), None, None, C.byref(z), None, None) == 0
    assert (w.value, z.value) == (1, 257)           # a null cfg: L = 0, the default grid
    assert L.gm_acq_local_plan(4, 3, None, 2.048e6, 2048, 3, None, 1, None, None, None, None, None, None) == INVALID


def test_a_null_handle_is_refused_without_a_device(gm):
    from gnss_sdr_rs_amd import _lib
    out, cand = _lib.AcqLocalOut(), _lib.AcqCand(0, 0, 0, 0)
    vp = lambda o: C.cast(C.byref(o), C.c_void_p)
    assert gm.lib().gm_acq_local_search(None, None, 0, vp(cand), 1, None, vp(out), None, None) == INVALID


# ---- the model against the simulated code start ---------------------------------------------------------------------------------
def _model_on_scene(oracle, c, centre_off, L=3, blend=True):
    N, fs, K, M = c["N"], c["fs"], c["K"], c["M"]
    tables = [oracle.DopplerShiftTable(c["f_if"], float(d), fs, N) for d in AM.DOP]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    d = 1
    p = LM.plan(K, M, fs, N, tf, d, L, c["span"])
    cp = (int(round(c["code_start_here"])) + centre_off) % N
    return LM.local(c["x"], tables[d].table, c["codes"][0], N, c["starts"][d], c["edge"], cp, L, tf[d], fs, p["span_periods"],
                    p["n_groups"], p["n_freq"], p["half_span_hz"], c["sec"], T_d=c["T"][d], code_rate=c["code_rate"], blend=blend)


def test_the_scene_builder_at_zero_is_the_refine_scene(oracle):
    for name in sorted(RM.TRUTH_SCENES):            # the builder's own signal code gives acq_refine_model's words at s0 = 0
        a, b = LM.truth_scene(oracle.ca_code_table(), name), RM.truth_scene(oracle.ca_code_table(), name)
        assert a["x"].dtype == b["x"].dtype and (a["x"] == b["x"]).all() and a["code_start_here"] == pytest.approx(b["code_start"])
    b = RM.truth_scene(oracle.ca_code_table(), "a")
    c = LM.truth_scene(oracle.ca_code_table(), "a", 0, seed_add=1)                     # another noise realisation
    assert c["x"].shape == b["x"].shape and not (c["x"] == b["x"]).all()
    later = LM.truth_scene(oracle.ca_code_table(), "a", LM.later_start(4))
    assert later["code_start_here"] == pytest.approx((12.3 - LM.later_start(4)) % RM.TRUTH_T)


@pytest.mark.parametrize("name", sorted(RM.TRUTH_SCENES))
@pytest.mark.parametrize("centre_off", [-1, 1])
def test_the_model_finds_the_simulated_code_start(oracle, name, centre_off):
    """60 dB-Hz, the window's centre one sample off the code start, L = 3: the model's code_phase_fine is within 0.25 sample of the
    simulated code start (measured on these scenes, real C/A row of PRN 5: printed below)."""
    assert RM.TRUTH_SCENES[name]["cn0"] == 60.0
    c = LM.truth_scene(oracle.ca_code_table(), name)
    r = _model_on_scene(oracle, c, centre_off)
    err = LM.circular_error(r["code_phase_fine"], c["code_start_here"], RM.TRUTH_T)
    plain = _model_on_scene(oracle, c, centre_off, blend=False)
    err_plain = LM.circular_error(plain["code_phase_fine"], c["code_start_here"], RM.TRUTH_T)
    print("scene %s, centre %+d: l* %d of 7, frac %+.3f, fine %.3f, code start %.3f, error %+.3f (without the blend term %+.3f), "
          "peak / floor %.1f over %d lags" % (name, centre_off, r["l"], r["frac"], r["code_phase_fine"], c["code_start_here"], err,
                                              err_plain, r["S"].max() / max(r["floor_power"], 1e-30), r["n_floor"]))
    assert r["lag_at_edge"] == 0 and r["freq_at_edge"] == 0, (name, r["l"], r["j"])
    assert abs(r["lam"] - c["code_start_here"]) <= 1.0 or abs(r["lam"] - c["code_start_here"]) >= c["N"] - 2, (name, r["lam"])
    assert abs(err) <= FINE_BOUND, (name, err)
    # the carrier is gm_acq_refine_doppler's: within its bound of the simulated one
    assert abs(r["carrier_hz"] - c["f_true"]) <= RM.truth_bound(c["K"] * c["M"]), name


@pytest.mark.parametrize("name", sorted(RM.TRUTH_SCENES))
def test_the_model_on_a_later_dwell(oracle, name):
    """a second dwell of the same signal, three secondary-row lengths on: expected code phase (code_start - s0) mod T, same bound"""
    s0 = LM.later_start(RM.TRUTH_SCENES[name]["K"])
    c = LM.truth_scene(oracle.ca_code_table(), name, s0, seed_add=100)
    r = _model_on_scene(oracle, c, 1)
    err = LM.circular_error(r["code_phase_fine"], c["code_start_here"], RM.TRUTH_T)
    print("scene %s from sample %d: fine %.3f, expected %.3f, error %+.3f" % (name, s0, r["code_phase_fine"], c["code_start_here"], err))
    assert r["lag_at_edge"] == 0 and abs(err) <= FINE_BOUND, (name, err)


def test_the_model_is_the_refine_model_at_every_lag(oracle):
    """row l of the model's surface is acq_refine_model.refine at code phase lambda_l; the floor's rows are the far ones"""
    c = LM.truth_scene(oracle.ca_code_table(), "b")
    r = _model_on_scene(oracle, c, 1, L=5)
    N, fs = c["N"], c["fs"]
    tables = [oracle.DopplerShiftTable(c["f_if"], float(d), fs, N) for d in AM.DOP]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    p = RM.plan(c["K"], c["M"], fs, N, tf, 1, c["span"])
    cp = (int(round(c["code_start_here"])) + 1) % N
    lam = LM.lags(cp, 5, N)
    assert lam.size == 11 and lam[5] == cp and (lam < N).all() and lam[0] > lam[-1]       # the window wraps: the code starts at N - 5
    for l in (0, 5, 10):
        want = RM.refine(c["x"], tables[1].table, c["codes"][0], N, c["starts"][1], c["edge"], int(lam[l]), tf[1], fs, p["span_periods"],
                         p["n_groups"], p["n_freq"], p["half_span_hz"], c["sec"])
        assert np.allclose(r["z"][l], want["z"], rtol=1e-12, atol=1e-9 * np.abs(want["z"]).max())
        assert np.allclose(r["S"][l], want["S"], rtol=1e-9)
    g = LM.guard_lags(fs, c["code_rate"])
    assert g == 4                                   # 2.0016 samples a chip: one chip and a sample
    far = [l for l in range(11) if abs(l - r["l"]) >= g]
    assert r["n_floor"] == len(far) and r["floor_power"] == pytest.approx(np.mean(r["S"][far]), rel=1e-12)
    assert r["S"].max() > 20.0 * r["floor_power"]
