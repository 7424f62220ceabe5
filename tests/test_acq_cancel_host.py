"""Subtracting found satellites from a dwell on the CPU: the two additive entries in every layer (this test fails without the feature),
the ABI number they leave alone, gm_acq_cancel_plan (host only, no device) against the bounds of the float64 model of
acq_cancel_model.py with every refusal, the model's self-checks, and the scene that motivates the entry: a 66 dB-Hz satellite whose
cross-correlation peaks hide a 42 dB-Hz one until it is subtracted.

The scene test runs the model and acq_model.search_model on seeds 100 .. 105 of acq_cancel_model.scene (the defaults: PRN 5 at
66 dB-Hz, code start 700.3, +130 Hz; PRN 6 at 42 dB-Hz, code start 1200.7, -170 Hz; int8 IQ; no rescan of seeds, levels or code starts
was needed).  Measured with this generator: before, the weak worker's best cell is at the true code phase in 0 of 6 seeds (arg-max
1644, 1644, 1644, 915, 46, 650); after, in 6 of 6 (1201 every time, peak-to-mean 7.6 to 9.7).  The strong worker's best peak-to-mean
falls from 347 .. 384 to 15.7, 5.2, 16.8, 9.0, 14.5, 8.0; STRONG_AFTER_BOUND = 34 is twice the largest of the six.  The candidates are
what acq_local_model.local returns for the strong cell (L = 3, span_periods = 4): carrier 2 to 8.4 Hz and code phase 0.05 to 0.1 sample
from the simulated values."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import acq_cancel_model as CM
import acq_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_cancel", "gm_acq_cancel_plan"]
INVALID = -1
SEEDS = tuple(range(100, 106))
STRONG_AFTER_BOUND = 34.0          # peak-to-mean of the strong worker's best cell after the subtraction: twice the largest measured
N = CM.N


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
    assert "gm_acq_cancel" in hpp and "cancel(" in hpp
    assert "pub fn cancel" in _read("rust", "src", "mi355x", "do_acquisition.rs")
    assert "GmAcqCancelCand" in rust and "GmAcqCancelOut" in rust
    assert "acq_cancel.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_cancel" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert hasattr(A.AcquisitionEngine, "cancel") and hasattr(A.AcquisitionEngine, "cancel_cands_from_local") and hasattr(A, "cancel_plan")
    for words in ("gm_acq_cancel_cand", "gm_acq_cancel_out", "32 bytes", "NO detection decision", "PARALLEL cancellation", "in place"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "Cancelling found satellites" in _read("README.md") and "4.2g" in _read("DESIGN.md")
    # the ctypes structs have the header's layout: 32 and 32 bytes
    assert C.sizeof(_lib.AcqCancelCand) == 32 and C.sizeof(_lib.AcqCancelOut) == 32
    assert _lib.AcqCancelCand.carrier_hz.offset == 8 and _lib.AcqCancelCand.period_samples.offset == 24
    assert _lib.AcqCancelOut.removed_energy.offset == 0 and _lib.AcqCancelOut.amp_rms.offset == 8


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"
    assert C.sizeof(_lib.AcqLocalOut) == 88 and C.sizeof(_lib.AcqCand) == 16              # no existing struct changed


# (dwell_samples, fft_size, code_phase, period_samples)
D_DRIFT = 24572                    # the scene's dwell: floor(11 (N - 0.4) + 0.5) + N, no multiple of 8
PLAN_CASES = [
    (D_DRIFT, N, 0.0, N - 0.4),                     # q0 = 0: no leading partial segment
    (D_DRIFT, N, 2.5, N - 0.4),                     # a 3-sample first segment
    (D_DRIFT, N, N - 0.25, N - 0.4),
    (D_DRIFT, N, 2047.8, 2047.6),                   # cp >= T: q0 = -2
    (12 * N, N, 700.3, 0.0),                        # T = 0: N
    (D_DRIFT, N, 700.3, N - 8.0),
    (D_DRIFT, N, 700.3, N + 7.9),
    (12 * (N - 8), N, 0.0, N - 8.0),                # D a multiple of T
    (12 * (N - 8), N, 0.5, N - 8.0),
    (12 * (N - 8) + 1, N, 0.5, N - 8.0),            # the last segment starts inside the dwell's last sample: empty
    (N, N, 100.0, 0.0),                             # D = N
    (N, N, 0.0, 0.0),
]
REFUSED = [
    (D_DRIFT, N, -0.5, 0.0), (D_DRIFT, N, float(N), 0.0), (D_DRIFT, N, N + 3.0, 0.0), (D_DRIFT, N, math.nan, 0.0),   # cp
    (D_DRIFT, N, 1.0, N - 8.1), (D_DRIFT, N, 1.0, N + 8.1), (D_DRIFT, N, 1.0, 1.0), (D_DRIFT, N, 1.0, -float(N)),    # |T - N| > 8
    (D_DRIFT, N, 1.0, math.nan), (D_DRIFT, N, 1.0, math.inf),
    (0, N, 1.0, 0.0),
]


@pytest.mark.parametrize("case", PLAN_CASES)
def test_cancel_plan_gives_the_models_bounds(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    D, n, cp, T = case
    want = CM.plan(D, n, cp, T)
    assert want is not None, case
    got = A.cancel_plan(D, n, cp, T)
    assert got["n_segments"] == want["n_segments"] and got["bounds"].dtype == np.uint64, (got, want)
    assert (got["bounds"].astype(np.int64) == want["bounds"]).all(), (got, want)
    b = want["bounds"]
    assert b[0] == 0 and b[-1] == D and (np.diff(b) >= 0).all() and (np.diff(b)[1:-1] > 0).all() and np.diff(b).max() <= n + 9


def test_the_plan_cases_are_what_they_say():
    first = lambda c: int(np.diff(CM.plan(*c)["bounds"])[0])
    last = lambda c: int(np.diff(CM.plan(*c)["bounds"])[-1])
    assert first(PLAN_CASES[0]) == 2048 and last(PLAN_CASES[0]) == 0          # o_12 = 24571.2: inside the dwell's last sample, empty
    assert first(PLAN_CASES[1]) == 3 and last(PLAN_CASES[1]) == 2045
    assert first(PLAN_CASES[2]) == 1                             # cp = N - 0.25 >= T too: o_1 = 0.15
    assert first(PLAN_CASES[3]) == 1                             # o_0 = 2047.8 - 2 * 2047.6 < 0, o_1 = 0.2: one sample
    assert [first(c) for c in PLAN_CASES[4:7]] == [701, 701, 701] and [last(c) for c in PLAN_CASES[4:7]] == [1347, 1431, 1256]
    assert CM.plan(*PLAN_CASES[7])["n_segments"] == 12 and CM.plan(*PLAN_CASES[8])["n_segments"] == 13
    assert CM.plan(*PLAN_CASES[9])["n_segments"] == 14 and last(PLAN_CASES[9]) == 0
    assert CM.plan(*PLAN_CASES[10])["n_segments"] == 2 and CM.plan(*PLAN_CASES[11])["n_segments"] == 1


@pytest.mark.parametrize("case", REFUSED)
def test_cancel_plan_refuses(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    assert CM.plan(*case) is None, case
    with pytest.raises(GmError) as e:
        A.cancel_plan(*case)
    assert e.value.status == INVALID, case


def test_cancel_plan_checks_the_capacity_and_takes_null_outputs(gm):
    L = gm.lib()
    want = CM.plan(*PLAN_CASES[1])
    Q = want["n_segments"]
    q = C.c_uint32(77)
    b = np.full(Q + 2, 99, np.uint64)
    bp = b.ctypes.data_as(C.c_void_p)
    assert L.gm_acq_cancel_plan(D_DRIFT, N, 2.5, N - 0.4, C.byref(q), bp, Q) == INVALID       # one short
    assert q.value == 77 and (b == 99).all()                                                   # nothing written
    assert L.gm_acq_cancel_plan(D_DRIFT, N, 2.5, N - 0.4, None, bp, Q + 1) == 0
    assert (b[:Q + 1].astype(np.int64) == want["bounds"]).all() and b[Q + 1] == 99
    assert L.gm_acq_cancel_plan(D_DRIFT, N, 2.5, N - 0.4, C.byref(q), None, 0) == 0 and q.value == Q
    assert L.gm_acq_cancel_plan(D_DRIFT, N, 2.5, N - 0.4, None, None, 0) == 0


def test_a_null_handle_is_refused_without_a_device(gm):
    from gnss_sdr_rs_amd import _lib
    cand, out = _lib.AcqCancelCand(0, 0, 1.0, 0.0, 0.0), _lib.AcqCancelOut()
    vp = lambda o: C.cast(C.byref(o), C.c_void_p)
    assert gm.lib().gm_acq_cancel(None, None, 0, vp(cand), 1, C.c_void_p(4096), vp(out), None, 0) == INVALID


# ---- the model's self-checks -------------------------------------------------------------------------------------------------------
def _random_dwell(seed, D):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) + 1j * rng.standard_normal(D), np.sign(rng.standard_normal(1023))


@pytest.mark.parametrize("case", PLAN_CASES[:7])
def test_the_model_is_a_projection(case):
    """cancelling the model's own output again with the same candidate finds nothing: amplitudes below 1e-12 of the first pass's"""
    D, n, cp, T = case
    x, code = _random_dwell(3, D)
    y, a1, b = CM.cancel(x, code, cp, 513.1e3, T or float(n), CM.FS, 1023, False)
    assert (b == CM.plan(*case)["bounds"]).all()
    _, a2, _ = CM.cancel(y, code, cp, 513.1e3, T or float(n), CM.FS, 1023, False)
    assert np.abs(a2).max() <= 1e-12 * np.abs(a1).max()
    assert (np.abs(a1) > 0.0).sum() >= len(a1) - 1               # (the dwell's last segment may be empty: a = 0)


def test_the_models_real_output_is_real():
    x, code = _random_dwell(4, D_DRIFT)
    y, a, _ = CM.cancel(x.real.astype(np.complex128), code, 2.5, 513.1e3, N - 0.4, CM.FS, 1023, True)
    assert (y.imag == 0.0).all() and np.abs(a).min() > 0.0 and not (y.real == x.real).all()
    yy, aa, bb = CM.cancel_all(np.rint(20 * x.real).astype(np.int8), [code, -code],
                               [dict(worker=0, carrier_hz=513.1e3, code_phase=2.5, period_samples=N - 0.4),
                                dict(worker=1, carrier_hz=511.0e3, code_phase=99.0)], CM.FS, N, True)
    assert (yy.imag == 0.0).all() and len(aa) == len(bb) == 2 and len(aa[1]) == CM.plan(D_DRIFT, N, 99.0)["n_segments"]


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene_run(oracle, seed):
    """One seed of the scene through search_model, the strong cell's local evaluation, the model's subtraction and search_model
    again: computed once, shared (tests/test_gpu_cancel.py takes seed SEEDS[0]) and left unchanged."""
    if seed in _SCENES:
        return _SCENES[seed]
    c = CM.scene(oracle.ca_code_table(), seed)
    tabs = [oracle.DopplerShiftTable(CM.F_IF, float(d), CM.FS, N) for d in AM.DOP]
    tables = [t.table for t in tabs]
    tf = np.array([t.doppler_freq_hz for t in tabs], np.float32)
    search = lambda x: AM.search_model(x, tables, c["codes"], N, 1, CM.PERIODS, tf, CM.FS, starts=c["starts"])
    mx, am, sm = search(c["x"])
    ds, strong_before = CM.best_cell(mx, sm, CM.STRONG["worker"])
    dw, _ = CM.best_cell(mx, sm, CM.WEAK["worker"])
    cand = CM.strong_candidate(c, tables, tf, ds, am[CM.STRONG["worker"], 0, ds])
    y, amps, bounds = CM.cancel_all(c["x"], c["chips"], [cand], CM.FS, N, False)
    mx2, am2, sm2 = search(y.astype(np.complex64))
    _, strong_after = CM.best_cell(mx2, sm2, CM.STRONG["worker"])
    dw2, weak_after = CM.best_cell(mx2, sm2, CM.WEAK["worker"])
    _SCENES[seed] = dict(c=c, cand=cand, strong_bin=ds, strong_phase=int(am[CM.STRONG["worker"], 0, ds]), strong_before=strong_before,
                         strong_after=strong_after, weak_before=int(am[CM.WEAK["worker"], 0, dw]),
                         weak_after=int(am2[CM.WEAK["worker"], 0, dw2]), weak_ratio_after=weak_after, y=y, amps=amps[0], bounds=bounds[0])
    return _SCENES[seed]


def test_the_weak_satellite_appears_once_the_strong_one_is_subtracted(oracle):
    """Condition 1: before, the weak worker's best cell is at the true code phase {1200, 1201} in at most 1 of 6 seeds.  Condition 2:
    after, in 6 of 6.  The strong worker's best peak-to-mean after is at most STRONG_AFTER_BOUND = 34 (measured: 15.7, 5.2, 16.8,
    9.0, 14.5, 8.0; before: 347 to 384)."""
    before = after = 0
    for seed in SEEDS:
        r = scene_run(oracle, seed)
        print("seed %d: strong cell bin %d phase %d, peak-to-mean %.1f -> %.1f; candidate carrier %+.2f Hz, code phase %+.3f sample "
              "off; weak best cell's arg-max %d -> %d (peak-to-mean %.1f after)"
              % (seed, r["strong_bin"], r["strong_phase"], r["strong_before"], r["strong_after"],
                 r["cand"]["carrier_hz"] - (CM.F_IF + CM.STRONG["doppler"]), r["cand"]["code_phase"] - CM.STRONG["code_start"],
                 r["weak_before"], r["weak_after"], r["weak_ratio_after"]))
        before += r["weak_before"] in CM.WEAK_PHASES
        after += r["weak_after"] in CM.WEAK_PHASES
        assert r["strong_before"] > 100.0 and r["strong_phase"] in (700, 701), seed
        assert r["strong_after"] <= STRONG_AFTER_BOUND, (seed, r["strong_after"])
        assert r["cand"]["period_samples"] == CM.T_TRUE
    assert before <= 1, before
    assert after == len(SEEDS), after
