"""Fine Doppler from per-period prompts on the CPU: the two additive entries in every layer (this test fails without the feature), the
ABI number they leave alone, gm_acq_refine_plan (host only, no device) against the numpy rules of acq_refine_model.py with every
GM_ERR_INVALID_ARG case, and the float64 model against the simulated Doppler of the truth scenes the GPU file runs end to end."""
import os
import re

import numpy as np
import pytest

import acq_model as AM
import acq_refine_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_refine_doppler", "gm_acq_refine_plan"]
INVALID = -1


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
    assert "gm_acq_refine_doppler" in hpp and "bool refine_doppler" in hpp
    assert "pub fn refine_doppler" in _read("rust", "src", "mi355x", "do_acquisition.rs")
    assert "acq_refine.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert hasattr(A.AcquisitionEngine, "refine_doppler") and hasattr(A, "refine_plan")
    for words in ("gm_acq_refine_cfg", "gm_acq_refine_out", "NOT compensated"):
        assert words in header, words
    # the ctypes structs have the header's layout: 12 and 56 bytes, the double first
    import ctypes as C
    assert C.sizeof(_lib.AcqRefineCfg) == 12 and C.sizeof(_lib.AcqRefineOut) == 56 and _lib.AcqRefineOut.carrier_hz.offset == 0


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"


# (K, M, fs, N, table_freq, bin, span_periods, n_freq, half_span_hz)
EVEN = [-300.0, 0.0, 300.0]
UNEVEN = [-300.0, 0.0, 500.0]
VALID = [
    (4, 3, 2.048e6, 2048, EVEN, 1, 0, 0, 0.0),                  # the defaults: J = K, G = M, Z = 257, half the bin spacing
    (4, 3, 2.048e6, 2048, EVEN, 1, 4, 0, 0.0),                  # span_periods = K is allowed
    (0, 10, 8.0e6, 8000, EVEN, 0, 0, 0, 0.0),                   # K = 0 counts as 1: J = M, G = 1; an edge bin has one neighbour
    (1, 10, 8.0e6, 8000, EVEN, 2, 3, 0, 0.0),                   # J = 3, G = floor(10 / 3) = 3
    (1, 6, 2.048e6, 2048, UNEVEN, 1, 6, 0, 0.0),                # the farther neighbour: 250 Hz
    (1, 6, 2.048e6, 2048, UNEVEN, 0, 2, 0, 0.0),                # 150 Hz
    (1, 6, 2.048e6, 2048, UNEVEN, 2, 2, 3, 0.0),                # 250 Hz; the smallest grid
    (20, 4, 16.3676e6, 16368, [4.1304e6], 0, 0, 4097, 0.0),     # one bin: fs / (2 N K); the largest grid
    (1, 2, 2.0e6, 2000, [0.0], 0, 0, 0, 0.0),                   # one bin at K = 1: fs / (2 N)
    (3, 2, 2.0e6, 2000, EVEN, 1, 0, 33, 500.0),                 # a given half-span at the limit fs / (2 N)
    (3, 2, 2.0e6, 2000, [-3000.0, 0.0, 3000.0], 1, 0, 0, 0.0),  # a default above the limit is cut to it
    (32, 1, 2.0e6, 2000, EVEN, 1, 0, 0, 12.5),
]
INVALID_CASES = [
    (33, 1, 2.0e6, 2000, EVEN, 1, 0, 0, 0.0),                   # K > 32
    (4, 3, 2.0e6, 2000, EVEN, 1, 3, 0, 0.0),                    # span_periods neither 0 nor K on a coherent handle
    (1, 1, 2.0e6, 2000, EVEN, 1, 0, 0, 0.0),                    # J = M = 1: one period carries no frequency information
    (1, 6, 2.0e6, 2000, EVEN, 1, 1, 0, 0.0),                    # J = 1
    (1, 6, 2.0e6, 2000, EVEN, 1, 7, 0, 0.0),                    # J > M: no group
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 2, 0.0),                    # n_freq below 3
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 256, 0.0),                  # even
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 4099, 0.0),                 # above 4097
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 0, 500.5),                  # a half-span above fs / (2 N)
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 0, -10.0),                  # negative
    (4, 3, 2.0e6, 2000, EVEN, 1, 0, 0, float("nan")),
    (4, 3, 2.0e6, 2000, EVEN, 3, 0, 0, 0.0),                    # bin >= n_bins
    (4, 0, 2.0e6, 2000, EVEN, 1, 0, 0, 0.0),                    # n_integrations = 0
    (4, 3, 2.0e6, 0, EVEN, 1, 0, 0, 0.0),                       # fft_size = 0
    (4, 3, 2.0e6, 2000, [], 0, 0, 0, 0.0),                      # no bins
]


@pytest.mark.parametrize("case", VALID)
def test_refine_plan_follows_the_numpy_rules(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    K, M, fs, N, tf, b, span, Z, hs = case
    want = RM.plan(K, M, fs, N, tf, b, span, Z, hs)
    assert want is not None, case
    got = A.refine_plan(K, M, fs, N, tf, b, span, Z, hs)
    assert {k: got[k] for k in ("span_periods", "n_groups", "n_freq")} == {k: want[k] for k in ("span_periods", "n_groups", "n_freq")}, (got, want)
    assert got["half_span_hz"] == pytest.approx(want["half_span_hz"], rel=1e-12) and got["step_hz"] == pytest.approx(want["step_hz"], rel=1e-12)
    assert got["step_hz"] * ((got["n_freq"] - 1) // 2) == pytest.approx(got["half_span_hz"], rel=1e-12)


def test_refine_plan_values():
    """the numpy rules themselves, on the cases the header spells out"""
    assert RM.plan(4, 3, 2.048e6, 2048, EVEN, 1) == dict(span_periods=4, n_groups=3, n_freq=257, half_span_hz=150.0, step_hz=150.0 / 128)
    assert RM.plan(1, 6, 2.048e6, 2048, UNEVEN, 1, 6)["half_span_hz"] == 250.0
    assert RM.plan(1, 6, 2.048e6, 2048, UNEVEN, 0, 2)["half_span_hz"] == 150.0
    assert RM.plan(1, 10, 8.0e6, 8000, EVEN, 2, 3)["n_groups"] == 3
    assert RM.plan(20, 4, 16.3676e6, 16368, [4.1304e6])["half_span_hz"] == pytest.approx(16.3676e6 / (2 * 16368 * 20), rel=1e-7)
    assert RM.plan(3, 2, 2.0e6, 2000, [-3000.0, 0.0, 3000.0], 1)["half_span_hz"] == 500.0


@pytest.mark.parametrize("case", INVALID_CASES)
def test_refine_plan_refuses(gm, case):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    assert RM.plan(*case) is None, case
    with pytest.raises(GmError) as e:
        A.refine_plan(*case)
    assert e.value.status == INVALID, case


def test_refine_plan_takes_null_outputs_and_a_null_cfg(gm):
    import ctypes as C
    tf = np.array(EVEN, np.float32)
    L = gm.lib()
    z = C.c_uint32(0)
    assert L.gm_acq_refine_plan(4, 3, None, 2.048e6, 2048, 3, tf.ctypes.data_as(C.c_void_p), 1, None, None, C.byref(z), None, None) == 0
    assert z.value == 257
    assert L.gm_acq_refine_plan(4, 3, None, 2.048e6, 2048, 3, None, 1, None, None, None, None, None) == INVALID


def test_a_null_handle_is_refused_without_a_device(gm):
    import ctypes as C
    from gnss_sdr_rs_amd import _lib
    out = _lib.AcqRefineOut()
    res, found = _lib.AcqResult(), C.c_uint8(1)
    st = gm.lib().gm_acq_refine_doppler(None, C.cast(C.byref(res), C.c_void_p), C.cast(C.byref(found), C.c_void_p), 1, None,
                                        C.cast(C.byref(out), C.c_void_p), None, None)
    assert st == INVALID


# ---- the model against the simulated Doppler -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RM.TRUTH_SCENES))
def test_the_model_finds_the_simulated_doppler(oracle, name):
    """The float64 search model finds the satellite's cell (bin 1, the edge's offset, the code start); the float64 estimator on that
    cell lands within 1 / (4 R_u T_code) of the simulated carrier — a quarter of the dwell's own frequency resolution."""
    c = RM.truth_scene(oracle.ca_code_table(), name)
    N, fs, K, M = c["N"], c["fs"], c["K"], c["M"]
    tables = [oracle.DopplerShiftTable(c["f_if"], float(d), fs, N) for d in AM.DOP]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    tab = np.stack([t.table for t in tables])
    mx, am, _ = AM.search_model(c["x"], tab, c["codes"], N, K, M, tf, fs, c["starts"], c["offsets"], c["sec"])
    h, d = np.unravel_index(int(np.argmax(mx[0])), mx[0].shape)
    offs = c["offsets"] or [0]
    assert d == 1 and offs[h] == c["edge"], (name, mx[0])
    others = mx[0].copy()
    others[h, d] = 0.0
    print("scene %s: the largest other cell is %.3f of the true cell" % (name, others.max() / mx[0, h, d]))
    assert others.max() <= (1.0 - RM.TRUTH_MARGIN) * mx[0, h, d], (name, mx[0])      # (the device's words are within 1e-5 of these)
    cp = int(am[0, h, d])
    assert c["cp_window"][0] <= cp <= c["cp_window"][1], (name, cp)
    p = RM.plan(K, M, fs, N, tf, d, c["span"])
    J, G = p["span_periods"], p["n_groups"]
    r = RM.refine(c["x"], tab[d], c["codes"][0], N, c["starts"][d], offs[h], cp, tf[d], fs, J, G, p["n_freq"], p["half_span_hz"], c["sec"])
    err, bound = r["carrier_hz"] - c["f_true"], RM.truth_bound(J * G)
    print("scene %s: R_u %d, model error %+.2f Hz, bound %.1f Hz, step %.2f Hz" % (name, J * G, err, bound, r["step_hz"]))
    assert r["at_edge"] == 0 and abs(err) <= bound, (name, err, bound)
    # S at delta = 0 is the cell's accumulated peak power where the groups are the search's own
    if K >= 2:
        assert r["S"][(p["n_freq"] - 1) // 2] == pytest.approx(mx[0, h, d], rel=1e-9)
    else:
        z = RM.prompts(c["x"], tab[d], c["codes"][0], N, c["starts"][d], 0, M, cp)
        assert float(N) ** 2 * np.sum(np.abs(z) ** 2) == pytest.approx(mx[0, h, d], rel=1e-9)
