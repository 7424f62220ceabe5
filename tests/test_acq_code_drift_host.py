"""Code-drift compensation of acquisition on the CPU: the five additive entries in every layer, the ABI number they leave alone, and
gm_acq_code_drift_plan (host only, no device) against numpy's float64 floor(p * T + 0.5), with its argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_set_code_drift", "gm_acq_code_drift_plan", "gm_acq_dwell_samples", "gm_acq_code_drift_starts",
           "gm_acq_code_drift_phasors"]
INVALID = -1
L1 = 1575.42e6
PERIODS = [16367.6, 16368.0, 16368.3, 8000.0 / (1.0 + 5000.0 / L1)]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _n_of(T):
    return int(round(T / 8.0)) * 8


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    L = gm.lib()
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    # the dynamic symbols of the built library, read from its file
    with open(_lib.library_path(), "rb") as f:
        blob = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "pub fn %s(" % name in rust, name
        assert re.fullmatch(pattern.replace("*", ".*"), name), (pattern, name)
        assert getattr(L, name) is not None
        assert name.encode() + b"\0" in blob, name
    assert "set_code_drift" in _read("rust", "src", "mi355x", "do_acquisition.rs")
    hpp = _read("gnss-sdr-rs_amd", "host", "gnss_sdr.hpp")
    assert "set_code_drift" in hpp and "gm_acq_dwell_samples" in hpp
    assert "acq_stage_f_drift.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "NOT compensated" in header      # gm_acq_finer_doppler says so


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"


def _plan(gm, N, R, T, want_starts=True):
    t = np.ascontiguousarray(T, np.float64).reshape(-1)
    starts = np.full((t.size, R), 0xFFFFFFFFFFFFFFFF, np.uint64)
    out = C.c_uint64(0)
    st = gm.lib().gm_acq_code_drift_plan(N, R, t.size, t.ctypes.data_as(C.c_void_p),
                                         starts.ctypes.data_as(C.c_void_p) if want_starts else None, C.byref(out))
    return st, starts, out.value


def _numpy_starts(T, R):
    t = np.asarray(T, np.float64).reshape(-1)
    return np.floor(np.arange(R, dtype=np.float64)[None, :] * t[:, None] + 0.5).astype(np.uint64)


@pytest.mark.parametrize("T", PERIODS)
@pytest.mark.parametrize("R", [1, 2, 59, 95])
def test_plan_is_numpys_floor(gm, T, R):
    N = _n_of(T)
    st, starts, dwell = _plan(gm, N, R, [T])
    want = _numpy_starts([T], R)
    assert st == 0 and starts.dtype == want.dtype and (starts == want).all()
    assert dwell == int(want[0, R - 1]) + N
    assert starts[0, 0] == 0
    # within half a sample of p T
    assert np.abs(starts[0].astype(np.float64) - np.arange(R) * T).max() <= 0.5
    # starts may be NULL
    assert _plan(gm, N, R, [T], want_starts=False)[::2] == (0, dwell)


def test_plan_with_bins_that_differ(gm):
    from gnss_sdr_rs_amd import acquisition as A
    N, R = 16368, 95
    T = A.code_period_samples(16.3676e6, 1023, 1.023e6, np.array([-5000.0, 0.0, 5000.0]), L1)
    assert T.dtype == np.float64 and T[0] > T[1] > T[2] and T[1] == 16.3676e6 * 1023 / 1.023e6
    assert A.code_period_samples(16.3676e6, 1023, 1.023e6, 5000.0) == T[1]            # no carrier: the geometry alone
    st, starts, dwell = _plan(gm, N, R, T)
    want = _numpy_starts(T, R)
    assert st == 0 and (starts == want).all()
    assert dwell == int(want[:, R - 1].max()) + N == int(want[0, R - 1]) + N
    assert not (want[0] == want[2]).all()
    s2, d2 = A.code_drift_plan(N, R, T)
    assert (s2 == want).all() and d2 == dwell
    # mixed: the dwell is the longest bin's
    T2 = np.array([16368.3, 16367.6, 16368.0])
    st, starts, dwell = _plan(gm, N, R, T2)
    assert st == 0 and (starts == _numpy_starts(T2, R)).all() and dwell == int(np.floor(94 * 16368.3 + 0.5)) + N


@pytest.mark.parametrize("N", [8000, 16368])
def test_a_period_of_fft_size_is_today(gm, N):
    R = 95
    st, starts, dwell = _plan(gm, N, R, [float(N)] * 3)
    assert st == 0 and (starts == (np.arange(R, dtype=np.uint64) * np.uint64(N))[None, :]).all() and dwell == R * N


def test_argument_checks(gm):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    N = 16368
    assert _plan(gm, N, 10, [N + 8.0])[0] == 0 and _plan(gm, N, 10, [N - 8.0])[0] == 0
    assert _plan(gm, N, 10, [N + 8.001])[0] == INVALID
    assert _plan(gm, N, 10, [N - 8.001])[0] == INVALID
    assert _plan(gm, N, 10, [float(N), 16000.0])[0] == INVALID            # one bad bin among good ones
    assert _plan(gm, N, 10, [float("nan")])[0] == INVALID
    assert _plan(gm, N, 10, [float("inf")])[0] == INVALID
    assert _plan(gm, N, 10, [])[0] == INVALID                              # n_bins = 0
    assert _plan(gm, N, 0, [float(N)])[0] == INVALID                       # no periods
    assert _plan(gm, N + 4, 10, [float(N)])[0] == INVALID                  # fft_size not a multiple of 8
    out = C.c_uint64(0)
    assert gm.lib().gm_acq_code_drift_plan(N, 10, 3, None, None, C.byref(out)) == INVALID
    t = np.array([float(N)])
    assert gm.lib().gm_acq_code_drift_plan(N, 10, 1, t.ctypes.data_as(C.c_void_p), None, None) == INVALID
    with pytest.raises(GmError):
        A.code_drift_plan(N, 10, [N + 9.0])
    # the handle's entries refuse a null handle without a device
    assert gm.lib().gm_acq_set_code_drift(None, 1, t.ctypes.data_as(C.c_void_p)) == INVALID
    assert gm.lib().gm_acq_dwell_samples(None, C.byref(out)) == INVALID
    assert gm.lib().gm_acq_code_drift_starts(None, None) == INVALID
    assert gm.lib().gm_acq_code_drift_phasors(None, 0, None) == INVALID
