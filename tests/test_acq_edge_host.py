"""The edge search of coherent acquisition on the CPU: the five additive entries in every layer, the ABI number they leave alone, the
argument rules of gm_acq_edge_dwell_periods (host only, no device), and the B1I Neumann-Hoffman row."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_edge_dwell_periods", "gm_acq_set_edge_search", "gm_acq_edge_metrics", "gm_acq_edge_choice", "gm_acq_result_offsets"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    L = gm.lib()
    # exports.map exports by pattern: every entry must match it and be a dynamic symbol of the built library
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "pub fn %s(" % name in rust, name
        assert re.fullmatch(pattern.replace("*", ".*"), name), (pattern, name)
        assert getattr(L, name) is not None
    assert "set_edge_search" in _read("rust", "src", "mi355x", "do_acquisition.rs")
    hpp = _read("gnss-sdr-rs_amd", "host", "gnss_sdr.hpp")
    assert "set_edge_search" in hpp and "gm_acq_result_offsets" in hpp


def test_the_abi_number_and_the_trailing_field_stay(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"


def _dwell(gm, K, M, offsets, row=None):
    off = np.ascontiguousarray(offsets, np.uint32)
    sec = None if row is None else np.ascontiguousarray(row, np.int8)
    out = C.c_uint64(0)
    st = gm.lib().gm_acq_edge_dwell_periods(K, M, off.size, off.ctypes.data_as(C.c_void_p),
                                            sec.ctypes.data_as(C.c_void_p) if sec is not None else None, C.byref(out))
    return st, out.value


def test_edge_dwell_periods(gm):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    assert _dwell(gm, 20, 2, list(range(20))) == (0, 59)
    assert _dwell(gm, 10, 1, [0, 5]) == (0, 15)
    assert _dwell(gm, 20, 2, list(range(20)), A.NH20) == (0, 59)
    assert A.edge_dwell_periods(10, 1, [0, 5]) == 15
    INVALID = -1
    assert _dwell(gm, 1, 2, [0, 1])[0] == INVALID                      # K = 1
    assert _dwell(gm, 4, 2, list(range(33)))[0] == INVALID             # H = 33
    assert _dwell(gm, 4, 2, [0, 64])[0] == INVALID                     # an offset of 64
    assert _dwell(gm, 4, 2, [3, 3])[0] == INVALID
    assert _dwell(gm, 4, 2, [5, 2])[0] == INVALID
    assert _dwell(gm, 4, 2, [0, 1], [1, -1, 0, 1])[0] == INVALID       # a row holding 0
    assert _dwell(gm, 4, 2, [0, 63], [1, -1, -1, 1]) == (0, 71)
    assert _dwell(gm, 4, 2, list(range(32))) == (0, 39)
    with pytest.raises(GmError):
        A.edge_dwell_periods(1, 2, [0, 1])


def test_nh20():
    from gnss_sdr_rs_amd import acquisition as A
    nh = A.NH20
    assert nh.dtype == np.int8 and nh.size == 20 and int((nh == 1).sum()) == 12 and int((nh == -1).sum()) == 8
    assert nh[5] == -1
    bits = [0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0]
    assert [int(v) for v in nh] == [1 - 2 * b for b in bits]
