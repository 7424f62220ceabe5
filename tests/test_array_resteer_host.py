"""Re-steering on the device, what needs no device: gm_trk_array_prompts_dev, gm_array_solve_plan, gm_array_rows_solve_dev and
gm_beamformer_set_steering_dev (include/gnss_mi355x.h, "Re-steering on the device").

1. The entries are in every layer: the header, exports.map, the built library's dynamic symbols, _lib, gnss_sdr.hpp, Rust, README,
   DESIGN, INTEGRATION; array_solve.hip is in build.py; the kernel stats file is there.
2. The ABI number is 9, gm_array_row_info keeps its 24 bytes and offsets, gm_array_solve_cfg has one layout in C, ctypes and Rust.
3. gm_array_solve_plan: every rule at its edges and the extents of both layouts, against `_plan` below.
4. The refusals of the three device entries that are made before a device is touched: the process never initialises one here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_trk_array_prompts_dev", "gm_array_solve_plan", "gm_array_rows_solve_dev", "gm_beamformer_set_steering_dev"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, acquisition, beamformer, tracking
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    rust_wrappers = _read("rust", "src", "mi355x", "do_acquisition.rs") + _read("rust", "src", "mi355x", "do_tracking.rs")
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
        assert name in hpp and name in rust_wrappers, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in _read(doc), (doc, name)
    assert "gm_array_solve_cfg" in header and "pub struct GmArraySolveCfg" in rust
    for fn in ("array_prompts_dev(", "solve_plan(", "solve_rows_dev(", "set_steering_dev("):
        assert fn in hpp and "pub fn " + fn in rust_wrappers, fn
    assert callable(acquisition.solve_plan) and callable(acquisition.solve_rows_dev)
    assert hasattr(tracking.TrackingManager, "array_prompts_dev") and hasattr(beamformer.Beamformer, "set_steering_dev")
    assert "array_solve.hip" in _read("gnss-sdr-rs_amd", "build.py")
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_array_solve" in internal and "launch_beam_install" in internal
    for words in ("Re-steering on the device", "PARALLEL-ORDER cyclic Jacobi", "STATUS.", "Not built: per-antenna prompts from the tracker"):
        assert words in header, words
    assert "4.4j" in _read("DESIGN.md") and "## Re-steering on the device" in _read("README.md")
    stats = _read("profiles", "array_solve_kernel_stats.txt")
    assert "array_solve_kernel" in stats and "beam_install_kernel" in stats and "scratch" in stats


def test_the_abi_number_and_the_layouts(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    Info = _lib.ArrayRowInfo
    assert C.sizeof(Info) == 24
    assert [(f[0], getattr(Info, f[0]).offset) for f in Info._fields_] == [("lambda1", 0), ("lambda2", 8), ("ref_index", 16), ("reserved", 20)]
    Cfg = _lib.ArraySolveCfg
    assert C.sizeof(Cfg) == 56
    assert [(f[0], getattr(Cfg, f[0]).offset) for f in Cfg._fields_] == [("m", 0), ("n", 4), ("n_rows", 8), ("n_blocks", 12), ("row_stride", 16),
                                                                        ("vec_stride", 24), ("loading", 32), ("reserved", 36)]
    # the header's fields in order, then Rust's
    body = re.search(r"typedef struct \{([^}]*)\} gm_array_solve_cfg;", _read("include", "gnss_mi355x.h"), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t m, n, n_rows, n_blocks", "uint64_t row_stride, vec_stride", "float    loading", "uint32_t reserved[5]"]
    rust = re.search(r"pub struct GmArraySolveCfg\s*\{([^}]*)\}", _read("rust", "src", "mi355x.rs"), re.S).group(1)
    fields = re.findall(r"pub\s+(\w+)\s*:\s*([^,]+),", re.sub(r"//[^\n]*", "", rust))
    assert fields == [("m", "u32"), ("n", "u32"), ("n_rows", "u32"), ("n_blocks", "u32"), ("row_stride", "u64"), ("vec_stride", "u64"),
                      ("loading", "f32"), ("reserved", "[u32; 5]")]


def _plan(m, n, n_rows, n_blocks, rs, vs, loading, reserved=(0, 0, 0, 0, 0)):
    """the header's rules in a few lines -> (z_words, R_words, row_words) or None"""
    if any(reserved) or not 2 <= m <= 32 or not 1 <= n <= 4096 or not 1 <= n_rows <= 1024 or n_blocks > 1 << 20:
        return None
    if (rs == 0) != (vs == 0):
        return None
    rs, vs = (rs, vs) if rs else (n * m, m)
    if rs < m or vs < m or rs > 1 << 40 or vs > 1 << 40:
        return None
    f = np.float32(loading)
    if f != 0 and not (np.float32(1e-6) <= f <= np.float32(1.0)):
        return None
    return ((n_rows - 1) * rs + (n - 1) * vs + m, n_blocks * m * m, n_rows * m)


def _raw_plan(gm, m, n, n_rows, n_blocks, rs, vs, loading, reserved=(0, 0, 0, 0, 0)):
    from gnss_sdr_rs_amd import _lib
    cfg = _lib.ArraySolveCfg(m, n, n_rows, n_blocks, rs, vs, loading)
    for k, v in enumerate(reserved):
        cfg.reserved[k] = v
    out = [C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)]
    rc = gm.lib().gm_array_solve_plan(C.byref(cfg), *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out), cfg


def test_solve_plan_holds_every_rule(gm):
    from gnss_sdr_rs_amd import acquisition
    good = dict(m=8, n=10, n_rows=12, n_blocks=20, rs=0, vs=0, loading=0.0)
    cases = [good]
    for key, values in (("m", (0, 1, 2, 3, 32, 33, 1 << 31)), ("n", (0, 1, 4096, 4097)), ("n_rows", (0, 1, 1024, 1025)),
                        ("n_blocks", (0, 1, 1 << 20, (1 << 20) + 1)),
                        ("loading", (1e-6, 0.99e-6, 1.0, 1.0001, -1e-3, float("nan"), float("inf"), 1e-2))):
        cases += [dict(good, **{key: v}) for v in values]
    # the strides: both or neither, at least m, the tracker form, overlapping rows (row_stride < n vec_stride is the tracker form's normal case)
    for rs, vs in ((0, 8), (80, 0), (8, 8), (7, 8), (8, 7), (8, 96), (80, 8), (81, 9), (1 << 40, 8), ((1 << 40) + 1, 8), (8, (1 << 40) + 1),
                   (1 << 63, 1 << 63)):
        cases.append(dict(good, rs=rs, vs=vs))
    cases += [dict(good, reserved=tuple(int(j == k) for j in range(5))) for k in range(5)]
    n_ok = 0
    for kw in cases:
        want = _plan(**kw)
        rc, got, _ = _raw_plan(gm, **kw)
        if want is None:
            assert rc == INVALID and got == (77, 78, 79), kw
        else:
            assert rc == 0 and got == want, (kw, got, want)
            n_ok += 1
            if "reserved" not in kw:
                assert acquisition.solve_plan(kw["m"], kw["n"], kw["n_rows"], kw["n_blocks"], kw["rs"], kw["vs"], kw["loading"]) == \
                    dict(z_words=want[0], R_words=want[1], row_words=want[2])
    assert n_ok >= 15 and len(cases) - n_ok >= 15               # (both sides of the rules were visited)
    # the two layouts by hand: acquisition's [n_cands][R_u][m]; a history [n][P][m] of tracker calls
    assert _raw_plan(gm, 8, 10, 12, 20, 0, 0, 0.0)[1] == (12 * 10 * 8, 20 * 64, 96)
    assert _raw_plan(gm, 8, 10, 12, 20, 8, 96, 0.0)[1] == (10 * 12 * 8, 20 * 64, 96)
    # a NULL cfg; any output may be NULL
    assert gm.lib().gm_array_solve_plan(None, None, None, None) == INVALID
    _, _, cfg = _raw_plan(gm, **good)
    assert gm.lib().gm_array_solve_plan(C.byref(cfg), None, None, None) == 0
    with pytest.raises(gm.GmError):
        acquisition.solve_plan(1, 10, 1)


def test_the_refusals_that_need_no_device(gm):
    """NULL handles, NULL pointers and bad cfgs return INVALID_ARG with their own words (a call that reached the device layer without
    one would answer with a HIP status or fault on the made-up addresses)"""
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    fake = C.c_void_p(0x1000)                                    # never dereferenced: every call below is refused before that
    err = lambda: L.gm_last_error().decode() if hasattr(L, "gm_last_error") else ""
    # gm_array_rows_solve_dev: the plan's rules first, then the pointers
    _, _, good = _raw_plan(gm, 8, 10, 12, 20, 0, 0, 0.0)
    for kw in (dict(m=1), dict(n=0), dict(n_rows=1025), dict(n_blocks=(1 << 20) + 1), dict(rs=8, vs=0), dict(rs=7, vs=8), dict(loading=2.0),
               dict(reserved=(0, 0, 1, 0, 0))):
        _, _, cfg = _raw_plan(gm, **dict(dict(m=8, n=10, n_rows=12, n_blocks=20, rs=0, vs=0, loading=0.0), **kw))
        assert L.gm_array_rows_solve_dev(C.byref(cfg), fake, fake, fake, fake, None) == INVALID, kw
    assert L.gm_array_rows_solve_dev(None, fake, fake, fake, fake, None) == INVALID
    for args in ((None, fake, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert L.gm_array_rows_solve_dev(C.byref(good), *args, None) == INVALID, args
        assert "null" in err()
    assert L.gm_array_rows_solve_dev(C.byref(good), fake, None, fake, fake, None) == INVALID          # n_blocks = 20 without d_R
    assert "n_blocks" in err()
    _, _, ident = _raw_plan(gm, 8, 10, 12, 0, 0, 0, 0.0)
    assert L.gm_array_rows_solve_dev(C.byref(ident), fake, fake, fake, fake, None) == INVALID          # d_R with n_blocks = 0
    assert "n_blocks" in err()
    # gm_beamformer_set_steering_dev and gm_trk_array_prompts_dev: a NULL handle is refused before anything else is looked at
    assert L.gm_beamformer_set_steering_dev(None, 0, 1, fake, None, 0.0, None, None) == INVALID
    tcfg = _lib.TrkArrayCfg()
    tcfg.n_antennas, tcfg.taps = 4, 2
    st = (C.c_uint8 * 4096)()
    assert L.gm_trk_array_prompts_dev(None, fake, 0, 0, 100, C.cast(st, C.c_void_p), 1, C.byref(tcfg), fake, fake, None) == INVALID
