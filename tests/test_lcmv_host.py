"""Several constraints on one beam on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number
and gm_beamformer left alone, gm_lcmv_plan (host only, no device) against the float64 model of lcmv_model.py, the model's own facts, and
the two scenes that motivate the entry: a second signal with the satellite's code that one constraint leaves standing, and a space-time
beam whose single constraint skews the correlation triangle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import beam_model as BM
import lcmv_model as LM
import stap_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_lcmv_plan", "gm_lcmv_create", "gm_lcmv_destroy", "gm_lcmv_reset", "gm_lcmv_stats", "gm_lcmv_synchronize",
           "gm_lcmv_set_constraints", "gm_lcmv_set_weights", "gm_lcmv_capture", "gm_lcmv_process_dev", "gm_lcmv_process"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, lcmv
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
    assert "class Lcmv" in hpp
    assert "GmLcmvCfg" in rust and "pub enum GmLcmv" in rust
    build = _read("gnss-sdr-rs_amd", "build.py")
    assert "lcmv_kernels.hip" in build and "stap_core.h" in build
    assert '#include "stap_core.h"' in _read("gnss-sdr-rs_amd", "csrc", "lcmv_kernels.hip")
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_lcmv" in internal and "LcmvArgs" in internal
    assert gnss_sdr_rs_amd.Lcmv is lcmv.Lcmv
    for method in ("plan", "process", "process_dev", "set_constraints", "set_weights", "capture", "reset", "stats", "synchronize", "want_blocks"):
        assert hasattr(lcmv.Lcmv, method), method
    assert callable(lcmv.plan)
    for words in ("gm_lcmv_cfg", "C^H w = f", "conj(f_q)", "NOT word for word", "w0_p = C (C^H C)^-1 f", "1e-10"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "lcmv_kernels.hip" in _read("README.md") and "4.4k" in _read("DESIGN.md")
    stats = _read("profiles", "lcmv_kernel_stats.txt")
    assert "lcmv_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: six 4-byte words, three pointers, one 8-byte word
    Cfg = _lib.LcmvCfg
    assert C.sizeof(Cfg) == 56 and Cfg.n_beams.offset == 16 and Cfg.reserved32.offset == 20 and Cfg.n_constraints.offset == 24
    assert Cfg.constraints.offset == 32 and Cfg.response.offset == 40 and Cfg.reserved.offset == 48
    body = re.search(r"pub struct GmLcmvCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in Cfg._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} gm_lcmv_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in Cfg._fields_]


def test_the_abi_number_and_the_beamformer_stay(gm):
    from gnss_sdr_rs_amd import _lib, beamformer
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.BeamformerCfg) == 40 and _lib.BeamformerCfg.steering.offset == 24
    assert beamformer.plan(4, 4, np.eye(16, dtype=np.complex64)[:2], n_in=5000) == dict(block=1024, loading=float(np.float32(1e-4)), n_out=4096)


# ---- gm_lcmv_plan ----------------------------------------------------------------------------------------------------------------------
def _unit(M, qs):
    """beam p: rows e_k .. e_{k + Q_p - 1} (k = p mod M, wrapping), responses 1, 0, .."""
    out = []
    for p, Q in enumerate(qs):
        rows = np.zeros((Q, M), np.complex64)
        for q in range(Q):
            rows[q, (p + q) % M] = 1.0
        out.append((rows, np.array([1.0] + [0.0] * (Q - 1), np.complex64)))
    return out


def _plan(cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import lcmv
    return lcmv.plan(inputs_so_far=so_far, n_in=n_in, **cfg)


def _raw(gm, cfg, so_far=0, n_in=10):
    """gm_lcmv_plan on the packed words of a configuration that the wrapper's own shape rules may not take"""
    from gnss_sdr_rs_amd import _lib
    c = dict(cfg)
    beams = c.pop("constraints")
    A, L = c["n_antennas"], c["taps"]
    rows = np.ascontiguousarray(np.concatenate([np.asarray(r).astype(np.complex64).reshape(-1) for r, _ in beams]))
    f = np.ascontiguousarray(np.concatenate([np.asarray(v).astype(np.complex64).reshape(-1) for _, v in beams]))
    q = np.array([np.asarray(v).size for _, v in beams], np.uint32)
    raw = _lib.LcmvCfg(A, L, c.get("block", 0), c.get("loading", 0.0), len(q), 0, q.ctypes.data, rows.ctypes.data, f.ctypes.data, 0)
    return gm.lib().gm_lcmv_plan(C.byref(raw), so_far, n_in, None, None, None)


PAIRS = [(A, L) for A in range(2, 9) for L in range(1, 9) if A * L <= 32]


def test_plan_fills_in_the_defaults(gm):
    assert len(PAIRS) == 43
    for A, L in PAIRS:
        M = A * L
        for qs in ([1], [min(M, 8)], [1] * 16, [min(M, 8), min(M, 8)]):
            cs = _unit(M, qs)
            assert _plan(dict(n_antennas=A, taps=L, constraints=cs)) == dict(block=1024, loading=float(np.float32(1e-4)), n_out=0), (A, L, qs)
            p = LM.resolve(A, L, cs)
            assert (p["A"], p["L"], p["M"], p["B"], p["loading"], p["P"], p["Q"]) == (A, L, M, 1024, float(np.float32(1e-4)), len(qs), qs)
    for B in SM.BLOCKS:
        got = _plan(dict(n_antennas=4, taps=4, constraints=_unit(16, [2, 2, 1]), block=B, loading=1e-2))
        assert got == dict(block=B, loading=float(np.float32(1e-2)), n_out=0)
    for ld in (1e-6, 1.0):
        assert _plan(dict(n_antennas=2, taps=8, constraints=_unit(16, [8, 8]), loading=ld))["loading"] == float(np.float32(ld))
        assert LM.resolve(2, 8, _unit(16, [8, 8]), loading=ld)["loading"] == float(np.float32(ld))
    # the alternative form: rows per beam and responses per beam
    cs = _unit(8, [2, 1])
    assert _plan(dict(n_antennas=4, taps=2, constraints=[r for r, _ in cs], response=[f for _, f in cs], block=512))["block"] == 512


@pytest.mark.parametrize("cfg", [dict(n_antennas=2, taps=8, block=256, constraints=_unit(16, [8, 8])),
                                 dict(n_antennas=4, taps=4, constraints=_unit(16, [1] * 16)),
                                 dict(n_antennas=8, taps=4, block=16384, constraints=_unit(32, [3, 2, 8])),
                                 dict(n_antennas=2, taps=1, block=4096, constraints=[([[1, 1j], [1, -1j]], [1, 0.5j])])])
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, cfg):
    p = LM.resolve(**cfg)
    B = p["B"]
    for T in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, (1 << 32) + 5, 1 << 62):
        n = LM.total_out(p, T)
        assert n == B * (T // B) and _plan(cfg, 0, T)["n_out"] == n, T
    for so_far in (0, 1, B - 1, B, B + 1, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5 * B - 7):
        for n_in in (0, 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7):
            assert _plan(cfg, so_far, n_in)["n_out"] == LM.plan(p, so_far, n_in), (so_far, n_in)
    assert _plan(cfg, 1 << 62, 0)["n_out"] == 0
    so_far = total = 0
    for n_in in (1, B - 1, 7, B, 1000, 3001):                     # the sum of the calls is the count of the whole, whatever the cuts
        total += _plan(cfg, so_far, n_in)["n_out"]
        so_far += n_in
    assert total == LM.total_out(p, so_far)


def _beamformer_refusals():
    """gm_beamformer's refusals of the shape, the block and the loading (test_stap_host.REFUSED's), with a good beam"""
    import test_stap_host as TH
    out = []
    for cfg in TH.REFUSED:
        if "steering" in cfg:
            continue
        A, L = cfg["n_antennas"], cfg["taps"]
        M = A * L if 0 < A * L <= 64 else 4
        out.append(dict(cfg, constraints=_unit(M, [1])))
    return out


_R4 = np.array([[1, 2, 0, 1j], [0, 1, 1, 0], [1, 3, 1, 1j]], np.complex64)          # the third row is the sum of the first two
REFUSED = _beamformer_refusals() + [
    dict(n_antennas=2, taps=2, constraints=_unit(4, [1] * 17)),                                   # P = 17
    dict(n_antennas=4, taps=4, constraints=_unit(16, [8, 8, 1])),                                 # sum Q = 17
    dict(n_antennas=4, taps=4, constraints=_unit(16, [2] * 8 + [1])),
    dict(n_antennas=2, taps=1, constraints=[(np.eye(3, 2), [1, 0, 0])]),                          # Q above M
    dict(n_antennas=4, taps=4, constraints=[(np.eye(9, 16), [1] * 9)]),                           # Q above 8
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0], [0, 0, 0, 0]], [1, 0])]),             # a row that is all zero
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0]], [1]), ([[0, 0, 0, 0]], [1])]),
    dict(n_antennas=3, taps=1, constraints=[([[1, 0, 0], [1, math.nan, 0]], [1, 0])]),            # a row that is not finite
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, complex(0, math.inf)]], [1])]),
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0]], [math.nan])]),                       # a response that is not finite
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0], [0, 1, 0, 0]], [1, complex(0, -math.inf)])]),
    dict(n_antennas=2, taps=2, constraints=[([[1, 1j, 0, 2], [1, 1j, 0, 2]], [1, 0])]),           # dependent rows: equal,
    dict(n_antennas=2, taps=2, constraints=[([[1, 1j, 0, 2], [2j, -2, 0, 4j]], [1, 0])]),         # a multiple,
    dict(n_antennas=2, taps=2, constraints=[(_R4, [1, 0, 0])]),                                   # a sum,
    dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0]], [1]), (_R4, [1, 0, 0])]),            # in a later beam,
    dict(n_antennas=2, taps=2, constraints=[([[1, 1, 1, 1], [1, 1, 1, 1 + 1e-6]], [1, 0])]),      # and nearly: pivot 1.7e-13 of the norm
]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_refuses(gm, cfg):
    assert LM.resolve(**cfg) is None, cfg
    assert _raw(gm, cfg) == INVALID, cfg


def test_plan_takes_the_limits(gm):
    """Q = M, sum Q = 16, rows that are close but independent, and the same rows in two beams"""
    for cfg in (dict(n_antennas=2, taps=1, constraints=[([[1, 1j], [1, -1j]], [1, 0])]),
                dict(n_antennas=4, taps=2, constraints=_unit(8, [8, 8])),
                dict(n_antennas=4, taps=4, constraints=_unit(16, [8, 7, 1])),
                dict(n_antennas=2, taps=2, constraints=[([[1, 1, 1, 1], [1, 1, 1, 1.001]], [1, 0])]),         # pivot 1.9e-7 of the norm
                dict(n_antennas=2, taps=2, constraints=[([[1, 0, 0, 0], [0, 1, 0, 0]], [1, 0]), ([[1, 0, 0, 0], [0, 1, 0, 0]], [0, 1])])):
        assert LM.resolve(**cfg) is not None, cfg
        assert _raw(gm, cfg) == 0, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    Cfg = _lib.LcmvCfg
    cs = _unit(16, [1] * 16)
    q = np.ones(16, np.uint32)
    rows = np.ascontiguousarray(np.concatenate([r for r, _ in cs]))
    f = np.ones(16, np.complex64)
    args = (q.ctypes.data, rows.ctypes.data, f.ctypes.data)
    ok = Cfg(4, 4, 0, 0.0, 16, 0, *args, 0)
    n = C.c_uint64(77)
    plan = lambda cfg, so_far, n_in: L.gm_lcmv_plan(cfg, so_far, n_in, None, None, C.byref(n))
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 1, *args, 0)), 0, 10) == INVALID and LM.resolve(4, 4, cs, reserved32=1) is None
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, *args, 1)), 0, 10) == INVALID and LM.resolve(4, 4, cs, reserved=1) is None
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, *args, 1 << 40)), 0, 10) == INVALID
    for k in range(3):                                             # each of the three pointers is required
        a = list(args)
        a[k] = None
        assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, *a, 0)), 0, 10) == INVALID
    assert LM.resolve(4, 4, None) is None
    for P in (0, 17, 1 << 31):
        assert plan(C.byref(Cfg(4, 4, 0, 0.0, P, 0, *args, 0)), 0, 10) == INVALID, P
    for bad in (0, 9, 17, 1 << 31):                                # a Q_p outside its range
        q2 = q.copy()
        q2[3] = bad
        assert plan(C.byref(Cfg(4, 4, 0, 0.0, 4, 0, q2.ctypes.data, rows.ctypes.data, f.ctypes.data, 0)), 0, 10) == INVALID, bad
    assert plan(None, 0, 10) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert LM.plan(LM.resolve(4, 4, cs), so_far, n_in) is None
        assert plan(C.byref(ok), so_far, n_in) == INVALID
    assert n.value == 77                                           # nothing written
    assert L.gm_lcmv_plan(C.byref(ok), 0, 5000, None, None, None) == 0
    assert plan(C.byref(ok), 0, 5000) == 0 and n.value == 4096     # per beam
    # a null handle is refused without a device
    assert L.gm_lcmv_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None) == INVALID
    assert L.gm_lcmv_process(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None, None, 0) == INVALID
    assert L.gm_lcmv_reset(None, 0) == INVALID and L.gm_lcmv_stats(None, None, None, None, None) == INVALID
    assert L.gm_lcmv_set_weights(None, None) == INVALID and L.gm_lcmv_capture(None, None, None, 0) == INVALID
    assert L.gm_lcmv_set_constraints(None, 0, 1, rows.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.gm_lcmv_synchronize(None) == INVALID and L.gm_lcmv_destroy(None) == 0


# ---- the model's own facts -------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1, [2]), (4, 2, [2, 2, 1]), (2, 8, [8, 8]), (3, 5, [3, 3, 3, 3, 3])]


@pytest.mark.parametrize("A,L,qs", SHAPES)
def test_the_models_own_facts(A, L, qs):
    rng = np.random.default_rng(100 * A + 10 * L + len(qs))
    B, M = 256, A * L
    x = LM.interfered(rng, 4 * B, A)
    x[B - (L - 1):2 * B] = 0.0                                     # an all-zero block, the samples its taps reach back to included
    cs, _ = LM.draw(rng, M, qs)
    p = LM.resolve(A, L, cs, B, 1e-4)
    assert p["P"] == len(qs) and p["Q"] == qs
    r = LM.run(p, x)
    for k in range(p["P"]):
        Ck, fk = p["C"][k], p["f"][k]
        err = np.abs(np.einsum("mq,bm->bq", Ck.conj(), r["w"][:, k]) - fk[None, :]).max()
        assert err <= 1e-12 * max(1.0, np.abs(fk).max()), (k, err)                                # C^H w = f
        assert np.abs(Ck.conj().T @ p["w0"][k] - fk).max() <= 1e-12 * max(1.0, np.abs(fk).max())  # and C^H w0 = f
        assert (r["w"][1, k] == p["w0"][k]).all()                                                 # the all-zero block: w0
        assert list(r["fallback"][:, k]) == [False, True, False, False] and not r["y"][k, B:2 * B].any()
        if qs[k] == M:                                                                            # Q = M: w = C^-H f whatever R is
            want = np.linalg.solve(Ck.conj().T, fk)
            for b in (0, 2, 3):
                assert np.abs(r["w"][b, k] - want).max() <= 1e-9 * np.abs(want).max()
    # a beam's words depend neither on P nor on the other beams
    two = LM.run(LM.resolve(A, L, [cs[-1], cs[0]], B, 1e-4), x)
    assert (two["y"][0] == r["y"][-1]).all() and (two["y"][1] == r["y"][0]).all()
    # Q = 1 with f = 1 is the beamformer's beam
    s = np.stack([c[0][0] for c in cs])
    one = LM.run(LM.resolve(A, L, [([row], [1.0]) for row in s], B, 1e-4), x)
    bm = BM.run(BM.resolve(A, L, s, B, 1e-4), x)
    for k in range(len(s)):
        assert np.abs(one["w"][:, k] - bm[k]["w"]).max() <= 1e-12 * np.abs(bm[k]["w"]).max()
        assert (one["fallback"][:, k] == bm[k]["fallback"]).all()
    # the static mode takes the words as they are
    ws = (rng.standard_normal((len(qs), M)) + 1j * rng.standard_normal((len(qs), M))).astype(np.complex64)
    st = LM.run(p, x, static_w=ws)
    assert st["R"] is None and (st["w32"] == ws[None]).all() and st["y"].shape == (len(qs), 4 * B)


def test_q_equal_m_ignores_r():
    rng = np.random.default_rng(5)
    cs, _ = LM.draw(rng, 2, [2])
    p = LM.resolve(2, 1, cs, 256, 1e-4)
    want = np.linalg.solve(p["C"][0].conj().T, p["f"][0])
    for scale in (1e-3, 1.0, 1e3):
        x = scale * LM.interfered(rng, 256, 2)
        assert np.abs(LM.run(p, x)["w"][0, 0] - want).max() <= 1e-9 * np.abs(want).max()


def test_the_seeds_of_the_gpu_tests_need_no_redraw():
    for case in LM.CASES + [LM.FALLBACK_CASE]:
        assert LM.drawn(case)[1] == 0, case
    for seed, M, qs in LM.DRAWS:
        assert LM.draw(np.random.default_rng(seed), M, qs)[1] == 0, (seed, M, qs)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("L", [1, 2])
def test_a_second_row_removes_the_second_signal(L, seed):
    """B = 1024, loading 1e-4, A = 4, J/N 40 dB.  numpy gave, ratio at (bin 2, 700) / at (bin 2, 1200), seeds 1 / 2 / 3:
    L = 1: one row 109.0, 43.1 / 109.3, 37.0 / 103.5, 40.3; rows (1, 0) 101.8, 0.9 / 101.2, 1.0 / 94.2, 0.7;
           rows (0, 1) 0.7, 237.9 / 0.6, 239.6 / 0.6, 242.5;
    L = 2: one row 109.5, 41.9 / 109.4, 36.0 / 103.6, 39.1; rows (1, 0) 101.7, 0.9 / 100.9, 0.9 / 94.0, 0.7;
           rows (0, 1) 0.7, 237.4 / 0.6, 239.2 / 0.6, 241.4."""
    one, keep, swap = LM.spoofer_cells(seed, L)
    print("L = %d, seed %d: %s" % (L, seed, [(c["best"][:2], round(c["sat"], 1), round(c["other"], 1)) for c in (one, keep, swap)]))
    sat, other = (LM.SAT["bin"], LM.SAT["code_phase"]), (LM.SPOOF["bin"], LM.SPOOF["code_phase"])
    assert one["other"] > LM.DETECT                                # one constraint leaves the second signal standing
    assert keep["other"] < 3.0 and keep["best"][:2] == sat and keep["sat"] > LM.DETECT
    assert swap["sat"] < 3.0 and swap["best"][:2] == other and swap["other"] > LM.DETECT


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("L", [2, 4])
def test_a_row_a_tap_straightens_the_triangle(L, seed):
    """B = 1024, loading 1e-4, A = 4, the jammer and the CW at 40 dB.  numpy gave P[699] / P[700], P[701] / P[700], the ratio at 700,
    seeds 1 / 2 / 3:
    L = 2: one row 0.311, 0.134, 89.6 / 0.311, 0.134, 85.2 / 0.352, 0.149, 82.7; a row a tap 0.252, 0.253, 86.5 / 0.257, 0.268, 81.4 /
           0.292, 0.270, 79.4;
    L = 4: one row 0.276, 0.165, 98.9 / 0.281, 0.169, 94.6 / 0.301, 0.195, 94.2; a row a tap 0.251, 0.250, 94.2 / 0.258, 0.262, 90.4 /
           0.276, 0.283, 90.0."""
    one, taps = LM.triangle_cells(seed, L)
    print("L = %d, seed %d: %s" % (L, seed, [(c["peak"], round(c["early"], 3), round(c["late"], 3), round(c["ratio"], 1)) for c in (one, taps)]))
    assert abs(taps["early"] - taps["late"]) < 0.04
    assert abs(one["early"] - one["late"]) > 0.08
    assert one["peak"] == taps["peak"] == LM.SAT["code_phase"]
