"""One beam per satellite on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number and
gm_stap left alone, gm_beamformer_plan (host only, no device) against the float64 model of beam_model.py, the model's own facts, and the
scenes that motivate the entry: two 45 dB-Hz satellites on a line array, searched plainly at N = 2048 behind the power-inversion row e_0
and behind a row that points at each of them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import beam_model as BM
import stap_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_beamformer_plan", "gm_beamformer_create", "gm_beamformer_destroy", "gm_beamformer_reset", "gm_beamformer_stats",
           "gm_beamformer_synchronize", "gm_beamformer_set_steering", "gm_beamformer_set_weights", "gm_beamformer_capture",
           "gm_beamformer_process_dev", "gm_beamformer_process"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, beamformer
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
    assert "class Beamformer" in hpp
    assert "GmBeamformerCfg" in rust and "pub enum GmBeamformer" in rust
    build = _read("gnss-sdr-rs_amd", "build.py")
    assert "beam_kernels.hip" in build and "stap_core.h" in build
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_beam" in internal and "BeamArgs" in internal
    assert gnss_sdr_rs_amd.Beamformer is beamformer.Beamformer
    for method in ("process", "process_dev", "set_steering", "set_weights", "capture", "reset", "stats", "synchronize"):
        assert hasattr(beamformer.Beamformer, method), method
    assert callable(beamformer.plan)
    for words in ("gm_beamformer_cfg", "THE CONTRACT THAT FIXES EVERY WORD", "d_out + p * out_stride", "BOTH ENTRIES ARE SYNCHRONOUS",
                  "s_p / (s_p^H s_p)", "[d_out, d_out + (P - 1) out_stride + count)"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "beam_kernels.hip" in _read("README.md") and "4.4h" in _read("DESIGN.md")
    for doc in ("README.md", os.path.join("include", "gnss_mi355x.h")):
        assert "distortionless or" not in _read(doc) and "several constraints on ONE beam (LCMV)" in _read(doc), doc
    stats = _read("profiles", "beam_kernel_stats.txt")
    assert "beam_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: six 4-byte words, the pointer, one 8-byte word
    Cfg = _lib.BeamformerCfg
    assert C.sizeof(Cfg) == 40 and Cfg.n_beams.offset == 16 and Cfg.reserved32.offset == 20 and Cfg.steering.offset == 24
    assert Cfg.reserved.offset == 32
    body = re.search(r"pub struct GmBeamformerCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in Cfg._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} gm_beamformer_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in Cfg._fields_]


def test_the_abi_number_and_stap_stay(gm):
    from gnss_sdr_rs_amd import _lib, stap
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.StapCfg) == 32 and _lib.StapCfg.steering.offset == 16 and _lib.StapCfg.reserved.offset == 24
    assert stap.plan(4, 4, n_in=5000) == dict(block=1024, loading=float(np.float32(1e-4)), n_out=4096)
    assert gm.lib().gm_stap_plan(C.byref(_lib.StapCfg(4, 4, 0, 0.0, None, 1)), 0, 10, None, None, None) == INVALID


# ---- gm_beamformer_plan ----------------------------------------------------------------------------------------------------------------
def _e0(P, M):
    s = np.zeros((P, M), np.complex64)
    s[:, 0] = 1.0
    return s


def _plan(cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import beamformer
    return beamformer.plan(inputs_so_far=so_far, n_in=n_in, **cfg)


PAIRS = [(A, L) for A in range(2, 9) for L in range(1, 9) if A * L <= 32]


def test_plan_fills_in_the_defaults(gm):
    assert len(PAIRS) == 43
    for A, L in PAIRS:
        for P in (1, 16):
            s = _e0(P, A * L)
            assert _plan(dict(n_antennas=A, taps=L, steering=s)) == dict(block=1024, loading=float(np.float32(1e-4)), n_out=0)
            p = BM.resolve(A, L, s)
            assert (p["A"], p["L"], p["M"], p["B"], p["loading"], p["P"]) == (A, L, A * L, 1024, float(np.float32(1e-4)), P)
    for B in SM.BLOCKS:
        got = _plan(dict(n_antennas=4, taps=4, steering=_e0(3, 16), block=B, loading=1e-2))
        assert got == dict(block=B, loading=float(np.float32(1e-2)), n_out=0)
    for ld in (1e-6, 1.0):
        assert _plan(dict(n_antennas=2, taps=8, steering=_e0(2, 16), loading=ld))["loading"] == float(np.float32(ld))
        assert BM.resolve(2, 8, _e0(2, 16), loading=ld)["loading"] == float(np.float32(ld))


@pytest.mark.parametrize("cfg", [dict(n_antennas=2, taps=8, block=256, steering=_e0(1, 16)), dict(n_antennas=4, taps=4, steering=_e0(16, 16)),
                                 dict(n_antennas=8, taps=4, block=16384, steering=_e0(5, 32)),
                                 dict(n_antennas=3, taps=2, block=4096, steering=[[1, 1j, -1, 0, 0, 0.5], [0, 0, 0, 0, 0, 2]])])
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, cfg):
    p = BM.resolve(**cfg)
    B = p["B"]
    for T in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, (1 << 32) + 5, 1 << 62):
        n = BM.total_out(p, T)
        assert n == B * (T // B) and _plan(cfg, 0, T)["n_out"] == n, T
    for so_far in (0, 1, B - 1, B, B + 1, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5 * B - 7):
        for n_in in (0, 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7):
            assert _plan(cfg, so_far, n_in)["n_out"] == BM.plan(p, so_far, n_in), (so_far, n_in)
    assert _plan(cfg, 1 << 62, 0)["n_out"] == 0
    so_far = total = 0
    for n_in in (1, B - 1, 7, B, 1000, 3001):                     # the sum of the calls is the count of the whole, whatever the cuts
        total += _plan(cfg, so_far, n_in)["n_out"]
        so_far += n_in
    assert total == BM.total_out(p, so_far)


def _stap_refusals():
    """gm_stap's refusals (test_stap_host.REFUSED's configurations without a steering of their own), with a good row"""
    import test_stap_host as TH
    out = []
    for cfg in TH.REFUSED:
        if "steering" in cfg:
            continue
        A, L = cfg["n_antennas"], cfg["taps"]
        M = A * L if 0 < A * L <= 64 else 4
        out.append(dict(cfg, steering=_e0(1, M)))
    return out


REFUSED = _stap_refusals() + [
    dict(n_antennas=2, taps=2, steering=_e0(17, 4)),                                              # P = 17
    dict(n_antennas=2, taps=2, steering=[[1, 0, 0, 0], [0, 0, 0, 0]]),                            # a row that is all zero
    dict(n_antennas=2, taps=2, steering=[[0, 0, 0, 0], [1, 0, 0, 0]]),
    dict(n_antennas=3, taps=1, steering=[[1, 0, 0], [1, math.nan, 0]]),                           # a row that is not finite
    dict(n_antennas=2, taps=2, steering=[[1, 0, 0, complex(0, math.inf)]]),
    dict(n_antennas=2, taps=1, steering=[[1, 1], [1, 1], [complex(-math.inf, 0), 1]]),
]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_refuses(gm, cfg):
    from gnss_sdr_rs_amd import _lib
    assert BM.resolve(**cfg) is None, cfg
    c = dict(cfg)
    s = np.ascontiguousarray(np.asarray(c.pop("steering")).astype(np.complex64))
    A, L = c["n_antennas"], c["taps"]
    P = max(1, s.size // (A * L)) if 0 < A * L <= 64 else 1
    raw = _lib.BeamformerCfg(A, L, c.get("block", 0), c.get("loading", 0.0), P, 0, s.ctypes.data, 0)
    assert gm.lib().gm_beamformer_plan(C.byref(raw), 0, 10, None, None, None) == INVALID, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    Cfg = _lib.BeamformerCfg
    s = _e0(16, 16)
    ok = Cfg(4, 4, 0, 0.0, 16, 0, s.ctypes.data, 0)
    n = C.c_uint64(77)
    plan = lambda cfg, so_far, n_in: L.gm_beamformer_plan(cfg, so_far, n_in, None, None, C.byref(n))
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 1, s.ctypes.data, 0)), 0, 10) == INVALID and BM.resolve(4, 4, s, reserved32=1) is None
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, s.ctypes.data, 1)), 0, 10) == INVALID and BM.resolve(4, 4, s, reserved=1) is None
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, s.ctypes.data, 1 << 40)), 0, 10) == INVALID
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 16, 0, None, 0)), 0, 10) == INVALID and BM.resolve(4, 4, None) is None      # steering is required
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 0, 0, s.ctypes.data, 0)), 0, 10) == INVALID                                  # P = 0
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 17, 0, s.ctypes.data, 0)), 0, 10) == INVALID
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, 1 << 31, 0, s.ctypes.data, 0)), 0, 10) == INVALID
    assert plan(None, 0, 10) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert BM.plan(BM.resolve(4, 4, s), so_far, n_in) is None
        assert plan(C.byref(ok), so_far, n_in) == INVALID
    assert n.value == 77                                           # nothing written
    assert L.gm_beamformer_plan(C.byref(ok), 0, 5000, None, None, None) == 0
    assert plan(C.byref(ok), 0, 5000) == 0 and n.value == 4096     # per beam
    # the steering pointer is read: P M words of it, whatever lies behind
    t = np.array([0, 1j, 0, 2, math.nan], np.complex64)
    assert plan(C.byref(Cfg(2, 1, 0, 0.0, 2, 0, t.ctypes.data, 0)), 0, 10) == 0 and plan(C.byref(Cfg(5, 1, 0, 0.0, 1, 0, t.ctypes.data, 0)), 0, 10) == INVALID
    # a null handle is refused without a device
    assert L.gm_beamformer_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None) == INVALID
    assert L.gm_beamformer_process(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None, None, 0) == INVALID
    assert L.gm_beamformer_reset(None, 0) == INVALID and L.gm_beamformer_stats(None, None, None, None, None) == INVALID
    assert L.gm_beamformer_set_weights(None, None) == INVALID and L.gm_beamformer_capture(None, None, None, 0) == INVALID
    assert L.gm_beamformer_set_steering(None, 0, s.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.gm_beamformer_synchronize(None) == INVALID and L.gm_beamformer_destroy(None) == 0


# ---- the model's own facts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,L,P", [(2, 1, 1), (2, 8, 16), (3, 5, 5), (4, 8, 16), (8, 4, 3)])
def test_the_models_own_facts(A, L, P):
    import test_stap_host as TH
    rng = np.random.default_rng(100 * A + 10 * L + P)
    B, M = 256, A * L
    x = TH._interfered(rng, 4 * B, A)
    x[B - (L - 1):2 * B] = 0.0                                     # an all-zero block, the samples its taps reach back to included
    s = (rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M))).astype(np.complex64)
    s[P - 1] = 0
    s[P - 1, 0] = 1.0                                              # the last row is e_0
    p = BM.resolve(A, L, s, B, 1e-4)
    assert p["P"] == P and (p["s"] == s.astype(np.complex128)).all()
    beams = BM.run(p, x)
    assert len(beams) == P
    for k, r in enumerate(beams):
        sk = p["s"][k]
        assert np.abs(np.einsum("bm,m->b", r["w"].conj(), sk) - 1.0).max() <= 1e-12           # w_p^H s_p = 1
        assert np.abs(r["w"][1] - sk / np.vdot(sk, sk).real).max() == 0.0                     # the all-zero block: s_p / (s_p^H s_p)
        assert list(r["fallback"]) == [False, True, False, False] and not r["y"][B:2 * B].any()
        assert (r["R"] == beams[0]["R"]).all()                                                  # ONE Gram matrix
        alone = SM.run(SM.resolve(A, L, B, 1e-4, s[k]), x)                                      # a beam is the stap model with its row
        assert (alone["w"] == r["w"]).all() and (alone["y"] == r["y"]).all()
    # a beam's words depend neither on P nor on the other rows
    two = BM.run(BM.resolve(A, L, np.stack([s[P - 1], s[0]]), B, 1e-4), x)
    assert (two[0]["y"] == beams[P - 1]["y"]).all() and (two[1]["y"] == beams[0]["y"]).all()


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name,gain", [("clean", None), ("T1", 1.25), ("T2", 3.0)])
def test_every_beam_finds_its_own_satellite(name, gain, seed):
    """B = 1024, loading 1e-4; clean at L = 1, T1 at L = 2, T2 at L = 1.  numpy gave, peak-to-mean of the true cells, seeds 1 / 2 / 3:
    clean: sat 0 behind e_0 29.0 / 26.4 / 29.8, behind its beam 111.9 / 109.5 / 104.7; sat 1 24.6 / 26.1 / 28.1, 100.6 / 109.0 / 100.9;
    T1:    sat 0 53.5 / 51.5 / 50.5, 107.5 / 104.5 / 100.1; sat 1 41.4 / 45.4 / 42.5, 60.9 / 62.1 / 58.7 (smallest ratio 1.38);
    T2:    sat 0 21.1 / 19.6 / 18.8, 175.3 / 167.9 / 170.9; sat 1 32.7 / 33.1 / 34.5, 169.3 / 171.2 / 177.3 (smallest ratio 4.9)."""
    c = BM.cells(name, seed)
    print("%s, seed %d: %s" % (name, seed, {k: (v[0], v[1], round(v[2], 1)) for k, v in c.items()}))
    for w in (0, 1):
        for k in ("e0", "beam"):
            assert BM.found(c[(w, k)], w) and c[(w, k)][2] > BM.DETECT, (w, k, c[(w, k)])
        if gain is not None:
            assert c[(w, "beam")][2] >= gain * c[(w, "e0")][2], (w, c[(w, "beam")][2] / c[(w, "e0")][2])
