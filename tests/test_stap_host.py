"""Space-time adaptive nulling on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number they
leave alone, gm_stap_plan (host only, no device) against the float64 model of stap_model.py, the model's own facts, and the scenes that
motivate the entry: a 45 dB-Hz signal on a line array of A antennas under as many 40 dB interferers as antennas, one of them a plain CW,
searched plainly at N = 2048.  A spatial nuller has A - 1 degrees of freedom and loses the signal; with taps the CW costs a temporal one."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import nuller_model as NM
import stap_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_stap_plan", "gm_stap_create", "gm_stap_destroy", "gm_stap_reset", "gm_stap_stats", "gm_stap_synchronize",
           "gm_stap_set_weights", "gm_stap_capture", "gm_stap_process_dev", "gm_stap_process"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, stap
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
    assert "class Stap" in hpp
    assert "GmStapCfg" in rust and "pub enum GmStap" in rust
    assert "stap_kernels.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_stap" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert gnss_sdr_rs_amd.Stap is stap.Stap
    for method in ("process", "process_dev", "set_weights", "capture", "reset", "stats", "synchronize"):
        assert hasattr(stap.Stap, method), method
    assert callable(stap.plan)
    for words in ("gm_stap_cfg", "total_out(T) = B * (T div B)", "z[t][l A + a] = x_a[t - l]", "d = 32, 16, 8, 4, 2, 1", "l ASCENDING",
                  "w = s / (s^H s)", "not a Toeplitz approximation", "Limits"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "stap_kernels.hip" in _read("README.md") and "4.4g" in _read("DESIGN.md")
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "gnss_mi355x.h")):
        assert "taps in time (STAP)" not in _read(doc), doc         # no longer under "Not built"
    stats = _read("profiles", "stap_kernel_stats.txt")
    assert "stap_kernel" in stats and "stap_state_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: four 4-byte words, the pointer, one 8-byte word
    assert C.sizeof(_lib.StapCfg) == 32 and _lib.StapCfg.steering.offset == 16 and _lib.StapCfg.reserved.offset == 24
    body = re.search(r"pub struct GmStapCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.StapCfg._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} gm_stap_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in _lib.StapCfg._fields_]


def test_the_abi_number_and_the_nuller_stay(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.NullerCfg) == 24 and _lib.NullerCfg.reserved.offset == 12        # gm_nuller_cfg is untouched
    assert gm.lib().gm_nuller_plan(C.byref(_lib.NullerCfg(4, 0, 0.0, 1, None)), 0, 10, None, None, None) == INVALID


# ---- gm_stap_plan ----------------------------------------------------------------------------------------------------------------------
def _plan(cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import stap
    return stap.plan(inputs_so_far=so_far, n_in=n_in, **cfg)


PAIRS = [(A, L) for A in range(2, 9) for L in range(1, 9) if A * L <= 32]


def test_plan_fills_in_the_defaults(gm):
    assert len(PAIRS) == 43
    for A, L in PAIRS:
        got = _plan(dict(n_antennas=A, taps=L))
        assert got == dict(block=1024, loading=float(np.float32(1e-4)), n_out=0)
        p = SM.resolve(A, L)
        assert (p["A"], p["L"], p["M"], p["B"], p["loading"]) == (A, L, A * L, 1024, float(np.float32(1e-4)))
        assert (p["s"] == np.eye(A * L)[0]).all()
    for B in SM.BLOCKS:
        assert _plan(dict(n_antennas=4, taps=4, block=B, loading=1e-2)) == dict(block=B, loading=float(np.float32(1e-2)), n_out=0)
    for ld in (1e-6, 1.0):
        assert _plan(dict(n_antennas=2, taps=8, loading=ld))["loading"] == SM.resolve(2, 8, loading=ld)["loading"] == float(np.float32(ld))


@pytest.mark.parametrize("cfg", [dict(n_antennas=2, taps=8, block=256), dict(n_antennas=4, taps=4), dict(n_antennas=8, taps=4, block=16384),
                                 dict(n_antennas=3, taps=2, block=4096, steering=[1, 1j, -1, 0, 0, 0.5])])
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, cfg):
    p = SM.resolve(**cfg)
    B = p["B"]
    for T in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, (1 << 32) + 5, 1 << 62):
        n = SM.total_out(p, T)
        assert n == B * (T // B) and _plan(cfg, 0, T)["n_out"] == n, T
    for so_far in (0, 1, B - 1, B, B + 1, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5 * B - 7):
        for n_in in (0, 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7):
            assert _plan(cfg, so_far, n_in)["n_out"] == SM.plan(p, so_far, n_in), (so_far, n_in)
    assert _plan(cfg, 1 << 62, 0)["n_out"] == 0
    so_far = total = 0
    for n_in in (1, B - 1, 7, B, 1000, 3001):                     # the sum of the calls is the count of the whole, whatever the cuts
        total += _plan(cfg, so_far, n_in)["n_out"]
        so_far += n_in
    assert total == SM.total_out(p, so_far)


REFUSED = [dict(n_antennas=0, taps=2), dict(n_antennas=1, taps=2), dict(n_antennas=9, taps=2), dict(n_antennas=1 << 31, taps=1),
           dict(n_antennas=4, taps=0), dict(n_antennas=4, taps=9), dict(n_antennas=2, taps=1 << 31), dict(n_antennas=1 << 16, taps=1 << 16),
           dict(n_antennas=5, taps=7), dict(n_antennas=6, taps=6), dict(n_antennas=7, taps=5), dict(n_antennas=8, taps=5),
           dict(n_antennas=4, taps=2, block=128), dict(n_antennas=4, taps=2, block=255), dict(n_antennas=4, taps=2, block=1000),
           dict(n_antennas=4, taps=2, block=1536), dict(n_antennas=4, taps=2, block=32768), dict(n_antennas=4, taps=2, block=1 << 31),
           dict(n_antennas=4, taps=2, loading=9e-7), dict(n_antennas=4, taps=2, loading=1.0001), dict(n_antennas=4, taps=2, loading=-1e-4),
           dict(n_antennas=4, taps=2, loading=math.nan), dict(n_antennas=4, taps=2, loading=math.inf),
           dict(n_antennas=4, taps=2, loading=-math.inf),
           dict(n_antennas=2, taps=2, steering=[0, 0, 0, 0]), dict(n_antennas=3, taps=1, steering=[1, math.nan, 0]),
           dict(n_antennas=2, taps=2, steering=[1, 0, 0, complex(0, math.inf)]), dict(n_antennas=2, taps=1, steering=[complex(math.nan, 0), 1])]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_refuses(gm, cfg):
    from gnss_sdr_rs_amd import _lib
    assert SM.resolve(**cfg) is None, cfg
    with pytest.raises(_lib.GmError) as e:
        _plan(cfg)
    assert e.value.status == INVALID, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    Cfg = _lib.StapCfg
    ok = Cfg(4, 4, 0, 0.0, None, 0)
    n = C.c_uint64(77)
    plan = lambda cfg, so_far, n_in: L.gm_stap_plan(cfg, so_far, n_in, None, None, C.byref(n))
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, None, 1)), 0, 10) == INVALID and SM.resolve(4, 4, reserved=1) is None      # reserved
    assert plan(C.byref(Cfg(4, 4, 0, 0.0, None, 1 << 40)), 0, 10) == INVALID
    assert plan(None, 0, 10) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert SM.plan(SM.resolve(4, 4), so_far, n_in) is None
        assert plan(C.byref(ok), so_far, n_in) == INVALID
    assert n.value == 77                                           # nothing written
    assert L.gm_stap_plan(C.byref(ok), 0, 5000, None, None, None) == 0
    assert plan(C.byref(ok), 0, 5000) == 0 and n.value == 4096
    # the steering pointer is read: M = A L words of it, whatever lies behind
    s = np.array([0, 1j, 0, 0, math.nan], np.complex64)
    assert plan(C.byref(Cfg(2, 2, 0, 0.0, s.ctypes.data, 0)), 0, 10) == 0 and plan(C.byref(Cfg(5, 1, 0, 0.0, s.ctypes.data, 0)), 0, 10) == INVALID
    # a null handle is refused without a device
    assert L.gm_stap_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None) == INVALID
    assert L.gm_stap_process(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None, None, 0) == INVALID
    assert L.gm_stap_reset(None, 0) == INVALID and L.gm_stap_stats(None, None, None, None, None) == INVALID
    assert L.gm_stap_set_weights(None, None) == INVALID and L.gm_stap_capture(None, None, None, 0) == INVALID
    assert L.gm_stap_synchronize(None) == INVALID and L.gm_stap_destroy(None) == 0


# ---- the model's own facts -------------------------------------------------------------------------------------------------------------
def _interfered(rng, n, A, jn_db=30.0):
    x = rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))
    jam = 10.0 ** (jn_db / 20.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + jam[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    cw = np.sqrt(2.0) * 10.0 ** (jn_db / 20.0) * np.exp(2j * np.pi * 0.0617 * np.arange(n))
    return x + cw[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]


@pytest.mark.parametrize("A,L", [(2, 1), (2, 8), (3, 5), (4, 8), (8, 4)])
def test_the_models_own_facts(A, L):
    rng = np.random.default_rng(10 * A + L)
    B, M = 256, A * L
    x = _interfered(rng, 4 * B, A)
    x[B - (L - 1):2 * B] = 0.0                                     # an all-zero block, the samples its taps reach back to included
    s = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    for steering in (None, s):
        p = SM.resolve(A, L, B, 1e-4, steering)
        r = SM.run(p, x)
        assert r["R"].shape == (4, M, M) and r["w"].shape == (4, M) and r["y"].shape == (4 * B,)
        assert np.abs(r["R"] - np.conj(np.swapaxes(r["R"], 1, 2))).max() == 0.0          # Hermitian
        assert np.abs(np.einsum("bm,m->b", r["w"].conj(), p["s"]) - 1.0).max() <= 1e-12  # w^H s = 1
        assert np.abs(r["w"][1] - p["s"] / np.vdot(p["s"], p["s"]).real).max() == 0.0    # the all-zero block
        assert list(r["fallback"]) == [False, True, False, False] and not r["y"][B:2 * B].any()
        if steering is None:
            assert (SM.to_f32(r["w"])[:, 0].real == np.float32(1.0)).all() and np.abs(r["w"][:, 0].imag).max() <= 1e-12
        # the stacked sample is the definition's, with zeros before the stream's start
        z, xc = r["zb"].reshape(4 * B, M), SM.as_c128(x)
        for l in range(L):
            assert (z[l:, l * A:(l + 1) * A] == xc[:4 * B - l]).all() and not z[:l, l * A:(l + 1) * A].any()
    # a non-positive-definite or non-finite matrix takes the fallback and is counted
    p = SM.resolve(A, L, B)
    with np.errstate(all="ignore"):
        bad = np.stack([-np.eye(M), np.eye(M) * np.inf, np.eye(M)]).astype(np.complex128)
        w, fb = SM.weights(p, bad, want_fallback=True)
    assert list(fb) == [True, True, False] and (w[0] == p["s"]).all() and (w[1] == p["s"]).all() and np.isfinite(w.view(np.float64)).all()
    # the static mode is the plain combination, and device words handed in are used as they are
    wst = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    st = SM.run(p, x, static_w=wst)
    want = sum(np.concatenate([np.zeros(l), SM.as_c128(x)[:4 * B - l] @ wst[l * A:(l + 1) * A].astype(np.complex128).conj()]) for l in range(L))
    assert np.abs(st["y"] - want).max() <= 1e-12 * st["y_weight"].max()
    handed = SM.run(p, x, w=np.tile(wst, (4, 1)))
    assert (handed["y"] == st["y"]).all()
    # the cuts of the stream and a reset index only move the block edges; the samples before the index are zeros
    assert SM.blocks_of(p, x[:B - 1]).shape[0] == 0 and SM.blocks_of(p, x[:B - 1], input_index=(1 << 40) + 1).shape[0] == 1
    lead = SM.blocks_of(p, x, input_index=5 * B + 3)
    assert lead.shape[0] == 4 and not lead[0, :3].any() and (lead[0, 3:, :A] == x[:B - 3]).all()
    if L > 1:
        assert not lead[0, 3, A:].any() and (lead[0, 4, A:2 * A] == x[0]).all()


@pytest.mark.parametrize("A", range(2, 9))
def test_one_tap_is_the_nullers_model(A):
    rng = np.random.default_rng(A)
    B = 256
    x = _interfered(rng, 3 * B + 5, A)
    s = (rng.standard_normal(A) + 1j * rng.standard_normal(A)).astype(np.complex64)
    for steering in (None, s):
        for index in (0, 777):
            r = SM.run(SM.resolve(A, 1, B, 1e-3, steering), x, input_index=index)
            n = NM.run(NM.resolve(A, B, 1e-3, steering), x, input_index=index)
            assert (r["R"] == n["R"]).all() and (r["w"] == n["w"]).all() and (r["y"] == n["y"]).all()


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
_CELLS = {}


def cells(name, seed):
    """the scene of `seed` -> {"alone": cell of antenna 0, L: cell behind the model at L taps}; computed once and shared"""
    if (name, seed) not in _CELLS:
        x = SM.scene(name, seed)
        taps = {"S1": (1, 4, 8), "S2": (1, 4, 8), "S3": (1, 4), "clean": (4,)}[name]
        out = {"alone": SM.search(x[:, 0])}
        for L in taps:
            out[L] = SM.search(SM.nulled(x, L))
        _CELLS[(name, seed)] = out
    return _CELLS[(name, seed)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_the_signal_is_found_where_the_interferers_are_as_many_as_the_antennas(name, seed):
    """B = 1024, loading 1e-4, e_0.  numpy gave, peak-to-mean of the true worker's best cell, seeds 1 / 2 / 3:
    S1 (A = 2): antenna 0 3.2 / 3.5 / 3.3, L = 1 3.5 / 3.1 / 3.2 (wrong cells), L = 4 23.6 / 24.2 / 22.4, L = 8 28.8 / 30.1 / 28.5;
    S2 (A = 4): antenna 0 3.3 / 2.9 / 3.0, L = 1 3.2 / 2.8 / 3.1, L = 4 45.8 / 43.0 / 40.9, L = 8 56.6 / 53.4 / 49.5;
    S3 (A = 8): antenna 0 3.2 / 2.6 / 2.7, L = 1 3.4 / 3.1 / 3.2, L = 4 91.0 / 87.2 / 90.2 (all found cells at 700 in the 1 kHz bin)."""
    c = cells(name, seed)
    print("%s, seed %d: %s" % (name, seed, {k: (v[0], v[1], round(v[2], 1)) for k, v in c.items()}))
    assert c["alone"][2] < SM.DETECT and c[1][2] < SM.DETECT
    for L in (4, 8) if name != "S3" else (4,):
        assert SM.found(c[L]) and c[L][:2] == (2, 700) and c[L][2] > SM.DETECT, (L, c[L])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_taps_cost_little_where_nothing_is_there(seed):
    """the clean A = 4 scene through L = 4: numpy gave 28.6 / 26.1 / 29.2 (L = 1: 29.4 / 26.5 / 30.3)"""
    c = cells("clean", seed)
    print("clean, seed %d: %s" % (seed, c))
    assert SM.found(c[4]) and c[4][:2] == (2, 700) and c[4][2] > SM.DETECT
