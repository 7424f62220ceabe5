"""The adaptive spatial nuller on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number they
leave alone, gm_nuller_plan (host only, no device) against the float64 model of nuller_model.py, the model's own facts, and the scene
that motivates the entry: a 45 dB-Hz signal on a four-antenna line array under a white noise jammer, searched plainly at N = 2048."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import nuller_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_nuller_plan", "gm_nuller_create", "gm_nuller_destroy", "gm_nuller_reset", "gm_nuller_stats", "gm_nuller_synchronize",
           "gm_nuller_set_weights", "gm_nuller_capture", "gm_nuller_process_dev", "gm_nuller_process"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, nuller
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
    assert "class Nuller" in hpp
    assert "GmNullerCfg" in rust and "pub enum GmNuller" in rust
    assert "nuller_kernels.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_nuller" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert gnss_sdr_rs_amd.Nuller is nuller.Nuller
    for method in ("process", "process_dev", "set_weights", "capture", "reset", "stats", "synchronize"):
        assert hasattr(nuller.Nuller, method), method
    assert callable(nuller.plan)
    for words in ("gm_nuller_cfg", "total_out(T) = B * (T div B)", "d = 32, 16, 8, 4, 2, 1", "R = (W0 + W1) + (W2 + W3)", "a ASCENDING",
                  "w = s / (s^H s)", "Not built"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "nuller_kernels.hip" in _read("README.md") and "4.4f" in _read("DESIGN.md")
    stats = _read("profiles", "nuller_kernel_stats.txt")
    assert "nuller_kernel" in stats and "nuller_state_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: four 4-byte words, then the pointer
    assert C.sizeof(_lib.NullerCfg) == 24 and _lib.NullerCfg.reserved.offset == 12 and _lib.NullerCfg.steering.offset == 16
    body = re.search(r"pub struct GmNullerCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.NullerCfg._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} gm_nuller_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in _lib.NullerCfg._fields_]


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.ResamplerCfg) == 32 and C.sizeof(_lib.ExcisorCfg) == 32 and C.sizeof(_lib.DdcCfg) == 40    # no existing struct changed
    assert C.sizeof(_lib.ChannelizerCfg) == 40


# ---- gm_nuller_plan ------------------------------------------------------------------------------------------------------------------
def _plan(cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import nuller
    return nuller.plan(inputs_so_far=so_far, n_in=n_in, **cfg)


def test_plan_fills_in_the_defaults(gm):
    for A in range(2, 9):
        got = _plan(dict(n_antennas=A))
        assert got == dict(block=1024, loading=float(np.float32(1e-4)), n_out=0)
        p = NM.resolve(A)
        assert (p["A"], p["B"], p["loading"]) == (A, 1024, float(np.float32(1e-4))) and (p["s"] == np.eye(A)[0]).all()
    for B in NM.BLOCKS:
        assert _plan(dict(n_antennas=4, block=B, loading=1e-2)) == dict(block=B, loading=float(np.float32(1e-2)), n_out=0)
    for ld in (1e-6, 1.0):
        assert _plan(dict(n_antennas=2, loading=ld))["loading"] == NM.resolve(2, loading=ld)["loading"] == float(np.float32(ld))


@pytest.mark.parametrize("cfg", [dict(n_antennas=2, block=256), dict(n_antennas=4), dict(n_antennas=8, block=16384),
                                 dict(n_antennas=3, block=4096, steering=[1, 1j, -1])])
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, cfg):
    p = NM.resolve(**cfg)
    B = p["B"]
    for T in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, (1 << 32) + 5, 1 << 62):
        n = NM.total_out(p, T)
        assert n == B * (T // B) and _plan(cfg, 0, T)["n_out"] == n, T
    for so_far in (0, 1, B - 1, B, B + 1, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5 * B - 7):
        for n_in in (0, 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7):
            assert _plan(cfg, so_far, n_in)["n_out"] == NM.plan(p, so_far, n_in), (so_far, n_in)
    assert _plan(cfg, 1 << 62, 0)["n_out"] == 0
    so_far = total = 0
    for n_in in (1, B - 1, 7, B, 1000, 3001):                     # the sum of the calls is the count of the whole, whatever the cuts
        total += _plan(cfg, so_far, n_in)["n_out"]
        so_far += n_in
    assert total == NM.total_out(p, so_far)


REFUSED = [dict(n_antennas=0), dict(n_antennas=1), dict(n_antennas=9), dict(n_antennas=1 << 31),
           dict(n_antennas=4, block=128), dict(n_antennas=4, block=255), dict(n_antennas=4, block=1000), dict(n_antennas=4, block=1536),
           dict(n_antennas=4, block=32768), dict(n_antennas=4, block=1 << 31),
           dict(n_antennas=4, loading=9e-7), dict(n_antennas=4, loading=1.0001), dict(n_antennas=4, loading=-1e-4),
           dict(n_antennas=4, loading=math.nan), dict(n_antennas=4, loading=math.inf), dict(n_antennas=4, loading=-math.inf),
           dict(n_antennas=4, steering=[0, 0, 0, 0]), dict(n_antennas=3, steering=[1, math.nan, 0]),
           dict(n_antennas=3, steering=[1, 0, complex(0, math.inf)]), dict(n_antennas=2, steering=[complex(math.nan, 0), 1])]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_refuses(gm, cfg):
    from gnss_sdr_rs_amd import _lib
    assert NM.resolve(**cfg) is None, cfg
    with pytest.raises(_lib.GmError) as e:
        _plan(cfg)
    assert e.value.status == INVALID, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    Cfg = _lib.NullerCfg
    ok = Cfg(4, 0, 0.0, 0, None)
    n = C.c_uint64(77)
    plan = lambda cfg, so_far, n_in: L.gm_nuller_plan(cfg, so_far, n_in, None, None, C.byref(n))
    assert plan(C.byref(Cfg(4, 0, 0.0, 1, None)), 0, 10) == INVALID and NM.resolve(4, reserved=1) is None     # reserved
    assert plan(None, 0, 10) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert NM.plan(NM.resolve(4), so_far, n_in) is None
        assert plan(C.byref(ok), so_far, n_in) == INVALID
    assert n.value == 77                                           # nothing written
    assert L.gm_nuller_plan(C.byref(ok), 0, 5000, None, None, None) == 0
    assert plan(C.byref(ok), 0, 5000) == 0 and n.value == 4096
    # the steering pointer is read: two antennas of it where A = 2, whatever lies behind
    s = np.array([0, 1j, math.nan], np.complex64)
    assert plan(C.byref(Cfg(2, 0, 0.0, 0, s.ctypes.data)), 0, 10) == 0 and plan(C.byref(Cfg(3, 0, 0.0, 0, s.ctypes.data)), 0, 10) == INVALID
    # a null handle is refused without a device
    assert L.gm_nuller_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None) == INVALID
    assert L.gm_nuller_process(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None, None, None, 0) == INVALID
    assert L.gm_nuller_reset(None, 0) == INVALID and L.gm_nuller_stats(None, None, None, None) == INVALID
    assert L.gm_nuller_set_weights(None, None) == INVALID and L.gm_nuller_capture(None, None, None, 0) == INVALID
    assert L.gm_nuller_synchronize(None) == INVALID and L.gm_nuller_destroy(None) == 0


# ---- the model's own facts -----------------------------------------------------------------------------------------------------------
def _noise_and_jammer(rng, n, A, jn_db=30.0):
    x = rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))
    jam = 10.0 ** (jn_db / 20.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x + jam[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]


@pytest.mark.parametrize("A", range(2, 9))
def test_the_models_own_facts(A):
    rng = np.random.default_rng(A)
    B = 256
    x = _noise_and_jammer(rng, 3 * B, A)
    x[B:2 * B] = 0.0                                               # an all-zero block
    s = (rng.standard_normal(A) + 1j * rng.standard_normal(A)).astype(np.complex64)
    for steering in (None, s):
        p = NM.resolve(A, B, 1e-4, steering)
        r = NM.run(p, x)
        assert r["R"].shape == (3, A, A) and r["w"].shape == (3, A) and r["y"].shape == (3 * B,)
        assert np.abs(r["R"] - np.conj(np.swapaxes(r["R"], 1, 2))).max() == 0.0          # Hermitian
        assert np.abs(np.einsum("ba,a->b", r["w"].conj(), p["s"]) - 1.0).max() <= 1e-12  # w^H s = 1
        assert np.abs(r["w"][1] - p["s"] / np.vdot(p["s"], p["s"]).real).max() == 0.0    # the all-zero block
        assert not r["y"][B:2 * B].any()
        if steering is None:
            assert (NM.to_f32(r["w"])[:, 0].real == np.float32(1.0)).all() and np.abs(r["w"][:, 0].imag).max() <= 1e-12
        # the jammer is gone: the output power of a jammed block is near one antenna's noise power, far below the jammer's 2000
        assert np.mean(np.abs(r["y"][:B]) ** 2) < 40.0 * np.abs(r["w"][0]).max() ** 2
        # a permutation of the antennas permutes w
        perm = rng.permutation(A)
        q = NM.resolve(A, B, 1e-4, None if steering is None else s[perm])
        if steering is None:
            perm = np.concatenate([[0], 1 + rng.permutation(A - 1)])                     # e_0 stays the reference
        rp = NM.run(q, x[:, perm])
        assert np.abs(rp["w"] - r["w"][:, perm]).max() <= 1e-9 * np.abs(r["w"]).max()
        assert np.abs(rp["y"] - r["y"]).max() <= 1e-9 * r["y_weight"].max()
    # the static mode is the plain combination, and device words handed in are used as they are
    w = (rng.standard_normal(A) + 1j * rng.standard_normal(A)).astype(np.complex64)
    st = NM.run(NM.resolve(A, B), x, static_w=w)
    assert np.abs(st["y"] - x @ w.astype(np.complex128).conj()).max() <= 1e-12 * st["y_weight"].max()
    handed = NM.run(NM.resolve(A, B), x, w=np.tile(w, (3, 1)))
    assert (handed["y"] == st["y"]).all()
    # the cuts of the stream and a reset index only move the block edges
    p = NM.resolve(A, B)
    assert NM.blocks_of(p, x[:B - 1]).shape[0] == 0 and NM.blocks_of(p, x[:B - 1], input_index=(1 << 40) + 1).shape[0] == 1
    lead = NM.blocks_of(p, x, input_index=5 * B + 3)
    assert lead.shape[0] == 3 and not lead[0, :3].any() and (lead[0, 3:] == x[:B - 3]).all()


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene_run(seed):
    """every scene of `seed` through the model and a plain search -> {name: dict(x, y, alone, nulled)}; computed once and shared"""
    if seed not in _SCENES:
        out = {}
        for name, jn, int8 in NM.SCENES:
            x = NM.scene(seed, 4, jn, int8)
            y = NM.nulled(x, 1024, 1e-4)
            out[name] = dict(x=x, y=y, alone=NM.search(NM.as_c128(x)[:, 0]), nulled=NM.search(y))
        _SCENES[seed] = out
    return _SCENES[seed]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_jammed_signal_is_found_behind_the_nuller(seed):
    """A = 4, B = 1024, loading 1e-4, e_0.  numpy's default_rng(seed) gave, peak-to-mean of the true worker's best cell, seeds 1 / 2 / 3:
    clean, c32: antenna 0 alone 31.8 / 29.2 / 32.5, nulled 29.4 / 26.5 / 30.3 (all at 700 in the 1 kHz bin);
    J/N 40 dB, c32: alone 2.6 / 2.6 / 2.5 (wrong cell), nulled 36.0 / 36.3 / 38.2;
    J/N 50 dB, c32: alone 2.6 / 2.6 / 2.5 (wrong cell), nulled 37.2 / 37.4 / 39.0;
    J/N 30 dB, int8: alone 2.6 / 2.6 / 2.5 (wrong cell), nulled 9.8 / 10.2 / 14.3."""
    r = scene_run(seed)
    for name, jn, int8 in NM.SCENES:
        a, n = r[name]["alone"], r[name]["nulled"]
        print("seed %d, %s: antenna 0 alone %s, nulled %s" % (seed, name, (a[0], a[1], round(a[2], 1)), (n[0], n[1], round(n[2], 1))))
        assert NM.found(n) and n[2] > NM.DETECT, (name, n)
        if jn is None:
            assert NM.found(a) and a[2] > NM.DETECT, (name, a)
        else:
            assert a[2] < NM.DETECT, (name, a)


def test_a_steering_vector_towards_the_satellite_does_no_worse():
    """the c32 J/N 40 dB scene of seed 1 with s = the satellite's steering vector: the cell is right and the peak-to-mean is not below
    the e_0 value's (numpy's default_rng(1) gave 110.4 against 36.0: the antennas add up coherently towards the satellite)"""
    r = scene_run(1)["J/N 40 dB, c32"]
    y = NM.nulled(r["x"], 1024, 1e-4, NM.steer(NM.SAT_AZ, 4))
    steered = NM.search(y)
    print("e_0 %s, steered %s" % (r["nulled"], steered))
    assert NM.found(steered) and steered[2] >= r["nulled"][2] > NM.DETECT
