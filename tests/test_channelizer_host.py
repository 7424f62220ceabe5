"""The polyphase filter bank on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number they
leave alone, gm_channelizer_plan and gm_channelizer_design (host only, no device) against the float64 model of channelizer_model.py,
the GLONASS L1OF code, the two forms of the definition against each other, the prototype filter's gain, and the scene that motivates the
entry: three L1OF signals on three FDMA carriers of one 18 Msps int8 capture, separated into 2 Msps planes and searched plainly at
N = 2000."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import channelizer_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_channelizer_plan", "gm_channelizer_design", "gm_channelizer_create", "gm_channelizer_destroy", "gm_channelizer_reset",
           "gm_channelizer_taps", "gm_channelizer_stats", "gm_channelizer_synchronize", "gm_channelizer_process_dev",
           "gm_channelizer_process", "gm_glonass_code"]
INVALID = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, channelizer
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
        assert name in hpp or name in ("gm_channelizer_plan", "gm_channelizer_design"), name
    assert "class Channelizer" in hpp
    assert "GmChannelizerCfg" in rust and "pub enum GmChannelizer" in rust
    assert "channelizer_kernels.hip" in _read("gnss-sdr-rs_amd", "build.py")
    assert "launch_channelizer" in _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert gnss_sdr_rs_amd.Channelizer is channelizer.Channelizer
    for method in ("process", "process_dev", "reset", "taps", "stats", "synchronize"):
        assert hasattr(channelizer.Channelizer, method), method
    for fn in ("plan", "design", "glonass_channels", "glonass_code"):
        assert callable(getattr(channelizer, fn)), fn
    for words in ("gm_channelizer_cfg", "n0 = m D - (L/2 - 1)", "p ASCENDING", "total_out(A) = max(0, ceil((A - L/2) / D))"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "channelizer_kernels.hip" in _read("README.md") and "4.4e" in _read("DESIGN.md")
    stats = _read("profiles", "channelizer_kernel_stats.txt")
    assert "channelizer_kernel" in stats and "channelizer_state_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout: eight 4-byte words, then the pointer
    assert C.sizeof(_lib.ChannelizerCfg) == 40 and _lib.ChannelizerCfg.reserved.offset == 28 and _lib.ChannelizerCfg.out_channels.offset == 32
    body = re.search(r"pub struct GmChannelizerCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.ChannelizerCfg._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} gm_channelizer_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in _lib.ChannelizerCfg._fields_]


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.ResamplerCfg) == 32 and C.sizeof(_lib.ExcisorCfg) == 32 and C.sizeof(_lib.DdcCfg) == 40     # no existing struct changed


# ---- gm_channelizer_plan -----------------------------------------------------------------------------------------------------------
def _plan(cfg, so_far=0, n_in=0):
    from gnss_sdr_rs_amd import channelizer
    rest = {k: v for k, v in cfg.items() if k not in ("n_channels", "decim")}
    return channelizer.plan(cfg["n_channels"], cfg["decim"], so_far, n_in, **rest)


def test_plan_fills_in_the_defaults(gm):
    for M in (4, 8, 16, 32, 64):
        got = _plan(dict(n_channels=M, decim=M))
        assert got == dict(n_out_channels=M, taps_per_branch=16, n_taps=16 * M, n_out=0)
    got = _plan(dict(n_channels=32, decim=9, taps_per_branch=8, channels=[5, 0, 31]))
    assert (got["n_out_channels"], got["taps_per_branch"], got["n_taps"]) == (3, 8, 256)
    p = CM.resolve(32, 9)
    assert (p["P"], p["L"], p["cutoff"], p["beta"], p["channels"]) == (16, 512, 0.9, 8.0, list(range(32)))


@pytest.mark.parametrize("cfg", [dict(n_channels=4, decim=1, taps_per_branch=2), dict(n_channels=4, decim=3, taps_per_branch=4),
                                 dict(n_channels=16, decim=5, taps_per_branch=32), dict(n_channels=32, decim=9),
                                 dict(n_channels=64, decim=64, taps_per_branch=32), dict(n_channels=64, decim=18, channels=[63, 1])])
def test_plan_counts_what_the_model_counts_however_the_stream_is_cut(gm, cfg):
    p = CM.resolve(**cfg)
    half, D = p["L"] // 2, p["D"]
    for A in (0, half - 1, half, half + 1, half + D, half + D + 1, (1 << 32) + 5, 1 << 62):
        n = CM.total_out(p, A)
        assert n == max(0, -(-(A - half) // D)) and _plan(cfg, 0, A)["n_out"] == n, A
        if n:
            assert (n - 1) * D + half <= A - 1 < n * D + half                  # the last input of output n - 1 exists, that of n does not
    for so_far in (0, half - 1, half, half + 1, (1 << 32) - 3, (1 << 40) + 12345, (1 << 62) - 5000):
        for n_in in (0, 1, half - 1, half, half + 1, p["L"] - 1, 4095, 4113):
            assert _plan(cfg, so_far, n_in)["n_out"] == CM.plan(p, so_far, n_in), (so_far, n_in)
    assert _plan(cfg, 1 << 62, 0)["n_out"] == 0
    # the sum of the calls is the count of the whole, whatever the cuts
    so_far = total = 0
    for n_in in (1, half, 7, p["L"], 1000, 3001):
        total += _plan(cfg, so_far, n_in)["n_out"]
        so_far += n_in
    assert total == CM.total_out(p, so_far)


REFUSED = [dict(n_channels=0, decim=1), dict(n_channels=2, decim=1), dict(n_channels=12, decim=4), dict(n_channels=128, decim=4),
           dict(n_channels=32, decim=0), dict(n_channels=32, decim=33),
           dict(n_channels=32, decim=9, taps_per_branch=1), dict(n_channels=32, decim=9, taps_per_branch=33),
           dict(n_channels=32, decim=9, cutoff=-0.1), dict(n_channels=32, decim=9, cutoff=1.01), dict(n_channels=32, decim=9, cutoff=math.nan),
           dict(n_channels=32, decim=9, cutoff=math.inf),
           dict(n_channels=32, decim=9, kaiser_beta=-1.0), dict(n_channels=32, decim=9, kaiser_beta=20.5),
           dict(n_channels=32, decim=9, kaiser_beta=math.nan), dict(n_channels=32, decim=9, kaiser_beta=-math.inf),
           dict(n_channels=32, decim=9, blank_threshold=-1.0), dict(n_channels=32, decim=9, blank_threshold=math.nan),
           dict(n_channels=32, decim=9, blank_threshold=math.inf),
           dict(n_channels=32, decim=9, channels=[]), dict(n_channels=32, decim=9, channels=[3, 4, 3]),
           dict(n_channels=32, decim=9, channels=[32]), dict(n_channels=4, decim=2, channels=[0, 1, 2, 3, 0]),
           dict(n_channels=8, decim=2, channels=[1 << 31])]


@pytest.mark.parametrize("cfg", REFUSED)
def test_plan_and_design_refuse(gm, cfg):
    from gnss_sdr_rs_amd import _lib, channelizer
    assert CM.resolve(**cfg) is None, cfg
    design_cfg = {k: v for k, v in cfg.items() if k != "channels"}
    calls = [lambda: _plan(cfg)]
    if "channels" not in cfg:
        calls.append(lambda: channelizer.design(**design_cfg))
    for call in calls:
        with pytest.raises(_lib.GmError) as e:
            call()
        assert e.value.status == INVALID, cfg


def test_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    Cfg = _lib.ChannelizerCfg
    ok = Cfg(32, 9, 0, 0.0, 0.0, 0.0, 0, 0, None)
    n = C.c_uint64(77)
    plan = lambda cfg, so_far, n_in: L.gm_channelizer_plan(cfg, so_far, n_in, None, None, None, C.byref(n))
    assert plan(C.byref(Cfg(32, 9, 0, 0.0, 0.0, 0.0, 0, 1, None)), 0, 10) == INVALID          # reserved
    assert plan(None, 0, 10) == INVALID
    lst = (C.c_uint32 * 2)(3, 4)
    assert plan(C.byref(Cfg(32, 9, 0, 0.0, 0.0, 0.0, 2, 0, None)), 0, 10) == INVALID          # a count without a list
    assert plan(C.byref(Cfg(32, 9, 0, 0.0, 0.0, 0.0, 0, 0, C.cast(lst, C.POINTER(C.c_uint32)))), 0, 10) == INVALID     # a list without a count
    assert plan(C.byref(Cfg(32, 9, 0, 0.0, 0.0, 0.0, 33, 0, C.cast(lst, C.POINTER(C.c_uint32)))), 0, 10) == INVALID
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        assert CM.plan(CM.resolve(32, 9), so_far, n_in) is None
        assert plan(C.byref(ok), so_far, n_in) == INVALID
    assert n.value == 77                                                                      # nothing written
    assert L.gm_channelizer_plan(C.byref(ok), 0, 1000, None, None, None, None) == 0
    assert plan(C.byref(Cfg(32, 9, 0, 0.0, 0.0, 0.0, 2, 0, C.cast(lst, C.POINTER(C.c_uint32)))), 0, 1000) == 0 and n.value == CM.plan(CM.resolve(32, 9), 0, 1000)
    assert L.gm_channelizer_design(C.byref(ok), None) == INVALID
    # a null handle is refused without a device
    assert L.gm_channelizer_process_dev(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, 8, None, None) == INVALID
    assert L.gm_channelizer_process(None, C.c_void_p(4096), 0, 8, C.c_void_p(1 << 20), 8, None) == INVALID
    assert L.gm_channelizer_reset(None, 0) == INVALID and L.gm_channelizer_stats(None, None, None, None) == INVALID
    assert L.gm_channelizer_taps(None, None) == INVALID and L.gm_channelizer_synchronize(None) == INVALID
    assert L.gm_channelizer_destroy(None) == 0
    assert L.gm_glonass_code(None) == INVALID


# ---- gm_channelizer_design ---------------------------------------------------------------------------------------------------------
DESIGNS = [dict(n_channels=4, decim=1, taps_per_branch=2), dict(n_channels=4, decim=3, taps_per_branch=4), dict(n_channels=8, decim=4),
           dict(n_channels=8, decim=8, taps_per_branch=8), dict(n_channels=16, decim=5, taps_per_branch=32), dict(n_channels=32, decim=9),
           dict(n_channels=32, decim=16, cutoff=1.0, kaiser_beta=20.0), dict(n_channels=64, decim=18, cutoff=0.5, kaiser_beta=0.5),
           dict(n_channels=64, decim=64, taps_per_branch=32)]


@pytest.mark.parametrize("cfg", DESIGNS)
def test_design_gives_the_models_words_bit_for_bit(gm, cfg):
    """the model evaluates the definition with the library's float64 operations in the library's order, so the float32 words are
    equal; numpy's own sinc and i0 give float64 values within 1e-15 of them; the words sum to 1 within L 2^-25"""
    from gnss_sdr_rs_amd import channelizer
    p = CM.resolve(**cfg)
    want = CM.design(p)
    got = channelizer.design(**cfg)
    assert got.shape == (p["L"],) and got.dtype == np.float32
    assert (got.view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()
    assert np.abs(want - CM.design_numpy(p)).max() <= 1e-15
    assert abs(got.astype(np.float64).sum() - 1.0) <= p["L"] * 2.0 ** -25
    assert want[p["L"] // 2 - 1] == want.max()                                    # centred on tap L/2 - 1
    assert np.abs(want[:p["L"] - 1] - want[:p["L"] - 1][::-1]).max() <= 1e-15     # and symmetric about it


# ---- the GLONASS L1OF code ---------------------------------------------------------------------------------------------------------
def test_the_glonass_code(gm):
    from gnss_sdr_rs_amd import channelizer
    chips = channelizer.glonass_code()
    assert chips.shape == (1, 511) and chips.dtype == np.int8 and set(np.unique(chips)) == {-1, 1}
    logic = (1 - chips[0].astype(np.int64)) // 2                     # +1 stands for logic 0
    assert "".join(str(v) for v in logic[:24]) == "111111100000111101111100"
    assert int(logic.sum()) == 256
    assert (logic == CM.glonass_logic()).all() and (chips[0] == CM.glonass_chips()).all()
    # the period is exactly 511: the register's next 511 outputs repeat, and no shorter shift maps the sequence onto itself;
    # the cyclic autocorrelation of a maximal-length sequence is -1 at every non-zero shift
    c = chips[0].astype(np.int64)
    corr = np.array([int((c * np.roll(c, s)).sum()) for s in range(511)])
    assert corr[0] == 511 and (corr[1:] == -1).all()
    s = [1] * 9
    states = set()
    for _ in range(511):
        states.add(tuple(s))
        s = [s[4] ^ s[8]] + s[:8]
    assert len(states) == 511 and s == [1] * 9
    assert channelizer.glonass_channels(32) == [25, 26, 27, 28, 29, 30, 31, 0, 1, 2, 3, 4, 5, 6]
    assert channelizer.glonass_channels(16) == [9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6]


# ---- the two forms of the definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 8, 16, 32, 64])
def test_the_polyphase_form_is_the_direct_sum(M):
    """both forms in float64 on the same noise, in blocks, from an odd absolute index: within 1e-11 of sum |g| |x| — for D = 1, a D
    that does not divide M, and D = M, with shuffled channel lists"""
    rng = np.random.default_rng(M)
    for D in (1, M - 1, M):
        channels = [int(k) for k in rng.permutation(M)[:max(2, M // 2)]]
        p = CM.resolve(M, D, channels=channels, taps_per_branch=4)
        g = CM.design(p)
        n = 3 * p["L"] + 37
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        index = (1 << 40) + 12345
        a, wa, ma = CM.run(p, g, x, blocks=101, input_index=index, form="direct")
        b, wb, mb = CM.run(p, g, x, blocks=None, input_index=index, form="polyphase")
        assert a.shape == b.shape == (len(channels), CM.plan(p, index, n)) and a.shape[1] > 0
        assert (wa == wb).all()
        worst = float((np.abs(a - b) / wa[None, :]).max())
        assert worst <= 1e-11, (M, D, worst)
        # a plane's values do not depend on which other channels are listed
        one = CM.resolve(M, D, channels=channels[1:2], taps_per_branch=4)
        c, _, _ = CM.run(one, g, x, input_index=index)
        assert (c[0] == b[1]).all()


def test_a_tone_on_a_channel_centre_comes_out_as_dc():
    """channel k is centred at k fs / M and its phase runs on the absolute input index: a unit tone exp(j 2 pi k n / M) gives y_k[m] = 1
    (the filter's DC gain; within the float32 rounding of the 16 distinct input words) and nothing in the channels two away"""
    M, D = 16, 5
    p = CM.resolve(M, D)
    g = CM.design(p)
    n = 4 * p["L"]
    k = 11
    x = np.exp(2j * np.pi * k * np.arange(n) / M)
    y, _, _ = CM.run(p, g, x)
    settled = slice(p["L"] // D + 1, None)
    assert np.abs(y[k] - 1.0)[settled].max() <= 2.0 ** -23
    assert np.abs(y[(k + 2) % M])[settled].max() <= 1e-4 and np.abs(y[(k - 2) % M])[settled].max() <= 1e-4


# ---- the prototype filter's gain ---------------------------------------------------------------------------------------------------
def test_the_filter_passes_and_stops():
    """in units of the output Nyquist frequency fs / (2 D): flat within 0.01 dB up to 0.75, -6.02 dB at the cutoff 0.9, at most -80 dB
    from 1.0 on (what folds back into the plane), at P = 16; P = 8 reaches that only from 1.1 on"""
    for M, D in ((32, 9), (64, 18)):
        p = CM.resolve(M, D)
        g = CM.design(p).astype(np.float32)
        ny = 0.5 / D
        gain = lambda f: CM.tone_gain_db(p, g, f * ny)
        flat = max(abs(gain(f)) for f in np.linspace(0.0, 0.75, 61))
        stop = max(gain(f) for f in np.concatenate([np.linspace(1.0, 2.0, 201), np.linspace(2.0, D, 301)]))
        far = max(gain(f) for f in np.linspace(1.1, D, 400))
        print("(%d, %d, 16): flat within %.4f dB to 0.75, %.2f dB at 0.9, %.1f dB at 1.0, at most %.1f dB from 1.0 on, %.1f dB from 1.1 on"
              % (M, D, flat, gain(0.9), gain(1.0), stop, far))
        assert flat <= 0.01 and abs(gain(0.9) + 6.02) <= 0.01 and stop <= -80.0 and far <= -88.0
    p = CM.resolve(32, 9, taps_per_branch=8)
    g = CM.design(p).astype(np.float32)
    at1, at11 = CM.tone_gain_db(p, g, 0.5 / 9), CM.tone_gain_db(p, g, 1.1 * 0.5 / 9)
    print("(32, 9, 8): %.1f dB at 1.0, %.1f dB at 1.1" % (at1, at11))
    assert abs(at1 + 25.6) <= 0.1 and abs(at11 + 83.9) <= 0.1


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene_run(seed):
    """the scene of `seed` through the model (the library's filter words, float32) and a plain search of the three occupied planes and
    the empty one -> dict(x, p, g, y [4][n], cells {channel: (bin, code phase, peak-to-mean)}); computed once and shared"""
    if seed not in _SCENES:
        channels = [s["channel"] for s in CM.SIGNALS] + [CM.EMPTY]
        p = CM.resolve(CM.M, CM.D, channels=channels, taps_per_branch=CM.P)
        g = CM.design(p).astype(np.float32)
        x = CM.scene(seed)
        y, _, m = CM.run(p, g, x, blocks=27000)
        assert y.shape == (4, CM.total_out(p, CM.N_IN)) and y.shape[1] >= CM.M_SEARCH * CM.N
        _SCENES[seed] = dict(x=x, p=p, g=g, y=y, cells={k: CM.search(y[i]) for i, k in enumerate(channels)})
    return _SCENES[seed]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_three_carriers_are_found_in_their_planes(seed):
    """numpy's default_rng(seed) gave, seeds 1 / 2 / 3: channel 3 (700, +1 kHz) 20.5 / 22.5 / 25.5; channel 4 (100, -500 Hz) 388 / 384 /
    377; channel 27 (1400, 0 Hz) 15.4 / 16.0 / 15.5; the empty channel 10 2.4 to 2.7"""
    r = scene_run(seed)
    print("seed %d: %s" % (seed, {k: (b, ph, round(ratio, 1)) for k, (b, ph, ratio) in r["cells"].items()}))
    for k, (phase, b) in CM.EXPECTED.items():
        got = r["cells"][k]
        assert (got[1], got[0]) == (phase, b) and got[2] > CM.DETECT, (k, got)
    assert r["cells"][CM.EMPTY][2] < CM.DETECT
    # without the bank the strong neighbour hides the weak carriers: the 60 dB-Hz signal is 562.5 kHz away from channel 3's, and a
    # plane's stop band keeps it 84 dB down
    assert r["cells"][4][2] > 10 * r["cells"][3][2]
