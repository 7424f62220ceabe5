"""The excisor's block-adapt mode on the CPU: the additive entries in every layer (this test fails without the feature), the ABI number
they leave alone, gm_excisor_block_plan (host only, no device) against excise_block_model.py with every refusal, the portable
selection rule of csrc/excise_core.h lane by lane under g++, and the scenes that motivate the mode: a CW 30 or 40 dB above the noise
that sweeps over 1.6 MHz during the dwell, which the static gains cannot follow and the per-block rule removes."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import excise_block_model as BM
import excise_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_excisor_block_plan", "gm_excisor_set_block_adapt", "gm_excisor_block_stats", "gm_excisor_block_capture"]
INVALID = -1
SEEDS = (1, 2, 3)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, excise
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
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
        assert name in hpp or name == "gm_excisor_block_plan", name
    for method in ("set_block_adapt", "block_stats", "block_capture"):
        assert hasattr(excise.Excisor, method), method
        assert method in hpp, method
    assert callable(excise.block_plan)
    assert "want_blocks" in excise.Excisor.process.__code__.co_varnames
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "block_adapt" in internal and "launch_excise" in internal and "bstat" in internal
    core = _read("gnss-sdr-rs_amd", "csrc", "excise_core.h")
    assert "ex_sel_step" in core and "ex_zeroed" in core
    for words in ("gm_excisor_block_cfg", "Block-adapt mode", "with the low 16 bits of its f32 word cleared", "count(p < v) <= rank",
                  "flag[k] = p[k] > factor * med_b", "Y_b[k] = (g[k] * m_b[k]) * X_b[k]", "block 0 is never counted",
                  "GM_ERR_OUT_OF_RANGE before anything runs"):
        assert words in header, words
    # the ring entries say that they pick the mode up
    for entry in ("gm_frontend_write_ring_conditioned", "gm_ddc_write_ring"):
        comment = header[:header.index("int %s(" % entry)].rsplit("/*", 1)[1]
        assert "gm_excisor_set_block_adapt" in comment, entry
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert all(name in _read(doc) for name in ENTRIES), doc
    assert "Per-block adaptive excision" in _read("README.md") and "4.4d" in _read("DESIGN.md")
    stats = _read("profiles", "excise_kernel_stats.txt")
    assert "block-adapt" in stats
    # the struct layouts: eight 4-byte words
    assert C.sizeof(_lib.ExcisorBlockCfg) == 32 and _lib.ExcisorBlockCfg.guard_bins.offset == 4 and _lib.ExcisorBlockCfg.reserved.offset == 8
    body = re.search(r"pub struct GmExcisorBlockCfg\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in _lib.ExcisorBlockCfg._fields_]
    assert re.search(r"pub\s+reserved\s*:\s*\[u32;\s*6\]", body)
    cstruct = re.search(r"typedef struct \{([^}]*)\}\s*gm_excisor_block_cfg;", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", cstruct, flags=re.S)) == [f[0] for f in _lib.ExcisorBlockCfg._fields_]


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.ExcisorCfg) == 32 and C.sizeof(_lib.ResamplerCfg) == 32                # no existing struct changed


# ---- gm_excisor_block_plan ---------------------------------------------------------------------------------------------------------
def test_block_plan_fills_in_the_defaults(gm):
    from gnss_sdr_rs_amd import excise
    assert excise.block_plan() == dict(threshold_factor=16.0, guard_bins=0)
    assert BM.resolve() == dict(factor=16.0, guard=0)
    for factor, guard in ((1.5, 16), (6.0, 2), (math.inf, 0), (1.0000001, 7)):
        want = BM.resolve(factor, guard)
        assert excise.block_plan(factor, guard) == dict(threshold_factor=want["factor"], guard_bins=want["guard"])


REFUSED = [dict(threshold_factor=1.0), dict(threshold_factor=0.5), dict(threshold_factor=-16.0), dict(threshold_factor=math.nan),
           dict(threshold_factor=-math.inf), dict(guard_bins=17), dict(guard_bins=1 << 31)]


@pytest.mark.parametrize("cfg", REFUSED)
def test_block_plan_refuses(gm, cfg):
    from gnss_sdr_rs_amd import _lib, excise
    assert BM.resolve(**cfg) is None, cfg
    with pytest.raises(_lib.GmError) as e:
        excise.block_plan(**cfg)
    assert e.value.status == INVALID, cfg


def test_block_plan_refuses_the_rest_and_takes_null_outputs(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    f, g = C.c_float(77.0), C.c_uint32(77)
    for k in range(6):
        res = [0] * 6
        res[k] = 1
        assert BM.resolve(reserved=res) is None
        bad = _lib.ExcisorBlockCfg(16.0, 2, (C.c_uint32 * 6)(*res))
        assert L.gm_excisor_block_plan(C.byref(bad), C.byref(f), C.byref(g)) == INVALID
    assert L.gm_excisor_block_plan(None, C.byref(f), C.byref(g)) == INVALID
    assert (f.value, g.value) == (77.0, 77)                                                       # nothing written
    ok = _lib.ExcisorBlockCfg(0.0, 3)
    assert L.gm_excisor_block_plan(C.byref(ok), None, None) == 0
    assert L.gm_excisor_block_plan(C.byref(ok), C.byref(f), None) == 0 and f.value == 16.0
    assert L.gm_excisor_block_plan(C.byref(ok), None, C.byref(g)) == 0 and g.value == 3
    # a null handle is refused without a device
    assert L.gm_excisor_set_block_adapt(None, C.byref(ok)) == INVALID and L.gm_excisor_set_block_adapt(None, None) == INVALID
    assert L.gm_excisor_block_stats(None, None, None, None, None) == INVALID
    assert L.gm_excisor_block_capture(None, None, None, 0) == INVALID


# ---- the model's own rule ----------------------------------------------------------------------------------------------------------
def test_the_truncated_median_and_the_guard():
    p = np.ones(256, np.float32)
    p[0] = 100.0
    p[200] = 16.0                                                    # exactly factor * median: not flagged (strictly greater)
    med, flag, mask = BM.decide(p, 16.0, 2)
    assert med == 1.0 and flag.sum() == 1 and (np.flatnonzero(mask == 0) == [0, 1, 2, 254, 255]).all() and mask.dtype == np.uint8
    # the truncation keeps the sign, the exponent and 7 mantissa bits: 1 + 2^-7 + 2^-8 + 2^-20 becomes 1 + 2^-7, less than 2^-7 below
    v = np.float32(1.0 + 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -20)
    med, _, _ = BM.decide(np.full(256, v, np.float32), 16.0, 0)
    assert med == np.float32(1.0 + 2.0 ** -7) and 2.0 ** -9 < (v - med) / v < 2.0 ** -7
    # all zeros: med = 0 and nothing is flagged; rows are decided independently
    P = np.stack([np.zeros(256, np.float32), p])
    med, flag, mask = BM.decide(P, 16.0, 16)
    assert med[0] == 0 and not flag[0].any() and mask[0].all() and (mask[1] == 0).sum() == 33
    c = BM.count([flag], [mask])
    assert c == dict(blocks=1, blocks_flagged=1, bins_flagged=1, bins_zeroed=33)                 # the first block of a call is not counted


def test_the_selection_rule_lane_by_lane_on_the_cpu():
    """tests/cpu/test_excise_block.cpp: the portable rule of csrc/excise_core.h the way the kernel's lanes run it (15 counting rounds,
    the flags as a bit image, the guard from three words of it) against a sort and a naive circular window"""
    exe = os.path.join(tempfile.mkdtemp(prefix="gm_excise_block_"), "test_excise_block")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "test_excise_block.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    for words in ("all zeros", "ties at the rank", "denormals", "one infinity", "B=  256", "B= 4096", "\n0 failures"):
        assert words in r.stdout, words


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene_run(seed):
    """The scenes of one noise seed through the models: computed once, shared and left unchanged."""
    if seed in _SCENES:
        return _SCENES[seed]
    r = {}
    clean = EM.scene(seed)
    r["clean"] = EM.search(clean)
    y, masks, m = BM.excise_blocks(clean)
    plain = EM.process(EM.resolve(1024), clean)[:EM.DWELL]
    r["clean_blocks"], r["clean_masks"], r["clean_counters"] = EM.search(y), masks, m.counters
    r["clean_y"], r["clean_plain"] = y, plain.astype(np.complex64)
    p4 = EM.resolve(1024, 2, 4.0)
    for jn in (30.0, 40.0):
        x = BM.sweep_scene(seed, jn)
        tag = "%d" % jn
        r["jammed" + tag] = EM.search(x)
        r["static_whole" + tag] = (EM.search(EM.excise(x)[0]), EM.excise(x)[1])
        _, _, g = EM.detect(EM.psd(p4, x[:4 * EM.N]), 4.0, 2)
        r["static_four" + tag] = (EM.search(EM.process(p4, x, g)[:EM.DWELL].astype(np.complex64)), int((g == 0).sum()))
        y, masks, m = BM.excise_blocks(x)
        r["blocks" + tag] = (EM.search(y), (masks == 0).sum(axis=1), m.counters)
    y, masks, m = BM.excise_blocks(EM.scene(seed, 30.0))
    r["fixed_cw"] = (EM.search(y), EM.search(EM.excise(EM.scene(seed, 30.0))[0]))
    x = BM.hop_scene(seed)
    y, masks, m = BM.excise_blocks(x)
    r["hopper"] = (EM.search(y), EM.search(EM.excise(x)[0]), EM.search(x))
    _SCENES[seed] = r
    return r


@pytest.mark.parametrize("seed", SEEDS)
def test_the_per_block_rule_brings_a_swept_search_back(seed):
    """excise_model's scene (fs = 2.048 MHz, N = 2048, K = 1, M = 10, 45 dB-Hz, the true cell bin 2 (1 kHz), code phase 700) with its CW
    replaced by one that sweeps linearly from -800 kHz to +800 kHz over the 11 periods of N_IN; B = 1024, guard 2.  Peak-to-mean of the
    true worker's best cell (code phase), measured on seeds 1, 2, 3:
      clean                                          37.2 (700), 30.0 (700), 29.2 (700)
      + sweep, J/N 30 dB, not excised                2.4 (942), 2.4 (941), 2.4 (941): missed
      static: adapt on the whole dwell (factor 4)    2.4, 2.4, 2.4: missed (0 bins flagged: the sweep lifts the median everywhere)
      static: adapt on the first 4 periods           2.9, 2.9, 2.9: missed (300 bins zeroed)
      per-block rule, factor 16                      34.0 (700), 28.0 (700), 26.9 (700): 0.91, 0.93, 0.92 of clean;
                                                     51 bins zeroed a block on average, at most 101
      the same at J/N 40 dB                          30.4 (700), 24.6 (700), 23.9 (700); about 62 a block, at most 116
      fixed CW of excise_model at 30 dB, per block   35.0 (700), 28.1 (700), 26.6 (700)   (static adapt: 32.3, 25.6, 24.8)
      clean scene through the per-block rule         37.2, 30.0, 29.2: 1 of 43 blocks flagged on seed 1, none on seeds 2 and 3
      hopper (a new frequency every 700 samples)     5.4 (700), 4.9 (700), 4.6 (700)   (static adapt and no excision: missed)"""
    r = scene_run(seed)
    print(seed, {k: v for k, v in r.items() if k not in ("clean_masks", "clean_y", "clean_plain")})
    assert EM.found(r["clean"]) and r["clean"][2] >= 20.0
    for tag in ("30", "40"):
        cell, zeroed, counters = r["blocks" + tag]
        assert EM.found(cell), tag                                                               # found at (bin 2, 700)
        assert not EM.found(r["jammed" + tag])                                                  # missed without excision
        assert not EM.found(r["static_whole" + tag][0]) and not EM.found(r["static_four" + tag][0])       # and with both static adapts
        assert counters["blocks_flagged"] == counters["blocks"] == 43 and zeroed.max() <= 160
    assert r["blocks30"][0][2] >= 0.8 * r["clean"][2]
    assert EM.found(r["fixed_cw"][0]) and EM.found(r["fixed_cw"][1]) and r["fixed_cw"][0][2] >= r["fixed_cw"][1][2]
    assert EM.found(r["hopper"][0]) and not EM.found(r["hopper"][1]) and not EM.found(r["hopper"][2])


@pytest.mark.parametrize("seed", SEEDS)
def test_the_clean_scene_passes_the_per_block_rule_unchanged(seed):
    """factor 16 on noise alone: a noise-only bin of one block is exponentially distributed, P(p > f median) = 2^-f, so
    2^-16 * 1024 = 1.6 % of clean blocks of B = 1024 carry a flag by noise alone; measured 1 of 43, 0 and 0 blocks on the three seeds.
    At most 5 % of them may: a condition on the chosen inputs, which these seeds meet."""
    r = scene_run(seed)
    c, masks = r["clean_counters"], r["clean_masks"]
    print(seed, c)
    assert c["blocks"] == 43 and c["blocks_flagged"] <= 0.05 * c["blocks"]
    # the words are unchanged in blocks with no flag: an output whose two blocks carry no flag is the unexcised one's
    H = 512
    y, plain = r["clean_y"], r["clean_plain"]
    flagged = (masks == 0).any(axis=1)
    untouched = np.repeat(~(flagged[:-1] | flagged[1:]), H)[:EM.DWELL]
    assert untouched.sum() >= 0.9 * EM.DWELL and (y[untouched] == plain[untouched]).all()
    assert abs(r["clean_blocks"][2] / r["clean"][2] - 1.0) <= 0.01 and EM.found(r["clean_blocks"])
