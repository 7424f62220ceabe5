"""The float64 model of gm_acq_finer_doppler (acq_fine_model.py) and the scenes of test_gpu_fine_doppler.py, checked without a GPU.

1. The model against the oracle (the float32 restatement of the legacy) where the oracle is cheap: 2^16 and 2^17.
2. Every scene the GPU test refines has a peak where it was placed, GAP clear of the next value, and does not clip in int8: an exact
   index comparison on the GPU then cannot fail on a tie.  A scene that fails here gets another seed in acq_fine_model.SEEDS.
3. The host's factor rule restated: the nine reachable (N1, N2) pairs, their row tiles, and a geometry for each.
4. The header states the supported range.
"""
import os
import re

import numpy as np
import pytest

import acq_fine_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def codes(gm):
    from gnss_sdr_rs_amd import acquisition as A
    return np.asarray(A.ca_code_table(), np.int8)


@pytest.mark.parametrize("g", [0, 1])
def test_model_against_the_oracle(oracle, codes, g):
    """c32 scenes at 2^16 and 2^17: same fft_size, same peak index, |X| at the peak within 1e-4 relative (the tolerance the oracle
    tests of the entry use: the oracle transforms in float32), the same float32 frequency word"""
    N, periods, fmt, fs, sats, _ = FM.case(g, "c32")
    x = FM.case_scene(g, codes, "c32")
    for s in sats:
        o = oracle.finer_doppler(x, s["cp"], codes[s["row"]], fs, (periods - 1) * N)
        m = FM.fine_model(FM.as_complex(x), s["cp"], codes[s["row"]], 1.023e6, fs, periods, N)
        assert m["fft_size"] == o["fft_size"] == FM.fft_size_of(N, periods)
        assert m["peak_index"] == o["peak_index"], (g, s, m["peak_index"], o)
        assert abs(m["mag"][m["peak_index"]] - o["peak_mag"]) <= 1e-4 * o["peak_mag"], (g, s, m["mag"][m["peak_index"]], o)
        assert np.float32(o["freq_hz"]).view(np.uint32) == m["freq_hz"].view(np.uint32), (g, s, m["freq_hz"], o)
        assert o["upper_half"] == (s["idx"] > m["fft_size"] // 2)


def test_frequency_rule_at_the_half():
    """one_side in float32: 2^23 at n = 2^24 (the sum 2^24 + 1 rounds back), n / 2 + 1 below"""
    n, fs = 1 << 24, 16.384e6
    assert FM.freq_rule((1 << 23) + 1, n, fs) < 0 and FM.freq_rule(1 << 23, n, fs) > 0
    n = 1 << 20
    assert FM.freq_rule(n // 2 + 2, n, fs) < 0 and FM.freq_rule(n // 2 + 1, n, fs) > 0
    assert FM.freq_rule(n - 1, n, fs) == -FM.freq_rule(1, n, fs)


def _check_scene(x, fmt, sats, chips_of, code_rate, fs, periods, N, what):
    raw = np.asarray(x)
    if raw.dtype == np.int8:
        assert int(np.abs(raw.astype(np.int16)).max()) < 127, what        # nothing clipped
    xc = FM.as_complex(x)
    for s in sats:
        m = FM.fine_model(xc, s["cp"], chips_of(s), code_rate, fs, periods, N)
        n, k = m["fft_size"], m["peak_index"]
        if fmt == "real":
            assert k in (s["idx"], n - s["idx"]), (what, s, k)
            gap = FM.real_gap(m["mag"], k)
        else:
            assert k == s["idx"], (what, s, k)
            gap = m["gap"]
        assert gap > FM.GAP, (what, s, gap)


@pytest.mark.parametrize("g", range(len(FM.geometries())))
def test_scenes_have_one_clear_peak(codes, g):
    """Every geometry, satellite and format: the model's peak is the bin the satellite was placed on, more than GAP = 1e-3 clear of
    the next value (a tone on a bin centre with size_use / p2 >= 1/2 leaves its neighbours 0.6 % below it).  For the real format the
    maximum is the pair k, n - k and the check is on the next distinct value."""
    for fmt in FM.FORMATS:
        N, periods, _, fs, sats, _ = FM.case(g, fmt)
        x = FM.case_scene(g, codes, fmt)
        _check_scene(x, fmt, sats, lambda s: codes[s["row"]], 1.023e6, fs, periods, N, (g, fmt))


def test_placements_reach_the_rows_they_name():
    for g in range(len(FM.geometries())):
        for fmt in FM.FORMATS:
            N, periods, _, _, sats, _ = FM.case(g, fmt)
            n = FM.fft_size_of(N, periods)
            N1, N2, RT = FM.FACTOR_TABLE[n]
            one_side = n // 2 if n == 1 << 24 else n // 2 + 1
            a, b = sats[0], sats[1]
            assert a["idx"] % N1 == N1 - 1 and (a["idx"] % N1) % RT == RT - 1 and a["idx"] // N1 < 8
            assert (b["idx"] % N1) % RT == 0 and RT <= b["idx"] % N1 < N1 - RT and b["idx"] > one_side and b["idx"] // N1 >= N2 // 2
            assert len(sats) == (2 if n >= 1 << 23 else 3)
            if len(sats) == 3:
                c = sats[2]
                assert c["idx"] % N1 == 1 and (c["idx"] < N1 or fmt == "real")
            cps = [s["cp"] for s in sats]
            assert 0 in cps and N - 1 in cps and len(set(cps)) == len(cps)
            assert len(set(s["row"] for s in sats)) == len(sats)
    # the formats rotate: each at a small (<= 2^18), a middle and a large (>= 2^22) size
    for fmt in FM.FORMATS:
        sizes = [FM.fft_size_of(*FM.geometries()[g]) for g in range(len(FM.geometries())) if FM.case(g)[2] == fmt]
        assert min(sizes) <= 1 << 18 and max(sizes) >= 1 << 22 and any(1 << 18 < v < 1 << 22 for v in sizes), (fmt, sizes)


def test_custom_code_scene():
    N, periods, fmt, fs, code_rate, ccodes, sats, _ = FM.custom_case()
    assert ccodes.shape[1] != 1023 and code_rate != 1.023e6 and FM.fft_size_of(N, periods) == 1 << 18
    # the float32 chip index is not the float64 one on this geometry: the model keeps the float32 rule
    m = np.arange((periods - 1) * N)
    f64 = np.floor(m.astype(np.float64) * code_rate / fs).astype(np.int64) % ccodes.shape[1]
    assert (FM.chip_index(m, code_rate, fs, ccodes.shape[1]) != f64).any()
    _check_scene(FM.custom_scene(), fmt, sats, lambda s: ccodes[s["row"]], code_rate, fs, periods, N, "custom")


def test_edge_scene(codes):
    """The several-passes scene: per satellite the offset the search is to choose is the strongest hypothesis of its cell by more than
    a factor 1.5 (noise-free: 18 against 10), the satellites do not all choose the same one, and the model on x[o N:] has one clear
    peak on the satellite's bin"""
    e = FM.edge_case()
    x = FM.edge_scene(codes)
    N, periods = e["N"], e["K"] * e["M"]
    assert FM.fft_size_of(N, periods) == e["n"] == 1 << 17 and len(set(e["chosen"])) > 1
    for s, o in zip(e["sats"], e["chosen"]):
        p = FM.edge_cell_powers(x, e, s, codes[s["row"]])
        h = e["offsets"].index(o)
        assert all(p[h] > 1.5 * p[j] for j in range(len(p)) if j != h), (s, p)
        _check_scene(x[o * N:(o + periods) * N], e["fmt"], [s], lambda s: codes[s["row"]], 1.023e6, e["fs"], periods, N, ("edge", o))


def _supported(gm):
    import ctypes as C
    lib = gm.lib()
    n = lib.gm_fft_supported_sizes(None, 0)
    buf = (C.c_uint32 * n)()
    assert lib.gm_fft_supported_sizes(C.cast(buf, C.c_void_p), n) == n
    return set(int(v) for v in buf)


def test_factor_table(gm):
    """The `l2` loop of gm_acq_finer_doppler restated over the library's own plan list: exactly the nine pairs of FACTOR_TABLE, nothing
    below 2^16 or above 2^24 is asked for, the row tiles follow FineRows<PL>::RT, and every pair has a geometry.  A new power-of-two
    plan fails here until the model's tables, and a geometry for any new pair, follow."""
    sizes = _supported(gm)
    pow2 = {s for s in sizes if s & (s - 1) == 0}
    assert pow2 == set(FM.POW2_PLANS), pow2
    # the restated plans are the header's
    text = open(os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc", "fft_plans.h")).read()
    for N, (T, radices) in FM.POW2_PLANS.items():
        mt = re.search(r"using Plan%d = Plan<%d, (\d+), ([\d, ]+)>;" % (N, N), text)
        assert mt and int(mt.group(1)) == T and tuple(int(v) for v in mt.group(2).split(",")) == radices, N
        assert int(np.prod(radices)) == N
    for lg in range(10, 29):
        n = 1 << lg
        pair = FM.factor_pair(n, pow2)
        if 16 <= lg <= 24:
            assert pair is not None and pair + (FM.row_tile(pair[1]),) == FM.FACTOR_TABLE[n], (n, pair)
        else:
            assert n not in FM.FACTOR_TABLE
            assert lg > 24 or pair is None, (n, pair)       # (above 2^24 the entry refuses before it factors)
    assert FM.row_tile(256) == 4 and 256 // 16 < FM.POW2_PLANS[256][0]     # Plan256: 16 of 64 lanes own a pass-0 butterfly
    reached = {}
    for N, periods in FM.geometries():
        assert N in sizes
        reached.setdefault(FM.fft_size_of(N, periods), []).append((N, periods))
    assert set(reached) == set(FM.FACTOR_TABLE)
    assert FM.fft_size_of(2048, 2) == 1 << 14 and FM.fft_size_of(4096, 2) == 1 << 15      # the refused sizes below
    assert (2048, 5) in reached[1 << 16] and (16384, 129) in reached[1 << 24] and 130 * 16384 - 16384 > 1 << 21


def test_header_states_the_range():
    header = open(os.path.join(ROOT, "include", "gnss_mi355x.h")).read()
    start = header.index("/* Fine-Doppler refinement after detection")
    para = " ".join(header[start:header.index("int gm_acq_finer_doppler", start)].replace("\n *", " ").split())
    assert "8*next_pow2((K*M-1)*N) must lie in 2^16 .. 2^24, else GM_ERR_UNSUPPORTED_N" in para
    assert "Entries of not-found PRNs are left untouched" in para
    assert "below fft_size, else GM_ERR_OUT_OF_RANGE" in para
