"""gm_acq_finer_doppler on the GPU against the float64 model of acq_fine_model.py, at every (N1, N2) pair the host's factor rule reaches.

The entry runs a four-step N1 x N2 transform: fine_cols_kernel (plan N1, inter-factor twiddle by sincospif), fine_rows_kernel (plan
N2, FineRows<PL>::RT rows a workgroup, first-index arg-max), fine_mean_kernel, fine_final_kernel.  Every case places its satellites
by row k1 = idx % N1 and column k2 = idx // N1 (acq_fine_model.placements): the last row of the last workgroup's tile, the first row
of a tile in the middle with a negative frequency, and row 1.  test_acq_fine_host.py has checked on the CPU that each scene's peak is
on that bin and 1e-3 clear of the next value, so index and frequency are compared exactly.

The bound on the peak's magnitude, derived and not measured:  | peak_mag - |X_model[idx]| | <= c 2^-24 sum_n |x_n| + size_use |dm|
with x_n = (s[cp + n] - mean) chip(n), the transform's input.  One output is a sum over all inputs, each carrying the relative errors
of the operations on its path; in units of 2^-24 (half an ulp), counted in acq_fine_model.bound_constant:
  1          (s - mean) in float32; the product with the chip, +-1, is exact
  3 lg n     a radix-r pass as log2 r radix-2 stages, each a sum (1) and a complex product with a constant (2): lg n stages in all
  tw(R)      per pass after a plan's first, the pass twiddle W^r, r < R: a float32 table word (1) taken to the power r <= R - 1 through
             the power tree's products (fft_core.h TwPow; at most 5 products for R = 16, 4 for R = 8, 2 roundings each):
             tw(16) = 15 + 10, tw(8) = 7 + 8
  2 + 2      the inter-factor twiddle: a sincospif result (2^-23) and its complex product
  1 + 2      fmaf(x, x, y * y) — two roundings of the power are one of the magnitude — and sqrtf, on |X|
so c = 106 at 2^16 (256 x 256: two passes tw(16)) and 180 at 2^24 (4096 x 4096: four).  dm = mean_dev - mean_model enters every input
alike, so it moves an output by at most size_use |dm|; fine_mean_kernel's tree (a lane's sequential sum of ceil(L / 1024) terms, six
shuffle levels, fifteen sequential sums, one division: mean_depth) bounds each component of dm by depth 2^-24 mean(|Re s| + |Im s|).
The model's own float64 error is nine orders below.  A worst-case bound adds moduli where the roundings add like a random walk, so the
ratios are small; one above 1 would be a finding.

Largest error over bound per size, as printed by test_every_pair_against_the_model on an MI355X:
  2^16 = 256 x 256   (2048 x 4, c32)    0.0225      2^16 (2048 x 5, c32)     0.0121
  2^17 = 512 x 256   (2048 x 6, i8)     0.0219
  2^18 = 512 x 512   (2048 x 10, real)  0.0028
  2^19 = 1024 x 512  (4096 x 10, c32)   0.0092
  2^20 = 1024 x 1024 (8192 x 10, i8)    0.0054
  2^21 = 2048 x 1024 (16384 x 10, real) 0.0039
  2^22 = 2048 x 2048 (16384 x 18, c32)  0.0029
  2^23 = 4096 x 2048 (16384 x 34, i8)   0.0006
  2^24 = 4096 x 4096 (16384 x 66, real) 0.0013      2^24 (16384 x 129, i8)   0.0011
(the ratio falls like 1 / sqrt(size_use), as a random walk against a sum of moduli does; the bound itself is 1.3e-5 of the peak at
2^16 and 2.2e-4 at 129 periods, where the mean's term is the larger part).  The several-passes scene reaches 0.0277, the 2046-chip
code 0.0066.
"""
import ctypes as C

import numpy as np
import pytest

import acq_fine_model as FM

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED_N, OUT_OF_RANGE = -1, -2, -5
CA_RATE = 1.023e6


@pytest.fixture(scope="module")
def codes(gpu):
    from gnss_sdr_rs_amd import acquisition as A
    return np.asarray(A.ca_code_table(), np.int8)


def _f32_word(v):
    return int(np.float32(v).view(np.uint32))


def _words(fine):
    """A worker's three output words: the frequency's and the magnitude's float32 bits and the index"""
    return None if fine is None else (_f32_word(fine["freq_hz"]), int(fine["peak_index"]), _f32_word(fine["peak_mag"]))


def _hand(sats, fs, found=None):
    """Hand-made results with the scene's code phases; worker w refines satellite w"""
    return [dict(prn=w + 1, code_phase_samples=s["cp"], code_phase_chips=0.0, carrier_freq=0.0, fs=fs, mag_relative=0.0,
                 sample_global_index=0, doppler_bin=0) if found is None or found[w] else None for w, s in enumerate(sats)]


def _engine(N, periods, fs, codes=None, code_rate=CA_RATE, K=1, doppler_hz=0.0):
    from gnss_sdr_rs_amd import acquisition as A
    assert periods % K == 0
    return A.AcquisitionEngine(fs, 0.0, N, doppler_hz=np.array([doppler_hz], np.float32), prn_ids=[1, 2, 3], n_integrations=periods // K,
                               codes=codes, code_rate=code_rate, coherent_periods=K)


def _refine(eng, sats, fs, found=None):
    hand = _hand(sats, fs, found) + [None] * (3 - len(sats))
    return eng.finer_doppler(hand)


def _summary(x, sats, chips_of, code_rate, fs, periods, N):
    """Per satellite the scalars of the model a comparison needs (the 2^24 magnitudes themselves are not kept)"""
    xc = FM.as_complex(x)
    out = []
    for s in sats:
        m = FM.fine_model(xc, s["cp"], chips_of(s), code_rate, fs, periods, N)
        n, k = m["fft_size"], m["peak_index"]
        out.append(dict(n=n, peak=k, image=(n - k) % n, mag={k: float(m["mag"][k]), (n - k) % n: float(m["mag"][(n - k) % n])},
                        bound=FM.bound(m, periods, N)))
    return out


_CASES = {}


def _case(g, codes):
    """Geometry g's scene and model, computed once and shared by the tests that refine it"""
    if g not in _CASES:
        N, periods, fmt, fs, sats, _ = FM.case(g)
        x = FM.case_scene(g, codes)
        _CASES[g] = (x, _summary(x, sats, lambda s: codes[s["row"]], CA_RATE, fs, periods, N))
    return _CASES[g]


def _compare(fine, model, fmt, fs, what):
    """index, frequency word and magnitude of one worker against the model; -> error over bound"""
    n = model["n"]
    assert fine["fft_size"] == n, (what, fine)
    k = fine["peak_index"]
    if fmt == "real":       # |X[k]| = |X[n - k]| for a real snapshot: either image, with equal |freq|
        assert k in (model["peak"], model["image"]), (what, fine, model["peak"])
        assert abs(FM.freq_rule(k, n, fs)) == abs(FM.freq_rule(model["peak"], n, fs))
    else:
        assert k == model["peak"], (what, fine, model["peak"])
    assert _f32_word(fine["freq_hz"]) == _f32_word(FM.freq_rule(k, n, fs)), (what, fine, FM.freq_rule(k, n, fs))
    err = abs(fine["peak_mag"] - model["mag"][k])
    ratio = err / model["bound"]
    print("%s: idx %d |X| %.6e model %.6e error %.3e bound %.3e ratio %.4f" % (what, k, fine["peak_mag"], model["mag"][k], err,
                                                                            model["bound"], ratio))
    assert err <= model["bound"], (what, fine, model["mag"][k], model["bound"])
    return ratio


@pytest.mark.parametrize("g", range(len(FM.geometries())))
def test_every_pair_against_the_model(gpu, codes, g):
    """The eleven geometries, the three formats rotating over them: fft_size, the peak's index, the frequency's float32 word by the
    header's rule, and the magnitude within the derived bound"""
    N, periods, fmt, fs, sats, _ = FM.case(g)
    x, models = _case(g, codes)
    eng = _engine(N, periods, fs)
    eng.search(x)
    fine = _refine(eng, sats, fs)
    eng.close()
    n = FM.fft_size_of(N, periods)
    assert fine[len(sats):] == [None] * (3 - len(sats))
    worst = max(_compare(fine[w], models[w], fmt, fs, "N %d periods %d %s sat %d" % (N, periods, fmt, w)) for w in range(len(sats)))
    N1, N2, RT = FM.FACTOR_TABLE[n]
    print("fine Doppler 2^%d = %d x %d (RT %d), N %d x %d periods, %s: largest error over bound %.4f"
          % (n.bit_length() - 1, N1, N2, RT, N, periods, fmt, worst))


@pytest.mark.parametrize("g", [1, 6])
def test_company_and_repetition(gpu, codes, g):
    """2^17 and 2^22: a worker's words do not depend on who is refined with it (alone the call has S = 1 and worker 2 sits in slot 0)
    nor on a call before it"""
    N, periods, fmt, fs, sats, _ = FM.case(g)
    x, models = _case(g, codes)
    eng = _engine(N, periods, fs)
    eng.search(x)
    alone = [_refine(eng, sats, fs, found=[i == w for i in range(3)]) for w in (2, 0, 1)]
    for w, fine in zip((2, 0, 1), alone):
        assert [f is not None for f in fine] == [i == w for i in range(3)]
    together = _refine(eng, sats, fs)
    again = _refine(eng, sats, fs)
    eng.close()
    for w, fine in zip((2, 0, 1), alone):
        assert _words(fine[w]) == _words(together[w]) == _words(again[w]), (g, w, fine[w], together[w], again[w])
        _compare(fine[w], models[w], fmt, fs, "alone, geometry %d sat %d" % (g, w))


def _raw(eng, sats, fs, found, want, sentinel_f=-12345.0, sentinel_i=0xDEADBEEFCAFE):
    """The C entry itself with prefilled outputs; want = (freq, index, mag, size): which output pointers are not NULL"""
    from gnss_sdr_rs_amd._lib import AcqResult, lib
    res = (AcqResult * 3)()
    for w, s in enumerate(sats):
        res[w].prn, res[w].code_phase_samples, res[w].fs, res[w].doppler_bin = w + 1, s["cp"], fs, 0
    fnd = np.asarray(found, np.uint8)
    f = np.full(3, sentinel_f, np.float32)
    idx = np.full(3, sentinel_i, np.uint64)
    mag = np.full(3, sentinel_f, np.float32)
    size = C.c_uint64(sentinel_i)
    ptr = lambda a, on: C.c_void_p(a.ctypes.data) if on else None
    rc = lib().gm_acq_finer_doppler(eng._h, C.cast(res, C.c_void_p), ptr(fnd, True), 3, ptr(f, want[0]), ptr(idx, want[1]),
                                    ptr(mag, want[2]), C.cast(C.byref(size), C.c_void_p) if want[3] else None)
    return rc, f.view(np.uint32), idx, mag.view(np.uint32), size.value


def test_not_found_entries_and_null_outputs(gpu, codes):
    """found = [1, 0, 1] through the C entry: worker 1's entries keep what the caller put there, the others are the words of the call
    that refines all three; every combination of NULL output pointers returns 0 and fills the outputs that are given alike"""
    g = 1
    N, periods, fmt, fs, sats, _ = FM.case(g)
    x, models = _case(g, codes)
    eng = _engine(N, periods, fs)
    eng.search(x)
    ref = [_words(f) for f in _refine(eng, sats, fs)]
    sent_f, sent_i = _f32_word(-12345.0), 0xDEADBEEFCAFE
    for bits in range(16):
        want = [bool(bits >> b & 1) for b in range(4)]
        rc, f, idx, mag, size = _raw(eng, sats, fs, [1, 0, 1], want)
        assert rc == 0, (want, rc)
        for w in range(3):
            hit = w != 1
            assert int(f[w]) == (ref[w][0] if hit and want[0] else sent_f), (want, w)
            assert int(idx[w]) == (ref[w][1] if hit and want[1] else sent_i), (want, w)
            assert int(mag[w]) == (ref[w][2] if hit and want[2] else sent_f), (want, w)
        assert size == (FM.fft_size_of(N, periods) if want[3] else sent_i)
    # nothing found: nothing written, fft_size still reported
    rc, f, idx, mag, size = _raw(eng, sats, fs, [0, 0, 0], [True] * 4)
    assert rc == 0 and (f == sent_f).all() and (idx == sent_i).all() and (mag == sent_f).all() and size == FM.fft_size_of(N, periods)
    eng.close()
    for w in (0, 2):
        _compare(dict(zip(("freq_hz", "peak_index", "peak_mag"), (np.uint32(ref[w][0]).view(np.float32), ref[w][1],
                                                                  np.uint32(ref[w][2]).view(np.float32))), fft_size=models[w]["n"]),
                 models[w], fmt, fs, "raw entry sat %d" % w)


def test_several_passes(gpu, codes):
    """A coherent handle with the edge search on a scene whose satellites' bit edges make the search choose the offsets 0, 1 and 1:
    the call that refines all three runs two passes (the second with two workers, more than any call before it, so the per-satellite
    buffers grow between the passes) and gives the words of the calls that refine each satellite alone; each agrees with the model on
    x[o N:] for its own offset"""
    e = FM.edge_case()
    N, K, M, fs, fmt, sats = e["N"], e["K"], e["M"], e["fs"], e["fmt"], e["sats"]
    periods = K * M
    x = FM.edge_scene(codes)
    eng = _engine(N, periods, fs, K=K, doppler_hz=e["doppler_hz"])
    eng.set_edge_search(e["offsets"])
    assert eng.dwell_samples == len(x)
    eng.search(x)
    chosen = [int(e["offsets"][h]) for h in eng.edge_choice()[:, 0]]
    assert chosen == e["chosen"], chosen                    # the real search's own choice: two distinct offsets
    alone = [_refine(eng, sats, fs, found=[i == w for i in range(3)])[w] for w in range(3)]      # every call so far: S = 1
    full = _refine(eng, sats, fs)                           # offset 0: S = 1, offset 1: S = 2
    again = [_refine(eng, sats, fs, found=[i == w for i in range(3)])[w] for w in range(3)]
    eng.close()
    for w, s in enumerate(sats):
        assert _words(full[w]) == _words(alone[w]) == _words(again[w]), (w, full[w], alone[w], again[w])
        o = chosen[w]
        model = _summary(x[o * N:(o + periods) * N], [s], lambda s: codes[s["row"]], CA_RATE, fs, periods, N)[0]
        assert model["peak"] == s["idx"]
        _compare(full[w], model, fmt, fs, "edge offset %d sat %d" % (o, w))


def test_another_code(gpu):
    """2046 chips at 2.046 Mchip/s on 2048 samples a period, at 2^18: a chip is hardly longer than a sample, so the float32 chip index
    of the kernel has to be the model's at every sample"""
    N, periods, fmt, fs, code_rate, ccodes, sats, _ = FM.custom_case()
    x = FM.custom_scene()
    models = _summary(x, sats, lambda s: ccodes[s["row"]], code_rate, fs, periods, N)
    eng = _engine(N, periods, fs, codes=ccodes, code_rate=code_rate)
    eng.search(x)
    fine = _refine(eng, sats, fs)
    eng.close()
    for w in range(3):
        _compare(fine[w], models[w], fmt, fs, "2046-chip code sat %d" % w)


def test_refusals(gpu, codes):
    """Each refusal with its status, and a good call after each gives the words it gave before"""
    from gnss_sdr_rs_amd._lib import GmError
    g = 0
    N, periods, fmt, fs, sats, _ = FM.case(g)
    x, _ = _case(g, codes)
    good = _engine(N, periods, fs)
    good.search(x)
    ref = [_words(f) for f in _refine(good, sats, fs)]

    def refused(status, fn):
        with pytest.raises(GmError) as ei:
            fn()
        assert ei.value.status == status, ei.value
        assert [_words(f) for f in _refine(good, sats, fs)] == ref

    # before any search
    fresh = _engine(N, periods, fs)
    refused(INVALID, lambda: _refine(fresh, sats, fs))
    fresh.search(x)
    assert [_words(f) for f in _refine(fresh, sats, fs)] == ref      # the refused call left the handle usable
    fresh.close()
    # one period: nothing after the code phase
    one = _engine(N, 1, fs)
    one.search(x[:N])
    refused(INVALID, lambda: _refine(one, sats, fs))
    one.close()
    # 2^14 and 2^15: below the smallest pair of plans
    for n_small in (2048, 4096):
        small = _engine(n_small, 2, 1000.0 * n_small)
        small.search(np.zeros(2 * n_small, np.complex64))
        refused(UNSUPPORTED_N, lambda: _refine(small, sats, fs))
        small.close()
    # (16384, 130): (periods - 1) N is one period above 2^21
    big = _engine(16384, 130, 16.384e6)
    big.search(np.zeros((130 * 16384, 2), np.int8))
    refused(UNSUPPORTED_N, lambda: _refine(big, sats, 16.384e6))
    big.close()
    # a code phase of a whole period is not a code phase
    late = [dict(s, cp=N) if w == 1 else s for w, s in enumerate(sats)]
    refused(OUT_OF_RANGE, lambda: _refine(good, late, fs))
    good.close()
