"""FFT-domain narrowband interference excision on the GPU (gm_excisor, csrc/excise_kernels.hip) against the float64 model of
excise_model.py, which is handed the library's own window words (gm_excisor_windows) and gains (gm_excisor_gains).

1. Words.  Per output |device - model| <= 1e-5 max|xb| over the two blocks the output comes from: the project's 1e-5 parity bar, taken
   relative to the transforms' INPUT scale — a transform's rounding error scales with its input, not with its possibly excised output.
   B = 256, 512, 1024, 2048, 4096 (every plan), both sample formats (the int8 stream holds -128), call lengths 1, H - 1, H, H + 1, 3H - 1, 5B + 7 and 40 H,
   gains all one, random in [0, 1] and a 0/1 mask; a 60 dB-above-noise CW on and off a bin centre; a call of 2299 segments (tiles of two
   segments, the last tile short).  The largest error over bound seen is printed.
2. Cutting: one call against the same stream in blocks of 1, 7, H - 1, 1000 and 3001, bit for bit; after reset; at absolute indices
   2^32 - 3 and 2^40 + 12345.
3. Blanking: spikes on block edges (every segment is a tile edge at these lengths), in the history and across call boundaries; exactly
   at the threshold; the blanked count against the model.
4. adapt, at every B: P against the model within 1e-5 max_k P_model[k]; the median word is the rank-(B - 1) div 2 element of the device's own P; the
   counts and the gains equal detect() on the device's P words; guard 0, 2, 16; a CW in bin 0 and bin B - 1 (the circular guard); two
   calls give the same words; adapt_dev followed by process_dev with no host call in between uses the new gains.
5. Every refusal, with nothing written and the state untouched.
6. The ring path over two wraps, word for word against front-end, then excisor, then resampler run separately; with and without a
   resampler.
7. The chain: the host test's J/N 30 dB scene through Excisor.adapt on its first four periods, process, then a plain search_dev."""
import ctypes as C

import numpy as np
import pytest

import excise_model as EM
import stage_instantiations as SI

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
REL = 1e-5


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "i8":
        x = rng.integers(-128, 128, (n, 2)).astype(np.int8)
        if n:
            x[n // 3] = (-128, 127)
            x[n // 2] = (-128, -128)
        return x
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _bps(fmt):
    return 2 if fmt == "i8" else 8


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, ex, d_x, fmt, n, blocks=None, cap=None):
    """the n samples at d_x through ex.process_dev in blocks (None: one call) -> complex64 outputs, all of them behind each other in
    one device buffer whose tail must stay as it was filled"""
    cap = cap if cap is not None else n + 4096                      # a call delivers at most its inputs + H - 1
    d_y = hipbuf.alloc(cap * 8 + 64, fill=0x5A)
    done = got = 0
    step = blocks or max(n, 1)
    while True:
        k = min(step, n - done)
        got += ex.process_dev(d_x + done * _bps(fmt), _fmt(fmt), k, d_y + got * 8, cap - got)
        done += k
        if done >= n:
            break
    ex.synchronize()
    raw = hipbuf.download(d_y, cap * 8 + 64, np.complex64)
    assert (raw[got:].view(np.uint8) == 0x5A).all()                     # nothing behind the last output
    return raw[:got].copy()


def _check(tag, got, want, scale):
    assert got.size == want.size, (tag, got.size, want.size)
    if not got.size:
        return 0.0
    assert np.isfinite(got.view(np.float32)).all(), tag
    err = np.abs(got.astype(np.complex128) - want)
    bound = REL * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (tag, worst)
    return worst


def _gain_sets(B, seed):
    rng = np.random.default_rng(seed)
    g = rng.random(B).astype(np.float32)
    g[::17] = 0.0
    g[5::29] = 1.0
    return [("ones", np.ones(B, np.float32)), ("random", g), ("mask", (rng.random(B) > 0.3).astype(np.float32))]


@pytest.mark.parametrize("block", SI.BLOCKS)
def test_words_against_the_model(gpu, hipbuf, block):
    from gnss_sdr_rs_amd import excise
    ex = excise.Excisor(block)
    p = EM.resolve(block)
    B, H = block, block // 2
    assert ex.block == B
    wa, ws = ex.windows()
    lengths = [1, H - 1, H, H + 1, 3 * H - 1, 5 * B + 7, 40 * H]
    worst = 0.0
    for fmt in ("i8", "c32"):
        x = _stream(fmt, lengths[-1], 17 + B)
        d_x = hipbuf.upload(x)
        for name, g in _gain_sets(B, B):
            ex.set_gains(g)
            assert (_words(ex.gains()) == _words(g)).all()
            for n in lengths:
                ex.reset(0)
                got = _feed(hipbuf, ex, d_x, fmt, n)
                want, scale, m = EM.run(p, x[:n], wa, ws, g)
                assert got.size == EM.total_out(B, n)
                worst = max(worst, _check((B, fmt, name, n), got, want, scale))
                assert ex.stats() == dict(inputs=n, outputs=EM.total_out(B, n), blanked=0)
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()           # the input is only read
    # unit gains reconstruct the input: the filter bank is transparent
    ex.set_gains(np.ones(B, np.float32))
    ex.reset(0)
    got = _feed(hipbuf, ex, d_x, "c32", lengths[-1])
    assert np.abs(got - x[:got.size]).max() <= REL * np.abs(x).max()
    print("B = %d: largest error / bound %.3f" % (B, worst))
    ex.close()


def test_a_long_call_runs_tiles_of_two_segments(gpu, hipbuf):
    """2299 segments of B = 256: the kernel's tiles hold two segments and the last tile one; the words are the model's and those of the
    same stream cut into calls whose tiles hold one segment"""
    from gnss_sdr_rs_amd import excise
    B, H = 256, 128
    ex = excise.Excisor(B, blank_threshold=3.0)
    p = EM.resolve(B, blank_threshold=3.0)
    wa, ws = ex.windows()
    g = _gain_sets(B, 3)[1][1]
    ex.set_gains(g)
    n = H * 2300 + 5
    x = _stream("c32", n, 41)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, ex, d_x, "c32", n)
    want, scale, m = EM.run(p, x, wa, ws, g)
    assert whole.size == 2299 * H and m.blanked > 100
    print("largest error / bound %.3f" % _check("long", whole, want, scale))
    assert ex.stats() == dict(inputs=n, outputs=whole.size, blanked=m.blanked)
    ex.reset(0)
    assert (_words(_feed(hipbuf, ex, d_x, "c32", n, 100 * H + 3)) == _words(whole)).all()
    ex.close()


@pytest.mark.parametrize("block,offset", [(1024, 0.0), (1024, 0.37), (4096, 0.5)])
def test_a_strong_cw_on_and_off_a_bin_centre(gpu, hipbuf, block, offset):
    """a CW 60 dB above the noise: the error stays within 1e-5 of the INPUT scale with unit gains, and with the adapted mask, which
    takes the carrier out"""
    from gnss_sdr_rs_amd import excise
    B, H = block, block // 2
    n = 40 * H
    rng = np.random.default_rng(5)
    k0 = 100 + offset
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n) +
         np.sqrt(2.0) * 1000.0 * np.exp(2j * np.pi * k0 * np.arange(n) / B)).astype(np.complex64)
    ex = excise.Excisor(B, guard_bins=2)
    p = EM.resolve(B, guard_bins=2)
    wa, ws = ex.windows()
    d_x = hipbuf.upload(x)
    got = _feed(hipbuf, ex, d_x, "c32", n)
    want, scale, _ = EM.run(p, x, wa, ws)
    worst = _check("unit gains", got, want, scale)
    ex.adapt_dev(d_x, _fmt("c32"), n)
    g = ex.gains()
    assert g[100] == 0.0 and 5 <= (g == 0).sum() <= B // 4
    ex.reset(0)
    got = _feed(hipbuf, ex, d_x, "c32", n)
    want, scale, _ = EM.run(p, x, wa, ws, g)
    worst = max(worst, _check("adapted", got, want, scale))
    inner = got[B:-B]
    print("B = %d, CW at bin %.2f: largest error / bound %.3f; rms in %.1f, out %.2f" %
          (B, k0, worst, np.sqrt(np.mean(np.abs(x) ** 2)), np.sqrt(np.mean(np.abs(inner) ** 2))))
    assert np.sqrt(np.mean(np.abs(inner) ** 2)) < 0.05 * np.sqrt(np.mean(np.abs(x) ** 2))       # 60 dB above the noise in, within 26 dB of it out
    ex.close()


SPLITS = (1, 7, None, 1000, 3001)          # None: H - 1


@pytest.mark.parametrize("block,fmt,n", [(1024, "i8", 6007), (256, "c32", 6007), (2048, "c32", 9001), (4096, "i8", 12301),
                                         (512, "i8", 6007), (512, "c32", 6007)])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, block, fmt, n):
    from gnss_sdr_rs_amd import excise
    B, H = block, block // 2
    ex = excise.Excisor(B)
    p = EM.resolve(B)
    wa, ws = ex.windows()
    g = _gain_sets(B, 7)[1][1]
    ex.set_gains(g)
    x = _stream(fmt, n, 5)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, ex, d_x, fmt, n)
    want, scale, _ = EM.run(p, x, wa, ws, g)
    _check((B, "whole"), whole, want, scale)
    for blocks in SPLITS:
        ex.reset(0)
        got = _feed(hipbuf, ex, d_x, fmt, n, blocks or H - 1)
        assert (_words(got) == _words(whole)).all(), (B, blocks)
    ex.reset(0)
    assert (_words(_feed(hipbuf, ex, d_x, fmt, n)) == _words(whole)).all()                      # again after reset: the same words
    assert (_words(ex.gains()) == _words(g)).all()                                               # reset keeps the gains
    # absolute indices above 2^32: the model at those indices, and the cuts still do not matter
    for index in ((1 << 40) + 12345, (1 << 32) - 3):
        ex.reset(index)
        far = _feed(hipbuf, ex, d_x, fmt, n)
        want, scale, m = EM.run(p, x, wa, ws, g, input_index=index)
        assert far.size == m.outputs == EM.plan(B, index, n)
        _check((B, index), far, want, scale)
        ex.reset(index)
        assert (_words(_feed(hipbuf, ex, d_x, fmt, n, 1000)) == _words(far)).all()
        assert ex.stats() == dict(inputs=n, outputs=far.size, blanked=0)
    ex.close()


def _spiky(fmt, H, n):
    """a quiet stream (|re|, |im| <= 20) with spikes around block edges (multiples of H), around the cuts of the 1000-sample split, at
    the stream's two ends, and the pair that sits exactly at / just above the threshold 100"""
    rng = np.random.default_rng(9)
    x = rng.integers(-20, 21, (n, 2)).astype(np.int8)
    spikes = [0, 700, H - 1, H, H + 1, 2 * H - 1, 2 * H, 3 * H, 999, 1000, 1001, 1999, 2000, 2000 + H, 2999, 5 * H - 1, 5 * H, n - 1]
    for s in spikes:
        x[s] = (127, -128)
    x[300] = (60, 80)                                              # 3600 + 6400 = 10000 = thr^2: kept
    x[301] = (60, 81)                                              # blanked
    x[302] = (-100, 0)                                             # kept
    x[303] = (0, 101)                                              # blanked
    n_blank = len(set(spikes)) + 2
    if fmt == "c32":
        return (x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64), n_blank
    return x, n_blank


@pytest.mark.parametrize("fmt", ["i8", "c32"])
def test_blanking(gpu, hipbuf, fmt):
    from gnss_sdr_rs_amd import excise
    B, H = 1024, 512
    ex = excise.Excisor(B, blank_threshold=100.0)
    p = EM.resolve(B, blank_threshold=100.0)
    wa, ws = ex.windows()
    n = 5003
    x, n_blank = _spiky(fmt, H, n)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, ex, d_x, fmt, n)
    want, scale, m = EM.run(p, x, wa, ws)
    assert m.blanked == n_blank
    _check((fmt, "whole"), whole, want, scale)
    assert ex.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank)
    for blocks in SPLITS:
        ex.reset(0)
        got = _feed(hipbuf, ex, d_x, fmt, n, blocks or H - 1)
        assert (_words(got) == _words(whole)).all(), blocks
        assert ex.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank), blocks       # each input once, whatever the cuts
    # the blanked samples matter: the model without blanking is somewhere else
    want_plain, scale_plain, _ = EM.run(EM.resolve(B), x, wa, ws)
    assert np.abs(want_plain - want).max() > 10.0
    # threshold 0 is a handle without blanking
    off, zero = excise.Excisor(B), excise.Excisor(B, blank_threshold=0.0)
    a, b = _feed(hipbuf, off, d_x, fmt, n), _feed(hipbuf, zero, d_x, fmt, n)
    assert (_words(a) == _words(b)).all() and zero.stats()["blanked"] == 0
    _check((fmt, "off"), a, want_plain, scale_plain)
    for h in (ex, off, zero):
        h.close()


def _adapt_input(B, J, kind, seed):
    H = B // 2
    n = (J + 1) * H + 3                                              # three samples that belong to no block
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if kind == "cw":
        x += np.sqrt(2.0 * 1000.0) * np.exp(2j * np.pi * 0.06032 * np.arange(n))
    elif kind == "bin0":
        x += 30.0
    elif kind == "last":
        x += 30.0 * np.exp(-2j * np.pi * np.arange(n) / B)
    return x.astype(np.complex64)


def _check_adapt(ex, p, x, wa, tag):
    B = p["B"]
    r = ex.psd()
    P = r["P"]
    want = EM.psd(p, x, wa)
    err = np.abs(P.astype(np.float64) - want).max() / (REL * want.max())
    assert err <= 1.0, (tag, err)
    assert _words(np.array([r["median"]], np.float32))[0] == _words(np.sort(P)[(B - 1) // 2:(B - 1) // 2 + 1])[0], tag
    med, flag, g = EM.detect(P, np.float32(p["factor"]), p["guard"])
    assert (r["n_flagged"], r["n_zeroed"]) == (int(flag.sum()), int((g == 0).sum())), tag
    assert (_words(ex.gains()) == _words(g)).all(), tag
    return err, r


@pytest.mark.parametrize("block", SI.BLOCKS)
def test_adapt(gpu, hipbuf, block):
    from gnss_sdr_rs_amd import excise
    B, H = block, block // 2
    worst = 0.0
    for kind, J, guard, fmt in (("noise", 31, 0, "c32"), ("noise", 64, 2, "c32"), ("cw", 64, 2, "c32"), ("cw", 31, 0, "c32"),
                                ("bin0", 40, 16, "c32"), ("last", 40, 16, "c32"), ("bin0", 40, 2, "c32"), ("noise", 33, 2, "i8")):
        ex = excise.Excisor(B, guard_bins=guard, blank_threshold=150.0 if fmt == "i8" else 0.0)
        p = EM.resolve(B, guard, 0.0, 150.0 if fmt == "i8" else 0.0)
        wa, _ = ex.windows()
        x = _stream("i8", (J + 1) * H, J) if fmt == "i8" else _adapt_input(B, J, kind, J + guard)
        d_x = hipbuf.upload(x)
        assert ex.psd()["n_zeroed"] == 0 and not ex.psd()["P"].any()                            # before the first adapt
        ex.adapt_dev(d_x, _fmt(fmt), x.size // 2 if fmt == "i8" else x.size)
        err, r = _check_adapt(ex, p, x, wa, (B, kind, J, guard))
        worst = max(worst, err)
        g = ex.gains()
        if kind == "noise" and fmt == "c32" and ((B == 256 and J >= 64) or (B == 1024 and J >= 31)):
            assert r["n_flagged"] == 0 and g.all()                                              # (the host test: max / median <= 2.05 there)
        if kind == "cw":
            assert g[int(round(0.06032 * B))] == 0.0 and 1 <= r["n_flagged"] <= r["n_zeroed"] <= 64
        if kind == "bin0":
            assert g[0] == 0.0 and not g[:guard + 1].any() and not g[B - guard:].any() and g[B // 2] == 1.0     # the guard wraps
        if kind == "last":
            assert g[B - 1] == 0.0 and not g[:guard].any() and not g[B - 1 - guard:].any() and g[B // 2] == 1.0
        first = (ex.psd(), ex.gains())
        ex.adapt_dev(d_x, _fmt(fmt), x.size // 2 if fmt == "i8" else x.size)
        again = ex.psd()
        assert (_words(again["P"]) == _words(first[0]["P"])).all() and (_words(ex.gains()) == _words(first[1])).all()
        assert (again["median"], again["n_flagged"], again["n_zeroed"]) == (first[0]["median"], first[0]["n_flagged"], first[0]["n_zeroed"])
        assert ex.stats() == dict(inputs=0, outputs=0, blanked=0)                               # adapt is no part of the stream
        ex.close()
    print("B = %d: largest P error / bound %.3f" % (B, worst))


def test_adapt_with_long_chunks_and_the_host_form(gpu, hipbuf):
    """J = 5000 blocks of 256: chunks of ceil(5000 / 512) = 10 blocks; Excisor.adapt on host samples gives adapt_dev's words"""
    from gnss_sdr_rs_amd import excise
    B = 256
    ex = excise.Excisor(B, guard_bins=1)
    p = EM.resolve(B, 1)
    wa, _ = ex.windows()
    x = _adapt_input(B, 5000, "cw", 77)
    d_x = hipbuf.upload(x)
    ex.adapt_dev(d_x, _fmt("c32"), x.size)
    err, r = _check_adapt(ex, p, x, wa, "long")
    ex2 = excise.Excisor(B, guard_bins=1)
    ex2.adapt(x)
    assert (_words(ex2.psd()["P"]) == _words(r["P"])).all() and (_words(ex2.gains()) == _words(ex.gains())).all()
    print("largest P error / bound %.3f, %d bins zeroed" % (err, r["n_zeroed"]))
    ex.close(); ex2.close()


def test_process_behind_adapt_uses_the_new_gains(gpu, hipbuf):
    """adapt_dev and process_dev enqueued back to back on the handle's stream, no host call in between: the outputs are the model's with
    the gains the adapt installed; the same on a stream of the caller's behind a set_gains"""
    from gnss_sdr_rs_amd import excise
    B, H = 1024, 512
    n = 20 * H
    x = _adapt_input(B, 19, "cw", 3)[:n]
    ex = excise.Excisor(B, guard_bins=2)
    p = EM.resolve(B, 2)
    wa, ws = ex.windows()
    d_x = hipbuf.upload(x)
    d_y = hipbuf.alloc(n * 8)
    ex.adapt_dev(d_x, _fmt("c32"), n)
    got = ex.process_dev(d_x, _fmt("c32"), n, d_y, n)
    ex.synchronize()
    y = hipbuf.download(d_y, got * 8, np.complex64)
    g = ex.gains()
    assert (g == 0).sum() >= 5
    want, scale, _ = EM.run(p, x, wa, ws, g)
    _check("behind adapt", y, want, scale)
    with_ones, _, _ = EM.run(p, x, wa, ws)
    assert np.abs(with_ones - want).max() > 10.0                                                # the gains matter
    ex.close()


REFUSED = [dict(block=100), dict(block=1000), dict(block=128), dict(block=8192), dict(guard_bins=17), dict(threshold_factor=1.0),
           dict(threshold_factor=0.5), dict(threshold_factor=-4.0), dict(threshold_factor=float("nan")), dict(blank_threshold=-1.0),
           dict(blank_threshold=float("nan"))]


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, excise
    L = gpu.lib()
    for cfg in REFUSED:
        assert EM.resolve(**cfg) is None, cfg
        with pytest.raises(_lib.GmError) as e:
            excise.Excisor(**cfg)
        assert e.value.status == INVALID, cfg
    h = C.c_void_p()
    bad = _lib.ExcisorCfg(1024, 0, 0.0, 0.0, (C.c_uint32 * 4)(0, 0, 1, 0))
    assert L.gm_excisor_create(C.byref(bad), C.byref(h)) == INVALID and not h.value
    assert L.gm_excisor_create(None, C.byref(h)) == INVALID and L.gm_excisor_create(C.byref(_lib.ExcisorCfg()), None) == INVALID
    B, H = 1024, 512
    ex = excise.Excisor(B, blank_threshold=3.0, guard_bins=1)
    p = EM.resolve(B, 1, 0.0, 3.0)
    wa, ws = ex.windows()
    g = _gain_sets(B, 11)[1][1]
    ex.set_gains(g)
    n = 6000
    x = _stream("c32", n, 31)
    room = np.zeros(3 * n, np.complex64)                            # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    d_y = hipbuf.alloc(2 * n * 8, fill=0x5A)
    first = 2500
    n1 = ex.process_dev(d_x, _lib.FMT_C32, first, d_y, 2 * n)
    state = ex.stats()
    assert state["inputs"] == first and state["outputs"] == n1 == EM.plan(B, 0, first) and state["blanked"] > 0
    rest = n - first
    n2 = EM.plan(B, first, rest)
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, cap: L.gm_excisor_process_dev(ex._h, d_in, fmt, n_in, d_out, cap, C.byref(got), None)
    src = d_x + first * 8
    assert call(src, _lib.FMT_I8_REAL, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(src, 7, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(None, _lib.FMT_C32, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(src, _lib.FMT_C32, rest, None, 2 * n) == INVALID
    assert call(src, _lib.FMT_C32, rest, d_y + n1 * 8, n2 - 1) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, rest, d_y + n1 * 8, 0) == OUT_OF_RANGE
    for d_out in (src, src + 8, src - 8 * (n2 - 1), src + rest * 8 - 8):          # d_out overlapping d_in
        assert call(src, _lib.FMT_C32, rest, d_out, n2) == INVALID, d_out - src
    assert got.value == 77 and ex.stats() == state
    assert L.gm_excisor_reset(ex._h, (1 << 62) + 1) == INVALID and ex.stats() == state
    # gains outside [0, 1] or not a number; adapt with n < B, a null pointer, the real format: nothing changes
    for k, v in ((0, -0.01), (B - 1, 1.5), (7, float("nan")), (8, float("inf"))):
        gb = g.copy()
        gb[k] = v
        assert L.gm_excisor_set_gains(ex._h, gb.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.gm_excisor_set_gains(ex._h, None) == INVALID and L.gm_excisor_gains(ex._h, None) == INVALID
    assert L.gm_excisor_adapt_dev(ex._h, d_x, _lib.FMT_C32, B - 1, None) == INVALID
    assert L.gm_excisor_adapt_dev(ex._h, None, _lib.FMT_C32, n, None) == INVALID
    assert L.gm_excisor_adapt_dev(ex._h, d_x, _lib.FMT_I8_REAL, n, None) == INVALID
    assert (_words(ex.gains()) == _words(g)).all() and ex.psd()["n_zeroed"] == 0 and not ex.psd()["P"].any() and ex.stats() == state
    assert (hipbuf.download(d_y + n1 * 8, 64, np.uint8) == 0x5A).all()            # nothing was written
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and ex.stats() == state       # n_in = 0
    # d_out right behind d_in is no overlap; the next good call continues the stream as if nothing had been refused
    assert call(src, _lib.FMT_C32, rest, d_x + n * 8, 2 * n) == 0 and got.value == n2
    ex.synchronize()
    y = np.concatenate([hipbuf.download(d_y, n1 * 8, np.complex64), hipbuf.download(d_x + n * 8, n2 * 8, np.complex64)])
    want, scale, m = EM.run(p, x, wa, ws, g)
    _check("after the refusals", y, want, scale)
    assert ex.stats() == dict(inputs=n, outputs=y.size, blanked=m.blanked)
    # the host-buffer form: the same words, the same refusals
    ex.reset(0)
    assert (_words(ex.process(x)) == _words(y)).all()
    out = np.zeros(4, np.complex64)
    st = L.gm_excisor_process(ex._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_C32, 1000, out.ctypes.data_as(C.c_void_p), 4, None)
    assert st == OUT_OF_RANGE and ex.stats()["inputs"] == n and not out.any()
    assert L.gm_excisor_process(ex._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_I8_REAL, 100, out.ctypes.data_as(C.c_void_p), 4, None) == INVALID
    ex.close()


@pytest.mark.parametrize("with_resampler", [False, True])
def test_the_ring_path(gpu, hipbuf, with_resampler):
    """write_ring with an excisor (and a resampler) into a 2^12 ring, call after call over two wraps, against process_dev(front-end) ->
    process_dev(excisor) (-> process_dev(resampler)) with the same block cuts (a call longer than the ring's 4096-sample staging slot
    is two blocks)"""
    from gnss_sdr_rs_amd import _lib, excise, frontend, resample, tracking
    F_IF, FS = 1.25e6, 8.0e6
    B, H = 256, 128
    ring = tracking.MulticastRingBuffer(1 << 12)
    fe, fe_ref = frontend.DigitalFrontend(F_IF, FS, FS), frontend.DigitalFrontend(F_IF, FS, FS)
    mk = lambda: excise.Excisor(B, blank_threshold=150.0)
    ex, ex_ref = mk(), mk()
    g = _gain_sets(B, 13)[1][1]
    ex.set_gains(g); ex_ref.set_gains(g)
    rs = rs_ref = None
    if with_resampler:
        rs, rs_ref = resample.Resampler(2, 3), resample.Resampler(2, 3)
        calls = [20, 3000, 6000, 4096, 17, 4091, 1234]             # 6000: blocks of 4096 and 1904
    else:
        calls = [20, 3052, 4200, 4096, 17, 4091, 1234]             # 4200 at a multiple of H: blocks of 4096 and 104, 4096 outputs
    x = _stream("i8", sum(calls), 23)
    d_x = hipbuf.upload(x)
    d_mid, d_e, d_y = hipbuf.alloc(4096 * 8), hipbuf.alloc(4352 * 8), hipbuf.alloc(4096 * 8)
    done = head = 0
    for n in calls:
        total = fe.write_ring(ring, x[done:done + n], excisor=ex, resampler=rs)
        ref = []
        for s in range(0, n, 4096):
            k = min(4096, n - s)
            fe_ref.process_dev(d_x + (done + s) * 2, _lib.FMT_I8_IQ, d_mid, k)
            fe_ref.synchronize()
            got = ex_ref.process_dev(d_mid, _lib.FMT_C32, k, d_e, 4352)
            ex_ref.synchronize()
            if with_resampler:
                got = rs_ref.process_dev(d_e, _lib.FMT_C32, got, d_y, 4096) if got else 0
                rs_ref.synchronize()
            ref.append(hipbuf.download(d_y, 4096 * 8, np.complex64)[:got] if with_resampler else hipbuf.download(d_e, 4352 * 8, np.complex64)[:got])
        ref = np.concatenate(ref)
        want_n = ref.size
        assert total == want_n and ring.get_enqueued_head() == head + want_n
        ring.flush()
        assert ring.get_head() == head + want_n
        if n == 20:
            assert want_n == 0 and ring.get_head() == 0              # too short to yield output: the head stays
        assert (_words(ring.copy_to_slice(head, want_n)) == _words(ref)).all(), n
        head += want_n
        done += n
    assert head > 2 * (1 << 12)                                      # the ring wrapped twice
    assert ex.stats() == ex_ref.stats() and ex.stats()["inputs"] == sum(calls) and ex.stats()["blanked"] >= 0
    if with_resampler:
        assert rs.stats() == rs_ref.stats() and rs.stats()["outputs"] == head
    else:
        assert ex.stats()["outputs"] == head
    # more outputs than the ring holds: refused, nothing moved
    with pytest.raises(_lib.GmError) as e:
        fe.write_ring(ring, x[:7000], excisor=ex, resampler=rs)
    assert e.value.status == OUT_OF_RANGE and ring.get_enqueued_head() == head and ex.stats()["inputs"] == sum(calls)
    st = gpu.lib().gm_frontend_write_ring_conditioned(fe._h, ex._h, rs._h if rs else None, ring._h, x.ctypes.data_as(C.c_void_p), 64,
                                                      _lib.FMT_I8_REAL, None)
    assert st == INVALID and ring.get_enqueued_head() == head
    st = gpu.lib().gm_frontend_write_ring_conditioned(fe._h, None, None, ring._h, x.ctypes.data_as(C.c_void_p), 64, _lib.FMT_I8_IQ, None)
    assert st == INVALID and ring.get_enqueued_head() == head
    for h in (fe, fe_ref, ex, ex_ref, ring) + ((rs, rs_ref) if with_resampler else ()):
        h.close()


def test_an_excised_dwell_is_found_again(gpu, hipbuf):
    """The host test's scene (N = 2048, ten periods, a 45 dB-Hz signal at code phase 700 in the 1 kHz bin, a CW 30 dB above the noise):
    Excisor.adapt on the first four periods, process, then a plain search_dev finds the true worker's best cell at code phase 700 in
    the 1 kHz bin; the same search on the jammed dwell does not."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, excise
    x = EM.scene(2, 30.0)
    ex = excise.Excisor(1024, guard_bins=2)
    ex.adapt(x[:4 * EM.N])
    y = ex.process(x)
    r = ex.psd()
    print("adapt on four periods: %d bins flagged, %d zeroed" % (r["n_flagged"], r["n_zeroed"]))
    assert y.size >= EM.DWELL and 5 <= r["n_zeroed"] <= 100
    eng = A.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                              codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == EM.DWELL
    w = EM.SAT["worker"]
    d_y, d_x = hipbuf.upload(y[:EM.DWELL]), hipbuf.upload(x[:EM.DWELL])
    eng.search_dev(d_y, _lib.FMT_C32)
    excised = EM.best_cell(*eng.metrics(), w)
    eng.search_dev(d_x, _lib.FMT_C32)
    jammed = EM.best_cell(*eng.metrics(), w)
    print("GPU: jammed %s, excised %s" % (jammed, excised))
    assert EM.found(excised) and excised[2] >= 6.0
    assert not EM.found(jammed)
    eng.close()
    ex.close()
