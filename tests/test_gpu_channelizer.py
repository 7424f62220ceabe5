"""The polyphase filter bank on the GPU (gm_channelizer, csrc/channelizer_kernels.hip) against the float64 model of
channelizer_model.py, which is handed the library's own filter words (gm_channelizer_taps).

1. Words.  Per output and channel |device - model| <= 1e-5 sum_j |g_j| |xb[n0 + j]|: the project's 1e-5 parity bar relative to the input
   scale.  The derived rounding bound of the float32 arithmetic, (P + 4 log2 M + 8) 2^-24 of that sum, is at most 3.8e-6.  The largest
   fraction seen is printed per shape (on an MI355X: 1.69e-7 at (4, 1, 2) down to 6.5e-8 at (64, 64, 32)).  Every shape of SHAPES, both sample formats (the int8 stream holds -128), the channel lists
   all / one / reversed / GLONASS's fourteen, and call lengths where the tile, halo and history logic can go wrong.  The input is noise
   plus a tone exactly on a channel centre and one half-way between two.
2. Cuts: one call against the same stream in blocks of 1, 7, L - 1, 1000 and 3001, bit for bit; again after a reset to 2^32 - 3 and
   to 2^40 + 12345, where the words also go against the model.
3. Two runs give the same words; a plane's words do not depend on which other channels are listed; an out_stride larger than the count
   leaves the gap untouched (every _feed checks it).
4. Blanking: spikes on tile edges, in the history and across call boundaries; stats equals the model's counts.
5. Every refusal, with state and outputs untouched.
6. The chain: the host test's scene of seed 1 through Channelizer, then a plain search_dev per plane at fft_size 2000."""
import ctypes as C
import math

import numpy as np
import pytest

import channelizer_model as CM

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
BAR = 1e-5

# (M, D, P)
SHAPES = [(4, 1, 2), (4, 3, 4), (8, 4, 16), (8, 8, 8), (16, 5, 32), (32, 9, 16), (32, 16, 16), (64, 18, 16), (64, 64, 32)]
GAP = 5                                                   # words between a plane's capacity and the next plane


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream(fmt, n, seed, M):
    """noise + a tone exactly on the centre of channel M/4 + 1 + a tone half-way between channels M - 2 and M - 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    k1, k2 = M // 4 + 1, M - 1.5
    tones = np.exp(2j * np.pi * ((k1 * t) % M) / M) + np.exp(2j * np.pi * ((k2 * t) % M) / M + 0.3j)
    if fmt == "i8":
        v = 20.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 30.0 * tones
        x = np.stack([np.clip(np.rint(v.real), -128, 127), np.clip(np.rint(v.imag), -128, 127)], axis=1).astype(np.int8)
        if n > 2:
            x[n // 3] = (-128, 127)
            x[n // 2] = (-128, -128)
        return x
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n) + 1.5 * tones).astype(np.complex64)


def _bps(fmt):
    return 2 if fmt == "i8" else 8


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, ch, d_x, fmt, n, blocks=None):
    """the n samples at d_x through ch.process_dev in blocks (None: one call) -> complex64 [C][n_out]; every plane's outputs lie behind
    each other in its row of one [C][stride] device buffer whose other words must stay as they were filled"""
    planes = len(ch.channels)
    cap = n // ch.decim + 2
    stride = cap + GAP
    d_y = hipbuf.alloc(planes * stride * 8, fill=0x5A)
    done = got = 0
    step = blocks or max(n, 1)
    while True:
        k = min(step, n - done)
        got += ch.process_dev(d_x + done * _bps(fmt), _fmt(fmt), k, d_y + got * 8, stride, cap - got)
        done += k
        if done >= n:
            break
    ch.synchronize()
    raw = hipbuf.download(d_y, planes * stride * 8, np.complex64).reshape(planes, stride)
    assert (raw[:, got:].view(np.uint8) == 0x5A).all()                  # nothing behind a plane's last output
    return raw[:, :got].copy()


def _check(tag, got, want, weight):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not got.size:
        return 0.0
    assert np.isfinite(got.view(np.float32)).all(), tag
    frac = np.abs(got.astype(np.complex128) - want) / np.maximum(weight[None, :], 1e-300)
    worst = float(frac.max())
    assert worst <= BAR, (tag, worst)
    return worst


def _lengths(p):
    """call lengths of a fresh stream: one input, no output yet (L/2 - 1, L/2), the first output, a call shorter than the history, one
    tile of outputs give or take an input, the second tile's first output, and about 20000 with a ragged tail"""
    L, D, tile = p["L"], p["D"], CM.tile_outputs(p)
    n_tile = L // 2 + (tile - 1) * D + 1
    assert CM.total_out(p, n_tile - 1) == tile - 1 and CM.total_out(p, n_tile) == tile
    assert CM.total_out(p, L // 2) == 0 and CM.total_out(p, L // 2 + 1) == 1
    return [1, L // 2 - 1, L // 2, L // 2 + 1, L - 1, n_tile - 1, n_tile, n_tile + 1, n_tile + D, 20011]


def _lists(M):
    from gnss_sdr_rs_amd import channelizer
    lists = dict(all=None, one=[M - 1], reversed=list(range(M - 1, -1, -1)))
    if M >= 16:
        lists["glonass"] = channelizer.glonass_channels(M)
    return lists


@pytest.mark.parametrize("shape", SHAPES)
def test_words_against_the_model(gpu, hipbuf, shape):
    from gnss_sdr_rs_amd import channelizer
    M, D, P = shape
    worst = 0.0
    planes_of_all = {}
    for name, channels in _lists(M).items():
        ch = channelizer.Channelizer(M, D, channels=channels, taps_per_branch=P)
        p = CM.resolve(M, D, channels=channels, taps_per_branch=P)
        assert (ch.taps_per_branch, ch.n_taps, ch.channels) == (p["P"], p["L"], p["channels"])
        g = ch.taps()
        assert (_words(g) == _words(CM.design(p).astype(np.float32))).all()
        lengths = _lengths(p)
        for fmt in ("i8", "c32"):
            x = _stream(fmt, lengths[-1], 17 + M + D, M)
            d_x = hipbuf.upload(x)
            for n in lengths:
                ch.reset(0)
                got = _feed(hipbuf, ch, d_x, fmt, n)
                want, weight, m = CM.run(p, g, x[:n])
                worst = max(worst, _check((shape, name, fmt, n), got, want, weight))
                assert ch.stats() == dict(inputs=n, outputs=CM.total_out(p, n), blanked=0)
                if n == lengths[-1]:
                    # a plane's words do not depend on which other channels are listed
                    if name == "all":
                        planes_of_all[fmt] = got
                    else:
                        assert (_words(got) == _words(planes_of_all[fmt][p["channels"]])).all(), (shape, name, fmt)
                    ch.reset(0)
                    assert (_words(_feed(hipbuf, ch, d_x, fmt, n)) == _words(got)).all()       # a second run: the same words
            assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()       # the input is only read
        ch.close()
    derived = (P + 4 * math.log2(M) + 8) * 2.0 ** -24
    print("%s: tile %d outputs, largest |device - model| / sum |g||x| = %.3g (derived bound %.3g, bar %.0e)"
          % (shape, CM.tile_outputs(CM.resolve(M, D, taps_per_branch=P)), worst, derived, BAR))


def test_the_tones_land_where_the_definition_puts_them(gpu, hipbuf):
    """a tone of amplitude 1.5 on the centre of channel k1 comes out of plane k1 as the constant 1.5 (the channel's phase runs on the
    absolute input index, the filter's DC gain is 1) and of the planes two away as nothing"""
    from gnss_sdr_rs_amd import channelizer
    M, D = 32, 9
    ch = channelizer.Channelizer(M, D)
    n = 8000
    t = np.arange(n, dtype=np.float64)
    k1 = M // 4 + 1
    x = (1.5 * np.exp(2j * np.pi * ((k1 * t) % M) / M)).astype(np.complex64)
    y = ch.process(x)
    settled = slice(ch.n_taps // D + 1, None)
    assert y.shape == (M, CM.total_out(CM.resolve(M, D), n))
    assert np.abs(y[k1] - 1.5)[settled].max() <= 1e-5 * 1.5 * 2           # sum |g| |x| is below 2 x 1.5
    assert np.abs(y[(k1 + 2) % M])[settled].max() <= 1e-3 and np.abs(y[(k1 - 2) % M])[settled].max() <= 1e-3
    ch.close()


SPLITS = (1, 7, None, 1000, 3001)          # None: L - 1


@pytest.mark.parametrize("shape,fmt", [((4, 3, 4), "i8"), ((16, 5, 32), "c32"), ((32, 9, 16), "i8"), ((64, 64, 32), "c32")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, shape, fmt):
    from gnss_sdr_rs_amd import channelizer
    M, D, P = shape
    channels = None if M != 32 else channelizer.glonass_channels(M)
    ch = channelizer.Channelizer(M, D, channels=channels, taps_per_branch=P)
    p = CM.resolve(M, D, channels=channels, taps_per_branch=P)
    g = ch.taps()
    n = 6007
    x = _stream(fmt, n, 5, M)
    d_x = hipbuf.upload(x)
    for index in (0, (1 << 32) - 3, (1 << 40) + 12345):
        ch.reset(index)
        whole = _feed(hipbuf, ch, d_x, fmt, n)
        want, weight, m = CM.run(p, g, x, input_index=index)
        assert whole.shape[1] == m.outputs == CM.plan(p, index, n) > 0
        _check((shape, index), whole, want, weight)
        for blocks in SPLITS:
            ch.reset(index)
            got = _feed(hipbuf, ch, d_x, fmt, n, blocks or p["L"] - 1)
            assert (_words(got) == _words(whole)).all(), (shape, index, blocks)
            assert ch.stats() == dict(inputs=n, outputs=whole.shape[1], blanked=0)
    ch.close()


def _spiky(fmt, p, n):
    """a quiet stream (|re|, |im| <= 20) with spikes inside the first tile, around the inputs the second tile starts and the first tile
    ends at (both tiles' halos), around the cuts of the 1000-sample split (the history), and the pairs that sit exactly at / just above
    the threshold 100"""
    rng = np.random.default_rng(9)
    x = rng.integers(-20, 21, (n, 2)).astype(np.int8)
    L, D, tile = p["L"], p["D"], CM.tile_outputs(p)
    first = tile * D - (L // 2 - 1)                               # n0 of the second tile's first output
    last = (tile - 1) * D + L // 2                                # the last input of the first tile's last output
    spikes = [0, 700, first - 1, first, first + 1, last - 1, last, last + 1, tile * D, 999, 1000, 1001, 1999, 2000, 2000 + L // 2, 2999, n - 1]
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
    from gnss_sdr_rs_amd import channelizer
    M, D = 32, 9
    channels = [3, 4, 27, 10]
    ch = channelizer.Channelizer(M, D, channels=channels, blank_threshold=100.0)
    p = CM.resolve(M, D, channels=channels, blank_threshold=100.0)
    assert CM.tile_outputs(p) == 256 and p["L"] == 512
    g = ch.taps()
    n = 7003
    x, n_blank = _spiky(fmt, p, n)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, ch, d_x, fmt, n)
    want, weight, m = CM.run(p, g, x)
    assert m.blanked == n_blank and whole.shape[1] > 2 * 256
    _check((fmt, "whole"), whole, want, weight)
    assert ch.stats() == dict(inputs=n, outputs=whole.shape[1], blanked=n_blank)
    for blocks in SPLITS:
        ch.reset(0)
        got = _feed(hipbuf, ch, d_x, fmt, n, blocks or p["L"] - 1)
        assert (_words(got) == _words(whole)).all(), blocks
        assert ch.stats() == dict(inputs=n, outputs=whole.shape[1], blanked=n_blank), blocks      # each input once, whatever the cuts
    # the blanked samples matter: the model without blanking is somewhere else
    plain_p = CM.resolve(M, D, channels=channels)
    want_plain, weight_plain, _ = CM.run(plain_p, g, x)
    assert np.abs(want_plain - want).max() > 1.0
    # threshold 0 is a handle without blanking
    off, zero = channelizer.Channelizer(M, D, channels=channels), channelizer.Channelizer(M, D, channels=channels, blank_threshold=0.0)
    a, b = _feed(hipbuf, off, d_x, fmt, n), _feed(hipbuf, zero, d_x, fmt, n)
    assert (_words(a) == _words(b)).all() and zero.stats()["blanked"] == 0
    _check((fmt, "off"), a, want_plain, weight_plain)
    for h in (ch, off, zero):
        h.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, channelizer
    import test_channelizer_host as TH
    L = gpu.lib()
    for cfg in TH.REFUSED:
        with pytest.raises(_lib.GmError) as e:
            channelizer.Channelizer(**cfg)
        assert e.value.status == INVALID, cfg
    h = C.c_void_p()
    ok = _lib.ChannelizerCfg(32, 9, 0, 0.0, 0.0, 0.0, 0, 0, None)
    assert L.gm_channelizer_create(None, C.byref(h)) == INVALID and L.gm_channelizer_create(C.byref(ok), None) == INVALID
    assert L.gm_channelizer_create(C.byref(_lib.ChannelizerCfg(32, 9, 0, 0.0, 0.0, 0.0, 0, 1, None)), C.byref(h)) == INVALID and not h.value
    M, D = 16, 5
    channels = [2, 15, 7]
    ch = channelizer.Channelizer(M, D, channels=channels, taps_per_branch=8, blank_threshold=3.0)
    p = CM.resolve(M, D, channels=channels, taps_per_branch=8, blank_threshold=3.0)
    g = ch.taps()
    n = 2500
    x = _stream("c32", n, 31, M)
    room = np.zeros(n + 3 * n, np.complex64)                        # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    stride = n
    d_y = hipbuf.alloc(3 * stride * 8, fill=0x5A)
    first = 1000
    n1 = ch.process_dev(d_x, _lib.FMT_C32, first, d_y, stride, stride)
    state = ch.stats()
    assert state["inputs"] == first and state["outputs"] == n1 == CM.plan(p, 0, first) and state["blanked"] > 0
    rest = n - first
    n2 = CM.plan(p, first, rest)
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, strd, cap: L.gm_channelizer_process_dev(ch._h, d_in, fmt, n_in, d_out, strd, cap, C.byref(got), None)
    src = d_x + first * 8
    out = d_y + n1 * 8
    assert call(src, _lib.FMT_I8_REAL, rest, out, stride, n2) == INVALID
    assert call(src, 7, rest, out, stride, n2) == INVALID
    assert call(None, _lib.FMT_C32, rest, out, stride, n2) == INVALID
    assert call(src, _lib.FMT_C32, rest, None, stride, n2) == INVALID
    assert call(src, _lib.FMT_C32, rest, out, stride, n2 - 1) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, rest, out, stride, 0) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, rest, out, n2 - 1, n2) == OUT_OF_RANGE                       # out_stride below out_cap
    assert call(src, _lib.FMT_C32, (1 << 31) + 1, out, stride, n2) == INVALID
    # the C x out_stride region overlapping d_in: its first plane, its last plane, its last word, the input's last word
    for d_out in (src, src + 8, src - 8 * (3 * n2 - 1), src + rest * 8 - 8, src - 8 * 2 * n2):
        assert call(src, _lib.FMT_C32, rest, d_out, n2, n2) == INVALID, d_out - src
    assert got.value == 77 and ch.stats() == state
    assert L.gm_channelizer_reset(ch._h, (1 << 62) + 1) == INVALID and ch.stats() == state
    raw = hipbuf.download(d_y, 3 * stride * 8, np.complex64).reshape(3, stride)
    assert (raw[:, n1:].view(np.uint8) == 0x5A).all()               # nothing was written
    assert call(None, _lib.FMT_C32, 0, None, 0, 0) == 0 and got.value == 0 and ch.stats() == state      # n_in = 0
    # d_out right behind d_in is no overlap; the next good call continues the stream as if nothing had been refused
    assert call(src, _lib.FMT_C32, rest, d_x + n * 8, n, n) == 0 and got.value == n2
    ch.synchronize()
    tail = hipbuf.download(d_x + n * 8, 3 * n * 8, np.complex64).reshape(3, n)[:, :n2]
    y = np.concatenate([raw[:, :n1], tail], axis=1)
    want, weight, m = CM.run(p, g, x)
    _check("after the refusals", y, want, weight)
    assert ch.stats() == dict(inputs=n, outputs=y.shape[1], blanked=m.blanked)
    # the host-buffer form: the same words, the same refusals
    ch.reset(0)
    assert (_words(ch.process(x)) == _words(y)).all()
    small = np.zeros((3, 4), np.complex64)
    st = L.gm_channelizer_process(ch._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_C32, 200, small.ctypes.data_as(C.c_void_p), 4, None)
    assert st == OUT_OF_RANGE and ch.stats()["inputs"] == n and not small.any()
    assert L.gm_channelizer_process(ch._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_I8_REAL, 100, small.ctypes.data_as(C.c_void_p), 4, None) == INVALID
    ch.close()


def test_the_glonass_scene_through_the_bank_and_a_plain_search(gpu, hipbuf):
    """The host test's scene of seed 1 (three L1OF signals on channels 3, 4 and 27 of an 18 Msps int8 capture): Channelizer (32, 9, 16),
    then a plain search_dev per plane at fft_size 2000 with the GLONASS code.  The cells are the model's, and the peak-to-mean is within
    1e-3 relative of the model's search of the model's planes with the handle's own replica and mix tables: both stages meet the 1e-5
    parity bar, which implies that with two orders of margin."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, channelizer
    import acq_model as AM
    import test_channelizer_host as TH
    r = TH.scene_run(1)
    channels = r["p"]["channels"]
    ch = channelizer.Channelizer(CM.M, CM.D, channels=channels, taps_per_branch=CM.P)
    assert (_words(ch.taps()) == _words(r["g"])).all()
    d_x = hipbuf.upload(r["x"])
    n_out = CM.total_out(r["p"], CM.N_IN)
    d_y = hipbuf.alloc(len(channels) * n_out * 8)
    assert ch.process_dev(d_x, _lib.FMT_I8_IQ, CM.N_IN, d_y, n_out, n_out) == n_out
    ch.synchronize()
    chips = channelizer.glonass_code()
    eng = A.AcquisitionEngine(CM.FS / CM.D, 0.0, CM.N, doppler_hz=CM.DOP.astype(np.float32), prn_ids=[1], n_integrations=CM.M_SEARCH,
                              codes=chips, code_rate=511e3)
    assert eng.dwell_samples == CM.M_SEARCH * CM.N <= n_out
    replica = AM.sample_codes(chips, 511e3, CM.FS / CM.D, CM.N)[0]
    tables = eng.tables()
    for i, k in enumerate(channels):
        eng.search_dev(d_y + i * n_out * 8, _lib.FMT_C32)                  # a plane pointer goes straight into the search
        mx, am, sm = eng.metrics()
        ratio = mx[0].astype(np.float64) * CM.N / sm[0].astype(np.float64)
        b = int(np.argmax(ratio))
        got = (b, int(am[0][b]), float(ratio[b]))
        want = CM.search(r["y"][i], replica=replica, tables=tables)
        print("channel %d: GPU %s, model %s, model with its own replica %s" % (k, got, want, r["cells"][k]))
        if k != CM.EMPTY:
            assert got[:2] == want[:2] == r["cells"][k][:2] == (CM.EXPECTED[k][1], CM.EXPECTED[k][0])
            assert abs(got[2] - want[2]) <= 1e-3 * want[2]
            assert got[2] > CM.DETECT
        else:
            assert got[2] < CM.DETECT
    eng.close()
    ch.close()
