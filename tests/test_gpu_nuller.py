"""The adaptive spatial nuller on the GPU (gm_nuller, csrc/nuller_kernels.hip) against the float64 model of nuller_model.py, on noise
plus a rank-one jammer 30 dB above it.  Each step is held to its own bar:

  R   against the float64 sum:                                   |dR[i][j]| <= 1e-5 sum_t |x_i| |x_j|   (derived: (B/256 + 12) 2^-24)
  w   against the model's w computed from the DEVICE's R words:  |dw[a]|    <= 2^-22 max_a |w[a]|       (one f32 rounding + the f64 solve)
  y   against the model handed the device's w words:             |dy|       <= 1e-5 sum_a |w[a]| |x_a|  (derived: (A + 2) 2^-24)

1. Shapes: A = 2, 3, 4, 8 at B = 256 and 1024, A = 5, 6, 7 at B = 256, A = 8 at B = 16384; both formats (the int8 stream holds -128),
   loading 1e-4 and 1e-2, e_0 and a random complex s, call lengths 1, B - 1, B, B + 1, 3B - 1, 5B + 7.  The largest fraction of each bar
   is printed per shape.
2. Cuts: one call against calls of 1, 7, B - 1, 1000 and 3001 time samples, bit for bit, for y, the captured R and w, and stats; again
   after a reset to 2^32 - 3 and to 2^40 + 12345, where the words also go against the model.  Two runs give the same words.
3. Input pointers that are not aligned for the wide loads.
4. Static mode; a switch to it and back; a capture in static mode writes w only.
5. An all-zero block.
6. Every refusal, with state and outputs untouched.
7. The chain: the host test's jammed scenes of seed 1 through Nuller.process, then a plain search_dev at fft_size 2048."""
import ctypes as C

import numpy as np
import pytest

import nuller_model as NM

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
BAR_R, BAR_W, BAR_Y = 1e-5, 2.0 ** -22, 1e-5
GAP = 5


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream(fmt, n, A, seed):
    """[n, A] complex64 or [n, A, 2] int8: unit noise (int8: 3 LSB) plus a rank-one white jammer 30 dB above it"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))
    jam = 10.0 ** 1.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + jam[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    if fmt == "i8":
        v = 1.2 * x
        q = np.stack([np.clip(np.rint(v.real), -128, 127), np.clip(np.rint(v.imag), -128, 127)], axis=-1).astype(np.int8)
        if n > 2:
            q[n // 3, A - 1] = (-128, 127)
            q[n // 2, 0] = (-128, -128)
        return q
    return x.astype(np.complex64)


def _bps(fmt, A):
    return A * (2 if fmt == "i8" else 8)


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, nl, d_x, fmt, n, step=None):
    """the n time samples at d_x through nl.process_dev in calls of `step` (None: one call), each call's blocks captured behind the
    earlier calls' -> (y, R [blocks, A, A], w [blocks, A]); words behind the outputs and behind the captured blocks must stay as filled"""
    A, B = nl.n_antennas, nl.block
    cap = n + B
    nb_cap = cap // B + 1
    d_y = hipbuf.alloc((cap + GAP) * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(nb_cap * A * A * 8, fill=0x5A), hipbuf.alloc(nb_cap * A * 8, fill=0x5A)
    done = got = 0
    step = step or max(n, 1)
    while True:
        k = min(step, n - done)
        nb = got // B
        nl.capture(d_R + nb * A * A * 8, d_w + nb * A * 8, nb_cap - nb)
        got += nl.process_dev(d_x + done * _bps(fmt, A), _fmt(fmt), k, d_y + got * 8, cap - got)
        done += k
        if done >= n:
            break
    nl.synchronize()
    nl.capture(None, None, 0)
    nb = got // B
    raw = hipbuf.download(d_y, (cap + GAP) * 8, np.complex64)
    R = hipbuf.download(d_R, nb_cap * A * A * 8, np.complex64).reshape(nb_cap, A, A)
    w = hipbuf.download(d_w, nb_cap * A * 8, np.complex64).reshape(nb_cap, A)
    assert (raw[got:].view(np.uint8) == 0x5A).all() and (w[nb:].view(np.uint8) == 0x5A).all() and (R[nb:].view(np.uint8) == 0x5A).all()
    return raw[:got].copy(), R[:nb].copy(), w[:nb].copy()


def _check(tag, p, x, y, R, w, input_index=0):
    """the three bars -> the largest fraction of each"""
    m = NM.run(p, x, input_index=input_index)
    nb = m["xb"].shape[0]
    assert y.shape == (nb * p["B"],) and R.shape == (nb, p["A"], p["A"]) and w.shape == (nb, p["A"]), tag
    if not nb:
        return 0.0, 0.0, 0.0
    for a in (y, R, w):
        assert np.isfinite(a.view(np.float32)).all(), tag
    assert (R == np.conj(np.swapaxes(R, 1, 2))).all() and not R[:, np.arange(p["A"]), np.arange(p["A"])].imag.any(), tag
    fr = float((np.abs(R.astype(np.complex128) - m["R"]) / np.maximum(m["R_weight"], 1e-300)).max())
    wm = NM.weights(p, R)                                              # from the device's R words
    fw = float((np.abs(w.astype(np.complex128) - wm) / np.abs(wm).max(axis=1, keepdims=True)).max())
    ym, yw = NM.combine(m["xb"], w)                                    # handed the device's w words
    fy = float((np.abs(y.astype(np.complex128) - ym) / np.maximum(yw, 1e-300)).max())
    print("%s: R %.3g of its bar, w %.3g, y %.3g" % (tag, fr / BAR_R, fw / BAR_W, fy / BAR_Y))
    assert fr <= BAR_R and fw <= BAR_W and fy <= BAR_Y, (tag, fr, fw, fy)
    return fr / BAR_R, fw / BAR_W, fy / BAR_Y


SHAPES = [(2, 256), (2, 1024), (3, 256), (3, 1024), (4, 256), (4, 1024), (8, 256), (8, 1024), (5, 256), (6, 256), (7, 256), (8, 16384)]


@pytest.mark.parametrize("shape", SHAPES)
def test_words_against_the_model(gpu, hipbuf, shape):
    from gnss_sdr_rs_amd import nuller
    A, B = shape
    lengths = [1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7] if B < 16384 else [B - 1, B + 1, 2 * B + 5]
    s = (np.random.default_rng(A).standard_normal(A) + 1j * np.random.default_rng(B).standard_normal(A)).astype(np.complex64)
    worst = np.zeros(3)
    for fmt in ("i8", "c32"):
        x = _stream(fmt, lengths[-1], A, 100 * A + B % 97)
        d_x = hipbuf.upload(x)
        for loading, steering in ((1e-4, None), (1e-2, s), (1e-2, None), (1e-4, s)):
            nl = nuller.Nuller(A, B, loading, steering)
            p = NM.resolve(A, B, loading, steering)
            assert (nl.block, nl.loading) == (p["B"], p["loading"])
            for n in (lengths if steering is None and loading == 1e-4 else lengths[-1:]):
                nl.reset(0)
                y, R, w = _feed(hipbuf, nl, d_x, fmt, n)
                worst = np.maximum(worst, _check((shape, fmt, loading, steering is not None, n), p, x[:n], y, R, w))
                assert nl.stats() == dict(inputs=n, outputs=NM.total_out(p, n), blocks=n // B)
                if steering is None:
                    assert (w[:, 0].real == np.float32(1.0)).all()
            nl.reset(0)
            again = _feed(hipbuf, nl, d_x, fmt, lengths[-1])           # a second run: the same words
            assert all((_words(a) == _words(b)).all() for a, b in zip(again, (y, R, w)))
            nl.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()       # the input is only read
    print("%s: largest fractions of the bars: R %.3g (derived bound %.3g of the bar), w %.3g, y %.3g (derived %.3g)"
          % (shape, worst[0], (B / 256 + 12) * 2.0 ** -24 / BAR_R, worst[1], worst[2], (A + 2) * 2.0 ** -24 / BAR_Y))


@pytest.mark.parametrize("A,B,fmt", [(3, 256, "i8"), (4, 1024, "c32"), (8, 256, "c32"), (2, 1024, "i8")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, A, B, fmt):
    from gnss_sdr_rs_amd import nuller
    nl = nuller.Nuller(A, B)
    p = NM.resolve(A, B)
    n = 6007
    x = _stream(fmt, n, A, 5)
    d_x = hipbuf.upload(x)
    for index in (0, (1 << 32) - 3, (1 << 40) + 12345):
        nl.reset(index)
        whole = _feed(hipbuf, nl, d_x, fmt, n)
        assert whole[0].size == NM.plan(p, index, n) > 0
        _check((A, B, fmt, index), p, x, *whole, input_index=index)
        state = nl.stats()
        assert state == dict(inputs=n, outputs=whole[0].size, blocks=whole[0].size // B)
        for step in (1, 7, B - 1, 1000, 3001):
            nl.reset(index)
            got = _feed(hipbuf, nl, d_x, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, whole)), (index, step)
            assert nl.stats() == state
    nl.close()


@pytest.mark.parametrize("A,fmt", [(3, "i8"), (8, "i8"), (4, "i8"), (4, "c32"), (3, "c32")])
def test_input_pointers_that_are_not_aligned(gpu, hipbuf, A, fmt):
    """the stream one, two and three elements behind an aligned address: the same words as at the aligned address"""
    from gnss_sdr_rs_amd import nuller
    B, n = 256, 3 * 256 + 11
    nl = nuller.Nuller(A, B)
    p = NM.resolve(A, B)
    x = _stream(fmt, n, A, 77)
    want = _feed(hipbuf, nl, hipbuf.upload(x), fmt, n)
    _check((A, fmt, "aligned"), p, x, *want)
    flat = x.reshape((n * A,) + x.shape[2:])
    for lead in (1, 2, 3):
        padded = np.concatenate([np.zeros((lead,) + flat.shape[1:], flat.dtype), flat])
        d = hipbuf.upload(padded) + lead * (2 if fmt == "i8" else 8)
        for step in (None, 100):
            nl.reset(0)
            got = _feed(hipbuf, nl, d, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, want)), (lead, step)
    nl.close()


def test_static_mode(gpu, hipbuf):
    from gnss_sdr_rs_amd import nuller
    rng = np.random.default_rng(12)
    for A, B, fmt in ((4, 256, "c32"), (3, 256, "i8"), (8, 1024, "i8")):
        n = 4 * B + 9
        x = _stream(fmt, n, A, 3)
        d_x = hipbuf.upload(x)
        nl, ref = nuller.Nuller(A, B), nuller.Nuller(A, B)
        p = NM.resolve(A, B)
        adaptive = _feed(hipbuf, ref, d_x, fmt, n)
        w = (rng.standard_normal(A) + 1j * rng.standard_normal(A)).astype(np.complex64)
        nl.set_weights(w)
        y, R, wc = _feed(hipbuf, nl, d_x, fmt, n, 1000)
        m = NM.run(p, x, static_w=w)
        assert y.shape == m["y"].shape and nl.stats() == dict(inputs=n, outputs=4 * B, blocks=4)      # counts and delivery unchanged
        frac = float((np.abs(y.astype(np.complex128) - m["y"]) / m["y_weight"]).max())
        print("static (%d, %d, %s): y %.3g of its bar" % (A, B, fmt, frac / BAR_Y))
        assert frac <= BAR_Y
        assert (_words(wc) == _words(np.tile(w, (4, 1)))).all()         # the capture holds the installed words
        assert (R.view(np.uint8) == 0x5A).all()                         # and R is not written in static mode
        # static for the first two blocks, adaptive again for the rest: the adaptive handle's words, bit for bit
        nl.reset(0)
        first = _feed(hipbuf, nl, d_x, fmt, 2 * B + 5)
        assert (_words(first[0]) == _words(y[:2 * B])).all()
        nl.set_weights(None)
        rest = _feed(hipbuf, nl, d_x + (2 * B + 5) * _bps(fmt, A), fmt, n - 2 * B - 5)
        assert all((_words(a) == _words(b[2:] if b.ndim > 1 else b[2 * B:])).all() for a, b in zip(rest, adaptive))
        # the host-buffer form: the same words in both modes
        nl.reset(0)
        hy, hR, hw = nl.process(x, want_blocks=True)
        assert all((_words(a) == _words(b)).all() for a, b in zip((hy, hR, hw), adaptive))
        nl.reset(0)
        assert (_words(nl.process(x)) == _words(adaptive[0])).all()
        nl.set_weights(w)
        nl.reset(0)
        hy, hR, hw = nl.process(x, want_blocks=True)
        assert (_words(hy) == _words(y)).all() and (_words(hw) == _words(wc)).all() and not hR.any()
        nl.close()
        ref.close()


def test_an_all_zero_block(gpu, hipbuf):
    from gnss_sdr_rs_amd import nuller
    A, B = 4, 256
    s = np.array([1 + 1j, -0.5j, 0.25, 2.0], np.complex64)
    for fmt in ("c32", "i8"):
        x = _stream(fmt, 3 * B, A, 8)
        x[B:2 * B] = 0
        for steering in (None, s):
            nl = nuller.Nuller(A, B, steering=steering)
            p = NM.resolve(A, B, steering=steering)
            y, R, w = _feed(hipbuf, nl, hipbuf.upload(x), fmt, 3 * B)
            _check((fmt, steering is not None), p, x, y, R, w)
            want = p["s"] / np.vdot(p["s"], p["s"]).real
            assert not R[1].any() and not y[B:2 * B].any() and y[:B].any() and y[2 * B:].any()
            assert np.abs(w[1].astype(np.complex128) - want).max() <= BAR_W * np.abs(want).max()
            nl.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, nuller
    import test_nuller_host as TH
    L = gpu.lib()
    for cfg in TH.REFUSED:
        with pytest.raises(_lib.GmError) as e:
            nuller.Nuller(**cfg)
        assert e.value.status == INVALID, cfg
    h = C.c_void_p()
    ok = _lib.NullerCfg(4, 256, 0.0, 0, None)
    assert L.gm_nuller_create(None, C.byref(h)) == INVALID and L.gm_nuller_create(C.byref(ok), None) == INVALID
    assert L.gm_nuller_create(C.byref(_lib.NullerCfg(4, 256, 0.0, 1, None)), C.byref(h)) == INVALID and not h.value
    A, B = 4, 256
    nl = nuller.Nuller(A, B)
    p = NM.resolve(A, B)
    n = 5 * B + 40
    x = _stream("c32", n, A, 31)
    room = np.zeros((2 * n, A), np.complex64)                      # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    d_y = hipbuf.alloc(n * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(8 * A * A * 8, fill=0x5A), hipbuf.alloc(8 * A * 8, fill=0x5A)
    first = B + 100
    nl.capture(d_R, d_w, 8)
    n1 = nl.process_dev(d_x, _lib.FMT_C32, first, d_y, n)
    state = nl.stats()
    assert state == dict(inputs=first, outputs=B, blocks=1) and n1 == B
    R1, w1 = hipbuf.download(d_R, 8 * A * A * 8, np.complex64), hipbuf.download(d_w, 8 * A * 8, np.complex64)
    rest = n - first
    n2 = NM.plan(p, first, rest)
    assert n2 == 4 * B
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, cap: L.gm_nuller_process_dev(nl._h, d_in, fmt, n_in, d_out, cap, C.byref(got), None)
    src = d_x + first * A * 8
    out = d_y + n1 * 8
    assert call(src, _lib.FMT_I8_REAL, rest, out, n2) == INVALID
    assert call(src, 7, rest, out, n2) == INVALID
    assert call(None, _lib.FMT_C32, rest, out, n2) == INVALID
    assert call(src, _lib.FMT_C32, rest, None, n2) == INVALID
    assert call(src, _lib.FMT_C32, rest, out, n2 - 1) == OUT_OF_RANGE           # out_cap one below the count
    assert call(src, _lib.FMT_C32, rest, out, 0) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, (1 << 31) + 1, out, n2) == INVALID
    for d_out in (src, src + 8, src - 8 * (n2 - 1), src + rest * A * 8 - 8):    # d_out overlapping d_in, at either end
        assert call(src, _lib.FMT_C32, rest, d_out, n2) == INVALID, d_out - src
    nl.capture(d_R, d_w, 3)                                                      # a capture smaller than the call's four blocks
    assert call(src, _lib.FMT_C32, rest, out, n2) == OUT_OF_RANGE
    nl.capture(d_R, d_w, 8)
    assert L.gm_nuller_capture(nl._h, d_R, None, 8) == INVALID and L.gm_nuller_capture(nl._h, None, d_w, 8) == INVALID
    assert L.gm_nuller_capture(nl._h, d_R, d_w, 0) == INVALID and L.gm_nuller_capture(nl._h, None, None, 8) == INVALID
    bad = np.array([1, 0, np.nan, 0], np.complex64)
    assert L.gm_nuller_set_weights(nl._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    bad[2] = complex(0, np.inf)
    assert L.gm_nuller_set_weights(nl._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    assert got.value == 77 and nl.stats() == state
    assert L.gm_nuller_reset(nl._h, (1 << 62) + 1) == INVALID and nl.stats() == state
    raw = hipbuf.download(d_y, n * 8, np.complex64)
    assert (raw[n1:].view(np.uint8) == 0x5A).all()                  # nothing was written
    assert (_words(hipbuf.download(d_R, 8 * A * A * 8, np.complex64)) == _words(R1)).all()
    assert (_words(hipbuf.download(d_w, 8 * A * 8, np.complex64)) == _words(w1)).all()
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and nl.stats() == state      # n_in = 0
    # the next good call continues the stream as if nothing had been refused (the refused set_weights left the adaptive rule);
    # d_out right behind d_in is no overlap
    assert call(src, _lib.FMT_C32, rest, d_x + n * A * 8, n2) == 0 and got.value == n2
    nl.synchronize()
    tail = hipbuf.download(d_x + n * A * 8, n2 * 8, np.complex64)
    y = np.concatenate([raw[:n1], tail])
    R = np.concatenate([R1.reshape(8, A, A)[:1], hipbuf.download(d_R, 4 * A * A * 8, np.complex64).reshape(4, A, A)])
    w = np.concatenate([w1.reshape(8, A)[:1], hipbuf.download(d_w, 4 * A * 8, np.complex64).reshape(4, A)])
    _check("after the refusals", p, x, y, R, w)
    assert nl.stats() == dict(inputs=n, outputs=5 * B, blocks=5)
    # the host-buffer form: the same words, the same refusals
    nl.reset(0)
    hy, hR, hw = nl.process(x, want_blocks=True)
    assert (_words(hy) == _words(y)).all() and (_words(hR) == _words(R)).all() and (_words(hw) == _words(w)).all()
    small = np.zeros(4, np.complex64)
    xp = x.ctypes.data_as(C.c_void_p)
    sp = small.ctypes.data_as(C.c_void_p)
    assert L.gm_nuller_process(nl._h, xp, _lib.FMT_C32, 300, sp, 4, None, None, None, 0) == OUT_OF_RANGE
    assert L.gm_nuller_process(nl._h, xp, _lib.FMT_I8_REAL, 100, sp, 4, None, None, None, 0) == INVALID
    big = np.zeros(2 * B, np.complex64)
    wbuf = np.zeros((1, A), np.complex64)
    assert L.gm_nuller_process(nl._h, xp, _lib.FMT_C32, 2 * B, big.ctypes.data_as(C.c_void_p), 2 * B, None, None,
                               wbuf.ctypes.data_as(C.c_void_p), 1) == OUT_OF_RANGE
    assert nl.stats()["inputs"] == n and not small.any() and not big.any() and not wbuf.any()
    nl.close()


def test_the_jammed_scenes_through_the_nuller_and_a_plain_search(gpu, hipbuf):
    """Seed 1's c32 J/N 40 dB and int8 J/N 30 dB scenes through Nuller.process (A = 4, B = 1024, loading 1e-4, e_0) and a plain
    search_dev at fft_size 2048: the cell is the model's, (bin 2, 700), and the peak-to-mean is within 1e-2 relative of the model's search
    of the model's output.  The stage meets its 1e-5 bar relative to sum |w||x|, which the jammer dominates: at J/N 40 dB that is up to
    2e-3 of the nulled output's own scale, and the search's own f32 tables add 1e-5; 1e-2 leaves a factor of five.
    On an MI355X: c32 40 dB GPU 35.972 (model 35.979), int8 30 dB GPU 9.79289 (model 9.79289); antenna 0 alone 2.65 at a wrong cell."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, nuller
    import excise_model as EM
    import test_nuller_host as TH
    r = TH.scene_run(1)
    eng = A.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                              codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == NM.DWELL
    for name in ("J/N 40 dB, c32", "J/N 30 dB, int8"):
        x = r[name]["x"]
        nl = nuller.Nuller(4, 1024, 1e-4)
        y = nl.process(x)
        assert y.shape == (NM.DWELL,)
        eng.search_dev(hipbuf.upload(y), _lib.FMT_C32)
        got = EM.best_cell(*eng.metrics(), EM.SAT["worker"])
        alone = np.ascontiguousarray(NM.as_c128(x)[:, 0].astype(np.complex64))
        eng.search_dev(hipbuf.upload(alone), _lib.FMT_C32)
        jammed = EM.best_cell(*eng.metrics(), EM.SAT["worker"])
        want = r[name]["nulled"]
        print("%s: GPU nulled %s, model %s; GPU antenna 0 alone %s" % (name, got, want, jammed))
        assert NM.found(got) and got[:2] == want[:2] and got[2] > NM.DETECT
        assert abs(got[2] - want[2]) <= 1e-2 * want[2]
        assert jammed[2] < NM.DETECT
        nl.close()
    eng.close()
