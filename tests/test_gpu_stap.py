"""Space-time adaptive nulling on the GPU (gm_stap, csrc/stap_kernels.hip) against the float64 model of stap_model.py, on noise plus a
rank-one white jammer 30 dB above it plus a CW 30 dB above it from another direction, so that the temporal freedoms do work.  Each step
is held to its own bar:

  R   against the float64 sum:                                   |dR[p][q]| <= 1e-5 sum_t |z_p| |z_q|   (derived: 5.8e-6 at B = 16384, L = 8)
  w   against the model's w computed from the DEVICE's R words:  |dw[p]|    <= 2^-22 max_p |w[p]|       (one f32 rounding + the f64 solve)
  y   against the model handed the device's w words:             |dy|       <= 1e-5 sum_p |w[p]| |z_p|  (derived: (M + 2) 2^-24)

1. Shapes (A, L, B): the twelve of SHAPES: every A once or twice, L = 1, 2, 4, 5, 6 and 8, both kernel forms (L <= 4, L > 4) but not
   at every A (<5, 1> and <6, 1> are not among them), B = 256, 1024 and 16384; both formats (the int8 stream holds -128), loading 1e-4
   and 1e-2, e_0 and a random complex s, call lengths 1, L - 1, B - 1, B, B + 1, 3B - 1, 5B + 7.  The first block of every stream has
   a halo of zeros.  The largest fraction of each bar is printed per shape.  Every (A, L) the stage accepts, and so every <A, NL> and
   L = 3 and 7, runs at B = 256 in tests/test_gpu_stage_instantiations.py.
2. Cuts: one call against calls of 1, 7, B - 1, 1000 and 3001 time samples, bit for bit, for y, the captured R and w, and stats; again
   after a reset to 2^32 - 3 and to 2^40 + 12345, where the words also go against the model.  Two runs give the same words.
3. Input pointers that are not aligned.
4. Static mode; a switch to it and back; a capture in static mode writes w only.
5. An all-zero block; a block whose sums overflow f32; a noise-free CW at loading 1e-6 (the fallback count).
6. L = 1 against gm_nuller.
7. Every refusal, with state, outputs and captures untouched.
8. process_dev on a caller's stream that is held back.
9. The chain: S1 and S2 of seed 1 through Stap.process at L = 4, then a plain search_dev at fft_size 2048."""
import ctypes as C

import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import nuller_model as NM
import stap_model as SM

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
BAR_R, BAR_W, BAR_Y = SM.BAR_R, SM.BAR_W, SM.BAR_Y
GAP = 5


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


_stream = SM.stream


def _bps(fmt, A):
    return A * (2 if fmt == "i8" else 8)


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, st, d_x, fmt, n, step=None):
    """the n time samples at d_x through st.process_dev in calls of `step` (None: one call), each call's blocks captured behind the
    earlier calls' -> (y, R [blocks, M, M], w [blocks, M]); words behind the outputs and behind the captured blocks must stay as filled"""
    A, M, B = st.n_antennas, st.n_weights, st.block
    cap = n + B
    nb_cap = cap // B + 1
    d_y = hipbuf.alloc((cap + GAP) * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(nb_cap * M * M * 8, fill=0x5A), hipbuf.alloc(nb_cap * M * 8, fill=0x5A)
    done = got = 0
    step = step or max(n, 1)
    while True:
        k = min(step, n - done)
        nb = got // B
        st.capture(d_R + nb * M * M * 8, d_w + nb * M * 8, nb_cap - nb)
        got += st.process_dev(d_x + done * _bps(fmt, A), _fmt(fmt), k, d_y + got * 8, cap - got)
        done += k
        if done >= n:
            break
    st.synchronize()
    st.capture(None, None, 0)
    nb = got // B
    raw = hipbuf.download(d_y, (cap + GAP) * 8, np.complex64)
    R = hipbuf.download(d_R, nb_cap * M * M * 8, np.complex64).reshape(nb_cap, M, M)
    w = hipbuf.download(d_w, nb_cap * M * 8, np.complex64).reshape(nb_cap, M)
    assert (raw[got:].view(np.uint8) == 0x5A).all() and (w[nb:].view(np.uint8) == 0x5A).all() and (R[nb:].view(np.uint8) == 0x5A).all()
    return raw[:got].copy(), R[:nb].copy(), w[:nb].copy()


def _check(tag, p, x, y, R, w, input_index=0):
    """the three bars -> the largest fraction of each"""
    m = SM.run(p, x, input_index=input_index)
    nb, M = m["zb"].shape[0], p["M"]
    assert y.shape == (nb * p["B"],) and R.shape == (nb, M, M) and w.shape == (nb, M), tag
    if not nb:
        return 0.0, 0.0, 0.0
    for a in (y, R, w):
        assert np.isfinite(a.view(np.float32)).all(), tag
    assert (R == np.conj(np.swapaxes(R, 1, 2))).all(), tag                                   # exactly Hermitian
    assert (_words(R[:, np.arange(M), np.arange(M)].imag) == 0).all(), tag                    # the diagonal's imaginary part is +0
    fr = float((np.abs(R.astype(np.complex128) - m["R"]) / np.maximum(m["R_weight"], 1e-300)).max())
    wm = SM.weights(p, R)                                              # from the device's R words
    fw = float((np.abs(w.astype(np.complex128) - wm) / np.abs(wm).max(axis=1, keepdims=True)).max())
    ym, yw = SM.combine(m["zb"], w)                                    # handed the device's w words
    fy = float((np.abs(y.astype(np.complex128) - ym) / np.maximum(yw, 1e-300)).max())
    print("%s: R %.3g of its bar, w %.3g, y %.3g" % (tag, fr / BAR_R, fw / BAR_W, fy / BAR_Y))
    assert fr <= BAR_R and fw <= BAR_W and fy <= BAR_Y, (tag, fr, fw, fy)
    return fr / BAR_R, fw / BAR_W, fy / BAR_Y


_derived_R = SM.derived_R


SHAPES = [(2, 1, 256), (2, 2, 256), (2, 8, 256), (3, 5, 256), (4, 4, 256), (4, 8, 256), (5, 6, 256), (6, 5, 256), (7, 4, 256), (8, 4, 256),
          (4, 4, 1024), (2, 8, 16384)]


def test_the_derived_bound_sits_below_the_bar():
    for A, L, B in SHAPES + [(4, 8, 16384)]:
        assert _derived_R(B, L) < BAR_R and (A * L + 2) * 2.0 ** -24 < BAR_Y


@pytest.mark.parametrize("shape", SHAPES)
def test_words_against_the_model(gpu, hipbuf, shape):
    from gnss_sdr_rs_amd import stap
    A, L, B = shape
    M = A * L
    lengths = sorted({1, L - 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7} - {0})
    s = (np.random.default_rng(M).standard_normal(M) + 1j * np.random.default_rng(B + L).standard_normal(M)).astype(np.complex64)
    worst = np.zeros(3)
    for fmt in ("i8", "c32"):
        x = _stream(fmt, lengths[-1], A, 100 * A + L + B % 97)
        d_x = hipbuf.upload(x)
        for loading, steering in ((1e-4, None), (1e-2, s), (1e-2, None), (1e-4, s)):
            st = stap.Stap(A, L, B, loading, steering)
            p = SM.resolve(A, L, B, loading, steering)
            assert (st.block, st.loading) == (p["B"], p["loading"])
            for n in (lengths if steering is None and loading == 1e-4 else lengths[-1:]):
                st.reset(0)
                y, R, w = _feed(hipbuf, st, d_x, fmt, n)
                worst = np.maximum(worst, _check((shape, fmt, loading, steering is not None, n), p, x[:n], y, R, w))
                assert st.stats() == dict(inputs=n, outputs=SM.total_out(p, n), blocks=n // B, fallback_blocks=0)
                if steering is None:
                    assert (w[:, 0].real == np.float32(1.0)).all()
            st.reset(0)
            again = _feed(hipbuf, st, d_x, fmt, lengths[-1])           # a second run: the same words
            assert all((_words(a) == _words(b)).all() for a, b in zip(again, (y, R, w)))
            st.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()       # the input is only read
    print("%s: largest fractions of the bars: R %.3g (derived bound %.3g of the bar), w %.3g, y %.3g (derived %.3g)"
          % (shape, worst[0], _derived_R(B, L) / BAR_R, worst[1], worst[2], (M + 2) * 2.0 ** -24 / BAR_Y))


@pytest.mark.parametrize("A,L,B,fmt", [(2, 8, 256, "i8"), (4, 4, 1024, "c32"), (3, 5, 256, "c32"), (8, 4, 256, "i8")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, A, L, B, fmt):
    from gnss_sdr_rs_amd import stap
    st = stap.Stap(A, L, B)
    p = SM.resolve(A, L, B)
    n = 6007
    x = _stream(fmt, n, A, 5)
    d_x = hipbuf.upload(x)
    for index in (0, (1 << 32) - 3, (1 << 40) + 12345):
        st.reset(index)
        whole = _feed(hipbuf, st, d_x, fmt, n)
        assert whole[0].size == SM.plan(p, index, n) > 0
        _check((A, L, B, fmt, index), p, x, *whole, input_index=index)
        state = st.stats()
        assert state == dict(inputs=n, outputs=whole[0].size, blocks=whole[0].size // B, fallback_blocks=0)
        for step in (1, 7, B - 1, 1000, 3001):
            st.reset(index)
            got = _feed(hipbuf, st, d_x, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, whole)), (index, step)
            assert st.stats() == state
    st.close()


def test_the_first_block_has_a_halo_of_zeros(gpu, hipbuf):
    """a handle that has carried another stream, then a reset: the first block's words are a fresh handle's and the model's, whose
    samples before the stream's start are zeros"""
    from gnss_sdr_rs_amd import stap
    A, L, B = 3, 8, 256
    p = SM.resolve(A, L, B)
    x, other = _stream("c32", B + 9, A, 41), _stream("c32", 2 * B + 100, A, 42)
    fresh, used = stap.Stap(A, L, B), stap.Stap(A, L, B)
    want = _feed(hipbuf, fresh, hipbuf.upload(x), "c32", B + 9)
    _check("first block", p, x, *want)
    _feed(hipbuf, used, hipbuf.upload(other), "c32", 2 * B + 100)
    used.reset(0)
    got = _feed(hipbuf, used, hipbuf.upload(x), "c32", B + 9)
    assert all((_words(a) == _words(b)).all() for a, b in zip(got, want))
    z = SM.blocks_of(p, x)
    assert not z[0, 0, A:].any() and z[0, 0, :A].all() and not z[0, L - 2, (L - 1) * A:].any()
    fresh.close()
    used.close()


@pytest.mark.parametrize("A,L,fmt", [(3, 5, "i8"), (8, 4, "i8"), (4, 8, "i8"), (4, 4, "c32"), (3, 2, "c32")])
def test_input_pointers_that_are_not_aligned(gpu, hipbuf, A, L, fmt):
    """the stream one, two and three elements behind an aligned address: the same words as at the aligned address"""
    from gnss_sdr_rs_amd import stap
    B, n = 256, 3 * 256 + 11
    st = stap.Stap(A, L, B)
    p = SM.resolve(A, L, B)
    x = _stream(fmt, n, A, 77)
    want = _feed(hipbuf, st, hipbuf.upload(x), fmt, n)
    _check((A, L, fmt, "aligned"), p, x, *want)
    flat = x.reshape((n * A,) + x.shape[2:])
    for lead in (1, 2, 3):
        padded = np.concatenate([np.zeros((lead,) + flat.shape[1:], flat.dtype), flat])
        d = hipbuf.upload(padded) + lead * (2 if fmt == "i8" else 8)
        for step in (None, 100):
            st.reset(0)
            got = _feed(hipbuf, st, d, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, want)), (lead, step)
    st.close()


def test_static_mode(gpu, hipbuf):
    from gnss_sdr_rs_amd import stap
    rng = np.random.default_rng(12)
    for A, L, B, fmt in ((4, 4, 256, "c32"), (3, 5, 256, "i8"), (8, 4, 1024, "i8")):
        M = A * L
        n = 4 * B + 9
        x = _stream(fmt, n, A, 3)
        d_x = hipbuf.upload(x)
        st, ref = stap.Stap(A, L, B), stap.Stap(A, L, B)
        p = SM.resolve(A, L, B)
        adaptive = _feed(hipbuf, ref, d_x, fmt, n)
        w = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
        st.set_weights(w)
        y, R, wc = _feed(hipbuf, st, d_x, fmt, n, 1000)
        m = SM.run(p, x, static_w=w)
        assert y.shape == m["y"].shape and st.stats() == dict(inputs=n, outputs=4 * B, blocks=4, fallback_blocks=0)
        frac = float((np.abs(y.astype(np.complex128) - m["y"]) / m["y_weight"]).max())
        print("static (%d, %d, %d, %s): y %.3g of its bar" % (A, L, B, fmt, frac / BAR_Y))
        assert frac <= BAR_Y
        assert (_words(wc) == _words(np.tile(w, (4, 1)))).all()         # the capture holds the installed words
        assert (R.view(np.uint8) == 0x5A).all()                         # and R is not written in static mode
        # static for the first two blocks, adaptive again for the rest: the adaptive handle's words, bit for bit
        st.reset(0)
        first = _feed(hipbuf, st, d_x, fmt, 2 * B + 5)
        assert (_words(first[0]) == _words(y[:2 * B])).all()
        st.set_weights(None)
        rest = _feed(hipbuf, st, d_x + (2 * B + 5) * _bps(fmt, A), fmt, n - 2 * B - 5)
        assert all((_words(a) == _words(b[2:] if b.ndim > 1 else b[2 * B:])).all() for a, b in zip(rest, adaptive))
        # the host-buffer form: the same words in both modes
        st.reset(0)
        hy, hR, hw = st.process(x, want_blocks=True)
        assert all((_words(a) == _words(b)).all() for a, b in zip((hy, hR, hw), adaptive))
        st.reset(0)
        assert (_words(st.process(x)) == _words(adaptive[0])).all()
        st.set_weights(w)
        st.reset(0)
        hy, hR, hw = st.process(x, want_blocks=True)
        assert (_words(hy) == _words(y)).all() and (_words(hw) == _words(wc)).all() and not hR.any()
        st.close()
        ref.close()


def test_an_all_zero_block(gpu, hipbuf):
    from gnss_sdr_rs_amd import stap
    A, L, B = 4, 3, 256
    M = A * L
    s = (np.arange(M) % 5 - 1.5 + 1j * (np.arange(M) % 3 - 1)).astype(np.complex64)
    for fmt in ("c32", "i8"):
        x = _stream(fmt, 4 * B, A, 8)
        x[B - (L - 1):2 * B] = 0                                       # block 1 and the halo it reaches back into
        for steering in (None, s):
            st = stap.Stap(A, L, B, steering=steering)
            p = SM.resolve(A, L, B, steering=steering)
            y, R, w = _feed(hipbuf, st, hipbuf.upload(x), fmt, 4 * B)
            _check((fmt, steering is not None), p, x, y, R, w)
            want = p["s"] / np.vdot(p["s"], p["s"]).real
            assert not R[1].any() and not y[B:2 * B].any() and y[:B].any() and y[2 * B:].any()
            assert np.abs(w[1].astype(np.complex128) - want).max() <= BAR_W * np.abs(want).max()
            assert st.stats()["fallback_blocks"] == 1
            st.reset(0)
            assert st.stats()["fallback_blocks"] == 0
            st.close()


@pytest.mark.parametrize("A,L", [(4, 4), (3, 6)])
def test_a_block_whose_sums_overflow_takes_the_fallback(gpu, hipbuf, A, L):
    """finite samples of around 3e19 in the interior of block 1: |x|^2 is above the largest f32, the trace is not finite, so no pivot is: the
    block takes w = e_0, its outputs are antenna 0's samples word for word and finite, and it is counted; the blocks around it, whose
    taps do not reach the large samples, stay within their bars"""
    from gnss_sdr_rs_amd import stap
    B, M = 256, A * L
    x = _stream("c32", 3 * B, A, 23)
    x[B + 10:2 * B - 10] *= np.float32(1e18)
    assert np.isfinite(x.view(np.float32)).all() and np.abs(x[B + 10:2 * B - 10].real).max(axis=0).min() > 2e19     # squares above f32
    st = stap.Stap(A, L, B)
    p = SM.resolve(A, L, B)
    y, R, w = _feed(hipbuf, st, hipbuf.upload(x), "c32", 3 * B)
    assert not np.isfinite(R[1].view(np.float32)).all()
    e0 = np.zeros(M, np.complex64)
    e0[0] = 1.0
    with np.errstate(all="ignore"):
        wm, fb = SM.weights(p, R, want_fallback=True)              # the model's rule on the device's R words
    assert list(fb) == [False, True, False] and (wm[1] == e0).all()
    assert (_words(w[1]) == _words(e0)).all() and np.isfinite(y.view(np.float32)).all()
    assert (y[B:2 * B] == x[B:2 * B, 0]).all()
    assert st.stats() == dict(inputs=3 * B, outputs=3 * B, blocks=3, fallback_blocks=1)
    keep = [0, 2]
    m = SM.run(p, x)
    fr = float((np.abs(R[keep].astype(np.complex128) - m["R"][keep]) / m["R_weight"][keep]).max())
    fw = float((np.abs(w[keep].astype(np.complex128) - wm[keep]) / np.abs(wm[keep]).max(axis=1, keepdims=True)).max())
    ym, yw = SM.combine(m["zb"], w)
    sel = np.r_[0:B, 2 * B:3 * B]
    fy = float((np.abs(y.astype(np.complex128) - ym)[sel] / yw[sel]).max())
    assert fr <= BAR_R and fw <= BAR_W and fy <= BAR_Y, (fr, fw, fy)
    st.close()


def test_a_noise_free_cw_at_the_smallest_loading(gpu, hipbuf):
    """a rank-one Gram matrix under loading 1e-6, which the f32 words' own rounding can exceed: every output is finite, and the
    captured rows equal to the fallback w = e_0 are as many as fallback_blocks says"""
    from gnss_sdr_rs_amd import stap
    for A, L, B in ((4, 4, 256), (2, 8, 1024), (8, 4, 256)):
        n = 8 * B
        t = np.arange(n)
        x = (100.0 * np.exp(2j * np.pi * 0.0931 * t)[:, None] * NM.steer(0.4, A)[None, :]).astype(np.complex64)
        st = stap.Stap(A, L, B, 1e-6)
        y, R, w = _feed(hipbuf, st, hipbuf.upload(x), "c32", n)
        assert y.shape == (n,) and all(np.isfinite(a.view(np.float32)).all() for a in (y, R, w))
        e0 = np.zeros(A * L, np.complex64)
        e0[0] = 1.0
        rows = int((_words(w) == _words(e0)[None, :]).all(axis=1).sum())
        got = st.stats()
        print("CW (%d, %d, %d): %d of %d blocks fell back" % (A, L, B, got["fallback_blocks"], got["blocks"]))
        assert got["blocks"] == 8 and rows == got["fallback_blocks"]
        st.close()


@pytest.mark.parametrize("A,B,fmt", [(2, 256, "i8"), (4, 1024, "c32"), (8, 256, "c32")])
def test_one_tap_against_the_nuller(gpu, hipbuf, A, B, fmt):
    """L = 1 is gm_nuller's definition with another summation order: R within the sum of the two R bars; with the same static weights
    y within the sum of the two y bars; and each handle's adaptive words within its own bars of the model"""
    from gnss_sdr_rs_amd import nuller, stap
    n = 3 * B + 17
    x = _stream(fmt, n, A, 9)
    d_x = hipbuf.upload(x)
    st, nl = stap.Stap(A, 1, B), nuller.Nuller(A, B)
    p = SM.resolve(A, 1, B)
    y, R, w = _feed(hipbuf, st, d_x, fmt, n)
    _check((A, B, fmt, "L = 1"), p, x, y, R, w)
    yn, Rn, wn = nl.process(x, want_blocks=True)
    m = SM.run(p, x)
    mn = NM.run(NM.resolve(A, B), x)
    assert np.abs(m["R"] - mn["R"]).max() == 0.0 and np.abs(m["y"] - mn["y"]).max() == 0.0
    assert (np.abs(R.astype(np.complex128) - Rn.astype(np.complex128)) <= 2 * BAR_R * m["R_weight"]).all()
    ws = (np.random.default_rng(3).standard_normal(A) + 1j * np.random.default_rng(4).standard_normal(A)).astype(np.complex64)
    st.set_weights(ws)
    nl.set_weights(ws)
    st.reset(0)
    nl.reset(0)
    ys, yns = st.process(x), nl.process(x)
    _, wt = SM.combine(m["zb"], ws)
    assert (np.abs(ys.astype(np.complex128) - yns.astype(np.complex128)) <= 2 * BAR_Y * wt).all()
    st.close()
    nl.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, stap
    import test_stap_host as TH
    L_ = gpu.lib()
    for cfg in TH.REFUSED:
        with pytest.raises(_lib.GmError) as e:
            stap.Stap(**cfg)
        assert e.value.status == INVALID, cfg
    h = C.c_void_p()
    ok = _lib.StapCfg(4, 2, 256, 0.0, None, 0)
    assert L_.gm_stap_create(None, C.byref(h)) == INVALID and L_.gm_stap_create(C.byref(ok), None) == INVALID
    assert L_.gm_stap_create(C.byref(_lib.StapCfg(4, 2, 256, 0.0, None, 1)), C.byref(h)) == INVALID and not h.value
    A, L, B = 4, 2, 256
    M = A * L
    st = stap.Stap(A, L, B)
    p = SM.resolve(A, L, B)
    n = 5 * B + 40
    x = _stream("c32", n, A, 31)
    room = np.zeros((2 * n, A), np.complex64)                      # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    d_y = hipbuf.alloc(n * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(8 * M * M * 8, fill=0x5A), hipbuf.alloc(8 * M * 8, fill=0x5A)
    first = B + 100
    st.capture(d_R, d_w, 8)
    n1 = st.process_dev(d_x, _lib.FMT_C32, first, d_y, n)
    state = st.stats()
    assert state == dict(inputs=first, outputs=B, blocks=1, fallback_blocks=0) and n1 == B
    R1, w1 = hipbuf.download(d_R, 8 * M * M * 8, np.complex64), hipbuf.download(d_w, 8 * M * 8, np.complex64)
    rest = n - first
    n2 = SM.plan(p, first, rest)
    assert n2 == 4 * B
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, cap: L_.gm_stap_process_dev(st._h, d_in, fmt, n_in, d_out, cap, C.byref(got), None)
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
    st.capture(d_R, d_w, 3)                                                      # a capture smaller than the call's four blocks
    assert call(src, _lib.FMT_C32, rest, out, n2) == OUT_OF_RANGE
    st.capture(d_R, d_w, 8)
    assert L_.gm_stap_capture(st._h, d_R, None, 8) == INVALID and L_.gm_stap_capture(st._h, None, d_w, 8) == INVALID
    assert L_.gm_stap_capture(st._h, d_R, d_w, 0) == INVALID and L_.gm_stap_capture(st._h, None, None, 8) == INVALID
    bad = np.zeros(M, np.complex64)
    bad[0], bad[M - 1] = 1, np.nan
    assert L_.gm_stap_set_weights(st._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    bad[M - 1] = complex(0, np.inf)
    assert L_.gm_stap_set_weights(st._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    assert got.value == 77 and st.stats() == state
    assert L_.gm_stap_reset(st._h, (1 << 62) + 1) == INVALID and st.stats() == state
    raw = hipbuf.download(d_y, n * 8, np.complex64)
    assert (raw[n1:].view(np.uint8) == 0x5A).all()                  # nothing was written
    assert (_words(hipbuf.download(d_R, 8 * M * M * 8, np.complex64)) == _words(R1)).all()
    assert (_words(hipbuf.download(d_w, 8 * M * 8, np.complex64)) == _words(w1)).all()
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and st.stats() == state      # n_in = 0
    # the next good call continues the stream as if nothing had been refused (the refused set_weights left the adaptive rule);
    # d_out right behind d_in is no overlap
    assert call(src, _lib.FMT_C32, rest, d_x + n * A * 8, n2) == 0 and got.value == n2
    st.synchronize()
    tail = hipbuf.download(d_x + n * A * 8, n2 * 8, np.complex64)
    y = np.concatenate([raw[:n1], tail])
    R = np.concatenate([R1.reshape(8, M, M)[:1], hipbuf.download(d_R, 4 * M * M * 8, np.complex64).reshape(4, M, M)])
    w = np.concatenate([w1.reshape(8, M)[:1], hipbuf.download(d_w, 4 * M * 8, np.complex64).reshape(4, M)])
    _check("after the refusals", p, x, y, R, w)
    assert st.stats() == dict(inputs=n, outputs=5 * B, blocks=5, fallback_blocks=0)
    # the host-buffer form: the same words, the same refusals
    st.reset(0)
    hy, hR, hw = st.process(x, want_blocks=True)
    assert (_words(hy) == _words(y)).all() and (_words(hR) == _words(R)).all() and (_words(hw) == _words(w)).all()
    small = np.zeros(4, np.complex64)
    xp = x.ctypes.data_as(C.c_void_p)
    sp = small.ctypes.data_as(C.c_void_p)
    assert L_.gm_stap_process(st._h, xp, _lib.FMT_C32, 300, sp, 4, None, None, None, 0) == OUT_OF_RANGE
    assert L_.gm_stap_process(st._h, xp, _lib.FMT_I8_REAL, 100, sp, 4, None, None, None, 0) == INVALID
    big = np.zeros(2 * B, np.complex64)
    wbuf = np.zeros((1, M), np.complex64)
    assert L_.gm_stap_process(st._h, xp, _lib.FMT_C32, 2 * B, big.ctypes.data_as(C.c_void_p), 2 * B, None, None,
                              wbuf.ctypes.data_as(C.c_void_p), 1) == OUT_OF_RANGE
    assert st.stats()["inputs"] == n and not small.any() and not big.any() and not wbuf.any()
    st.close()


@pytest.mark.parametrize("A,L,B,fmt", [(4, 4, 256, "c32"), (3, 5, 256, "i8")])
def test_process_dev_on_a_callers_stream_that_is_held_back(gpu, A, L, B, fmt):
    """the producer's H2D, two process_dev calls with a capture and the consumer's D2H all behind a held gate on the caller's stream,
    nothing waited for until the last library call has returned: bit for bit the synchronous run's words"""
    from gnss_sdr_rs_amd import stap
    M = A * L
    n, cut = 3 * B + 50, B + 77
    x = _stream(fmt, n, A, 19)
    ref = stap.Stap(A, L, B)
    want = ref.process(x, want_blocks=True)
    want_stats = ref.stats()
    ref.close()
    with SS.HeldStream() as S:
        st = S.own(stap.Stap(A, L, B))
        d_x, d_y = S.device(x.nbytes), S.device(3 * B * 8)
        d_R, d_w = S.device(3 * M * M * 8), S.device(3 * M * 8)
        staged = S.stage(x)
        S.hold("stap %d %d %d %s" % (A, L, B, fmt))
        S.h2d(d_x, staged)
        st.capture(d_R, d_w, 3)
        n1 = st.process_dev(d_x, _fmt(fmt), cut, d_y, 3 * B, stream=S.stream)
        st.capture(d_R + (n1 // B) * M * M * 8, d_w + (n1 // B) * M * 8, 3 - n1 // B)
        n2 = st.process_dev(d_x + cut * _bps(fmt, A), _fmt(fmt), n - cut, d_y + n1 * 8, 3 * B - n1, stream=S.stream)
        hy, hR, hw = S.d2h(d_y, 3 * B * 8), S.d2h(d_R, 3 * M * M * 8), S.d2h(d_w, 3 * M * 8)
        S.assert_held()
        S.sync()
        assert n1 + n2 == 3 * B
        got = (hy.view(np.complex64), hR.view(np.complex64).reshape(3, M, M), hw.view(np.complex64).reshape(3, M))
        assert all((_words(a) == _words(b)).all() for a, b in zip(got, want))
        assert st.stats() == want_stats


def test_the_jammed_scenes_through_the_stage_and_a_plain_search(gpu, hipbuf):
    """Seed 1's S1 (A = 2) and S2 (A = 4), as many 40 dB interferers as antennas with one of them a CW, through Stap.process (L = 4,
    B = 1024, loading 1e-4, e_0) and a plain search_dev at fft_size 2048: the cell is (bin 2, 700) above 7, where antenna 0 alone and
    Nuller.process stay below 7.  The peak-to-mean is printed next to the model's, and held to it within 1e-2 relative (the reasoning of
    test_gpu_nuller.py's chain: the stage's 1e-5 of sum |w||z|, which the interferers dominate, is up to 2e-3 of the output's scale)."""
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, nuller, stap
    import excise_model as EM
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == SM.DWELL

    def cell(y):
        eng.search_dev(hipbuf.upload(np.ascontiguousarray(y.astype(np.complex64))), _lib.FMT_C32)
        return EM.best_cell(*eng.metrics(), EM.SAT["worker"])

    for name in ("S1", "S2"):
        x = SM.scene(name, 1).astype(np.complex64)
        A = x.shape[1]
        st, nl = stap.Stap(A, 4, 1024, 1e-4), nuller.Nuller(A, 1024, 1e-4)
        y = st.process(x)
        assert y.shape == (SM.DWELL,)
        got, spatial, alone = cell(y), cell(nl.process(x)), cell(x[:, 0])
        want = SM.search(SM.nulled(x, 4))
        print("%s: GPU L = 4 %s, model %s; GPU Nuller %s; GPU antenna 0 alone %s" % (name, got, want, spatial, alone))
        assert SM.found(got) and got[:2] == want[:2] == (2, 700) and got[2] > SM.DETECT
        assert abs(got[2] - want[2]) <= 1e-2 * want[2]
        assert spatial[2] < SM.DETECT and alone[2] < SM.DETECT
        assert st.stats()["fallback_blocks"] == 0
        st.close()
        nl.close()
    eng.close()
