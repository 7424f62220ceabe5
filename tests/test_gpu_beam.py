"""One beam per satellite on the GPU (gm_beamformer, csrc/beam_kernels.hip).  The contract is that beam p's R, w and y words and its
fallback count are those of a gm_stap created with steering = s_p on the same stream, so the first bar is bit-for-bit equality with
Stap handles; two shapes also go against the float64 model (beam_model.py = stap_model.py per row) at gm_stap's three bars,

  R   against the float64 sum:                                   |dR[p][q]| <= 1e-5 sum_t |z_p| |z_q|
  w   against the model's w computed from the DEVICE's R words:  |dw[p]|    <= 2^-22 max_p |w[p]|
  y   against the model handed the device's w words:             |dy|       <= 1e-5 sum_p |w[p]| |z_p|

so that the file does not rest on gm_stap alone.  The input is test_gpu_stap.py's: noise plus a rank-one white jammer and a CW 30 dB up;
the int8 stream holds -128.

1. Shapes (A, L, B, P): the twelve of SHAPES (every A, but not every <A, NL>: <3, 1>, <5, 1> and <6, 1> are not among them): one
   chunk, two chunks and two groups of 1024; P below, at and one past a group of four and two substitution rounds; M = 32 with
   P = 16.  Both formats, loading 1e-4 and 1e-2, random complex rows and an e_0 row.  Every (A, L) the stage accepts runs at B = 256
   and P = 5, each beam against the model, in tests/test_gpu_stage_instantiations.py.
2. Cuts: calls of 1, 7, B - 1, 1000, 3001 against one call, bit for bit; again after a reset to 2^32 - 3; two runs give the same words.
3. out_stride equal to the count, and larger with sentinel words between and behind the planes.
4. A beam's words depend neither on P nor on the other rows.
5. set_steering between two calls.  6. Static mode and back; a static capture writes w only.
7. An all-zero block and an overflowing block.  8. Unaligned input pointers.  9. Every refusal.
10. process_dev on a caller's stream that is held back.  11. The chain: T1 through the beams, each plane into a plain search_dev."""
import ctypes as C

import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import beam_model as BM
import stap_model as SM
import test_gpu_stap as TS

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
GAP = 5
_words, _stream, _bps, _fmt = TS._words, TS._stream, TS._bps, TS._fmt


def _rows(P, M, seed, e0_last=True):
    """[P, M] complex64: random complex rows, the last one e_0 (where P > 1)"""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M))).astype(np.complex64)
    if e0_last and P > 1:
        s[P - 1] = 0
        s[P - 1, 0] = 1.0
    return s


def _feed(hipbuf, bf, d_x, fmt, n, step=None, stride=None):
    """the n time samples at d_x through bf.process_dev in calls of `step` (None: one call) into planes `stride` words apart (None:
    n + B, room for any count), each call's blocks captured behind the earlier calls' -> (y [P, got], R [blocks, M, M],
    w [blocks, P, M]); words behind a plane's outputs, between the planes and behind the captured blocks must stay as filled"""
    A, M, B, P = bf.n_antennas, bf.n_weights, bf.block, bf.n_beams
    stride = n + B if stride is None else stride
    nb_cap = (n + B) // B + 1
    d_y = hipbuf.alloc((P * stride + GAP) * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(nb_cap * M * M * 8, fill=0x5A), hipbuf.alloc(nb_cap * P * M * 8, fill=0x5A)
    done = got = 0
    step = step or max(n, 1)
    while True:
        k = min(step, n - done)
        nb = got // B
        bf.capture(d_R + nb * M * M * 8, d_w + nb * P * M * 8, nb_cap - nb)
        got += bf.process_dev(d_x + done * _bps(fmt, A), _fmt(fmt), k, d_y + got * 8, stride)
        done += k
        if done >= n:
            break
    bf.synchronize()
    bf.capture(None, None, 0)
    nb = got // B
    raw = hipbuf.download(d_y, (P * stride + GAP) * 8, np.complex64)
    R = hipbuf.download(d_R, nb_cap * M * M * 8, np.complex64).reshape(nb_cap, M, M)
    w = hipbuf.download(d_w, nb_cap * P * M * 8, np.complex64).reshape(nb_cap, P, M)
    planes = raw[:P * stride].reshape(P, stride)
    assert (planes[:, got:].view(np.uint8) == 0x5A).all() and (raw[P * stride:].view(np.uint8) == 0x5A).all()
    assert (w[nb:].view(np.uint8) == 0x5A).all() and (R[nb:].view(np.uint8) == 0x5A).all()
    return planes[:, :got].copy(), R[:nb].copy(), w[:nb].copy()


def _staps(A, L, B, loading, rows, x, input_index=0):
    """the yardstick: a Stap handle per row on the same stream -> [(y, R [blocks, M, M], w [blocks, M], fallback_blocks)]"""
    from gnss_sdr_rs_amd import stap
    out = []
    for s in rows:
        st = stap.Stap(A, L, B, loading, s)
        st.reset(input_index)
        out.append(st.process(x, want_blocks=True) + (st.stats()["fallback_blocks"],))
        st.close()
    return out


def _same(got, fallbacks, want, tag=""):
    """the beams' words (y [P, n], R, w [blocks, P, M]) and counters against the Stap handles', bit for bit"""
    y, R, w = got
    assert y.shape[0] == w.shape[1] == len(want) == len(fallbacks), tag
    for p, (ys, Rs, ws, fb) in enumerate(want):
        assert y[p].shape == ys.shape and R.shape == Rs.shape and w[:, p].shape == ws.shape, (tag, p)
        assert (_words(y[p]) == _words(ys)).all(), (tag, p, "y")
        assert (_words(w[:, p]) == _words(ws)).all(), (tag, p, "w")
        assert (_words(R) == _words(Rs)).all(), (tag, p, "R")
        assert fallbacks[p] == fb, (tag, p, "fallbacks")


SHAPES = [(2, 1, 256, 1), (2, 8, 256, 16), (3, 5, 256, 5), (4, 4, 256, 4), (4, 8, 256, 16), (8, 4, 256, 16), (8, 1, 256, 3), (5, 6, 256, 7),
          (7, 4, 256, 9), (6, 5, 512, 2), (4, 4, 2048, 5), (2, 8, 16384, 2)]
MODEL_SHAPES = [(4, 4, 256, 4), (2, 8, 16384, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_every_beam_is_a_stap_with_its_row(gpu, hipbuf, shape):
    from gnss_sdr_rs_amd import beamformer
    A, L, B, P = shape
    M = A * L
    n = (3 if B <= 2048 else 2) * B + 7
    worst = np.zeros(3)
    for fmt in ("i8", "c32"):
        x = _stream(fmt, n, A, 100 * A + L + B % 97 + P)
        d_x = hipbuf.upload(x)
        for loading in (1e-4, 1e-2):
            rows = _rows(P, M, 7 * M + P, e0_last=True)
            if P == 1 and loading == 1e-2:
                rows = np.eye(1, M, dtype=np.complex64)             # the only row is e_0
            bf = beamformer.Beamformer(A, L, rows, B, loading)
            p = BM.resolve(A, L, rows, B, loading)
            assert (bf.block, bf.loading, bf.n_beams) == (p["B"], p["loading"], P)
            got = _feed(hipbuf, bf, d_x, fmt, n)
            stats = bf.stats()
            assert stats == dict(inputs=n, outputs=BM.total_out(p, n), blocks=n // B, fallbacks=[0] * P)
            _same(got, stats["fallbacks"], _staps(A, L, B, loading, rows, x), (shape, fmt, loading))
            if P > 1 or loading == 1e-2:
                assert (got[2][:, P - 1, 0].real == np.float32(1.0)).all()                       # the e_0 row: Re w[0] = 1
            if shape in MODEL_SHAPES:
                for k in range(P):
                    worst = np.maximum(worst, TS._check((shape, fmt, loading, k), p["beams"][k], x, got[0][k], got[1], got[2][:, k]))
            bf.reset(0)
            again = _feed(hipbuf, bf, d_x, fmt, n)                                               # a second run: the same words
            assert all((_words(a) == _words(b)).all() for a, b in zip(again, got))
            bf.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()             # the input is only read
    if shape in MODEL_SHAPES:
        print("%s: largest fractions of the bars: R %.3g (derived bound %.3g of the bar), w %.3g, y %.3g (derived %.3g)"
              % (shape, worst[0], TS._derived_R(B, L) / TS.BAR_R, worst[1], worst[2], (M + 2) * 2.0 ** -24 / TS.BAR_Y))


@pytest.mark.parametrize("A,L,B,P,fmt", [(4, 4, 256, 5, "i8"), (3, 5, 256, 7, "c32")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, A, L, B, P, fmt):
    from gnss_sdr_rs_amd import beamformer
    rows = _rows(P, A * L, 3)
    bf = beamformer.Beamformer(A, L, rows, B)
    p = BM.resolve(A, L, rows, B)
    n = 3500
    x = _stream(fmt, n, A, 5)
    d_x = hipbuf.upload(x)
    for index in (0, (1 << 32) - 3):
        bf.reset(index)
        whole = _feed(hipbuf, bf, d_x, fmt, n)
        assert whole[0].shape == (P, BM.plan(p, index, n)) and whole[0].shape[1] > 0
        state = bf.stats()
        assert state == dict(inputs=n, outputs=whole[0].shape[1], blocks=whole[0].shape[1] // B, fallbacks=[0] * P)
        _same(whole, state["fallbacks"], _staps(A, L, B, 0.0, rows, x, index), (A, L, B, P, fmt, index))
        for step in (1, 7, B - 1, 1000, 3001):
            bf.reset(index)
            got = _feed(hipbuf, bf, d_x, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, whole)), (index, step)
            assert bf.stats() == state
        bf.reset(index)
        again = _feed(hipbuf, bf, d_x, fmt, n)
        assert all((_words(a) == _words(b)).all() for a, b in zip(again, whole)), index
    bf.close()


def test_out_stride_and_the_words_around_the_planes(gpu, hipbuf):
    """a stride equal to the count, and larger ones (in one call and in several): the same words, and _feed has checked that the words
    between and behind the planes stay as filled"""
    from gnss_sdr_rs_amd import beamformer
    A, L, B, P = 3, 3, 256, 6
    rows = _rows(P, A * L, 11)
    bf = beamformer.Beamformer(A, L, rows, B)
    n = 4 * B + 33
    x = _stream("c32", n, A, 2)
    d_x = hipbuf.upload(x)
    want = _feed(hipbuf, bf, d_x, "c32", n)
    assert want[0].shape == (P, 4 * B)
    for stride, step in ((4 * B, None), (4 * B, 300), (4 * B + 1, None), (4 * B + 777, 300), (9 * B, B + 1)):
        bf.reset(0)
        got = _feed(hipbuf, bf, d_x, "c32", n, step, stride)
        assert all((_words(a) == _words(b)).all() for a, b in zip(got, want)), (stride, step)
    bf.close()


def test_a_beam_depends_neither_on_p_nor_on_the_other_rows(gpu, hipbuf):
    from gnss_sdr_rs_amd import beamformer
    A, L, B = 4, 3, 256
    M = A * L
    rows = _rows(5, M, 21)
    rows[4] = rows[1]                                              # two equal rows
    n = 3 * B + 5
    for fmt in ("c32", "i8"):
        x = _stream(fmt, n, A, 6)
        d_x = hipbuf.upload(x)
        five, one = beamformer.Beamformer(A, L, rows, B), beamformer.Beamformer(A, L, rows[2:3], B)
        y5, R5, w5 = _feed(hipbuf, five, d_x, fmt, n)
        y1, R1, w1 = _feed(hipbuf, one, d_x, fmt, n)
        assert (_words(y5[2]) == _words(y1[0])).all() and (_words(w5[:, 2]) == _words(w1[:, 0])).all() and (_words(R5) == _words(R1)).all()
        assert (_words(y5[4]) == _words(y5[1])).all() and (_words(w5[:, 4]) == _words(w5[:, 1])).all()
        assert not (_words(y5[0]) == _words(y5[1])).all()
        five.close()
        one.close()


def test_set_steering_between_two_calls(gpu, hipbuf):
    """blocks of the first call keep the old row's words; blocks finished by the second take the new row's, as a Stap with the new row
    gives them on the whole stream; the other beams do not move"""
    from gnss_sdr_rs_amd import beamformer
    A, L, B, P = 4, 2, 256, 3
    M = A * L
    rows = _rows(P, M, 31)
    new = _rows(1, M, 32)[0]
    n, first = 4 * B + 9, B + 100                                  # block 1 is begun by the first call and finished by the second
    x = _stream("c32", n, A, 13)
    d_x = hipbuf.upload(x)
    bf = beamformer.Beamformer(A, L, rows, B)
    y1, R1, w1 = _feed(hipbuf, bf, d_x, "c32", first)
    bf.set_steering(1, new)
    y2, R2, w2 = _feed(hipbuf, bf, d_x + first * _bps("c32", A), "c32", n - first)
    assert y1.shape == (P, B) and y2.shape == (P, 3 * B)
    old = _staps(A, L, B, 0.0, rows, x)
    moved = _staps(A, L, B, 0.0, [new], x)[0]
    for p in range(P):
        ys, Rs, ws, _ = old[p]
        assert (_words(y1[p]) == _words(ys[:B])).all() and (_words(w1[:, p]) == _words(ws[:1])).all() and (_words(R1) == _words(Rs[:1])).all()
        if p == 1:
            ys, Rs, ws, _ = moved
        assert (_words(y2[p]) == _words(ys[B:])).all() and (_words(w2[:, p]) == _words(ws[1:])).all() and (_words(R2) == _words(Rs[1:])).all()
    assert not (_words(moved[0][B:]) == _words(old[1][0][B:])).all()
    assert bf.stats() == dict(inputs=n, outputs=4 * B, blocks=4, fallbacks=[0] * P)
    bf.close()


def test_static_mode_and_back(gpu, hipbuf):
    from gnss_sdr_rs_amd import beamformer, stap
    rng = np.random.default_rng(12)
    for A, L, B, P, fmt in ((4, 4, 256, 6, "c32"), (3, 5, 256, 3, "i8"), (8, 4, 1024, 16, "i8")):
        M = A * L
        n = 4 * B + 9
        x = _stream(fmt, n, A, 3)
        d_x = hipbuf.upload(x)
        rows = _rows(P, M, 5)
        bf = beamformer.Beamformer(A, L, rows, B)
        adaptive = _feed(hipbuf, bf, d_x, fmt, n)
        w = (rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M))).astype(np.complex64)
        bf.set_weights(w)
        bf.reset(0)
        y, R, wc = _feed(hipbuf, bf, d_x, fmt, n, 1000)
        assert bf.stats() == dict(inputs=n, outputs=4 * B, blocks=4, fallbacks=[0] * P)
        for p in range(P):                                              # a Stap in static mode with beam p's weights
            st = stap.Stap(A, L, B)
            st.set_weights(w[p])
            assert (_words(y[p]) == _words(st.process(x))).all(), p
            st.close()
        m = SM.run(SM.resolve(A, L, B), x, static_w=w[P - 1])          # and the model, so that this does not rest on gm_stap alone
        frac = float((np.abs(y[P - 1].astype(np.complex128) - m["y"]) / m["y_weight"]).max())
        assert frac <= TS.BAR_Y
        assert (_words(wc) == _words(np.tile(w[None], (4, 1, 1)))).all()    # the capture holds the installed words
        assert (R.view(np.uint8) == 0x5A).all()                             # and R is not written in static mode
        # static for the first two blocks, adaptive again for the rest: the adaptive handle's words, bit for bit
        bf.reset(0)
        first = _feed(hipbuf, bf, d_x, fmt, 2 * B + 5)
        assert (_words(first[0]) == _words(y[:, :2 * B])).all()
        bf.set_weights(None)
        rest = _feed(hipbuf, bf, d_x + (2 * B + 5) * _bps(fmt, A), fmt, n - 2 * B - 5)
        assert (_words(rest[0]) == _words(adaptive[0][:, 2 * B:])).all()
        assert (_words(rest[1]) == _words(adaptive[1][2:])).all() and (_words(rest[2]) == _words(adaptive[2][2:])).all()
        # the host-buffer form: the same words in both modes
        bf.reset(0)
        host = bf.process(x, want_blocks=True)
        assert all((_words(a) == _words(b)).all() for a, b in zip(host, adaptive))
        bf.reset(0)
        assert (_words(bf.process(x)) == _words(adaptive[0])).all()
        bf.set_weights(w)
        bf.reset(0)
        hy, hR, hw = bf.process(x, want_blocks=True)
        assert (_words(hy) == _words(y)).all() and (_words(hw) == _words(wc)).all() and not hR.any()
        bf.close()


def test_an_all_zero_block(gpu, hipbuf):
    from gnss_sdr_rs_amd import beamformer
    A, L, B, P = 4, 3, 256, 10
    M = A * L
    rows = _rows(P, M, 17)
    for fmt in ("c32", "i8"):
        x = _stream(fmt, 4 * B, A, 8)
        x[B - (L - 1):2 * B] = 0                                       # block 1 and the halo it reaches back into
        bf = beamformer.Beamformer(A, L, rows, B)
        p = BM.resolve(A, L, rows, B)
        y, R, w = _feed(hipbuf, bf, hipbuf.upload(x), fmt, 4 * B)
        stats = bf.stats()
        assert stats["fallbacks"] == [1] * P                           # every beam falls back, each counter moves by one
        _same((y, R, w), stats["fallbacks"], _staps(A, L, B, 0.0, rows, x), fmt)
        assert not R[1].any() and not y[:, B:2 * B].any() and y[:, :B].any(axis=1).all() and y[:, 2 * B:].any(axis=1).all()
        for k in range(P):
            want = p["s"][k] / np.vdot(p["s"][k], p["s"][k]).real
            assert np.abs(w[1, k].astype(np.complex128) - want).max() <= TS.BAR_W * np.abs(want).max()
        bf.reset(0)
        assert bf.stats()["fallbacks"] == [0] * P
        bf.close()


def test_a_block_whose_sums_overflow_takes_the_fallback(gpu, hipbuf):
    """finite samples of around 3e19 in the interior of block 1: the trace is not finite, so no pivot is: every beam of the block takes
    s_p / (s_p^H s_p) and is counted once; the blocks around it are a Stap's"""
    from gnss_sdr_rs_amd import beamformer
    A, L, B, P = 4, 4, 256, 9
    M = A * L
    rows = _rows(P, M, 19)
    x = _stream("c32", 3 * B, A, 23)
    x[B + 10:2 * B - 10] *= np.float32(1e18)
    assert np.isfinite(x.view(np.float32)).all()
    bf = beamformer.Beamformer(A, L, rows, B)
    p = BM.resolve(A, L, rows, B)
    y, R, w = _feed(hipbuf, bf, hipbuf.upload(x), "c32", 3 * B)
    assert not np.isfinite(R[1].view(np.float32)).all()
    stats = bf.stats()
    assert stats == dict(inputs=3 * B, outputs=3 * B, blocks=3, fallbacks=[1] * P)
    _same((y, R, w), stats["fallbacks"], _staps(A, L, B, 0.0, rows, x))
    for k in range(P):
        want = (p["s"][k] / np.vdot(p["s"][k], p["s"][k]).real)
        assert np.abs(w[1, k].astype(np.complex128) - want).max() <= TS.BAR_W * np.abs(want).max()
    assert (_words(w[1, P - 1]) == _words(rows[P - 1])).all() and (y[P - 1, B:2 * B] == x[B:2 * B, 0]).all()     # the e_0 row: antenna 0
    bf.close()


@pytest.mark.parametrize("A,L,P,fmt", [(3, 5, 5, "i8"), (8, 4, 16, "i8"), (4, 4, 3, "c32")])
def test_input_pointers_that_are_not_aligned(gpu, hipbuf, A, L, P, fmt):
    """the stream one, two and three elements behind an aligned address: the same words as at the aligned address"""
    from gnss_sdr_rs_amd import beamformer
    B, n = 256, 3 * 256 + 11
    bf = beamformer.Beamformer(A, L, _rows(P, A * L, 4), B)
    x = _stream(fmt, n, A, 77)
    want = _feed(hipbuf, bf, hipbuf.upload(x), fmt, n)
    flat = x.reshape((n * A,) + x.shape[2:])
    for lead in (1, 2, 3):
        padded = np.concatenate([np.zeros((lead,) + flat.shape[1:], flat.dtype), flat])
        d = hipbuf.upload(padded) + lead * (2 if fmt == "i8" else 8)
        for step in (None, 100):
            bf.reset(0)
            got = _feed(hipbuf, bf, d, fmt, n, step)
            assert all((_words(a) == _words(b)).all() for a, b in zip(got, want)), (lead, step)
    bf.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, beamformer
    import test_beam_host as TH
    L_ = gpu.lib()
    h = C.c_void_p()
    for cfg in TH.REFUSED:
        c = dict(cfg)
        s = np.ascontiguousarray(np.asarray(c.pop("steering")).astype(np.complex64))
        A, L = c["n_antennas"], c["taps"]
        P = max(1, s.size // (A * L)) if 0 < A * L <= 64 else 1
        raw = _lib.BeamformerCfg(A, L, c.get("block", 0), c.get("loading", 0.0), P, 0, s.ctypes.data, 0)
        assert L_.gm_beamformer_create(C.byref(raw), C.byref(h)) == INVALID and not h.value, cfg
    A, L, B, P = 4, 2, 256, 3
    M = A * L
    rows = _rows(P, M, 41)
    sp = rows.ctypes.data
    ok = _lib.BeamformerCfg(A, L, B, 0.0, P, 0, sp, 0)
    assert L_.gm_beamformer_create(None, C.byref(h)) == INVALID and L_.gm_beamformer_create(C.byref(ok), None) == INVALID
    for bad in (_lib.BeamformerCfg(A, L, B, 0.0, P, 1, sp, 0), _lib.BeamformerCfg(A, L, B, 0.0, P, 0, sp, 1),
                _lib.BeamformerCfg(A, L, B, 0.0, 0, 0, sp, 0), _lib.BeamformerCfg(A, L, B, 0.0, 17, 0, sp, 0),
                _lib.BeamformerCfg(A, L, B, 0.0, P, 0, None, 0)):
        assert L_.gm_beamformer_create(C.byref(bad), C.byref(h)) == INVALID and not h.value
    bf = beamformer.Beamformer(A, L, rows, B)
    p = BM.resolve(A, L, rows, B)
    n = 5 * B + 40
    x = _stream("c32", n, A, 31)
    stride = 5 * B
    lead = P * stride                                              # words: every address the overlap cases name lies in the buffer
    room = np.zeros(lead + n * A + P * stride, np.complex64)       # the stream with room for its planes in front of it and right behind it
    room[lead:lead + n * A] = x.reshape(-1)
    d_x = hipbuf.upload(room) + lead * 8
    d_y = hipbuf.alloc(P * stride * 8, fill=0x5A)
    d_R, d_w = hipbuf.alloc(8 * M * M * 8, fill=0x5A), hipbuf.alloc(8 * P * M * 8, fill=0x5A)
    first = B + 100
    bf.capture(d_R, d_w, 8)
    n1 = bf.process_dev(d_x, _lib.FMT_C32, first, d_y, stride)
    state = bf.stats()
    assert state == dict(inputs=first, outputs=B, blocks=1, fallbacks=[0] * P) and n1 == B
    R1, w1 = hipbuf.download(d_R, 8 * M * M * 8, np.complex64), hipbuf.download(d_w, 8 * P * M * 8, np.complex64)
    raw1 = hipbuf.download(d_y, P * stride * 8, np.complex64)
    rest = n - first
    n2 = BM.plan(p, first, rest)
    assert n2 == 4 * B
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, st: L_.gm_beamformer_process_dev(bf._h, d_in, fmt, n_in, d_out, st, C.byref(got), None)
    src = d_x + first * A * 8
    out = d_y + n1 * 8
    assert call(src, _lib.FMT_I8_REAL, rest, out, stride) == INVALID
    assert call(src, 7, rest, out, stride) == INVALID
    assert call(None, _lib.FMT_C32, rest, out, stride) == INVALID
    assert call(src, _lib.FMT_C32, rest, None, stride) == INVALID
    assert call(src, _lib.FMT_C32, rest, out, n2 - 1) == OUT_OF_RANGE             # out_stride one below the count
    assert call(src, _lib.FMT_C32, rest, out, 0) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, (1 << 31) + 1, out, stride) == INVALID
    # planes overlapping d_in at either end: the first word of plane 0, the last word of plane P - 1
    for d_out in (src, src + 8, src - 8 * ((P - 1) * stride + n2 - 1), src + rest * A * 8 - 8):
        assert call(src, _lib.FMT_C32, rest, d_out, stride) == INVALID, d_out - src
    bf.capture(d_R, d_w, 3)                                                        # a capture smaller than the call's four blocks
    assert call(src, _lib.FMT_C32, rest, out, stride) == OUT_OF_RANGE
    bf.capture(d_R, d_w, 8)
    assert L_.gm_beamformer_capture(bf._h, d_R, None, 8) == INVALID and L_.gm_beamformer_capture(bf._h, None, d_w, 8) == INVALID
    assert L_.gm_beamformer_capture(bf._h, d_R, d_w, 0) == INVALID and L_.gm_beamformer_capture(bf._h, None, None, 8) == INVALID
    bad = np.zeros((P, M), np.complex64)
    bad[:, 0], bad[P - 1, M - 1] = 1, np.nan
    assert L_.gm_beamformer_set_weights(bf._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    bad[P - 1, M - 1] = complex(0, np.inf)
    assert L_.gm_beamformer_set_weights(bf._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    row = np.zeros(M, np.complex64)
    rp = row.ctypes.data_as(C.c_void_p)
    assert L_.gm_beamformer_set_steering(bf._h, 0, rp) == INVALID                  # all zero
    row[0], row[1] = 1, np.nan
    assert L_.gm_beamformer_set_steering(bf._h, 0, rp) == INVALID                  # not finite
    row[1] = 0
    assert L_.gm_beamformer_set_steering(bf._h, P, rp) == INVALID and L_.gm_beamformer_set_steering(bf._h, 1 << 31, rp) == INVALID
    assert L_.gm_beamformer_set_steering(bf._h, 0, None) == INVALID
    assert got.value == 77 and bf.stats() == state
    assert L_.gm_beamformer_reset(bf._h, (1 << 62) + 1) == INVALID and bf.stats() == state
    assert (_words(hipbuf.download(d_y, P * stride * 8, np.complex64)) == _words(raw1)).all()      # nothing was written
    assert (raw1.reshape(P, stride)[:, n1:].view(np.uint8) == 0x5A).all()
    assert (_words(hipbuf.download(d_R, 8 * M * M * 8, np.complex64)) == _words(R1)).all()
    assert (_words(hipbuf.download(d_w, 8 * P * M * 8, np.complex64)) == _words(w1)).all()
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and bf.stats() == state    # n_in = 0
    # the next good call continues the stream as if nothing had been refused (the refused rows and weights changed nothing); planes
    # right behind d_in are no overlap
    behind = d_x + n * A * 8
    assert call(src, _lib.FMT_C32, rest, behind, stride) == 0 and got.value == n2
    bf.synchronize()
    tail = hipbuf.download(behind, P * stride * 8, np.complex64).reshape(P, stride)
    y = np.concatenate([raw1.reshape(P, stride)[:, :n1], tail[:, :n2]], axis=1)
    R = np.concatenate([R1.reshape(8, M, M)[:1], hipbuf.download(d_R, 4 * M * M * 8, np.complex64).reshape(4, M, M)])
    w = np.concatenate([w1.reshape(8, P, M)[:1], hipbuf.download(d_w, 4 * P * M * 8, np.complex64).reshape(4, P, M)])
    stats = bf.stats()
    assert stats == dict(inputs=n, outputs=5 * B, blocks=5, fallbacks=[0] * P)
    _same((y, R, w), stats["fallbacks"], _staps(A, L, B, 0.0, rows, x), "after the refusals")
    # the host-buffer form: the same words, the same refusals
    bf.reset(0)
    host = bf.process(x, want_blocks=True)
    assert all((_words(a) == _words(b)).all() for a, b in zip(host, (y, R, w)))
    small = np.zeros(P * 4, np.complex64)
    xp = x.ctypes.data_as(C.c_void_p)
    sp4 = small.ctypes.data_as(C.c_void_p)
    assert L_.gm_beamformer_process(bf._h, xp, _lib.FMT_C32, 300, sp4, 4, None, None, None, 0) == OUT_OF_RANGE
    assert L_.gm_beamformer_process(bf._h, xp, _lib.FMT_I8_REAL, 100, sp4, 4, None, None, None, 0) == INVALID
    big = np.zeros(P * 2 * B, np.complex64)
    wbuf = np.zeros((1, P, M), np.complex64)
    assert L_.gm_beamformer_process(bf._h, xp, _lib.FMT_C32, 2 * B, big.ctypes.data_as(C.c_void_p), 2 * B, None, None,
                                    wbuf.ctypes.data_as(C.c_void_p), 1) == OUT_OF_RANGE
    assert bf.stats()["inputs"] == n and not small.any() and not big.any() and not wbuf.any()
    bf.close()


@pytest.mark.parametrize("A,L,B,P,fmt", [(4, 4, 256, 5, "c32"), (3, 5, 256, 9, "i8")])
def test_process_dev_on_a_callers_stream_that_is_held_back(gpu, A, L, B, P, fmt):
    """the producer's H2D, two process_dev calls with a capture and the consumer's D2H all behind a held gate on the caller's stream,
    nothing waited for until the last library call has returned: bit for bit the synchronous run's words"""
    from gnss_sdr_rs_amd import beamformer
    M = A * L
    n, cut = 3 * B + 50, B + 77
    x = _stream(fmt, n, A, 19)
    rows = _rows(P, M, 8)
    ref = beamformer.Beamformer(A, L, rows, B)
    want = ref.process(x, want_blocks=True)
    want_stats = ref.stats()
    ref.close()
    with SS.HeldStream() as S:
        bf = S.own(beamformer.Beamformer(A, L, rows, B))
        d_x, d_y = S.device(x.nbytes), S.device(P * 3 * B * 8)
        d_R, d_w = S.device(3 * M * M * 8), S.device(3 * P * M * 8)
        staged = S.stage(x)
        S.hold("beam %d %d %d %d %s" % (A, L, B, P, fmt))
        S.h2d(d_x, staged)
        bf.capture(d_R, d_w, 3)
        n1 = bf.process_dev(d_x, _fmt(fmt), cut, d_y, 3 * B, stream=S.stream)
        bf.capture(d_R + (n1 // B) * M * M * 8, d_w + (n1 // B) * P * M * 8, 3 - n1 // B)
        n2 = bf.process_dev(d_x + cut * _bps(fmt, A), _fmt(fmt), n - cut, d_y + n1 * 8, 3 * B, stream=S.stream)
        hy, hR, hw = S.d2h(d_y, P * 3 * B * 8), S.d2h(d_R, 3 * M * M * 8), S.d2h(d_w, 3 * P * M * 8)
        S.assert_held()
        S.sync()
        assert n1 + n2 == 3 * B
        got = (hy.view(np.complex64).reshape(P, 3 * B), hR.view(np.complex64).reshape(3, M, M), hw.view(np.complex64).reshape(3, P, M))
        assert all((_words(a) == _words(b)).all() for a, b in zip(got, want))
        assert bf.stats() == want_stats


def test_the_scene_through_the_beams_and_a_plain_search(gpu, hipbuf):
    """T1 of seed 1 (A = 4, a white jammer and a CW 40 dB up, two satellites) through Beamformer(4, 2, [e_0, b0, b1]) at B = 1024, each
    plane straight from device memory into a plain search_dev at fft_size 2048: each satellite's true cell is found behind e_0 and behind
    its own beam, with the peak-to-mean within 1 % of the model's on the same input.  The 1 % is a guard against a wrong plane, not a
    parity bar (test_gpu_stap.py's chain gives the reasoning); the parity bars are the cases above."""
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, beamformer
    import excise_model as EM
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == BM.DWELL
    x = BM.scene("T1", 1).astype(np.complex64)
    A, L = x.shape[1], BM.TAPS["T1"]
    rows = BM.rows(A, L)
    bf = beamformer.Beamformer(A, L, rows, 1024, 1e-4)
    d_y = hipbuf.alloc(3 * BM.DWELL * 8)
    assert bf.process_dev(hipbuf.upload(x), _lib.FMT_C32, x.shape[0], d_y, BM.DWELL) == BM.DWELL
    bf.synchronize()
    model = BM.beams(x, L, rows)
    for plane, worker in ((0, 0), (0, 1), (1, 0), (2, 1)):
        eng.search_dev(d_y + plane * BM.DWELL * 8, _lib.FMT_C32)
        got = EM.best_cell(*eng.metrics(), worker)
        want = BM.search(model[plane], worker)
        print("T1 seed 1, plane %d, satellite %d: GPU %s, model %s" % (plane, worker, got, want))
        assert BM.found(got, worker) and got[:2] == want[:2] and got[2] > BM.DETECT
        assert abs(got[2] - want[2]) <= 1e-2 * want[2]
    assert bf.stats()["fallbacks"] == [0, 0, 0]
    bf.close()
    eng.close()
