"""Several constraints on one beam on the GPU (gm_lcmv, csrc/lcmv_kernels.hip) against the float64 model of lcmv_model.py, each step held
to its own bar as test_gpu_stap.py does:

  R   against the float64 sum:                                   |dR[p][q]| <= 1e-5 sum_t |z_p| |z_q|, exactly Hermitian, and bit for
      bit the R a Beamformer handle captures on the same input
  w   against the model's w computed from the DEVICE's R words:  |dw[j]|    <= 2^-22 max_j |w[j]| per beam: the single f32 rounding (the
      f64 solve adds nothing at the conditioning drawn here: cond(C^H C) <= 100, interferers 30 dB up, loading >= 1e-4)
  C^H w = f on the device's own w words:                         |c_q^H w - f_q| <= (M + 2) 2^-24 sum_j |c_q[j]| |w[j]|
  y   against the model handed the device's w words:             |dy|       <= 1e-5 sum_j |w[j]| |z_j|
  Q = 1, f = 1 against a Beamformer's w:                         |dw[j]|    <= 2^-22 max_j |w[j]|

The input is test_gpu_stap.py's: noise plus a rank-one white jammer and a CW 30 dB up, in both formats; the int8 stream holds -128.  The
constraint rows and responses are lcmv_model.draw's (test_lcmv_host.py checks that the seeds used here need no redraw).

The shapes are lcmv_model.CASES: A = 2, 3, 4 and 8 only, so six of the twelve <A, NL> of lcmv_kernel.  Every (A, L) the stage accepts runs
at B = 256 with three beams, through this file's _check, in tests/test_gpu_stage_instantiations.py."""
import ctypes as C

import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import lcmv_model as LM
import stap_model as SM
import test_gpu_beam as TB
import test_gpu_stap as TS

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
BAR_R, BAR_W, BAR_Y = TS.BAR_R, TS.BAR_W, TS.BAR_Y
_words, _stream, _bps, _fmt, _feed = TS._words, TS._stream, TS._bps, TS._fmt, TB._feed

CASES, _seed, drawn = LM.CASES, LM.case_seed, LM.drawn


def _check(tag, p, x, y, R, w, input_index=0):
    """the bars -> the largest fraction of each (R, w, C^H w = f, y)"""
    m = LM.run(p, x, input_index=input_index)
    nb, M, P = m["zb"].shape[0], p["M"], p["P"]
    assert y.shape == (P, nb * p["B"]) and R.shape == (nb, M, M) and w.shape == (nb, P, M), tag
    if not nb:
        return np.zeros(4)
    for a in (y, R, w):
        assert np.isfinite(a.view(np.float32)).all(), tag
    assert (R == np.conj(np.swapaxes(R, 1, 2))).all(), tag                                   # exactly Hermitian
    assert (_words(R[:, np.arange(M), np.arange(M)].imag) == 0).all(), tag                    # the diagonal's imaginary part is +0
    fr = float((np.abs(R.astype(np.complex128) - m["R"]) / np.maximum(m["R_weight"], 1e-300)).max())
    wm, fb = LM.weights(p, R, want_fallback=True)                      # from the device's R words
    assert not fb.any(), tag
    w128 = w.astype(np.complex128)
    fw = float((np.abs(w128 - wm) / np.abs(wm).max(axis=2, keepdims=True)).max())
    fc = fy = 0.0
    for k in range(P):
        Ck, fk = p["C"][k], p["f"][k]
        res = np.abs(np.einsum("mq,bm->bq", Ck.conj(), w128[:, k]) - fk[None, :])
        bar = (M + 2) * 2.0 ** -24 * np.einsum("mq,bm->bq", np.abs(Ck), np.abs(w128[:, k]))
        fc = max(fc, float((res / bar).max()))
        ym, yw = SM.combine(m["zb"], w[:, k])                          # handed the device's w words
        fy = max(fy, float((np.abs(y[k].astype(np.complex128) - ym) / np.maximum(yw, 1e-300)).max()))
    print("%s: R %.3g of its bar, w %.3g, C^H w = f %.3g, y %.3g" % (tag, fr / BAR_R, fw / BAR_W, fc, fy / BAR_Y))
    assert fr <= BAR_R and fw <= BAR_W and fc <= 1.0 and fy <= BAR_Y, (tag, fr, fw, fc, fy)
    return np.array([fr / BAR_R, fw / BAR_W, fc, fy / BAR_Y])


def _same(a, b):
    return all((_words(u) == _words(v)).all() for u, v in zip(a, b))


@pytest.mark.parametrize("case", CASES)
def test_every_step_at_its_own_bar(gpu, hipbuf, case):
    from gnss_sdr_rs_amd import beamformer, lcmv
    A, L, B, qs = case
    M, P = A * L, len(qs)
    cs, _ = drawn(case)
    n = 3 * B + 7
    for fmt, loading in (("i8", 1e-4), ("c32", 1e-2)):
        x = _stream(fmt, n, A, _seed(case))
        d_x = hipbuf.upload(x)
        lc = lcmv.Lcmv(A, L, cs, block=B, loading=loading)
        p = LM.resolve(A, L, cs, B, loading)
        assert (lc.block, lc.loading, lc.n_beams, lc.n_constraints) == (p["B"], p["loading"], P, qs)
        got = _feed(hipbuf, lc, d_x, fmt, n)
        assert lc.stats() == dict(inputs=n, outputs=LM.total_out(p, n), blocks=n // B, fallbacks=[0] * P)
        _check((case, fmt, loading), p, x, *got)
        # R is a Beamformer's, bit for bit; and with the beams' first rows answering 1 alone, w is a Beamformer's to the rounding
        s = np.stack([rows[0] for rows, _ in cs])
        bf = beamformer.Beamformer(A, L, s, B, loading)
        yb, Rb, wb = _feed(hipbuf, bf, d_x, fmt, n)
        bf.close()
        assert (_words(got[1]) == _words(Rb)).all()
        one = lcmv.Lcmv(A, L, [([row], [1.0]) for row in s], block=B, loading=loading)
        y1, R1, w1 = _feed(hipbuf, one, d_x, fmt, n)
        one.close()
        assert (_words(R1) == _words(Rb)).all()
        frac = np.abs(w1.astype(np.complex128) - wb.astype(np.complex128)) / np.abs(wb).max(axis=2, keepdims=True)
        assert frac.max() <= BAR_W, (case, fmt, frac.max())
        # a second run gives the same words; the host-buffer form too
        lc.reset(0)
        assert _same(_feed(hipbuf, lc, d_x, fmt, n), got)
        lc.reset(0)
        assert _same(lc.want_blocks(x), got)
        lc.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()             # the input is only read


@pytest.mark.parametrize("case,fmt", [((4, 2, 256, [2, 2, 1]), "c32"), ((3, 5, 256, [3, 3, 3, 3, 3]), "i8")])
def test_call_lengths(gpu, hipbuf, case, fmt):
    from gnss_sdr_rs_amd import lcmv
    A, L, B, qs = case
    cs, _ = drawn(case)
    lc = lcmv.Lcmv(A, L, cs, block=B)
    p = LM.resolve(A, L, cs, B)
    x = _stream(fmt, 5 * B + 7, A, 9)
    d_x = hipbuf.upload(x)
    for n in (1, L - 1, B - 1, B, B + 1, 3 * B - 1, 5 * B + 7):
        if n == 0:
            continue
        lc.reset(0)
        got = _feed(hipbuf, lc, d_x, fmt, n)
        assert got[0].shape == (len(qs), LM.plan(p, 0, n))
        _check((case, fmt, n), p, x[:n], *got)
        assert lc.stats() == dict(inputs=n, outputs=n // B * B, blocks=n // B, fallbacks=[0] * len(qs))
    lc.close()


@pytest.mark.parametrize("case,fmt", [((4, 2, 256, [2, 2, 1]), "i8"), ((3, 5, 256, [3, 3, 3, 3, 3]), "c32")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, case, fmt):
    from gnss_sdr_rs_amd import lcmv
    A, L, B, qs = case
    P = len(qs)
    cs, _ = drawn(case)
    lc = lcmv.Lcmv(A, L, cs, block=B)
    p = LM.resolve(A, L, cs, B)
    n = 3500
    x = _stream(fmt, n, A, 5)
    d_x = hipbuf.upload(x)
    for index in (0, (1 << 32) - 3, (1 << 40) + 12345):
        lc.reset(index)
        whole = _feed(hipbuf, lc, d_x, fmt, n)
        assert whole[0].shape == (P, LM.plan(p, index, n)) and whole[0].shape[1] > 0
        state = lc.stats()
        assert state == dict(inputs=n, outputs=whole[0].shape[1], blocks=whole[0].shape[1] // B, fallbacks=[0] * P)
        _check((case, fmt, index), p, x, *whole, input_index=index)
        for step in (1, 7, B - 1, 1000, 3001):
            lc.reset(index)
            assert _same(_feed(hipbuf, lc, d_x, fmt, n, step), whole), (index, step)
            assert lc.stats() == state
        lc.reset(index)
        assert _same(_feed(hipbuf, lc, d_x, fmt, n), whole), index                      # repetition
    lc.close()


def test_a_beam_depends_neither_on_p_nor_on_the_other_beams(gpu, hipbuf):
    from gnss_sdr_rs_amd import lcmv
    A, L, B = 4, 3, 256
    M = A * L
    cs, redraws = LM.draw(np.random.default_rng(21), M, [3, 1, 2, 8, 2])
    assert redraws == 0
    n = 3 * B + 5
    for fmt in ("c32", "i8"):
        x = _stream(fmt, n, A, 6)
        d_x = hipbuf.upload(x)
        five = lcmv.Lcmv(A, L, cs, block=B)
        y5, R5, w5 = _feed(hipbuf, five, d_x, fmt, n)
        five.close()
        for keep in ([2], [3], [4, 0], [3, 2, 1]):                     # alone, in another slot, behind other rows below the matrix
            few = lcmv.Lcmv(A, L, [cs[k] for k in keep], block=B)
            y, R, w = _feed(hipbuf, few, d_x, fmt, n)
            few.close()
            assert (_words(R) == _words(R5)).all()
            for i, k in enumerate(keep):
                assert (_words(y[i]) == _words(y5[k])).all() and (_words(w[:, i]) == _words(w5[:, k])).all(), (fmt, keep, k)
        assert not (_words(y5[0]) == _words(y5[1])).all()


def test_set_constraints_between_two_calls(gpu, hipbuf):
    """blocks of the first call keep the old words; blocks finished by the second take the new beam's, as a handle created with the new
    beam gives them on the whole stream; the other beams do not move.  The beam goes from two rows to three, then to one."""
    from gnss_sdr_rs_amd import lcmv
    A, L, B = 4, 2, 256
    M = A * L
    cs, r0 = LM.draw(np.random.default_rng(31), M, [2, 2, 1])
    new3, r1 = LM.draw(np.random.default_rng(32), M, [3])
    new1, r2 = LM.draw(np.random.default_rng(33), M, [1])
    assert r0 == r1 == r2 == 0
    n, first = 4 * B + 9, B + 100                                  # block 1 is begun by the first call and finished by the second
    x = _stream("c32", n, A, 13)
    d_x = hipbuf.upload(x)
    for new in (new3[0], new1[0]):
        lc = lcmv.Lcmv(A, L, cs, block=B)
        y1, R1, w1 = _feed(hipbuf, lc, d_x, "c32", first)
        lc.set_constraints(1, *new)
        assert lc.n_constraints == [2, len(new[1]), 1]
        y2, R2, w2 = _feed(hipbuf, lc, d_x + first * _bps("c32", A), "c32", n - first)
        assert lc.stats() == dict(inputs=n, outputs=4 * B, blocks=4, fallbacks=[0, 0, 0])
        lc.close()
        assert y1.shape == (3, B) and y2.shape == (3, 3 * B)
        old = lcmv.Lcmv(A, L, cs, block=B)
        yo, Ro, wo = old.want_blocks(x)
        old.close()
        moved = lcmv.Lcmv(A, L, [cs[0], new, cs[2]], block=B)
        ym, Rm, wm = moved.want_blocks(x)
        moved.close()
        assert (_words(y1) == _words(yo[:, :B])).all() and (_words(w1) == _words(wo[:1])).all() and (_words(R1) == _words(Ro[:1])).all()
        assert (_words(y2) == _words(ym[:, B:])).all() and (_words(w2) == _words(wm[1:])).all() and (_words(R2) == _words(Rm[1:])).all()
        assert (_words(ym[0]) == _words(yo[0])).all() and (_words(ym[2]) == _words(yo[2])).all() and not (_words(ym[1]) == _words(yo[1])).all()
        _check(("moved", len(new[1])), LM.resolve(A, L, [cs[0], new, cs[2]], B), x, ym, Rm, wm)


def test_static_mode_and_back(gpu, hipbuf):
    from gnss_sdr_rs_amd import lcmv
    rng = np.random.default_rng(12)
    for case, fmt in (((4, 2, 256, [2, 2, 1]), "c32"), ((8, 4, 256, [1] * 16), "i8"), ((4, 4, 1024, [2, 2]), "i8")):
        A, L, B, qs = case
        M, P = A * L, len(qs)
        n = 4 * B + 9
        x = _stream(fmt, n, A, 3)
        d_x = hipbuf.upload(x)
        cs, _ = drawn(case)
        lc = lcmv.Lcmv(A, L, cs, block=B)
        p = LM.resolve(A, L, cs, B)
        adaptive = _feed(hipbuf, lc, d_x, fmt, n)
        w = (rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M))).astype(np.complex64)
        lc.set_weights(w)
        lc.reset(0)
        y, R, wc = _feed(hipbuf, lc, d_x, fmt, n, 1000)
        assert lc.stats() == dict(inputs=n, outputs=4 * B, blocks=4, fallbacks=[0] * P)
        m = LM.run(p, x, static_w=w)
        assert float((np.abs(y.astype(np.complex128) - m["y"]) / m["y_weight"]).max()) <= BAR_Y
        assert (_words(wc) == _words(np.tile(w[None], (4, 1, 1)))).all()    # the capture holds the installed words
        assert (R.view(np.uint8) == 0x5A).all()                             # and R is not written in static mode
        # static for the first two blocks, adaptive again for the rest: the adaptive run's words, bit for bit
        lc.reset(0)
        first = _feed(hipbuf, lc, d_x, fmt, 2 * B + 5)
        assert (_words(first[0]) == _words(y[:, :2 * B])).all()
        lc.set_weights(None)
        rest = _feed(hipbuf, lc, d_x + (2 * B + 5) * _bps(fmt, A), fmt, n - 2 * B - 5)
        assert (_words(rest[0]) == _words(adaptive[0][:, 2 * B:])).all()
        assert (_words(rest[1]) == _words(adaptive[1][2:])).all() and (_words(rest[2]) == _words(adaptive[2][2:])).all()
        # the host-buffer form in static mode
        lc.set_weights(w)
        lc.reset(0)
        hy, hR, hw = lc.want_blocks(x)
        assert (_words(hy) == _words(y)).all() and (_words(hw) == _words(wc)).all() and not hR.any()
        lc.close()


def test_an_all_zero_block_and_an_overflowing_block_take_w0(gpu, hipbuf):
    """every beam of such a block takes its quiescent weights and is counted once; the blocks around it pass the bars"""
    from gnss_sdr_rs_amd import lcmv
    case = LM.FALLBACK_CASE
    A, L, B, qs = case
    M, P = A * L, len(qs)
    cs, redraws = drawn(case)
    assert redraws == 0
    p = LM.resolve(A, L, cs, B)
    w0 = p["w0"]
    for kind, fmt in (("zero", "c32"), ("zero", "i8"), ("overflow", "c32")):
        x = _stream(fmt, 4 * B, A, 8)
        if kind == "zero":
            x[B - (L - 1):2 * B] = 0                                   # block 1 and the halo it reaches back into
        else:
            x[B + 10:2 * B - 10] *= np.float32(1e18)                   # finite samples of around 3e19: the trace is not finite
            assert np.isfinite(x.view(np.float32)).all()
        lc = lcmv.Lcmv(A, L, cs, block=B)
        y, R, w = _feed(hipbuf, lc, hipbuf.upload(x), fmt, 4 * B)
        assert lc.stats() == dict(inputs=4 * B, outputs=4 * B, blocks=4, fallbacks=[1] * P), kind
        assert np.isfinite(w.view(np.float32)).all() and not np.isnan(y.view(np.float32)).any()
        for k in range(P):
            assert np.abs(w[1, k].astype(np.complex128) - w0[k]).max() <= BAR_W * np.abs(w0[k]).max(), (kind, k)
        if kind == "zero":
            assert not R[1].any() and not y[:, B:2 * B].any()
        else:
            assert not np.isfinite(R[1].view(np.float32)).all()
        with np.errstate(all="ignore"):
            wm, fb = LM.weights(p, R, want_fallback=True)              # the model on the device's R words falls back where it did
        assert fb.tolist() == [[False] * P, [True] * P, [False] * P, [False] * P], kind
        assert (np.abs(w.astype(np.complex128) - wm) / np.abs(wm).max(axis=2, keepdims=True)).max() <= BAR_W, kind
        lc.reset(0)
        assert lc.stats()["fallbacks"] == [0] * P
        lc.close()


def test_one_beam_alone_falls_back(gpu, hipbuf):
    """beam 1's row lies 0.1 off the block's strongest interference direction and answers 1e38: its quiescent weights are finite in f32
    (around 4e37) but the adaptive ones, which steer away from the interference, are not (around 8e38, in the model and on the device
    alike, a factor of two above the f32 range).  Beam 1 takes w0 in every block and is counted; beams 0 and 2 pass the bars.  The
    stream is scaled by 2^-10 so that beam 1's plane stays finite."""
    from gnss_sdr_rs_amd import lcmv
    A, L, B = 4, 2, 256
    M = A * L
    x = (_stream("c32", 3 * B, A, 23) * np.float32(2.0 ** -10)).astype(np.complex64)
    st = SM.resolve(A, L, B)
    v1 = np.linalg.eigh(SM.covariance(SM.blocks_of(st, x))[0][0])[1][:, -1]
    rng = np.random.default_rng(3)
    d = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    c = (v1 + 0.1 * d / np.linalg.norm(d)).astype(np.complex64)
    others, redraws = LM.draw(np.random.default_rng(5), M, [2, 3])
    assert redraws == 0
    cs = [others[0], ([c], [1e38]), others[1]]
    p = LM.resolve(A, L, cs, B)
    m = LM.run(p, x)
    assert m["fallback"].tolist() == [[False, True, False]] * 3
    lc = lcmv.Lcmv(A, L, cs, block=B)
    y, R, w = _feed(hipbuf, lc, hipbuf.upload(x), "c32", 3 * B)
    assert lc.stats() == dict(inputs=3 * B, outputs=3 * B, blocks=3, fallbacks=[0, 3, 0])
    lc.close()
    assert np.isfinite(w.view(np.float32)).all() and np.isfinite(y.view(np.float32)).all()
    wm, fb = LM.weights(p, R, want_fallback=True)
    assert fb.tolist() == [[False, True, False]] * 3
    assert (np.abs(w.astype(np.complex128) - wm) / np.abs(wm).max(axis=2, keepdims=True)).max() <= BAR_W
    assert np.abs(w[:, 1].astype(np.complex128) - p["w0"][1][None]).max() <= BAR_W * np.abs(p["w0"][1]).max()


@pytest.mark.parametrize("case,fmt", [((3, 5, 256, [3, 3, 3, 3, 3]), "i8"), ((8, 4, 256, [1] * 16), "i8"), ((4, 2, 256, [2, 2, 1]), "c32")])
def test_input_pointers_that_are_not_aligned(gpu, hipbuf, case, fmt):
    """the stream one, two and three elements behind an aligned address: the same words as at the aligned address"""
    from gnss_sdr_rs_amd import lcmv
    A, L, B, qs = case
    n = 3 * B + 11
    lc = lcmv.Lcmv(A, L, drawn(case)[0], block=B)
    x = _stream(fmt, n, A, 77)
    want = _feed(hipbuf, lc, hipbuf.upload(x), fmt, n)
    flat = x.reshape((n * A,) + x.shape[2:])
    for lead in (1, 2, 3):
        padded = np.concatenate([np.zeros((lead,) + flat.shape[1:], flat.dtype), flat])
        d = hipbuf.upload(padded) + lead * (2 if fmt == "i8" else 8)
        for step in (None, 100):
            lc.reset(0)
            assert _same(_feed(hipbuf, lc, d, fmt, n, step), want), (lead, step)
    lc.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, lcmv
    import test_lcmv_host as TH
    L_ = gpu.lib()
    h = C.c_void_p()

    def raw_cfg(cfg):
        c = dict(cfg)
        beams = c.pop("constraints")
        rows = np.ascontiguousarray(np.concatenate([np.asarray(r).astype(np.complex64).reshape(-1) for r, _ in beams]))
        f = np.ascontiguousarray(np.concatenate([np.asarray(v).astype(np.complex64).reshape(-1) for _, v in beams]))
        q = np.array([np.asarray(v).size for _, v in beams], np.uint32)
        keep = (q, rows, f)
        return _lib.LcmvCfg(c["n_antennas"], c["taps"], c.get("block", 0), c.get("loading", 0.0), len(q), 0, q.ctypes.data, rows.ctypes.data,
                            f.ctypes.data, 0), keep

    for cfg in TH.REFUSED:
        raw, keep = raw_cfg(cfg)
        assert L_.gm_lcmv_create(C.byref(raw), C.byref(h)) == INVALID and not h.value, cfg
    A, L, B = 4, 2, 256
    M = A * L
    cs, redraws = LM.draw(np.random.default_rng(41), M, [2, 1, 3])
    assert redraws == 0
    P = 3
    ok, keep = raw_cfg(dict(n_antennas=A, taps=L, block=B, constraints=cs))
    assert L_.gm_lcmv_create(None, C.byref(h)) == INVALID and L_.gm_lcmv_create(C.byref(ok), None) == INVALID
    for field, value in (("reserved32", 1), ("reserved", 1), ("n_beams", 0), ("n_beams", 17), ("n_constraints", None), ("constraints", None),
                         ("response", None)):
        bad, keep2 = raw_cfg(dict(n_antennas=A, taps=L, block=B, constraints=cs))
        setattr(bad, field, value)
        assert L_.gm_lcmv_create(C.byref(bad), C.byref(h)) == INVALID and not h.value, field
    lc = lcmv.Lcmv(A, L, cs, block=B)
    p = LM.resolve(A, L, cs, B)
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
    lc.capture(d_R, d_w, 8)
    n1 = lc.process_dev(d_x, _lib.FMT_C32, first, d_y, stride)
    state = lc.stats()
    assert state == dict(inputs=first, outputs=B, blocks=1, fallbacks=[0] * P) and n1 == B
    R1, w1 = hipbuf.download(d_R, 8 * M * M * 8, np.complex64), hipbuf.download(d_w, 8 * P * M * 8, np.complex64)
    raw1 = hipbuf.download(d_y, P * stride * 8, np.complex64)
    rest = n - first
    n2 = LM.plan(p, first, rest)
    assert n2 == 4 * B
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, st: L_.gm_lcmv_process_dev(lc._h, d_in, fmt, n_in, d_out, st, C.byref(got), None)
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
    lc.capture(d_R, d_w, 3)                                                        # a capture smaller than the call's four blocks
    assert call(src, _lib.FMT_C32, rest, out, stride) == OUT_OF_RANGE
    lc.capture(d_R, d_w, 8)
    assert L_.gm_lcmv_capture(lc._h, d_R, None, 8) == INVALID and L_.gm_lcmv_capture(lc._h, None, d_w, 8) == INVALID
    assert L_.gm_lcmv_capture(lc._h, d_R, d_w, 0) == INVALID and L_.gm_lcmv_capture(lc._h, None, None, 8) == INVALID
    bad = np.zeros((P, M), np.complex64)
    bad[:, 0], bad[P - 1, M - 1] = 1, np.nan
    assert L_.gm_lcmv_set_weights(lc._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    bad[P - 1, M - 1] = complex(0, np.inf)
    assert L_.gm_lcmv_set_weights(lc._h, bad.ctypes.data_as(C.c_void_p)) == INVALID
    # set_constraints: a bad row, a bad response, dependent rows, a count outside its range, a sum above 16, a bad beam, nulls
    rows = np.zeros((8, M), np.complex64)
    f = np.ones(8, np.complex64)
    rp, fp = rows.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    setc = lambda beam, nq: L_.gm_lcmv_set_constraints(lc._h, beam, nq, rp, fp)
    rows[:] = np.eye(8, M)
    rows[1] = 0
    assert setc(0, 2) == INVALID                                                   # all zero
    rows[1, 1], rows[1, 2] = 1, np.nan
    assert setc(0, 2) == INVALID                                                   # not finite
    rows[1] = rows[0]
    assert setc(0, 2) == INVALID                                                   # dependent
    rows[:] = np.eye(8, M)
    f[1] = np.inf
    assert setc(0, 2) == INVALID                                                   # a response that is not finite
    f[1] = 1
    assert setc(0, 0) == INVALID and setc(0, 9) == INVALID and setc(P, 1) == INVALID and setc(1 << 31, 1) == INVALID
    assert L_.gm_lcmv_set_constraints(lc._h, 0, 1, None, fp) == INVALID and L_.gm_lcmv_set_constraints(lc._h, 0, 1, rp, None) == INVALID
    big = lcmv.Lcmv(A, L, [cs[0]] * 2 + [(np.eye(6, M), np.ones(6))] * 2, block=B)  # 16 rows: beam 0 may not grow
    assert L_.gm_lcmv_set_constraints(big._h, 0, 3, rp, fp) == INVALID and L_.gm_lcmv_set_constraints(big._h, 0, 2, rp, fp) == 0
    big.close()
    assert got.value == 77 and lc.stats() == state
    assert L_.gm_lcmv_reset(lc._h, (1 << 62) + 1) == INVALID and lc.stats() == state
    assert (_words(hipbuf.download(d_y, P * stride * 8, np.complex64)) == _words(raw1)).all()      # nothing was written
    assert (raw1.reshape(P, stride)[:, n1:].view(np.uint8) == 0x5A).all()
    assert (_words(hipbuf.download(d_R, 8 * M * M * 8, np.complex64)) == _words(R1)).all()
    assert (_words(hipbuf.download(d_w, 8 * P * M * 8, np.complex64)) == _words(w1)).all()
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and lc.stats() == state    # n_in = 0
    # the next good call continues the stream as if nothing had been refused (the refused rows and weights changed nothing); planes
    # right behind d_in are no overlap
    behind = d_x + n * A * 8
    assert call(src, _lib.FMT_C32, rest, behind, stride) == 0 and got.value == n2
    lc.synchronize()
    tail = hipbuf.download(behind, P * stride * 8, np.complex64).reshape(P, stride)
    y = np.concatenate([raw1.reshape(P, stride)[:, :n1], tail[:, :n2]], axis=1)
    R = np.concatenate([R1.reshape(8, M, M)[:1], hipbuf.download(d_R, 4 * M * M * 8, np.complex64).reshape(4, M, M)])
    w = np.concatenate([w1.reshape(8, P, M)[:1], hipbuf.download(d_w, 4 * P * M * 8, np.complex64).reshape(4, P, M)])
    assert lc.stats() == dict(inputs=n, outputs=5 * B, blocks=5, fallbacks=[0] * P)
    _check("after the refusals", p, x, y, R, w)
    # the host-buffer form: the same words, the same refusals
    lc.reset(0)
    assert _same(lc.want_blocks(x), (y, R, w))
    small = np.zeros(P * 4, np.complex64)
    xp = x.ctypes.data_as(C.c_void_p)
    sp4 = small.ctypes.data_as(C.c_void_p)
    assert L_.gm_lcmv_process(lc._h, xp, _lib.FMT_C32, 300, sp4, 4, None, None, None, 0) == OUT_OF_RANGE
    assert L_.gm_lcmv_process(lc._h, xp, _lib.FMT_I8_REAL, 100, sp4, 4, None, None, None, 0) == INVALID
    bigy = np.zeros(P * 2 * B, np.complex64)
    wbuf = np.zeros((1, P, M), np.complex64)
    assert L_.gm_lcmv_process(lc._h, xp, _lib.FMT_C32, 2 * B, bigy.ctypes.data_as(C.c_void_p), 2 * B, None, None,
                              wbuf.ctypes.data_as(C.c_void_p), 1) == OUT_OF_RANGE
    assert lc.stats()["inputs"] == n and not small.any() and not bigy.any() and not wbuf.any()
    lc.close()


@pytest.mark.parametrize("case,fmt", [((4, 2, 256, [2, 2, 1]), "c32"), ((3, 5, 256, [3, 3, 3, 3, 3]), "i8")])
def test_process_dev_on_a_callers_stream_that_is_held_back(gpu, case, fmt):
    """the producer's H2D, two process_dev calls with a capture and the consumer's D2H all behind a held gate on the caller's stream,
    nothing waited for until the last library call has returned: bit for bit the synchronous run's words"""
    from gnss_sdr_rs_amd import lcmv
    A, L, B, qs = case
    M, P = A * L, len(qs)
    n, cut = 3 * B + 50, B + 77
    x = _stream(fmt, n, A, 19)
    cs, _ = drawn(case)
    ref = lcmv.Lcmv(A, L, cs, block=B)
    want = ref.want_blocks(x)
    want_stats = ref.stats()
    ref.close()
    with SS.HeldStream() as S:
        lc = S.own(lcmv.Lcmv(A, L, cs, block=B))
        d_x, d_y = S.device(x.nbytes), S.device(P * 3 * B * 8)
        d_R, d_w = S.device(3 * M * M * 8), S.device(3 * P * M * 8)
        staged = S.stage(x)
        S.hold("lcmv %d %d %d %d %s" % (A, L, B, P, fmt))
        S.h2d(d_x, staged)
        lc.capture(d_R, d_w, 3)
        n1 = lc.process_dev(d_x, _fmt(fmt), cut, d_y, 3 * B, stream=S.stream)
        lc.capture(d_R + (n1 // B) * M * M * 8, d_w + (n1 // B) * P * M * 8, 3 - n1 // B)
        n2 = lc.process_dev(d_x + cut * _bps(fmt, A), _fmt(fmt), n - cut, d_y + n1 * 8, 3 * B, stream=S.stream)
        hy, hR, hw = S.d2h(d_y, P * 3 * B * 8), S.d2h(d_R, 3 * M * M * 8), S.d2h(d_w, 3 * P * M * 8)
        S.assert_held()
        S.sync()
        assert n1 + n2 == 3 * B
        got = (hy.view(np.complex64).reshape(P, 3 * B), hR.view(np.complex64).reshape(3, M, M), hw.view(np.complex64).reshape(3, P, M))
        assert _same(got, want)
        assert lc.stats() == want_stats


def test_the_scene_through_the_beams_and_a_plain_search(gpu, hipbuf):
    """the spoofer scene of seed 1 (A = 4, a white jammer 40 dB up, the satellite at lag 700 and the same code again at lag 1200 from
    another direction) through Lcmv(4, 1, lcmv_model.spoofer_beams) at B = 1024, each plane straight from device memory into a plain
    search_dev at fft_size 2048.  The host test's three facts, with every ratio taken to the plane's mean without its peak: behind the
    single row lag 1200 of bin 2 stands above the detector's 7; behind rows (1, 0) it is below 3 and the engine's best cell is
    (bin 2, 700), above 7; behind rows (0, 1) the engine's best cell is (bin 2, 1200) and lag 700 is below 3.  The best cells are the
    engine's own (search_dev on the device plane); the ratios at a named lag are the float64 search of the device plane's words, since
    the engine reports each bin's peak alone.  Each best cell agrees with the model's on the same input to 1 %: a guard against a wrong
    plane, not a parity bar; the parity bars are the cases above."""
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, lcmv
    import excise_model as EM
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == LM.DWELL
    x = LM.spoofer_scene(1).astype(np.complex64)
    A, L = x.shape[1], 1
    cs = LM.spoofer_beams(A, L)
    lc = lcmv.Lcmv(A, L, cs, block=1024, loading=1e-4)
    d_y = hipbuf.alloc(3 * LM.DWELL * 8)
    assert lc.process_dev(hipbuf.upload(x), _lib.FMT_C32, x.shape[0], d_y, LM.DWELL) == LM.DWELL
    lc.synchronize()
    assert lc.stats()["fallbacks"] == [0, 0, 0]
    lc.close()
    y = hipbuf.download(d_y, 3 * LM.DWELL * 8, np.complex64).reshape(3, LM.DWELL)
    model = LM.beams(x, L, cs)
    sat, other = (LM.SAT["bin"], LM.SAT["code_phase"]), (LM.SPOOF["bin"], LM.SPOOF["code_phase"])
    cells = []
    for plane in range(3):
        eng.search_dev(d_y + plane * LM.DWELL * 8, _lib.FMT_C32)
        mx, am, sm = (np.asarray(a).reshape(2, -1)[0].astype(np.float64) for a in eng.metrics())
        ratio = mx / ((sm - mx) / (LM.N - 1))                         # per bin: the peak over the plane's mean without it
        d = int(np.argmax(ratio))
        got = (d, int(am[d]), float(ratio[d]))
        want = LM.best(LM.planes(model[plane]))
        r = LM.ratios(LM.planes(y[plane])[LM.SAT["bin"]])             # the GPU plane's own words, every lag of bin 2
        cells.append(dict(best=got, sat=float(r[sat[1]]), other=float(r[other[1]])))
        print("spoofer scene seed 1, plane %d: GPU best %s, model best %s; lag 700 %.1f, lag 1200 %.1f" % (plane, got, want, r[sat[1]], r[other[1]]))
        assert got[:2] == want[:2] and abs(got[2] - want[2]) <= 1e-2 * want[2]
    one, keep, swap = cells
    assert one["other"] > LM.DETECT
    assert keep["other"] < 3.0 and keep["best"][:2] == sat and keep["best"][2] > LM.DETECT
    assert swap["sat"] < 3.0 and swap["best"][:2] == other and swap["best"][2] > LM.DETECT
    eng.close()
