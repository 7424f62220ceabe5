"""Every (A, L) that gm_stap, gm_beamformer and gm_lcmv accept, on the GPU against the float64 models: the 43 pairs of
stage_instantiations.py, so every <A, NL> of stap_kernel, beam_kernel and lcmv_kernel and, within a form, every way the lags fall on the
four waves of st_gram (a wave carries the lags `wave` and `wave + 4` below L: L = 7 leaves wave 3 with one lag and the others with two,
L = 3 leaves wave 3 with none).  The other five stages' forms run in their own files; tests/test_stage_instantiations_host.py reads
those files' parametrisations and checks that they reach every form.

Per case: B = 256, both formats (the int8 stream holds -128), 3 B + 7 time samples of test_gpu_stap.py's stream: three blocks, the
first with its halo of zeros, then a pending tail.  Once in one call and once in calls of 300, which end at 300, 600 and 775, so that
blocks 1 and 2 are begun by one call and finished by the next: the words of y and of the captured R and w are equal bit for bit.
The one-call words go through the stage's own _check, so every bar is the one already in force:

  R   against the float64 sum:                                   |dR[p][q]| <= 1e-5 sum_t |z_p| |z_q|
  w   against the model's w computed from the DEVICE's R words:  |dw[p]|    <= 2^-22 max_p |w[p]|
  y   against the model handed the device's w words:             |dy|       <= 1e-5 sum_p |w[p]| |z_p|
  gm_lcmv also: C^H w = f on the device's own w words:           |c_q^H w - f_q| <= (M + 2) 2^-24 sum_j |c_q[j]| |w[j]|

No block falls back (the host test shows that the model takes none on these streams), and _feed checks that the words behind the
outputs and behind the captured blocks stay as filled.  Each case prints the largest fraction of each bar it saw."""
import numpy as np
import pytest

import beam_model as BM
import lcmv_model as LM
import stage_instantiations as SI
import stap_model as SM
import test_gpu_beam as TB
import test_gpu_lcmv as TL
import test_gpu_stap as TS

pytestmark = pytest.mark.gpu
B, N, STEP, LOADING = SI.SWEEP_BLOCK, SI.SWEEP_N, SI.SWEEP_STEP, SI.SWEEP_LOADING
_words = TS._words


def _same(a, b):
    return all(u.shape == v.shape and (_words(u) == _words(v)).all() for u, v in zip(a, b))


@pytest.mark.parametrize("A,L", SI.PAIRS)
def test_stap_at_every_pair(gpu, hipbuf, A, L):
    """e_0 on the int8 stream, a random complex s on the c32 one"""
    from gnss_sdr_rs_amd import stap
    M = A * L
    s = (np.random.default_rng(M).standard_normal(M) + 1j * np.random.default_rng(B + L).standard_normal(M)).astype(np.complex64)
    worst = np.zeros(3)
    for fmt, steering in (("i8", None), ("c32", s)):
        x = TS._stream(fmt, N, A, SI.sweep_seed(A, L))
        d_x = hipbuf.upload(x)
        st = stap.Stap(A, L, B, LOADING, steering)
        p = SM.resolve(A, L, B, LOADING, steering)
        whole = TS._feed(hipbuf, st, d_x, fmt, N)
        assert st.stats() == dict(inputs=N, outputs=3 * B, blocks=3, fallback_blocks=0)
        worst = np.maximum(worst, TS._check(("stap", A, L, fmt), p, x, *whole))
        st.reset(0)
        cut = TS._feed(hipbuf, st, d_x, fmt, N, STEP)
        assert _same(cut, whole), (A, L, fmt)
        assert st.stats() == dict(inputs=N, outputs=3 * B, blocks=3, fallback_blocks=0)
        st.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()           # the input is only read
    print("sweep stap (%d, %d) <%d, %d>: R %.3g of its bar, w %.3g, y %.3g" % ((A, L) + SI.array_form(A, L) + tuple(worst)))


@pytest.mark.parametrize("A,L", SI.PAIRS)
def test_beamformer_at_every_pair(gpu, hipbuf, A, L):
    """five rows of test_gpu_beam.py's recipe (random complex rows, the last one e_0): a full group of four beams and a partial one.
    Each beam goes against the model as the stap with its row, and against a Stap handle with its row bit for bit"""
    from gnss_sdr_rs_amd import beamformer
    M, P = A * L, SI.BEAM_ROWS
    rows = TB._rows(P, M, 7 * M + P, e0_last=True)
    worst = np.zeros(3)
    for fmt in ("i8", "c32"):
        x = TS._stream(fmt, N, A, SI.sweep_seed(A, L))
        d_x = hipbuf.upload(x)
        bf = beamformer.Beamformer(A, L, rows, B, LOADING)
        p = BM.resolve(A, L, rows, B, LOADING)
        whole = TB._feed(hipbuf, bf, d_x, fmt, N)
        stats = bf.stats()
        assert stats == dict(inputs=N, outputs=3 * B, blocks=3, fallbacks=[0] * P)
        for k in range(P):
            worst = np.maximum(worst, TS._check(("beamformer", A, L, fmt, k), p["beams"][k], x, whole[0][k], whole[1], whole[2][:, k]))
        TB._same(whole, stats["fallbacks"], TB._staps(A, L, B, LOADING, rows, x), (A, L, fmt))
        assert (whole[2][:, P - 1, 0].real == np.float32(1.0)).all()                            # the e_0 row: Re w[0] = 1
        bf.reset(0)
        cut = TB._feed(hipbuf, bf, d_x, fmt, N, STEP)
        assert _same(cut, whole), (A, L, fmt)
        assert bf.stats() == stats
        bf.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()
    print("sweep beamformer (%d, %d) <%d, %d>: R %.3g of its bar, w %.3g, y %.3g" % ((A, L) + SI.array_form(A, L) + tuple(worst)))


@pytest.mark.parametrize("A,L", SI.PAIRS)
def test_lcmv_at_every_pair(gpu, hipbuf, A, L):
    """three beams of stage_instantiations.lcmv_qs(M) rows (all different but at M = 2), drawn by lcmv_model.draw from the case's seed
    (no redraw: the host test)"""
    from gnss_sdr_rs_amd import lcmv
    case = SI.lcmv_case(A, L)
    qs = case[3]
    P = len(qs)
    cs, redraws = LM.drawn(case)
    assert redraws == 0
    worst = np.zeros(4)
    for fmt in ("i8", "c32"):
        x = TS._stream(fmt, N, A, LM.case_seed(case))
        d_x = hipbuf.upload(x)
        lc = lcmv.Lcmv(A, L, cs, block=B, loading=LOADING)
        p = LM.resolve(A, L, cs, B, LOADING)
        assert lc.n_constraints == qs
        whole = TB._feed(hipbuf, lc, d_x, fmt, N)
        stats = lc.stats()
        assert stats == dict(inputs=N, outputs=3 * B, blocks=3, fallbacks=[0] * P)
        worst = np.maximum(worst, TL._check(("lcmv", A, L, fmt), p, x, *whole))
        lc.reset(0)
        cut = TB._feed(hipbuf, lc, d_x, fmt, N, STEP)
        assert _same(cut, whole), (A, L, fmt)
        assert lc.stats() == stats
        lc.close()
        assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()
    print("sweep lcmv (%d, %d) <%d, %d>: R %.3g of its bar, w %.3g, C^H w = f %.3g, y %.3g" % ((A, L) + SI.array_form(A, L) + tuple(worst)))
