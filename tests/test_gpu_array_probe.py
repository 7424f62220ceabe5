"""Beam rows from the array's own correlations (gm_acq_array_prompts, csrc/acq_array.hip; gm_array_row_solve) on the GPU.

1. Parity.  Every word of z against the float64 model of array_probe_model.py within REL = 1e-5 (the project's bar) of its envelope
   sum_n |x_a[s + n - l]| (|ref| = 1); the header's order gives about (N / 128 + 12) 2^-24 of it, 8.3e-6 at N = 16368 and 1.7e-6 at
   N = 2048.  Shapes, both formats, -128 in the int8 stream: N = 2048 with (A, L) = (2, 1), (3, 2), (4, 2), (4, 8), (8, 4), (8, 1); the
   smallest size gm_fft_supported_sizes lists with (4, 2) (N at or below one tile); N = 8184 with (3, 3) (no multiple of 256); N = 2048
   with (4, 2), K = 2, M = 3, the code drift T = N - 0.4, an edge search and candidates at non-zero offsets.  Candidates: cp = 0, 1,
   N - 1, the first and the last bin, both workers; calls of 1, 5 and 40 candidates.
2. Zero halo: with a 0 Hz bin (table words 1 + 0j) and int8 samples every sum is a sum of integers below 2^24, so the device's words
   EQUAL the model's — at o = 0, i = 0, l > 0, where the first l terms are missing, and everywhere else.  The input sits at the start of
   an allocation: nothing in front of it may be read.
3. Bit for bit: a candidate alone equals the same candidate among 40 (inside test 1); a second call equals the first; an input
   pointer offset by one element equals the aligned copy.
4. Cross-check at L = 1: antenna a's words against gm_acq_local_search(lag_half_window = 0, want_prompts) on the de-interleaved antenna,
   within 2 REL of the envelope (the order of the sum differs).
5. Every refusal: z stays full of sentinels, the metrics stay, a following refine_doppler gives the words it gave before.
6. The chain on the device, T1 of seed 1: Beamformer(4, 2, [e_0]) with capture, plane 0 into search_dev, array_prompts at the two found
   cells on the same device input, solve_rows with the captured R, Beamformer(4, 2, [e_0, row0, row1]), each plane into search_dev.

Measured on an MI355X: the largest fraction of test 1 is 1.8e-8 (N = 256, int8; 5.7e-9 to 9.2e-9 at the other sizes: the test streams
carry a jammer 30 dB up, so the envelopes are large), of test 4 1.3e-8; the chain gives 93.778 (model 93.779) and 54.4641 (54.4653)
behind the estimated rows, 53.471 and 41.4449 behind e_0."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_stap as TS           # (imports torch before the HIP library)
import test_gpu_local_search as TL
import acq_model as AM
import array_probe_model as PM
import beam_model as BM
import excise_model as EM
import stap_model as SM
from test_array_probe_host import BARS

pytestmark = pytest.mark.gpu
REL = AM.REL
INVALID = -1
DOP = np.array([-500.0, 0.0, 500.0], np.float32)
P, D = 2, 3
_words, _stream, _fmt = TS._words, TS._stream, TS._fmt


def _chips():
    return np.where(np.random.default_rng(11).integers(0, 2, (P, 1023)) > 0, 1, -1).astype(np.int8)


_ENGINES = {}


def _setup(N, special=False):
    """an engine at fft_size N (K = 1, M = 3; special: K = 2, M = 3, the code drift T = N - 0.4 in every bin, an edge search over
    offsets (0, 2) with the row (1, -1)) and what the model needs: the device's tables, the sampled codes, the period starts;
    built once per size and shared"""
    from gnss_sdr_rs_amd import acquisition as AQ
    key = (N, special)
    if key not in _ENGINES:
        fs = N * 1000.0
        K = 2 if special else 1
        eng = AQ.AcquisitionEngine(fs, 0.0, N, doppler_hz=DOP, prn_ids=[1, 2], n_integrations=3, codes=_chips(), code_rate=1.023e6,
                                   coherent_periods=K)
        R_u, o_max = K * 3, 0
        starts = np.arange(R_u, dtype=np.int64)[None, :].repeat(D, 0) * N
        if special:
            eng.set_edge_search([0, 2], [1, -1])
            eng.set_code_drift(N - 0.4)
            o_max = 2
            starts = np.floor(np.arange(R_u + o_max)[None, :].repeat(D, 0) * (N - 0.4) + 0.5).astype(np.int64)
            assert (eng.code_drift_starts().astype(np.int64) == starts).all()
        dwell = int(eng.dwell_samples)
        assert dwell == int(starts.max()) + N and AQ.array_plan(K, 3, 4, 2) == dict(periods=R_u, words_per_cand=R_u * 8)
        _ENGINES[key] = dict(eng=eng, N=N, fs=fs, K=K, R_u=R_u, o_max=o_max, starts=starts, dwell=dwell, tab=eng.tables(),
                             codes=AM.sample_codes(_chips(), 1.023e6, fs, N))
    return _ENGINES[key]


def _cands(N, o_max, n=40):
    """40 candidates: cp = 0, 1, N - 1 in the first and the last bin for both workers first, then a seeded spread over every
    worker, bin, code phase and offset"""
    rng = np.random.default_rng(N)
    out = [TL._cand(w, d, cp, o_max if (w + d) % 2 else 0) for d in (0, D - 1) for cp in (0, 1, N - 1) for w in range(P)]
    while len(out) < n:
        out.append(TL._cand(rng.integers(P), rng.integers(D), rng.integers(N), rng.integers(o_max + 1)))
    return out[:n]


def _model(s, x, cand, A, L):
    return PM.prompts(x, s["tab"][cand["doppler_bin"]], s["codes"][cand["worker"]], s["N"], s["starts"][cand["doppler_bin"]],
                      cand["offset_periods"], s["R_u"], cand["code_phase_samples"], L, want_envelope=True)


def _fraction(s, x, cands, got, A, L):
    """the largest |z_dev - z_model| / envelope over the candidates' words"""
    worst = 0.0
    for c, z in zip(cands, got):
        want, env = _model(s, x, c, A, L)
        assert z.shape == want.shape == (s["R_u"], L, A)
        worst = max(worst, float(np.max(np.abs(z.astype(np.complex128) - want) / env)))
    return worst


def _smallest():
    from gnss_sdr_rs_amd import fft
    return int(min(fft.supported_sizes()))


SHAPES = [(2048, 2, 1, False), (2048, 3, 2, False), (2048, 4, 2, False), (2048, 4, 8, False), (2048, 8, 4, False), (2048, 8, 1, False),
          ("smallest", 4, 2, False), (8184, 3, 3, False), (2048, 4, 2, True)]


# ---- 1. parity, and a candidate alone against the same candidate among 40 --------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c32", "i8"])
@pytest.mark.parametrize("N,A,L,special", SHAPES, ids=["%s-A%d-L%d%s" % (n, a, l, "-drift-edge" if sp else "") for n, a, l, sp in SHAPES])
def test_every_word_against_the_model(gpu, hipbuf, N, A, L, special, fmt):
    if N == "smallest":
        N = _smallest()
        assert N <= 1024                                                  # at or below one tile of the kernel
    s = _setup(N, special)
    eng = s["eng"]
    xd = _stream(fmt, s["dwell"], A, 100 * A + L)
    if fmt == "i8":
        assert (xd == -128).any()
    x = SM.as_c128(xd)
    d_x = hipbuf.upload(xd)
    cands = _cands(N, s["o_max"])
    if special:
        assert any(c["offset_periods"] for c in cands[:12])
    z40 = eng.array_prompts(cands, d_x, A, L, _fmt(fmt))
    z5 = eng.array_prompts(cands[:5], d_x, A, L, _fmt(fmt))
    z1 = eng.array_prompts([cands[17]], d_x, A, L, _fmt(fmt))
    assert z40.shape == (40, s["R_u"], L, A) and z40.dtype == np.complex64 and z5.shape[0] == 5 and z1.shape[0] == 1
    worst = _fraction(s, x, cands, z40, A, L)
    print("N %d, A %d, L %d, %s%s: largest |z - model| / envelope %.2e (bar %.0e)" % (N, A, L, fmt, ", drift + edge" if special else "",
                                                                                       worst, REL))
    assert worst <= REL
    assert (_words(z5) == _words(z40[:5])).all() and (_words(z1[0]) == _words(z40[17])).all()
    assert not (_words(z40[0]) == _words(z40[2])).all()


# ---- 2. the zero halo --------------------------------------------------------------------------------------------------------------------
def test_the_zero_halo_is_exact(gpu, hipbuf):
    N, A, L = 2048, 4, 8
    s = _setup(N)
    assert DOP[1] == 0.0 and (s["tab"][1] == np.complex64(1.0)).all()
    xd = _stream("i8", s["dwell"], A, 7)
    d_x = hipbuf.upload(xd)                                              # the start of an allocation
    cands = [TL._cand(w, 1, cp, 0) for w in range(P) for cp in (0, 1, 700, N - 1)]
    got = s["eng"].array_prompts(cands, d_x, A, L, _fmt("i8"))
    x = SM.as_c128(xd)
    for c, z in zip(cands, got):
        want, env = _model(s, x, c, A, L)
        assert env.max() < 2.0 ** 24 / 1.5                                # |re| + |im| sums stay below 2^24: every partial sum is exact
        assert (z.astype(np.complex128)[0, 1:] == want[0, 1:]).all(), c   # o = 0, i = 0, l > 0: the first l terms are missing
        assert (z.astype(np.complex128) == want).all(), c


# ---- 3. bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,L,fmt", [(4, 2, "c32"), (8, 4, "i8"), (3, 3, "i8"), (2, 8, "c32")])
def test_repetition_and_an_unaligned_pointer(gpu, hipbuf, A, L, fmt):
    N = 2048
    s = _setup(N)
    xd = _stream(fmt, s["dwell"], A, 31 * A + L)
    cands = _cands(N, 0)[:12]
    d_x = hipbuf.upload(xd)
    first = s["eng"].array_prompts(cands, d_x, A, L, _fmt(fmt))
    again = s["eng"].array_prompts(cands, d_x, A, L, _fmt(fmt))
    assert (_words(first) == _words(again)).all()
    # one element (8 or 2 bytes) in front: period starts leave the wide loads' alignment
    flat = np.ascontiguousarray(xd).reshape(-1) if fmt == "c32" else np.ascontiguousarray(xd).reshape(-1, 2)
    padded = np.concatenate([flat[:1], flat])
    elem = 8 if fmt == "c32" else 2
    d_p = hipbuf.upload(padded)
    moved = s["eng"].array_prompts(cands, d_p + elem, A, L, _fmt(fmt))
    assert (_words(first) == _words(moved)).all()


# ---- 4. the cross-check against gm_acq_local_search ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c32", "i8"])
def test_tap_zero_is_local_searchs_prompt_per_antenna(gpu, hipbuf, fmt):
    N, A = 2048, 3
    s = _setup(N)
    eng = s["eng"]
    xd = _stream(fmt, s["dwell"], A, 5)
    x = SM.as_c128(xd)
    cands = _cands(N, 0)[:12]
    got = eng.array_prompts(cands, hipbuf.upload(xd), A, 1, _fmt(fmt))
    worst = 0.0
    for a in range(A):
        d_a = hipbuf.upload(np.ascontiguousarray(xd[:, a]))
        ref = eng.local_search(cands, samples=d_a, lag_half_window=0, want_prompts=True, fmt=_fmt(fmt))
        for c, z, r in zip(cands, got, ref):
            assert r["prompts"].shape == (1, s["R_u"])
            env = _model(s, x, c, A, 1)[1][:, 0, a]
            worst = max(worst, float(np.max(np.abs(z[:, 0, a].astype(np.complex128) - r["prompts"][0].astype(np.complex128)) / env)))
    print("%s: largest |z - local_search's prompt| / envelope %.2e (bar %.0e)" % (fmt, worst, 2 * REL))
    assert worst <= 2 * REL


# ---- 5. every refusal --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing_and_leaves_the_handle_alone(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib
    N, A, L = 2048, 4, 2
    eng, c, am, off = TL._searched(oracle, N, "lds", 0, 2)           # coherent (K = 3, M = 2), c32, no edge search, searched
    R_u = c["K"] * c["M"]
    xd = _stream("c32", int(eng.dwell_samples), A, 9)
    d_x = hipbuf.upload(xd)
    res = [dict(doppler_bin=1, code_phase_samples=int(am[w, 1])) for w in range(AM.P)]
    metrics_before = [_words(a).copy() for a in eng.metrics()]
    refine_before = eng.refine_doppler(res, want_prompts=True, want_spectrum=True)
    ok = (0, 1, 5, 0)
    SENT = np.complex64(7 + 7j)

    def call(cands, samples=d_x, fmt=0, A=A, L=L, null=None, n=None):
        cs = (_lib.AcqCand * max(len(cands), 1))(*[_lib.AcqCand(*t) for t in cands])
        z = np.full(3 * R_u * 32, SENT)
        st = _lib.lib().gm_acq_array_prompts(None if null == "handle" else eng._h, None if null == "samples" else C.c_void_p(samples), fmt,
                                             A, L, None if null == "cands" else C.cast(cs, C.c_void_p), len(cands) if n is None else n,
                                             None if null == "z" else z.ctypes.data_as(C.c_void_p))
        return st, bool((z == SENT).all()), z

    st, untouched, z = call([ok, ok])
    assert st == 0 and not (z[:2 * R_u * A * L] == SENT).any() and (z[2 * R_u * A * L:] == SENT).all()
    bad = [dict(cands=[ok], null="handle"), dict(cands=[ok], null="samples"), dict(cands=[ok], null="cands"),
           dict(cands=[ok], fmt=_lib.FMT_I8_REAL), dict(cands=[ok], fmt=3), dict(cands=[ok], fmt=-1),
           dict(cands=[ok], A=1), dict(cands=[ok], A=9), dict(cands=[ok], A=0), dict(cands=[ok], L=0), dict(cands=[ok], L=9),
           dict(cands=[ok], A=5, L=7), dict(cands=[ok], A=8, L=5),                       # A L > 32
           dict(cands=[ok], n=1025),                                                     # (refused before a candidate is read)
           dict(cands=[ok, (AM.P, 1, 5, 0)]), dict(cands=[ok, (0, AM.D, 5, 0)]), dict(cands=[(0, -1, 5, 0)]),
           dict(cands=[ok, (0, 1, N, 0)]), dict(cands=[(0, 1, 5, 1)])]                   # no edge search: the offset must be 0
    for kw in bad:
        st, untouched, _ = call(**kw)
        assert st == INVALID and untouched, kw
    assert _lib.lib().gm_acq_array_prompts(eng._h, C.c_void_p(d_x), 0, A, L, C.cast((_lib.AcqCand * 1)(), C.c_void_p), 1, None) == INVALID
    st, untouched, _ = call([])                                           # n_cands = 0: GM_OK, nothing written
    assert st == 0 and untouched
    for a, b in zip(metrics_before, [_words(a) for a in eng.metrics()]):
        assert (a == b).all()
    for a, b in zip(refine_before, eng.refine_doppler(res, want_prompts=True, want_spectrum=True)):
        TL._same_entry(a, b)
    eng.close()


# ---- 6. the chain ------------------------------------------------------------------------------------------------------------------------
def test_the_rows_come_from_the_arrays_own_correlations(gpu, hipbuf):
    """T1 of seed 1 on the device, the steps of the docstring.  Both satellites are found at their true cells behind their estimated rows;
    each peak-to-mean is within 1 % of the model's for the same steps (the beam chain's bar: a guard against a wrong plane, not a parity
    bar) and above the e_0 plane's by the host test's bar for T1 at L = 2."""
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, beamformer
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == BM.DWELL
    x = BM.scene("T1", 1).astype(np.complex64)
    A, L, M = x.shape[1], 2, 8
    assert (A, BM.TAPS["T1"], x.shape[0]) == (4, L, BM.DWELL)
    nb = BM.DWELL // 1024
    e0 = BM.rows(A, L)[:1]
    d_x = hipbuf.upload(x)
    # 1, 2: the e_0 beam with capture, its plane into the search
    bf = beamformer.Beamformer(A, L, e0, 1024, 1e-4)
    d_y, d_R, d_w = hipbuf.alloc(BM.DWELL * 8), hipbuf.alloc(nb * M * M * 8), hipbuf.alloc(nb * M * 8)
    bf.capture(d_R, d_w, nb)
    assert bf.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y, BM.DWELL) == BM.DWELL
    bf.synchronize()
    R = hipbuf.download(d_R, nb * M * M * 8, np.complex64).reshape(nb, M, M)
    eng.search_dev(d_y, _lib.FMT_C32)
    first = [EM.best_cell(*eng.metrics(), w) for w in (0, 1)]
    assert all(BM.found(first[w], w) and first[w][2] > BM.DETECT for w in (0, 1)), first
    bf.close()
    # 3, 4: the prompts at the two found cells on the same device input, the rows with the captured R
    cands = [TL._cand(w, first[w][0], first[w][1], 0) for w in (0, 1)]
    z = eng.array_prompts(cands, d_x, A, L, _lib.FMT_C32)
    rows, infos = AQ.solve_rows(z, R, 1e-4)
    assert rows.shape == (2, L, A) and all(i["lambda1"] >= 2.0 * i["lambda2"] for i in infos), infos
    # the model for the same steps
    xm = x.astype(np.complex128)
    Rm = PM.gram(xm, L)
    est, _ = PM.estimated_rows(xm, L, Rm)
    model = PM.beams(xm, L, np.concatenate([e0, est]), Rm)
    for w in (0, 1):
        print("satellite %d: largest |row - model's row| %.2e" % (w, np.abs(rows[w].reshape(-1) - est[w]).max()))
    # 5, 6: the three beams, each plane into the search
    bf = beamformer.Beamformer(A, L, np.concatenate([e0, rows.reshape(2, M)]), 1024, 1e-4)
    d_y3 = hipbuf.alloc(3 * BM.DWELL * 8)
    assert bf.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y3, BM.DWELL) == BM.DWELL
    bf.synchronize()
    got = {}
    for plane, w in ((0, 0), (0, 1), (1, 0), (2, 1)):
        eng.search_dev(d_y3 + plane * BM.DWELL * 8, _lib.FMT_C32)
        got[(plane, w)] = EM.best_cell(*eng.metrics(), w)
        want = BM.search(model[plane], w)
        print("T1 seed 1, plane %d, satellite %d: GPU %s, model %s, lambda1 / lambda2 %.1f"
              % (plane, w, got[(plane, w)], want, infos[w]["lambda1"] / infos[w]["lambda2"]))
        assert BM.found(got[(plane, w)], w) and got[(plane, w)][:2] == want[:2] and got[(plane, w)][2] > BM.DETECT
        assert abs(got[(plane, w)][2] - want[2]) <= 1e-2 * want[2]
    for w in (0, 1):
        assert got[(1 + w, w)][2] >= BARS[("T1", 2)][1] * got[(0, w)][2], (w, got)
    assert bf.stats()["fallbacks"] == [0, 0, 0]
    bf.close()
    eng.close()
