"""Every kernel class of gm_acq_array_prompts (csrc/acq_array.hip) and gm_trk_array_prompts (csrc/trk_array.hip) on both load forms,
against the float64 models of array_probe_model.py and trk_array_model.py.

The two files build <FMT, A, LC> for 26 (A, tap class) a format, and each holds 22 load forms (array_prompt_classes.py states both
rules; test_array_prompt_classes_host.py holds the list below to the library's plan entries and to the tables).  The neighbouring files
test_gpu_array_probe.py and test_gpu_trk_array.py run seven (A, L) pairs; this one runs all 43, each on c32 and int8 IQ, each from an
aligned pointer and from a pointer one element (8 or 2 bytes) off, which selects the element loads wherever a wide form exists.

Shapes: the smallest that cross the kernels' own edges.  Acquisition: N = 2048, K = 1, M = 3 (three tiles of 1024 time samples once
L > 1, so the L - 1 halo passes from one LDS image to the next twice).  Tracking: n = 4097, fs = 1000 n, a FIXED-mode C/A handle (a second
slice of ONE time sample; the taps of slice 0's last samples reach ref words behind the slice edge).

Per (A, L) and kernel:
(a) Exact.  An int8 IQ stream with -128 in it against a reference of +-1 (acquisition: the 0 Hz bin, whose table words are 1 + 0j;
    tracking: carrier_freq = 0, carrier_phase = 0): every sum is a sum of integers whose |re| + |im| stays below 2^24 / 1.5 (asserted on the
    envelope, and on the worst case in the host test), so the device's words EQUAL the model's, every period, tap and antenna.  The same
    integers as a complex64 stream give the int8 run's words bit for bit, and so do both streams from a buffer with one element in
    front.  The unshifted input sits at the start of its allocation; the element in front of the shifted copy and 64 bytes behind it
    are 0x5A (90 + 90j as int8, 1.5e16 as f32): one of them in a sum breaks the equality.
    Acquisition: both workers at cp = 0, 1, 700, N - 1.  Tracking: records at s = 0, 1, 3, L - 2, L - 1, L, 1001 and the buffer's end
    with the code phases of test_gpu_trk_array's exact test, at tap_chips 0 and -2.25.
(b) Bar.  The jammer-laden stream of test_gpu_stap._stream in both formats from an aligned pointer; acquisition: the twelve first- and
    last-bin candidates of test_gpu_array_probe._cands; tracking: twelve records of test_gpu_trk_array._records at tap_chips 0.5.
    Every word within REL = 1e-5 of its envelope: the bar and the envelope of the two neighbouring files.

No new tolerance: (a) is equality, (b) the project's bar against the existing models.

Measured on an MI355X (one run): every case of (a) equal; the largest fraction of (b) over the 43 pairs and both formats is 1.2e-8 for
gm_acq_array_prompts ((8, 3), c32; 5.5e-9 and up elsewhere) and 9.2e-9 for gm_trk_array_prompts ((3, 6), int8; 4.6e-9 and up elsewhere):
the streams carry a jammer 30 dB up, so the envelopes are large.  A case takes 0.02 to 0.2 s."""
import numpy as np
import pytest

import test_gpu_stap as TS           # (imports torch before the HIP library)
import test_gpu_local_search as TL
import test_gpu_array_probe as TA
import test_gpu_trk_array as TT
import array_prompt_classes as AC
import stap_model as SM
import trk_array_model as M

pytestmark = pytest.mark.gpu
REL = 1e-5
assert TA.REL == TT.REL == REL
_words, _stream, _fmt = TS._words, TS._stream, TS._fmt
IDS = ["A%d-L%d" % p for p in AC.PAIRS]


def _as_c64(xi):
    """the int8 IQ stream's integers as complex64 (exact)"""
    return (xi[..., 0].astype(np.float32) + 1j * xi[..., 1].astype(np.float32)).astype(np.complex64)


def _moved(hipbuf, xd, fmt):
    """the stream behind one element of 0x5A bytes, 64 bytes of 0x5A behind it -> the device pointer of its first sample"""
    raw = np.ascontiguousarray(xd).view(np.uint8).reshape(-1)
    elem = AC.ELEM[fmt]
    d = hipbuf.upload(np.concatenate([np.full(elem, 0x5A, np.uint8), raw, np.full(64, 0x5A, np.uint8)]))
    assert d % 256 == 0                                                        # so d + elem is no multiple of any V above the element
    return d + elem


def _forms(hipbuf, xi, A):
    """the four (format, pointer) forms of one integer stream -> [(tag, device pointer, fmt)]; the first is int8 from an aligned pointer"""
    xc = _as_c64(xi)
    assert (SM.as_c128(xc) == SM.as_c128(xi)).all()
    out = [("i8 " + AC.load_form("i8", A, True), hipbuf.upload(xi), "i8"), ("c32 " + AC.load_form("c32", A, True), hipbuf.upload(xc), "c32"),
           ("i8 moved " + AC.load_form("i8", A, False), _moved(hipbuf, xi, "i8"), "i8"),
           ("c32 moved " + AC.load_form("c32", A, False), _moved(hipbuf, xc, "c32"), "c32")]
    assert out[0][1] % 256 == 0 and out[1][1] % 256 == 0                       # (the start of an allocation, and aligned to every V)
    return out


# ---- gm_acq_array_prompts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,L", AC.PAIRS, ids=IDS)
def test_acq_class_on_both_load_forms(gpu, hipbuf, A, L):
    N = AC.EXACT_TERMS["acq"]
    s = TA._setup(N)
    eng = s["eng"]
    assert (N, s["R_u"], s["dwell"]) == (2048, 3, 3 * 2048) and (N + L - 1 + 1023) // 1024 == (3 if L > 1 else 2)
    assert TA.DOP[1] == 0.0 and (s["tab"][1] == np.complex64(1.0)).all()
    # (a) exact
    xi = _stream("i8", s["dwell"], A, 1000 + 10 * A + L)
    assert (xi == -128).any()
    x = SM.as_c128(xi)
    cands = [TL._cand(w, 1, cp, 0) for w in range(TA.P) for cp in (0, 1, 700, N - 1)]
    first = None
    for tag, d_x, fmt in _forms(hipbuf, xi, A):
        got = eng.array_prompts(cands, d_x, A, L, _fmt(fmt))
        assert got.shape == (len(cands), 3, L, A) and got.dtype == np.complex64
        if first is None:
            first = got
            for c, z in zip(cands, got):
                want, env = TA._model(s, x, c, A, L)
                assert env.max() < AC.EXACT_BOUND
                assert (want.real == np.rint(want.real)).all() and (want.imag == np.rint(want.imag)).all()
                assert (z.astype(np.complex128) == want).all(), (tag, c)
        else:
            assert (_words(got) == _words(first)).all(), tag
    assert not (_words(first[0]) == _words(first[1])).all()
    # (b) the bar
    cands = TA._cands(N, 0)[:12]
    assert {c["doppler_bin"] for c in cands} == {0, TA.D - 1}
    worst = {}
    for fmt in AC.FORMATS:
        xd = _stream(fmt, s["dwell"], A, 100 * A + L)
        z = eng.array_prompts(cands, hipbuf.upload(xd), A, L, _fmt(fmt))
        worst[fmt] = TA._fraction(s, SM.as_c128(xd), cands, z, A, L)
    print("acq A %d, L %d (class %d; %s, %s): largest |z - model| / envelope %.2e c32, %.2e i8 (bar %.0e)"
          % (A, L, AC.tap_class(A, L), AC.load_form("c32", A, True), AC.load_form("i8", A, True), worst["c32"], worst["i8"], REL))
    assert max(worst.values()) <= REL


# ---- gm_trk_array_prompts ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(oracle):
    return oracle.ca_code_table()


@pytest.fixture(scope="module")
def mgr(gpu):
    from gnss_sdr_rs_amd import tracking as T
    m = T.TrackingManager(1000.0 * AC.EXACT_TERMS["trk"], n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    yield m
    m.close()


@pytest.mark.parametrize("A,L", AC.PAIRS, ids=IDS)
def test_trk_class_on_both_load_forms(gpu, hipbuf, table, mgr, A, L):
    from gnss_sdr_rs_amd import tracking as T
    n = AC.EXACT_TERMS["trk"]
    fs = 1000.0 * n
    assert n == 4097 and M.slices(n) == 2 and T.array_plan(fs, A, L)["samples"] == n
    # (a) exact
    n_time = 2 * n + 100
    xi = _stream("i8", n_time, A, 2000 + 10 * A + L)
    assert (xi == -128).any()
    x = SM.as_c128(xi)
    at = [(0, 0.0), (1, 0.5), (3, 511.25), (max(L - 2, 0), 1022.75), (L - 1, 100.0), (L, 3.0), (1001, 77.7), (n_time - n, 0.0)]
    recs = [TT._record(T, 3 + k, s0, 0.0, code_phase=cp, carrier_phase=0.0) for k, (s0, cp) in enumerate(at)]
    rows = TT._rows(table, recs, M.FIXED)
    forms = _forms(hipbuf, xi, A)
    for tau in (0.0, -2.25):
        first = None
        for tag, d_x, fmt in forms:
            z, done = mgr.array_prompts(d_x, n_time, A, L, states=recs, tap_chips=tau, fmt=_fmt(fmt))
            assert z.shape == (len(recs), L, A) and done.all(), (tag, tau)
            if first is None:
                first = z
                for r, st in enumerate(recs):
                    want, env = M.prompts_state(x, st, fs, rows[r], L, tau, M.FIXED)
                    assert env.max() < AC.EXACT_BOUND
                    assert (want.real == np.rint(want.real)).all() and (want.imag == np.rint(want.imag)).all()
                    assert (z[r].astype(np.complex128) == want).all(), (tag, tau, r)
            else:
                assert (_words(z) == _words(first)).all(), (tag, tau)
        assert not (_words(first[0]) == _words(first[1])).all()
    # (b) the bar
    n_time = 2 * n + 777
    recs = TT._records(T, n, L, n_time, 12, n + A + L)
    rows = TT._rows(table, recs, M.FIXED)
    worst = {}
    for fmt in AC.FORMATS:
        xd = _stream(fmt, n_time, A, 100 * A + L)
        z, done = mgr.array_prompts(hipbuf.upload(xd), n_time, A, L, states=recs, tap_chips=0.5, fmt=_fmt(fmt))
        worst[fmt] = TT._worst(z, done, recs, SM.as_c128(xd), fs, rows, L, 0.5, M.FIXED)
    print("trk A %d, L %d (class %d; %s, %s): largest |z - model| / envelope %.2e c32, %.2e i8 (bar %.0e)"
          % (A, L, AC.tap_class(A, L), AC.load_form("c32", A, True), AC.load_form("i8", A, True), worst["c32"], worst["i8"], REL))
    assert max(worst.values()) <= REL
