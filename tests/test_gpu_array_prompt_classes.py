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
import trk_form_classes as FC

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


# ---- gm_trk_array_prompts: the general arithmetic forms (trk_form_classes.py) ----------------------------------------------------------------
# ta_ref_image<FASTC = false>, and the general division behind FASTC = true, on every launch class; the bar is (b)'s, against the same model.
@pytest.fixture(scope="module")
def form_mgrs(gpu):
    """the handles of trk_form_classes.HANDLES (FIXED mode, C/A), made when first asked for"""
    from gnss_sdr_rs_amd import tracking as T
    made = {}

    def get(name):
        if name not in made:
            made[name] = T.TrackingManager(n_channels=1, code_index_mode=T.CODE_INDEX_FIXED, **FC.HANDLES[name])
        return made[name]
    yield get
    for m in made.values():
        m.close()


def _pointer_forms(hipbuf, n_time, A, seed):
    """the jammer-laden stream in both formats, each from an aligned pointer and from one element behind it -> [(fmt, aligned, pointer, x)]"""
    out = []
    for fmt in AC.FORMATS:
        xd = _stream(fmt, n_time, A, seed)
        x = SM.as_c128(xd)
        out += [(fmt, True, hipbuf.upload(xd), x), (fmt, False, _moved(hipbuf, xd, fmt), x)]
    return out


def _form_record(T, t, prn, s):
    return TT._record(T, prn, s, **FC.state_of(t))


TAU_FORMS = -2.25                     # with code_phase = -0.75 the tap's phase is negative on the first samples and wraps to the row's end


@pytest.mark.parametrize("A,L", AC.PAIRS, ids=IDS)
def test_trk_general_forms_on_every_launch_class(gpu, hipbuf, table, form_mgrs, A, L):
    """Every (format, A, L, pointer form) x the four classes of trk_form_classes.SWEEP, one record a class in one call, n = 2048: eligible,
    code_phase = -0.75, carrier_phase = 1.2e5 and both.  (The aligned forms' code-general / carrier-fast class is reached by (b) above
    through test_gpu_trk_array._records' code_phase = -3.25: the census keeps that case and none is added there.)  Then the eligible
    record on the handle whose early-late spacing is 1.5 — ta_ref_image<false>, the tap does not depend on the spacing: the SAME WORDS."""
    from gnss_sdr_rs_amd import tracking as T
    fs = FC.HANDLES["base"]["fs"]
    n = FC.samples_per_code(fs)
    n_time = n + 64
    base, el15 = form_mgrs("base"), form_mgrs("el15")
    worst = {i: 0.0 for i in FC.SWEEP}
    for fmt, aligned, d_x, x in _pointer_forms(hipbuf, n_time, A, 300 * A + L):
        ids = [i for i in FC.SWEEP if not (aligned and i == "code-phase-negative")]
        recs = [_form_record(T, FC.BY_ID[i], 3 + k, L - 1 + 7 * k) for k, i in enumerate(ids)]
        rows = TT._rows(table, recs, M.FIXED)
        z, done = base.array_prompts(d_x, n_time, A, L, states=recs, tap_chips=TAU_FORMS, fmt=_fmt(fmt))
        for k, i in enumerate(ids):
            worst[i] = max(worst[i], TT._worst(z[k:k + 1], done[k:k + 1], recs[k:k + 1], x, fs, rows[k:k + 1], L, TAU_FORMS, M.FIXED))
        z2, d2 = el15.array_prompts(d_x, n_time, A, L, states=recs[:1], tap_chips=TAU_FORMS, fmt=_fmt(fmt))
        assert d2[0] == 1 and (_words(z2[0]) == _words(z[0])).all(), (fmt, aligned)
    print("trk forms A %d, L %d (class %d): largest |z - model| / envelope %s (bar %.0e)"
          % (A, L, AC.tap_class(A, L), ", ".join("%s %.2e" % (i, worst[i]) for i in FC.SWEEP), REL))
    assert max(worst.values()) <= REL


@pytest.mark.parametrize("A,L", FC.ARRAY_SMALLEST, ids=["A%d-L%d" % p for p in FC.ARRAY_SMALLEST])
def test_trk_every_trigger_on_the_smallest_pair_of_a_tap_class(gpu, hipbuf, table, form_mgrs, A, L):
    """The triggers the sweep above leaves: code_phase = len + 0.5, the spacings of 1.5 (three and five arms), 20 MHz at 50 Msps (n = 50 000),
    fs = 2^24 - 1 (n = 16 777) and |2 pi f| = 6.3e-13 — on the smallest (A, L) of each tap class, both formats, both pointer forms."""
    from gnss_sdr_rs_amd import tracking as T
    assert sorted({AC.tap_class(a, l) for a, l in FC.ARRAY_SMALLEST}) == sorted({AC.tap_class(a, l) for a, l in AC.PAIRS})
    left = [t for t in FC.triggers("array") if t["id"] not in FC.SWEEP[1:]]
    worst = {t["id"]: 0.0 for t in left}
    for fs in sorted({FC.HANDLES[t["handle"]]["fs"] for t in left}):
        trig = [t for t in left if FC.HANDLES[t["handle"]]["fs"] == fs]
        n = FC.samples_per_code(fs)
        n_time = n + 64
        for fmt, aligned, d_x, x in _pointer_forms(hipbuf, n_time, A, 500 * A + L + int(fs) % 97):
            words = {}
            for k, t in enumerate(trig):
                rec = _form_record(T, t, 3 + k, L + 2)
                z, done = form_mgrs(t["handle"]).array_prompts(d_x, n_time, A, L, states=[rec], tap_chips=TAU_FORMS, fmt=_fmt(fmt))
                worst[t["id"]] = max(worst[t["id"]], TT._worst(z, done, [rec], x, fs, TT._rows(table, [rec], M.FIXED), L, TAU_FORMS, M.FIXED))
                words[t["id"]] = (rec.prn, _words(z[0]))
            if "eligible" in words:            # the same state on the spacing-1.5 handles (another prn, so another row: made equal first)
                for tid in ("early-late-1.5", "very-early-late-1.5-five-arms"):
                    rec = _form_record(T, FC.BY_ID[tid], words["eligible"][0], L + 2)
                    z, _ = form_mgrs(FC.BY_ID[tid]["handle"]).array_prompts(d_x, n_time, A, L, states=[rec], tap_chips=TAU_FORMS, fmt=_fmt(fmt))
                    assert (_words(z[0]) == words["eligible"][1]).all(), (tid, fmt, aligned)
    print("trk triggers A %d, L %d (class %d): largest |z - model| / envelope %s (bar %.0e)"
          % (A, L, AC.tap_class(A, L), ", ".join("%s %.2e" % kv for kv in worst.items()), REL))
    assert max(worst.values()) <= REL
