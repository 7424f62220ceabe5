"""Per-antenna prompts at tracked states (gm_trk_array_prompts, csrc/trk_array.hip) on the GPU against trk_array_model.py.

fs = 1000 n with a C/A handle (1.023e6 / 1023 = 1000 periods a second, exactly), so n is small.

1. Parity.  Every word of z against the model within REL = 1e-5 (the project's bar) of its envelope sum_i |x_a[s + i - l]| (|ref| = 1).
   Shapes: n = 2048 (below one slice of 4096 time samples), 4096 (exactly one), 9000 (three, not a multiple of 256), each at (A, L) =
   (4, 2); n = 4097 (a second slice of ONE time sample; the taps of the last samples of slice 0 reach ref words behind the slice edge)
   at (2, 1), (3, 2), (4, 2), (4, 8), (8, 4), (8, 1).  c32 and int8 IQ with -128 in the stream; the streams carry a jammer 30 dB up
   (test_gpu_stap._stream).  Calls of 40, 5 and 1 records at tap_chips 0, +0.5 and -2.25; records at s = 0, 1, L - 1 (the zero halo), at
   odd s (the wide loads' alignment), at the buffer's end, with a negative code phase (the general fmod and division).  Both code-index
   modes, a strict_libm handle and a boc11 custom-code handle at n = 4097.
2. Exact integers: carrier_freq = 0, carrier_phase = 0, int8: ref = +-1 and every sum is a sum of integers below 2^24, so the device's
   words EQUAL the model's — at s = 0 and 0 < s < L - 1, l > 0 (the zero halo) and everywhere else, across two slices.  The input sits
   at the start of an allocation: nothing in front of it may be read.
3. Bit for bit: a record alone against the same record among 40 (inside test 1); a second call; an input pointer one element off against
   the aligned copy; the same records on a buffer that begins exactly at s_min - (L-1) with that first_index against the whole stream.
4. Cross-check at L = 1: antenna a's words against gm_trk_bank (T = 1 at tap_chips, F = 1) on a ring holding the de-interleaved
   antenna, within 2 REL of the envelope (the bank rounds x * w first and sums in another order).
5. Skips and refusals: every kind of skipped record gives zeros and done 0 beside records that run; every refusal leaves z and done full
   of sentinels; the states before and after are byte for byte equal; a twin handle that tracks ten more epochs gives the same words as
   one on which the entry was never called.
6. The chain on the device, T1 of seed 1: (a) records made up from the two cells found behind the e_0 beam, rows from their tracker-form
   prompts, the beams behind those rows against the beams behind AcquisitionEngine.array_prompts' rows (at least 0.9 of them: the host
   test's bar and reason); (b) plane 0 through a ring and nine tracked epochs, the prompts at the states saved before each epoch against
   the model at those states (parity only: no quality bar rests on the loop's pull-in).

Measured on an MI355X (one run): the largest fraction of test 1 is 9.3e-9 (n = 2048, (4, 2), c32; 3.9e-9 to 8.0e-9 on the other shapes,
4.6e-9 to 6.3e-9 on the other handles: the test streams carry a jammer 30 dB up, so the envelopes are large), of test 4 8.6e-9; the chain
gives 93.92 and 54.04 behind the rows of (a) against 93.78 and 54.46 behind AcquisitionEngine.array_prompts' rows (1.002 and 0.992 of
them), 93.90 and 54.00 behind the rows of (b), whose prompts are within 6.2e-9 of the model."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_stap as TS           # (imports torch before the HIP library)
import test_gpu_local_search as TL
import array_probe_model as PM
import beam_model as BM
import excise_model as EM
import stap_model as SM
import trk_array_model as M
import trk_bank_model as TB

pytestmark = pytest.mark.gpu
REL = 1e-5
QUALITY_BAR = 0.9                     # test_trk_array_host.QUALITY_BAR: the margin test_array_probe_host.BARS gives an estimated row
INVALID, RANGE = -1, -5
_words, _stream, _fmt = TS._words, TS._stream, TS._fmt


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.ca_code_table()


def _record(T, prn, nxt, carrier_freq, code_phase=0.0, code_rate=1.023e6, carrier_phase=0.3, active=1):
    s = T.TrkState()
    s.prn, s.active, s.next_sample_index = prn, active, nxt
    s.carrier_freq, s.carrier_phase, s.code_phase, s.code_rate = carrier_freq, carrier_phase, code_phase, code_rate
    return s


def _records(T, n, L, n_time, count, seed, n_prn=31):
    """`count` records that run: s = 0, 1, L - 1 (the zero halo), 3, the buffer's end, one before it, then a seeded spread; the fifth has
    a negative code phase (the general fmod and division instead of the exact fast forms)"""
    rng = np.random.default_rng(seed)
    starts = [0, 1, max(L - 1, 2), 3, n_time - n, n_time - n - 1] + [int(v) for v in rng.integers(0, n_time - n + 1, count)]
    recs = []
    for k, s in enumerate(starts[:count]):
        recs.append(_record(T, int(rng.integers(1, n_prn + 1)), s, float(rng.uniform(-5000.0, 5000.0)),
                            code_phase=-3.25 if k == 4 else float(rng.uniform(0.0, 1023.0)), carrier_phase=float(rng.uniform(-3.0, 3.0))))
    return recs


def _rows(table, recs, mode):
    return [table[st.prn if mode == M.FAITHFUL else st.prn - 1] for st in recs]


def _worst(z, done, recs, x, fs, rows, L, tau, mode, boc=False, first_index=0):
    """the largest |device - model| / envelope over the records' words; every record ran"""
    worst = 0.0
    for r, st in enumerate(recs):
        assert done[r] == 1, r
        want, env = M.prompts_state(x, st, fs, rows[r], L, tau, mode, boc, first_index)
        assert z[r].shape == want.shape
        worst = max(worst, float(np.max(np.abs(z[r].astype(np.complex128) - want) / env)))
    return worst


# ---- 1. parity, and a record alone against the same record among 40 -------------------------------------------------------------------
SHAPES = [(2048, 4, 2), (4096, 4, 2), (9000, 4, 2), (4097, 2, 1), (4097, 3, 2), (4097, 4, 2), (4097, 4, 8), (4097, 8, 4), (4097, 8, 1)]


@pytest.mark.parametrize("fmt", ["c32", "i8"])
@pytest.mark.parametrize("n,A,L", SHAPES, ids=["n%d-A%d-L%d" % s for s in SHAPES])
def test_every_word_against_the_model(gpu, hipbuf, table, n, A, L, fmt):
    from gnss_sdr_rs_amd import tracking as T
    fs = 1000.0 * n
    assert TB.samples_per_code(fs, 1.023e6, 1023) == n and M.slices(n) == (n + 4095) // 4096
    n_time = 2 * n + 777
    xd = _stream(fmt, n_time, A, 100 * A + L)
    if fmt == "i8":
        assert (xd == -128).any()
    x = SM.as_c128(xd)
    d_x = hipbuf.upload(xd)
    mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED)
    recs = _records(T, n, L, n_time, 40, n + A + L)
    rows = _rows(table, recs, M.FIXED)
    z40, d40 = mgr.array_prompts(d_x, n_time, A, L, states=recs, fmt=_fmt(fmt))
    assert z40.shape == (40, L, A) and z40.dtype == np.complex64 and d40.dtype == np.uint8
    worst = [_worst(z40, d40, recs, x, fs, rows, L, 0.0, M.FIXED)]
    z5, d5 = mgr.array_prompts(d_x, n_time, A, L, states=recs[:5], tap_chips=0.5, fmt=_fmt(fmt))
    worst.append(_worst(z5, d5, recs[:5], x, fs, rows[:5], L, 0.5, M.FIXED))
    z1, d1 = mgr.array_prompts(d_x, n_time, A, L, states=[recs[17]], tap_chips=-2.25, fmt=_fmt(fmt))
    worst.append(_worst(z1, d1, [recs[17]], x, fs, [rows[17]], L, -2.25, M.FIXED))
    print("n %d, A %d, L %d, %s: largest |z - model| / envelope %.2e / %.2e / %.2e at 40 / 5 / 1 records (bar %.0e)"
          % (n, A, L, fmt, worst[0], worst[1], worst[2], REL))
    assert max(worst) <= REL
    # alone and among 39 others: the same words
    for r in (0, 4, 17, 39):
        alone, da = mgr.array_prompts(d_x, n_time, A, L, states=[recs[r]], fmt=_fmt(fmt))
        assert da[0] == 1 and (_words(alone[0]) == _words(z40[r])).all(), r
    assert not (_words(z40[0]) == _words(z40[5])).all()
    mgr.close()


HANDLES = [dict(code_index_mode=0), dict(code_index_mode=1, strict_libm=True), dict(code_index_mode=1, boc11=True, custom=True)]


@pytest.mark.parametrize("kw", HANDLES, ids=["faithful", "strict_libm", "boc11-custom"])
def test_modes_and_handles(gpu, hipbuf, table, kw):
    from gnss_sdr_rs_amd import tracking as T
    n, A, L, fmt = 4097, 4, 2, "i8"
    fs, n_time = 1000.0 * n, 2 * n + 777
    kw = dict(kw)
    custom = kw.pop("custom", False)
    codes = np.where(np.random.default_rng(56).integers(0, 2, (3, 1023)) > 0, 1, -1).astype(np.int8) if custom else None
    mode, boc = kw["code_index_mode"], bool(kw.get("boc11"))
    mgr = T.TrackingManager(fs, n_channels=1, codes=codes, nominal_code_rate=1.023e6 if custom else 0.0, **kw)
    xd = _stream(fmt, n_time, A, 61)
    x = SM.as_c128(xd)
    d_x = hipbuf.upload(xd)
    recs = _records(T, n, L, n_time, 12, 9, n_prn=3 if custom else 31)
    recs[1].code_phase = 0.125                       # a tap below -1 then asks for a negative phase: FAITHFUL saturates to chip 0
    rows = [codes[st.prn - 1] for st in recs] if custom else _rows(table, recs, mode)
    for tau in (0.0, 0.5, -2.25):
        z, done = mgr.array_prompts(d_x, n_time, A, L, states=recs, tap_chips=tau, fmt=_fmt(fmt))
        worst = _worst(z, done, recs, x, fs, rows, L, tau, mode, boc)
        print("%s, tap %g: largest |z - model| / envelope %.2e (bar %.0e)" % (sorted(kw.items()), tau, worst, REL))
        assert worst <= REL
    if boc:                                          # the sub-carrier matters: the same records without it are somewhere else entirely
        z, _ = mgr.array_prompts(d_x, n_time, A, L, states=recs[:1], tap_chips=0.5, fmt=_fmt(fmt))
        plain, env = M.prompts_state(x, recs[0], fs, rows[0], L, 0.5, mode, False)
        assert np.max(np.abs(z[0] - plain) / env) > 100 * REL
    mgr.close()


# ---- 2. exact integers ------------------------------------------------------------------------------------------------------------------
def test_integer_sums_are_exact_and_the_halo_is_zero(gpu, hipbuf, table):
    from gnss_sdr_rs_amd import tracking as T
    n, A, L = 4097, 4, 8
    fs, n_time = 1000.0 * n, 2 * n + 100
    xd = _stream("i8", n_time, A, 7)
    x = SM.as_c128(xd)
    d_x = hipbuf.upload(xd)                                              # the start of an allocation
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    recs = [_record(T, 3 + k, s, 0.0, code_phase=cp, carrier_phase=0.0)
            for k, (s, cp) in enumerate([(0, 0.0), (1, 0.5), (3, 511.25), (6, 1022.75), (7, 100.0), (8, 3.0), (1001, 77.7), (n_time - n, 0.0)])]
    rows = _rows(table, recs, M.FIXED)
    for tau in (0.0, -2.25):
        z, done = mgr.array_prompts(d_x, n_time, A, L, states=recs, tap_chips=tau, fmt=_fmt("i8"))
        for r, st in enumerate(recs):
            want, env = M.prompts_state(x, st, fs, rows[r], L, tau, M.FIXED)
            assert done[r] == 1 and env.max() < 2.0 ** 24 / 1.5           # |re| + |im| sums stay below 2^24: every partial sum is exact
            assert (want.real == np.rint(want.real)).all() and (want.imag == np.rint(want.imag)).all()
            assert (z[r].astype(np.complex128) == want).all(), (tau, r)
    mgr.close()


# ---- 3. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,L,fmt", [(4, 2, "c32"), (8, 4, "i8"), (3, 3, "i8"), (2, 8, "c32")])
def test_repetition_an_unaligned_pointer_and_a_buffer_that_starts_late(gpu, hipbuf, table, A, L, fmt):
    from gnss_sdr_rs_amd import tracking as T
    n = 4097
    fs, n_time = 1000.0 * n, 2 * n + 777
    xd = _stream(fmt, n_time, A, 31 * A + L)
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    recs = _records(T, n, L, n_time, 12, 5)
    d_x = hipbuf.upload(xd)
    first, d0 = mgr.array_prompts(d_x, n_time, A, L, states=recs, fmt=_fmt(fmt))
    again, d1 = mgr.array_prompts(d_x, n_time, A, L, states=recs, fmt=_fmt(fmt))
    assert d0.all() and d1.all() and (_words(first) == _words(again)).all()
    # one element (8 or 2 bytes) in front: the records' starts leave the wide loads' alignment
    flat = np.ascontiguousarray(xd).reshape(-1) if fmt == "c32" else np.ascontiguousarray(xd).reshape(-1, 2)
    elem = 8 if fmt == "c32" else 2
    d_p = hipbuf.upload(np.concatenate([flat[:1], flat]))
    moved, d2 = mgr.array_prompts(d_p + elem, n_time, A, L, states=recs, fmt=_fmt(fmt))
    assert d2.all() and (_words(first) == _words(moved)).all()
    # a buffer that begins exactly at s_min - (L-1), with that first_index: the same words; one time sample later the first record skips
    late = [st for st in recs if st.next_sample_index >= 500]
    idx = [r for r, st in enumerate(recs) if st.next_sample_index >= 500]
    assert len(late) >= 5
    f0 = min(st.next_sample_index for st in late) - (L - 1)
    d_late = hipbuf.upload(np.ascontiguousarray(xd[f0:]))
    got, d3 = mgr.array_prompts(d_late, n_time - f0, A, L, states=late, first_index=f0, fmt=_fmt(fmt))
    assert d3.all() and (_words(got) == _words(first[idx])).all()
    got, d4 = mgr.array_prompts(d_x + f0 * A * elem, n_time - f0, A, L, states=late, first_index=f0, fmt=_fmt(fmt))      # inside the allocation
    assert d4.all() and (_words(got) == _words(first[idx])).all()
    mgr.close()


# ---- 4. the cross-check against gm_trk_bank ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c32", "i8"])
def test_tap_zero_is_the_banks_word_per_antenna(gpu, hipbuf, table, fmt):
    from gnss_sdr_rs_amd import tracking as T
    n, A = 4097, 3
    fs, n_time = 1000.0 * n, 2 * n + 777
    xd = _stream(fmt, n_time, A, 5)
    x = SM.as_c128(xd)
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    recs = _records(T, n, 1, n_time, 12, 3)
    rows = _rows(table, recs, M.FIXED)
    d_x = hipbuf.upload(xd)
    worst = 0.0
    for tau in (0.0, -2.25):
        z, done = mgr.array_prompts(d_x, n_time, A, 1, states=recs, tap_chips=tau, fmt=_fmt(fmt))
        assert done.all()
        for a in range(A):
            ring = T.MulticastRingBuffer(1 << 14)
            ring.write_samples(x[:, a].astype(np.complex64))             # (int8 values are exact in complex64)
            ref, ok = mgr.bank(ring, [tau], states=recs)
            assert ok.all()
            for r, st in enumerate(recs):
                env = M.prompts_state(x, st, fs, rows[r], 1, tau, M.FIXED)[1][0, a]
                worst = max(worst, abs(complex(z[r, 0, a]) - complex(ref[r, 0, 0])) / env)
            ring.close()
    print("%s: largest |z - gm_trk_bank's word| / envelope %.2e (bar %.0e)" % (fmt, worst, 2 * REL))
    assert worst <= 2 * REL
    mgr.close()


# ---- 5. skips and refusals --------------------------------------------------------------------------------------------------------------
def test_skipped_records_give_zeros_beside_records_that_run(gpu, hipbuf, table):
    from gnss_sdr_rs_amd import tracking as T
    n, A, L = 2048, 4, 4
    fs, n_time, f0 = 1000.0 * n, 3 * n, 1000
    xd = _stream("c32", n_time, A, 12)
    x = SM.as_c128(xd)
    d_x = hipbuf.upload(xd)
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    good = [_record(T, 3, f0 + L - 1, 1500.0), _record(T, 9, f0 + n_time - n, -700.0, code_phase=3.5), _record(T, 17, f0 + 2500, 40.0)]
    group = [_record(T, 3, f0 + 2000, 0.0, active=0), good[0],
             _record(T, 33, f0 + 2000, 0.0),                      # row 32 is outside the table
             _record(T, 0, f0 + 2000, 0.0),                       # FIXED: row prn - 1 = -1
             _record(T, 3, f0 + n_time - n + 1, 0.0), good[1],    # s + n is past the buffer
             _record(T, 3, f0 + L - 2, 0.0),                      # part of the halo lies in front of first_index > 0
             _record(T, 3, f0 - 1, 0.0), _record(T, 3, 5, 0.0),   # the record starts in front of the buffer
             _record(T, 3, f0 + 2000, 0.0, code_rate=0.0),        # n = round(fs / 0) is no count
             _record(T, 3, f0 + 2000, 0.0, code_rate=0.5),        # n = 4.2e9 >= 2^31
             _record(T, 3, (1 << 63) + 5, 0.0), good[2]]
    z, done = mgr.array_prompts(d_x, n_time, A, L, states=group, first_index=f0)
    assert list(done) == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    assert not z[done == 0].view(np.uint32).any()
    rows = _rows(table, good, M.FIXED)
    worst = _worst(z[done == 1], done[done == 1], good, x, fs, rows, L, 0.0, M.FIXED, first_index=f0)
    print("records that run beside skipped ones: largest fraction of the envelope %.2e" % worst)
    assert worst <= REL
    alone, d1 = mgr.array_prompts(d_x, n_time, A, L, states=[good[0]], first_index=f0)
    assert d1[0] == 1 and (_words(alone[0]) == _words(z[1])).all()
    for st, want in zip(group, done):                             # the model's rule, record by record
        row = st.prn - 1
        assert M.runs(st.active, row, 32, TB.samples_per_code(fs, st.code_rate, 1023), st.next_sample_index, L, f0, n_time) == bool(want)
    # nothing runs at all: still a success
    z, done = mgr.array_prompts(d_x, n_time, A, L, states=[group[0], group[4]], first_index=f0)
    assert not done.any() and not z.view(np.uint32).any()
    # n_time = 0: every record is skipped
    z, done = mgr.array_prompts(d_x, 0, A, L, states=good, first_index=f0)
    assert not done.any() and not z.view(np.uint32).any()
    mgr.close()


SENTINEL = np.float32(-12345.5)


def _raw(Lib, T, mgr, d_x, recs, n_states, A=4, L=2, tau=0.0, fmt=0, first_index=0, n_time=6144, reserved=None, null=None):
    """gm_trk_array_prompts itself on sentinel-filled outputs -> (status, outputs untouched)"""
    from gnss_sdr_rs_amd import _lib
    cfg = _lib.TrkArrayCfg()
    cfg.n_antennas, cfg.taps, cfg.tap_chips = A, L, tau
    if reserved is not None:
        cfg.reserved[reserved] = 1
    z = np.full(2 * 1030 * 32, SENTINEL, np.float32)
    done = np.full(1030, 0x5a, np.uint8)
    arr = None if recs is None else (T.TrkState * len(recs))(*recs)
    rc = Lib.gm_trk_array_prompts(None if null == "handle" else mgr._h, None if null == "samples" else C.c_void_p(d_x), fmt, first_index, n_time,
                                  None if arr is None else C.cast(arr, C.c_void_p), n_states, None if null == "cfg" else C.byref(cfg),
                                  None if null == "z" else z.ctypes.data_as(C.c_void_p), done.ctypes.data_as(C.c_void_p))
    return rc, bool(np.all(z == SENTINEL) and np.all(done == 0x5a))


def test_every_refusal_leaves_the_outputs(gpu, hipbuf, table):
    from gnss_sdr_rs_amd import _lib, tracking as T
    Lib = _lib.lib()
    n, A = 2048, 4
    fs, n_time = 1000.0 * n, 3 * n
    d_x = hipbuf.upload(_stream("c32", n_time, 8, 3))                    # (8 antennas' worth: the passing calls below read A = 8 too)
    mgr = T.TrackingManager(fs, n_channels=5, code_index_mode=T.CODE_INDEX_FIXED)
    one = [_record(T, 3, 100, 250.0)]
    cases = [(dict(null="handle"), INVALID), (dict(null="samples"), INVALID), (dict(null="cfg"), INVALID), (dict(null="z"), INVALID),
             (dict(fmt=_lib.FMT_I8_REAL), INVALID), (dict(fmt=3), INVALID), (dict(fmt=-1), INVALID),
             (dict(A=1), RANGE), (dict(A=9), RANGE), (dict(A=0), RANGE), (dict(L=0), RANGE), (dict(L=9), RANGE),
             (dict(A=5, L=7), RANGE), (dict(A=8, L=5), RANGE),
             (dict(tau=float("nan")), INVALID), (dict(tau=float("inf")), INVALID), (dict(tau=64.5), RANGE), (dict(tau=-512.0), RANGE),
             (dict(first_index=1 << 62), RANGE), (dict(first_index=(1 << 62) - n_time), RANGE), (dict(n_time=1 << 62), RANGE),
             (dict(first_index=(1 << 64) - 1, n_time=2), RANGE)] + [(dict(reserved=k), INVALID) for k in range(5)]
    for kw, status in cases:
        rc, untouched = _raw(Lib, T, mgr, d_x, one, 1, **kw)
        assert rc == status and untouched, (kw, rc, untouched)
    for n_states, status in ((0, RANGE), (1025, RANGE)):
        rc, untouched = _raw(Lib, T, mgr, d_x, one * 1030, n_states)
        assert rc == status and untouched, n_states
    rc, untouched = _raw(Lib, T, mgr, d_x, None, 4)                       # states NULL: n_states must be n_channels (5)
    assert rc == INVALID and untouched
    # the limits themselves pass
    for kw in (dict(A=8, L=4, tau=64.0), dict(A=4, L=8, tau=-64.0), dict(A=2, L=1)):
        rc, untouched = _raw(Lib, T, mgr, d_x, one * 1024, 1024, **kw)
        assert rc == 0 and not untouched, kw
    rc, untouched = _raw(Lib, T, mgr, d_x, None, 5)                       # the handle's own channels: none is active, all skipped
    assert rc == 0 and not untouched
    # |tau| < code_len / 2 on a 100-chip code
    short = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED, codes=np.ones((1, 100), np.int8))
    assert _raw(Lib, T, short, d_x, one, 1, tau=50.0) == (RANGE, True)
    assert _raw(Lib, T, short, d_x, one, 1, tau=-49.5)[0] == 0
    short.close()
    mgr.close()


def test_nothing_moves(gpu, hipbuf, table):
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n = 2.048e6, 2048
    prns = [3, 9, 17]
    sc = synth.tracking_scene(table, fs, 0.0, prns, 14, config_id=74, cn0=50.0)
    x = synth.to_c32(sc["x"])
    ring = T.MulticastRingBuffer(1 << 15)
    ring.write_samples(x)
    xa = np.ascontiguousarray(np.stack([x, (0.5j * x).astype(np.complex64)], axis=1))      # a two-antenna stream that holds the satellites
    d_x = hipbuf.upload(xa)
    mgrs = [T.TrackingManager(fs, n_channels=4, code_index_mode=T.CODE_INDEX_FIXED) for _ in range(2)]
    for m in mgrs:
        for i, s in enumerate(sc["sats"]):
            m.channels[i].start(dict(prn=s["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s["doppler_hz"] + 10.0,
                                     fs=fs, mag_relative=10.0, sample_global_index=s["code_start"], doppler_bin=0))
        m.update_all(ring, 2)
    a, twin = mgrs
    before = a.get_states()
    own, done = a.array_prompts(d_x, x.size, 2, 3)                          # states = None: the handle's channels as they stand
    assert list(done) == [1, 1, 1, 0]                                        # the fourth channel was never started
    after = a.get_states()
    assert b"".join(bytes(s) for s in before) == b"".join(bytes(s) for s in after)
    given, done2 = a.array_prompts(d_x, x.size, 2, 3, states=before)
    assert (_words(own) == _words(given)).all() and (done == done2).all()
    rows = [table[s["prn"] - 1] for s in sc["sats"]]
    worst = _worst(own[:3], done[:3], before[:3], xa.astype(np.complex128), fs, rows, 3, 0.0, M.FIXED)
    assert worst <= REL
    assert np.abs(own[:3, 0, 0]).min() > 100.0                               # a signal is under the correlator
    got = a.update_all(ring, 10)
    want = twin.update_all(ring, 10)                                         # the twin made no array_prompts call
    for g, e in zip(got[:3], want[:3]):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(e).view(np.uint8))
    assert got[3] == want[3] == 10
    assert b"".join(bytes(s) for s in a.get_states()) == b"".join(bytes(s) for s in twin.get_states())
    for m in mgrs:
        m.close()
    ring.close()


# ---- 6. the chain -------------------------------------------------------------------------------------------------------------------------
def test_the_rows_come_from_tracked_states(gpu, hipbuf):
    """T1 of seed 1 on the device, the steps of the docstring.  (a) holds the beams behind the tracker-form rows to QUALITY_BAR of the
    beams behind AcquisitionEngine.array_prompts' rows in the same test; (b) is parity at the tracked states."""
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, beamformer, tracking as T
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    assert eng.dwell_samples == BM.DWELL
    x = BM.scene("T1", 1).astype(np.complex64)
    xm = x.astype(np.complex128)
    A, L, Mw, N = x.shape[1], 2, 8, BM.N
    assert (A, BM.TAPS["T1"], x.shape[0]) == (4, L, BM.DWELL)
    nb = BM.DWELL // 1024
    e0 = BM.rows(A, L)[:1]
    d_x = hipbuf.upload(x)
    # the e_0 beam with capture, its plane into the search: the two results
    bf = beamformer.Beamformer(A, L, e0, 1024, 1e-4)
    d_y, d_R, d_w = hipbuf.alloc(BM.DWELL * 8), hipbuf.alloc(nb * Mw * Mw * 8), hipbuf.alloc(nb * Mw * 8)
    bf.capture(d_R, d_w, nb)
    assert bf.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y, BM.DWELL) == BM.DWELL
    bf.synchronize()
    R = hipbuf.download(d_R, nb * Mw * Mw * 8, np.complex64).reshape(nb, Mw, Mw)
    plane0 = hipbuf.download(d_y, BM.DWELL * 8, np.complex64)
    eng.search_dev(d_y, _lib.FMT_C32)
    first = [EM.best_cell(*eng.metrics(), w) for w in (0, 1)]
    assert all(BM.found(first[w], w) and first[w][2] > BM.DETECT for w in (0, 1)), first
    bf.close()
    # a result as the tracker takes it: the dwell starts at absolute sample 0, so the found code phase is the sample_global_index
    results = [dict(prn=w + 1, code_phase_samples=int(first[w][1]), code_phase_chips=0.0, carrier_freq=float(EM.DOP[first[w][0]]), fs=EM.FS,
                    mag_relative=float(first[w][2]), sample_global_index=int(first[w][1]), doppler_bin=int(first[w][0])) for w in (0, 1)]
    codes = EM.scene_codes()
    mgr = T.TrackingManager(EM.FS, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED, codes=codes, nominal_code_rate=1.023e6)

    def beam_figures(rows):
        """each satellite's cell behind its row: a new Beamformer with the two rows, each plane into search_dev"""
        b = beamformer.Beamformer(A, L, np.ascontiguousarray(rows.reshape(2, Mw)), 1024, 1e-4)
        d_y2 = hipbuf.alloc(2 * BM.DWELL * 8)
        assert b.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y2, BM.DWELL) == BM.DWELL
        b.synchronize()
        out = []
        for w in (0, 1):
            eng.search_dev(d_y2 + w * BM.DWELL * 8, _lib.FMT_C32)
            out.append(EM.best_cell(*eng.metrics(), w))
        b.close()
        return out

    # the yardstick: the rows AcquisitionEngine.array_prompts gives at the two found cells
    z_acq = eng.array_prompts([TL._cand(w, first[w][0], first[w][1], 0) for w in (0, 1)], d_x, A, L, _lib.FMT_C32)
    rows_acq, _ = AQ.solve_rows(z_acq, R, 1e-4)
    acq = beam_figures(rows_acq)
    # (a) records made up from the two results
    recs = [_record(T, r["prn"], r["sample_global_index"] + p * N, r["carrier_freq"], carrier_phase=0.0) for r in results for p in range(9)]
    z, done = mgr.array_prompts(d_x, BM.DWELL, A, L, states=recs)
    assert done.all() and z.shape == (18, L, A)
    worst = _worst(z, done, recs, xm, EM.FS, [codes[st.prn - 1] for st in recs], L, 0.0, M.FIXED)
    rows_a, infos = AQ.solve_rows(z.reshape(2, 9, L, A), R, 1e-4)
    assert all(i["lambda1"] >= 2.0 * i["lambda2"] for i in infos), infos
    got_a = beam_figures(rows_a)
    for w in (0, 1):
        print("T1 seed 1 (a), satellite %d: behind the tracker-form row %s, behind the acquisition-form row %s (%.3f of it, bar %.1f), "
              "lambda1 / lambda2 %.1f" % (w, got_a[w], acq[w], got_a[w][2] / acq[w][2], QUALITY_BAR, infos[w]["lambda1"] / infos[w]["lambda2"]))
        assert BM.found(got_a[w], w) and got_a[w][2] > BM.DETECT
        assert got_a[w][2] >= QUALITY_BAR * acq[w][2]
    print("(a) largest |z - model| / envelope %.2e" % worst)
    assert worst <= REL
    # (b) plane 0 into a ring, nine tracked epochs, the prompts at the states saved before each
    ring = T.MulticastRingBuffer(1 << 15)
    ring.write_samples(plane0)
    for w in (0, 1):
        mgr.channels[w].start(results[w])
    saved = []
    for _ in range(9):
        saved.append(mgr.get_states())
        _, proc, lost, ep = mgr.update_all(ring, 1)
        assert ep == 1 and proc.all() and not lost.any()
    recs_b = [saved[p][w] for w in (0, 1) for p in range(9)]
    zb, done_b = mgr.array_prompts(d_x, BM.DWELL, A, L, states=recs_b)
    assert done_b.all()
    worst_b = _worst(zb, done_b, recs_b, xm, EM.FS, [codes[st.prn - 1] for st in recs_b], L, 0.0, M.FIXED)
    print("(b) largest |z - model| / envelope at the tracked states %.2e (bar %.0e)" % (worst_b, REL))
    assert worst_b <= REL
    rows_b, infos_b = AQ.solve_rows(zb.reshape(2, 9, L, A), R, 1e-4)
    got_b = beam_figures(rows_b)
    for w in (0, 1):
        print("T1 seed 1 (b), satellite %d: behind the row from the tracked states %s, lambda1 / lambda2 %.1f (no bar: one run)"
              % (w, got_b[w], infos_b[w]["lambda1"] / max(infos_b[w]["lambda2"], 1e-300)))
    ring.close(); mgr.close(); eng.close()
