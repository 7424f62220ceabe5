"""gm_trk_bank / gm_trk_bank_samples on the GPU against trk_bank_model.py (the definition in numpy, f64 sums).

Bar: every word within REL = 1e-5 of env, the model's |out| at df = 0, tau = 0 for that record — the project's tracking bar (REL in
test_gpu_tracking_shapes.py).  Records are built on a signal, so that env > 100, and the tests assert it.  Shapes are the smallest
at which the kernel can go wrong: n below one slice of 4096 samples (2048, and 2047 / 2049 through code_rate), two slices with the
second partial (5000), a third slice of under 1024 samples (9000), a 4092-chip BOC code at n = 16368; tap groups full, one over and
four (T = 1, 3, 16, 17, 64), F = 1, 3, 8 with one F x T = 256 case; both code-index modes.

The records above are all eligible for the exact fast forms (trk_form_classes.py, test_trk_form_classes_host.py).  The last two tests run
that helper's triggers — records outside fast_code_ok, outside fast_car_ok, outside both, and with carrier offsets on both sides — on
T = 1, 3, 7, 17 (TG 1, 4, 8, 16), each a record of its own at n = 2048 (16 777 and 50 000 where the sample rate is the trigger), to the
same bar; and hold an eligible record's words on FASTC = true and FASTC = false equal.  Measured on an MI355X: at most 2.2e-7 of env."""
import ctypes as C

import numpy as np
import pytest

import trk_bank_model as M
import trk_form_classes as FC

pytestmark = pytest.mark.gpu
REL = 1e-5
INVALID, RANGE = -1, -5

TAP_SETS = {1: np.array([0.0]), 3: np.array([0.0, 0.5, -0.5]), 16: np.linspace(-1.875, 1.875, 16),
            17: np.concatenate([np.linspace(-2.0, 2.0, 16), [-1.5]]), 64: np.linspace(-64.0, 64.0, 64),
            32: np.concatenate([np.linspace(-3.0, 3.0, 31), [-1.25]])}
OFF_SETS = {1: np.array([0.0]), 3: np.array([0.0, 500.0, -250.0]), 8: np.array([0.0, 100.0, -100.0, 400.0, -400.0, 1000.0, -1000.0, 37.5])}
COMBOS = [(1, 1), (3, 3), (16, 1), (17, 1), (64, 1), (32, 8), (3, 8)]        # (T, F); 32 x 8 = 256 words


def _record(T, prn, nxt, n, carrier_freq, code_phase=0.0, code_rate=1.023e6, carrier_phase=0.3, active=1):
    s = T.TrkState()
    s.prn, s.active, s.next_sample_index, s.num_samples_per_code = prn, active, nxt, n
    s.carrier_freq, s.carrier_phase, s.code_phase, s.code_rate = carrier_freq, carrier_phase, code_phase, code_rate
    return s


def _worst(out, done, recs, x, fs, rows, taps, offs, mode, boc=False, linear_n=None):
    """the largest |device - model| / env over the records that ran; asserts the bar and env > 100"""
    worst = 0.0
    for r, st in enumerate(recs):
        assert done[r] == 1, r
        seg = x[st.next_sample_index:]
        want = M.bank_state(seg, st, fs, rows[r], taps, offs, mode, boc, n=linear_n)
        env = float(np.abs(M.bank_state(seg, st, fs, rows[r], [0.0], [0.0], mode, boc, n=linear_n)[0, 0]))
        assert env > 100.0, (r, env)                       # a signal is under the correlator
        frac = float(np.max(np.abs(out[r].astype(np.complex128) - want))) / env
        print("record", r, "T x F", len(taps), len(offs), "fraction of env", frac)
        assert frac <= REL, (r, frac)
        worst = max(worst, frac)
    return worst


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.ca_code_table()


SHAPES = [(2.048e6, 1.023e6, 2048), (2.048e6, 1.0235e6, 2047), (2.048e6, 1.0225e6, 2049), (5.0e6, 1.023e6, 5000), (9.0e6, 1.023e6, 9000)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fs,code_rate,n", SHAPES)
def test_bank_against_the_model(gpu, table, fs, code_rate, n, mode):
    from gnss_sdr_rs_amd import tracking as T, synth
    assert M.samples_per_code(fs, code_rate, 1023) == n
    prns = [3, 9, 17, 25]
    air = [p if mode == 0 else p - 1 for p in prns]          # FAITHFUL indexes row `prn`: that code is in the air
    sc = synth.tracking_scene(table, fs, 0.0, prns, 4, config_id=71, cn0=50.0, code_rows=air)
    x = synth.to_c32(sc["x"])
    ring = T.MulticastRingBuffer(1 << 16)
    ring.write_samples(x)
    mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=mode)
    # five records: the four satellites, the last of them one period on; code phases near 0 — in FAITHFUL mode a tap below -1 then
    # asks for a negative phase, which saturates to chip 0
    recs, rows = [], []
    for k, s in enumerate(sc["sats"] + sc["sats"][:1]):
        nxt = s["code_start"] + (n if k == 4 else 0)
        recs.append(_record(T, s["prn"], nxt, n, s["doppler_hz"] + 7.0 * k, code_phase=0.125 * (k % 3), code_rate=code_rate))
        rows.append(table[air[k % 4]])
    worst = 0.0
    for nt, nf in COMBOS:
        taps, offs = TAP_SETS[nt], OFF_SETS[nf]
        out, done = mgr.bank(ring, taps, offs, states=recs)
        assert out.shape == (5, nf, nt) and out.dtype == np.complex64
        worst = max(worst, _worst(out, done, recs, x, fs, rows, taps, offs, mode))
    print("n", n, "mode", mode, "largest fraction of env", worst)
    mgr.close(); ring.close()


def _boc_scene(codes, fs, rate, n_samples, dopp, starts, amp=0.6, sigma=8.0, seed=5):
    L = codes.shape[1]
    tt = np.arange(n_samples, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) * sigma
    for c in range(codes.shape[0]):
        cp = ((tt - starts[c]) * rate / fs) % L
        sub = np.where((cp - np.floor(cp)) < 0.5, 1.0, -1.0)
        x += amp * codes[c][np.floor(cp).astype(np.int64)] * sub * np.exp(2j * np.pi * dopp[c] * tt / fs + 0.3j * c)
    return x.astype(np.complex64)


def test_five_arm_boc_handle(gpu):
    """a custom 4092-chip table at fs = 4.092 MHz, n = 16368 (four slices), BOC(1,1): taps at half-chip fractions, where the
    sub-carrier sign matters; and the bank against the handle's own five arms"""
    from gnss_sdr_rs_amd import tracking as T
    fs, L, rate, n = 4.092e6, 4092, 1.023e6, 16368
    assert M.samples_per_code(fs, rate, L) == n
    rng = np.random.default_rng(56)
    codes = np.where(rng.integers(0, 2, (3, L)) > 0, 1, -1).astype(np.int8)
    dopp, starts = [-1500.0, 200.0, 2750.0], [100, 3000, 9000]
    x = _boc_scene(codes, fs, rate, 3 * n, dopp, starts)
    ring = T.MulticastRingBuffer(1 << 16)
    ring.write_samples(x)
    el, vel = 0.25, 0.6
    mgr = T.TrackingManager(fs, n_channels=3, n_arms=5, code_index_mode=T.CODE_INDEX_FIXED, early_late_space=el,
                            very_early_late_space=vel, boc11=True, codes=codes, nominal_code_rate=rate)
    recs = [_record(T, c + 1, starts[c], n, dopp[c] + 5.0, code_phase=0.25 * c, code_rate=rate) for c in range(3)]
    rows = [codes[c] for c in range(3)]
    taps = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 0.25, -0.25, 1.5, -1.5, 0.75, -0.75, 2.5, -2.5, 0.499, -0.501, 30.5, -30.5])
    offs = OFF_SETS[3]
    out, done = mgr.bank(ring, taps, offs, states=recs)
    print("boc largest fraction of env", _worst(out, done, recs, x, fs, rows, taps, offs, M.FIXED, boc=True))
    # the sub-carrier matters: the same taps without it are somewhere else entirely
    plain = M.bank_state(x[starts[0]:], recs[0], fs, rows[0], taps, offs, M.FIXED, False)
    assert np.max(np.abs(out[0] - plain)) > 0.1 * np.abs(out[0, 0, 0])
    # against the handle's own arms on the same samples and state: p, e, l, ve, vl <-> taps 0, +el, -el, +vel, -vel
    arms = np.array([0.0, el, -el, vel, -vel])
    for c in range(3):
        seg = x[starts[c]:starts[c] + n]
        ch = mgr.channels[c]
        ch.set_state(prn=c + 1, active=1, next_sample_index=starts[c], num_samples_per_code=n, carrier_freq=dopp[c] + 5.0,
                     carrier_phase=0.3, code_phase=0.25 * c, code_rate=rate)
        got = ch.bank(seg, arms)[0]
        same = mgr.bank(ring, arms, states=[ch.state])[0][0, 0]
        assert np.array_equal(got.view(np.uint32), same.view(np.uint32))                  # linear form == ring form
        ref = np.array(ch.early_late_correlation(seg), np.float64)
        env = float(np.hypot(ref[0], ref[1]))
        assert env > 100.0
        frac = float(np.max(np.abs(np.stack([got.real, got.imag], 1).ravel() - ref))) / env
        print("boc channel", c, "bank against the arms, fraction of env", frac)
        assert frac <= REL
    mgr.close(); ring.close()


@pytest.mark.parametrize("strict_libm", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_bank_against_early_late_correlation(gpu, table, mode, strict_libm):
    """df = 0, taps [0, +el, -el]: the per-sample products are gm_trk_correlate's own, the sums agree within the bar"""
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n, prn = 5.0e6, 5000, 7
    row = prn if mode == 0 else prn - 1
    sats = [dict(prn_row=row, cn0_dbhz=50.0, doppler_hz=1830.0, code_start=0, phase=0.7)]
    x = synth.to_c32(synth.make_scene(table, fs, 0.0, 2 * n, sats, config_id=72))
    mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=mode, strict_libm=strict_libm)
    ch = mgr.channels[1]
    ch.start(dict(prn=prn, code_phase_samples=0, code_phase_chips=0.3, carrier_freq=1800.0, fs=fs, mag_relative=10.0,
                  sample_global_index=0, doppler_bin=0))
    for ep in range(2):                                          # the second epoch starts from an advanced phase
        seg = x[ep * n:(ep + 1) * n]
        st = ch.state
        got = ch.bank(seg, [0.0, 0.5, -0.5])[0]
        assert bytes(ch.state) == bytes(st)                      # nothing moved
        ref = np.array(ch.early_late_correlation(seg), np.float64)      # (this one advances the phases)
        env = float(np.hypot(ref[0], ref[1]))
        assert env > 100.0
        frac = float(np.max(np.abs(np.stack([got.real, got.imag], 1).ravel() - ref))) / env
        print("mode", mode, "strict_libm", strict_libm, "epoch", ep, "fraction of env", frac)
        assert frac <= REL
        want = M.bank_state(seg, st, fs, table[row], [0.0, 0.5, -0.5], [0.0], mode, n=n)[0]
        assert np.max(np.abs(got - want)) <= REL * env
    mgr.close()


@pytest.fixture(scope="module")
def wrapped(gpu, table):
    """fs = 2.048 MHz, a ring of 2^14 samples written past its end (20 periods): the ring holds [24576, 40960)"""
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n = 2.048e6, 2048
    prns = [3, 9, 17, 25]
    sc = synth.tracking_scene(table, fs, 0.0, prns, 20, config_id=73, cn0=50.0)
    x = synth.to_c32(sc["x"])
    ring = T.MulticastRingBuffer(1 << 14)
    for k in range(0, x.size, 4096):
        ring.write_samples(x[k:k + 4096])
    assert ring.get_head() == 40960
    mgr = T.TrackingManager(fs, n_channels=5, code_index_mode=T.CODE_INDEX_FIXED)
    yield dict(fs=fs, n=n, sc=sc, x=x, ring=ring, mgr=mgr, T=T, table=table)
    mgr.close(); ring.close()


def _forty(w):
    """40 records that run: the four satellites at every period start the ring still holds"""
    recs, rows = [], []
    k = 0
    while len(recs) < 40:
        s = w["sc"]["sats"][k % 4]
        first = -(-(24576 - s["code_start"]) // w["n"])                   # the first period start at or behind 24576
        nxt = s["code_start"] + (first + (k // 4) % 7) * w["n"]
        assert 24576 <= nxt and nxt + w["n"] <= 40960
        recs.append(_record(w["T"], s["prn"], nxt, w["n"], s["doppler_hz"] - 3.0 * (k // 4), code_phase=0.01 * k))
        rows.append(w["table"][s["prn"] - 1])
        k += 1
    return recs, rows


def test_record_counts_skips_and_the_wrap(wrapped):
    w = wrapped
    T, mgr, ring, n = w["T"], w["mgr"], w["ring"], w["n"]
    recs, rows = _forty(w)
    taps, offs = TAP_SETS[17], OFF_SETS[3]
    # one whose epoch wraps the ring's end (32768 = 2 x 2^14 lies inside it), one at the oldest sample the ring holds
    s0 = w["sc"]["sats"][0]
    wrap = _record(T, s0["prn"], 32768 - 1000, n, s0["doppler_hz"], code_phase=float(((32768 - 1000 - s0["code_start"]) * 1.023e6 / w["fs"]) % 1023))
    oldest = _record(T, s0["prn"], 24576, n, s0["doppler_hz"], code_phase=float(((24576 - s0["code_start"]) * 1.023e6 / w["fs"]) % 1023))
    newest = _record(T, s0["prn"], 40960 - n, n, s0["doppler_hz"], code_phase=float(((40960 - n - s0["code_start"]) * 1.023e6 / w["fs"]) % 1023))
    for group, grows in (([wrap], rows[:1]), ([wrap, oldest, newest] + recs[:2], rows[:1] * 3 + rows[:2]), (recs, rows)):
        out, done = mgr.bank(ring, taps, offs, states=group)
        _worst(out, done, group, w["x"], w["fs"], grows, taps, offs, M.FIXED)
    # skipped records: done 0 and zeros, the call succeeds, the others are what they are alone
    inactive = _record(T, 3, recs[0].next_sample_index, n, recs[0].carrier_freq, active=0)
    bad_row = _record(T, 33, recs[0].next_sample_index, n, recs[0].carrier_freq)
    row_zero = _record(T, 0, recs[0].next_sample_index, n, recs[0].carrier_freq)          # FIXED: row prn - 1 = -1
    not_reached = _record(T, 3, 40960 - n + 1, n, recs[0].carrier_freq)
    overwritten = _record(T, 3, 24575, n, recs[0].carrier_freq)
    long_gone = _record(T, 3, 100, n, recs[0].carrier_freq)
    no_rate = _record(T, 3, recs[0].next_sample_index, n, recs[0].carrier_freq, code_rate=0.0)      # n = round(fs / 0) is no count
    tiny_rate = _record(T, 3, recs[0].next_sample_index, n, recs[0].carrier_freq, code_rate=0.5)    # n = 4.2e9 >= 2^31
    group = [inactive, recs[0], bad_row, row_zero, not_reached, recs[1], overwritten, long_gone, no_rate, tiny_rate]
    out, done = mgr.bank(ring, taps, offs, states=group)
    assert list(done) == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    assert not out[[0, 2, 3, 4, 6, 7, 8, 9]].view(np.uint32).any()
    alone, d1 = mgr.bank(ring, taps, offs, states=[recs[0]])
    assert d1[0] == 1 and np.array_equal(out[1].view(np.uint32), alone[0].view(np.uint32))
    # nothing runs at all: still a success
    out, done = mgr.bank(ring, taps, offs, states=[inactive, not_reached])
    assert not done.any() and not out.view(np.uint32).any()


def test_independence_repetition_and_the_linear_form(wrapped):
    w = wrapped
    mgr, ring = w["mgr"], w["ring"]
    recs, _ = _forty(w)
    for nt, nf in ((17, 3), (64, 1), (32, 8)):
        taps, offs = TAP_SETS[nt], OFF_SETS[nf]
        many, done = mgr.bank(ring, taps, offs, states=recs)
        again, _ = mgr.bank(ring, taps, offs, states=recs)
        assert done.all() and np.array_equal(many.view(np.uint32), again.view(np.uint32))           # two calls, the same words
        for r in (0, 7, 39):
            alone, _ = mgr.bank(ring, taps, offs, states=[recs[r]])
            assert np.array_equal(alone[0].view(np.uint32), many[r].view(np.uint32)), (nt, nf, r)     # alone and among 39 others
            seg = ring.copy_to_slice(recs[r].next_sample_index, w["n"])
            lin = mgr.channels[0].bank(seg, taps, offs, state=recs[r])
            assert np.array_equal(lin.view(np.uint32), many[r].view(np.uint32)), (nt, nf, r)          # the ring form == the linear form


def test_nothing_moves(gpu, table):
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n = 2.048e6, 2048
    prns = [3, 9, 17]
    sc = synth.tracking_scene(table, fs, 0.0, prns, 7, config_id=74, cn0=50.0)
    x = synth.to_c32(sc["x"])
    ring = T.MulticastRingBuffer(1 << 14)
    ring.write_samples(x[:4096]); ring.write_samples(x[4096:8192]); ring.write_samples(x[8192:])
    mgrs = [T.TrackingManager(fs, n_channels=4, code_index_mode=T.CODE_INDEX_FIXED) for _ in range(2)]
    for m in mgrs:
        for i, s in enumerate(sc["sats"]):
            m.channels[i].start(dict(prn=s["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s["doppler_hz"] + 10.0,
                                     fs=fs, mag_relative=10.0, sample_global_index=s["code_start"], doppler_bin=0))
        m.update_all(ring, 2)
    a, twin = mgrs
    taps, offs = TAP_SETS[17], OFF_SETS[3]
    before = a.get_states()
    own, done = a.bank(ring, taps, offs)                                     # states = None: the handle's channels as they stand
    assert list(done) == [1, 1, 1, 0]                                        # the fourth channel was never started
    after = a.get_states()
    assert b"".join(bytes(s) for s in before) == b"".join(bytes(s) for s in after)
    given, done2 = a.bank(ring, taps, offs, states=before)
    assert np.array_equal(own.view(np.uint32), given.view(np.uint32)) and np.array_equal(done, done2)
    rows = [table[s["prn"] - 1] for s in sc["sats"]]
    _worst(own[:3], done[:3], before[:3], x, fs, rows, taps, offs, M.FIXED)
    got = a.update_all(ring, 3)
    want = twin.update_all(ring, 3)                                          # the twin made no bank call
    for g, e in zip(got[:3], want[:3]):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(e).view(np.uint8))
    assert got[3] == want[3] == 3
    assert b"".join(bytes(s) for s in a.get_states()) == b"".join(bytes(s) for s in twin.get_states())
    for m in mgrs:
        m.close()
    ring.close()


SENTINEL = np.float32(-12345.5)


def _raw(L, T, mgr, ring, recs, n_states, taps, offs, n_taps=None, n_offsets=None, null_taps=False, null_cfg=False, null_ring=False,
         null_out=False):
    """gm_trk_bank itself on sentinel-filled outputs -> (status, outputs untouched)"""
    from gnss_sdr_rs_amd import _lib
    t = np.ascontiguousarray(taps, np.float32)
    o = np.ascontiguousarray(offs, np.float32)
    cfg = _lib.TrkBankCfg()
    cfg.n_taps = t.size if n_taps is None else n_taps
    cfg.n_offsets = o.size if n_offsets is None else n_offsets
    cfg.taps_chips = None if null_taps else t.ctypes.data
    cfg.offsets_hz = o.ctypes.data if o.size else None
    out = np.full(2 * 1030 * 256, SENTINEL, np.float32)
    done = np.full(1030, 0x5a, np.uint8)
    arr = None if recs is None else (T.TrkState * len(recs))(*recs)
    rc = L.gm_trk_bank(mgr._h, None if null_ring else ring._h, None if arr is None else C.cast(arr, C.c_void_p), n_states,
                       None if null_cfg else C.byref(cfg), None if null_out else out.ctypes.data_as(C.c_void_p),
                       done.ctypes.data_as(C.c_void_p))
    return rc, bool(np.all(out == SENTINEL) and np.all(done == 0x5a))


def test_every_refusal_leaves_the_outputs(wrapped):
    w = wrapped
    T, mgr, ring = w["T"], w["mgr"], w["ring"]
    from gnss_sdr_rs_amd import _lib
    L = _lib.lib()
    recs, _ = _forty(w)
    one = recs[:1]
    ok = ([0.0, 0.5], [0.0])
    cases = [
        (dict(taps=[0.0], offs=[0.0], n_taps=0), RANGE), (dict(taps=np.zeros(65), offs=[0.0]), RANGE),
        (dict(taps=[0.0], offs=np.zeros(9)), RANGE), (dict(taps=np.zeros(33), offs=np.zeros(8)), RANGE),
        (dict(taps=[0.0, 64.5], offs=[0.0]), RANGE), (dict(taps=[-512.0], offs=[0.0]), RANGE),
        (dict(taps=[0.0, np.nan], offs=[0.0]), INVALID), (dict(taps=[np.inf], offs=[0.0]), INVALID),
        (dict(taps=[0.0], offs=[np.nan]), INVALID), (dict(taps=[0.0], offs=[-np.inf]), INVALID),
        (dict(taps=[0.0], offs=[1.0241e6]), RANGE), (dict(taps=[0.0], offs=[-1.0241e6]), RANGE),
        (dict(taps=[0.0], offs=[0.0], null_taps=True), INVALID), (dict(taps=[0.0], offs=[], n_offsets=2), INVALID),
        (dict(taps=ok[0], offs=ok[1], null_cfg=True), INVALID), (dict(taps=ok[0], offs=ok[1], null_ring=True), INVALID),
        (dict(taps=ok[0], offs=ok[1], null_out=True), INVALID),
    ]
    for kw, status in cases:
        rc, untouched = _raw(L, T, mgr, ring, one, 1, **kw)
        assert rc == status and untouched, (kw, rc, untouched)
    for n_states, status in ((0, RANGE), (1025, RANGE)):
        rc, untouched = _raw(L, T, mgr, ring, recs[:1] * 1030, n_states, *ok)
        assert rc == status and untouched, n_states
    rc, untouched = _raw(L, T, mgr, ring, None, 4, *ok)                   # states NULL: n_states must be n_channels (5)
    assert rc == INVALID and untouched
    assert L.gm_trk_bank(None, ring._h, None, 1, None, None, None) == INVALID
    # the limits themselves pass
    rc, untouched = _raw(L, T, mgr, ring, recs[:1] * 1024, 1024, [64.0, -64.0], [1.024e6, -1.024e6])
    assert rc == 0 and not untouched
    # |tau| < code_len / 2 on a 100-chip code
    short = T.TrackingManager(w["fs"], n_channels=1, code_index_mode=T.CODE_INDEX_FIXED, codes=np.ones((1, 100), np.int8))
    assert _raw(L, T, short, ring, one, 1, [50.0], [0.0]) == (RANGE, True)
    assert _raw(L, T, short, ring, one, 1, [-49.5], [0.0])[0] == 0
    short.close()
    # the linear form: n must equal num_samples_per_code, the row must exist; the output stays as it was
    seg = np.ascontiguousarray(w["x"][recs[0].next_sample_index:recs[0].next_sample_index + w["n"]])
    cfg = _lib.TrkBankCfg()
    taps = np.zeros(3, np.float32)
    cfg.n_taps, cfg.taps_chips = 3, taps.ctypes.data
    out = np.full(6, SENTINEL, np.float32)
    args = lambda st, s, n, c=cfg, o=out: (mgr._h, None if st is None else C.byref(st), None if s is None else s.ctypes.data_as(C.c_void_p),
                                           n, None if c is None else C.byref(c), None if o is None else o.ctypes.data_as(C.c_void_p))
    bad_row = _record(T, 40, 0, w["n"], 0.0)
    no_n = _record(T, 3, 0, 0, 0.0)
    for a, status in ((args(recs[0], seg, w["n"] - 1), RANGE), (args(recs[0], seg, w["n"] + 1), RANGE), (args(no_n, seg, 0), RANGE),
                      (args(bad_row, seg, w["n"]), RANGE), (args(None, seg, w["n"]), INVALID), (args(recs[0], None, w["n"]), INVALID),
                      (args(recs[0], seg, w["n"], None), INVALID), (args(recs[0], seg, w["n"], cfg, None), INVALID)):
        assert L.gm_trk_bank_samples(*a) == status
        assert np.all(out == SENTINEL)
    taps[1] = np.nan
    assert L.gm_trk_bank_samples(*args(recs[0], seg, w["n"])) == INVALID and np.all(out == SENTINEL)
    taps[1] = 0.5
    assert L.gm_trk_bank_samples(*args(recs[0], seg, w["n"])) == 0 and not np.any(out == SENTINEL)


def test_one_chain_acquire_track_bank(gpu, table):
    """the acquire-then-track scene of test_gpu_pipeline.py, cut to what this needs: acquisition on a ring snapshot, ten epochs of
    update_all, then the bank on the live states: the correlation function of every channel peaks at tau = 0 and falls on both sides.

    The margin: the scene's noise is sigma = 16 per component and sample, so a tap's I or Q carries sigma sqrt(n) = 1024 of it; taps
    0.25 chip apart share 1 - 0.25 of their chips, so the noise of a DIFFERENCE of two neighbouring taps has sigma sqrt(n)
    sqrt(2 x 0.25) = 724 per component, and the envelope's difference no more than that; four of these, 2896, is the margin a step
    may go the wrong way by.  The model's step for this C/N0 is a quarter of the envelope sigma sqrt(2 x 10^4.9 / fs) n = 3227."""
    from gnss_sdr_rs_amd import acquisition as A, tracking as T, synth
    fs, N, Mint, n_ms = 4_096_000.0, 4096, 10, 26
    truth = {4: (-1730.0, 1111), 11: (640.0, 4000), 23: (2210.0, 77), 30: (-420.0, 2500)}
    sats = [dict(prn=p, prn_row=p - 1, cn0_dbhz=49.0, doppler_hz=d, code_start=c, phase=0.1 * p) for p, (d, c) in truth.items()]
    x = synth.to_c32(synth.make_scene(table, fs, 0.0, n_ms * N, sats, config_id=61))
    ring = T.MulticastRingBuffer(1 << 17)
    dop = np.arange(-2500.0, 2500.1, 100.0, dtype=np.float32)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, n_integrations=Mint)
    ring.write_samples(x[:12 * N])
    res, local_tail = eng.search_ring(ring)
    found = {r["prn"]: r for r in res if r}
    assert set(found) == set(truth)
    mx, _, _ = eng.metrics()
    mgr = T.TrackingManager(fs, n_channels=4, code_index_mode=T.CODE_INDEX_FIXED)
    for i, (prn, r) in enumerate(sorted(found.items())):
        mgr.channels[i].start(dict(r, carrier_freq=float(eng.table_freq[int(np.argmax(mx[prn - 1]))])))
    ring.write_samples(x[12 * N:])
    _, proc, lost, done = mgr.update_all(ring, 10)
    assert done == 10 and proc.all() and not lost.any()
    taps = np.arange(-4, 5) * 0.25
    states = mgr.get_states()
    out, ok = mgr.bank(ring, taps)
    assert ok.all()
    sigma, amp = 16.0, 16.0 * np.sqrt(2.0 * 10.0 ** 4.9 / fs)
    margin = 4.0 * sigma * np.sqrt(N) * np.sqrt(2.0 * 0.25)
    assert abs(margin - 2896.3) < 0.1 and abs(0.25 * amp * N - 3226.7) < 0.1
    for i, (prn, r) in enumerate(sorted(found.items())):
        env = np.abs(out[i, 0])
        want = M.bank_state(x[states[i].next_sample_index:], states[i], fs, table[prn - 1], taps, [0.0], M.FIXED)
        assert np.max(np.abs(out[i, 0] - want[0])) <= REL * np.abs(want[0, 4])
        print("prn", prn, "envelope over the taps", np.round(env))
        assert np.argmax(env) == 4                                             # the peak is at tau = 0
        assert np.all(np.diff(env[:5]) > -margin) and np.all(np.diff(env[4:]) < margin)
        assert env[4] > 0.5 * amp * N and env[0] < 0.5 * env[4] and env[8] < 0.5 * env[4]
    mgr.close(); eng.close(); ring.close()


# ---- the general arithmetic forms: every trigger of trk_form_classes.TRIGGERS on every tap group ---------------------------------------------
TAP_SETS[7] = np.array([0.0, 0.5, -0.5, 1.25, -1.25, 2.0, -60.5])
assert [FC.tap_group(t) for t in (1, 3, 7, 17)] == [1, 4, 8, 16] and tuple(OFF_SETS[3]) == FC.OFFSETS


def _form_classes(T, row, prn, mode, nt, boc=False, **kw):
    """Every bank trigger of trk_form_classes on nt taps: each is ONE record of its own call, on a signal at its own state, held to REL by
    _worst; the ring form's words equal the linear form's; and a record that is eligible for the exact fast forms gives the SAME WORDS on
    the handles whose spacing is 1.5 (FASTC = false: the bank's taps do not depend on the spacings), with the carrier offsets on both
    sides of fast_car_ok as well.  -> {trigger id: fraction of env}"""
    taps = TAP_SETS[nt]
    by_fs, words, worst = {}, {}, {}
    for t in FC.triggers("bank"):
        by_fs.setdefault(FC.HANDLES[t["handle"]]["fs"], []).append(t)
    for fs, trig in by_fs.items():
        segs, parts, pos = {}, [], 0                   # the samples: one stretch per distinct (state, n), a signal at that state under it
        for t in trig:
            st, n = FC.state_of(t), FC.samples_of(t)
            key = (tuple(sorted(st.items())), n)
            if key not in segs:
                segs[key] = pos
                parts.append(FC.replica(row, fs, n, st["carrier_freq"], st["code_phase"], boc=boc) + FC.noise(n, 500 + len(segs)))
                pos += n
        x = np.concatenate(parts).astype(np.complex64)
        ring = T.MulticastRingBuffer(1 << 17)
        ring.write_samples(x)
        mgrs = {}

        def run(name, t, offs):
            if name not in mgrs:
                mgrs[name] = T.TrackingManager(n_channels=1, code_index_mode=mode, boc11=boc, **dict(FC.HANDLES[name], **kw))
            st, n = FC.state_of(t), FC.samples_of(t)
            start = segs[(tuple(sorted(st.items())), n)]
            rec = _record(T, prn, start, n, **st)
            lin = mgrs[name].channels[0].bank(x[start:start + n], taps, offs, state=rec)
            if n != FC.samples_per_code(fs):           # only gm_trk_bank_samples takes n from the record
                return lin[None], np.ones(1, np.uint8), rec, n
            out, done = mgrs[name].bank(ring, taps, offs, states=[rec])
            assert np.array_equal(out[0].view(np.uint32), lin.view(np.uint32)), (t["id"], name)      # the ring form == the linear form
            return out, done, rec, None

        for t in trig:
            offs = np.array(t.get("offsets", FC.OFFSETS))
            out, done, rec, linear_n = run(t["handle"], t, offs)
            worst[t["id"]] = _worst(out, done, [rec], x, fs, [row], taps, offs, mode, boc, linear_n)
            words[t["id"]] = out.view(np.uint32)
        if "el15" in mgrs:                             # form independence, bit for bit
            for tid in ("early-late-1.5", "very-early-late-1.5-five-arms"):
                assert np.array_equal(words[tid], words["eligible"]), (nt, mode, tid)
            t = FC.BY_ID["offsets-on-both-sides"]
            out, _, _, _ = run("el15", t, np.array(t["offsets"]))
            assert np.array_equal(out.view(np.uint32), words[t["id"]]), (nt, mode, "offsets on both sides")
        for m in mgrs.values():
            m.close()
        ring.close()
    for t in FC.triggers("bank"):
        print("T %d (TG %d) mode %d %-30s %-44s fraction of env %.2e = %.4f of the bar"
              % (nt, FC.tap_group(nt), mode, t["id"], "/".join("%s-%s" % f for f in FC.forms_of(t)), worst[t["id"]], worst[t["id"]] / REL))
    return worst


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nt", [1, 3, 7, 17])
def test_general_forms_on_every_tap_group(gpu, table, nt, mode):
    """T = 1, 3, 7, 17 (TG 1, 4, 8, 16) x F = 3 in both code-index modes: the four FASTC = false bodies, the general division beside the
    fast one inside one record, and the words of an eligible record on both bodies.  FAITHFUL and FIXED differ exactly where
    floor(phase) < 0, which code_phase = -0.75 reaches on every tap."""
    from gnss_sdr_rs_amd import tracking as T
    prn = 7
    w = _form_classes(T, table[prn if mode == 0 else prn - 1], prn, mode, nt)
    assert set(w) == {t["id"] for t in FC.triggers("bank")}


@pytest.mark.parametrize("kind", ["boc11", "strict_libm"])
def test_general_forms_boc_and_strict_libm(gpu, table, kind):
    """the same triggers on a BOC(1,1) handle (a custom 1023-chip table; T = 7 with taps at half-chip fractions: the sub-carrier's half chip
    of a negative phase) and on a strict_libm handle (T = 3)"""
    from gnss_sdr_rs_amd import tracking as T
    if kind == "boc11":
        codes = np.where(np.random.default_rng(57).integers(0, 2, (3, FC.LEN)) > 0, 1, -1).astype(np.int8)
        _form_classes(T, codes[1], 2, M.FIXED, 7, boc=True, codes=codes, nominal_code_rate=FC.RATE)
    else:
        _form_classes(T, table[6], 7, M.FIXED, 3, strict_libm=True)
