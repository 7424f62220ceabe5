"""Acquisition at any multiple-of-8 fft_size (gm_acq_cfg.any_length, acq_long.hip) against the generalised oracle, whose FFT plans
any length: the native long form (L = N = Q x a base, Q up to 32) and the padded form (L >= 2N, the circular correlation through a
zero-padded periodic extension).  Same checks as the composite sizes' parity tests: per-(worker, bin) max / first argmax / sum,
identical decisions; then the other entry points, strict_sum_order, and the acquire-then-track chain at 50 Msps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-5


def _codes(n_codes, code_len, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, (n_codes, code_len)) > 0, 1, -1).astype(np.int8)


def _setup(oracle, N, code_len, code_rate, n_prn, seed):
    """fs for one code period of N samples; GPS C/A (codes None) or a random +-1 family"""
    fs = float(N) * code_rate / code_len
    if code_len == 1023:
        prn_ids = [3, 9, 21][:n_prn]
        return fs, None, prn_ids, oracle.ca_code_table(), [p - 1 for p in prn_ids]
    codes = _codes(n_prn, code_len, seed)
    return fs, codes, list(range(1, n_prn + 1)), codes, list(range(n_prn))


def _check_against_oracle(oracle, eng, x, fs, N, M, dop, prn_ids, codes, code_rate):
    """metrics of the last search and its decisions against the oracle's worker (its plane sum is in the reference's own order),
    per (worker, bin)"""
    got = eng.last_results
    mx, am, sm = eng.metrics()
    tables = [oracle.DopplerShiftTable(0.0, float(d), fs, N) for d in dop]
    xc = x if x.dtype == np.complex64 else (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)
    for w, prn in enumerate(prn_ids):
        ow = oracle.AcquisitionWorker(prn, N, fs, code=(codes[w] if codes is not None else None), code_rate=code_rate)
        exp, (bmax, barg, bsum, _) = ow.search_satellite(xc, tables, 0, M, want_planes=True, no_early_exit=True)
        assert np.allclose(mx[w], bmax, rtol=REL), (N, w, mx[w], bmax)
        assert np.allclose(sm[w], bsum, rtol=REL), (N, w, sm[w], bsum)
        assert (am[w] == barg).all(), (N, w, am[w], barg)
        assert (got[w] is None) == (exp is None), (N, w, got[w], exp)
        if exp:
            for k in ("prn", "code_phase_samples", "doppler_bin", "carrier_freq"):
                assert got[w][k] == exp[k], (N, w, k, got[w], exp)
    return mx, am, sm


@pytest.mark.parametrize("N,code_len,form", [(50000, 1023, "long"),           # GPS C/A at 50 Msps
                                             (200000, 4092, "long"),          # 4 ms 4092-chip code at 50 Msps (configs[4]'s rate)
                                             (61440, 1023, "long"),           # 15 x 4096
                                             (4088, 1023, "long_padded"),
                                             (16024, 1023, "long_padded"),    # 8 x 2003
                                             (38400, 1023, "long_padded"),    # 38.4 Msps
                                             (40520, 4092, "long_padded")])
def test_any_length_parity_with_the_oracle(gpu, oracle, N, code_len, form):
    from gnss_sdr_rs_amd import acquisition as A, synth
    rate, M = 1.023e6, 2
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    fs, codes, prn_ids, table, rows = _setup(oracle, N, code_len, rate, 3, N)
    sats = [dict(prn_row=rows[0], cn0_dbhz=50.0, doppler_hz=180.0, code_start=N - 77),
            dict(prn_row=rows[2], cn0_dbhz=49.0, doppler_hz=-390.0, code_start=(N * 3) // 7)]
    x = synth.to_i8_iq(synth.make_scene(table, fs, 0.0, M * N, sats, config_id=300 + code_len, code_rate=rate))
    with pytest.raises(Exception):       # the flag is what opens the size: without it, GM_ERR_UNSUPPORTED_N as before
        A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prn_ids, n_integrations=M, codes=codes, code_rate=rate)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prn_ids, n_integrations=M, codes=codes, code_rate=rate,
                              any_length=True)
    assert eng.plan_info()["form"] == form
    words = []
    for src in (x, (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)):      # int8 IQ and c32
        eng.last_results = eng.search(src)
        mx, am, sm = _check_against_oracle(oracle, eng, src, fs, N, M, dop, prn_ids, codes, rate)
        words.append((eng.last_results, am.copy()))
    assert words[0][0] == words[1][0] and (words[0][1] == words[1][1]).all()
    assert am[0][int(np.argmax(mx[0]))] == N - 77 and am[2][int(np.argmax(mx[2]))] == (N * 3) // 7
    assert abs(float(dop[int(np.argmax(mx[0]))]) - 180.0) <= 250.0
    eng.close()


def test_any_length_largest_padded_size(gpu, oracle):
    """N = 262136 = 8 x 7 x 31 x 151 (padded to 32 x 16384 = 2^19), one PRN, one bin, one integration."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, M, rate = 262136, 1, 1.023e6
    fs = float(N) * 1000.0
    dop = np.array([0.0], np.float32)
    sats = [dict(prn_row=6, cn0_dbhz=50.0, doppler_hz=60.0, code_start=123457)]
    x = synth.to_c32(synth.make_scene(oracle.ca_code_table(), fs, 0.0, M * N, sats, config_id=311))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[7], n_integrations=M, any_length=True)
    assert eng.plan_info() == dict(form="long_padded", base=16384, q=32, transform_len=1 << 19)
    eng.last_results = eng.search(x)
    _, am, _ = _check_against_oracle(oracle, eng, x, fs, N, M, dop, [7], None, rate)
    assert am[0][0] == 123457
    eng.close()


@pytest.mark.parametrize("N", [8000, 16368, 32000])
def test_any_length_keeps_todays_paths_bit_identical(gpu, N):
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    fs, M = float(N) * 1000.0, 2
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=48.0, doppler_hz=220.0, code_start=N // 3)]
    x = synth.to_i8_iq(synth.make_scene(O.ca_code_table(), fs, 0.0, M * N, sats, config_id=320))
    out = []
    for flag in (False, True):
        eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, any_length=flag)
        res = eng.search(x)
        mx, am, sm = eng.metrics()
        out.append((res, mx.view(np.uint32).copy(), am.copy(), sm.view(np.uint32).copy(), eng.code_fft(0).view(np.uint32).copy()))
        eng.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert (a == b).all()


@pytest.mark.parametrize("N", [50000, 16024])
def test_any_length_strict_sum_order(gpu, oracle, N):
    from gnss_sdr_rs_amd import acquisition as A, synth
    rate, M = 1.023e6, 2
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    fs, codes, prn_ids, table, rows = _setup(oracle, N, 1023, rate, 2, N)
    sats = [dict(prn_row=rows[1], cn0_dbhz=50.0, doppler_hz=-140.0, code_start=N // 5)]
    x = synth.to_c32(synth.make_scene(table, fs, 0.0, M * N, sats, config_id=330))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prn_ids, n_integrations=M, strict_sum_order=True, any_length=True)
    eng.last_results = eng.search(x)
    _check_against_oracle(oracle, eng, x, fs, N, M, dop, prn_ids, codes, rate)
    assert eng.last_results[1] and eng.last_results[1]["code_phase_samples"] == N // 5
    eng.close()


def test_any_length_entry_points(gpu, oracle, hipbuf):
    """On a padded size: the device ring, search_dev + decide_dev, prepare_dev / search_prepared_dev and deferred decisions give the
    words of search(); code_fft is the length-N spectrum; reference_products is refused on the long path."""
    from gnss_sdr_rs_amd import acquisition as A, tracking as T, synth, GmError
    N, M, rate = 16024, 2, 1.023e6
    fs = float(N) * 1000.0
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    prns = [5, 12, 20]
    P, D = len(prns), dop.size
    sats = [dict(prn_row=4, cn0_dbhz=50.0, doppler_hz=120.0, code_start=12000),
            dict(prn_row=11, cn0_dbhz=50.0, doppler_hz=-310.0, code_start=55)]
    x = synth.to_c32(synth.make_scene(oracle.ca_code_table(), fs, 0.0, 3 * N, sats, config_id=340))
    with pytest.raises(GmError) as e:
        A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prns, n_integrations=M, reference_products=True, any_length=True)
    assert e.value.status == -1
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prns, n_integrations=M, any_length=True)
    for w, p in enumerate(prns):
        ref = oracle.AcquisitionWorker(p, N, fs).ca_code_samples_fft
        assert np.linalg.norm(eng.code_fft(w) - ref) / np.linalg.norm(ref) < REL
    key = lambda r: r and (r["prn"], r["code_phase_samples"], r["doppler_bin"], r["mag_relative"], r["sample_global_index"])
    res = eng.search(x[N:(M + 1) * N], local_tail=N)
    mx, am, sm = eng.metrics()
    assert res[0]["code_phase_samples"] == 12000 and res[1]["code_phase_samples"] == 55
    # device ring: the M*N samples ending at the head
    ring = T.MulticastRingBuffer(1 << 16)
    ring.write_samples(x)
    rres, tail = eng.search_ring(ring)
    assert tail == N and [key(r) for r in rres] == [key(r) for r in res]
    ring.close()
    # device pointers
    words = 3 * P * D
    d_x = hipbuf.upload(x[N:(M + 1) * N])
    d_met = hipbuf.alloc(words * 4)
    eng.search_dev(d_x, A.FMT_C32, d_met)
    eng.decide_dev(d_met, local_tail=N)
    assert [key(r) for r in eng.fetch_results(P)] == [key(r) for r in res]
    plain = hipbuf.download(d_met, words * 4, np.uint32).copy()
    assert (plain[:P * D].view(np.float32).reshape(P, D) == mx).all() and (plain[P * D:2 * P * D].reshape(P, D) == am).all()
    assert (plain[2 * P * D:].view(np.float32).reshape(P, D) == sm).all()
    eng.set_deferred_decision(True)
    tok = eng.prepare_dev(d_x, A.FMT_C32)
    for _ in range(3):
        eng.search_prepared_dev(tok, d_met)
        tok = eng.prepare_dev(d_x, A.FMT_C32)
        eng.decide_dev(d_met, local_tail=N)
    eng.synchronize()
    assert (hipbuf.download(d_met, words * 4, np.uint32) == plain).all()
    assert [key(r) for r in eng.fetch_results(P)] == [key(r) for r in res]
    eng.search_dev(d_x, A.FMT_C32, None)
    eng.decide_dev(None, local_tail=N)
    assert [key(r) for r in eng.fetch_results(P)] == [key(r) for r in res]
    eng.set_deferred_decision(False)
    eng.close()


def test_any_length_acquire_then_track_gps_50msps(gpu, oracle):
    """configs[4]'s rate: GPS C/A at N = 50000 acquired from the device ring, then a 3-arm FIXED TrackingManager started from the
    results holds every channel in lock (carrier within 15 Hz of the truth, prompt above early and late)."""
    from gnss_sdr_rs_amd import acquisition as A, tracking as T, synth
    t = oracle.ca_code_table()
    fs, N, M, n_ms = 50.0e6, 50000, 2, 40
    truth = {4: (-1730.0, 11111), 11: (640.0, 40000), 23: (2210.0, 77), 30: (-420.0, 25000)}
    sats = [dict(prn=p, prn_row=p - 1, cn0_dbhz=49.0, doppler_hz=d, code_start=c, phase=0.1 * p) for p, (d, c) in truth.items()]
    x = synth.to_c32(synth.make_scene(t, fs, 0.0, n_ms * N, sats, config_id=350))
    ring = T.MulticastRingBuffer(1 << 22)
    dop = np.arange(-2500.0, 2500.1, 100.0, dtype=np.float32)
    prns = [4, 7, 11, 23, 30]
    # (the strongest bin of the grid: with tens of thousands of cells per plane the reference's first-passing-bin rule stops on noise
    # or on a neighbouring bin — a PLL is handed the best one, as the C++ receiver's decision_mode option does)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prns, n_integrations=M, decision_mode=A.DECIDE_BEST_BIN,
                              any_length=True)
    assert eng.plan_info()["form"] == "long"
    ring.write_samples(x[:3 * N])
    res, local_tail = eng.search_ring(ring)
    assert local_tail == N
    # (PRN 7 is not in the scene: the reference's peak / mean > 7 test may false-alarm on its 51 x 50 000-cell noise planes, as at
    # every size of this order — only the simulated satellites are pinned and tracked)
    found = {r["prn"]: (w, r) for w, r in enumerate(res) if r and r["prn"] in truth}
    assert set(found) == set(truth)
    mx, _, _ = eng.metrics()
    mgr = T.TrackingManager(fs, n_channels=4, code_index_mode=T.CODE_INDEX_FIXED)
    for i, (prn, (w, r)) in enumerate(sorted(found.items())):
        # a chip is 49 samples at 50 Msps: the correlation triangle's top is flat to the noise within a few samples
        assert abs(int(r["code_phase_samples"]) - truth[prn][1]) <= 4, (prn, r)
        assert r["sample_global_index"] == local_tail + r["code_phase_samples"]
        best = int(np.argmax(mx[w]))
        assert abs(dop[best] - truth[prn][0]) <= 50.0
        mgr.channels[i].start(dict(r, carrier_freq=float(eng.table_freq[best])))
    ring.write_samples(x[3 * N:])
    outs, proc, lost, done = mgr.update_all(ring, n_ms)
    assert not lost.any()
    for i, (prn, (w, r)) in enumerate(sorted(found.items())):
        n_run = int(proc[:, i].sum())
        assert n_run >= 30
        s = mgr.channels[i].state
        assert s.active and s.prn == prn and s.lost_counter == 0
        assert abs(s.carrier_freq - truth[prn][0]) < 15.0
        ip, qp = outs[:n_run, i, 0], outs[:n_run, i, 1]
        e = np.hypot(outs[n_run - 10:n_run, i, 2], outs[n_run - 10:n_run, i, 3]).mean()
        l = np.hypot(outs[n_run - 10:n_run, i, 4], outs[n_run - 10:n_run, i, 5]).mean()
        p = np.hypot(ip[-10:], qp[-10:]).mean()
        assert p > e and p > l
    eng.close(); mgr.close(); ring.close()


def _boc_scene(codes, fs, rate, L, n_samples, dopp, starts, amp=0.6, sigma=8.0, seed=5):
    """BOC(1,1) signals (a +-1 square sub-carrier of one period per chip) of the codes' rows in complex Gaussian noise"""
    tt = np.arange(n_samples, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) * sigma
    for c in range(codes.shape[0]):
        cp = ((tt - starts[c]) * rate / fs) % L
        sub = np.where((cp - np.floor(cp)) < 0.5, 1.0, -1.0)
        x += amp * codes[c][np.floor(cp).astype(np.int64)] * sub * np.exp(2j * np.pi * dopp[c] * tt / fs + 0.3j * c)
    return x.astype(np.complex64)


def test_any_length_acquire_then_track_boc11_50msps(gpu, oracle):
    """configs[4] itself: a 4092-chip BOC(1,1) code at 50 Msps, N = 200 000 = 20 x 10 000.  The acquisition replica is the code as
    +-1 half-chips (8184 at 2.046 Mcps); the results start the five-arm boc11 TrackingManager, which holds every channel in lock."""
    from gnss_sdr_rs_amd import acquisition as A, tracking as T
    fs, L, rate, C, E = 50.0e6, 4092, 1.023e6, 4, 40
    N = int(round(fs / (rate / L)))
    assert N == 200000
    codes = _codes(C, L, 77)
    dopp = np.array([-740.0, 410.0, 160.0, -310.0])
    cstart = np.array([1234, 150000, 77, 99999])
    x = _boc_scene(codes, fs, rate, L, (E + 2) * N, dopp, cstart)
    half = (np.repeat(codes, 2, axis=1) * np.tile(np.array([1, -1], np.int8), L)[None, :]).astype(np.int8)
    dop = np.arange(-1000.0, 1000.1, 50.0, dtype=np.float32)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=np.arange(1, C + 1), n_integrations=1, codes=half,
                              code_rate=2 * rate, decision_mode=A.DECIDE_BEST_BIN, any_length=True)
    assert eng.plan_info() == dict(form="long", base=10000, q=20, transform_len=N)
    ring = T.MulticastRingBuffer(1 << 24)
    ring.write_samples(x[:2 * N])
    res, local_tail = eng.search_ring(ring)
    assert local_tail == N
    mx, _, _ = eng.metrics()
    kw = dict(n_arms=5, early_late_space=0.25, very_early_late_space=0.6, boc11=True, codes=codes)
    mgr = T.TrackingManager(fs, n_channels=C, code_index_mode=T.CODE_INDEX_FIXED, nominal_code_rate=rate, **kw)
    for c in range(C):
        r = res[c]
        assert r and r["prn"] == c + 1, (c, r)
        assert abs(int(r["code_phase_samples"]) - int(cstart[c] - local_tail) % N) <= 2, (c, r, cstart[c])      # (12 samples per half-chip)
        best = int(np.argmax(mx[c]))
        assert abs(dop[best] - dopp[c]) <= 50.0
        mgr.channels[c].start(dict(r, carrier_freq=float(eng.table_freq[best])))
    ring.write_samples(x[2 * N:])
    outs, proc, lost, done = mgr.update_all(ring, E)
    assert not lost.any()
    for c in range(C):
        n_run = int(proc[:, c].sum())
        assert n_run >= E - 3
        s = mgr.channels[c].state
        assert s.active and s.prn == c + 1 and s.lost_counter == 0
        assert abs(s.carrier_freq - dopp[c]) < 15.0
        ip, qp = outs[:n_run, c, 0], outs[:n_run, c, 1]
        e = np.hypot(outs[n_run - 10:n_run, c, 2], outs[n_run - 10:n_run, c, 3]).mean()
        l = np.hypot(outs[n_run - 10:n_run, c, 4], outs[n_run - 10:n_run, c, 5]).mean()
        p = np.hypot(ip[-10:], qp[-10:]).mean()
        assert p > e and p > l
    eng.close(); mgr.close(); ring.close()
