"""Coherent integration over K code periods (gm_acq_cfg.coherent_periods, CohLoad in acq_stage_f_variants.h) on the GPU.

The fold y_{d,m}[n] = sum_k rho_{d,k} x[(m K + k) N + n] is restated on the host in float32 with the handle's own phasor words and the
same arithmetic (every product and sum rounded on its own, k ascending); the folded groups then go through the unchanged oracle, one
Doppler table at a time.  Then: K <= 1 is today's search bit for bit, every entry point agrees, and the sensitivity the fold buys."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-5


def _codes(n_codes, code_len, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, (n_codes, code_len)) > 0, 1, -1).astype(np.int8)


def _as_c64(x):
    x = np.asarray(x)
    if x.dtype == np.int8 and x.ndim == 2:
        return x[:, 0].astype(np.float32), x[:, 1].astype(np.float32)
    if x.dtype == np.int8:
        return x.astype(np.float32), np.zeros(x.size, np.float32)
    x = x.astype(np.complex64)
    return x.real.astype(np.float32), x.imag.astype(np.float32)


def _fold(x, N, K, M, rho_d):
    """[M][N] complex64 folded groups, in float32 with the device's arithmetic (separate real arrays, no fused operations)"""
    xr, xi = _as_c64(x)
    xr, xi = xr[:K * M * N].reshape(M, K, N), xi[:K * M * N].reshape(M, K, N)
    rr, ri = rho_d.real.astype(np.float32), rho_d.imag.astype(np.float32)
    are = rr[0] * xr[:, 0] - ri[0] * xi[:, 0]
    aim = rr[0] * xi[:, 0] + ri[0] * xr[:, 0]
    for k in range(1, K):
        are = are + (rr[k] * xr[:, k] - ri[k] * xi[:, k])
        aim = aim + (rr[k] * xi[:, k] + ri[k] * xr[:, k])
    y = np.empty((M, N), np.complex64)
    y.real, y.imag = are, aim
    return y


def _rho_f64(freq, K, N, fs):
    k = np.arange(K, dtype=np.float64)
    cyc = np.float64(freq)[:, None] * (k[None, :] * N) / np.float64(fs)
    ang = 2.0 * np.pi * (cyc - np.floor(cyc))
    return (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)


def _check_against_oracle(oracle, eng, x, fs, f_if, N, K, M, dop, prn_ids, codes, code_rate):
    got = eng.last_results
    mx, am, sm = eng.metrics()
    rho = eng.coherent_phasors()
    tables = [oracle.DopplerShiftTable(f_if, float(d), fs, N) for d in dop]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    assert (tf == eng.table_freq).all()
    emax, earg, esum = (np.zeros((len(prn_ids), len(dop)), t) for t in (np.float32, np.uint32, np.float32))
    for d in range(len(dop)):
        y = _fold(x, N, K, M, rho[d]).reshape(-1)
        for w, prn in enumerate(prn_ids):
            ow = oracle.AcquisitionWorker(prn, N, fs, code=(codes[w] if codes is not None else None), code_rate=code_rate)
            _, (bmax, barg, bsum, _) = ow.search_satellite(y, [tables[d]], 0, M, want_planes=True, no_early_exit=True)
            emax[w, d], earg[w, d], esum[w, d] = bmax[0], barg[0], bsum[0]
    assert np.allclose(mx, emax, rtol=REL), (N, K, mx, emax)
    assert np.allclose(sm, esum, rtol=REL), (N, K, sm, esum)
    assert (am == earg).all(), (N, K, am, earg)
    for w, prn in enumerate(prn_ids):
        exp = oracle.decide_from_metrics(emax[w], earg[w], esum[w], tf, N, prn, fs, 0)
        assert (got[w] is None) == (exp is None), (N, K, w, got[w], exp)
        if exp:
            for k in ("prn", "code_phase_samples", "carrier_freq"):
                assert got[w][k] == exp[k], (N, K, w, k, got[w], exp)
    return mx, am, sm


@pytest.mark.parametrize("N,K", [(8000, 1), (8000, 7), (16368, 10), (50000, 5)])
def test_coherent_phasors(gpu, N, K):
    from gnss_sdr_rs_amd import acquisition as A
    fs, f_if = (16.3676e6, 4.1304e6) if N == 16368 else (N * 1000.0, 0.0)
    dop = np.arange(-1000.0, 1001.0, 250.0, dtype=np.float32)
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=[1, 2], n_integrations=2, coherent_periods=K,
                              any_length=N == 50000)
    rho = eng.coherent_phasors()
    assert rho.shape == (dop.size, K)
    if K == 1:
        assert (rho == np.complex64(1.0)).all() and not np.signbit(rho.imag).any()
    want = _rho_f64(eng.table_freq, K, N, fs)
    for part in ("real", "imag"):
        g, w = getattr(rho, part), getattr(want, part)
        assert (np.abs(g - w) <= np.spacing(np.maximum(np.abs(g), np.abs(w)))).all(), (part, g, w)
    eng.close()


# (N, K, M, fmt, f_if, code_len, form)
CASES = [(8000, 5, 2, "i8", 0.0, 1023, "lds"), (8000, 5, 2, "c32", 0.0, 1023, "lds"), (8000, 5, 2, "real", 0.0, 1023, "lds"),
         (16368, 10, 1, "real", 4.1304e6, 1023, "lds"),
         (32000, 2, 2, "i8", 0.0, 1023, "composite"),
         (25000, 4, 1, "i8", 0.0, 1023, "composite"),
         (50000, 5, 2, "i8", 0.0, 1023, "long"),
         (16024, 3, 2, "c32", 0.0, 1023, "long_padded"),
         (16000, 3, 2, "i8", 0.0, 4092, "lds")]


@pytest.mark.parametrize("N,K,M,fmt,f_if,code_len,form", CASES)
def test_coherent_parity_with_the_oracle(gpu, oracle, N, K, M, fmt, f_if, code_len, form):
    from gnss_sdr_rs_amd import acquisition as A, synth
    from gnss_sdr_rs_amd._lib import GmError
    rate = 1.023e6 if code_len == 1023 else 4.092e6
    fs = 16.3676e6 if N == 16368 else float(N) * rate / code_len
    codes = None if code_len == 1023 else _codes(3, code_len, N)
    table = oracle.ca_code_table() if codes is None else codes
    prn_ids, rows = ([3, 9, 21], [2, 8, 20]) if codes is None else ([1, 2, 3], [0, 1, 2])
    dop = np.array([-400.0, -200.0, 0.0, 200.0, 400.0], np.float32)
    sats = [dict(prn_row=rows[0], cn0_dbhz=44.0, doppler_hz=130.0, code_start=N - 91),
            dict(prn_row=rows[2], cn0_dbhz=43.0, doppler_hz=-260.0, code_start=(N * 3) // 7)]
    x = synth.make_scene(table, fs, f_if, K * M * N, sats, config_id=400 + K, code_rate=rate, real_only=fmt == "real")
    x = {"i8": synth.to_i8_iq, "c32": synth.to_c32, "real": synth.to_i8_real}[fmt](x)
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=prn_ids, n_integrations=M, codes=codes, code_rate=rate,
                              coherent_periods=K, any_length=form.startswith("long"))
    assert eng.plan_info()["form"] == form
    with pytest.raises(GmError, match="coherent_periods"):
        eng.search(x[:K * M * N - 8])         # the library's length check counts K * M * N samples
    eng.last_results = eng.search(x)
    mx, am, _ = _check_against_oracle(oracle, eng, x, fs, f_if, N, K, M, dop, prn_ids, codes, rate)
    # (16368 samples are not one code period at 16.3676 MHz: the scene's code drifts 0.39 samples per period against the replica)
    tol = 4 if N == 16368 else 0
    assert abs(int(am[0][int(np.argmax(mx[0]))]) - (N - 91)) <= tol and abs(int(am[2][int(np.argmax(mx[2]))]) - (N * 3) // 7) <= tol
    eng.close()


def test_coherent_strict_sum_order(gpu, oracle):
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, K, M, fs = 32000, 3, 2, 32.0e6
    dop = np.array([-300.0, 0.0, 300.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=44.0, doppler_hz=90.0, code_start=12345)]
    x = synth.to_i8_iq(synth.make_scene(oracle.ca_code_table(), fs, 0.0, K * M * N, sats, config_id=431))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, strict_sum_order=True)
    eng.last_results = eng.search(x)
    _check_against_oracle(oracle, eng, x, fs, 0.0, N, K, M, dop, [5, 6], None, 1.023e6)
    eng.close()


@pytest.mark.parametrize("N", [8000, 16368, 32000, 50000])
def test_coherent_one_period_is_todays_search(gpu, N):
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    fs = 16.3676e6 if N == 16368 else N * 1000.0
    M = 2
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=48.0, doppler_hz=220.0, code_start=N // 3)]
    x = synth.to_i8_iq(synth.make_scene(O.ca_code_table(), fs, 0.0, M * N, sats, config_id=432))
    out = []
    for kw in ({}, dict(coherent_periods=0), dict(coherent_periods=1)):
        eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, any_length=N == 50000, **kw)
        res = eng.search(x)
        mx, am, sm = eng.metrics()
        out.append((res, mx.view(np.uint32).copy(), am.copy(), sm.view(np.uint32).copy()))
        eng.close()
    for o in out[1:]:
        assert o[0] == out[0][0]
        for a, b in zip(o[1:], out[0][1:]):
            assert (a == b).all()


def test_coherent_entry_points_agree(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import acquisition as A, synth, tracking as T
    N, K, M, fs = 8000, 4, 2, 8.0e6
    dop = np.array([-300.0, -100.0, 100.0, 300.0], np.float32)
    sats = [dict(prn_row=6, cn0_dbhz=46.0, doppler_hz=80.0, code_start=3001)]
    x = synth.to_c32(synth.make_scene(oracle.ca_code_table(), fs, 0.0, K * M * N, sats, config_id=433))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[7, 8], n_integrations=M, coherent_periods=K)
    ref = eng.search(x)
    ref_w = [a.copy() for a in eng.metrics()]
    assert ref[0] is not None and ref[0]["code_phase_samples"] == 3001

    def same(res, tail=0):
        assert [r and dict(r, sample_global_index=r["sample_global_index"] - tail) for r in res] == ref
        for a, b in zip(eng.metrics(), ref_w):
            assert (a.view(np.uint32) == b.view(np.uint32)).all()

    d_x = hipbuf.upload(x)
    for deferred in (False, True):
        eng.set_deferred_decision(deferred)        # (a coherent handle accepts the call and decides at once)
        eng.search_dev(d_x, 0)
        eng.decide_dev()
        same(eng.fetch_results())
        tok = eng.prepare_dev(d_x, 0)
        eng.search_prepared_dev(tok)
        eng.decide_dev()
        same(eng.fetch_results())
    eng.set_deferred_decision(False)
    # the ring: the dwell wraps the ring's end
    size = 1 << 16
    ring = T.MulticastRingBuffer(size)
    lead = size - 5000
    ring.write_samples(np.zeros(lead, np.complex64))
    ring.write_samples(x)
    res, tail = eng.search_ring(ring)
    assert tail == lead and (lead % size) + K * M * N > size
    same(res, tail)
    ring.close()
    # fine Doppler on the K*M-period snapshot
    res = eng.search(x)
    fine = eng.finer_doppler(res)
    o = oracle.finer_doppler(x, res[0]["code_phase_samples"], oracle.ca_code_table()[6], fs, (K * M - 1) * N)
    assert fine[0]["fft_size"] == o["fft_size"] and fine[0]["peak_index"] == o["peak_index"], (fine[0], o)
    eng.close()


def _sens_scene(synth, table, cn0, config_id, data_bits=None, sat=True):
    N, fs = 8000, 8.0e6
    sats = [dict(prn_row=11, cn0_dbhz=cn0, doppler_hz=1206.0, code_start=2345)] if sat else []
    if data_bits is not None:
        sats[0].update(data_bits=data_bits, bit_edge_ms=-7)       # bit edges at periods 13, 33: inside the second group of 10
    return synth.to_c32(synth.make_scene(table, fs, 0.0, 20 * N, sats, config_id=config_id)), N, fs


def _ratio(eng, w, d):
    """max / mean of the other cells of plane (w, d): the ratio the decision tests (do_acquisition.rs:236-237)"""
    mx, _, sm = eng.metrics()
    return float(mx[w, d] / ((sm[w, d] - mx[w, d]) / (eng.fft_size - 1)))


def test_coherent_sensitivity(gpu, oracle):
    """35 dB-Hz, 20 ms, no data bits: the reference configuration (K = 1, M = 20, +-5 kHz at 250 Hz, threshold 7) misses it; K = 10,
    M = 2 over +-1 kHz at 50 Hz with the Gamma(2) threshold for 1e-6 false alarms per search finds it."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    table = oracle.ca_code_table()
    x, N, fs = _sens_scene(synth, table, 35.0, 440)
    true_dop = 1206.0
    ref = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=np.arange(-5000.0, 5001.0, 250.0, dtype=np.float32), prn_ids=[12],
                              n_integrations=20, threshold=7.0)
    assert ref.search(x)[0] is None
    d_ref = int(np.argmin(np.abs(ref.table_freq - true_dop)))
    r_ref = _ratio(ref, 0, d_ref)
    ref.close()
    thr = A.detection_threshold(2, 8000 * 41, 1e-6)
    assert 14.0 < thr < 16.0
    dop = np.arange(-1000.0, 1001.0, 50.0, dtype=np.float32) + 1200.0
    coh = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[12], n_integrations=2, coherent_periods=10,
                              decision_mode=A.DECIDE_BEST_BIN, threshold=thr)
    got = coh.search(x)[0]
    assert got is not None
    assert abs(int(got["code_phase_samples"]) - 2345) <= 1 and abs(got["carrier_freq"] - true_dop) <= 50.0, got
    d_coh = int(np.argmin(np.abs(coh.table_freq - true_dop)))
    r_coh = _ratio(coh, 0, d_coh)
    assert r_coh >= 3.0 * r_ref, (r_coh, r_ref)
    noise, _, _ = _sens_scene(synth, table, 35.0, 441, sat=False)
    assert coh.search(noise)[0] is None
    coh.close()


def test_coherent_data_bit_edge_in_a_group(gpu, oracle):
    """40 dB-Hz with 50 bit/s data whose edge falls inside the second group: the clean first group alone carries it."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    x, N, fs = _sens_scene(synth, oracle.ca_code_table(), 40.0, 442, data_bits=[1, -1, 1, 1])
    thr = A.detection_threshold(2, 8000 * 41, 1e-6)
    dop = np.arange(-1000.0, 1001.0, 50.0, dtype=np.float32) + 1200.0
    coh = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[12], n_integrations=2, coherent_periods=10,
                              decision_mode=A.DECIDE_BEST_BIN, threshold=thr)
    got = coh.search(x)[0]
    assert got is not None and abs(int(got["code_phase_samples"]) - 2345) <= 1 and abs(got["carrier_freq"] - 1206.0) <= 50.0, got
    coh.close()
