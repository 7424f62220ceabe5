"""The edge search of a coherent handle (gm_acq_set_edge_search, EdgeLoad in acq_stage_f_variants.h) on the GPU.

Hypothesis h is the coherent search on the samples from period o_h on with s[k] * rho[d][k] in the fold.  The host restates that fold
in float32 with the handle's own phasor words (every product and sum rounded on its own, k ascending; the multiplication by +-1 is
exact) and sends the folded groups through the unchanged oracle, one Doppler table at a time.  The reduction over the hypotheses is
checked word for word against numpy on the device's own block.  Then: a hypothesis is a shifted coherent search, off is today's
handle, every entry point agrees, and what the search buys on a data-bit edge and under a secondary code."""
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


def _fold(x, N, K, M, rho_d, offset=0, sec=None):
    """[M][N] complex64 folded groups of the dwell from period `offset` on, with sec[k] * rho_d[k] as the phasor words: float32 with the
    device's arithmetic (separate real arrays, no fused operations)"""
    xr, xi = _as_c64(x)
    lo = offset * N
    xr, xi = xr[lo:lo + K * M * N].reshape(M, K, N), xi[lo:lo + K * M * N].reshape(M, K, N)
    s = np.ones(K, np.float32) if sec is None else np.asarray(sec, np.float32)
    rr, ri = s * rho_d.real.astype(np.float32), s * rho_d.imag.astype(np.float32)
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
    cyc = np.asarray(freq, np.float64)[:, None] * (k[None, :] * N) / np.float64(fs)
    ang = 2.0 * np.pi * (cyc - np.floor(cyc))
    return (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)


def _restate(oracle, x, fs, f_if, N, K, M, dop, prn_ids, codes, code_rate, offsets, sec, rho):
    """The CPU restatement: (max, argmax, sum), each [P][H][D], from the numpy fold and the oracle, and the tables' frequencies"""
    tables = [oracle.DopplerShiftTable(f_if, float(d), fs, N) for d in dop]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    P, H, D = len(prn_ids), len(offsets), len(dop)
    emax, earg, esum = (np.zeros((P, H, D), t) for t in (np.float32, np.uint32, np.float32))
    workers = [oracle.AcquisitionWorker(prn, N, fs, code=(codes[w] if codes is not None else None), code_rate=code_rate)
               for w, prn in enumerate(prn_ids)]
    for h, o in enumerate(offsets):
        for d in range(D):
            y = _fold(x, N, K, M, rho[d], int(o), sec).reshape(-1)
            for w, ow in enumerate(workers):
                _, (bmax, barg, bsum, _) = ow.search_satellite(y, [tables[d]], 0, M, want_planes=True, no_early_exit=True)
                emax[w, h, d], earg[w, h, d], esum[w, h, d] = bmax[0], barg[0], bsum[0]
    return emax, earg, esum, tf


def _reduce(fmx, fam, fsm):
    """numpy's reduction of a [P][H][D] block: per cell the largest max, the lowest h on ties (np.argmax returns the first)"""
    ch = np.argmax(fmx, axis=1).astype(np.uint32)
    pick = lambda a: np.take_along_axis(a, ch[:, None, :].astype(np.int64), axis=1)[:, 0, :]
    return pick(fmx), pick(fam), pick(fsm), ch


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_edge(oracle, eng, got, x, fs, f_if, N, K, M, dop, prn_ids, codes, code_rate, offsets, sec, threshold=7.0):
    fmx, fam, fsm = eng.edge_metrics()
    emax, earg, esum, tf = _restate(oracle, x, fs, f_if, N, K, M, dop, prn_ids, codes, code_rate, offsets, sec, eng.coherent_phasors())
    assert (tf == eng.table_freq).all()
    assert (fam == earg).all(), (N, K, fam, earg)
    assert np.allclose(fmx, emax, rtol=REL, atol=0.0), (N, K, fmx, emax)
    assert np.allclose(fsm, esum, rtol=REL, atol=0.0), (N, K, fsm, esum)
    # the reduction, word for word on the device's own block
    rmx, ram, rsm, ch = _reduce(fmx, fam, fsm)
    mx, am, sm = eng.metrics()
    assert (_words(mx) == _words(rmx)).all() and (am == ram).all() and (_words(sm) == _words(rsm)).all()
    assert (eng.edge_choice() == ch).all()
    for w, prn in enumerate(prn_ids):
        exp = oracle.decide_from_metrics(rmx[w], ram[w], rsm[w], tf, N, prn, fs, 0, threshold)
        assert (got[w] is None) == (exp is None), (N, K, w, got[w], exp)
        if exp:
            for k in ("prn", "code_phase_samples", "carrier_freq"):
                assert got[w][k] == exp[k], (N, K, w, k, got[w], exp)
            assert got[w]["edge_offset_periods"] == int(offsets[ch[w, got[w]["doppler_bin"]]]), (got[w], ch[w])
    return fmx, fam, fsm


# (N, K, M, fmt, f_if, code_len, form)
CASES = [(8000, 5, 2, "i8", 0.0, 1023, "lds"), (8000, 5, 2, "real", 0.0, 1023, "lds"),
         (16368, 10, 1, "real", 4.1304e6, 1023, "lds"),
         (32000, 2, 2, "i8", 0.0, 1023, "composite"),
         (50000, 5, 2, "i8", 0.0, 1023, "long"),
         (16024, 3, 2, "c32", 0.0, 1023, "long_padded"),
         (16000, 3, 2, "i8", 0.0, 4092, "lds")]
OFFSETS = [0, 2, 5]


@pytest.mark.parametrize("with_row", [False, True])
@pytest.mark.parametrize("N,K,M,fmt,f_if,code_len,form", CASES)
def test_edge_parity_with_the_oracle(gpu, oracle, N, K, M, fmt, f_if, code_len, form, with_row):
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
    n = (K * M + OFFSETS[-1]) * N
    x = synth.make_scene(table, fs, f_if, n, sats, config_id=600 + K, code_rate=rate, real_only=fmt == "real")
    x = {"i8": synth.to_i8_iq, "c32": synth.to_c32, "real": synth.to_i8_real}[fmt](x)
    sec = np.where(np.random.default_rng(N + K).integers(0, 2, K) > 0, 1, -1).astype(np.int8) if with_row else None
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=prn_ids, n_integrations=M, codes=codes, code_rate=rate,
                              coherent_periods=K, any_length=form.startswith("long"))
    assert eng.plan_info()["form"] == form
    eng.set_edge_search(OFFSETS, sec)
    assert eng.dwell_samples == n
    with pytest.raises(GmError, match="samples_chunk shorter"):
        eng.search(x[:n - 8])
    got = eng.search(x)
    _check_edge(oracle, eng, got, x, fs, f_if, N, K, M, dop, prn_ids, codes, rate, OFFSETS, sec)
    eng.close()


def test_edge_strict_sum_order(gpu, oracle):
    """strict_sum_order on a composite size: the stored power planes grow by H"""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, K, M, fs = 32000, 3, 2, 32.0e6
    offsets = [1, 4]
    dop = np.array([-300.0, 0.0, 300.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=44.0, doppler_hz=90.0, code_start=12345)]
    x = synth.to_i8_iq(synth.make_scene(oracle.ca_code_table(), fs, 0.0, (K * M + 4) * N, sats, config_id=631))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, strict_sum_order=True)
    eng.set_edge_search(offsets, [1, -1, 1])
    got = eng.search(x)
    _check_edge(oracle, eng, got, x, fs, 0.0, N, K, M, dop, [5, 6], None, 1.023e6, offsets, [1, -1, 1])
    eng.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N", [8000, 32000, 50000])
def test_a_hypothesis_is_a_shifted_coherent_search(gpu, N, strict):
    """Without a row, hypothesis h's planes are those a plain coherent handle gets from x[o_h N : o_h N + K M N]: the same 32-bit words,
    with strict_sum_order and in default mode alike (a cell's words do not depend on what shares the launch: the tail split of stage C
    adds an item's planes in the order an uncut item does)."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    from oracle import oracle as O
    K, M, fs = 3, 2, N * 1000.0
    offsets = [0, 1, 4]
    dop = np.array([-300.0, 0.0, 300.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=46.0, doppler_hz=90.0, code_start=N // 5)]
    x = synth.to_i8_iq(synth.make_scene(O.ca_code_table(), fs, 0.0, (K * M + 4) * N, sats, config_id=632))
    kw = dict(doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, strict_sum_order=strict, any_length=N == 50000)
    plain = A.AcquisitionEngine(fs, 0.0, N, **kw)
    eng = A.AcquisitionEngine(fs, 0.0, N, **kw)
    eng.set_edge_search(offsets)
    eng.search(x)
    fmx, fam, fsm = eng.edge_metrics()
    for h, o in enumerate(offsets):
        plain.search(x[o * N:o * N + K * M * N])
        mx, am, sm = plain.metrics()
        assert (fam[:, h] == am).all(), (N, h)
        assert np.allclose(fmx[:, h], mx, rtol=REL, atol=0.0) and np.allclose(fsm[:, h], sm, rtol=REL, atol=0.0), (N, h)
        assert (_words(fmx[:, h]) == _words(mx)).all() and (_words(fsm[:, h]) == _words(sm)).all(), (N, h, strict, fmx[:, h], mx, fsm[:, h], sm)
    plain.close()
    eng.close()


@pytest.mark.parametrize("N", [8000, 32000, 50000])
def test_edge_off_is_todays_handle(gpu, N):
    from gnss_sdr_rs_amd import acquisition as A, synth
    from gnss_sdr_rs_amd._lib import GmError
    from oracle import oracle as O
    K, M, fs = 3, 2, N * 1000.0
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    sats = [dict(prn_row=4, cn0_dbhz=48.0, doppler_hz=220.0, code_start=N // 3)]
    x = synth.to_i8_iq(synth.make_scene(O.ca_code_table(), fs, 0.0, (K * M + 3) * N, sats, config_id=633))
    xs = x[:K * M * N]

    def words(eng):
        mx, am, sm = eng.metrics()
        return _words(mx).copy(), am.copy(), _words(sm).copy()

    # (the strongest bin under the cell-count threshold: the default 7 passes noise cells of a 50000-cell plane at M = 2)
    kw = dict(doppler_hz=dop, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, any_length=N == 50000,
              decision_mode=A.DECIDE_BEST_BIN, threshold=A.detection_threshold(M, N * dop.size * 2, 1e-6))
    ref = A.AcquisitionEngine(fs, 0.0, N, **kw)        # never sees set_edge_search
    ref_res, ref_w = ref.search(xs), words(ref)
    assert ref_res[0] is not None and ref_res[0]["code_phase_samples"] == N // 3 and "edge_offset_periods" not in ref_res[0]
    assert ref.dwell_samples == K * M * N
    with pytest.raises(GmError):
        ref.edge_metrics()
    ref.close()
    eng = A.AcquisitionEngine(fs, 0.0, N, **kw)
    # one hypothesis at offset 0 without a row: the plain coherent search's words
    eng.set_edge_search([0])
    res = eng.search(xs)
    assert [r and {k: v for k, v in r.items() if k != "edge_offset_periods"} for r in res] == ref_res
    assert res[0]["edge_offset_periods"] == 0
    for a, b in zip(words(eng), ref_w):
        assert (a == b).all()
    # on, then off: the handle as it was
    eng.set_edge_search([0, 3])
    assert eng.dwell_samples == (K * M + 3) * N
    on = eng.search(x)
    assert on[0] is not None and "edge_offset_periods" in on[0]
    eng.set_edge_search([])
    assert eng.dwell_samples == K * M * N
    assert eng.search(xs) == ref_res
    for a, b in zip(words(eng), ref_w):
        assert (a == b).all()
    eng.close()


def test_edge_entry_points_agree(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import acquisition as A, synth, tracking as T
    from gnss_sdr_rs_amd._lib import GmError
    N, K, M, fs = 8000, 4, 2, 8.0e6
    offsets, sec = [0, 3, 6], [1, -1, -1, 1]
    dop = np.array([-300.0, -100.0, 100.0, 300.0], np.float32)
    sats = [dict(prn_row=6, cn0_dbhz=46.0, doppler_hz=80.0, code_start=3001)]
    n = (K * M + 6) * N
    x = synth.to_c32(synth.make_scene(oracle.ca_code_table(), fs, 0.0, n, sats, config_id=634))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[7, 8], n_integrations=M, coherent_periods=K)
    eng.set_edge_search(offsets, sec)
    assert eng.dwell_samples == n
    with pytest.raises(GmError, match="samples_chunk shorter"):
        eng.search(x[:n - 8])
    ref = eng.search(x)
    ref_w = [a.copy() for a in eng.metrics() + eng.edge_metrics() + (eng.edge_choice(),)]
    assert ref[0] is not None and ref[0]["code_phase_samples"] == 3001 and ref[0]["edge_offset_periods"] in offsets

    def same(res, tail=0):
        assert [r and dict(r, sample_global_index=r["sample_global_index"] - tail) for r in res] == ref
        for a, b in zip(eng.metrics() + eng.edge_metrics() + (eng.edge_choice(),), ref_w):
            assert (_words(a) == _words(b)).all()

    d_x = hipbuf.upload(x)
    for deferred in (False, True):
        eng.set_deferred_decision(deferred)        # (accepted; a coherent handle decides at once)
        eng.search_dev(d_x, 0)
        eng.decide_dev()
        same(eng.fetch_results())
        tok = eng.prepare_dev(d_x, 0)
        eng.search_prepared_dev(tok)
        eng.decide_dev()
        same(eng.fetch_results())
    eng.set_deferred_decision(False)
    # a preparation does not survive a change of the edge search
    tok = eng.prepare_dev(d_x, 0)
    eng.set_edge_search(offsets, sec)
    with pytest.raises(GmError):
        eng.search_prepared_dev(tok)
    # the ring: the dwell wraps the ring's end
    size = 1 << 17
    ring = T.MulticastRingBuffer(size)
    lead = size - 5000
    ring.write_samples(np.zeros(lead, np.complex64))
    ring.write_samples(x)
    res, tail = eng.search_ring(ring)
    assert tail == lead + n - eng.dwell_samples == lead and (lead % size) + n > size
    same(res, tail)
    ring.close()
    # fine Doppler from the winning hypothesis's offset on
    res = eng.search(x)
    o = res[0]["edge_offset_periods"]
    fine = eng.finer_doppler(res)
    want = oracle.finer_doppler(x[o * N:o * N + K * M * N], res[0]["code_phase_samples"], oracle.ca_code_table()[6], fs, (K * M - 1) * N)
    assert fine[0]["fft_size"] == want["fft_size"] and fine[0]["peak_index"] == want["peak_index"], (fine[0], want)
    eng.close()


# ---- what the search buys -----------------------------------------------------------------------------------------------------
BUY = dict(N=8000, fs=8.0e6, K=20, M=2, true_dop=1206.0, code_start=2345, row=11, prn=12)
BUY_DOP = (np.arange(-250.0, 251.0, 25.0) + 1200.0).astype(np.float32)
BUY_OFFSETS = list(range(20))
GPS_CN0, GPS_ID = 40.0, 640
SEC_CN0, SEC_ID = 38.0, 641
# the CPU restatement's own gain on this seed is 53.33 / 15.92 = 5.25 dB; the asserted factor is half of it in dB: 10 ** (5.25 / 20)
SEC_FACTOR = 1.83
NOISE_ID = 642


def _buy_threshold(A):
    return A.detection_threshold(2, 8000 * 21 * 20, 1e-6)


def _gps_scene(synth, table, sat=True, config_id=GPS_ID):
    n = (BUY["K"] * BUY["M"] + 19) * BUY["N"]
    sats = [dict(prn_row=BUY["row"], cn0_dbhz=GPS_CN0, doppler_hz=BUY["true_dop"], code_start=BUY["code_start"],
                 data_bits=[1, -1], bit_edge_ms=10)] if sat else []
    return synth.to_c32(synth.make_scene(table, BUY["fs"], 0.0, n, sats, config_id=config_id))


def _sec_scene(synth, table, nh20):
    """One satellite under NH20 with alternating data: the code table's row is the tiered sequence [NH20 (x) code, -NH20 (x) code]
    (40 periods), rolled by 7 periods — make_scene indexes chip % row length"""
    n = (BUY["K"] * BUY["M"] + 19) * BUY["N"]
    code = table[BUY["row"]].astype(np.int8)
    tier = np.concatenate([np.kron(nh20, code), -np.kron(nh20, code)]).astype(np.int8)
    tier = np.roll(tier, 7 * code.size)[None, :]
    sats = [dict(prn_row=0, cn0_dbhz=SEC_CN0, doppler_hz=BUY["true_dop"], code_start=BUY["code_start"])]
    return synth.to_c32(synth.make_scene(tier, BUY["fs"], 0.0, n, sats, config_id=SEC_ID))


def _ratios(mx, sm, N):
    return mx / ((sm - mx) / np.float32(N - 1))


def test_edge_search_finds_the_gps_bit_edge(gpu, oracle):
    """40 dB-Hz, 50 bit/s data [1, -1] with the bit edge ten periods into the dwell; K = 20, M = 2, 21 bins at 25 Hz, offsets 0..19,
    best bin, threshold detection_threshold(2, 8000*21*20, 1e-6) = 16.18.
    CPU restatement (numpy fold + oracle) on this seed: the strongest cell is offset 10, bin 1200 Hz, code phase 2345, ratio 142.3
    (8.8 x the threshold; 97.1 at 38 dB-Hz); the neighbouring offsets 9 and 11 reach 122.6 and 125.4.  The plain coherent search of the
    first 40 periods peaks in bin 1175 Hz at ratio 92.1.  The noise-only scene's strongest cell has ratio 9.0."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    x = _gps_scene(synth, oracle.ca_code_table())
    eng = A.AcquisitionEngine(BUY["fs"], 0.0, BUY["N"], doppler_hz=BUY_DOP, prn_ids=[BUY["prn"]], n_integrations=BUY["M"],
                              coherent_periods=BUY["K"], decision_mode=A.DECIDE_BEST_BIN, threshold=_buy_threshold(A))
    eng.set_edge_search(BUY_OFFSETS)
    got = eng.search(x)[0]
    assert got is not None
    assert abs(int(got["code_phase_samples"]) - BUY["code_start"]) <= 1 and abs(got["carrier_freq"] - BUY["true_dop"]) <= 12.5, got
    assert got["edge_offset_periods"] in (9, 10, 11), got
    assert eng.search(_gps_scene(synth, oracle.ca_code_table(), sat=False, config_id=NOISE_ID))[0] is None
    eng.close()


def test_edge_search_wipes_a_secondary_code(gpu, oracle):
    """38 dB-Hz under NH20 aligned at period 7 with alternating data, same grid and threshold (16.18), the NH20 row.
    CPU restatement (numpy fold + oracle) on this seed: the strongest cell is offset 7, bin 1200 Hz, code phase 2345, ratio 53.3
    (3.3 x the threshold; 78.8 at 40 dB-Hz, 43.5 at 37); the other nineteen offsets stay at 7.1 .. 18.3.  The plain coherent search of
    the first 40 periods has its strongest cell in bin 1425 Hz, 219 Hz from the true carrier (at 37, 38 and 40 dB-Hz alike), at ratio
    15.9: a gain of 5.25 dB, of which the test asserts half (SEC_FACTOR = 1.83).  The noise-only scene under the row stays at 8.5."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, K, M = BUY["N"], BUY["K"], BUY["M"]
    x = _sec_scene(synth, oracle.ca_code_table(), A.NH20)
    eng = A.AcquisitionEngine(BUY["fs"], 0.0, N, doppler_hz=BUY_DOP, prn_ids=[BUY["prn"]], n_integrations=M,
                              coherent_periods=K, decision_mode=A.DECIDE_BEST_BIN, threshold=_buy_threshold(A))
    # the plain coherent search of the same handle on the first K*M periods: its strongest cell is far from the true carrier
    eng.search(x[:K * M * N])
    mx, _, sm = eng.metrics()
    r_plain = _ratios(mx[0], sm[0], N)
    d_plain = int(np.argmax(mx[0]))
    assert abs(float(eng.table_freq[d_plain]) - BUY["true_dop"]) >= 100.0, (d_plain, eng.table_freq[d_plain])
    eng.set_edge_search(BUY_OFFSETS, A.NH20)
    got = eng.search(x)[0]
    assert got is not None
    assert abs(int(got["code_phase_samples"]) - BUY["code_start"]) <= 1 and abs(got["carrier_freq"] - BUY["true_dop"]) <= 12.5, got
    assert got["edge_offset_periods"] == 7, got
    fmx, _, fsm = eng.edge_metrics()
    r_best = float(_ratios(fmx[0], fsm[0], N).max())
    assert r_best >= SEC_FACTOR * float(r_plain[d_plain]), (r_best, r_plain[d_plain])
    assert eng.search(_gps_scene(synth, oracle.ca_code_table(), sat=False, config_id=NOISE_ID))[0] is None
    eng.close()
