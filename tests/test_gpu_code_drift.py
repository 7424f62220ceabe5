"""Code-drift compensation of acquisition (gm_acq_set_code_drift, DriftLoad in acq_stage_f_variants.h) on the GPU.

Period p of the dwell starts at s[d][p] = floor(p T_d + 0.5) in bin d.  Off, and T = fft_size, are the handle as it was, word for
word.  At K = 1 bin d's words are those of a plain search of the gathered samples x'[m N + n] = x[s[d][m] + n].  At K >= 2 (with
the edge search or without) the host restates the fold in float32 with the handle's own phasor words and starts and sends the folded
groups through the unchanged oracle.  Then: the phasor words, every entry point, the composition order with the edge search, and what
the compensation buys at the reference's sample rate.

Dwell lengths: the K = 1 cases run M = 16 periods.  At 0.4 samples per period the starts of a dwell of one or two periods are p N, the
plain search's own, and bins 0.01 samples apart first differ in period 14: a shorter dwell would check nothing here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-5          # the project's bound on max and sum against the oracle
L1 = 1575.42e6


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


def _fold(x, N, K, M, rho_dm, starts_d, offset=0, sec=None):
    """[M][N] complex64 folded groups: period k of group m is the N samples from starts_d[offset + m K + k] on, with
    sec[k] * rho_dm[m][k] as the phasor words — float32 with the device's arithmetic (separate real arrays, no fused operations; a
    copy of test_gpu_edge_search.py's _fold with per-period starts)"""
    xr, xi = _as_c64(x)
    s = np.ones(K, np.float32) if sec is None else np.asarray(sec, np.float32)
    y = np.empty((M, N), np.complex64)
    for m in range(M):
        st = [int(v) for v in starts_d[offset + m * K:offset + (m + 1) * K]]
        rr, ri = s * rho_dm[m].real.astype(np.float32), s * rho_dm[m].imag.astype(np.float32)
        gr, gi = xr[st[0]:st[0] + N], xi[st[0]:st[0] + N]
        are = rr[0] * gr - ri[0] * gi
        aim = rr[0] * gi + ri[0] * gr
        for k in range(1, K):
            gr, gi = xr[st[k]:st[k] + N], xi[st[k]:st[k] + N]
            are = are + (rr[k] * gr - ri[k] * gi)
            aim = aim + (rr[k] * gi + ri[k] * gr)
        y[m].real, y[m].imag = are, aim
    return y


def _gather(x, N, M, starts_d):
    """x'[m N + n] = x[s[d][m] + n]"""
    return np.concatenate([x[int(s):int(s) + N] for s in starts_d[:M]])


def _reduce(fmx, fam, fsm):
    ch = np.argmax(fmx, axis=1).astype(np.uint32)
    pick = lambda a: np.take_along_axis(a, ch[:, None, :].astype(np.int64), axis=1)[:, 0, :]
    return pick(fmx), pick(fam), pick(fsm), ch


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _all_words(eng, edge=False):
    out = [_words(a).copy() for a in eng.metrics()]
    if edge:
        out += [_words(a).copy() for a in eng.edge_metrics()] + [eng.edge_choice().copy()]
    return out


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and (u == v).all()


def _scene(synth, table, fs, f_if, n, fmt, config_id, sats, rate=1.023e6):
    x = synth.make_scene(table, fs, f_if, n, sats, config_id=config_id, code_rate=rate, real_only=fmt == "real")
    return {"i8": synth.to_i8_iq, "c32": synth.to_c32, "real": synth.to_i8_real}[fmt](x)


def _geometry(N):
    return (16.3676e6, 4.1304e6) if N == 16368 else (N * 1000.0, 0.0)


def _numpy_starts(T, R):
    t = np.asarray(T, np.float64).reshape(-1)
    return np.floor(np.arange(R, dtype=np.float64)[None, :] * t[:, None] + 0.5).astype(np.uint64)


DOP = np.array([-300.0, 0.0, 300.0], np.float32)


# ---- 1. off is today, and T = N is today ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("N", [8000, 16368])
def test_off_and_a_period_of_fft_size_are_todays_handle(gpu, oracle, N, K):
    from gnss_sdr_rs_amd import acquisition as A, synth
    from gnss_sdr_rs_amd._lib import GmError
    M = 2
    fs, f_if = _geometry(N)
    fmt = "real" if N == 16368 else "i8"
    offsets = [0, 2]
    sats = [dict(prn_row=4, cn0_dbhz=48.0, doppler_hz=20.0, code_start=N // 3)]
    x = _scene(synth, oracle.ca_code_table(), fs, f_if, (K * M + 2) * N, fmt, 660 + K, sats)
    xs = x[:K * M * N]
    kw = dict(doppler_hz=DOP, prn_ids=[5, 6], n_integrations=M, coherent_periods=K)
    ref = A.AcquisitionEngine(fs, f_if, N, **kw)              # never sees set_code_drift
    ref_res, ref_w = ref.search(xs), _all_words(ref)
    assert ref_res[0] is not None and abs(int(ref_res[0]["code_phase_samples"]) - N // 3) <= 2
    assert ref.dwell_samples == K * M * N
    with pytest.raises(GmError):
        ref.code_drift_starts()
    if K > 1:
        ref.set_edge_search(offsets)
        ref_eres, ref_ew = ref.search(x), _all_words(ref, edge=True)
    ref.close()
    eng = A.AcquisitionEngine(fs, f_if, N, **kw)
    for T in (None, float(N), N - 0.4, None):                  # off; fft_size itself; on and off again: the handle as it was
        eng.set_code_drift(T)
        if T == N - 0.4:
            assert eng.dwell_samples == int(np.floor((K * M - 1) * T + 0.5)) + N
            continue
        assert eng.dwell_samples == K * M * N
        assert eng.search(xs) == ref_res
        _same(_all_words(eng), ref_w)
        if T is not None:
            assert (eng.code_drift_starts() == (np.arange(K * M, dtype=np.uint64) * np.uint64(N))[None, :]).all()
            assert (_words(eng.code_drift_phasors()) == _words(np.broadcast_to(eng.coherent_phasors()[:, None, :], (3, M, K)))).all()
    if K > 1:
        for T in (None, float(N)):
            eng.set_code_drift(T)
            eng.set_edge_search(offsets)
            assert eng.dwell_samples == (K * M + 2) * N
            assert eng.search(x) == ref_eres
            _same(_all_words(eng, edge=True), ref_ew)
            eng.set_edge_search([])
    eng.close()


# ---- 2. K = 1, word for word ---------------------------------------------------------------------------------------------------
# (N, fmt, form, base period offset, strict_sum_order)
K1_CASES = [(2048, "c32", "lds", -0.4, False), (2048, "i8", "lds", -0.4, True),
            (16368, "real", "lds", -0.4, False),
            (18000, "i8", "composite", -0.4, False),
            (6144, "i8", "long", -0.4, False), (6144, "c32", "long", 0.3, False), (6144, "real", "long", -0.4, True),
            (4088, "c32", "long_padded", -0.4, False)]


@pytest.mark.parametrize("N,fmt,form,dT,strict", K1_CASES)
def test_k1_is_a_plain_search_of_the_gathered_samples(gpu, oracle, N, fmt, form, dT, strict):
    """T_d = N + dT + 0.01 d: bin d's three words equal, word for word, bin d's words of a plain search of x' on a second handle (a
    cell's words do not depend on what shares the launch)."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    from gnss_sdr_rs_amd._lib import GmError
    M = 16
    fs, f_if = _geometry(N)
    T = N + dT + 0.01 * np.arange(3)
    starts = _numpy_starts(T, M)
    dwell = int(starts[:, -1].max()) + N
    assert (dwell > M * N) == (dT > 0) and not (starts[0] == starts[2]).all()
    sats = [dict(prn_row=4, cn0_dbhz=47.0, doppler_hz=40.0, code_start=N // 3 + 0.3)]
    x = _scene(synth, oracle.ca_code_table(), fs, f_if, max(dwell, M * N), fmt, 670, sats)
    kw = dict(doppler_hz=DOP, prn_ids=[5, 6], n_integrations=M, any_length=form.startswith("long"), strict_sum_order=strict)
    eng = A.AcquisitionEngine(fs, f_if, N, **kw)
    plain = A.AcquisitionEngine(fs, f_if, N, **kw)
    assert eng.plan_info()["form"] == form
    eng.set_code_drift(T)
    assert eng.dwell_samples == dwell and (eng.code_drift_starts() == starts).all()
    assert (eng.code_drift_phasors() == np.complex64(1.0)).all()
    with pytest.raises(GmError, match="samples_chunk shorter"):
        eng.search(x[:dwell - 1])
    got = eng.search(x[:dwell])
    # (sanity only: the scene's own period is N samples except at 16368, so reading period p from s[d][p] moves its code by
    #  p N - s[d][p] samples and the peak lies somewhere along that slide)
    slide = np.arange(M, dtype=np.int64) * N - starts[0].astype(np.int64)
    cp = int(got[0]["code_phase_samples"]) if got[0] is not None else -1
    assert got[0] is not None and N // 3 + int(slide.min()) - 1 <= cp <= N // 3 + int(slide.max()) + 2, got[0]
    mx, am, sm = eng.metrics()
    for d in range(3):
        plain.search(_gather(x, N, M, starts[d]))
        pmx, pam, psm = plain.metrics()
        assert (am[:, d] == pam[:, d]).all(), (N, d, am[:, d], pam[:, d])
        assert (_words(mx[:, d]) == _words(pmx[:, d])).all(), (N, d, mx[:, d], pmx[:, d])
        assert (_words(sm[:, d]) == _words(psm[:, d])).all(), (N, d, sm[:, d], psm[:, d])
    plain.close()
    eng.close()


# ---- 3. K >= 2 and the edge search against the oracle ---------------------------------------------------------------------------
def _restate(oracle, x, fs, f_if, N, K, M, dop, prn_ids, offsets, sec, eng):
    tables = [oracle.DopplerShiftTable(f_if, float(d), fs, N) for d in dop]
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    P, H, D = len(prn_ids), len(offsets), len(dop)
    starts = eng.code_drift_starts()
    emax, earg, esum = (np.zeros((P, H, D), t) for t in (np.float32, np.uint32, np.float32))
    workers = [oracle.AcquisitionWorker(prn, N, fs) for prn in prn_ids]
    for h, o in enumerate(offsets):
        rho = eng.code_drift_phasors(h)
        for d in range(D):
            y = _fold(x, N, K, M, rho[d], starts[d], int(o), sec).reshape(-1)
            for w, ow in enumerate(workers):
                _, (bmax, barg, bsum, _) = ow.search_satellite(y, [tables[d]], 0, M, want_planes=True, no_early_exit=True)
                emax[w, h, d], earg[w, h, d], esum[w, h, d] = bmax[0], barg[0], bsum[0]
    return emax, earg, esum, tf


# (N, K, M, fmt, form, offsets, secondary row)
ORACLE_CASES = [(8000, 5, 2, "i8", "lds", None, False), (8000, 5, 2, "i8", "lds", [0, 2, 5], False), (8000, 5, 2, "i8", "lds", [0, 2, 5], True),
                (16368, 5, 1, "real", "lds", None, False),
                (32000, 2, 2, "i8", "composite", None, False), (18000, 2, 2, "c32", "composite", [1, 3], True),
                (6144, 3, 2, "c32", "long", None, False), (6144, 3, 2, "i8", "long", [0, 4], True)]


@pytest.mark.parametrize("N,K,M,fmt,form,offsets,with_row", ORACLE_CASES)
def test_fold_from_the_real_starts_against_the_oracle(gpu, oracle, N, K, M, fmt, form, offsets, with_row):
    """T_d = N - 0.4 + 0.3 d (the bins' starts differ and the last bin's dwell grows).  Arg-max words equal, max and sum within 1e-5
    relative of the oracle on the host's float32 fold; with offsets the reduction word for word against numpy on the device's block."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    fs, f_if = _geometry(N)
    prn_ids = [5, 6]
    T = N - 0.4 + 0.3 * np.arange(3)
    o_max = offsets[-1] if offsets else 0
    R = K * M + o_max
    starts = _numpy_starts(T, R)
    dwell = int(starts[:, -1].max()) + N
    sats = [dict(prn_row=4, cn0_dbhz=46.0, doppler_hz=90.0, code_start=N - 91.0)]
    x = _scene(synth, oracle.ca_code_table(), fs, f_if, dwell, fmt, 680 + K, sats)
    sec = np.where(np.random.default_rng(N + K).integers(0, 2, K) > 0, 1, -1).astype(np.int8) if with_row else None
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=DOP, prn_ids=prn_ids, n_integrations=M, coherent_periods=K,
                              any_length=form.startswith("long"))
    assert eng.plan_info()["form"] == form
    if offsets:
        eng.set_edge_search(offsets, sec)
    eng.set_code_drift(T)
    assert eng.dwell_samples == dwell and (eng.code_drift_starts() == starts).all()
    got = eng.search(x)
    emax, earg, esum, tf = _restate(oracle, x, fs, f_if, N, K, M, DOP, prn_ids, offsets or [0], sec, eng)
    assert (tf == eng.table_freq).all()
    mx, am, sm = eng.metrics()
    if offsets:
        fmx, fam, fsm = eng.edge_metrics()
    else:
        fmx, fam, fsm = mx[:, None, :], am[:, None, :], sm[:, None, :]
    assert (fam == earg).all(), (N, K, fam, earg)
    assert np.allclose(fmx, emax, rtol=REL, atol=0.0), (N, K, fmx, emax)
    assert np.allclose(fsm, esum, rtol=REL, atol=0.0), (N, K, fsm, esum)
    rmx, ram, rsm, ch = _reduce(fmx, fam, fsm)
    if offsets:     # the reduction, word for word on the device's own block
        assert (_words(mx) == _words(rmx)).all() and (am == ram).all() and (_words(sm) == _words(rsm)).all()
        assert (eng.edge_choice() == ch).all()
    for w, prn in enumerate(prn_ids):
        exp = oracle.decide_from_metrics(rmx[w], ram[w], rsm[w], tf, N, prn, fs, 0, 7.0)
        assert (got[w] is None) == (exp is None), (N, K, w, got[w], exp)
        if exp:
            for k in ("prn", "code_phase_samples", "carrier_freq"):
                assert got[w][k] == exp[k], (N, K, w, k, got[w], exp)
    eng.close()


# ---- 4. the phasor words -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(8000, 5), (16368, 20), (8000, 1)])
def test_phasor_words(gpu, N, K):
    from gnss_sdr_rs_amd import acquisition as A
    fs, f_if = _geometry(N)
    M, offsets = 2, [0, 3]
    dop = np.arange(-1000.0, 1001.0, 500.0, dtype=np.float32)
    T = A.code_period_samples(fs, 1023, 1.023e6, dop, L1) if N == 8000 else np.full(dop.size, 16367.6)
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=[1], n_integrations=M, coherent_periods=K)
    if K > 1:
        eng.set_edge_search(offsets)
    else:
        offsets = [0]
    eng.set_code_drift(T)
    starts = eng.code_drift_starts()
    assert (starts == _numpy_starts(T, K * M + offsets[-1])).all()
    for h, o in enumerate(offsets):
        rho = eng.code_drift_phasors(h)
        assert rho.shape == (dop.size, M, K)
        s = starts[:, o:o + K * M].reshape(dop.size, M, K)
        delta = (s - s[:, :, :1]).astype(np.float64)
        cyc = eng.table_freq.astype(np.float64)[:, None, None] * delta / np.float64(fs)
        ang = 2.0 * np.pi * (cyc - np.floor(cyc))
        want = (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)
        if K == 1:
            assert (rho == np.complex64(1.0)).all() and not np.signbit(rho.imag).any()
        for part in ("real", "imag"):
            g, w = getattr(rho, part), getattr(want, part)
            assert (np.abs(g - w) <= np.spacing(np.maximum(np.abs(g), np.abs(w)))).all(), (part, h, g, w)
    eng.close()


# ---- 5. entry points agree ------------------------------------------------------------------------------------------------------
def test_entry_points_agree(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import acquisition as A, synth, tracking as T
    from gnss_sdr_rs_amd._lib import GmError
    N, K, M, fs = 8000, 1, 16, 8.0e6
    Td = N - 0.4 + 0.01 * np.arange(3)
    sats = [dict(prn_row=6, cn0_dbhz=46.0, doppler_hz=-280.0, code_start=3000.3)]
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=DOP, prn_ids=[7, 8], n_integrations=M, coherent_periods=K)
    # the argument rules leave the handle as it was
    for bad in ([N + 8.5] * 3, [float("nan")] * 3, [float(N)] * 2):
        with pytest.raises(GmError):
            eng.set_code_drift(np.array(bad))
        assert eng.dwell_samples == M * N
    eng.set_code_drift(Td)
    n = eng.dwell_samples
    assert n == int(np.floor(15 * Td[2] + 0.5)) + N < M * N
    with pytest.raises(GmError):
        eng.set_code_drift([N + 8.5] * 3)
    assert eng.dwell_samples == n and (eng.code_drift_starts() == _numpy_starts(Td, M)).all()
    x = _scene(synth, oracle.ca_code_table(), fs, 0.0, n, "c32", 690, sats)
    with pytest.raises(GmError, match="samples_chunk shorter"):
        eng.search(x[:n - 1])
    ref = eng.search(x)
    ref_w = _all_words(eng)
    # (sanity only: this scene's own period is N samples, so the starts slide its code by up to 6 samples over the 16 periods)
    assert ref[0] is not None and 3000 <= int(ref[0]["code_phase_samples"]) <= 3008, ref[0]

    def same(res, tail=0):
        assert [r and dict(r, sample_global_index=r["sample_global_index"] - tail) for r in res] == ref
        _same(_all_words(eng), ref_w)

    d_x = hipbuf.upload(x)
    for deferred in (False, True):
        eng.set_deferred_decision(deferred)        # (accepted; a drift handle decides at once)
        eng.search_dev(d_x, 0)
        eng.decide_dev()
        same(eng.fetch_results())
        tok = eng.prepare_dev(d_x, 0)
        eng.search_prepared_dev(tok)
        eng.decide_dev()
        same(eng.fetch_results())
    eng.set_deferred_decision(False)
    # a preparation does not survive a change of the compensation
    tok = eng.prepare_dev(d_x, 0)
    eng.set_code_drift(Td)
    with pytest.raises(GmError):
        eng.search_prepared_dev(tok)
    # the ring: too few samples yet, then the dwell wraps the ring's end
    size = 1 << 18
    ring = T.MulticastRingBuffer(size)
    ring.write_samples(np.zeros(n - 1, np.complex64))
    assert eng.search_ring(ring) == (None, None)
    lead = size - 5000
    ring.write_samples(np.zeros(lead - (n - 1), np.complex64))
    ring.write_samples(x)
    res, tail = eng.search_ring(ring)
    assert tail == lead and (lead % size) + n > size
    same(res, tail)
    ring.close()
    eng.close()


# ---- 6. what it buys ------------------------------------------------------------------------------------------------------------
BUY = dict(fs=16.3676e6, f_if=4.1304e6, N=16368, K=20, M=4, dop=1000.0, code_start=3000.3, row=11, prn=12, cn0=34.0, config_id=651)


def test_the_compensation_keeps_the_peak_at_the_reference_sample_rate(gpu, oracle):
    """fs = 16.3676 MHz, N = 16368, real int8, one satellite at 34 dB-Hz, code_start 3000.3, Doppler 1000 Hz on the middle of three bins
    25 Hz apart; K = 20, M = 4 (80 periods: the code slides 32 samples against the replica), T = 16367.6.
    CPU restatement (numpy float32 fold + the oracle on host-gathered samples) on this seed: the plain coherent search peaks at code
    phase 2983 with peak-to-mean 18.6, the search from the real starts at 3001 with 45.1 (seeds 650..653: 16.6 .. 19.7 at 2977 .. 2992
    against 43.8 .. 51.7 at 3000 .. 3001)."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    fs, f_if, N, K, M = BUY["fs"], BUY["f_if"], BUY["N"], BUY["K"], BUY["M"]
    T = A.code_period_samples(fs, 1023, 1.023e6)
    assert T == fs * 1023 / 1.023e6 and abs(T - 16367.6) < 1e-6
    dop = np.array([BUY["dop"] - 25.0, BUY["dop"], BUY["dop"] + 25.0], np.float32)
    sats = [dict(prn_row=BUY["row"], cn0_dbhz=BUY["cn0"], doppler_hz=BUY["dop"], code_start=BUY["code_start"])]
    x = synth.to_i8_real(synth.make_scene(oracle.ca_code_table(), fs, f_if, K * M * N, sats, config_id=BUY["config_id"], real_only=True))
    eng = A.AcquisitionEngine(fs, f_if, N, doppler_hz=dop, prn_ids=[BUY["prn"]], n_integrations=M, coherent_periods=K,
                              decision_mode=A.DECIDE_BEST_BIN, threshold=A.detection_threshold(M, N * 3, 1e-6))

    def best(samples):
        res = eng.search(samples)[0]
        mx, am, sm = eng.metrics()
        d = int(np.argmax(mx[0]))
        return res, int(am[0, d]), float(mx[0, d] / ((sm[0, d] - mx[0, d]) / np.float32(N - 1)))

    _, cp_plain, r_plain = best(x)
    assert abs(cp_plain - 3001) >= 8, (cp_plain, r_plain)
    eng.set_code_drift(T)
    assert eng.dwell_samples == int(np.floor(79 * T + 0.5)) + N <= K * M * N
    res, cp, r = best(x[:eng.dwell_samples])
    assert abs(cp - 3001) <= 1 and r > r_plain, (cp, r, cp_plain, r_plain)
    assert res is not None and abs(int(res["code_phase_samples"]) - 3001) <= 1 and abs(res["carrier_freq"] - (f_if + BUY["dop"])) <= 12.5, res
    eng.close()


# ---- 7. composition order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8000, 32000, 6144])
def test_composition_order_does_not_matter(gpu, oracle, N):
    from gnss_sdr_rs_amd import acquisition as A, synth
    K, M = 3, 2
    fs, f_if = _geometry(N)
    offsets, sec = [0, 1, 4], [1, -1, -1]
    T = N - 0.4 + 0.3 * np.arange(3)
    dwell = int(_numpy_starts(T, K * M + 4)[:, -1].max()) + N
    sats = [dict(prn_row=4, cn0_dbhz=46.0, doppler_hz=90.0, code_start=N // 5)]
    x = _scene(synth, oracle.ca_code_table(), fs, f_if, dwell, "i8", 700, sats)
    kw = dict(doppler_hz=DOP, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, any_length=N == 6144)
    a = A.AcquisitionEngine(fs, f_if, N, **kw)
    a.set_edge_search(offsets, sec)
    a.set_code_drift(T)
    b = A.AcquisitionEngine(fs, f_if, N, **kw)
    b.set_code_drift(T)
    assert b.dwell_samples == int(_numpy_starts(T, K * M)[:, -1].max()) + N
    b.set_edge_search(offsets, sec)
    assert a.dwell_samples == b.dwell_samples == dwell
    assert (a.code_drift_starts() == b.code_drift_starts()).all()
    for h in range(3):
        assert (_words(a.code_drift_phasors(h)) == _words(b.code_drift_phasors(h))).all()
    assert a.search(x) == b.search(x)
    _same(_all_words(a, edge=True), _all_words(b, edge=True))
    # the edge search off again under the compensation: the dwell is planned again
    b.set_edge_search([])
    assert b.dwell_samples == int(_numpy_starts(T, K * M)[:, -1].max()) + N and b.code_drift_starts().shape == (3, K * M)
    b.search(x)
    a.close()
    b.close()


# ---- 8. switched off under an edge search set while it was on ---------------------------------------------------------------------
@pytest.mark.parametrize("N,dT", [(8000, -0.4), (8000, -8.0), (6144, -8.0)])
def test_off_after_an_edge_search_set_under_a_short_period(gpu, oracle, N, dT):
    """Compensation with T < N, then the edge search, then the compensation off: the dwell is (K M + o_max) N again, longer than the
    compensated one, and the internal sample buffer of the host-buffer and ring entries must hold it (c32: 8 bytes a sample).  Every word
    equals those of a handle that never saw set_code_drift."""
    from gnss_sdr_rs_amd import acquisition as A, synth, tracking as T
    K, M = 3, 2
    fs, f_if = _geometry(N)
    offsets = [0, 2, 5]
    n = (K * M + 5) * N
    sats = [dict(prn_row=4, cn0_dbhz=47.0, doppler_hz=90.0, code_start=N // 5)]
    x = _scene(synth, oracle.ca_code_table(), fs, f_if, n, "c32", 720, sats)
    kw = dict(doppler_hz=DOP, prn_ids=[5, 6], n_integrations=M, coherent_periods=K, any_length=N == 6144)
    ref = A.AcquisitionEngine(fs, f_if, N, **kw)
    ref.set_edge_search(offsets)
    ref_res, ref_w = ref.search(x), _all_words(ref, edge=True)
    ref.close()
    eng = A.AcquisitionEngine(fs, f_if, N, **kw)
    eng.set_code_drift(N + dT)
    eng.set_edge_search(offsets)
    short = eng.dwell_samples
    assert short == int(np.floor((K * M + 4) * (N + dT) + 0.5)) + N < n
    eng.search(x[:short])
    eng.set_code_drift(None)
    assert eng.dwell_samples == n
    assert eng.search(x) == ref_res
    _same(_all_words(eng, edge=True), ref_w)
    # the ring entry copies the same dwell into the same buffer
    ring = T.MulticastRingBuffer(1 << 18)
    ring.write_samples(x)
    res, tail = eng.search_ring(ring)
    assert tail == 0 and res == ref_res
    _same(_all_words(eng, edge=True), ref_w)
    ring.close()
    # and the other way round: the edge search off under the compensation, then the compensation off
    eng.set_code_drift(N + dT)
    eng.set_edge_search([])
    eng.set_code_drift(None)
    assert eng.dwell_samples == K * M * N
    eng.search(x[:K * M * N])
    eng.close()
