"""The float64 model of tests/acq_model.py on the CPU: against the oracle, the plan-coverage guard of the stage-F variant cases, and
the scenes those cases run on.

(a) validates the model here, without a GPU: on what the oracle computes (an f32 FFT pipeline) the model's arg-max is the oracle's
and max and sum agree within REL = 1e-5.  (b) walks gm_acq_plan_info over every fft_size and demands one row of acq_model.CASES per
(form, base) pair it can return: a plan added later fails here until tests/test_gpu_stage_f_variants.py launches it.  (c) makes the
GPU test's demand of an exact arg-max in every cell sound: in every cell of every variant the model alone finds the simulated code
phase, with the second-largest lag at least GAP = 1e-3 below the largest — a hundred times what REL lets an FFT's rounding move."""
import numpy as np
import pytest

import acq_model as AM

REL = AM.REL
DOP = AM.DOP


def _tables(oracle, fs, N, f_if=0.0):
    return [oracle.DopplerShiftTable(f_if, float(d), fs, N) for d in DOP]


def _close(model, got, what):
    assert np.allclose(got, model, rtol=REL, atol=0.0), (what, got, model, np.max(np.abs(got / model - 1.0)))


# ---- (a) the model against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,fmt", [(2048, "i8"), (2048, "real"), (3064, "c32")])
def test_model_matches_the_oracle_on_a_plain_search(oracle, N, fmt):
    from gnss_sdr_rs_amd import synth
    fs, M, prn_ids = N * 1000.0, 3, (5, 6)
    sats = [dict(prn_row=4, cn0_dbhz=50.0, doppler_hz=130.0, code_start=N - 91),
            dict(prn_row=5, cn0_dbhz=47.0, doppler_hz=-170.0, code_start=(3 * N) // 7)]
    x = AM.convert(synth.make_scene(oracle.ca_code_table(), fs, 0.0, M * N, sats, config_id=880), fmt)
    tables = _tables(oracle, fs, N)
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    codes = np.stack([oracle.generate_ca_code_samples(p, 1.023e6, fs) for p in prn_ids])
    assert codes.shape == (2, N)
    mx, am, sm = AM.search_model(x, np.stack([t.table for t in tables]), codes, N, 1, M, tf, fs)
    assert mx.shape == am.shape == sm.shape == (2, 1, 3)
    xc = AM.as_c128(x).astype(np.complex64)
    for w, prn in enumerate(prn_ids):
        _, (bmax, barg, bsum, done) = oracle.AcquisitionWorker(prn, N, fs).search_satellite(xc, tables, 0, M, want_planes=True,
                                                                                           no_early_exit=True)
        assert done == 3 and (barg == am[w, 0]).all(), (N, w, barg, am[w, 0])
        assert int(barg[1]) == sats[w]["code_start"]
        _close(mx[w, 0], bmax, ("max", N, w))
        _close(sm[w, 0], bsum, ("sum", N, w))


@pytest.mark.parametrize("N,with_row", [(2048, False), (3064, True)])
def test_model_matches_the_oracle_on_the_host_fold_from_per_bin_starts(oracle, N, with_row):
    """K = 3, M = 2, offsets [0, 2], T_d = N - 0.4 + 0.3 d, the replica at the scene's chip rate (a custom code, as the variant cases
    use it): the host's float32 fold (acq_model.fold, with float32 roundings of the model's own phasors) through the oracle, one table
    at a time, against the model on the raw samples."""
    from gnss_sdr_rs_amd import synth
    from test_gpu_code_drift import _fold as existing_fold
    fs, K, M, offsets = N * 1000.0, 3, 2, [0, 2]
    sec = np.array([1, -1, -1], np.int8) if with_row else None
    T = N - 0.4 + 0.3 * np.arange(3)
    starts = AM.drift_starts(T, K * M + 2)
    assert not (starts[0] == starts[2]).all()
    chips = AM.case_chips(oracle.ca_code_table(), N)
    rate = fs * 1023.0 / float(T[1])
    sats = [dict(prn_row=0, cn0_dbhz=52.0, doppler_hz=130.0, code_start=N - 91),
            dict(prn_row=1, cn0_dbhz=50.0, doppler_hz=-170.0, code_start=(3 * N) // 7)]
    x = AM.convert(synth.make_scene(chips, fs, 0.0, int(starts[:, -1].max()) + N, sats, config_id=881, code_rate=rate), "i8")
    tables = _tables(oracle, fs, N)
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    codes = AM.sample_codes(chips, rate, fs, N)
    mx, am, sm = AM.search_model(x, np.stack([t.table for t in tables]), codes, N, K, M, tf, fs, starts, offsets, sec)
    workers = [oracle.AcquisitionWorker(AM.PRN_IDS[w], N, fs, code=chips[w], code_rate=rate) for w in range(2)]
    for h, o in enumerate(offsets):
        rho = AM.phasors_f64(tf, fs, starts, K, M, o).astype(np.complex64)
        for d in range(3):
            y = AM.fold(x, N, K, M, rho[d], starts[d], o, sec)
            assert (y.view(np.uint32) == existing_fold(x, N, K, M, rho[d], starts[d], o, sec).view(np.uint32)).all()
            y = y.reshape(-1)
            for w, ow in enumerate(workers):
                _, (bmax, barg, bsum, _) = ow.search_satellite(y, [tables[d]], 0, M, want_planes=True, no_early_exit=True)
                assert barg[0] == am[w, h, d], (N, w, h, d, barg, am[w, h, d])
                _close(mx[w, h, d], bmax[0], ("max", N, w, h, d))
                _close(sm[w, h, d], bsum[0], ("sum", N, w, h, d))


# ---- (b) every plan the planner can return has a row --------------------------------------------------------------------------------
def test_every_form_and_base_of_the_planner_has_a_case(gm):
    from gnss_sdr_rs_amd import acquisition as A
    seen = set()
    for any_length in (False, True):
        for n in range(8, (1 << 18) + 1, 8):
            st, info = A.plan_info(n, any_length)
            if st == 0:
                seen.add((info["form"], info["base"]))
    rows = [(form, base) for _, form, base in AM.CASES]
    assert len(set(rows)) == len(rows) == len(AM.CASES)
    assert seen == set(rows), (sorted(seen - set(rows)), sorted(set(rows) - seen))
    for N, form, base in AM.CASES:         # and every row is what it says
        st, info = A.plan_info(N, form.startswith("long"))
        assert st == 0 and (info["form"], info["base"]) == (form, base), (N, form, base, info)
        if form == "lds":
            assert base == N
    assert set(AM.STRICT_ROWS) <= set(n for n, _, _ in AM.CASES)
    assert sorted(form for n, form, _ in AM.CASES if n in AM.STRICT_ROWS) == ["composite", "lds", "long", "long_padded"]
    # each form sees each sample format under each variant
    for v in range(len(AM.VARIANTS)):
        for form in ("lds", "composite", "long", "long_padded"):
            fmts = set(AM.FORMATS[(AM.VARIANTS[v][6] + i) % 3] for i, (_, f, _) in enumerate(AM.CASES) if f == form)
            assert fmts == set(AM.FORMATS), (v, form, fmts)


# ---- (c) the scenes: a clean peak in every cell -------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", range(len(AM.CASES)), ids=["%d-%s" % (n, f) for n, f, _ in AM.CASES])
def test_every_cell_of_every_variant_has_a_clean_peak(oracle, row):
    N = AM.CASES[row][0]
    tables = _tables(oracle, N * 1000.0, N)
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    assert (tf == DOP).all()
    tab = np.stack([t.table for t in tables])
    for v in range(len(AM.VARIANTS)):
        c = AM.build_case(oracle.ca_code_table(), N, v, row)
        assert len(c["x"]) == c["dwell"]
        mx, am, sm, gap = AM.search_model(c["x"], tab, c["codes"], N, c["K"], c["M"], tf, c["fs"], c["starts"], c["offsets"], c["sec"],
                                          with_gap=True)
        lo, hi = c["expect"][..., 0], c["expect"][..., 1]
        if c["T"] is None:
            assert (lo == hi).all()        # without the compensation: the simulated code phase itself
        assert ((am >= lo) & (am <= hi)).all(), (N, c["name"], am, lo, hi)
        assert (gap >= AM.GAP).all(), (N, c["name"], gap)
