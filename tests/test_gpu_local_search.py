"""Lag window x fine Doppler at known cells (gm_acq_local_search, csrc/acq_local.hip) on the GPU.

1. EVERY (worker, bin) cell as a candidate, centred on the search's arg-max, against the float64 model of acq_local_model.py, on
   acq_model.build_case scenes: N below one tile (256, c32, coherent), N no multiple of 256 with odd byte starts (2000, real, drift at
   K = 1, J = 3), drift + fold + edge (2048, i8), a padded-long handle (3064).  L in {0, 3, 64} at 256 and 2048, L = 3 elsewhere.
2. Against the parent's code: row l of the surface is refine_doppler(code_phase = lambda_l)'s spectrum.
3. The window wraps: centres 1 and N - 2 with L = 4, codes starting at N - 91, near 0 and near N.
4. A centre 2 samples off brings the peak back to the arg-max; a centre L + 1 off sets lag_at_edge.
5. Fresh samples: the same buffer as d_samples gives the NULL route's words; a later dwell gives the shifted code phase; the
   snapshot and the search's words stay.
6. A candidate's words depend neither on what else is in the call nor on repetition.
7. An offset that is not one of the edge search's.  8. Every error case, nothing written on an error, the no-op, a plain handle
   (2 L + 1 > N cannot be reached on a handle: the smallest fft_size a handle takes is 256 and L <= 64; the rule is the host code of
   gm_acq_local_plan, which tests/test_acq_local_host.py drives with N = 128 and N = 8).

Bounds.  REL = acq_model.REL = 1e-5.  Prompts: |z_dev - z_model| <= REL max |z_model| over the candidate's [W][R_u]; surface:
|S_dev - S_model| <= 3 REL max S_model over the candidate's [W][Z] — gm_acq_refine_doppler's bounds, for the same reasons
(test_gpu_refine_doppler.py).  The device's peak is a maximum of the model's surface to within that bound.

code_phase_fine.  It is lambda_{l*} + frac plus terms that are exact in f64, frac = n / den with n = a+ - a-, den = 2 (a0 - min(a-, a+)),
a = sqrt(S).  The surface bound e = 3 REL max S_model moves an amplitude by at most delta_i = e / a_i (|sqrt(S + e) - sqrt(S)| =
e / (sqrt(S + e) + sqrt(S))), so n moves by dn <= delta+ + delta-, den by dd <= 2 (delta0 + max(delta-, delta+)), and
    |frac_dev - frac_model| <= (dn + |n / den| dd) / (den - dd)                     (clamping to +-0.5 does not increase a difference)
which _fine_bound evaluates on the MODEL's three amplitudes for every cell.  For the ideal correlation triangle at c samples per chip
(c >= 2 here) the three points are at most 1.5 samples from the vertex: a_i >= a0 (1 - 1.5 / c) >= a0 / 4, max S = a0^2, delta_i <=
12 REL a0, den = 2 a0 / c, |n / den| <= 1/2, so the bound is (24 + 24) REL a0 / (2 a0 / c - 48 REL a0) ~ 24 REL c: 5e-4 sample at 2
samples per chip, 7e-4 at 3.  A cell whose peak is flat-topped (a bin that reads the periods a fraction of a sample apart from the
scene's) has a smaller den and so, by the same formula, a wider bound; the test prints the measured worst and the bound beside it.

Measured on an MI355X (tests 1 and 2): prompts within 5.0e-7, the surface within 8.7e-7 of the largest model value, rows within 8.2e-7 of
gm_acq_refine_doppler's; code_phase_fine within 2.6e-7 sample of the model's, against bounds of 1.4e-4 to 2.5e-4 on those cells."""
import ctypes as C
import math

import numpy as np
import pytest

import acq_local_model as LM
import acq_model as AM
import acq_refine_model as RM

pytestmark = pytest.mark.gpu
REL = AM.REL
INVALID = -1
FINE_BOUND = 0.25          # samples: tests/test_acq_local_host.py

# (fft_size, form, variant index in AM.VARIANTS, row_index -> sample format, span_periods, the L values)
CASES = [(256, "lds", 0, 2, 0, (0, 3, 64)),           # coherent, c32: N below one tile
         (2000, "lds", 3, 1, 3, (3,)),                # drift at K = 1, real, J = 3: odd byte starts, no multiple of 256
         (2048, "lds", 2, 1, 0, (0, 3, 64)),          # drift + fold + edge, i8
         (3064, "long_padded", 0, 0, 0, (3,))]        # coherent: the kernel must not care about the form
FORMATS = {256: "c32", 2000: "real", 2048: "i8"}
CELL_PARAMS = [(i, L) for i, c in enumerate(CASES) for L in c[5]]
CELL_IDS = ["%d-%s-%s-L%d" % (CASES[i][0], CASES[i][1], AM.VARIANTS[CASES[i][2]][0], L) for i, L in CELL_PARAMS]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fmt(c):
    from gnss_sdr_rs_amd import _lib
    return {"c32": _lib.FMT_C32, "i8": _lib.FMT_I8_IQ, "real": _lib.FMT_I8_REAL}[c["fmt"]]


def _engine(A, c, form, **kw):
    return A.AcquisitionEngine(c["fs"], kw.pop("f_if", 0.0), c["N"], doppler_hz=AM.DOP, prn_ids=kw.pop("prn_ids", list(AM.PRN_IDS)),
                               n_integrations=c["M"], codes=c["chips"], code_rate=c["code_rate"], coherent_periods=c["K"],
                               any_length=form.startswith("long"), **kw)


def _setup(eng, c):
    if c["offsets"]:
        eng.set_edge_search(c["offsets"], c["sec"])
    if c["T"] is not None:
        eng.set_code_drift(c["T"])
    assert eng.dwell_samples == c["dwell"] == len(c["x"])


def _searched(oracle, N, form, v, row_index):
    """-> (engine after a search of the build_case scene, scene, arg-max [P][D], chosen offsets [P][D] in periods)"""
    from gnss_sdr_rs_amd import acquisition as A
    c = AM.build_case(oracle.ca_code_table(), N, v, row_index)
    eng = _engine(A, c, form)
    assert eng.plan_info()["form"] == form
    _setup(eng, c)
    eng.search(c["x"])
    am = eng.metrics()[1]
    offs = np.asarray(c["offsets"] or [0])
    ch = eng.edge_choice() if c["offsets"] else np.zeros((AM.P, AM.D), np.uint32)
    return eng, c, am, offs[ch.astype(np.int64)]


def _cand(w, d, cp, o=0):
    return dict(worker=int(w), doppler_bin=int(d), code_phase_samples=int(cp), offset_periods=int(o))


def _model(c, tab, tf, cand, L, span=0, n_freq=0, x=None):
    w, d, o = cand["worker"], cand["doppler_bin"], cand["offset_periods"]
    p = LM.plan(c["K"], c["M"], c["fs"], c["N"], tf, d, L, span, n_freq)
    T_d = None if c["T"] is None else c["T"][d]
    r = LM.local(c["x"] if x is None else x, tab[d], c["codes"][w], c["N"], c["starts"][d], o, cand["code_phase_samples"], L, tf[d],
                 c["fs"], p["span_periods"], p["n_groups"], p["n_freq"], p["half_span_hz"], c["sec"], T_d=T_d, code_rate=c["code_rate"])
    return dict(r, plan=p, T_d=T_d)


def _fine_bound(S, l, j):
    """the docstring's bound on |frac_dev - frac_model| from the model's surface; inf where the derivation does not apply"""
    e = 3 * REL * float(S.max())
    a = [math.sqrt(float(S[l + u][j])) for u in (-1, 0, 1)]
    dl = [e / v if v > 0.0 else math.sqrt(e) for v in a]
    n, den = a[2] - a[0], 2.0 * (a[1] - min(a[0], a[2]))
    dn, dd = dl[0] + dl[2], 2.0 * (dl[1] + max(dl[0], dl[2]))
    return (dn + abs(n / den) * dd) / (den - dd) if den > dd else math.inf


def _check_against_model(tag, c, got, want, cand, L):
    """the assertions of test 1 for one candidate; -> (prompt error, surface error, fine difference, fine bound)"""
    N, p = c["N"], want["plan"]
    W, Z, R_u = 2 * L + 1, p["n_freq"], p["span_periods"] * p["n_groups"]
    assert (got["n_lags"], got["span_periods"], got["n_groups"], got["n_freq"]) == (W, p["span_periods"], p["n_groups"], Z), tag
    assert got["doppler_bin"] == cand["doppler_bin"] and got["offset_periods"] == cand["offset_periods"], (tag, got)
    assert got["step_hz"] == pytest.approx(p["step_hz"], rel=1e-6) and got["half_span_hz"] == pytest.approx(p["half_span_hz"], rel=1e-6)
    z, S = got["prompts"].astype(np.complex128), got["surface"].astype(np.float64)
    assert z.shape == (W, R_u) and S.shape == (W, Z), tag
    zerr = float(np.max(np.abs(z - want["z"])) / np.max(np.abs(want["z"])))
    serr = float(np.max(np.abs(S - want["S"])) / np.max(want["S"]))
    assert zerr <= REL, (tag, zerr)
    assert serr <= 3 * REL, (tag, serr)
    l, j = got["peak_lag_index"], got["peak_freq_index"]
    assert want["S"][l][j] >= (1.0 - 3 * REL) * want["S"].max(), tag
    # the peak, the flags, the floor and the fine code phase agree with the device's own surface
    assert (l, j) == tuple(int(v) for v in np.unravel_index(int(np.argmax(got["surface"])), (W, Z))), tag      # first in (l, j) order
    assert got["peak_power"] == got["surface"][l][j] == got["surface"].max(), tag
    assert got["freq_at_edge"] == int(j in (0, Z - 1)) and got["lag_at_edge"] == int(l in (0, W - 1)), tag
    assert got["code_phase_samples"] == int(LM.lags(cand["code_phase_samples"], L, N)[l]), tag
    fl, nf = LM.floor_of(S, l, LM.guard_lags(c["fs"], c["code_rate"]), N)
    assert got["n_floor"] == nf and got["floor_power"] == pytest.approx(fl, rel=1e-6), (tag, got["floor_power"], fl)
    if not got["freq_at_edge"]:
        _, delta, _ = RM.peak_interp(S[l], p["step_hz"])
        assert got["delta_hz"] == pytest.approx(delta, abs=1e-4 * p["step_hz"] + 1e-6 * abs(delta)), tag
    assert got["carrier_hz"] == pytest.approx(float(AM.DOP[cand["doppler_bin"]]) + got["delta_hz"], abs=1e-3), tag
    own = LM.fine_from_surface(S, l, j, cand["code_phase_samples"], L, N, c["starts"][cand["doppler_bin"]], cand["offset_periods"], R_u,
                               want["T_d"])
    assert abs(LM.circular_error(got["code_phase_fine"], own[3], N)) <= 1e-9 * N, (tag, got["code_phase_fine"], own)
    assert 0.0 <= got["code_phase_fine"] < N, tag
    # ... and the fine code phase with the model's, at the device's peak
    ref = LM.fine_from_surface(want["S"], l, j, cand["code_phase_samples"], L, N, c["starts"][cand["doppler_bin"]],
                               cand["offset_periods"], R_u, want["T_d"])
    diff, bound = 0.0, 0.0
    if not got["lag_at_edge"]:
        diff, bound = abs(LM.circular_error(got["code_phase_fine"], ref[3], N)), _fine_bound(want["S"], l, j)
        assert diff <= bound, (tag, diff, bound)
    return zerr, serr, diff, bound


_CELLS = {}


def _cells(oracle, i):
    """One search of CASES[i] and, per L, one call with every (worker, bin) cell as a candidate, with the model's values: computed
    once, shared and left unchanged."""
    if i in _CELLS:
        return _CELLS[i]
    N, form, v, row_index, span, Ls = CASES[i]
    eng, c, am, off = _searched(oracle, N, form, v, row_index)
    assert FORMATS.get(N, c["fmt"]) == c["fmt"]
    tab, tf = eng.tables(), eng.table_freq
    cands = [_cand(w, d, am[w, d], off[w, d]) for w in range(AM.P) for d in range(AM.D)]
    out = {}
    for L in Ls:
        got = eng.local_search(cands, lag_half_window=L, span_periods=span, want_prompts=True, want_surface=True)
        out[L] = [(cand, g, _model(c, tab, tf, cand, L, span)) for cand, g in zip(cands, got)]
    eng.close()
    _CELLS[i] = dict(c=c, am=am, out=out)
    return _CELLS[i]


# ---- 1. every cell against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,L", CELL_PARAMS, ids=CELL_IDS)
def test_every_cell_against_the_model(gpu, oracle, i, L):
    r = _cells(oracle, i)
    c = r["c"]
    assert int(r["am"][0].max()) > c["N"] - 100                  # worker 0's code starts at N - 91
    worst = [0.0, 0.0, 0.0, 0.0]
    for cand, got, want in r["out"][L]:
        tag = (CELL_IDS[CELL_PARAMS.index((i, L))], cand["worker"], cand["doppler_bin"])
        res = _check_against_model(tag, c, got, want, cand, L)
        print("%s: prompts %.2e, surface %.2e of the largest; peak (%d, %d) / model (%d, %d); fine %.4f, model %.4f, difference %.2e "
              "(bound %.2e)" % (tag, res[0], res[1], got["peak_lag_index"], got["peak_freq_index"], want["l"], want["j"],
                                got["code_phase_fine"], want["code_phase_fine"], res[2], res[3]))
        worst = [max(a, b) for a, b in zip(worst[:3], res[:3])] + [max(worst[3], res[3] if math.isfinite(res[3]) else 0.0)]
    print("worst: prompts %.2e (bound %.0e), surface %.2e (bound %.0e), fine code phase %.2e sample (largest finite bound %.2e)"
          % (worst[0], REL, worst[1], 3 * REL, worst[2], worst[3]))


def test_a_dwell_longer_than_the_staged_prompts(gpu, oracle):
    """K = 1, M = 1030 periods of 256 samples, span_periods = 515: R_u = 1030 prompts per lag, past the 1024 the scan kernel stages in
    LDS — it then reads them from global memory.  L = 1; same bounds against the model."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, M, J, L = 256, 1030, 515, 1
    fs = N * 1000.0
    chips = AM.case_chips(oracle.ca_code_table(), N)
    rate = 1000.0 * chips.shape[1]
    sats = [dict(prn_row=0, cn0_dbhz=44.0, doppler_hz=130.0, code_start=N - 91, phase=0.4)]
    x = AM.convert(synth.make_scene(chips, fs, 0.0, M * N, sats, config_id=930, code_rate=rate), "c32")
    c = dict(N=N, K=1, M=M, fs=fs, x=x, sec=None, T=None, starts=AM.plain_starts(AM.D, M, N), codes=AM.sample_codes(chips, rate, fs, N),
             code_rate=rate)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=M, codes=chips, code_rate=rate)
    eng.search(x)
    am = eng.metrics()[1]
    cands = [_cand(w, 1, am[w, 1]) for w in range(AM.P)]
    got = eng.local_search(cands, lag_half_window=L, span_periods=J, want_prompts=True, want_surface=True)
    tab, tf = eng.tables(), eng.table_freq
    eng.close()
    for cand, g in zip(cands, got):
        assert (g["span_periods"], g["n_groups"], g["prompts"].shape) == (J, 2, (3, 1030))
        res = _check_against_model(("long dwell", cand["worker"]), c, g, _model(c, tab, tf, cand, L, J), cand, L)
        print("worker %d: prompts %.2e, surface %.2e of the largest" % (cand["worker"], res[0], res[1]))
    assert got[0]["code_phase_samples"] == int(am[0, 1]) and abs(got[0]["carrier_hz"] - 130.0) <= 2 * got[0]["step_hz"]


# ---- 2. against the parent's code ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2], ids=["256", "2048"])
def test_rows_are_refine_dopplers_spectra(gpu, oracle, i):
    """Row l of the surface equals refine_doppler(code_phase = lambda_l)'s spectrum within 3 REL of the row's maximum (not word
    equality: the N-term sums are added in another order) — every row of every cell at L = 3, every row of bin 1 at L = 64; at
    L = 0 the carrier is within one grid step of refine_doppler's."""
    N, form, v, row_index, span, _ = CASES[i]
    eng, c, am, off = _searched(oracle, N, form, v, row_index)
    worst = 0.0
    for L, bins in ((3, range(AM.D)), (64, (1,))):
        for d in bins:
            cands = [_cand(w, d, am[w, d], off[w, d]) for w in range(AM.P)]
            got = eng.local_search(cands, lag_half_window=L, want_surface=True)
            for l in range(2 * L + 1):
                res = [dict(doppler_bin=d, code_phase_samples=int(LM.lags(am[w, d], L, N)[l])) for w in range(AM.P)]
                ref = eng.refine_doppler(res, want_spectrum=True)
                for w in range(AM.P):
                    assert ref[w]["offset_periods"] == off[w, d]
                    row, want = got[w]["surface"][l].astype(np.float64), ref[w]["spectrum"].astype(np.float64)
                    err = float(np.max(np.abs(row - want)) / want.max())
                    worst = max(worst, err)
                    assert err <= 3 * REL, (N, L, d, w, l, err)
    print("N %d: worst row difference %.2e of the row's maximum" % (N, worst))
    for d in range(AM.D):
        cands = [_cand(w, d, am[w, d], off[w, d]) for w in range(AM.P)]
        got = eng.local_search(cands)
        ref = eng.refine_doppler([dict(doppler_bin=d, code_phase_samples=int(am[w, d])) for w in range(AM.P)])
        for w in range(AM.P):
            assert got[w]["n_lags"] == 1 and got[w]["lag_at_edge"] == 1 and got[w]["code_phase_fine"] == float(am[w, d])
            assert abs(got[w]["carrier_hz"] - ref[w]["carrier_hz"]) <= ref[w]["step_hz"], (d, w)
            assert got[w]["peak_power"] == pytest.approx(ref[w]["peak_power"], rel=3 * REL)
    eng.close()


# ---- 3. the window wraps ---------------------------------------------------------------------------------------------------------
def test_the_window_wraps(gpu, oracle):
    """L = 4 around the centres 1 and N - 2: the lags run over the end of the period.  A scene of its own with one code starting at
    1 and one at N - 2 (the peaks are inside both windows), and the 2048 case, whose worker 0 starts at N - 91 (outside: the model
    still has to agree)."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, M, L = 2048, 3, 4
    fs = N * 1000.0
    chips = AM.case_chips(oracle.ca_code_table(), N)
    starts_at = (1, N - 2)
    sats = [dict(prn_row=w, cn0_dbhz=60.0, doppler_hz=AM.SAT_DOPPLER[w], code_start=starts_at[w], phase=0.4 + w) for w in range(AM.P)]
    x = AM.convert(synth.make_scene(chips, fs, 0.0, M * N, sats, config_id=941, code_rate=1.023e6), "i8")
    c = dict(N=N, K=1, M=M, fs=fs, x=x, sec=None, T=None, starts=AM.plain_starts(AM.D, M, N), codes=AM.sample_codes(chips, 1.023e6, fs, N),
             code_rate=1.023e6)
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=M, codes=chips, code_rate=1.023e6)
    eng.search(x)
    am = eng.metrics()[1]
    assert [int(am[w, 1]) for w in range(AM.P)] == list(starts_at), am
    tab, tf = eng.tables(), eng.table_freq
    cands = [_cand(w, 1, cp) for w in range(AM.P) for cp in (1, N - 2)]
    got = eng.local_search(cands, lag_half_window=L, want_prompts=True, want_surface=True)
    eng.close()
    for cand, g in zip(cands, got):
        lam = LM.lags(cand["code_phase_samples"], L, N)
        assert lam.max() > N - 7 and lam.min() < 6                                         # the window wraps
        _check_against_model(("wrap", cand["worker"], cand["code_phase_samples"]), c, g, _model(c, tab, tf, cand, L), cand, L)
        assert g["code_phase_samples"] == starts_at[cand["worker"]] and g["lag_at_edge"] == 0, (cand, g["code_phase_samples"])
        assert abs(LM.circular_error(g["code_phase_fine"], starts_at[cand["worker"]], N)) <= 0.5, g["code_phase_fine"]
    # the 2048 case (drift + fold + edge): worker 0's code starts at N - 91
    N2, form, v, row_index, span, _ = CASES[2]
    eng, c2, am2, off = _searched(oracle, N2, form, v, row_index)
    tab, tf = eng.tables(), eng.table_freq
    cands = [_cand(w, d, cp, off[w, d]) for w in range(AM.P) for d in (0, 1) for cp in (1, N2 - 2)]
    got = eng.local_search(cands, lag_half_window=L, want_prompts=True, want_surface=True)
    eng.close()
    for cand, g in zip(cands, got):
        _check_against_model(("wrap-2048", cand["worker"], cand["doppler_bin"], cand["code_phase_samples"]), c2, g,
                             _model(c2, tab, tf, cand, L), cand, L)


# ---- 4. peak recovery ------------------------------------------------------------------------------------------------------------
def test_the_peak_comes_back_to_the_arg_max(gpu, oracle):
    N, L = 2048, 3
    eng, c, am, off = _searched(oracle, N, "lds", 0, 2)           # coherent, c32, no drift: 2.002 samples a chip
    for w in range(AM.P):
        best = int(am[w, 1])
        for shift in (-2, 2):
            g = eng.local_search([_cand(w, 1, (best + shift) % N)], lag_half_window=L)[0]
            assert g["code_phase_samples"] == best and g["peak_lag_index"] == L - shift and g["lag_at_edge"] == 0, (w, shift, g)
            assert abs(LM.circular_error(g["code_phase_fine"], best, N)) <= 0.5
        for shift in (-(L + 1), L + 1):                           # the arg-max is one lag outside the window
            g = eng.local_search([_cand(w, 1, (best + shift) % N)], lag_half_window=L)[0]
            assert g["lag_at_edge"] == 1 and g["peak_lag_index"] == (2 * L if shift < 0 else 0), (w, shift, g)
            assert g["code_phase_fine"] == float(g["code_phase_samples"]) == float((best + (1 if shift > 0 else -1)) % N)
    eng.close()


# ---- 5. fresh samples ------------------------------------------------------------------------------------------------------------
def _same_entry(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and (_words(a[k]) == _words(b[k])).all(), k
        else:
            assert np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes(), (k, a[k], b[k])


def test_the_same_buffer_as_fresh_samples_gives_the_same_words(gpu, oracle, hipbuf):
    N, form, v, row_index, span, _ = CASES[1]                     # 2000, real, drift: odd byte starts on both routes
    eng, c, am, off = _searched(oracle, N, form, v, row_index)
    kw = dict(lag_half_window=5, span_periods=span, want_prompts=True, want_surface=True, n_freq=65)
    cands = [_cand(w, d, am[w, d], off[w, d]) for w in range(AM.P) for d in range(AM.D)]
    search_words = lambda: [_words(a).copy() for a in eng.metrics()]
    before = search_words()
    res = [dict(doppler_bin=1, code_phase_samples=int(am[w, 1])) for w in range(AM.P)]
    refine_before = eng.refine_doppler(res, span_periods=span, want_prompts=True, want_spectrum=True)
    null_route = eng.local_search(cands, **kw)
    d_x = hipbuf.upload(c["x"])
    fresh = eng.local_search(cands, samples=d_x, fmt=_fmt(c), **kw)
    for a, b in zip(null_route, fresh):
        _same_entry(a, b)
    # other samples at the same place in the call: other words, and the snapshot is still the search's
    d_y = hipbuf.upload(np.ascontiguousarray(c["x"][::-1]))
    other = eng.local_search(cands, samples=d_y, fmt=_fmt(c), **kw)
    assert not (_words(other[0]["prompts"]) == _words(null_route[0]["prompts"])).all()
    for a, b in zip(refine_before, eng.refine_doppler(res, span_periods=span, want_prompts=True, want_spectrum=True)):
        _same_entry(a, b)
    for a, b in zip(null_route, eng.local_search(cands, **kw)):
        _same_entry(a, b)
    for u, w_ in zip(before, search_words()):
        assert u.shape == w_.shape and (u == w_).all()
    eng.close()


@pytest.mark.parametrize("name", sorted(RM.TRUTH_SCENES))
def test_a_later_dwell_gives_the_shifted_code_phase(gpu, oracle, hipbuf, name):
    """The search runs on the truth scene's first dwell; a second dwell of the same signal, three secondary-row lengths on, is passed
    as fresh samples with the window's centre one sample off the expected code phase (code_start - s0) mod T: code_phase_fine is within
    0.25 sample of it (the bound of tests/test_acq_local_host.py), on the first dwell's snapshot within 0.25 of the code start."""
    from gnss_sdr_rs_amd import acquisition as A
    first = LM.truth_scene(oracle.ca_code_table(), name)
    later = LM.truth_scene(oracle.ca_code_table(), name, LM.later_start(first["K"]), seed_add=100)
    eng = _engine(A, first, "lds", f_if=first["f_if"], prn_ids=[RM.TRUTH_PRN], decision_mode=A.DECIDE_BEST_BIN)
    _setup(eng, first)
    res = eng.search(first["x"])
    assert res[0] is not None and res[0]["doppler_bin"] == 1, res
    d_later = hipbuf.upload(later["x"])
    for c, samples in ((first, None), (later, d_later)):
        cp = (int(round(c["code_start_here"])) + 1) % c["N"]
        g = eng.local_search([_cand(0, 1, cp, c["edge"])], samples=samples, fmt=_fmt(c), lag_half_window=5, span_periods=c["span"])[0]
        err = LM.circular_error(g["code_phase_fine"], c["code_start_here"], RM.TRUTH_T)
        print("scene %s from sample %d: fine %.3f, expected %.3f, error %+.3f; carrier error %+.2f Hz; peak / floor %.0f"
              % (name, c["s0"], g["code_phase_fine"], c["code_start_here"], err, g["carrier_hz"] - c["f_true"],
                 g["peak_power"] / g["floor_power"]))
        assert g["lag_at_edge"] == 0 and g["freq_at_edge"] == 0, g
        assert abs(err) <= FINE_BOUND, (name, c["s0"], err)
        assert abs(g["carrier_hz"] - c["f_true"]) <= RM.truth_bound(c["K"] * c["M"]) + g["step_hz"]
        assert g["n_floor"] >= 2 and g["peak_power"] > 20.0 * g["floor_power"]      # W = 11, the guard is 4 lags: lags are left on a side
    eng.close()


# ---- 6. independence and repetition -----------------------------------------------------------------------------------------------
def test_words_depend_neither_on_company_nor_on_repetition(gpu, oracle):
    N, form, v, row_index, span, _ = CASES[2]
    eng, c, am, off = _searched(oracle, N, form, v, row_index)
    kw = dict(lag_half_window=9, want_prompts=True, want_surface=True, n_freq=33)
    cands = [_cand(w, d, am[w, d], off[w, d]) for w in range(AM.P) for d in range(AM.D)]
    six = eng.local_search(cands, **kw)
    alone = eng.local_search([cands[4]], **kw)
    moved = eng.local_search(cands[::-1], **kw)
    again = eng.local_search(cands, **kw)
    _same_entry(six[4], alone[0])
    _same_entry(six[4], moved[1])
    for a, b in zip(six, again):
        _same_entry(a, b)
    assert not (_words(six[4]["prompts"]) == _words(six[3]["prompts"])).all()
    eng.close()


# ---- 7. an offset between the searched ones --------------------------------------------------------------------------------------
def test_an_offset_that_was_not_searched(gpu, oracle):
    """the edge search ran offsets (0, 2); a predicted edge at 1 is a legal candidate, and 3 is above the last"""
    from gnss_sdr_rs_amd._lib import GmError
    N, form, v, row_index, span, _ = CASES[2]
    eng, c, am, off = _searched(oracle, N, form, v, row_index)
    assert c["offsets"] == [0, 2]
    tab, tf = eng.tables(), eng.table_freq
    cands = [_cand(w, 1, am[w, 1], 1) for w in range(AM.P)]
    got = eng.local_search(cands, lag_half_window=2, want_prompts=True, want_surface=True)
    for cand, g in zip(cands, got):
        assert g["offset_periods"] == 1
        _check_against_model(("offset-1", cand["worker"]), c, g, _model(c, tab, tf, cand, 2), cand, 2)
    with pytest.raises(GmError) as e:
        eng.local_search([_cand(0, 1, 5, 3)])
    assert e.value.status == INVALID
    eng.close()


# ---- 8. errors, the no-op, a plain handle -----------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib
    N = 2048
    eng, c, am, off = _searched(oracle, N, "lds", 0, 2)           # coherent (K = 3), c32, no edge search
    d_x = hipbuf.upload(c["x"])
    ok = (0, 1, 5, 0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    W, R_u, Z = 7, c["K"] * c["M"], 257

    def call(cands, cfg=(3, 0, 0, 0.0), samples=None, fmt=0, null=None):
        cs = (_lib.AcqCand * max(len(cands), 1))(*[_lib.AcqCand(*t) for t in cands])
        out = np.full(2 * C.sizeof(_lib.AcqLocalOut), 0xAB, np.uint8)
        z = np.full(2 * 129 * R_u, np.complex64(7 + 7j))
        s = np.full(2 * 129 * Z, np.float32(7.0))
        st = _lib.lib().gm_acq_local_search(None if null == "handle" else eng._h, C.c_void_p(samples) if samples else None, fmt,
                                            None if null == "cands" else C.cast(cs, C.c_void_p), len(cands),
                                            C.byref(_lib.AcqLocalCfg(*cfg)) if cfg else None, None if null == "out" else vp(out),
                                            vp(z), vp(s))
        untouched = bool((out == 0xAB).all() and (z == np.complex64(7 + 7j)).all() and (s == 7.0).all())
        return st, untouched, out, z, s

    st, untouched, out, z, s = call([ok, ok])
    assert st == 0 and not untouched
    assert not (z[:2 * W * R_u] == np.complex64(7 + 7j)).any() and (z[2 * W * R_u:] == np.complex64(7 + 7j)).all()
    assert not (s[:2 * W * Z] == 7.0).any() and (s[2 * W * Z:] == 7.0).all()
    bad = [dict(cands=[ok], null="handle"), dict(cands=[ok], null="cands"), dict(cands=[ok], null="out"),
           dict(cands=[ok, (AM.P, 1, 5, 0)]),                                          # worker >= P
           dict(cands=[ok, (0, AM.D, 5, 0)]), dict(cands=[(0, -1, 5, 0)]),             # bin outside D
           dict(cands=[ok, (0, 1, N, 0)]),                                             # cp >= N
           dict(cands=[(0, 1, 5, 1)]),                                                 # no edge search: the offset must be 0
           dict(cands=[ok], cfg=(65, 0, 0, 0.0)),                                      # L > 64
           dict(cands=[ok], cfg=(3, 2, 0, 0.0)),                                       # K = 3: span_periods must be 0 or K
           dict(cands=[ok], cfg=(3, 0, 64, 0.0)), dict(cands=[ok], cfg=(3, 0, 1, 0.0)), dict(cands=[ok], cfg=(3, 0, 4099, 0.0)),
           dict(cands=[ok], cfg=(3, 0, 0, 501.0)), dict(cands=[ok], cfg=(3, 0, 0, -1.0)), dict(cands=[ok], cfg=(3, 0, 0, float("nan"))),
           dict(cands=[ok], samples=d_x, fmt=3), dict(cands=[ok], samples=d_x, fmt=-1)]         # not a format
    for kw in bad:
        st, untouched, *_ = call(**kw)
        assert st == INVALID and untouched, kw
    # n_cands = 0: GM_OK, nothing written; a bad format is not looked at without samples of the caller's
    st, untouched, *_ = call([])
    assert st == 0 and untouched
    st, untouched, *_ = call([ok], fmt=99)
    assert st == 0 and not untouched
    # a null cfg is the defaults: L = 0
    st, untouched, out, z, s = call([ok], cfg=None)
    assert st == 0 and not (z[:R_u] == np.complex64(7 + 7j)).any() and (z[R_u:] == np.complex64(7 + 7j)).all()
    eng.close()


def test_no_search_yet_and_a_plain_handle_after_the_setters(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    c = AM.build_case(oracle.ca_code_table(), 2048, 0, 2)
    N = c["N"]
    eng = _engine(A, c, "lds")
    cand = [_cand(0, 1, N - 91), _cand(1, 1, (3 * N) // 7)]
    kw = dict(lag_half_window=3, want_prompts=True, want_surface=True, n_freq=33)
    with pytest.raises(GmError) as e:          # no search yet: the NULL route has no snapshot ...
        eng.local_search(cand, **kw)
    assert e.value.status == INVALID
    d_x = hipbuf.upload(c["x"])
    fresh = eng.local_search(cand, samples=d_x, fmt=_fmt(c), **kw)          # ... the caller's samples need none
    eng.search(c["x"])
    ref = eng.local_search(cand, **kw)
    for a, b in zip(ref, fresh):
        _same_entry(a, b)
    assert [g["code_phase_samples"] for g in ref] == [N - 91, (3 * N) // 7]
    # both setters on, a search, and off again: the setters drop the snapshot, and the plain handle's words come back
    eng.set_edge_search([0, 2], AM.ROW)
    eng.set_code_drift(N - 0.4 + 0.3 * np.arange(AM.D))
    with pytest.raises(GmError) as e:
        eng.local_search(cand, **kw)
    assert e.value.status == INVALID
    n = eng.dwell_samples
    eng.search(np.concatenate([c["x"], c["x"]])[:n])
    assert eng.local_search([_cand(0, 1, 5, 1)], **kw)[0]["offset_periods"] == 1
    eng.set_edge_search([])
    eng.set_code_drift(None)
    with pytest.raises(GmError) as e:          # an offset is refused again
        eng.local_search([_cand(0, 1, 5, 1)], samples=d_x, fmt=_fmt(c), **kw)
    assert e.value.status == INVALID
    eng.search(c["x"])
    for a, b in zip(ref, eng.local_search(cand, **kw)):
        _same_entry(a, b)
    eng.close()
