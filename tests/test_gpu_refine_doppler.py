"""Fine Doppler from per-period prompts (gm_acq_refine_doppler, csrc/acq_refine.hip) on the GPU.

1. Prompts, spectrum and peak of EVERY (worker, bin) cell against the float64 model of acq_refine_model.py, on acq_model.build_case
   scenes of six sizes: every form gm_acq_plan_info reports, every sample format, N below one workgroup's 2048 samples a step (256), N
   no multiple of 256 with 1-byte starts anywhere (2000, real, drift), a replica rotation that wraps (one code starts at N - 91).
2. center_power is the search's own accumulated peak power of the cell (K >= 2; at K = 1 that power is N^2 sum |z|^2).
3. Truth: numpy-built scenes with a secondary row, data bits and a code period of N - 0.4 samples; the search finds the satellite and
   the edge and the refined carrier is within a quarter of the dwell's frequency resolution (plus one grid step) of the simulated one.
4. Where gm_acq_finer_doppler cannot go (a drift dwell shorter than K M N contiguous samples) the new entry runs.
5. A satellite's words depend neither on what else is refined in the call nor on repetition, and the search's words stay.
6. Every search entry, the argument errors, the no-op, and the handle after both setters were switched off.

Bounds.  REL = acq_model.REL = 1e-5 is the project's bound for correlator sums: |z_dev - z_model| <= REL max |z_model| per cell (the
worst-order f32 restatement of the N-term sum stayed within 2.9e-6).  |S_dev - S_model| <= 3 REL max S_model: twice the prompts'
bound from the squaring, one more for the f32 phasors and sums.  Neighbouring grid values differ by about 1e-6 of the peak, so the
device's peak index may be a tie of the model's: S_model[peak_index_dev] >= (1 - 3 REL) max S_model, and the interpolated offsets
agree to one grid step."""
import ctypes as C

import numpy as np
import pytest

import acq_model as AM
import acq_refine_model as RM

pytestmark = pytest.mark.gpu
REL = AM.REL
INVALID, OUT_OF_RANGE = -1, -5

# (fft_size, form, variant index in AM.VARIANTS, row_index -> sample format, span_periods)
CELL_CASES = [(256, "lds", 0, 2, 0),           # coherent, c32
              (2000, "lds", 3, 1, 3),          # drift at K = 1, real, J = 3
              (2048, "lds", 2, 1, 0),          # drift + fold + edge, i8
              (18000, "composite", 1, 0, 0),   # edge
              (6144, "long", 2, 0, 0),         # drift + fold + edge
              (3064, "long_padded", 0, 0, 0)]  # coherent
CELL_IDS = ["%d-%s-%s" % (n, f, AM.VARIANTS[v][0]) for n, f, v, _, _ in CELL_CASES]
CELL_FORMATS = {256: "c32", 2000: "real", 2048: "i8"}


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def _cell_results(am, d):
    """one results entry per worker for bin d: the cell's own first arg-max as the code phase"""
    return [dict(doppler_bin=d, code_phase_samples=int(am[w][d])) for w in range(am.shape[0])]


_CELLS = {}


def _cells(oracle, i):
    """One search and the refinement of every (worker, bin) cell of CELL_CASES[i], with the model's values: computed once, shared by
    the tests below and left unchanged."""
    if i in _CELLS:
        return _CELLS[i]
    from gnss_sdr_rs_amd import acquisition as A
    N, form, v, row_index, span = CELL_CASES[i]
    c = AM.build_case(oracle.ca_code_table(), N, v, row_index)
    assert CELL_FORMATS.get(N, c["fmt"]) == c["fmt"]
    eng = _engine(A, c, form)
    assert eng.plan_info()["form"] == form
    _setup(eng, c)
    eng.search(c["x"])
    mx, am, _ = eng.metrics()
    offs = c["offsets"] or [0]
    if c["offsets"]:
        fmx, ch = eng.edge_metrics()[0], eng.edge_choice()
        cell_max = np.take_along_axis(fmx, ch[:, None, :].astype(np.int64), axis=1)[:, 0, :]
    else:
        ch, cell_max = np.zeros((AM.P, AM.D), np.uint32), mx
    tab = eng.tables()
    tf = eng.table_freq
    dev, model = {}, {}
    for d in range(AM.D):
        p = RM.plan(c["K"], c["M"], c["fs"], N, tf, d, span)
        got = eng.refine_doppler(_cell_results(am, d), span_periods=span, want_prompts=True, want_spectrum=True)
        for w in range(AM.P):
            o = offs[int(ch[w, d])]
            dev[w, d] = got[w]
            model[w, d] = dict(RM.refine(c["x"], tab[d], c["codes"][w], N, c["starts"][d], o, int(am[w, d]), tf[d], c["fs"],
                                         p["span_periods"], p["n_groups"], p["n_freq"], p["half_span_hz"], c["sec"]), plan=p, offset=o)
    eng.close()
    _CELLS[i] = dict(c=c, dev=dev, model=model, cell_max=cell_max, am=am)
    return _CELLS[i]


# ---- 1. every cell against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CELL_CASES)), ids=CELL_IDS)
def test_prompts_spectrum_and_peak_of_every_cell_against_the_model(gpu, oracle, i):
    r = _cells(oracle, i)
    c = r["c"]
    assert c["starts"].shape[0] == AM.D and int(r["am"][0].max()) > c["N"] - 100       # worker 0's code starts at N - 91: the rotation wraps
    for (w, d), got in r["dev"].items():
        want, tag = r["model"][w, d], (CELL_IDS[i], w, d)
        p = want["plan"]
        assert (got["span_periods"], got["n_groups"], got["n_freq"]) == (p["span_periods"], p["n_groups"], p["n_freq"]), tag
        assert got["doppler_bin"] == d and got["offset_periods"] == want["offset"], (tag, got)
        assert got["step_hz"] == pytest.approx(p["step_hz"], rel=1e-6) and got["half_span_hz"] == pytest.approx(p["half_span_hz"], rel=1e-6)
        z, S = got["prompts"].astype(np.complex128), got["spectrum"].astype(np.float64)
        zerr = float(np.max(np.abs(z - want["z"])) / np.max(np.abs(want["z"])))
        serr = float(np.max(np.abs(S - want["S"])) / np.max(want["S"]))
        print("%s: prompts %.2e, spectrum %.2e of the largest, peak %d / %d, delta %+.3f / %+.3f Hz"
              % (tag, zerr, serr, got["peak_index"], want["peak_index"], got["delta_hz"], want["delta_hz"]))
        assert zerr <= REL, tag
        assert serr <= 3 * REL, tag
        assert want["S"][got["peak_index"]] >= (1.0 - 3 * REL) * want["S"].max(), tag
        assert got["peak_power"] == got["spectrum"][got["peak_index"]] == got["spectrum"].max(), tag
        assert got["peak_index"] == int(np.argmax(got["spectrum"])), tag                   # the first index of the device's own maximum
        assert got["center_power"] == got["spectrum"][(p["n_freq"] - 1) // 2], tag
        assert got["at_edge"] == int(got["peak_index"] in (0, p["n_freq"] - 1)), tag
        if not got["at_edge"] and not want["at_edge"]:
            assert abs(got["delta_hz"] - want["delta_hz"]) <= p["step_hz"], tag
        assert got["carrier_hz"] == pytest.approx(float(AM.DOP[d]) + got["delta_hz"], abs=1e-3), tag


def test_a_dwell_longer_than_the_staged_prompts(gpu, oracle):
    """K = 1, M = 1030 periods of 256 samples, span_periods = 515: G = 2 groups at K = 1 and R_u = 1030 prompts per satellite, past the
    1024 the scan kernel stages in LDS — its other instantiation reads them from global memory.  Same bounds against the model."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, M, J = 256, 1030, 515
    fs = N * 1000.0
    chips = AM.case_chips(oracle.ca_code_table(), N)
    rate = 1000.0 * chips.shape[1]
    sats = [dict(prn_row=0, cn0_dbhz=44.0, doppler_hz=130.0, code_start=N - 91, phase=0.4)]
    x = AM.convert(synth.make_scene(chips, fs, 0.0, M * N, sats, config_id=930, code_rate=rate), "c32")
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=M, codes=chips, code_rate=rate)
    eng.search(x)
    am = eng.metrics()[1]
    assert abs(int(am[0, 1]) - (N - 91)) <= 1, am
    got = eng.refine_doppler(_cell_results(am, 1), span_periods=J, want_prompts=True, want_spectrum=True)
    tab = eng.tables()
    eng.close()
    codes = AM.sample_codes(chips, rate, fs, N)
    starts = AM.plain_starts(AM.D, M, N)
    for w in range(AM.P):
        assert (got[w]["span_periods"], got[w]["n_groups"], got[w]["prompts"].size) == (J, 2, 1030)
        want = RM.refine(x, tab[1], codes[w], N, starts[1], 0, int(am[w, 1]), 0.0, fs, J, 2, 257, 150.0)
        z, S = got[w]["prompts"].astype(np.complex128), got[w]["spectrum"].astype(np.float64)
        zerr = float(np.max(np.abs(z - want["z"])) / np.max(np.abs(want["z"])))
        serr = float(np.max(np.abs(S - want["S"])) / np.max(want["S"]))
        print("worker %d: prompts %.2e, spectrum %.2e of the largest, peak %d / %d" % (w, zerr, serr, got[w]["peak_index"], want["peak_index"]))
        assert zerr <= REL and serr <= 3 * REL, (w, zerr, serr)
        assert want["S"][got[w]["peak_index"]] >= (1.0 - 3 * REL) * want["S"].max(), w
    # the satellite's line: 130 Hz, to the grid's step (the line of a 515 ms span is 2 Hz wide, the step 1.17 Hz)
    assert got[0]["at_edge"] == 0 and abs(got[0]["carrier_hz"] - 130.0) <= 2 * got[0]["step_hz"], got[0]["carrier_hz"]


# ---- 2. the centre of the grid is the search's own cell -------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CELL_CASES)), ids=CELL_IDS)
def test_center_power_is_the_cells_accumulated_peak_power(gpu, oracle, i):
    """K >= 2: S at delta = 0 and metrics() max of the cell (with the edge search: edge_metrics() max of the chosen hypothesis) are
    both within REL of the same float64 value.  K = 1 (J = M here): that power is the non-coherent sum N^2 sum_i |z[i]|^2 — the
    coherent S is another quantity there."""
    r = _cells(oracle, i)
    c = r["c"]
    for (w, d), got in r["dev"].items():
        want = float(r["cell_max"][w, d])
        if c["K"] >= 2:
            have = float(got["center_power"])
        else:
            assert got["span_periods"] * got["n_groups"] == c["M"]
            z = got["prompts"].astype(np.complex128)
            have = float(c["N"]) ** 2 * float(np.sum(z.real ** 2 + z.imag ** 2))
        print("%s: cell %d,%d centre / search - 1 = %+.2e" % (CELL_IDS[i], w, d, have / want - 1.0))
        assert abs(have - want) <= 2 * REL * want, (CELL_IDS[i], w, d, have, want)


# ---- 3. truth ----------------------------------------------------------------------------------------------------------------
def _truth(oracle, name, offsets=None):
    """-> (engine after the search, scene, the search's results); offsets: search these hypotheses only (the dwell then ends earlier)"""
    from gnss_sdr_rs_amd import acquisition as A
    c = RM.truth_scene(oracle.ca_code_table(), name)
    if offsets is not None:
        R = c["K"] * c["M"] + offsets[-1]
        c["offsets"], c["starts"] = list(offsets), c["starts"][:, :R]
        c["dwell"] = int(c["starts"][:, -1].max()) + c["N"]
        c["x"] = c["x"][:c["dwell"]]
    eng = _engine(A, c, "lds", f_if=c["f_if"], prn_ids=[RM.TRUTH_PRN], decision_mode=A.DECIDE_BEST_BIN)
    _setup(eng, c)
    res = eng.search(c["x"])
    return eng, c, res


@pytest.mark.parametrize("name", sorted(RM.TRUTH_SCENES))
def test_the_refined_carrier_is_the_simulated_one(gpu, oracle, name):
    eng, c, res = _truth(oracle, name)
    r = res[0]
    assert r is not None and r["doppler_bin"] == 1, (name, res)                            # the search finds the satellite ...
    assert c["cp_window"][0] <= r["code_phase_samples"] <= c["cp_window"][1], (name, r)
    if c["offsets"]:
        assert r["edge_offset_periods"] == c["edge"], (name, r)                            # ... and the edge
    got = eng.refine_doppler(res, span_periods=c["span"])[0]
    eng.close()
    R_u = got["span_periods"] * got["n_groups"]
    assert R_u == c["K"] * c["M"] and got["offset_periods"] == c["edge"]
    err, bound = got["carrier_hz"] - c["f_true"], RM.truth_bound(R_u)
    print("scene %s: carrier error %+.2f Hz, bound %.1f + step %.2f Hz" % (name, err, bound, got["step_hz"]))
    assert got["at_edge"] == 0, (name, got)
    assert abs(err) <= bound + got["step_hz"], (name, err, bound)


# ---- 4. where the legacy estimator cannot go ------------------------------------------------------------------------------------
def test_a_drift_dwell_the_legacy_estimator_refuses(gpu, oracle):
    """Scene (a)'s samples with the hypotheses up to the true edge only, offsets (0, 1): with all four the dwell runs to period 15, and
    the K M = 12 contiguous periods gm_acq_finer_doppler strips from the winning offset 1 on would still fit into it (13 x 2048 <
    14 x 2047.6 + 2048), so it would not refuse.  With the dwell ending at the true edge's last period, 0.4 samples a period short of
    N, it does — today's behaviour — and the new entry runs."""
    from gnss_sdr_rs_amd._lib import GmError
    eng, c, res = _truth(oracle, "a", offsets=(0, 1))
    assert res[0] is not None and res[0]["doppler_bin"] == 1 and res[0]["edge_offset_periods"] == c["edge"], res
    assert c["dwell"] < (c["K"] * c["M"] + c["edge"]) * c["N"]          # T < N: the dwell ends before K M contiguous periods from the edge
    with pytest.raises(GmError) as e:
        eng.finer_doppler(res)
    assert e.value.status == OUT_OF_RANGE
    assert eng.refine_doppler(res)[0]["at_edge"] == 0
    eng.close()


# ---- 5. words do not depend on company or repetition ----------------------------------------------------------------------------
def _same_entry(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert (_words(a[k]) == _words(b[k])).all(), k
        else:
            assert np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes(), (k, a[k], b[k])


def test_words_depend_neither_on_company_nor_on_repetition(gpu, oracle):
    from gnss_sdr_rs_amd import acquisition as A
    c = AM.build_case(oracle.ca_code_table(), 2048, 2, 1)
    eng = _engine(A, c, "lds")
    _setup(eng, c)
    eng.search(c["x"])
    search_words = lambda: [_words(a).copy() for a in eng.metrics() + eng.edge_metrics()] + [eng.edge_choice().copy()]
    before = search_words()
    both = _cell_results(eng.metrics()[1], 1)
    kw = dict(want_prompts=True, want_spectrum=True, n_freq=65)
    pair = eng.refine_doppler(both, **kw)
    alone = eng.refine_doppler([both[0], None], **kw)
    again = eng.refine_doppler(both, **kw)
    assert alone[1] is None and pair[1] is not None
    _same_entry(pair[0], alone[0])
    _same_entry(pair[0], again[0])
    _same_entry(pair[1], again[1])
    assert not (_words(pair[0]["prompts"]) == _words(pair[1]["prompts"])).all()
    for u, v in zip(before, search_words()):
        assert u.shape == v.shape and (u == v).all()
    eng.close()


# ---- 6. entry points and errors -----------------------------------------------------------------------------------------------
def test_every_search_entry_gives_the_same_words(gpu, oracle, hipbuf):
    """search (host), search_dev, search_prepared_dev and search_ring on the same samples; then the edge search and the code drift
    switched on and off again: the call follows the plain handle's starts."""
    from gnss_sdr_rs_amd import acquisition as A, tracking as T
    from gnss_sdr_rs_amd._lib import GmError
    c = AM.build_case(oracle.ca_code_table(), 2048, 0, 2)
    assert c["fmt"] == "c32"
    x, N = c["x"], c["N"]
    eng = _engine(A, c, "lds")
    kw = dict(want_prompts=True, want_spectrum=True, n_freq=33)
    with pytest.raises(GmError) as e:          # no search yet
        eng.refine_doppler([dict(doppler_bin=1, code_phase_samples=0)])
    assert e.value.status == INVALID
    eng.search(x)
    cells = _cell_results(eng.metrics()[1], 1)
    ref = eng.refine_doppler(cells, **kw)

    def same():
        got = eng.refine_doppler(cells, **kw)
        for a, b in zip(got, ref):
            _same_entry(a, b)

    d_x = hipbuf.upload(x)
    eng.search_dev(d_x, 0)
    same()
    tok = eng.prepare_dev(d_x, 0)
    eng.search_prepared_dev(tok)
    same()
    ring = T.MulticastRingBuffer(1 << 14)
    ring.write_samples(x)
    res, tail = eng.search_ring(ring)
    assert tail == 0
    same()
    ring.close()
    # both setters on (another dwell, other starts, a row), a search, and off again in the other order
    eng.set_edge_search([0, 2], AM.ROW)
    eng.set_code_drift(N - 0.4 + 0.3 * np.arange(AM.D))
    with pytest.raises(GmError) as e:          # the setters drop the snapshot
        eng.refine_doppler(cells)
    assert e.value.status == INVALID
    n = eng.dwell_samples
    eng.search(np.concatenate([x, x])[:n])
    assert eng.refine_doppler(cells, **kw)[0]["offset_periods"] in (0, 2)
    eng.set_edge_search([])
    eng.set_code_drift(None)
    eng.search(x)
    same()
    eng.close()


def test_argument_errors_and_the_no_op(gpu, oracle):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    from gnss_sdr_rs_amd._lib import GmError
    c = AM.build_case(oracle.ca_code_table(), 2048, 0, 2)
    eng = _engine(A, c, "lds")
    eng.search(c["x"])
    ok = dict(doppler_bin=1, code_phase_samples=5)
    assert eng.refine_doppler([ok, None])[0]["doppler_bin"] == 1
    bad = [([ok, ok, ok], {}),                                     # n_prn above the handle's workers
           ([dict(ok, doppler_bin=AM.D)], {}), ([dict(ok, doppler_bin=-1)], {}),
           ([dict(ok, code_phase_samples=c["N"])], {}),
           ([ok], dict(span_periods=2)),                           # K = 3: span_periods must be 0 or K
           ([ok], dict(n_freq=64)), ([ok], dict(n_freq=1)), ([ok], dict(n_freq=4099)),
           ([ok], dict(half_span_hz=501.0)), ([ok], dict(half_span_hz=-1.0))]
    for results, kw in bad:
        with pytest.raises(GmError) as e:
            eng.refine_doppler(results, **kw)
        assert e.value.status == INVALID, (results, kw)
    assert eng.refine_doppler([None, dict(ok, doppler_bin=0)])[0] is None
    # all found flags zero: GM_OK and nothing written; a not-found entry is not looked at, whatever it holds
    res = (_lib.AcqResult * 2)()
    res[0].doppler_bin = 99                                        # (not found: not looked at)
    found = np.zeros(2, np.uint8)
    out = np.full(2 * C.sizeof(_lib.AcqRefineOut), 0xAB, np.uint8)
    z = np.full(2 * 6, np.complex64(7 + 7j))
    s = np.full(2 * 257, np.float32(7.0))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _lib.lib().gm_acq_refine_doppler(eng._h, C.cast(res, C.c_void_p), vp(found), 2, None, vp(out), vp(z), vp(s)) == 0
    assert (out == 0xAB).all() and (z == np.complex64(7 + 7j)).all() and (s == 7.0).all()
    # one found: the other worker's entries stay untouched
    found[1] = 1
    res[1].doppler_bin, res[1].code_phase_samples = 1, 5
    assert _lib.lib().gm_acq_refine_doppler(eng._h, C.cast(res, C.c_void_p), vp(found), 2, None, vp(out), vp(z), vp(s)) == 0
    half = C.sizeof(_lib.AcqRefineOut)
    assert (out[:half] == 0xAB).all() and not (out[half:] == 0xAB).all()
    assert (z[:6] == np.complex64(7 + 7j)).all() and (s[:257] == 7.0).all() and not (s[257:] == 7.0).any()
    eng.close()
