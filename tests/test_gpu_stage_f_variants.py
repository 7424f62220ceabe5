"""Every stage-F kernel of the coherent, edge and drift handles (acq_stage_f_variants.h: one body per form, a loader per family) on every
plan it is built for: the 18 in-LDS plans, the eight composite bases find_comp can reach and the seven long-path bases, native and padded — one row
of acq_model.CASES per (form, base) pair gm_acq_plan_info can return (tests/test_acq_model_host.py holds the table to the planner).

Every row runs P = 2 codes, D = 3 bins, fs = 1000 N, f_if = 0 under four variants, the sample formats rotating over the rows:
  1. coherent          K = 3, M = 2
  2. edge              K = 3, M = 2, offsets [0, 2], row [1, -1, -1]
  3. drift, fold, edge K = 3, M = 2, the same offsets and row, T_d = N - 0.4 + 0.3 d
  4. drift at K = 1    M = 3, T_d = N - 3.7 + 1.3 d (the second period starts 4, 2 and 1 samples early)
D = 3 and M = 2 or 3 are no powers of two: the kernels' v / D, item / n_int and blockIdx % Q decompositions have to be right.

Two checks per variant.  Model: every cell of the device's block against the float64 model of acq_model.py — the arg-max equal (the
scene check on the CPU shows every cell's second lag at least 1e-3 below its peak), max and sum within REL = 1e-5; with offsets the
reduced block and the choice against numpy's reduction of the device's block.  Identity: the host forms the fold in float32 with the
handle's own phasor words and starts (acq_model.fold) and a plain handle (coherent_periods = 1, same size, bins, codes and
n_integrations) searches the M folded groups, one call per (h, d); column d of its three words equals the variant's [., h, d] words
as uint32 — "the host restates the fold exactly" (acq_stage_f_variants.h) and "a cell's words do not depend on what shares the launch".  The
composite bases are no exception: the wave-specialised kernel of base 16000 (acq_comp_ws.h) is stage C's, which the variants and the
plain handle share; stage F there is comp_fwd_sub_kernel and comp_fwd_sub_fold_kernel like everywhere else.

Then the two cases of acq_edge_reduce_kernel no other test reaches: ties between the hypotheses, and a PRN mask."""
import numpy as np
import pytest

import acq_model as AM

pytestmark = pytest.mark.gpu
REL = AM.REL
IDS = ["%d-%s" % (n, f) for n, f, _ in AM.CASES]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(A, c, form, K, M, strict):
    return A.AcquisitionEngine(c["fs"], 0.0, c["N"], doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=M, codes=c["chips"],
                               code_rate=c["code_rate"], coherent_periods=K, any_length=form.startswith("long"), strict_sum_order=strict)


def _run_variant(A, code_table, row, v, strict=False, model=True):
    N, form, base = AM.CASES[row]
    c = AM.build_case(code_table, N, v, row)
    K, M, offsets, sec, x = c["K"], c["M"], c["offsets"], c["sec"], c["x"]
    tag = (N, form, c["name"], c["fmt"], strict)
    eng = _engine(A, c, form, K, M, strict)
    info = eng.plan_info()
    assert (info["form"], info["base"]) == (form, base), (tag, info)
    if offsets:
        eng.set_edge_search(offsets, sec)
    if c["T"] is not None:
        eng.set_code_drift(c["T"])
        assert (eng.code_drift_starts() == c["starts"]).all(), tag
    assert eng.dwell_samples == c["dwell"] == len(x), tag
    assert (eng.table_freq == AM.DOP).all()
    eng.search(x)
    mx, am, sm = eng.metrics()
    if offsets:
        fmx, fam, fsm = eng.edge_metrics()
        rmx, ram, rsm, ch = AM.reduce_block(fmx, fam, fsm)      # the reduction, word for word on the device's own block
        assert (_words(mx) == _words(rmx)).all() and (am == ram).all() and (_words(sm) == _words(rsm)).all(), tag
        assert (eng.edge_choice() == ch).all(), tag
    else:
        fmx, fam, fsm = mx[:, None, :], am[:, None, :], sm[:, None, :]
    offs = offsets or [0]
    assert fmx.shape == (AM.P, len(offs), AM.D)

    if model:       # ---- every cell against the float64 model: nothing of the device but the mix tables
        emx, eam, esm = AM.search_model(x, eng.tables(), c["codes"], N, K, M, AM.DOP, c["fs"], c["starts"], offsets, sec)
        rel = lambda got, want: float(np.max(np.abs(got.astype(np.float64) / want - 1.0)))
        print("%s: max rel %.2e, sum rel %.2e" % (tag, rel(fmx, emx), rel(fsm, esm)))
        assert (fam == eam).all(), (tag, fam, eam)
        assert ((eam >= c["expect"][..., 0]) & (eam <= c["expect"][..., 1])).all(), (tag, eam)
        assert np.allclose(fmx, emx, rtol=REL, atol=0.0), (tag, fmx, emx)
        assert np.allclose(fsm, esm, rtol=REL, atol=0.0), (tag, fsm, esm)

    # ---- word for word: the plain search of the host's float32 fold
    plain = _engine(A, c, form, 1, M, strict)
    for h, o in enumerate(offs):
        rho = eng.code_drift_phasors(h) if c["T"] is not None else eng.coherent_phasors()       # [D][M][K] / [D][K]
        for d in range(AM.D):
            y = AM.fold(x, N, K, M, rho[d], c["starts"][d], o, sec)
            plain.search(y.reshape(-1))
            pmx, pam, psm = plain.metrics()
            assert (fam[:, h, d] == pam[:, d]).all(), (tag, h, d, fam[:, h, d], pam[:, d])
            assert (_words(fmx[:, h, d]) == _words(pmx[:, d])).all(), (tag, h, d, fmx[:, h, d], pmx[:, d])
            assert (_words(fsm[:, h, d]) == _words(psm[:, d])).all(), (tag, h, d, fsm[:, h, d], psm[:, d])
    plain.close()
    eng.close()


@pytest.mark.parametrize("row", range(len(AM.CASES)), ids=IDS)
def test_every_variant_against_the_model_and_the_plain_search(gpu, oracle, row):
    from gnss_sdr_rs_amd import acquisition as A
    for v in range(len(AM.VARIANTS)):
        _run_variant(A, oracle.ca_code_table(), row, v)


@pytest.mark.parametrize("row", [i for i, (n, _, _) in enumerate(AM.CASES) if n in AM.STRICT_ROWS],
                         ids=[i for i, (n, _, _) in zip(IDS, AM.CASES) if n in AM.STRICT_ROWS])
def test_the_identity_under_strict_sum_order(gpu, oracle, row):
    """one row per form: the variants and the plain handle both with strict_sum_order"""
    from gnss_sdr_rs_amd import acquisition as A
    for v in range(len(AM.VARIANTS)):
        _run_variant(A, oracle.ca_code_table(), row, v, strict=True, model=False)


# ---- the reduction over the hypotheses (acq_edge_reduce_kernel) ---------------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
def test_tied_hypotheses_choose_the_lowest(gpu, oracle, zero):
    """One period of a scene, noise included, tiled K M + 2 times (or an all-zero dwell): the hypotheses at offsets 0 and 2 read
    identical samples, so their planes are equal word for word and every cell must choose hypothesis 0."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, K, M, fs, offsets = 2048, 2, 2, 2.048e6, [0, 2]
    sats = [dict(prn_row=4, cn0_dbhz=52.0, doppler_hz=130.0, code_start=N - 91)]
    one = synth.to_i8_iq(synth.make_scene(oracle.ca_code_table(), fs, 0.0, N, sats, config_id=950))
    x = np.zeros(((K * M + 2) * N, 2), np.int8) if zero else np.tile(one, (K * M + 2, 1))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=AM.DOP, prn_ids=[5, 6], n_integrations=M, coherent_periods=K)
    eng.set_edge_search(offsets)
    assert eng.dwell_samples == len(x)
    got = eng.search(x)
    fmx, fam, fsm = eng.edge_metrics()
    for a in (fmx, fam, fsm):
        assert (_words(a[:, 0, :]) == _words(a[:, 1, :])).all(), a
    assert (eng.edge_choice() == 0).all(), eng.edge_choice()
    mx, am, sm = eng.metrics()
    assert (_words(mx) == _words(fmx[:, 0])).all() and (am == fam[:, 0]).all() and (_words(sm) == _words(fsm[:, 0])).all()
    if zero:
        assert (fmx == 0.0).all() and (fsm == 0.0).all()
    else:
        assert got[0] is not None and int(got[0]["code_phase_samples"]) == N - 91, got
    for r in got:
        assert r is None or r["edge_offset_periods"] == 0, r
    eng.close()


def test_edge_search_under_a_prn_mask(gpu, oracle):
    """Three workers, prn_mask selecting workers 0 and 2: their rows of metrics() and edge_choice() are those of the unmasked search
    word for word, worker 1 decides None and its rows stay as the search before left them."""
    from gnss_sdr_rs_amd import acquisition as A, synth
    N, K, M, fs, offsets = 2048, 2, 2, 2.048e6, [0, 2]
    dop = np.array([-300.0, 0.0, 300.0], np.float32)
    n = (K * M + 2) * N

    def scene(config_id, starts):
        sats = [dict(prn_row=4 + w, cn0_dbhz=52.0, doppler_hz=130.0 - 150.0 * w, code_start=s) for w, s in enumerate(starts)]
        return synth.to_i8_iq(synth.make_scene(oracle.ca_code_table(), fs, 0.0, n, sats, config_id=config_id))

    def words(eng):
        return [_words(a).copy() for a in eng.metrics()] + [eng.edge_choice().copy()]

    x, before = scene(951, (N - 91, (3 * N) // 7, 700)), scene(952, (300, 1200, 1500))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=[5, 6, 7], n_integrations=M, coherent_periods=K)
    eng.set_edge_search(offsets)
    ref_res = eng.search(x)
    ref = words(eng)
    assert ref_res[1] is not None, ref_res       # unmasked, worker 1 finds its satellite
    eng.search(before)                     # the search before, on other samples, unmasked
    prev = words(eng)
    assert not any((a[1] == b[1]).all() for a, b in zip(ref[:3], prev[:3]))      # worker 1's rows differ between the two dwells
    got = eng.search(x, prn_mask=0b101)
    now = words(eng)
    assert got[1] is None and got[0] == ref_res[0] and got[2] == ref_res[2], (got, ref_res)
    for a, r, p in zip(now, ref, prev):
        assert (a[0] == r[0]).all() and (a[2] == r[2]).all(), (a, r)
        assert (a[1] == p[1]).all(), (a, p)
    eng.close()
