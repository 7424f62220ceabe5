"""Stage C at N = 8000 with its constant twiddles folded into the butterflies (csrc/fft_core.h BflyTw, FuseTw<CorrPlan8000>), against
the float64 model of acq_model.py.

An N = 8000 handle, 2 PRNs (PRN 5 present at 50 dB-Hz, PRN 6 absent), 3 Doppler bins around the true one: once with M = 1, where the
items are uncut and the sums stay in registers, and once with M = 2, where the grid is small, so every item is cut and merged through
the ticket path (the launch's item map, csrc/acq_kernels.hip; the ABI does not report which items were cut, so that is assumed
here, not asserted: test_grid_8_shards_equal_1_shard and the parity sweep hold the cut path to the uncut one).  One transform already runs every k1 and j1 row of both fused passes: all eight waves take part.  On every one of
the 6 planes the arg-max is equal and max and sum are within REL = 1e-5.  One composite case, N = 32000 = 2 x 16000 with 1 code, 2 bins
and M = 1, confirms that the 16000 path (which keeps the plain form) still agrees.

The scene seeds are chosen so that, in the float64 model alone, the two largest cells of every plane differ by more than 1e-4
relative: an exact index comparison then cannot fail on a tie.  test_scene_planes_have_no_near_tie asserts that without a GPU, and
the GPU tests assert it again before they compare (same tables, same model: the mix tables are built by the host entry)."""
import functools

import numpy as np
import pytest

import acq_model as AM

REL = AM.REL
TIE = 1e-4
DOP = np.array([-250.0, 0.0, 250.0], np.float32)
# (fft_size, M) -> (PRN ids, bins, satellites, scene seed)
SCENES = {
    (8000, 1): ((5, 6), DOP, [dict(prn_row=4, cn0_dbhz=50.0, doppler_hz=60.0, code_start=8000 - 91, phase=0.4)], 0),
    (8000, 2): ((5, 6), DOP, [dict(prn_row=4, cn0_dbhz=50.0, doppler_hz=60.0, code_start=8000 - 91, phase=0.4)], 0),
    (32000, 1): ((5,), DOP[1:], [dict(prn_row=4, cn0_dbhz=60.0, doppler_hz=60.0, code_start=(3 * 32000) // 7, phase=0.4)], 0),
}


@functools.lru_cache(maxsize=None)
def _case(N, M):
    """The scene, the host-built mix tables and the model's [P][D] planes with their peak gaps: computed once, shared, not modified"""
    from gnss_sdr_rs_amd import acquisition as A, synth
    prns, dop, sats, seed = SCENES[(N, M)]
    fs = 1000.0 * N
    table = A.ca_code_table()
    x = synth.to_i8_iq(synth.make_scene(table, fs, 0.0, M * N, sats, config_id=970 + seed))
    tables = [A.DopplerShiftTable(0.0, float(f), fs, N) for f in dop]
    codes = AM.sample_codes(table[[p - 1 for p in prns]], 1.023e6, fs, N)
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    mx, am, sm, gap = AM.search_model(x, np.stack([t.table for t in tables]), codes, N, 1, M, tf, fs, with_gap=True)
    for a in (x, mx, am, sm, gap):
        a.setflags(write=False)
    return dict(N=N, M=M, fs=fs, prns=prns, x=x, tables=tables, mx=mx[:, 0], am=am[:, 0], sm=sm[:, 0], gap=gap[:, 0], sats=sats)


def _assert_no_near_tie(c):
    assert c["gap"].shape == (len(c["prns"]), len(c["tables"]))
    assert (c["gap"] > TIE).all(), (c["N"], c["M"], c["gap"])
    # the present satellite's peak is where the scene put it, in the bin next to its Doppler
    s = c["sats"][0]
    assert c["am"][0, np.argmax(c["mx"][0])] == s["code_start"], (c["am"], s)


@pytest.mark.parametrize("N,M", sorted(SCENES))
def test_scene_planes_have_no_near_tie(gm, N, M):
    _assert_no_near_tie(_case(N, M))


def _compare(A, N, M, form, base):
    c = _case(N, M)
    _assert_no_near_tie(c)
    eng = A.AcquisitionEngine(c["fs"], 0.0, N, tables=c["tables"], prn_ids=list(c["prns"]), n_integrations=M)
    info = eng.plan_info()
    assert (info["form"], info["base"]) == (form, base), info
    assert eng.dwell_samples == len(c["x"])
    got = eng.search(c["x"])
    mx, am, sm = eng.metrics()
    eng.close()
    rel = lambda a, b: float(np.max(np.abs(a.astype(np.float64) / b - 1.0)))
    print("N=%d M=%d: max rel %.2e, sum rel %.2e, least model gap %.2e" % (N, M, rel(mx, c["mx"]), rel(sm, c["sm"]), c["gap"].min()))
    assert mx.shape == c["mx"].shape
    assert (am == c["am"]).all(), (am, c["am"])
    assert np.allclose(mx, c["mx"], rtol=REL, atol=0.0), (mx, c["mx"])
    assert np.allclose(sm, c["sm"], rtol=REL, atol=0.0), (sm, c["sm"])
    assert got[0] is not None and int(got[0]["code_phase_samples"]) == c["sats"][0]["code_start"], got


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2])
def test_n8000_fused_stage_c_against_the_model(gpu, M):
    from gnss_sdr_rs_amd import acquisition as A
    _compare(A, 8000, M, "lds", 8000)


@pytest.mark.gpu
def test_composite_32000_on_the_plain_16000_plan_against_the_model(gpu):
    from gnss_sdr_rs_amd import acquisition as A
    _compare(A, 32000, 1, "composite", 16000)
