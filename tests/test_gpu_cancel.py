"""Subtracting found satellites from a dwell (gm_acq_cancel, csrc/acq_cancel.hip) on the GPU.

1. Parity with the float64 model of acq_cancel_model.py on handles of N = 2048, 3 bins, workers PRN 5 and 6, K = 1, M = 6: with the
   code drift T = N - 0.4 in every bin (the dwell, 12286 samples, is no multiple of 8) and without it (12288), on int8 IQ, int8 real and
   c32 samples; candidate sets: one candidate; five candidates with the same worker twice; the plan cases of the host test, each with its
   own T.  n_cands = 0 returns the converted dwell.
1b. Every pointer form: the five candidates on every (format, drift) with the input one element off (acq_cancel_amp_kernel and
   acq_cancel_subtract_kernel with ALIGNED = false), the output 8 bytes off (OUT_ALIGNED = false) and both, each bit for bit the aligned
   run's output and amplitude words; nothing written in front of a moved output or behind the dwell; n_cands = 0 from a moved input.
2. A handle of another form (N = 4088 with any_length: padded long), one candidate.
3. Repetition, in place, the NULL route, the snapshot and the metrics.
4. Every GM_ERR_INVALID_ARG case with a pre-filled d_out and `out` left untouched, the overlap rule, no search yet.
5. The chain on the GPU on seed 100 of the host test's scene: search, local_search on the strong cell, cancel_cands_from_local, cancel,
   search_dev on the output.

Bounds.  REL = acq_model.REL = 1e-5, the project's bar.  Every output component and every amplitude component is within
REL * max(1, max |x|) of the model's (max |x| over the components of the dwell).  What the device rounds: the turn to f32 (half an ulp
of a number below 2: 1.2e-7 of a half turn, 3.7e-7 rad), the f32 sine and cosine (a few ulp), the f32 products and the f32 sum of at
most N + 9 terms in a tree of 256 partial sums — each a few 1e-7 of max |x| — so the bar is 10 to 30 times what the arithmetic needs.
The chip index and the cycles are f64 on both sides, word for word, so no sample can take another chip.  b, n_segments, first_samples and
last_samples are exact; removed_energy and amp_rms equal the host formula on the returned amplitude words to 1e-12 and to f32.

Measured on an MI355X: output within 9.0e-8 to 1.6e-7 and amplitudes within 1.1e-8 to 2.8e-8 of max(1, max |x|) over all eighteen
(format, drift, candidate set) runs and the padded-long handle; the chain on seed 100: strong peak-to-mean 360.7 -> 15.7 (the model's
values), the weak worker's arg-max 1644 -> 1201 at a peak-to-mean of 8.5."""
import ctypes as C

import numpy as np
import pytest

import acq_cancel_model as CM
import acq_model as AM
from test_acq_cancel_host import PLAN_CASES, SEEDS, STRONG_AFTER_BOUND, scene_run

pytestmark = pytest.mark.gpu
REL = AM.REL
INVALID = -1
N, FS, F_IF = CM.N, CM.FS, CM.F_IF
M_PARITY = 6
F_STRONG, F_WEAK = F_IF + CM.STRONG["doppler"], F_IF + CM.WEAK["doppler"]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fmt(name):
    from gnss_sdr_rs_amd import _lib
    return {"c32": _lib.FMT_C32, "i8": _lib.FMT_I8_IQ, "real": _lib.FMT_I8_REAL}[name]


def _engine(c, M, drift):
    from gnss_sdr_rs_amd import acquisition as A
    eng = A.AcquisitionEngine(FS, F_IF, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=M, codes=c["chips"],
                              code_rate=c["code_rate"])
    if drift:
        eng.set_code_drift(c["T"])
    assert eng.dwell_samples == c["dwell"] == len(c["x"])
    return eng


def _cand(w, f, cp, T=0.0):
    return dict(worker=w, carrier_hz=float(f), code_phase=float(cp), period_samples=float(T))


def _candidate_sets(D):
    one = [_cand(0, F_STRONG + 3.0, 700.25, CM.T_TRUE)]
    five = [_cand(0, F_STRONG + 3.0, 700.25, CM.T_TRUE), _cand(1, F_WEAK, 1200.7, CM.T_TRUE), _cand(0, F_STRONG - 40.0, 703.5, CM.T_TRUE),
            _cand(1, -F_WEAK, 17.0, 0.0), _cand(0, 0.0, 2047.99, N + 3.3)]           # (a negative and a zero carrier are legal)
    # the host test's plan cases, each with its own T: cp = 0.0, 2.5 and N - 0.25 at T = N - 0.4, cp = 2047.8 at T = 2047.6, T = N + 7.9
    plan = [_cand(i % 2, F_STRONG if i % 2 == 0 else F_WEAK, cp, T) for i, (_, _, cp, T) in enumerate(PLAN_CASES[:4] + [PLAN_CASES[6]])]
    assert [c["code_phase"] for c in plan] == [0.0, 2.5, N - 0.25, 2047.8, 700.3] and plan[4]["period_samples"] == N + 7.9
    return dict(one=one, five=five, plan=plan)


def _check(tag, c, cands, got, y):
    """the assertions of test 1 for one call -> (worst output error, worst amplitude error) over the bound's scale"""
    from gnss_sdr_rs_amd import acquisition as A
    D, real = c["dwell"], c["fmt"] == "real"
    want_y, want_a, want_b = CM.cancel_all(c["x"], c["chips"], cands, FS, N, real)
    scale = max(1.0, float(np.abs(np.stack(AM.as_parts(c["x"]))).max()))
    yerr = max(float(np.abs(y.real.astype(np.float64) - want_y.real).max()), float(np.abs(y.imag.astype(np.float64) - want_y.imag).max()))
    assert yerr <= REL * scale, (tag, yerr, scale)
    if real:
        assert (_words(y.imag.copy()) == 0).all(), tag          # exactly +0
    aerr = 0.0
    for i, (cd, g) in enumerate(zip(cands, got)):
        p = A.cancel_plan(D, N, cd["code_phase"], cd["period_samples"])
        assert (p["bounds"].astype(np.int64) == want_b[i]).all() and g["n_segments"] == p["n_segments"] == len(want_a[i]), (tag, i)
        assert g["amps"].shape == (len(want_a[i]),) and g["worker"] == cd["worker"], (tag, i)
        d = g["amps"].astype(np.complex128) - want_a[i]
        aerr = max(aerr, float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
        own = CM.out_fields(g["amps"], want_b[i], D)
        assert (g["first_samples"], g["last_samples"]) == (own["first_samples"], own["last_samples"]), (tag, i, g)
        assert g["removed_energy"] == pytest.approx(own["removed_energy"], rel=1e-12), (tag, i)
        assert g["amp_rms"] == pytest.approx(own["amp_rms"], rel=1e-6), (tag, i)
        empty = np.diff(want_b[i]) == 0
        assert (g["amps"][empty] == 0).all(), (tag, i)
    assert aerr <= REL * scale, (tag, aerr, scale)
    return yerr / scale, aerr / scale


_SCENES = {}


def _scene(oracle, fmt, drift):
    """the scene of the host test at M = 6, once per (format, drift)"""
    key = (fmt, drift)
    if key not in _SCENES:
        c = CM.scene(oracle.ca_code_table(), 7, fmt=fmt, periods=M_PARITY, drift=drift)
        if fmt == "c32":
            c["x"] = (c["x"] * np.float32(0.731)).astype(np.complex64)             # (not whole numbers)
        _SCENES[key] = c
    return _SCENES[key]


# ---- 1. parity with the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False], ids=["drift", "plain"])
@pytest.mark.parametrize("fmt", AM.FORMATS)
def test_parity_with_the_model(gpu, oracle, hipbuf, fmt, drift):
    c = _scene(oracle, fmt, drift)
    D = c["dwell"]
    assert D == (12286 if drift else 12288) and (D % 8 != 0) == drift
    eng = _engine(c, M_PARITY, drift)
    d_x = hipbuf.upload(c["x"])
    for name, cands in _candidate_sets(D).items():
        d_out = hipbuf.alloc(D * 8 + 64, fill=0x5A)
        got = eng.cancel(cands, d_out, samples=d_x, fmt=_fmt(fmt), want_amps=True)
        raw = hipbuf.download(d_out, D * 8 + 64, np.complex64)
        assert (raw[D:].view(np.uint8) == 0x5A).all()                               # nothing behind the dwell's last sample
        yerr, aerr = _check((fmt, drift, name), c, cands, got, raw[:D])
        print("%s %s %s: output within %.2e, amplitudes within %.2e of max(1, max |x|) (bound %.0e); |a| of candidate 0: %.2f .. %.2f"
              % (fmt, "drift" if drift else "plain", name, yerr, aerr, REL, np.abs(got[0]["amps"]).min(), np.abs(got[0]["amps"]).max()))
    # n_cands = 0: the converted dwell, exactly
    d_out = hipbuf.alloc(D * 8, fill=0x5A)
    assert eng.cancel([], d_out, samples=d_x, fmt=_fmt(fmt)) == []
    y = hipbuf.download(d_out, D * 8, np.complex64)
    re, im = AM.as_parts(c["x"])
    assert (_words(y.real.copy()) == _words(re)).all() and (_words(y.imag.copy()) == _words(im)).all()
    eng.close()


# ---- 1b. every pointer form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False], ids=["drift", "plain"])
@pytest.mark.parametrize("fmt", AM.FORMATS)
def test_every_pointer_form_gives_the_aligned_words(gpu, oracle, hipbuf, fmt, drift):
    """launch_cancel picks acq_cancel_amp_kernel<FMT, ALIGNED> and acq_cancel_subtract_kernel<FMT, ALIGNED, OUT_ALIGNED> by the low bits of
    the dwell's and the output's addresses; a fresh allocation only ever selects <true, true>.  An input one element (2 / 1 / 8 bytes)
    behind a 256-byte boundary selects ALIGNED = false (element loads), an output 8 bytes behind one selects OUT_ALIGNED = false (stores
    of one sample).  The arithmetic is the same, so every output word and every amplitude word equals the aligned run's, which _check
    holds to the model.  The moved input lies between 0x5A bytes (90 as int8, 1.5e16 as f32) and the outputs are pre-filled with them."""
    c = _scene(oracle, fmt, drift)
    D = c["dwell"]
    assert D == (12286 if drift else 12288) and (D % 8 != 0) == drift
    eng = _engine(c, M_PARITY, drift)
    cands = _candidate_sets(D)["five"]
    elem = {"i8": 2, "real": 1, "c32": 8}[fmt]
    raw = np.ascontiguousarray(c["x"]).view(np.uint8).reshape(-1)
    assert raw.size == D * elem
    d_x = hipbuf.upload(c["x"])
    d_pad = hipbuf.upload(np.concatenate([np.full(elem, 0x5A, np.uint8), raw, np.full(64, 0x5A, np.uint8)]))
    assert d_x % 256 == 0 and d_pad % 256 == 0                                      # so d_pad + elem is aligned to its element only

    def run(samples, shift, cand_list=cands):
        d_out = hipbuf.alloc(shift + D * 8 + 64, fill=0x5A)
        assert d_out % 256 == 0                                                     # so d_out + 8 is 8-aligned and not 16-aligned
        got = eng.cancel(cand_list, d_out + shift, samples=samples, fmt=_fmt(fmt), want_amps=True)
        buf = hipbuf.download(d_out, shift + D * 8 + 64, np.uint8)
        assert (buf[:shift] == 0x5A).all() and (buf[shift + D * 8:] == 0x5A).all()  # nothing in front of the output, nothing behind it
        return got, buf[shift:shift + D * 8].view(np.complex64)

    ref, y_ref = run(d_x, 0)
    _check((fmt, drift, "five, aligned"), c, cands, ref, y_ref)
    for tag, samples, shift in (("input moved", d_pad + elem, 0), ("output moved", d_x, 8), ("both moved", d_pad + elem, 8)):
        got, y = run(samples, shift)
        assert (_words(y) == _words(y_ref)).all(), tag
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert g.keys() == r.keys()
            for k in r:
                assert np.asarray(g[k]).tobytes() == np.asarray(r[k]).tobytes(), (tag, k)
    # n_cands = 0 from the moved input, to both output forms: the converted dwell, exactly
    re, im = AM.as_parts(c["x"])
    for shift in (0, 8):
        got, y = run(d_pad + elem, shift, [])
        assert got == [] and (_words(y.real.copy()) == _words(re)).all() and (_words(y.imag.copy()) == _words(im)).all(), shift
    eng.close()


# ---- 2. a handle of another form ----------------------------------------------------------------------------------------------------
def test_a_padded_long_handle(gpu, oracle, hipbuf):
    """N = 4088 with any_length (padded long), coherent K = 3, M = 2, int8 IQ: nothing depends on the stage-C form"""
    from gnss_sdr_rs_amd import acquisition as A
    n = 4088
    c = AM.build_case(oracle.ca_code_table(), n, 0, 0)
    eng = A.AcquisitionEngine(c["fs"], 0.0, n, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=c["M"], codes=c["chips"],
                              code_rate=c["code_rate"], coherent_periods=c["K"], any_length=True)
    assert eng.plan_info()["form"] == "long_padded" and c["fmt"] == "i8" and eng.dwell_samples == c["dwell"]
    D = c["dwell"]
    cands = [_cand(0, AM.SAT_DOPPLER[0], n - 91.0)]
    d_x, d_out = hipbuf.upload(c["x"]), hipbuf.alloc(D * 8)
    got = eng.cancel(cands, d_out, samples=d_x, fmt=_fmt("i8"), want_amps=True)
    y = hipbuf.download(d_out, D * 8, np.complex64)
    want_y, want_a, want_b = CM.cancel_all(c["x"], c["chips"], cands, c["fs"], n, False)
    scale = float(np.abs(np.stack(AM.as_parts(c["x"]))).max())
    p = A.cancel_plan(D, n, cands[0]["code_phase"], 0.0)
    assert (p["bounds"].astype(np.int64) == want_b[0]).all() and got[0]["n_segments"] == len(want_a[0]) == 7
    yerr = max(np.abs(y.real - want_y.real).max(), np.abs(y.imag - want_y.imag).max())
    d = got[0]["amps"].astype(np.complex128) - want_a[0]
    aerr = max(np.abs(d.real).max(), np.abs(d.imag).max())
    print("4088 padded long: output within %.2e, amplitudes within %.2e of max |x|; |a| %.2f .. %.2f"
          % (yerr / scale, aerr / scale, np.abs(want_a[0]).min(), np.abs(want_a[0]).max()))
    assert yerr <= REL * scale and aerr <= REL * scale
    assert np.abs(want_a[0]).min() > 1.0                                            # the satellite is there: 60 dB-Hz
    eng.close()


# ---- 3. repetition, in place, the NULL route, the snapshot ---------------------------------------------------------------------------
def test_repetition_in_place_and_the_snapshot(gpu, oracle, hipbuf):
    c = _scene(oracle, "c32", True)
    D = c["dwell"]
    eng = _engine(c, M_PARITY, True)
    cands = _candidate_sets(D)["five"]
    d_x = hipbuf.upload(c["x"])
    run = lambda out, **kw: eng.cancel(cands, out, want_amps=True, **kw)

    def same(a, b):
        for u, v in zip(a, b):
            assert u.keys() == v.keys()
            for k in u:
                assert np.asarray(u[k]).tobytes() == np.asarray(v[k]).tobytes(), k

    d_1, d_2 = hipbuf.alloc(D * 8), hipbuf.alloc(D * 8)
    got_1 = run(d_1, samples=d_x, fmt=_fmt("c32"))
    got_2 = run(d_2, samples=d_x, fmt=_fmt("c32"))
    y_1 = _words(hipbuf.download(d_1, D * 8, np.complex64))
    assert (y_1 == _words(hipbuf.download(d_2, D * 8, np.complex64))).all()
    same(got_1, got_2)
    assert not (y_1 == _words(c["x"])).all()
    # in place
    d_z = hipbuf.upload(c["x"])
    same(got_1, run(d_z, samples=d_z, fmt=_fmt("c32")))
    assert (y_1 == _words(hipbuf.download(d_z, D * 8, np.complex64))).all()
    # the NULL route after a search_dev: the explicit pointer's words; the snapshot, the refinement and the metrics stay
    eng.search_dev(d_x, _fmt("c32"))
    metrics = [_words(a).copy() for a in eng.metrics()]
    am = eng.metrics()[1]
    res = [dict(doppler_bin=1, code_phase_samples=int(am[w, 1])) for w in range(AM.P)]
    refine = eng.refine_doppler(res, want_prompts=True, want_spectrum=True)
    d_3 = hipbuf.alloc(D * 8)
    same(got_1, run(d_3))
    assert (y_1 == _words(hipbuf.download(d_3, D * 8, np.complex64))).all()
    assert (_words(hipbuf.download(d_x, D * 8, np.complex64)) == _words(c["x"])).all()          # the input is only read
    same(refine, eng.refine_doppler(res, want_prompts=True, want_spectrum=True))
    for u, v in zip(metrics, [_words(a) for a in eng.metrics()]):
        assert (u == v).all()
    eng.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib
    from gnss_sdr_rs_amd._lib import GmError
    c = _scene(oracle, "c32", True)
    ci = _scene(oracle, "i8", True)
    D = c["dwell"]
    eng = _engine(c, M_PARITY, True)
    room = np.zeros(2 * D + 8 + 8 * D, np.int8)                  # an int8 IQ dwell with room for a c32 output right behind it
    room[:2 * D] = ci["x"].reshape(-1)
    d_x, d_i = hipbuf.upload(c["x"]), hipbuf.upload(room)
    d_out = hipbuf.alloc(D * 8, fill=0x5A)
    ok = (0, 0, F_STRONG, 700.25, CM.T_TRUE)
    Q = CM.plan(D, N, 700.25, CM.T_TRUE)["n_segments"]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(cands, samples=d_x, fmt=0, out_ptr=d_out, null=None, stride=Q, n=None):
        cs = (_lib.AcqCancelCand * max(len(cands), 1))(*[_lib.AcqCancelCand(*t) for t in cands])
        out = np.full(2 * C.sizeof(_lib.AcqCancelOut), 0xAB, np.uint8)
        amps = np.full(2 * Q, np.complex64(7 + 7j))
        st = _lib.lib().gm_acq_cancel(None if null == "handle" else eng._h, C.c_void_p(samples) if samples else None, fmt,
                                      None if null == "cands" else C.cast(cs, C.c_void_p), len(cands) if n is None else n,
                                      C.c_void_p(out_ptr) if out_ptr else None, vp(out), vp(amps), stride)
        host = bool((out == 0xAB).all() and (amps == np.complex64(7 + 7j)).all())
        return st, host, host and bool((hipbuf.download(d_out, D * 8, np.uint8) == 0x5A).all())

    nan = float("nan")
    bad = [dict(cands=[ok], null="handle"), dict(cands=[ok], null="cands"), dict(cands=[ok], out_ptr=None),
           dict(cands=[ok] * 65),                                                              # n_cands > 64
           dict(cands=[ok, (AM.P, 0, F_STRONG, 1.0, 0.0)]),                                    # worker >= P
           dict(cands=[ok, (0, 1, F_STRONG, 1.0, 0.0)]),                                       # reserved != 0
           dict(cands=[(0, 0, F_STRONG, -0.25, 0.0)]), dict(cands=[ok, (0, 0, F_STRONG, float(N), 0.0)]),
           dict(cands=[(0, 0, F_STRONG, nan, 0.0)]),                                           # cp
           dict(cands=[(0, 0, F_STRONG, 1.0, N - 8.1)]), dict(cands=[(0, 0, F_STRONG, 1.0, N + 8.1)]),
           dict(cands=[(0, 0, F_STRONG, 1.0, nan)]),                                           # T
           dict(cands=[(0, 0, nan, 1.0, 0.0)]), dict(cands=[(0, 0, FS, 1.0, 0.0)]), dict(cands=[(0, 0, -FS, 1.0, 0.0)]),   # f
           dict(cands=[ok], fmt=3), dict(cands=[ok], fmt=-1),                                  # not a format
           dict(cands=[ok], samples=None),                                                     # no search yet
           dict(cands=[ok], stride=Q - 1),                                                     # amps_stride below Q
           dict(cands=[ok], samples=d_out + 8), dict(cands=[ok], samples=d_out - 8),           # c32 ranges that overlap, not in place
           dict(cands=[ok], samples=d_out, fmt=_lib.FMT_I8_IQ),                                # the same pointer, but not c32
           dict(cands=[ok], samples=d_out + D * 8 - 2, fmt=_lib.FMT_I8_IQ),                    # the input's first sample is the output's last
           dict(cands=[ok], out_ptr=d_i + (2 * D - 8) // 8 * 8, samples=d_i, fmt=_lib.FMT_I8_IQ),   # the output's first is inside the input
           dict(cands=[ok], out_ptr=d_out + 4)]                                                # not aligned to a c32 sample
    for kw in bad:
        st, _, untouched = call(**kw)
        assert st == INVALID and untouched, kw
    assert (hipbuf.download(d_i, room.size, np.int8) == room).all()
    with pytest.raises(GmError) as e:
        eng.cancel([_cand(0, F_STRONG, 700.25)], d_out)                                        # the Python route: no search yet
    assert e.value.status == INVALID
    # ranges that only touch are fine, and so is a bad format without samples of the caller's once a search has run
    behind = 2 * D + (-2 * D) % 8
    st, host, _ = call([ok], out_ptr=d_i + behind, samples=d_i, fmt=_lib.FMT_I8_IQ)
    assert st == 0 and not host
    after = hipbuf.download(d_i, room.size, np.int8)
    assert (after[:behind] == room[:behind]).all() and after[behind:].any()
    eng.search_dev(d_x, _lib.FMT_C32)
    st, host, _ = call([ok, ok], samples=None, fmt=99)
    assert st == 0 and not host
    assert not (hipbuf.download(d_out, D * 8, np.uint8) == 0x5A).all()
    eng.close()


# ---- 5. the chain ------------------------------------------------------------------------------------------------------------------
def test_the_chain_brings_the_weak_satellite_out(gpu, oracle, hipbuf):
    """seed 100 of tests/test_acq_cancel_host.py's scene (accepted there: before 1644, after 1201), int8 IQ, K = 1, M = 12, T = N - 0.4"""
    from gnss_sdr_rs_amd import _lib
    r = scene_run(oracle, SEEDS[0])
    c = r["c"]
    assert r["weak_before"] not in CM.WEAK_PHASES and r["weak_after"] in CM.WEAK_PHASES
    eng = _engine(c, CM.PERIODS, True)
    eng.search(c["x"])
    mx, am, sm = eng.metrics()
    ds, strong_before = CM.best_cell(mx, sm, CM.STRONG["worker"])
    dw, _ = CM.best_cell(mx, sm, CM.WEAK["worker"])
    assert int(am[CM.WEAK["worker"], dw]) not in CM.WEAK_PHASES
    assert (ds, int(am[CM.STRONG["worker"], ds])) == (r["strong_bin"], r["strong_phase"])
    local = eng.local_search([dict(worker=CM.STRONG["worker"], doppler_bin=ds, code_phase_samples=int(am[CM.STRONG["worker"], ds]),
                                   offset_periods=0)], lag_half_window=CM.LOCAL_L, span_periods=CM.LOCAL_SPAN)
    cands = eng.cancel_cands_from_local(local, [CM.STRONG["worker"]])
    assert cands[0]["period_samples"] == CM.T_TRUE and cands[0]["worker"] == CM.STRONG["worker"]
    assert cands[0]["carrier_hz"] == pytest.approx(r["cand"]["carrier_hz"], abs=0.05)          # the model's parameters
    assert cands[0]["code_phase"] == pytest.approx(r["cand"]["code_phase"], abs=1e-3)
    d_out = hipbuf.alloc(c["dwell"] * 8)
    got = eng.cancel(cands, d_out)                                                             # the search's snapshot
    eng.search_dev(d_out, _lib.FMT_C32)
    mx2, am2, sm2 = eng.metrics()
    _, strong_after = CM.best_cell(mx2, sm2, CM.STRONG["worker"])
    dw2, weak_after = CM.best_cell(mx2, sm2, CM.WEAK["worker"])
    print("strong: peak-to-mean %.1f -> %.1f (model %.1f -> %.1f), amp_rms %.2f over %d segments; weak: arg-max %d -> %d, peak-to-mean "
          "%.1f after" % (strong_before, strong_after, r["strong_before"], r["strong_after"], got[0]["amp_rms"], got[0]["n_segments"],
                          int(am[CM.WEAK["worker"], dw]), int(am2[CM.WEAK["worker"], dw2]), weak_after))
    assert int(am2[CM.WEAK["worker"], dw2]) in CM.WEAK_PHASES
    assert strong_after < STRONG_AFTER_BOUND
    eng.close()
