"""The refusals that the six known-cell entries make in one shared host layer (CallBlock and what sits beside it, csrc/gm_api.hip):
gm_acq_refine_doppler, gm_acq_local_search, gm_acq_array_prompts, gm_acq_cancel, gm_trk_bank and gm_trk_array_prompts, and their six
gm_*_plan entries.  Each one's status AND the exact gm_last_error text, which the entries' own argument-error tests do not read.  The
texts are written out here; they are part of the behaviour, and a change to the shared layer must not move them.  Where two rules
are broken at once the text says which one the entry looks at first.

Shapes are those of the entries' argument-error tests: an acquisition handle at N = 2048, K = 3, M = 2, c32, two workers and three
bins for refine, local and the array prompts; the cancel scene's handle (K = 1, M = 6, the code drift on); a tracking handle of five
channels at fs = 2.048 MHz beside one ring block of 4096 samples and an array buffer of 3 x 2048 time samples.  One search per
acquisition handle, made after the no-search refusals.  Every case is refused before the device is touched: nothing is written, and
after each handle's walk one good call gives the bytes the first good call gave.  The gm_*_plan refusals need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import acq_cancel_model as CM
import acq_model as AM

INVALID, OUT_OF_RANGE = -1, -5
NULL_PTR, NO_SEARCH, BAD_FMT = "null pointer", "no search has run on this handle yet", "bad sample format"
CELL_RULES = [((AM.P, 1, 5, 0), "candidate.worker outside the handle's workers"),
              ((0, AM.D, 5, 0), "candidate.doppler_bin outside the handle's bins"),
              ((0, -1, 5, 0), "candidate.doppler_bin outside the handle's bins"),
              ((0, 1, 2048, 0), "candidate.code_phase_samples >= fft_size"),
              ((0, 1, 5, 1), "candidate.offset_periods above the edge search's last offset (0 without an edge search)")]
N_FREQ, HALF_SPAN = "n_freq must be odd, 3 .. 4097", "half_span_hz must lie in (0, fs / (2 fft_size)]"
SPAN_K = "span_periods must be 0 or coherent_periods on a coherent handle"
STATES_RULE = "states NULL: n_states must be n_channels"
SENT = np.complex64(7 + 7j)


def _last(lib):
    return (lib.gm_last_error() or b"").decode()


def _refused(lib, status, want_status, want_text, what):
    assert (status, _last(lib)) == (want_status, want_text), what


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Outputs:
    """sentinel-filled host outputs of one call; untouched() after a refusal, words() of a good call"""

    def __init__(self, **arrays):
        self.arrays = arrays
        self.fill = {k: a.copy() for k, a in arrays.items()}

    def untouched(self):
        return all(a.tobytes() == self.fill[k].tobytes() for k, a in self.arrays.items())

    def words(self):
        return b"".join(a.tobytes() for a in self.arrays.values())


# ---- gm_acq_refine_doppler, gm_acq_local_search, gm_acq_array_prompts: one handle, one search ---------------------------------------------
@pytest.mark.gpu
def test_refine_local_and_array_prompts_say_what_they_said(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    lib = gpu.lib()
    c = AM.build_case(oracle.ca_code_table(), 2048, 0, 2)             # coherent (K = 3, M = 2), c32, no edge search
    N, R_u, Z, W = c["N"], c["K"] * c["M"], 257, 7
    assert (N, c["fmt"], AM.P, AM.D) == (2048, "c32", 2, 3)
    eng = A.AcquisitionEngine(c["fs"], 0.0, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=c["M"], codes=c["chips"],
                              code_rate=c["code_rate"], coherent_periods=c["K"])
    d_x = hipbuf.upload(c["x"])
    rng = np.random.default_rng(9)
    n_arr, A_, L_ = int(eng.dwell_samples), 4, 2
    d_arr = hipbuf.upload((rng.standard_normal((n_arr, A_)) + 1j * rng.standard_normal((n_arr, A_))).astype(np.complex64))
    ok = (0, 1, 5, 0)

    def refine(results=((1, 5), (1, 7)), found=(1, 1), cfg=None, null=None, n_prn=None):
        res = (_lib.AcqResult * 3)()
        for r, (d, cp) in zip(res, results):
            r.doppler_bin, r.code_phase_samples = d, cp
        f = np.array(list(found) + [0], np.uint8)
        o = _Outputs(out=np.full(2 * C.sizeof(_lib.AcqRefineOut), 0xAB, np.uint8), z=np.full(2 * R_u, SENT), s=np.full(2 * Z, np.float32(7)))
        st = lib.gm_acq_refine_doppler(None if null == "handle" else eng._h, None if null == "results" else C.cast(res, C.c_void_p),
                                       None if null == "found" else _vp(f), len(results) if n_prn is None else n_prn,
                                       C.byref(_lib.AcqRefineCfg(*cfg)) if cfg else None, None if null == "out" else _vp(o.arrays["out"]),
                                       _vp(o.arrays["z"]), _vp(o.arrays["s"]))
        return st, o

    def local(cands=(ok, ok), cfg=(3, 0, 0, 0.0), samples=None, fmt=0, null=None):
        cs = (_lib.AcqCand * max(len(cands), 1))(*[_lib.AcqCand(*t) for t in cands])
        o = _Outputs(out=np.full(2 * C.sizeof(_lib.AcqLocalOut), 0xAB, np.uint8), z=np.full(2 * W * R_u, SENT),
                     s=np.full(2 * W * Z, np.float32(7)))
        st = lib.gm_acq_local_search(None if null == "handle" else eng._h, C.c_void_p(samples) if samples else None, fmt,
                                     None if null == "cands" else C.cast(cs, C.c_void_p), len(cands),
                                     C.byref(_lib.AcqLocalCfg(*cfg)) if cfg else None, None if null == "out" else _vp(o.arrays["out"]),
                                     _vp(o.arrays["z"]), _vp(o.arrays["s"]))
        return st, o

    def array(cands=(ok, ok), samples=d_arr, fmt=0, A=A_, L=L_, null=None, n=None):
        cs = (_lib.AcqCand * max(len(cands), 1))(*[_lib.AcqCand(*t) for t in cands])
        o = _Outputs(z=np.full(2 * R_u * 32, SENT))
        st = lib.gm_acq_array_prompts(None if null == "handle" else eng._h, None if null == "samples" else C.c_void_p(samples), fmt, A, L,
                                      None if null == "cands" else C.cast(cs, C.c_void_p), len(cands) if n is None else n,
                                      None if null == "z" else _vp(o.arrays["z"]))
        return st, o

    def walk(call, cases):
        for kw, text in cases:
            st, o = call(**kw)
            _refused(lib, st, INVALID, text, kw)
            assert o.untouched(), kw

    # no search yet: the snapshot rule of refine and of local's NULL route; the caller's samples need no snapshot, a bad format is refused
    walk(refine, [({}, NO_SEARCH), (dict(null="out"), NULL_PTR), (dict(n_prn=3), "n_prn exceeds the handle's workers")])
    walk(local, [({}, NO_SEARCH), (dict(fmt=7), NO_SEARCH), (dict(samples=d_x, fmt=3), BAD_FMT), (dict(null="cands"), NULL_PTR)])
    st, fresh = local(samples=d_x, fmt=_lib.FMT_C32)
    assert st == 0 and not fresh.untouched()
    eng.search(c["x"])
    first = {}
    for name, call in (("refine", refine), ("local", local), ("array", array)):
        st, o = call()
        assert st == 0 and not o.untouched(), name
        first[name] = o.words()
    assert first["local"] == fresh.words()                             # the snapshot holds the same samples

    walk(refine, [(dict(null=k), NULL_PTR) for k in ("handle", "results", "found", "out")] +
         [(dict(n_prn=3), "n_prn exceeds the handle's workers"),
          (dict(results=((1, 5), (AM.D, 7))), "result.doppler_bin outside the handle's bins"),
          (dict(results=((-1, 5), (1, 7))), "result.doppler_bin outside the handle's bins"),
          (dict(results=((1, 5), (1, N))), "result.code_phase_samples >= fft_size"),
          (dict(cfg=(2, 0, 0.0)), SPAN_K), (dict(cfg=(0, 64, 0.0)), N_FREQ), (dict(cfg=(0, 1, 0.0)), N_FREQ), (dict(cfg=(0, 4099, 0.0)), N_FREQ),
          (dict(cfg=(0, 0, 501.0)), HALF_SPAN), (dict(cfg=(0, 0, -1.0)), HALF_SPAN), (dict(cfg=(0, 0, math.nan)), HALF_SPAN),
          # the common rules first, then the results in their order, each one's own checks before its plan
          (dict(results=((AM.D, 5), (1, N)), cfg=(0, 64, 0.0)), N_FREQ),
          (dict(results=((1, N), (AM.D, 7))), "result.code_phase_samples >= fft_size"),
          (dict(results=((AM.D, N), (1, 7))), "result.doppler_bin outside the handle's bins")])
    st, o = refine(results=((99, N), (1, 7)), found=(0, 1))           # a not-found entry is not looked at
    assert st == 0 and o.arrays["out"].tobytes()[C.sizeof(_lib.AcqRefineOut):] == first["refine"][C.sizeof(_lib.AcqRefineOut):2 * C.sizeof(_lib.AcqRefineOut)]

    walk(local, [(dict(null=k), NULL_PTR) for k in ("handle", "cands", "out")] +
         [(dict(samples=d_x, fmt=3), BAD_FMT), (dict(samples=d_x, fmt=-1), BAD_FMT)] +
         [(dict(cands=(ok, cand)), text) for cand, text in CELL_RULES] +
         [(dict(cfg=(65, 0, 0, 0.0)), "lag_half_window > 64"), (dict(cfg=(3, 2, 0, 0.0)), SPAN_K), (dict(cfg=(3, 0, 64, 0.0)), N_FREQ),
          (dict(cfg=(3, 0, 0, 501.0)), HALF_SPAN), (dict(cfg=(3, 0, 0, math.nan)), HALF_SPAN),
          # the format before the common rules, those before any candidate, a candidate's cell rules before the next candidate's
          (dict(samples=d_x, fmt=3, cfg=(65, 0, 0, 0.0)), BAD_FMT),
          (dict(cands=((AM.P, 1, 5, 0), ok), cfg=(65, 0, 0, 0.0)), "lag_half_window > 64"),
          (dict(cands=((0, 1, N, 0), (AM.P, 1, 5, 0))), "candidate.code_phase_samples >= fft_size"),
          (dict(cands=((AM.P, AM.D, N, 1),)), "candidate.worker outside the handle's workers")])
    st, o = local(fmt=99)                                             # a bad format is not looked at without samples of the caller's
    assert st == 0 and o.words() == first["local"]

    array_fmt = "the array stream is GM_FMT_C32 or GM_FMT_I8_IQ"
    walk(array, [(dict(null=k), NULL_PTR) for k in ("handle", "samples", "cands", "z")] +
         [(dict(fmt=_lib.FMT_I8_REAL), array_fmt), (dict(fmt=3), array_fmt), (dict(fmt=-1), array_fmt),
          (dict(A=1), "n_antennas must be 2 .. 8"), (dict(L=9), "taps must be 1 .. 8"), (dict(A=5, L=7), "n_antennas * taps must not exceed 32"),
          (dict(n=1025), "n_cands > 1024")] +
         [(dict(cands=(ok, cand)), text) for cand, text in CELL_RULES] +
         [(dict(fmt=3, A=1), array_fmt), (dict(A=1, cands=((AM.P, 1, 5, 0),)), "n_antennas must be 2 .. 8"),
          (dict(n=1025, cands=((AM.P, 1, 5, 0),)), "n_cands > 1024"),
          (dict(cands=((0, 1, 5, 1), (AM.P, 1, 5, 0))), CELL_RULES[4][1])])

    for name, call in (("refine", refine), ("local", local), ("array", array)):
        st, o = call()
        assert st == 0 and o.words() == first[name], name
    eng.close()


# ---- gm_acq_cancel: the cancel scene's handle, one search ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cancel_says_what_it_said(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    lib = gpu.lib()
    c = CM.scene(oracle.ca_code_table(), 7, fmt="c32", periods=6, drift=True)
    N, FS, D = CM.N, CM.FS, c["dwell"]
    eng = A.AcquisitionEngine(FS, CM.F_IF, N, doppler_hz=AM.DOP, prn_ids=list(AM.PRN_IDS), n_integrations=6, codes=c["chips"],
                              code_rate=c["code_rate"])
    eng.set_code_drift(c["T"])
    assert eng.dwell_samples == D == len(c["x"])
    d_x = hipbuf.upload(c["x"])
    d_room = hipbuf.alloc(2 * D * 8, fill=0x5A)                       # the output is the second half: every input range below lies inside
    d_out = d_room + D * 8
    f = CM.F_IF + CM.STRONG["doppler"]
    ok = (0, 0, f, 700.25, CM.T_TRUE)
    Q = CM.plan(D, N, 700.25, CM.T_TRUE)["n_segments"]

    def cancel(cands=(ok,), samples=d_x, fmt=0, out_ptr=d_out, null=None, stride=Q, n=None):
        cs = (_lib.AcqCancelCand * max(len(cands), 1))(*[_lib.AcqCancelCand(*t) for t in cands])
        o = _Outputs(out=np.full(2 * C.sizeof(_lib.AcqCancelOut), 0xAB, np.uint8), amps=np.full(2 * Q, SENT))
        st = lib.gm_acq_cancel(None if null == "handle" else eng._h, C.c_void_p(samples) if samples else None, fmt,
                               None if null == "cands" else C.cast(cs, C.c_void_p), len(cands) if n is None else n,
                               C.c_void_p(out_ptr) if out_ptr else None, _vp(o.arrays["out"]), _vp(o.arrays["amps"]), stride)
        return st, o

    def walk(cases):
        for kw, text in cases:
            st, o = cancel(**kw)
            _refused(lib, st, INVALID, text, kw)
            assert o.untouched(), kw
        assert (hipbuf.download(d_room, 2 * D * 8, np.uint8) == 0x5A).all()

    overlap = "d_out overlaps the input (only d_out == the c32 input itself is allowed)"
    worker = "candidate.worker outside the handle's workers"
    walk([(dict(samples=None), NO_SEARCH), (dict(samples=None, fmt=7), NO_SEARCH), (dict(samples=None, n=65), "more than 64 candidates")])
    st, o = cancel()
    assert st == 0 and not o.untouched()
    first = o.words() + hipbuf.download(d_out, D * 8, np.uint8).tobytes()
    assert hipbuf.hip.hipMemset(d_room, 0x5A, 2 * D * 8) == 0 and hipbuf.hip.hipDeviceSynchronize() == 0
    eng.search_dev(d_x, _lib.FMT_C32)
    walk([(dict(null="handle"), NULL_PTR), (dict(null="cands"), NULL_PTR), (dict(out_ptr=None), NULL_PTR),
          (dict(n=65), "more than 64 candidates"), (dict(n=65, fmt=3), "more than 64 candidates"),
          (dict(fmt=3), BAD_FMT), (dict(fmt=-1), BAD_FMT),
          # the overlap rule reads the input's bytes per sample: its last sample on the output's first word, its first on the last
          (dict(samples=d_out - (D - 1) * 8), overlap), (dict(samples=d_out + D * 8 - 8), overlap),
          (dict(samples=d_out - (D - 1) * 2, fmt=_lib.FMT_I8_IQ), overlap), (dict(samples=d_out + D * 8 - 2, fmt=_lib.FMT_I8_IQ), overlap),
          (dict(samples=d_out - (D - 1), fmt=_lib.FMT_I8_REAL), overlap), (dict(samples=d_out + D * 8 - 1, fmt=_lib.FMT_I8_REAL), overlap),
          (dict(samples=d_out, fmt=_lib.FMT_I8_IQ), overlap),
          (dict(out_ptr=d_out + 4), "d_out is not aligned to a c32 sample"),
          # the overlap and the alignment before any candidate, a candidate's rules in their order, the stride behind them all
          (dict(samples=d_out + 8, cands=((AM.P, 0, f, 1.0, 0.0),)), overlap),
          (dict(out_ptr=d_out + 4, cands=((AM.P, 0, f, 1.0, 0.0),)), "d_out is not aligned to a c32 sample"),
          (dict(cands=(ok, (AM.P, 0, f, 1.0, 0.0))), worker), (dict(cands=((AM.P, 1, math.nan, -1.0, 0.0),)), worker),
          (dict(cands=(ok, (0, 1, f, 1.0, 0.0))), "candidate.reserved must be 0"),
          (dict(cands=((0, 0, FS, -1.0, 0.0),)), "candidate.carrier_hz is not a number or |carrier_hz| >= fs"),
          (dict(cands=((0, 0, f, float(N), 0.0),)), "code_phase outside [0, fft_size)"),
          (dict(cands=((0, 0, f, 1.0, N + 8.1),)), "period_samples not within 8 of fft_size (0: fft_size)"),
          (dict(stride=Q - 1), "amps_stride below the largest n_segments"),
          (dict(stride=Q - 1, cands=(ok, (AM.P, 0, f, 1.0, 0.0))), worker)])
    st, o = cancel()
    assert st == 0 and o.words() + hipbuf.download(d_out, D * 8, np.uint8).tobytes() == first
    eng.close()


# ---- gm_trk_bank and gm_trk_array_prompts: one handle, one ring block ---------------------------------------------------------------------
@pytest.mark.gpu
def test_bank_and_tracking_array_prompts_say_what_they_said(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, tracking as T
    lib = gpu.lib()
    n, A_, L_ = 2048, 4, 2
    fs, n_time = 1000.0 * n, 3 * n
    rng = np.random.default_rng(3)
    ring = T.MulticastRingBuffer(1 << 14)
    ring.write_samples((rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64))
    d_x = hipbuf.upload((rng.standard_normal((n_time, A_)) + 1j * rng.standard_normal((n_time, A_))).astype(np.complex64))
    mgr = T.TrackingManager(fs, n_channels=5, code_index_mode=T.CODE_INDEX_FIXED)
    rec = T.TrkState()
    rec.prn, rec.active, rec.next_sample_index, rec.num_samples_per_code = 3, 1, 100, n
    rec.carrier_freq, rec.carrier_phase, rec.code_phase, rec.code_rate = 250.0, 0.3, 0.0, 1.023e6
    taps = np.array([0.0, 0.5], np.float32)

    def bank(states=True, n_states=1, null=None, n_taps=2):
        cfg = _lib.TrkBankCfg()
        cfg.n_taps, cfg.n_offsets, cfg.taps_chips, cfg.offsets_hz = n_taps, 0, taps.ctypes.data, None
        o = _Outputs(out=np.full(5 * 2, SENT), done=np.full(5, 0x5A, np.uint8))
        arr = (T.TrkState * 1)(rec)
        st = lib.gm_trk_bank(None if null == "handle" else mgr._h, None if null == "ring" else ring._h,
                             C.cast(arr, C.c_void_p) if states else None, n_states, None if null == "cfg" else C.byref(cfg),
                             None if null == "out" else _vp(o.arrays["out"]), _vp(o.arrays["done"]))
        return st, o

    def array(states=True, n_states=1, null=None, fmt=0, first_index=0, n_time=n_time, A=A_):
        cfg = _lib.TrkArrayCfg()
        cfg.n_antennas, cfg.taps, cfg.tap_chips = A, L_, 0.0
        o = _Outputs(z=np.full(5 * A_ * L_, SENT), done=np.full(5, 0x5A, np.uint8))
        arr = (T.TrkState * 1)(rec)
        st = lib.gm_trk_array_prompts(None if null == "handle" else mgr._h, None if null == "samples" else C.c_void_p(d_x), fmt, first_index,
                                      n_time, C.cast(arr, C.c_void_p) if states else None, n_states, None if null == "cfg" else C.byref(cfg),
                                      None if null == "z" else _vp(o.arrays["z"]), _vp(o.arrays["done"]))
        return st, o

    def walk(call, cases):
        for kw, status, text in cases:
            st, o = call(**kw)
            _refused(lib, st, status, text, kw)
            assert o.untouched(), kw

    first = {}
    for name, call in (("bank", bank), ("array", array)):
        st, o = call()
        assert st == 0 and o.arrays["done"][0] == 1 and not o.untouched(), name
        first[name] = o.words()
    bank_null, array_null = "null handle, ring or out", "null handle, samples or z"
    walk(bank, [(dict(null=k), INVALID, bank_null) for k in ("handle", "ring", "out")] +
         [(dict(states=False, n_states=4), INVALID, STATES_RULE), (dict(states=False, n_states=1), INVALID, STATES_RULE),
          (dict(null="cfg"), INVALID, "null bank cfg"),
          (dict(n_states=0), OUT_OF_RANGE, "n_states must be in 1 .. 1024"), (dict(n_taps=0), OUT_OF_RANGE, "n_taps must be in 1 .. 64"),
          # the pointers, the count of a NULL states, the shared rules, the bank's own
          (dict(null="ring", states=False, n_states=4), INVALID, bank_null), (dict(null="cfg", states=False, n_states=4), INVALID, STATES_RULE),
          (dict(null="cfg", n_states=0), INVALID, "null bank cfg")])
    array_fmt, below = "fmt must be GM_FMT_C32 or GM_FMT_I8_IQ", "first_index + n_time must be below 2^62"
    walk(array, [(dict(null=k), INVALID, array_null) for k in ("handle", "samples", "z")] +
         [(dict(fmt=_lib.FMT_I8_REAL), INVALID, array_fmt), (dict(fmt=3), INVALID, array_fmt), (dict(fmt=-1), INVALID, array_fmt),
          (dict(states=False, n_states=4), INVALID, STATES_RULE), (dict(null="cfg"), INVALID, "null array cfg"),
          (dict(A=1), OUT_OF_RANGE, "n_antennas must be in 2 .. 8"), (dict(n_states=1025), OUT_OF_RANGE, "n_states must be in 1 .. 1024"),
          (dict(first_index=1 << 62), OUT_OF_RANGE, below), (dict(first_index=(1 << 62) - n_time), OUT_OF_RANGE, below),
          (dict(n_time=1 << 62), OUT_OF_RANGE, below), (dict(first_index=(1 << 64) - 1, n_time=2), OUT_OF_RANGE, below),
          # the format, the count of a NULL states, the shared rules, the array's own, the index range
          (dict(null="z", fmt=3), INVALID, array_null), (dict(fmt=3, states=False, n_states=4), INVALID, array_fmt),
          (dict(null="cfg", states=False, n_states=4), INVALID, STATES_RULE), (dict(null="cfg", first_index=1 << 62), INVALID, "null array cfg"),
          (dict(A=1, first_index=1 << 62), OUT_OF_RANGE, "n_antennas must be in 2 .. 8")])
    st, o = array(first_index=(1 << 62) - n_time - 1)                 # the largest range that is allowed: the record lies in front of it
    assert st == 0 and o.arrays["done"][0] == 0 and not o.arrays["z"][:A_ * L_].any()
    for name, call in (("bank", bank), ("array", array)):
        st, o = call(states=False, n_states=5)                        # the handle's own channels: none is active, all are skipped
        assert st == 0 and not o.arrays["done"].any(), name
        st, o = call()
        assert st == 0 and o.words() == first[name], name
    mgr.close()
    ring.close()


# ---- the six plan entries: host only ------------------------------------------------------------------------------------------------------
def test_every_plan_refusal_says_what_it_said(gm):
    from gnss_sdr_rs_amd import _lib
    lib = gm.lib()
    tf = np.array([-300.0, 0.0, 300.0], np.float32)
    u = [C.c_uint32(77) for _ in range(4)]
    dbl = [C.c_double(77.0) for _ in range(2)]
    fs, N = 2.048e6, 2048
    required = "n_integrations, fft_size, n_bins, table_freq and fs are required"

    def refine(K=3, M=2, cfg=(0, 0, 0.0), fs=fs, N=N, D=3, table=tf, d=1):
        return lib.gm_acq_refine_plan(K, M, C.byref(_lib.AcqRefineCfg(*cfg)) if cfg else None, fs, N, D, _vp(table) if table is not None else None,
                                      d, C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), C.byref(dbl[0]), C.byref(dbl[1]))

    def local(K=3, M=2, cfg=(3, 0, 0, 0.0), fs=fs, N=N, D=3, table=tf, d=1):
        return lib.gm_acq_local_plan(K, M, C.byref(_lib.AcqLocalCfg(*cfg)) if cfg else None, fs, N, D, _vp(table) if table is not None else None,
                                     d, C.byref(u[3]), C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), C.byref(dbl[0]), C.byref(dbl[1]))

    grid = [(dict(K=33), "coherent_periods > 32"), (dict(M=0), required), (dict(N=0), required), (dict(D=0), required), (dict(table=None), required),
            (dict(fs=0.0), required), (dict(fs=math.nan), required), (dict(d=3), "doppler bin outside the handle's bins"),
            (dict(K=1, M=1), "the fine Doppler needs at least 2 periods per group (one period carries no frequency information)"),
            (dict(K=33, M=0), "coherent_periods > 32"), (dict(M=0, d=3), required)]
    for kw, text in grid + [(dict(cfg=(2, 0, 0.0)), SPAN_K), (dict(K=1, M=4, cfg=(5, 0, 0.0)), "span_periods exceeds n_integrations"),
                            (dict(cfg=(0, 64, 0.0)), N_FREQ), (dict(cfg=(0, 0, 501.0)), HALF_SPAN), (dict(d=3, cfg=(0, 64, 0.0)), "doppler bin outside the handle's bins")]:
        _refused(lib, refine(**kw), INVALID, text, kw)
    for kw, text in grid + [(dict(cfg=(3, 2, 0, 0.0)), SPAN_K), (dict(cfg=(3, 0, 64, 0.0)), N_FREQ), (dict(cfg=(3, 0, 0, 501.0)), HALF_SPAN),
                            (dict(cfg=(65, 0, 0, 0.0)), "lag_half_window > 64"), (dict(cfg=(65, 0, 64, 0.0)), N_FREQ),
                            (dict(N=64, fs=64000.0, cfg=(32, 0, 0, 0.0)), "the lag window (2 lag_half_window + 1) exceeds fft_size")]:
        _refused(lib, local(**kw), INVALID, text, kw)

    array = lambda K=3, M=2, A=4, L=2: lib.gm_acq_array_plan(K, M, A, L, C.byref(u[0]), C.byref(u[1]))
    for kw, text in [(dict(K=33), "coherent_periods > 32"), (dict(M=0), "n_integrations is required"), (dict(A=1), "n_antennas must be 2 .. 8"),
                     (dict(A=9), "n_antennas must be 2 .. 8"), (dict(L=0), "taps must be 1 .. 8"), (dict(L=9), "taps must be 1 .. 8"),
                     (dict(A=5, L=7), "n_antennas * taps must not exceed 32"),
                     (dict(K=32, M=1 << 24, A=8, L=4), "periods * taps * n_antennas does not fit 32 bits"), (dict(M=0, A=1), "n_integrations is required")]:
        _refused(lib, array(**kw), INVALID, text, kw)

    bounds = np.full(16, 77, np.uint64)
    cancel = lambda D=12286, N=N, cp=700.25, T=0.0, cap=16: lib.gm_acq_cancel_plan(D, N, cp, T, C.byref(u[0]), _vp(bounds), cap)
    for kw, text in [(dict(N=15), "fft_size below 16"), (dict(D=0), "dwell_samples is 0 or above 2^40"), (dict(D=(1 << 40) + 1), "dwell_samples is 0 or above 2^40"),
                     (dict(D=1 << 40, N=16), "dwell_samples holds more than 2^24 code periods"), (dict(cp=-0.25), "code_phase outside [0, fft_size)"),
                     (dict(cp=float(N)), "code_phase outside [0, fft_size)"), (dict(cp=math.nan), "code_phase outside [0, fft_size)"),
                     (dict(T=N + 8.1), "period_samples not within 8 of fft_size (0: fft_size)"), (dict(T=math.nan), "period_samples not within 8 of fft_size (0: fft_size)"),
                     (dict(cap=6), "bounds_cap below n_segments + 1"), (dict(N=15, D=0), "fft_size below 16")]:
        _refused(lib, cancel(**kw), INVALID, text, kw)

    def trk(fs=fs, codes=False, n_codes=0, code_len=0):
        cfg = _lib.TrkCfg()
        cfg.fs, cfg.n_channels, cfg.n_arms = fs, 5, 3
        keep = np.ones((max(n_codes, 1), max(code_len, 1)), np.int8)
        cfg.codes, cfg.n_codes, cfg.code_len = (keep.ctypes.data if codes else None), n_codes, code_len
        return cfg, keep

    taps = np.zeros(2, np.float32)

    def bank(n_states=1, null=None, n_taps=2, **kw):
        t, keep = trk(**kw)
        cfg = _lib.TrkBankCfg()
        cfg.n_taps, cfg.taps_chips = n_taps, taps.ctypes.data
        out = _lib.TrkBankPlanOut()
        out.n_taps = 77
        st = lib.gm_trk_bank_plan(None if null == "trk" else C.byref(t), None if null == "cfg" else C.byref(cfg), n_states, C.byref(out))
        return st, out.n_taps == 77

    def tarray(n_states=1, null=None, A=4, **kw):
        t, keep = trk(**kw)
        cfg = _lib.TrkArrayCfg()
        cfg.n_antennas, cfg.taps = A, 2
        out = _lib.TrkArrayPlanOut()
        out.words_per_record = 77
        st = lib.gm_trk_array_plan(None if null == "trk" else C.byref(t), None if null == "cfg" else C.byref(cfg), n_states, C.byref(out))
        return st, out.words_per_record == 77

    shared = [(dict(null="trk"), "null tracking cfg"), (dict(fs=0.0), "fs is required"), (dict(fs=-1.0), "fs is required"),
              (dict(fs=math.nan), "fs is required"), (dict(fs=math.inf), "fs is required"),
              (dict(codes=True, n_codes=0, code_len=100), "n_codes/code_len required"), (dict(codes=True, n_codes=1, code_len=0), "n_codes/code_len required"),
              (dict(fs=0.0, codes=True), "fs is required")]                 # in their order
    for name, plan, own in (("bank", bank, dict(n_taps=0)), ("array", tarray, dict(A=1))):
        null_cfg = "null %s cfg" % name
        for kw, text in shared + [(dict(null="cfg"), null_cfg), (dict(null="cfg", fs=0.0), null_cfg), (dict(fs=0.0, **own), "fs is required"),
                                  (dict(codes=True, **own), "n_codes/code_len required")]:
            st, untouched = plan(**kw)
            _refused(lib, st, INVALID, text, (name, kw))
            assert untouched, (name, kw)
        st, untouched = plan(**own)                                   # each one's own rules behind the shared ones
        _refused(lib, st, OUT_OF_RANGE, "n_taps must be in 1 .. 64" if name == "bank" else "n_antennas must be in 2 .. 8", (name, own))
        st, untouched = plan(codes=True, n_codes=1, code_len=16385)
        _refused(lib, st, OUT_OF_RANGE, "the %s of at most 16384 chips" % ("bank serves codes" if name == "bank" else "array prompts serve codes"), name)
        st, untouched = plan()
        assert st == 0 and not untouched, name
    assert [v.value for v in u] == [77] * 4 and [v.value for v in dbl] == [77.0] * 2 and (bounds == 77).all()      # nothing written
    assert refine() == 0 and (u[0].value, u[1].value, u[2].value) == (3, 2, 257)
    assert cancel() == 0 and u[0].value == 7
