"""Mirror of the reference's acquisition API over the C ABI (names follow
src/acquisition/do_acquisition.rs and src/acquisition/doppler_shift.rs)."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import AcqCancelCand, AcqCancelOut, AcqCand, AcqCfg, AcqLocalCfg, AcqLocalOut, AcqPlan, AcqRefineCfg, AcqRefineOut, AcqResult, ArrayRowInfo, ArraySolveCfg, FMT_C32, FMT_I8_IQ, FMT_I8_REAL, check, lib

PRN_SEARCH_ACQUISITION_TOTAL = 32      # do_acquisition.rs:22
FREQ_SEARCH_ACQUISITION_HZ = 14e3      # :20
FREQ_SEARCH_STEP_HZ = 500              # :21
LONG_SAMPLES_LENGTH = 10               # :23


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cand_array(cands):
    """the gm_acq_cand array of local_search's candidate dicts (one spare entry for an empty list: the pointer is never null)"""
    cs = (AcqCand * max(len(cands), 1))()
    for i, c in enumerate(cands):
        cs[i] = AcqCand(int(c["worker"]), int(c["doppler_bin"]), int(c["code_phase_samples"]), int(c.get("offset_periods", 0)))
    return cs


def generate_ca_code_samples(prn, code_rate, f_sampling):
    """utilities::ca_code::generate_ca_code_samples (ca_code.rs:12-27)"""
    n = C.c_size_t(0)
    st = lib().gm_generate_ca_code_samples(prn, code_rate, f_sampling, None, 0, C.byref(n))
    check(st, "generate_ca_code_samples")
    out = np.zeros(n.value, np.int8)
    check(lib().gm_generate_ca_code_samples(prn, code_rate, f_sampling, _p(out), out.size, C.byref(n)),
          "generate_ca_code_samples")
    return out


def ca_code_table():
    t = np.zeros((32, 1023), np.int8)
    for r in range(32):
        check(lib().gm_ca_code_row(r, _p(t[r])), "gm_ca_code_row")
    return t


class DopplerShiftTable:
    """doppler_shift.rs:5-22: pub doppler_freq_hz (= IF + Doppler), pub table"""

    def __init__(self, f_if, doppler_freq_hz, fs, num_samples):
        self.table = np.zeros(num_samples, np.complex64)
        f = C.c_float(0)
        check(lib().gm_doppler_table_new(f_if, doppler_freq_hz, fs, num_samples, C.byref(f), _p(self.table)),
              "DopplerShiftTable::new")
        self.doppler_freq_hz = f.value


def apply_doppler_shift(samples, doppler_table, output):
    """doppler_shift.rs:25-40 (GPU)"""
    s = np.ascontiguousarray(samples, np.complex64)
    t = doppler_table.table if isinstance(doppler_table, DopplerShiftTable) else np.ascontiguousarray(doppler_table, np.complex64)
    assert output.dtype == np.complex64 and output.flags.c_contiguous and t.size >= s.size
    _lib.init(_lib._initialised or 0)
    check(lib().gm_apply_doppler_shift(_p(s), _p(t), _p(output), s.size), "apply_doppler_shift")
    return output


def doppler_grid(span_hz=FREQ_SEARCH_ACQUISITION_HZ, step_hz=FREQ_SEARCH_STEP_HZ):
    """run()'s bin list: -span/2 + i*step, i = 0..span/step (do_acquisition.rs:248,253-255)"""
    capacity = int(span_hz) // int(step_hz) + 1
    return np.array([np.float32(-span_hz / 2.0) + np.float32(i) * np.float32(step_hz) for i in range(capacity)], np.float32)


def b1i_codes(prns=range(1, 38), n_chips=2046):
    """BeiDou B1I ranging codes (BDS-SIS-ICD-B1I 11-stage Gold codes) as an int8 [len(prns)][n_chips] table of +-1."""
    prns = list(prns)
    t = np.zeros((len(prns), n_chips), np.int8)
    for i, p in enumerate(prns):
        check(lib().gm_b1i_code(int(p), _p(t[i]), n_chips), "gm_b1i_code")
    return t


DECIDE_REFERENCE, DECIDE_BEST_BIN = 0, 1   # gm_decision_mode
ACQ_FORMS = {0: "lds", 1: "composite", 2: "long", 3: "long_padded"}   # gm_acq_form


def plan_info(fft_size, any_length=False):
    """gm_acq_plan_info: (status, dict(form, base, q, transform_len)) — the path gm_acq_create takes for this fft_size
    (status 0), or the status it returns (the dict is then None).  Host only, no device needed."""
    o = AcqPlan()
    st = lib().gm_acq_plan_info(int(fft_size), int(bool(any_length)), C.byref(o))
    if st:
        return st, None
    return st, dict(form=ACQ_FORMS[o.form], base=int(o.base), q=int(o.q), transform_len=int(o.transform_len))


def detection_threshold(n_integrations, n_cells, pfa):
    """The smallest ratio t with n_cells * Q(M, t M) <= pfa, M = n_integrations: the ratio test's threshold for a grid of n_cells cells
    (PRNs x bins x fft_size) and a false-alarm probability pfa per search.  After the coherent fold a noise cell's accumulated power
    is Gamma(M) distributed whatever coherent_periods is, and Q(M, x) = exp(-x) sum_{i<M} x^i / i! is its survival function at
    x = t M (the plane mean estimates the noise power).  Pure Python (bisection to 1e-9)."""
    M, n_cells, pfa = int(n_integrations), float(n_cells), float(pfa)
    if M < 1 or n_cells <= 0 or not 0.0 < pfa:
        raise ValueError("n_integrations >= 1, n_cells > 0, pfa > 0")

    def q(t):
        x = t * M
        term, s = 1.0, 1.0
        for i in range(1, M):
            term *= x / i
            s += term
        return math.exp(-x) * s

    lo, hi = 0.0, 1.0
    while n_cells * q(hi) > pfa:
        lo, hi = hi, hi * 2.0
    while hi - lo > 1e-9 * hi:
        mid = 0.5 * (lo + hi)
        if n_cells * q(mid) > pfa:
            lo = mid
        else:
            hi = mid
    return hi


# BeiDou B1I's Neumann-Hoffman secondary code (BDS-SIS-ICD-B1I: 0 0 0 0 0 1 0 0 1 1 0 1 0 1 0 0 1 1 1 0 on the 1 ms periods of one
# 20 ms data bit; 0 <-> +1 as in b1i_codes): the `secondary` row of set_edge_search for coherent_periods = 20
NH20 = np.array([1 - 2 * b for b in (0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0)], np.int8)


def edge_dwell_periods(coherent_periods, n_integrations, offsets, secondary=None):
    """gm_acq_edge_dwell_periods: K * M + offsets[-1] after the argument checks of set_edge_search (GmError INVALID_ARG).  Host only."""
    off = np.ascontiguousarray(offsets, np.uint32)
    sec = None if secondary is None else np.ascontiguousarray(secondary, np.int8)
    out = C.c_uint64(0)
    check(lib().gm_acq_edge_dwell_periods(int(coherent_periods), int(n_integrations), off.size, _p(off),
                                          _p(sec) if sec is not None else None, C.byref(out)), "gm_acq_edge_dwell_periods")
    return out.value


def code_period_samples(fs, code_len, code_rate, doppler_hz=0.0, carrier_hz=None):
    """The true code period in samples, fs * code_len / code_rate / (1 + doppler_hz / carrier_hz): what set_code_drift takes per bin.
    carrier_hz None: without the Doppler factor (the geometry alone, e.g. 16367.6 at fs = 16.3676 MHz).  Scalars or arrays, float64."""
    t = np.float64(fs) * np.float64(code_len) / np.float64(code_rate)
    if carrier_hz is None:
        return t + 0.0 * np.asarray(doppler_hz, np.float64)
    return t / (1.0 + np.asarray(doppler_hz, np.float64) / np.float64(carrier_hz))


def code_drift_plan(fft_size, n_periods, period_samples):
    """gm_acq_code_drift_plan: (starts [D][n_periods] uint64, dwell_samples) with starts[d][p] = floor(p * T_d + 0.5) in float64 and
    dwell_samples = max_d starts[d][-1] + fft_size, after the argument checks of set_code_drift (GmError INVALID_ARG).  Host only."""
    t = np.ascontiguousarray(period_samples, np.float64).reshape(-1)
    starts = np.zeros((t.size, int(n_periods)), np.uint64)
    out = C.c_uint64(0)
    check(lib().gm_acq_code_drift_plan(int(fft_size), int(n_periods), t.size, _p(t) if t.size else None, _p(starts), C.byref(out)),
          "gm_acq_code_drift_plan")
    return starts, out.value


def refine_plan(coherent_periods, n_integrations, fs, fft_size, table_freq, bin=0, span_periods=0, n_freq=0, half_span_hz=0.0):
    """gm_acq_refine_plan: what refine_doppler would use for Doppler bin `bin` of a handle with these settings, after its argument
    checks (GmError INVALID_ARG) -> dict(span_periods, n_groups, n_freq, half_span_hz, step_hz); a dwell yields span_periods * n_groups
    prompts per satellite.  Host only."""
    tf = np.ascontiguousarray(table_freq, np.float32).reshape(-1)
    cfg = AcqRefineCfg(int(span_periods), int(n_freq), float(half_span_hz))
    j, g, z = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    hs, st = C.c_double(0), C.c_double(0)
    check(lib().gm_acq_refine_plan(int(coherent_periods), int(n_integrations), C.byref(cfg), float(fs), int(fft_size), tf.size,
                                   _p(tf) if tf.size else None, int(bin), C.byref(j), C.byref(g), C.byref(z), C.byref(hs),
                                   C.byref(st)), "gm_acq_refine_plan")
    return dict(span_periods=j.value, n_groups=g.value, n_freq=z.value, half_span_hz=hs.value, step_hz=st.value)


def local_plan(coherent_periods, n_integrations, fs, fft_size, table_freq, bin=0, lag_half_window=0, span_periods=0, n_freq=0,
               half_span_hz=0.0):
    """gm_acq_local_plan: what local_search would use for Doppler bin `bin` of a handle with these settings, after its argument checks
    (GmError INVALID_ARG) -> dict(n_lags, span_periods, n_groups, n_freq, half_span_hz, step_hz): refine_plan's rules plus the lag
    window's (lag_half_window 0 .. 64, 2 lag_half_window + 1 <= fft_size).  Host only."""
    tf = np.ascontiguousarray(table_freq, np.float32).reshape(-1)
    cfg = AcqLocalCfg(int(lag_half_window), int(span_periods), int(n_freq), float(half_span_hz))
    w, j, g, z = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    hs, st = C.c_double(0), C.c_double(0)
    check(lib().gm_acq_local_plan(int(coherent_periods), int(n_integrations), C.byref(cfg), float(fs), int(fft_size), tf.size,
                                  _p(tf) if tf.size else None, int(bin), C.byref(w), C.byref(j), C.byref(g), C.byref(z), C.byref(hs),
                                  C.byref(st)), "gm_acq_local_plan")
    return dict(n_lags=w.value, span_periods=j.value, n_groups=g.value, n_freq=z.value, half_span_hz=hs.value, step_hz=st.value)


def array_plan(coherent_periods, n_integrations, n_antennas, taps=1):
    """gm_acq_array_plan: the argument rules of array_prompts (n_antennas 2 .. 8, taps 1 .. 8, n_antennas * taps <= 32; GmError
    INVALID_ARG) -> dict(periods = R_u = max(1, coherent_periods) * n_integrations, words_per_cand = R_u * taps * n_antennas).  Host only."""
    r, w = C.c_uint32(0), C.c_uint32(0)
    check(lib().gm_acq_array_plan(int(coherent_periods), int(n_integrations), int(n_antennas), int(taps), C.byref(r), C.byref(w)),
          "gm_acq_array_plan")
    return dict(periods=r.value, words_per_cand=w.value)


def solve_row(z, R=None, loading=0.0):
    """gm_array_row_solve for one cell: z complex64 [n, m] prompt vectors (array_prompts' [R_u, L, A] of a candidate goes in as it
    comes out), R complex64 [n_blocks, m, m] or [m, m] as Stap.capture / Beamformer.capture write it, or None: the identity.
    -> (row complex64 [m], dict(lambda1, lambda2, ref_index)).  Host only, float64 inside; the library judges nothing."""
    z = np.ascontiguousarray(z, np.complex64)
    if z.ndim < 2:
        raise ValueError("z must be [n, m] or [n, L, A]")
    z = z.reshape(z.shape[0], -1)
    n, m = z.shape
    Rp, nb = None, 0
    if R is not None:
        R = np.ascontiguousarray(R, np.complex64)
        if R.size % (m * m) or R.shape[-2:] != (m, m):
            raise ValueError("R must be [n_blocks, m, m] with m = %d" % m)
        nb, Rp = R.size // (m * m), _p(R)
    row = np.zeros(m, np.complex64)
    info = ArrayRowInfo()
    check(lib().gm_array_row_solve(m, n, _p(z) if z.size else None, Rp, nb, float(loading), _p(row), C.byref(info)), "gm_array_row_solve")
    return row, info.as_dict()


def _solve_cfg(m, n, n_rows, n_blocks, row_stride, vec_stride, loading):
    return ArraySolveCfg(int(m), int(n), int(n_rows), int(n_blocks), int(row_stride), int(vec_stride), float(loading))


def solve_plan(m, n, n_rows, n_blocks=0, row_stride=0, vec_stride=0, loading=0.0):
    """gm_array_solve_plan: the argument rules of solve_rows_dev (GmError INVALID_ARG) -> dict(z_words, R_words, row_words): the
    complex64 words the call reads at d_z and d_R and writes at d_rows.  Host only."""
    cfg = _solve_cfg(m, n, n_rows, n_blocks, row_stride, vec_stride, loading)
    z, r, w = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().gm_array_solve_plan(C.byref(cfg), C.byref(z), C.byref(r), C.byref(w)), "gm_array_solve_plan")
    return dict(z_words=z.value, R_words=r.value, row_words=w.value)


def solve_rows_dev(m, n, n_rows, d_z, d_rows, d_info, d_R=None, n_blocks=0, row_stride=0, vec_stride=0, loading=0.0, stream=None):
    """gm_array_rows_solve_dev: solve_row for n_rows rows in one launch on the device, asynchronously on `stream` (None: the null
    stream).  Device pointers: d_z (vector i of row p at d_z + p * row_stride + i * vec_stride complex64 words; 0, 0: the dense
    [n_rows, n, m]), d_R [n_blocks, m, m] or None with n_blocks = 0, d_rows complex64 [n_rows, m], d_info [n_rows] ArrayRowInfo whose
    `reserved` holds the row's status (0: solved)."""
    cfg = _solve_cfg(m, n, n_rows, n_blocks, row_stride, vec_stride, loading)
    check(lib().gm_array_rows_solve_dev(C.byref(cfg), C.c_void_p(d_z), C.c_void_p(d_R), C.c_void_p(d_rows), C.c_void_p(d_info),
                                        C.c_void_p(stream)), "gm_array_rows_solve_dev")


def solve_rows(z, R=None, loading=0.0):
    """solve_row for every candidate of array_prompts' result: z complex64 [n_cands, R_u, L, A] -> (rows complex64 [n_cands, L, A],
    list of dict(lambda1, lambda2, ref_index)); R as solve_row takes it, shared by the candidates."""
    z = np.ascontiguousarray(z, np.complex64)
    if z.ndim != 4:
        raise ValueError("z must be [n_cands, R_u, L, A]")
    rows, infos = np.zeros((z.shape[0],) + z.shape[2:], np.complex64), []
    for c in range(z.shape[0]):
        row, info = solve_row(z[c], R, loading)
        rows[c] = row.reshape(z.shape[2:])
        infos.append(info)
    return rows, infos


def cancel_plan(dwell_samples, fft_size, code_phase, period_samples=0.0):
    """gm_acq_cancel_plan: the signal code periods ("segments") gm_acq_cancel cuts a dwell of dwell_samples samples into for a
    satellite whose code starts code_phase samples into the dwell and repeats every period_samples samples (0: fft_size), after its
    argument checks (GmError INVALID_ARG) -> dict(n_segments = Q, bounds = uint64 [Q + 1]: segment k is bounds[k] <= n < bounds[k + 1]).
    Host only."""
    q = C.c_uint32(0)
    check(lib().gm_acq_cancel_plan(int(dwell_samples), int(fft_size), float(code_phase), float(period_samples), C.byref(q), None, 0),
          "gm_acq_cancel_plan")
    b = np.zeros(q.value + 1, np.uint64)
    check(lib().gm_acq_cancel_plan(int(dwell_samples), int(fft_size), float(code_phase), float(period_samples), C.byref(q), _p(b),
                                   b.size), "gm_acq_cancel_plan")
    return dict(n_segments=q.value, bounds=b)


class AcquisitionEngine:
    """The batched replacement of `workers.par_iter_mut()` (do_acquisition.rs:268-271, 302-313):
    all AcquisitionWorkers of one stage in one handle."""

    def __init__(self, fs, f_if, fft_size, doppler_hz=None, prn_ids=None, n_integrations=LONG_SAMPLES_LENGTH,
                 tables=None, codes=None, code_rate=1.023e6, threshold=7.0, decision_mode=0, strict_sum_order=False, reference_products=False,
                 device=None, any_length=False, coherent_periods=1):
        _lib.init(device if device is not None else (_lib._initialised or 0))
        self.fs, self.f_if, self.fft_size, self.M = float(fs), float(f_if), int(fft_size), int(n_integrations)
        self.prn_ids = np.ascontiguousarray(prn_ids if prn_ids is not None else np.arange(1, 33), np.uint8)
        cfg = AcqCfg()
        cfg.fs, cfg.f_if, cfg.fft_size, cfg.n_integrations = self.fs, self.f_if, self.fft_size, self.M
        keep = []
        if tables is not None:   # &[DopplerShiftTable] built by the caller
            tb = np.ascontiguousarray(np.stack([t.table for t in tables]), np.complex64)
            tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
            cfg.tables, cfg.table_freq, cfg.n_bins = tb.ctypes.data, tf.ctypes.data, len(tables)
            keep += [tb, tf]
        else:
            dh = np.ascontiguousarray(doppler_hz if doppler_hz is not None else doppler_grid(), np.float32)
            cfg.doppler_hz, cfg.n_bins = dh.ctypes.data, dh.size
            keep.append(dh)
        self.D = int(cfg.n_bins)
        cfg.n_prn, cfg.prn_ids = self.prn_ids.size, self.prn_ids.ctypes.data
        if codes is not None:
            cd = np.ascontiguousarray(codes, np.int8)
            assert cd.ndim == 2 and cd.shape[0] == self.prn_ids.size
            cfg.codes, cfg.code_len, cfg.code_rate = cd.ctypes.data, cd.shape[1], code_rate
            keep.append(cd)
        cfg.threshold = threshold
        cfg.decision_mode = decision_mode
        cfg.strict_sum_order = int(bool(strict_sum_order))
        cfg.reference_products = int(bool(reference_products))
        cfg.any_length = int(bool(any_length))      # every multiple of 8 in [1024, 2^18] (gm_acq_cfg.any_length)
        self.any_length = bool(any_length)
        # K code periods integrated coherently (gm_acq_cfg.coherent_periods): a dwell is K * M periods, M groups of K folded per bin
        cfg.coherent_periods = int(coherent_periods)
        self.K = max(1, int(coherent_periods))
        self.P = int(cfg.n_prn)
        h = C.c_void_p()
        check(lib().gm_acq_create(C.byref(cfg), C.byref(h)), "gm_acq_create")
        self._h = h
        self.code_drift = None        # set_code_drift: the per-bin code periods while the compensation is on
        self.edge_offsets = None      # set_edge_search: the period offsets of the hypotheses while the edge search is on
        self.table_freq = np.zeros(self.D, np.float32)
        check(lib().gm_acq_tables(self._h, None, _p(self.table_freq)), "gm_acq_tables")

    def plan_info(self):
        """The path this handle's fft_size runs on: dict(form, base, q, transform_len) (module-level plan_info)."""
        st, info = plan_info(self.fft_size, self.any_length)
        check(st, "gm_acq_plan_info")
        return info

    def close(self):
        if getattr(self, "_h", None):
            lib().gm_acq_destroy(self._h)
            self._h = None

    def __del__(self):      # (at interpreter shutdown the module globals close() uses may be gone already)
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _fmt(samples):
        a = np.asarray(samples)
        if a.dtype == np.int8:
            if a.ndim == 2 and a.shape[1] == 2:
                return np.ascontiguousarray(a), FMT_I8_IQ, a.shape[0]
            return np.ascontiguousarray(a), FMT_I8_REAL, a.size
        a = np.ascontiguousarray(a, np.complex64)
        return a, FMT_C32, a.size

    # ---- edge search (gm_acq_set_edge_search): hypotheses about where the coherent groups start, with a secondary code's signs
    def set_edge_search(self, offsets, secondary=None):
        """H ascending period offsets (1 <= H <= 32, each 0..63) and an optional row of K entries +-1 (e.g. NH20 at K = 20); an empty
        list switches the search off.  While it is on a dwell is `dwell_samples` long and the result dicts gain `edge_offset_periods`:
        the offset of the hypothesis the winning bin chose."""
        off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
        sec = None
        if secondary is not None:
            sec = np.ascontiguousarray(secondary, np.int8).reshape(-1)
            if sec.size != self.K:
                raise ValueError("secondary needs coherent_periods entries")
        check(lib().gm_acq_set_edge_search(self._h, off.size, _p(off) if off.size else None, _p(sec) if sec is not None else None),
              "gm_acq_set_edge_search")
        self.edge_offsets = off.copy() if off.size else None

    @property
    def dwell_samples(self):
        """Samples every entry that takes a dwell counts (gm_acq_dwell_samples): K * M * N, plus the last offset's periods while the
        edge search is on; up to the end of the last compensated period while the code drift is set."""
        out = C.c_uint64(0)
        check(lib().gm_acq_dwell_samples(self._h, C.byref(out)), "gm_acq_dwell_samples")
        return out.value

    @property
    def dwell_periods(self):
        """Code periods one dwell holds: K * M, plus the last offset while the edge search is on"""
        return self.K * self.M + (int(self.edge_offsets[-1]) if self.edge_offsets is not None else 0)

    # ---- code-drift compensation (gm_acq_set_code_drift): every period read from where it really starts
    def set_code_drift(self, period_samples):
        """The true code period in samples (code_period_samples), a scalar or one per Doppler bin, each within 8 of fft_size; None
        switches the compensation off.  Period p of the dwell then starts at floor(p * T_d + 0.5) in bin d and a dwell is
        `dwell_samples` long."""
        if period_samples is None:
            check(lib().gm_acq_set_code_drift(self._h, 0, None), "gm_acq_set_code_drift")
            self.code_drift = None
            return
        t = np.ascontiguousarray(period_samples, np.float64).reshape(-1)
        if t.size == 1:
            t = np.full(self.D, t[0], np.float64)
        check(lib().gm_acq_set_code_drift(self._h, t.size, _p(t)), "gm_acq_set_code_drift")
        self.code_drift = t.copy()

    def code_drift_starts(self):
        """[D][R] uint64: the period starts in use (R = dwell_periods)"""
        s = np.zeros((self.D, self.dwell_periods), np.uint64)
        check(lib().gm_acq_code_drift_starts(self._h, _p(s)), "gm_acq_code_drift_starts")
        return s

    def code_drift_phasors(self, h=0):
        """[D][M][K] complex64: hypothesis h's phasor words as they sit in device memory (without the secondary row's signs)"""
        r = np.zeros((self.D, self.M, self.K), np.complex64)
        check(lib().gm_acq_code_drift_phasors(self._h, int(h), _p(r)), "gm_acq_code_drift_phasors")
        return r

    def edge_metrics(self):
        """(max, argmax, sum), each [P][H][D]: the planes of every hypothesis of the last search"""
        H = self.edge_offsets.size if self.edge_offsets is not None else 0
        mx = np.zeros((self.P, H, self.D), np.float32)
        am = np.zeros((self.P, H, self.D), np.uint32)
        sm = np.zeros((self.P, H, self.D), np.float32)
        check(lib().gm_acq_edge_metrics(self._h, _p(mx), _p(am), _p(sm)), "gm_acq_edge_metrics")
        return mx, am, sm

    def edge_choice(self):
        """[P][D] uint32: the hypothesis index each (worker, bin) cell of the last search chose"""
        ch = np.zeros((self.P, self.D), np.uint32)
        check(lib().gm_acq_edge_choice(self._h, _p(ch)), "gm_acq_edge_choice")
        return ch

    def _dicts(self, res, found, n):
        out = [res[i].as_dict() if found[i] else None for i in range(n)]
        if self.edge_offsets is not None and n <= self.P and found[:n].any():
            off = np.zeros(n, np.uint32)
            check(lib().gm_acq_result_offsets(self._h, C.cast(res, C.c_void_p), _p(found), n, _p(off)), "gm_acq_result_offsets")
            for i in range(n):
                if out[i] is not None:
                    out[i]["edge_offset_periods"] = int(off[i])
        return out

    def search(self, samples_chunk, local_tail=0, prn_mask=0xFFFFFFFFFFFFFFFF):
        """-> list (one per worker) of AcquisitionResult dict or None.  samples_chunk: K * M * N samples (coherent_periods K);
        `dwell_samples` of them while the edge search is on."""
        a, fmt, n = self._fmt(samples_chunk)      # (fewer samples: GM_ERR_OUT_OF_RANGE from the library's length check)
        res = (AcqResult * self.P)()
        found = np.zeros(self.P, np.uint8)
        check(lib().gm_acq_search(self._h, _p(a), n, fmt, int(local_tail), int(prn_mask) & (2**64 - 1),
                                  C.cast(res, C.c_void_p), _p(found)), "gm_acq_search")
        return self._dicts(res, found, self.P)

    def search_ring(self, ring, prn_mask=0xFFFFFFFFFFFFFFFF):
        """run()'s snapshot + fan-out against the device ring (do_acquisition.rs:297-313): -> (results, local_tail),
        or (None, None) while the ring holds fewer than M*N samples (:299)."""
        res = (AcqResult * self.P)()
        found = np.zeros(self.P, np.uint8)
        tail = C.c_uint64(0)
        st = lib().gm_acq_search_ring(self._h, ring._h, int(prn_mask) & (2**64 - 1), C.cast(res, C.c_void_p), _p(found),
                                      C.byref(tail))
        if st == -5:
            return None, None
        check(st, "gm_acq_search_ring")
        return self._dicts(res, found, self.P), tail.value

    def finer_doppler(self, results):
        """Fine-Doppler refinement (finer_doppler, acquisition_bk.rs:215-302) of the found results of the LAST search,
        on that search's snapshot.  -> list (per worker) of dict(freq_hz, peak_index, peak_mag, fft_size) or None."""
        n = len(results)
        res = (AcqResult * n)()
        found = np.zeros(n, np.uint8)
        for i, r in enumerate(results):
            if r:
                found[i] = 1
                for k, _ in AcqResult._fields_:
                    setattr(res[i], k, r[k])
        f = np.zeros(n, np.float32)
        idx = np.zeros(n, np.uint64)
        mag = np.zeros(n, np.float32)
        size = C.c_uint64(0)
        check(lib().gm_acq_finer_doppler(self._h, C.cast(res, C.c_void_p), _p(found), n, _p(f), _p(idx), _p(mag),
                                         C.byref(size)), "gm_acq_finer_doppler")
        return [dict(freq_hz=float(f[i]), peak_index=int(idx[i]), peak_mag=float(mag[i]), fft_size=size.value)
                if found[i] else None for i in range(n)]

    def _results_array(self, results):
        n = len(results)
        res = (AcqResult * n)()
        found = np.zeros(n, np.uint8)
        for i, r in enumerate(results):
            if r:
                found[i] = 1
                for k, _ in AcqResult._fields_:
                    setattr(res[i], k, r.get(k, 0))
        return res, found, n

    def refine_doppler(self, results, span_periods=0, n_freq=0, half_span_hz=0.0, want_prompts=False, want_spectrum=False):
        """Fine Doppler from per-period prompts (gm_acq_refine_doppler) for the found results of the LAST search, on that search's
        snapshot: the search's own statistic on n_freq grid points within +-half_span_hz of the winning bin's table frequency — with
        the handle's coherent groups, the edge search's offset and secondary row and the code-drift starts.  A result needs
        `doppler_bin` and `code_phase_samples` only.  -> list (per entry) of dict(carrier_hz, delta_hz, step_hz, half_span_hz,
        peak_power, center_power, peak_index, at_edge, doppler_bin, offset_periods, span_periods, n_groups, n_freq) or None; with
        want_prompts `prompts` (complex64 [span_periods * n_groups]), with want_spectrum `spectrum` (float32 [n_freq])."""
        res, found, n = self._results_array(results)
        cfg = AcqRefineCfg(int(span_periods), int(n_freq), float(half_span_hz))
        out = (AcqRefineOut * max(n, 1))()
        z = s = None
        if want_prompts or want_spectrum:
            plan = refine_plan(self.K, self.M, self.fs, self.fft_size, self.table_freq, 0, span_periods, n_freq, half_span_hz)
            if want_prompts:
                z = np.zeros((n, plan["span_periods"] * plan["n_groups"]), np.complex64)
            if want_spectrum:
                s = np.zeros((n, plan["n_freq"]), np.float32)
        check(lib().gm_acq_refine_doppler(self._h, C.cast(res, C.c_void_p), _p(found), n, C.byref(cfg), C.cast(out, C.c_void_p),
                                          _p(z) if z is not None else None, _p(s) if s is not None else None),
              "gm_acq_refine_doppler")
        ret = []
        for i in range(n):
            if not found[i]:
                ret.append(None)
                continue
            d = out[i].as_dict()
            if z is not None:
                d["prompts"] = z[i].copy()
            if s is not None:
                d["spectrum"] = s[i].copy()
            ret.append(d)
        return ret

    def local_search(self, cands, samples=None, lag_half_window=0, span_periods=0, n_freq=0, half_span_hz=0.0, want_prompts=False,
                     want_surface=False, fmt=FMT_C32):
        """Lag window x fine Doppler at known cells (gm_acq_local_search): refine_doppler's statistic on the 2 lag_half_window + 1 code
        phases around each candidate's, all lags from one pass over the samples.  A candidate is a dict with `worker`, `doppler_bin`,
        `code_phase_samples` (the window's centre) and `offset_periods`.  samples None: the snapshot of the last search; else a device
        pointer to dwell_samples samples in format `fmt` (as search_dev takes them) — any dwell, read only, not made the snapshot.
        -> list of dict(carrier_hz, code_phase_fine, delta_hz, step_hz, half_span_hz, peak_power, floor_power, peak_lag_index,
        peak_freq_index, code_phase_samples, lag_at_edge, freq_at_edge, n_floor, doppler_bin, offset_periods, span_periods, n_groups,
        n_freq, n_lags); with want_prompts `prompts` (complex64 [n_lags][span_periods * n_groups]), with want_surface `surface`
        (float32 [n_lags][n_freq]).  The library makes no detection decision."""
        n = len(cands)
        cs = _cand_array(cands)
        cfg = AcqLocalCfg(int(lag_half_window), int(span_periods), int(n_freq), float(half_span_hz))
        out = (AcqLocalOut * max(n, 1))()
        z = s = None
        if n and (want_prompts or want_surface):
            plan = local_plan(self.K, self.M, self.fs, self.fft_size, self.table_freq, 0, lag_half_window, span_periods, n_freq,
                              half_span_hz)
            if want_prompts:
                z = np.zeros((n, plan["n_lags"], plan["span_periods"] * plan["n_groups"]), np.complex64)
            if want_surface:
                s = np.zeros((n, plan["n_lags"], plan["n_freq"]), np.float32)
        check(lib().gm_acq_local_search(self._h, C.c_void_p(samples) if samples else None, int(fmt), C.cast(cs, C.c_void_p), n,
                                        C.byref(cfg), C.cast(out, C.c_void_p), _p(z) if z is not None else None,
                                        _p(s) if s is not None else None), "gm_acq_local_search")
        ret = []
        for i in range(n):
            d = out[i].as_dict()
            if z is not None:
                d["prompts"] = z[i].copy()
            if s is not None:
                d["surface"] = s[i].copy()
            ret.append(d)
        return ret

    def array_prompts(self, cands, samples, n_antennas, taps=1, fmt=FMT_C32):
        """Space-time prompts of an antenna array at known cells (gm_acq_array_prompts): every antenna and every tap delay of the
        interleaved stream against each candidate's replica, one vector a code period.  `samples`: a device pointer to dwell_samples
        TIME samples of n_antennas interleaved elements each (what Nuller / Stap / Beamformer take), FMT_C32 or FMT_I8_IQ; read only.
        A candidate is local_search's dict.  -> complex64 [n_cands, R_u, taps, n_antennas], R_u = max(1, K) * n_integrations; solve_rows
        turns it into constraint rows.  The library makes no detection decision."""
        n = len(cands)
        cs = _cand_array(cands)
        plan = array_plan(self.K, self.M, n_antennas, taps)
        z = np.zeros((max(n, 1), plan["periods"], int(taps), int(n_antennas)), np.complex64)
        check(lib().gm_acq_array_prompts(self._h, C.c_void_p(samples) if samples else None, int(fmt), int(n_antennas), int(taps),
                                         C.cast(cs, C.c_void_p), n, _p(z)), "gm_acq_array_prompts")
        return z[:n]

    def cancel(self, cands, out_ptr, samples=None, fmt=FMT_C32, want_amps=False):
        """Subtract found satellites from a dwell (gm_acq_cancel): one complex amplitude per signal code period and satellite is
        estimated from the input and the replica times it is subtracted; the result is written as c32 to the device pointer out_ptr
        (dwell_samples samples), which search_dev takes as a dwell.  A candidate is a dict with `worker`, `carrier_hz`, `code_phase`
        (what local_search returns as carrier_hz and code_phase_fine) and `period_samples` (the signal's true code period; 0 or
        missing: fft_size) — cancel_cands_from_local builds them.  samples None: the snapshot of the last search; else a device
        pointer to dwell_samples samples in format `fmt`, read only (out_ptr may be that pointer itself when fmt is FMT_C32: in place).
        -> list of dict(removed_energy, amp_rms, n_segments, first_samples, last_samples, worker); with want_amps `amps` (complex64
        [n_segments]).  The library makes no detection decision."""
        n = len(cands)
        cs = (AcqCancelCand * max(n, 1))()
        for i, c in enumerate(cands):
            cs[i] = AcqCancelCand(int(c["worker"]), 0, float(c["carrier_hz"]), float(c["code_phase"]), float(c.get("period_samples", 0.0)))
        out = (AcqCancelOut * max(n, 1))()
        amps, stride = None, 0
        if n and want_amps:
            D = self.dwell_samples
            stride = max(cancel_plan(D, self.fft_size, cs[i].code_phase, cs[i].period_samples)["n_segments"] for i in range(n))
            amps = np.zeros((n, stride), np.complex64)
        check(lib().gm_acq_cancel(self._h, C.c_void_p(samples) if samples else None, int(fmt), C.cast(cs, C.c_void_p), n,
                                  C.c_void_p(out_ptr) if out_ptr else None, C.cast(out, C.c_void_p),
                                  _p(amps) if amps is not None else None, stride), "gm_acq_cancel")
        ret = []
        for i in range(n):
            d = out[i].as_dict()
            if amps is not None:
                d["amps"] = amps[i, :d["n_segments"]].copy()
            ret.append(d)
        return ret

    def cancel_cands_from_local(self, local_outs, workers):
        """The candidates of cancel() from local_search's dicts and the workers they belong to: carrier_hz, code_phase =
        code_phase_fine and period_samples = the handle's code-drift period of the dict's doppler_bin (0, i.e. fft_size, while the
        compensation is off)."""
        return [dict(worker=int(w), carrier_hz=float(o["carrier_hz"]), code_phase=float(o["code_phase_fine"]),
                     period_samples=float(self.code_drift[int(o["doppler_bin"])]) if self.code_drift is not None else 0.0)
                for o, w in zip(local_outs, workers)]

    def metrics(self):
        mx = np.zeros((self.P, self.D), np.float32)
        am = np.zeros((self.P, self.D), np.uint32)
        sm = np.zeros((self.P, self.D), np.float32)
        check(lib().gm_acq_metrics(self._h, _p(mx), _p(am), _p(sm)), "gm_acq_metrics")
        return mx, am, sm

    def code_fft(self, worker):
        out = np.zeros(self.fft_size, np.complex64)
        check(lib().gm_acq_code_fft(self._h, worker, _p(out)), "gm_acq_code_fft")
        return out

    def tables(self):
        t = np.zeros((self.D, self.fft_size), np.complex64)
        check(lib().gm_acq_tables(self._h, _p(t), None), "gm_acq_tables")
        return t

    def coherent_phasors(self):
        """[n_bins][K] complex64: the coherent fold's phasor words exp(-j 2 pi f_d k N / fs) exactly as the device uses them
        (gm_acq_coherent_phasors); (1, 0) per bin at K = 1."""
        r = np.zeros((self.D, self.K), np.complex64)
        check(lib().gm_acq_coherent_phasors(self._h, _p(r)), "gm_acq_coherent_phasors")
        return r

    # ---- device-resident / asynchronous forms (bench, multi-GPU)
    def set_stream(self, stream_ptr):
        check(lib().gm_acq_set_stream(self._h, C.c_void_p(stream_ptr)), "gm_acq_set_stream")

    def set_prn_mask(self, mask):
        check(lib().gm_acq_set_prn_mask(self._h, int(mask) & (2**64 - 1)), "gm_acq_set_prn_mask")

    def search_dev(self, d_samples_ptr, fmt, d_metrics_ptr=None):
        check(lib().gm_acq_search_dev(self._h, C.c_void_p(d_samples_ptr), fmt,
                                      C.c_void_p(d_metrics_ptr) if d_metrics_ptr else None), "gm_acq_search_dev")

    def decide_dev(self, d_metrics_ptr=None, n_prn=None, prn_ids=None, local_tail=0):
        n = self.P if n_prn is None else int(n_prn)
        ids = None
        if prn_ids is not None:
            ids = np.ascontiguousarray(prn_ids, np.uint8)
        check(lib().gm_acq_decide_dev(self._h, C.c_void_p(d_metrics_ptr) if d_metrics_ptr else None, n,
                                      _p(ids) if ids is not None else None, int(local_tail)), "gm_acq_decide_dev")

    def fetch_results(self, n_prn=None):
        n = self.P if n_prn is None else int(n_prn)
        res = (AcqResult * n)()
        found = np.zeros(n, np.uint8)
        check(lib().gm_acq_fetch_results(self._h, n, C.cast(res, C.c_void_p), _p(found)), "gm_acq_fetch_results")
        return self._dicts(res, found, n)

    def synchronize(self):
        check(lib().gm_acq_synchronize(self._h), "gm_acq_synchronize")

    def prepare_dev(self, d_samples_ptr, fmt, ready_stream=None):
        """Stage F of the next dwell ahead of time, beside the current dwell's stage C (include/gnss_mi355x.h): a SNAPSHOT of the
        samples, named by the token this returns; search_prepared_dev(token) launches stage C on it.  ready_stream: the HIP stream
        whose queued work produces the samples (None: they are there already).  The samples must stay unchanged until the search
        that consumes the token has been synchronised."""
        tok = C.c_uint64(0)
        check(lib().gm_acq_prepare_dev(self._h, C.c_void_p(d_samples_ptr), fmt, C.c_void_p(ready_stream) if ready_stream else None,
                                       C.byref(tok)), "gm_acq_prepare_dev")
        return tok.value

    def search_prepared_dev(self, token, d_metrics_ptr=None):
        """Stage C on the spectra prepared under `token` (GmError INVALID_ARG when the token is stale, consumed, replaced or dropped)."""
        check(lib().gm_acq_search_prepared_dev(self._h, int(token), C.c_void_p(d_metrics_ptr) if d_metrics_ptr else None),
              "gm_acq_search_prepared_dev")

    def drop_prepared(self):
        check(lib().gm_acq_drop_prepared(self._h), "gm_acq_drop_prepared")

    def set_deferred_decision(self, on=True):
        """Back-to-back dwells: let decide_dev() ride with the next search_dev()'s first kernel (include/gnss_mi355x.h);
        synchronize() / fetch_results() run whatever is still pending."""
        check(lib().gm_acq_set_deferred_decision(self._h, int(on)), "gm_acq_set_deferred_decision")

    def debug_corr_grid(self):
        """gm_acq_debug_corr_grid: dict of the grid the launcher decided for the last stage-C launch of this handle (path 0: none yet;
        the GM_CORR_* numbers of include/gnss_mi355x.h)."""
        info = _lib.AcqCorrGridInfo()
        check(lib().gm_acq_debug_corr_grid(self._h, C.byref(info)), "gm_acq_debug_corr_grid")
        return info.as_dict()

    def enable_timing(self, on=True):
        check(lib().gm_acq_enable_timing(self._h, int(on)), "gm_acq_enable_timing")

    def last_timing(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        check(lib().gm_acq_last_timing(self._h, C.byref(a), C.byref(b), C.byref(c)), "gm_acq_last_timing")
        return {"mix_fft_ms": a.value, "corr_ms": b.value, "decide_ms": c.value}


    def timing_summary(self):
        n, a, b = C.c_uint32(0), C.c_float(0), C.c_float(0)
        check(lib().gm_acq_timing_summary(self._h, C.byref(n), C.byref(a), C.byref(b)), "gm_acq_timing_summary")
        return {"launches": n.value, "avg_mix_fft_ms": a.value, "avg_corr_ms": b.value}


class AcquisitionWorker:
    """AcquisitionWorker::new(prn, fft_size, freq_sampling_hz) + search_satellite(...)
    (do_acquisition.rs:130-226), one PRN per handle like the reference; the Doppler tables arrive
    with each call exactly as in the reference and are cached on the device by identity."""

    def __init__(self, prn, fft_size, freq_sampling_hz):
        self.prn, self.fft_size, self.freq_sampling_hz = int(prn), int(fft_size), float(freq_sampling_hz)
        if not 1 <= self.prn <= 32:
            raise IndexError("GPS_CA_CODE_32_PRN[prn - 1] out of bounds")
        self._eng = None
        self._key = None

    def search_satellite(self, samples_chunk, doppler_table, local_tail, num_integrations):
        key = (tuple(id(t) for t in doppler_table), int(num_integrations))
        if self._eng is None or self._key != key:
            if self._eng is not None:
                self._eng.close()
            self._eng = AcquisitionEngine(self.freq_sampling_hz, 0.0, self.fft_size, prn_ids=[self.prn],
                                          n_integrations=num_integrations, tables=doppler_table)
            self._key = key
        return self._eng.search(samples_chunk, local_tail)[0]

    @property
    def ca_code_samples_fft(self):
        if self._eng is None:
            tmp = AcquisitionEngine(self.freq_sampling_hz, 0.0, self.fft_size, doppler_hz=[0.0], prn_ids=[self.prn],
                                    n_integrations=1)
            out = tmp.code_fft(0)
            tmp.close()
            return out
        return self._eng.code_fft(0)


class SearchMode:
    ColdStart, WarmStart, SteadyState = 0, 1, 2


class AcquisitionManager:
    """do_acquisition.rs:39-74"""

    def __init__(self):
        self.mode = SearchMode.ColdStart

    def update_mode(self, trked_acount):
        self.mode = lib().gm_acq_manager_mode_for(int(trked_acount))

    def get_pacing_and_list(self, active_prns):
        am = 0
        for p in active_prns:
            am |= 1 << (p - 1)
        iv, m = C.c_uint64(0), C.c_uint32(0)
        check(lib().gm_acq_manager_pacing_and_list(self.mode, am, C.byref(iv), C.byref(m)), "get_pacing_and_list")
        return iv.value, m.value
