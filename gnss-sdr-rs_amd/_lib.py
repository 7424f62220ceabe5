"""ctypes binding of include/gnss_mi355x.h.  No fallback: a missing library is an ImportError-class failure."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("GM_LIB_PATH") or os.path.join(_HERE, "lib", "libgnss_mi355x.so")   # GM_LIB_PATH: an A/B build (build.py GM_LIB_SUFFIX), diagnostics only


class GmError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: gm_status {status} ({detail})")


class c32(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class AcqResult(C.Structure):
    _fields_ = [("prn", C.c_uint8), ("code_phase_samples", C.c_uint64), ("code_phase_chips", C.c_float),
                ("carrier_freq", C.c_float), ("fs", C.c_float), ("mag_relative", C.c_float),
                ("sample_global_index", C.c_uint64), ("doppler_bin", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AcqCfg(C.Structure):
    _fields_ = [("fs", C.c_float), ("f_if", C.c_float), ("fft_size", C.c_uint32), ("n_integrations", C.c_uint32),
                ("n_bins", C.c_uint32), ("doppler_hz", C.c_void_p), ("tables", C.c_void_p),
                ("table_freq", C.c_void_p), ("n_prn", C.c_uint32), ("prn_ids", C.c_void_p), ("codes", C.c_void_p),
                ("code_len", C.c_uint32), ("code_rate", C.c_float), ("threshold", C.c_float),
                ("decision_mode", C.c_int32), ("strict_sum_order", C.c_int32), ("reference_products", C.c_int32),
                ("any_length", C.c_int32), ("coherent_periods", C.c_uint32)]


class AcqPlan(C.Structure):
    _fields_ = [("form", C.c_int32), ("base", C.c_uint32), ("q", C.c_uint32), ("transform_len", C.c_uint32)]


class AcqCorrGridInfo(C.Structure):
    """gm_acq_corr_grid_info: the grid of a handle's last stage-C launch (gm_acq_debug_corr_grid)"""
    _fields_ = [(k, C.c_int32) for k in ("path", "n_workers", "n_bins", "n_int", "wg_per_cu", "split_planes", "map_mode", "share",
                                         "slots", "split_from", "split_k", "split_items", "grid", "cut", "why", "cb", "rows_max")] + \
               [("long_slab", C.c_uint32), ("long_slabs", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AcqRefineCfg(C.Structure):
    """gm_acq_refine_cfg: zeros are the defaults"""
    _fields_ = [("span_periods", C.c_uint32), ("n_freq", C.c_uint32), ("half_span_hz", C.c_float)]


class AcqRefineOut(C.Structure):
    """gm_acq_refine_out"""
    _fields_ = [("carrier_hz", C.c_double), ("delta_hz", C.c_float), ("step_hz", C.c_float), ("half_span_hz", C.c_float),
                ("peak_power", C.c_float), ("center_power", C.c_float), ("peak_index", C.c_uint32), ("at_edge", C.c_uint32),
                ("doppler_bin", C.c_uint32), ("offset_periods", C.c_uint32), ("span_periods", C.c_uint32),
                ("n_groups", C.c_uint32), ("n_freq", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AcqCand(C.Structure):
    """gm_acq_cand: a known (worker, bin, code phase, offset) cell for gm_acq_local_search"""
    _fields_ = [("worker", C.c_uint32), ("doppler_bin", C.c_int32), ("code_phase_samples", C.c_uint32), ("offset_periods", C.c_uint32)]


class AcqLocalCfg(C.Structure):
    """gm_acq_local_cfg: zeros are the defaults"""
    _fields_ = [("lag_half_window", C.c_uint32), ("span_periods", C.c_uint32), ("n_freq", C.c_uint32), ("half_span_hz", C.c_float)]


class AcqLocalOut(C.Structure):
    """gm_acq_local_out (88 bytes)"""
    _fields_ = [("carrier_hz", C.c_double), ("code_phase_fine", C.c_double), ("delta_hz", C.c_float), ("step_hz", C.c_float),
                ("half_span_hz", C.c_float), ("peak_power", C.c_float), ("floor_power", C.c_float), ("peak_lag_index", C.c_uint32),
                ("peak_freq_index", C.c_uint32), ("code_phase_samples", C.c_uint32), ("lag_at_edge", C.c_uint32),
                ("freq_at_edge", C.c_uint32), ("n_floor", C.c_uint32), ("doppler_bin", C.c_uint32), ("offset_periods", C.c_uint32),
                ("span_periods", C.c_uint32), ("n_groups", C.c_uint32), ("n_freq", C.c_uint32), ("n_lags", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ArrayRowInfo(C.Structure):
    """gm_array_row_info (24 bytes): what gm_array_row_solve reports beside the row"""
    _fields_ = [("lambda1", C.c_double), ("lambda2", C.c_double), ("ref_index", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ArraySolveCfg(C.Structure):
    """gm_array_solve_cfg (56 bytes): the shape of one gm_array_rows_solve_dev call; zero strides are the dense [n_rows][n][m]"""
    _fields_ = [("m", C.c_uint32), ("n", C.c_uint32), ("n_rows", C.c_uint32), ("n_blocks", C.c_uint32), ("row_stride", C.c_uint64),
                ("vec_stride", C.c_uint64), ("loading", C.c_float), ("reserved", C.c_uint32 * 5)]


class AcqCancelCand(C.Structure):
    """gm_acq_cancel_cand (32 bytes): a found satellite for gm_acq_cancel"""
    _fields_ = [("worker", C.c_uint32), ("reserved", C.c_uint32), ("carrier_hz", C.c_double), ("code_phase", C.c_double),
                ("period_samples", C.c_double)]


class AcqCancelOut(C.Structure):
    """gm_acq_cancel_out (32 bytes)"""
    _fields_ = [("removed_energy", C.c_double), ("amp_rms", C.c_float), ("n_segments", C.c_uint32), ("first_samples", C.c_uint32),
                ("last_samples", C.c_uint32), ("worker", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ResamplerCfg(C.Structure):
    """gm_resampler_cfg (32 bytes): zeros are the defaults"""
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32), ("n_phases", C.c_uint32), ("cutoff", C.c_float),
                ("kaiser_beta", C.c_float), ("blank_threshold", C.c_float), ("reserved", C.c_uint32)]


class DdcCfg(C.Structure):
    """gm_ddc_cfg (40 bytes): the mix frequency in cycles per input sample, then gm_resampler_cfg's fields"""
    _fields_ = [("mix_cycles_per_sample", C.c_double), ("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32),
                ("n_phases", C.c_uint32), ("cutoff", C.c_float), ("kaiser_beta", C.c_float), ("blank_threshold", C.c_float),
                ("reserved", C.c_uint32)]


class ChannelizerCfg(C.Structure):
    """gm_channelizer_cfg (40 bytes): zeros are the defaults; out_channels points at n_out_channels uint32 words, or is NULL"""
    _fields_ = [("n_channels", C.c_uint32), ("decim", C.c_uint32), ("taps_per_branch", C.c_uint32), ("cutoff", C.c_float),
                ("kaiser_beta", C.c_float), ("blank_threshold", C.c_float), ("n_out_channels", C.c_uint32), ("reserved", C.c_uint32),
                ("out_channels", C.POINTER(C.c_uint32))]


class NullerCfg(C.Structure):
    """gm_nuller_cfg (24 bytes): zeros are the defaults; steering points at n_antennas complex64 words, or is NULL (e_0)"""
    _fields_ = [("n_antennas", C.c_uint32), ("block", C.c_uint32), ("loading", C.c_float), ("reserved", C.c_uint32),
                ("steering", C.c_void_p)]


class StapCfg(C.Structure):
    """gm_stap_cfg (32 bytes): zeros are the defaults; steering points at taps * n_antennas complex64 words [taps][n_antennas], or is
    NULL (e_0)"""
    _fields_ = [("n_antennas", C.c_uint32), ("taps", C.c_uint32), ("block", C.c_uint32), ("loading", C.c_float),
                ("steering", C.c_void_p), ("reserved", C.c_uint64)]


class LcmvCfg(C.Structure):
    """gm_lcmv_cfg (56 bytes): zeros are the defaults of block and loading; n_constraints points at n_beams uint32 words Q_p, constraints at
    sum(Q) * taps * n_antennas complex64 words [sum Q][taps][n_antennas], response at sum(Q) complex64 words; all three are required"""
    _fields_ = [("n_antennas", C.c_uint32), ("taps", C.c_uint32), ("block", C.c_uint32), ("loading", C.c_float),
                ("n_beams", C.c_uint32), ("reserved32", C.c_uint32), ("n_constraints", C.c_void_p), ("constraints", C.c_void_p),
                ("response", C.c_void_p), ("reserved", C.c_uint64)]


class BeamformerCfg(C.Structure):
    """gm_beamformer_cfg (40 bytes): zeros are the defaults of block and loading; steering points at n_beams * taps * n_antennas
    complex64 words [n_beams][taps][n_antennas] and is required"""
    _fields_ = [("n_antennas", C.c_uint32), ("taps", C.c_uint32), ("block", C.c_uint32), ("loading", C.c_float),
                ("n_beams", C.c_uint32), ("reserved32", C.c_uint32), ("steering", C.c_void_p), ("reserved", C.c_uint64)]


class ExcisorCfg(C.Structure):
    """gm_excisor_cfg (32 bytes): zeros are the defaults"""
    _fields_ = [("block", C.c_uint32), ("guard_bins", C.c_uint32), ("threshold_factor", C.c_float), ("blank_threshold", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class ExcisorBlockCfg(C.Structure):
    """gm_excisor_block_cfg (32 bytes): zeros are the defaults"""
    _fields_ = [("threshold_factor", C.c_float), ("guard_bins", C.c_uint32), ("reserved", C.c_uint32 * 6)]


ACQ_FORM_LDS, ACQ_FORM_COMPOSITE, ACQ_FORM_LONG, ACQ_FORM_LONG_PADDED = 0, 1, 2, 3   # gm_acq_form


class TrkState(C.Structure):
    _fields_ = [("prn", C.c_uint8), ("active", C.c_uint8), ("reserved", C.c_uint8 * 2), ("lost_counter", C.c_uint32),
                ("next_sample_index", C.c_uint64), ("num_samples_per_code", C.c_uint64),
                ("carrier_freq", C.c_float), ("carrier_phase", C.c_float), ("carrier_error", C.c_float),
                ("carrier_nco", C.c_float), ("code_phase", C.c_float), ("code_error", C.c_float),
                ("code_nco", C.c_float), ("code_rate", C.c_float), ("i_prompt", C.c_float), ("q_prompt", C.c_float)]


class TrkOut(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("ip", "qp", "ie", "qe", "il", "ql", "ive", "qve", "ivl", "qvl")]


class NavStatus(C.Structure):
    _fields_ = [("flag_bit_sync", C.c_uint8), ("flag_frame_sync", C.c_uint8), ("sync_sw", C.c_uint8), ("bit", C.c_int8),
                ("polarity", C.c_int8), ("frame_sync_ind", C.c_uint32), ("n_frame_bits", C.c_uint64), ("i_p", C.c_float),
                ("sf_cnt", C.c_uint64), ("sf_start_biti", C.c_uint64), ("tow_expected_ind", C.c_uint64)]


class TrkCfg(C.Structure):
    _fields_ = [("fs", C.c_float), ("n_channels", C.c_uint32), ("n_arms", C.c_uint32),
                ("early_late_space", C.c_float), ("very_early_late_space", C.c_float),
                ("code_index_mode", C.c_int32), ("boc11", C.c_int32), ("codes", C.c_void_p),
                ("n_codes", C.c_uint32), ("code_len", C.c_uint32), ("nominal_code_rate", C.c_float),
                ("pll_bw", C.c_float), ("pll_zeta", C.c_float), ("pll_gain", C.c_float), ("dll_bw", C.c_float),
                ("dll_zeta", C.c_float), ("dll_gain", C.c_float), ("pll_dt", C.c_float), ("dll_dt", C.c_float),
                ("lock_threshold", C.c_float), ("max_lost_epochs", C.c_uint32), ("strict_libm", C.c_int32), ("strict_sum_order", C.c_int32),
                ("share_device", C.c_int32)]


class TrkBankCfg(C.Structure):
    """gm_trk_bank_cfg (40 bytes): taps in chips, carrier offsets in Hz (NULL with n_offsets 0: the single offset 0)"""
    _fields_ = [("n_taps", C.c_uint32), ("n_offsets", C.c_uint32), ("taps_chips", C.c_void_p), ("offsets_hz", C.c_void_p),
                ("reserved", C.c_uint32 * 4)]


class TrkBankPlanOut(C.Structure):
    """gm_trk_bank_plan_out (32 bytes)"""
    _fields_ = [("n_taps", C.c_uint32), ("n_offsets", C.c_uint32), ("out_words", C.c_uint64), ("samples", C.c_uint64),
                ("slices", C.c_uint32), ("tap_groups", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrkArrayCfg(C.Structure):
    """gm_trk_array_cfg (32 bytes): A antennas, L taps, the code tap in chips"""
    _fields_ = [("n_antennas", C.c_uint32), ("taps", C.c_uint32), ("tap_chips", C.c_float), ("reserved", C.c_uint32 * 5)]


class TrkArrayPlanOut(C.Structure):
    """gm_trk_array_plan_out (32 bytes)"""
    _fields_ = [("words_per_record", C.c_uint32), ("out_words", C.c_uint64), ("samples", C.c_uint64), ("slices", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrkPlanesPlanOut(C.Structure):
    """gm_trk_planes_plan_out (40 bytes)"""
    _fields_ = [("workgroups", C.c_uint32), ("threads", C.c_uint32), ("chip_row_bytes", C.c_uint32), ("planes_used", C.c_uint32),
                ("samples", C.c_uint64), ("samples_per_lane", C.c_uint32), ("reserved", C.c_uint32), ("result_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


FMT_C32, FMT_I8_IQ, FMT_I8_REAL = 0, 1, 2
CODE_INDEX_FAITHFUL, CODE_INDEX_FIXED = 0, 1

# every symbol include/gnss_mi355x.h declares: (name, restype, argtypes)
_vp, _f, _u64, _u32, _sz, _i = C.c_void_p, C.c_float, C.c_uint64, C.c_uint32, C.c_size_t, C.c_int
SIGNATURES = {
    "gm_abi_version": (_i, []),
    "gm_init": (_i, [_i]),
    "gm_device_count": (_i, [C.POINTER(_i)]),
    "gm_last_error": (C.c_char_p, []),
    "gm_status_string": (C.c_char_p, [_i]),
    "gm_ca_code_row": (_i, [_i, _vp]),
    "gm_b1i_code": (_i, [C.c_uint32, _vp, C.c_uint32]),
    "gm_generate_ca_code_samples": (_i, [C.c_uint8, _f, _f, _vp, _sz, C.POINTER(_sz)]),
    "gm_doppler_table_new": (_i, [_f, _f, _f, _sz, C.POINTER(_f), _vp]),
    "gm_apply_doppler_shift": (_i, [_vp, _vp, _vp, _sz]),
    "gm_fft_c2c_f32": (_i, [_sz, _i, _vp, _sz]),
    "gm_fft_power_spectrum_f32": (_i, [_sz, _vp, _vp]),
    "gm_rfft_f32": (_i, [_sz, _vp, _vp]),
    "gm_fft_supported_sizes": (_i, [_vp, _i]),
    "gm_acq_plan_info": (_i, [C.c_uint32, C.c_int32, C.POINTER(AcqPlan)]),
    "gm_acq_create": (_i, [C.POINTER(AcqCfg), C.POINTER(_vp)]),
    "gm_acq_destroy": (_i, [_vp]),
    "gm_acq_search": (_i, [_vp, _vp, _sz, _i, _u64, _u64, _vp, _vp]),
    "gm_acq_search_c32": (_i, [_vp, _vp, _sz, _u64, _u64, _vp, _vp]),
    "gm_acq_search_i8": (_i, [_vp, _vp, _sz, _u64, _u64, _vp, _vp]),
    "gm_acq_search_ring": (_i, [_vp, _vp, _u64, _vp, _vp, C.POINTER(_u64)]),
    "gm_acq_search_dev": (_i, [_vp, _vp, _i, _vp]),
    "gm_acq_set_prn_mask": (_i, [_vp, _u64]),
    "gm_acq_decide_dev": (_i, [_vp, _vp, _u32, _vp, _u64]),
    "gm_acq_finer_doppler": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "gm_comm_get_unique_id": (_i, [_vp]),
    "gm_comm_init": (_i, [_i, _i, _vp, _vp]),
    "gm_comm_destroy": (_i, [_vp]),
    "gm_comm_info": (_i, [_vp, _vp, _vp]),
    "gm_acq_allgather_metrics": (_i, [_vp, _vp, _vp, _vp]),
    "gm_acq_allgather_metrics_async": (_i, [_vp, _vp, _vp, _vp]),
    "gm_comm_wait": (_i, [_vp, _vp]),
    "gm_comm_allgather_words": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gm_grid_assemble_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "gm_acq_decide_planes_dev": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _f, _f, _f, _i, _u64, _vp, _vp, _vp]),
    "gm_acq_fetch_results": (_i, [_vp, _u32, _vp, _vp]),
    "gm_acq_decide_host": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _f, _f, _f, _u64, _vp, _vp]),
    "gm_acq_synchronize": (_i, [_vp]),
    "gm_acq_set_deferred_decision": (_i, [_vp, _i]),
    "gm_acq_prepare_dev": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_uint64)]),
    "gm_acq_search_prepared_dev": (_i, [_vp, C.c_uint64, _vp]),
    "gm_acq_drop_prepared": (_i, [_vp]),
    "gm_acq_set_stream": (_i, [_vp, _vp]),
    "gm_acq_metrics": (_i, [_vp, _vp, _vp, _vp]),
    "gm_acq_code_fft": (_i, [_vp, _u32, _vp]),
    "gm_acq_tables": (_i, [_vp, _vp, _vp]),
    "gm_acq_coherent_phasors": (_i, [_vp, _vp]),
    "gm_acq_edge_dwell_periods": (_i, [_u32, _u32, _u32, _vp, _vp, C.POINTER(_u64)]),
    "gm_acq_set_edge_search": (_i, [_vp, _u32, _vp, _vp]),
    "gm_acq_edge_metrics": (_i, [_vp, _vp, _vp, _vp]),
    "gm_acq_edge_choice": (_i, [_vp, _vp]),
    "gm_acq_result_offsets": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "gm_acq_set_code_drift": (_i, [_vp, _u32, _vp]),
    "gm_acq_code_drift_plan": (_i, [_u32, _u32, _u32, _vp, _vp, C.POINTER(_u64)]),
    "gm_acq_dwell_samples": (_i, [_vp, C.POINTER(_u64)]),
    "gm_acq_code_drift_starts": (_i, [_vp, _vp]),
    "gm_acq_code_drift_phasors": (_i, [_vp, _u32, _vp]),
    "gm_acq_refine_doppler": (_i, [_vp, _vp, _vp, _u32, C.POINTER(AcqRefineCfg), _vp, _vp, _vp]),
    "gm_acq_refine_plan": (_i, [_u32, _u32, C.POINTER(AcqRefineCfg), _f, _u32, _u32, _vp, _u32, C.POINTER(_u32), C.POINTER(_u32),
                            C.POINTER(_u32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gm_acq_local_search": (_i, [_vp, _vp, _i, _vp, _u32, C.POINTER(AcqLocalCfg), _vp, _vp, _vp]),
    "gm_acq_local_plan": (_i, [_u32, _u32, C.POINTER(AcqLocalCfg), _f, _u32, _u32, _vp, _u32, C.POINTER(_u32), C.POINTER(_u32),
                           C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gm_acq_array_prompts": (_i, [_vp, _vp, _i, _u32, _u32, _vp, _u32, _vp]),
    "gm_acq_array_plan": (_i, [_u32, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "gm_array_row_solve": (_i, [_u32, _u32, _vp, _vp, _sz, _f, _vp, C.POINTER(ArrayRowInfo)]),
    "gm_array_solve_plan": (_i, [C.POINTER(ArraySolveCfg), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_array_rows_solve_dev": (_i, [C.POINTER(ArraySolveCfg), _vp, _vp, _vp, _vp, _vp]),
    "gm_acq_cancel": (_i, [_vp, _vp, _i, _vp, _u32, _vp, _vp, _vp, _u32]),
    "gm_acq_cancel_plan": (_i, [C.c_uint64, _u32, C.c_double, C.c_double, C.POINTER(_u32), _vp, _u32]),
    "gm_acq_enable_timing": (_i, [_vp, _i]),
    "gm_acq_last_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f)]),
    "gm_acq_timing_summary": (_i, [_vp, C.POINTER(_u32), C.POINTER(_f), C.POINTER(_f)]),
    "gm_acq_debug_stamps": (_i, [_vp, _vp]),
    "gm_acq_debug_corr_grid": (_i, [_vp, C.POINTER(AcqCorrGridInfo)]),
    "gm_acq_manager_mode_for": (_i, [_sz]),
    "gm_acq_manager_pacing_and_list": (_i, [_i, _u32, C.POINTER(_u64), C.POINTER(_u32)]),
    "gm_ring_create": (_i, [_sz, C.POINTER(_vp)]),
    "gm_ring_destroy": (_i, [_vp]),
    "gm_ring_write_samples": (_i, [_vp, _vp, _sz]),
    "gm_ring_get_head": (_i, [_vp, C.POINTER(_u64)]),
    "gm_ring_copy_to_slice": (_i, [_vp, _u64, _vp, _sz]),
    "gm_ring_write_samples_async": (_i, [_vp, _vp, _sz]),
    "gm_ring_flush": (_i, [_vp]),
    "gm_ring_get_enqueued_head": (_i, [_vp, C.POINTER(_u64)]),
    "gm_ring_wait_head": (_i, [_vp, _u64, _u32, _vp]),
    "gm_nav_sync_create": (_i, [_i, _vp]),
    "gm_nav_sync_destroy": (_i, [_vp]),
    "gm_nav_sync_update": (_i, [_vp, _f, _f, _u64, _u64, _vp]),
    "gm_nav_sync_update_many": (_i, [_vp, _f, _vp, _sz, _sz, _u64, _u64, _vp, _vp, _vp]),
    "gm_nav_sync_frame_bits": (_i, [_vp, _vp, _sz, _vp]),
    "gm_nav_sync_histogram": (_i, [_vp, _vp]),
    "gm_nav_parity_check": (_i, [_vp, _vp, _vp]),
    "gm_frontend_create": (_i, [_f, _f, _f, _vp]),
    "gm_frontend_destroy": (_i, [_vp]),
    "gm_frontend_lut": (_i, [_vp, _vp, _vp, _vp]),
    "gm_frontend_get_state": (_i, [_vp, _vp, _vp, _vp]),
    "gm_frontend_set_state": (_i, [_vp, _f, _vp, _vp]),
    "gm_frontend_process_block": (_i, [_vp, _vp, _sz]),
    "gm_frontend_process_dev": (_i, [_vp, _vp, _i, _vp, _sz, _vp]),
    "gm_frontend_process_dev_batch": (_i, [_vp, _u32, _vp, _i, _vp, _sz, _vp]),
    "gm_frontend_synchronize": (_i, [_vp]),
    "gm_frontend_write_ring": (_i, [_vp, _vp, _vp, _sz, _i]),
    "gm_frontend_debug_repairs": (_i, [_vp, C.POINTER(_u32)]),
    "gm_frontend_debug_forms": (_i, [_vp, C.POINTER(_u32)]),
    "gm_resampler_plan": (_i, [C.POINTER(ResamplerCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32),
                           C.POINTER(_u64)]),
    "gm_resampler_design": (_i, [C.POINTER(ResamplerCfg), _vp]),
    "gm_resampler_create": (_i, [C.POINTER(ResamplerCfg), C.POINTER(_vp)]),
    "gm_resampler_destroy": (_i, [_vp]),
    "gm_resampler_reset": (_i, [_vp, _u64]),
    "gm_resampler_taps": (_i, [_vp, _vp]),
    "gm_resampler_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_resampler_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_resampler_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gm_resampler_synchronize": (_i, [_vp]),
    "gm_frontend_write_ring_resampled": (_i, [_vp, _vp, _vp, _vp, _sz, _i, C.POINTER(_u64)]),
    "gm_excisor_plan": (_i, [C.POINTER(ExcisorCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u64)]),
    "gm_excisor_windows": (_i, [C.POINTER(ExcisorCfg), _vp, _vp]),
    "gm_excisor_create": (_i, [C.POINTER(ExcisorCfg), C.POINTER(_vp)]),
    "gm_excisor_destroy": (_i, [_vp]),
    "gm_excisor_reset": (_i, [_vp, _u64]),
    "gm_excisor_set_gains": (_i, [_vp, _vp]),
    "gm_excisor_gains": (_i, [_vp, _vp]),
    "gm_excisor_adapt_dev": (_i, [_vp, _vp, _i, _sz, _vp]),
    "gm_excisor_psd": (_i, [_vp, _vp, C.POINTER(C.c_float), C.POINTER(_u32), C.POINTER(_u32)]),
    "gm_excisor_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_excisor_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_excisor_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gm_excisor_synchronize": (_i, [_vp]),
    "gm_excisor_block_plan": (_i, [C.POINTER(ExcisorBlockCfg), C.POINTER(C.c_float), C.POINTER(_u32)]),
    "gm_excisor_set_block_adapt": (_i, [_vp, C.POINTER(ExcisorBlockCfg)]),
    "gm_excisor_block_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_excisor_block_capture": (_i, [_vp, _vp, _vp, _sz]),
    "gm_frontend_write_ring_conditioned": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, C.POINTER(_u64)]),
    "gm_ddc_plan": (_i, [C.POINTER(DdcCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64),
                         C.POINTER(_u64)]),
    "gm_ddc_create": (_i, [C.POINTER(DdcCfg), C.POINTER(_vp)]),
    "gm_ddc_destroy": (_i, [_vp]),
    "gm_ddc_reset": (_i, [_vp, _u64]),
    "gm_ddc_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_ddc_synchronize": (_i, [_vp]),
    "gm_ddc_tables": (_i, [_vp, _vp, _vp, _vp]),
    "gm_ddc_process_dev": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_ddc_process": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gm_ddc_write_ring": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_u64)]),
    "gm_channelizer_plan": (_i, [C.POINTER(ChannelizerCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64)]),
    "gm_channelizer_design": (_i, [C.POINTER(ChannelizerCfg), _vp]),
    "gm_channelizer_create": (_i, [C.POINTER(ChannelizerCfg), C.POINTER(_vp)]),
    "gm_channelizer_destroy": (_i, [_vp]),
    "gm_channelizer_reset": (_i, [_vp, _u64]),
    "gm_channelizer_taps": (_i, [_vp, _vp]),
    "gm_channelizer_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_channelizer_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, _sz, C.POINTER(_sz), _vp]),
    "gm_channelizer_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gm_channelizer_synchronize": (_i, [_vp]),
    "gm_glonass_code": (_i, [_vp]),
    "gm_nuller_plan": (_i, [C.POINTER(NullerCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u64)]),
    "gm_nuller_create": (_i, [C.POINTER(NullerCfg), C.POINTER(_vp)]),
    "gm_nuller_destroy": (_i, [_vp]),
    "gm_nuller_reset": (_i, [_vp, _u64]),
    "gm_nuller_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_nuller_synchronize": (_i, [_vp]),
    "gm_nuller_set_weights": (_i, [_vp, _vp]),
    "gm_nuller_capture": (_i, [_vp, _vp, _vp, _sz]),
    "gm_nuller_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_nuller_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "gm_stap_plan": (_i, [C.POINTER(StapCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u64)]),
    "gm_stap_create": (_i, [C.POINTER(StapCfg), C.POINTER(_vp)]),
    "gm_stap_destroy": (_i, [_vp]),
    "gm_stap_reset": (_i, [_vp, _u64]),
    "gm_stap_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_stap_synchronize": (_i, [_vp]),
    "gm_stap_set_weights": (_i, [_vp, _vp]),
    "gm_stap_capture": (_i, [_vp, _vp, _vp, _sz]),
    "gm_stap_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_stap_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "gm_beamformer_plan": (_i, [C.POINTER(BeamformerCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u64)]),
    "gm_beamformer_create": (_i, [C.POINTER(BeamformerCfg), C.POINTER(_vp)]),
    "gm_beamformer_destroy": (_i, [_vp]),
    "gm_beamformer_reset": (_i, [_vp, _u64]),
    "gm_beamformer_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_beamformer_synchronize": (_i, [_vp]),
    "gm_beamformer_set_steering": (_i, [_vp, _u32, _vp]),
    "gm_beamformer_set_steering_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _f, _vp, _vp]),
    "gm_beamformer_set_weights": (_i, [_vp, _vp]),
    "gm_beamformer_capture": (_i, [_vp, _vp, _vp, _sz]),
    "gm_beamformer_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_beamformer_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "gm_lcmv_plan": (_i, [C.POINTER(LcmvCfg), _u64, _u64, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u64)]),
    "gm_lcmv_create": (_i, [C.POINTER(LcmvCfg), C.POINTER(_vp)]),
    "gm_lcmv_destroy": (_i, [_vp]),
    "gm_lcmv_reset": (_i, [_vp, _u64]),
    "gm_lcmv_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gm_lcmv_synchronize": (_i, [_vp]),
    "gm_lcmv_set_constraints": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "gm_lcmv_set_weights": (_i, [_vp, _vp]),
    "gm_lcmv_capture": (_i, [_vp, _vp, _vp, _sz]),
    "gm_lcmv_process_dev": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "gm_lcmv_process": (_i, [_vp, _vp, _i, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "gm_trk_create": (_i, [C.POINTER(TrkCfg), C.POINTER(_vp)]),
    "gm_trk_destroy": (_i, [_vp]),
    "gm_trk_start": (_i, [_vp, _u32, C.POINTER(AcqResult)]),
    "gm_trk_reset": (_i, [_vp, _u32]),
    "gm_trk_get_state": (_i, [_vp, _u32, C.POINTER(TrkState)]),
    "gm_trk_set_state": (_i, [_vp, _u32, C.POINTER(TrkState)]),
    "gm_trk_get_ca_chip": (_i, [_vp, _u32, _f, C.POINTER(_f)]),
    "gm_loop_filter_new": (_i, [_f, _f, _f, C.POINTER(_f), C.POINTER(_f)]),
    "gm_loop_filter_update": (_f, [_f, _f, _f, _f, _f]),
    "gm_trk_correlate": (_i, [_vp, _u32, _vp, _sz, C.POINTER(TrkOut)]),
    "gm_trk_do_work": (_i, [_vp, _u32, _vp, _sz, C.POINTER(TrkOut), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "gm_trk_update_all": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "gm_trk_update_all_dev": (_i, [_vp, _vp, _u32]),
    "gm_trk_update_all_async": (_i, [_vp, _vp, _u32, C.POINTER(C.c_uint64)]),
    "gm_trk_collect": (_i, [_vp, C.c_uint64, _i, _vp, _vp, _vp, _vp, C.POINTER(_u32), C.POINTER(_i)]),
    "gm_trk_get_states": (_i, [_vp, _vp]),
    "gm_trk_set_states": (_i, [_vp, _vp, _vp]),
    "gm_trk_synchronize": (_i, [_vp]),
    "gm_trk_set_stream": (_i, [_vp, _vp]),
    "gm_trk_debug_stamps": (_i, [_vp, _u32, _vp]),
    "gm_trk_enable_timing": (_i, [_vp, _i]),
    "gm_trk_last_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_u32)]),
    "gm_debug_math": (_i, [_i, _vp, _sz, _f, _f, _f, _vp, _vp]),
    "gm_debug_fft_four_step": (_i, [_u32, _u32, _i, _vp, _sz]),
    "gm_trk_bank_plan": (_i, [C.POINTER(TrkCfg), C.POINTER(TrkBankCfg), _u32, C.POINTER(TrkBankPlanOut)]),
    "gm_trk_bank": (_i, [_vp, _vp, _vp, _u32, C.POINTER(TrkBankCfg), _vp, _vp]),
    "gm_trk_bank_samples": (_i, [_vp, C.POINTER(TrkState), _vp, _sz, C.POINTER(TrkBankCfg), _vp]),
    "gm_trk_array_plan": (_i, [C.POINTER(TrkCfg), C.POINTER(TrkArrayCfg), _u32, C.POINTER(TrkArrayPlanOut)]),
    "gm_trk_array_prompts": (_i, [_vp, _vp, _i, _u64, _u64, _vp, _u32, C.POINTER(TrkArrayCfg), _vp, _vp]),
    "gm_trk_array_prompts_dev": (_i, [_vp, _vp, _i, _u64, _u64, _vp, _u32, C.POINTER(TrkArrayCfg), _vp, _vp, _vp]),
    "gm_plane_ring_plan": (_i, [_u32, _u64, C.POINTER(_u64)]),
    "gm_plane_ring_create": (_i, [_u32, _u64, C.POINTER(_vp)]),
    "gm_plane_ring_destroy": (_i, [_vp]),
    "gm_plane_ring_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_vp)]),
    "gm_plane_ring_write_dev": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "gm_plane_ring_write": (_i, [_vp, _vp, _sz, _sz]),
    "gm_plane_ring_get_head": (_i, [_vp, C.POINTER(_u64)]),
    "gm_plane_ring_copy_to_slice": (_i, [_vp, _u32, _u64, _vp, _sz]),
    "gm_plane_ring_synchronize": (_i, [_vp]),
    "gm_trk_planes_plan": (_i, [C.POINTER(TrkCfg), _u32, _vp, _u32, C.POINTER(TrkPlanesPlanOut)]),
    "gm_trk_set_channel_planes": (_i, [_vp, _vp]),
    "gm_trk_get_channel_planes": (_i, [_vp, _vp]),
    "gm_trk_update_planes": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "gm_trk_update_planes_dev": (_i, [_vp, _vp, _u32]),
}

_lib = None


def library_path():
    return _LIB_PATH


def lib():
    """Load libgnss_mi355x.so (built in-tree by build.py).  Raises if it is missing: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: run `python __graft_entry__.py build` (hipcc, gfx950). "
                          "There is no CPU fallback for the HIP path.")
    L = C.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)          # AttributeError if the header and the library drift apart
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(status, where):
    if status != 0:
        L = lib()
        raise GmError(status, where, (L.gm_status_string(status) or b"").decode() + "; " +
                      (L.gm_last_error() or b"").decode())


_initialised = None


def init(device=0):
    """gm_init(device): one process per GPU."""
    global _initialised
    if _initialised != device:
        check(lib().gm_init(device), "gm_init")
        _initialised = device
