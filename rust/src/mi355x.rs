// mi355x.rs — DESTINATION: src/mi355x.rs of kewei/gnss-sdr-rs (a NEW module; `pub mod mi355x;` is added to src/lib.rs after
// `pub mod constants;`, lib.rs:14).  Raw bindings of include/gnss_mi355x.h: the `extern "C"` block and the
// #[repr(C)] mirrors.  The wrappers that carry the reference's own names and signatures are its SUBMODULES — new sibling
// modules of the reference's own, which stay in the crate untouched (nothing is edited in place, nothing is replaced):
//   src/mi355x/doppler_shift.rs   DopplerShiftTable::new, apply_doppler_shift                 (cf. src/acquisition/doppler_shift.rs:5-40)
//   src/mi355x/do_acquisition.rs  AcquisitionWorker::{new, search_satellite}, AcquisitionEngine, run
//                                                                                              (cf. src/acquisition/do_acquisition.rs:130-226, 241-327)
//   src/mi355x/do_tracking.rs     TrackingChannel (22 pub fields, every method), TrackingManager::{new, process_channels}, run
//                                                                                              (cf. src/tracking/do_tracking.rs:88-415)
//   src/mi355x/fft.rs             FFT<f32>, RealFFT<f32>                                       (cf. src/fft.rs:5-56)
// They import the items that do NOT change (AcquisitionResult, AcqError, ChannelState, AcquisitionManager, LoopFilter,
// TrackingMessage, TrackingError, MulticastRingBuffer, the reference's DopplerShiftTable) from the reference's modules.
// main.rs switches two `use` lines (rust/patches/main_rs.diff); the thread wiring at main.rs:204-227 is unchanged.
// Shipped as source: the build image has no Rust toolchain, so these files were NOT compiled here; the same ABI is
// exercised end to end by gnss-sdr-rs_amd/host/gnss_sdr.hpp + tests/cpp/test_host_api.cpp (C++) and by the ctypes mirror
// used in tests/ (Python); tests/test_abi_and_host.py checks struct layouts, extern names, wrapper signatures and that every
// `use crate::...` path of these files names an item that exists in the reference's module tree or in these files.
#![allow(non_camel_case_types, dead_code)]

pub mod doppler_shift;
pub mod do_acquisition;
pub mod do_tracking;
pub mod fft;

// ------------------------------------------------------------------ raw bindings
use num_complex::Complex32;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqResult {            // gm_acq_result  <->  AcquisitionResult (do_acquisition.rs:93-116)
    pub prn: u8,
    pub code_phase_samples: u64,
    pub code_phase_chips: f32,
    pub carrier_freq: f32,
    pub fs: f32,
    pub mag_relative: f32,
    pub sample_global_index: u64,
    pub doppler_bin: i32,
}
#[repr(C)]
pub struct GmAcqCfg {               // gm_acq_cfg
    pub fs: f32, pub f_if: f32, pub fft_size: u32, pub n_integrations: u32, pub n_bins: u32,
    pub doppler_hz: *const f32, pub tables: *const Complex32, pub table_freq: *const f32,
    pub n_prn: u32, pub prn_ids: *const u8, pub codes: *const i8, pub code_len: u32, pub code_rate: f32,
    pub threshold: f32,
    pub decision_mode: i32,          // 0 = the reference's early exit (GM_DECIDE_REFERENCE), 1 = strongest bin
    pub strict_sum_order: i32,       // 1 = is_good_satellite's sum in the reference's 8-lane order (do_acquisition.rs:229-235)
    pub reference_products: i32,     // 1 = x conj(code) and norm_sqr() rounded as num-complex rounds them (no fused multiply-add; :184-192)
    pub any_length: i32,             // 1 = any fft_size % 8 == 0 in [1024, 2^18] (the long path), as rustfft plans any length (:130-143)
    pub coherent_periods: u32,       // K > 1 = K code periods folded coherently per group; a dwell is K * n_integrations periods (ABI 9)
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct GmTrkState {             // gm_trk_state  <->  the evolving fields of TrackingChannel (do_tracking.rs:88-116)
    pub prn: u8, pub active: u8, pub reserved: [u8; 2], pub lost_counter: u32,
    pub next_sample_index: u64, pub num_samples_per_code: u64,
    pub carrier_freq: f32, pub carrier_phase: f32, pub carrier_error: f32, pub carrier_nco: f32,
    pub code_phase: f32, pub code_error: f32, pub code_nco: f32, pub code_rate: f32,
    pub i_prompt: f32, pub q_prompt: f32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmTrkOut { pub ip: f32, pub qp: f32, pub ie: f32, pub qe: f32, pub il: f32, pub ql: f32,
                      pub ive: f32, pub qve: f32, pub ivl: f32, pub qvl: f32 }
#[repr(C)]
pub struct GmTrkCfg {               // gm_trk_cfg (zero = reference default)
    pub fs: f32, pub n_channels: u32, pub n_arms: u32, pub early_late_space: f32, pub very_early_late_space: f32,
    pub code_index_mode: i32, pub boc11: i32, pub codes: *const i8, pub n_codes: u32, pub code_len: u32,
    pub nominal_code_rate: f32, pub pll_bw: f32, pub pll_zeta: f32, pub pll_gain: f32, pub dll_bw: f32,
    pub dll_zeta: f32, pub dll_gain: f32, pub pll_dt: f32, pub dll_dt: f32, pub lock_threshold: f32,
    pub max_lost_epochs: u32,
    pub strict_libm: i32,           // 1 = the carrier's cos / sin are glibc's cosf / sinf restated on the device (bit-identical products)
    pub strict_sum_order: i32,      // 1 = the correlator sums added sample by sample like do_tracking.rs:256-262 (with strict_libm: bit-identical state)
    pub share_device: i32,          // 1 = a receiver: the tracking kernel leaves room for the front-end's and the acquisition's kernels beside it (ABI 6)
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqRefineCfg {         // gm_acq_refine_cfg (zeros: the defaults)
    pub span_periods: u32, pub n_freq: u32, pub half_span_hz: f32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqRefineOut {         // gm_acq_refine_out
    pub carrier_hz: f64,             // table_freq[doppler_bin] + delta_hz
    pub delta_hz: f32, pub step_hz: f32, pub half_span_hz: f32,
    pub peak_power: f32, pub center_power: f32,
    pub peak_index: u32, pub at_edge: u32,
    pub doppler_bin: u32, pub offset_periods: u32, pub span_periods: u32, pub n_groups: u32, pub n_freq: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqCand {              // gm_acq_cand: a known cell for gm_acq_local_search
    pub worker: u32, pub doppler_bin: i32, pub code_phase_samples: u32, pub offset_periods: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqLocalCfg {          // gm_acq_local_cfg (zeros: the defaults)
    pub lag_half_window: u32, pub span_periods: u32, pub n_freq: u32, pub half_span_hz: f32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqLocalOut {          // gm_acq_local_out (88 bytes)
    pub carrier_hz: f64,             // table_freq[doppler_bin] + delta_hz
    pub code_phase_fine: f64,        // samples, [0, fft_size)
    pub delta_hz: f32, pub step_hz: f32, pub half_span_hz: f32,
    pub peak_power: f32, pub floor_power: f32,
    pub peak_lag_index: u32, pub peak_freq_index: u32, pub code_phase_samples: u32,
    pub lag_at_edge: u32, pub freq_at_edge: u32, pub n_floor: u32,
    pub doppler_bin: u32, pub offset_periods: u32, pub span_periods: u32, pub n_groups: u32, pub n_freq: u32, pub n_lags: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmArrayRowInfo {         // gm_array_row_info (24 bytes): lambda1 / lambda2 is the estimate's quality; the caller judges
    pub lambda1: f64, pub lambda2: f64, pub ref_index: u32, pub reserved: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmArraySolveCfg {        // gm_array_solve_cfg (56 bytes): one gm_array_rows_solve_dev call; strides in Complex32 words, 0, 0: [n_rows][n][m]
    pub m: u32, pub n: u32, pub n_rows: u32, pub n_blocks: u32, pub row_stride: u64, pub vec_stride: u64, pub loading: f32, pub reserved: [u32; 5],
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqCancelCand {        // gm_acq_cancel_cand (32 bytes): a found satellite for gm_acq_cancel
    pub worker: u32, pub reserved: u32,
    pub carrier_hz: f64,             // IF + Doppler: GmAcqLocalOut::carrier_hz
    pub code_phase: f64,             // samples into the dwell, [0, fft_size): GmAcqLocalOut::code_phase_fine
    pub period_samples: f64,         // the signal's true code period; 0: fft_size
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmAcqCancelOut {         // gm_acq_cancel_out (32 bytes)
    pub removed_energy: f64,         // sum_k n_k |a_k|^2
    pub amp_rms: f32,
    pub n_segments: u32, pub first_samples: u32, pub last_samples: u32, pub worker: u32, pub reserved: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmResamplerCfg {         // gm_resampler_cfg (32 bytes; zeros: the defaults)
    pub up: u32, pub down: u32,      // fs_out = fs_in * up / down; reduced by their gcd inside; 1/16 <= up/down <= 16
    pub taps: u32,                   // a multiple of 8 in 8 .. 256; 0: min(256, 32 * ceil(max(1, down/up)))
    pub n_phases: u32,               // a power of two 16 .. 1024; 0: 256
    pub cutoff: f32,                 // (0, 1] of the narrower Nyquist band; 0: 0.9
    pub kaiser_beta: f32,            // [0, 20]; 0: 8.0
    pub blank_threshold: f32,        // 0: off; > 0: an input sample with re^2 + im^2 > thr^2 is replaced by (0, 0)
    pub reserved: u32,               // must be 0
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmExcisorCfg {           // gm_excisor_cfg (32 bytes; zeros: the defaults)
    pub block: u32,                  // B: 256, 512, 1024, 2048 or 4096; 0: 1024
    pub guard_bins: u32,             // 0 .. 16: bins zeroed on either side of a flagged one
    pub threshold_factor: f32,       // > 1; 0: 4.0 — a bin is flagged when P[k] > factor * median
    pub blank_threshold: f32,        // 0: off; > 0: an input sample with re^2 + im^2 > thr^2 is replaced by (0, 0) first
    pub reserved: [u32; 4],          // must be 0
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmExcisorBlockCfg {      // gm_excisor_block_cfg (32 bytes; zeros: the defaults)
    pub threshold_factor: f32,       // > 1; 0: 16.0 — a bin of a block is flagged when p[k] > factor * med_b
    pub guard_bins: u32,             // 0 .. 16: bins zeroed on either side of a flagged one
    pub reserved: [u32; 6],          // must be 0
}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmTrkBankCfg {           // gm_trk_bank_cfg (40 bytes): the correlator bank at tracked states
    pub n_taps: u32,                 // T: 1 .. 64
    pub n_offsets: u32,              // F: 0 .. 8, F * T <= 256; 0 with offsets_hz null: the single offset 0
    pub taps_chips: *const f32,      // [n_taps] chips, |tau| <= 64 and < code_len / 2
    pub offsets_hz: *const f32,      // [n_offsets] Hz, |df| <= fs / 2, or null
    pub reserved: [u32; 4],          // must be 0
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmTrkBankPlanOut {       // gm_trk_bank_plan_out (32 bytes)
    pub n_taps: u32,
    pub n_offsets: u32,              // the effective F
    pub out_words: u64,              // n_states * F * T complex words
    pub samples: u64,                // n for the configuration's nominal code rate
    pub slices: u32,                 // ceil(n / 4096)
    pub tap_groups: u32,             // ceil(T / 16)
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmTrkArrayCfg {          // gm_trk_array_cfg (32 bytes): per-antenna prompts of an array stream at tracked states
    pub n_antennas: u32,             // A: 2 .. 8
    pub taps: u32,                   // L: 1 .. 8, A * L <= 32
    pub tap_chips: f32,              // the code tap tau, chips: |tau| <= 64 and < code_len / 2
    pub reserved: [u32; 5],          // must be 0
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmTrkArrayPlanOut {      // gm_trk_array_plan_out (32 bytes)
    pub words_per_record: u32,       // L * A
    pub out_words: u64,              // n_states * L * A complex words
    pub samples: u64,                // n for the configuration's nominal code rate
    pub slices: u32,                 // ceil(n / 4096)
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmTrkPlanesPlanOut {     // gm_trk_planes_plan_out (40 bytes)
    pub workgroups: u32,             // one per channel: n_channels
    pub threads: u32,                // 256
    pub chip_row_bytes: u32,         // the workgroup's dynamic LDS: code_len int8 chips
    pub planes_used: u32,            // distinct planes the map names
    pub samples: u64,                // n for the configuration's nominal code rate
    pub samples_per_lane: u32,       // ceil(n / 256)
    pub reserved: u32,               // 0
    pub result_bytes: u64,           // max_epochs * n_channels * 43, rounded up to 4
}
pub enum GmPlaneRing {}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct GmDdcCfg {             // gm_ddc_cfg (40 bytes; zeros in the filter fields: the defaults)
    pub mix_cycles_per_sample: f64,  // f_mix / fs_in: the frequency brought to 0, cycles per input sample; any finite value
    pub up: u32, pub down: u32,      // as GmResamplerCfg, field by field
    pub taps: u32,
    pub n_phases: u32,
    pub cutoff: f32,
    pub kaiser_beta: f32,
    pub blank_threshold: f32,        // 0: off; > 0: an input sample with x^2 > thr^2 is replaced by 0
    pub reserved: u32,               // must be 0
}
pub enum GmDdc {}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmChannelizerCfg {       // gm_channelizer_cfg (40 bytes; zeros in the filter fields: the defaults)
    pub n_channels: u32,             // M: 4, 8, 16, 32 or 64
    pub decim: u32,                  // D: 1 .. M
    pub taps_per_branch: u32,        // P: 2 .. 32, L = M P taps in all; 0 -> 16
    pub cutoff: f32,                 // (0, 1] of the output Nyquist frequency; 0 -> 0.9
    pub kaiser_beta: f32,            // [0, 20]; 0 -> 8
    pub blank_threshold: f32,        // 0: off; > 0: an input sample with re^2 + im^2 > thr^2 is replaced by 0
    pub n_out_channels: u32,         // C <= M; 0 with a null list: all M in order
    pub reserved: u32,               // must be 0
    pub out_channels: *const u32,    // [C] distinct indices 0 .. M-1: plane i is channel out_channels[i]
}
pub enum GmChannelizer {}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmNullerCfg {            // gm_nuller_cfg (24 bytes; zeros: the defaults)
    pub n_antennas: u32,             // A: 2 .. 8, interleaved time sample by time sample in one stream
    pub block: u32,                  // B: a power of two in 256 .. 16384; 0 -> 1024
    pub loading: f32,                // [1e-6, 1] of the mean antenna power; 0 -> 1e-4
    pub reserved: u32,               // must be 0
    pub steering: *const Complex32,  // [A] finite words, not all zero; null -> e_0 (antenna 0 as the reference)
}
pub enum GmNuller {}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmStapCfg {              // gm_stap_cfg (32 bytes; zeros: the defaults)
    pub n_antennas: u32,             // A: 2 .. 8, interleaved time sample by time sample in one stream
    pub taps: u32,                   // L: 1 .. 8 taps in time behind every antenna, A L <= 32
    pub block: u32,                  // B: a power of two in 256 .. 16384; 0 -> 1024
    pub loading: f32,                // [1e-6, 1] of the mean stacked power; 0 -> 1e-4
    pub steering: *const Complex32,  // [L][A] finite words, not all zero; null -> e_0 (antenna 0 at tap 0)
    pub reserved: u64,               // must be 0
}
pub enum GmStap {}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmBeamformerCfg {        // gm_beamformer_cfg (40 bytes; zeros: the defaults of block and loading)
    pub n_antennas: u32,             // A: 2 .. 8, gm_stap's stream
    pub taps: u32,                   // L: 1 .. 8, A L <= 32
    pub block: u32,                  // B: a power of two in 256 .. 16384; 0 -> 1024
    pub loading: f32,                // [1e-6, 1] of the mean stacked power; 0 -> 1e-4
    pub n_beams: u32,                // P: 1 .. 16
    pub reserved32: u32,             // must be 0
    pub steering: *const Complex32,  // [P][L][A], every row finite and not all zero; required
    pub reserved: u64,               // must be 0
}
pub enum GmBeamformer {}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct GmLcmvCfg {              // gm_lcmv_cfg (56 bytes; zeros: the defaults of block and loading)
    pub n_antennas: u32,             // A: 2 .. 8, gm_stap's stream
    pub taps: u32,                   // L: 1 .. 8, A L <= 32
    pub block: u32,                  // B: a power of two in 256 .. 16384; 0 -> 1024
    pub loading: f32,                // [1e-6, 1] of the mean stacked power; 0 -> 1e-4
    pub n_beams: u32,                // P: 1 .. 16
    pub reserved32: u32,             // must be 0
    pub n_constraints: *const u32,   // [P]: Q_p in 1 .. 8, Q_p <= A L, their sum <= 16; required
    pub constraints: *const Complex32, // [sum Q][L][A], beam 0's rows first, a beam's rows independent; required
    pub response: *const Complex32,  // [sum Q], in the rows' order; required
    pub reserved: u64,               // must be 0
}
pub enum GmLcmv {}
pub enum GmAcq {} pub enum GmTrk {} pub enum GmRing {} pub enum GmComm {} pub enum GmFrontend {} pub enum GmResampler {} pub enum GmExcisor {}

extern "C" {
    pub fn gm_init(device: c_int) -> c_int;
    pub fn gm_last_error() -> *const c_char;
    // do_acquisition.rs:252-271  (tables + AcquisitionWorker::new for every PRN)
    pub fn gm_acq_create(cfg: *const GmAcqCfg, out: *mut *mut GmAcq) -> c_int;
    pub fn gm_acq_destroy(a: *mut GmAcq) -> c_int;
    // the coherent fold's phasor words [n_bins][coherent_periods] (gm_acq_cfg.coherent_periods, ABI 9)
    pub fn gm_acq_coherent_phasors(a: *mut GmAcq, out: *mut Complex32) -> c_int;
    // the edge search of a coherent handle (additive entries, ABI stays 9: detect them by the symbol): H period offsets and an
    // optional secondary row of +-1; a dwell is then (K * n_integrations + offsets[H-1]) periods
    pub fn gm_acq_edge_dwell_periods(coherent_periods: u32, n_integrations: u32, n_offsets: u32, offsets: *const u32,
                                     secondary: *const i8, dwell_periods: *mut u64) -> c_int;
    pub fn gm_acq_set_edge_search(a: *mut GmAcq, n_offsets: u32, offsets: *const u32, secondary: *const i8) -> c_int;
    pub fn gm_acq_edge_metrics(a: *mut GmAcq, max: *mut f32, argmax: *mut u32, sum: *mut f32) -> c_int;
    pub fn gm_acq_edge_choice(a: *mut GmAcq, hypothesis: *mut u32) -> c_int;
    pub fn gm_acq_result_offsets(a: *mut GmAcq, results: *const GmAcqResult, found: *const u8, n_prn: u32,
                                 offset_periods: *mut u32) -> c_int;
    // code-drift compensation (additive entries, ABI stays 9): per-bin true code periods in samples; period p of the dwell starts at
    // floor(p * T_d + 0.5) and a dwell is gm_acq_dwell_samples long
    pub fn gm_acq_set_code_drift(a: *mut GmAcq, n_bins: u32, period_samples: *const f64) -> c_int;
    pub fn gm_acq_code_drift_plan(fft_size: u32, n_periods: u32, n_bins: u32, period_samples: *const f64, starts: *mut u64,
                                  dwell_samples: *mut u64) -> c_int;
    pub fn gm_acq_dwell_samples(a: *mut GmAcq, out: *mut u64) -> c_int;
    pub fn gm_acq_code_drift_starts(a: *mut GmAcq, out: *mut u64) -> c_int;
    pub fn gm_acq_code_drift_phasors(a: *mut GmAcq, h: u32, out: *mut Complex32) -> c_int;
    // fine Doppler from per-period prompts (additive entries, ABI stays 9): the search's own statistic on a fine frequency grid around
    // the winning bin, with the handle's coherent groups, edge offset, secondary row and code-drift starts
    pub fn gm_acq_refine_doppler(a: *mut GmAcq, results: *const GmAcqResult, found: *const u8, n_prn: u32, cfg: *const GmAcqRefineCfg,
                                 out: *mut GmAcqRefineOut, prompts: *mut Complex32, spectrum: *mut f32) -> c_int;
    pub fn gm_acq_refine_plan(coherent_periods: u32, n_integrations: u32, cfg: *const GmAcqRefineCfg, fs: f32, fft_size: u32,
                              n_bins: u32, table_freq: *const f32, bin: u32, span_periods: *mut u32, n_groups: *mut u32,
                              n_freq: *mut u32, half_span_hz: *mut f64, step_hz: *mut f64) -> c_int;
    // lag window x fine Doppler at known cells (additive entries, ABI stays 9): gm_acq_refine_doppler's statistic on 2 L + 1 code
    // phases around a predicted one, from one pass over the samples; d_samples null: the snapshot of the last search
    pub fn gm_acq_local_search(a: *mut GmAcq, d_samples: *const c_void, fmt: c_int, cands: *const GmAcqCand, n_cands: u32,
                               cfg: *const GmAcqLocalCfg, out: *mut GmAcqLocalOut, prompts: *mut Complex32, surface: *mut f32) -> c_int;
    pub fn gm_acq_local_plan(coherent_periods: u32, n_integrations: u32, cfg: *const GmAcqLocalCfg, fs: f32, fft_size: u32,
                             n_bins: u32, table_freq: *const f32, bin: u32, n_lags: *mut u32, span_periods: *mut u32,
                             n_groups: *mut u32, n_freq: *mut u32, half_span_hz: *mut f64, step_hz: *mut f64) -> c_int;
    // beam rows from the array's own correlations (additive entries, ABI stays 9): every antenna and tap delay of an interleaved array
    // stream against a candidate's replica, z = [n_cands][R_u][taps][n_antennas] on the host; then a row per cell on the host in f64
    pub fn gm_acq_array_prompts(a: *mut GmAcq, d_samples: *const c_void, fmt: c_int, n_antennas: u32, taps: u32,
                                cands: *const GmAcqCand, n_cands: u32, z: *mut Complex32) -> c_int;
    pub fn gm_acq_array_plan(coherent_periods: u32, n_integrations: u32, n_antennas: u32, taps: u32, periods: *mut u32,
                             words_per_cand: *mut u32) -> c_int;
    pub fn gm_array_row_solve(m: u32, n: u32, z: *const Complex32, r: *const Complex32, n_blocks: usize, loading: f32,
                              row: *mut Complex32, info: *mut GmArrayRowInfo) -> c_int;
    /// re-steering on the device: the rules and extents of a batched solve (host only), and the solve itself, asynchronous on `stream`
    /// (d_info[p].reserved is row p's status, 0: solved)
    pub fn gm_array_solve_plan(cfg: *const GmArraySolveCfg, z_words: *mut u64, r_words: *mut u64, row_words: *mut u64) -> c_int;
    pub fn gm_array_rows_solve_dev(cfg: *const GmArraySolveCfg, d_z: *const c_void, d_r: *const c_void, d_rows: *mut c_void,
                                   d_info: *mut c_void, stream: *mut c_void) -> c_int;
    // subtracting found satellites from a dwell (additive entries, ABI stays 9): one amplitude per signal code period and candidate,
    // estimated from the input; the output is c32 in device memory; d_samples null: the snapshot of the last search
    pub fn gm_acq_cancel(a: *mut GmAcq, d_samples: *const c_void, fmt: c_int, cands: *const GmAcqCancelCand, n_cands: u32,
                         d_out: *mut c_void, out: *mut GmAcqCancelOut, amps: *mut Complex32, amps_stride: u32) -> c_int;
    pub fn gm_acq_cancel_plan(dwell_samples: u64, fft_size: u32, code_phase: f64, period_samples: f64, n_segments: *mut u32,
                              bounds: *mut u64, bounds_cap: u32) -> c_int;
    // do_acquisition.rs:302-313 + :158-226  (par_iter over workers / search_satellite)
    pub fn gm_acq_search_c32(a: *mut GmAcq, samples: *const Complex32, n: usize, local_tail: u64,
                             prn_mask: u64, results: *mut GmAcqResult, found: *mut u8) -> c_int;
    pub fn gm_acq_search_i8(a: *mut GmAcq, iq: *const i8, n: usize, local_tail: u64, prn_mask: u64,
                            results: *mut GmAcqResult, found: *mut u8) -> c_int;
    // doppler_shift.rs:10-22, :25-58
    pub fn gm_doppler_table_new(f_if: f32, doppler: f32, fs: f32, n: usize, freq_out: *mut f32, table: *mut Complex32) -> c_int;
    pub fn gm_apply_doppler_shift(s: *const Complex32, t: *const Complex32, out: *mut Complex32, n: usize) -> c_int;
    // multicast_ring_buffer.rs:46-129 (device mirror fed next to the host ring)
    pub fn gm_ring_create(buf_size: usize, out: *mut *mut GmRing) -> c_int;
    pub fn gm_ring_destroy(r: *mut GmRing) -> c_int;
    pub fn gm_ring_write_samples(r: *mut GmRing, s: *const Complex32, n: usize) -> c_int;
    pub fn gm_ring_get_head(r: *mut GmRing, head: *mut u64) -> c_int;
    pub fn gm_ring_write_samples_async(r: *mut GmRing, s: *const Complex32, n: usize) -> c_int;
    pub fn gm_ring_flush(r: *mut GmRing) -> c_int;
    pub fn gm_ring_get_enqueued_head(r: *mut GmRing, head: *mut u64) -> c_int;
    // rf/frontend.rs:19-62 (DigitalFrontend::new, process_block) and rf_thread.rs:43-48 (the block step into the ring)
    pub fn gm_frontend_create(f_if: f32, fs_in: f32, fs_out: f32, out: *mut *mut GmFrontend) -> c_int;
    pub fn gm_frontend_destroy(f: *mut GmFrontend) -> c_int;
    pub fn gm_frontend_process_block(f: *mut GmFrontend, raw_floats: *mut f32, n_floats: usize) -> c_int;
    pub fn gm_frontend_write_ring(f: *mut GmFrontend, ring: *mut GmRing, samples: *const c_void, n_samples: usize, fmt: c_int) -> c_int;
    // rate conversion and pulse blanking (additive entries, ABI stays 9): the two stages frontend.rs names in comments and leaves out;
    // fs_out = fs_in * up / down, every output defined by absolute sample indices; plan and design are host only
    pub fn gm_resampler_plan(cfg: *const GmResamplerCfg, inputs_so_far: u64, n_in: u64, up_reduced: *mut u32, down_reduced: *mut u32,
                             taps: *mut u32, n_phases: *mut u32, n_out: *mut u64) -> c_int;
    pub fn gm_resampler_design(cfg: *const GmResamplerCfg, table: *mut f32) -> c_int;
    pub fn gm_resampler_create(cfg: *const GmResamplerCfg, out: *mut *mut GmResampler) -> c_int;
    pub fn gm_resampler_destroy(r: *mut GmResampler) -> c_int;
    pub fn gm_resampler_reset(r: *mut GmResampler, input_index: u64) -> c_int;
    pub fn gm_resampler_taps(r: *mut GmResampler, table: *mut f32) -> c_int;
    pub fn gm_resampler_stats(r: *mut GmResampler, inputs: *mut u64, outputs: *mut u64, blanked: *mut u64) -> c_int;
    pub fn gm_resampler_process_dev(r: *mut GmResampler, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void,
                                    out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_resampler_process(r: *mut GmResampler, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32,
                                out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn gm_resampler_synchronize(r: *mut GmResampler) -> c_int;
    /// gm_frontend_write_ring with the resampler between the front-end and the ring: ring indices then count OUTPUT samples
    pub fn gm_frontend_write_ring_resampled(f: *mut GmFrontend, r: *mut GmResampler, ring: *mut GmRing, samples: *const c_void,
                                            n_samples: usize, fmt: c_int, n_out_total: *mut u64) -> c_int;
    // narrowband interference excision (additive entries, ABI stays 9): a 50 % overlap-add filter bank with a per-bin gain, same rate
    // and sample index; every output defined by absolute sample indices; plan and windows are host only
    pub fn gm_excisor_plan(cfg: *const GmExcisorCfg, inputs_so_far: u64, n_in: u64, block: *mut u32, guard_bins: *mut u32,
                           threshold_factor: *mut f32, n_out: *mut u64) -> c_int;
    pub fn gm_excisor_windows(cfg: *const GmExcisorCfg, analysis: *mut f32, synthesis: *mut f32) -> c_int;
    pub fn gm_excisor_create(cfg: *const GmExcisorCfg, out: *mut *mut GmExcisor) -> c_int;
    pub fn gm_excisor_destroy(x: *mut GmExcisor) -> c_int;
    pub fn gm_excisor_reset(x: *mut GmExcisor, input_index: u64) -> c_int;
    pub fn gm_excisor_set_gains(x: *mut GmExcisor, gains: *const f32) -> c_int;
    pub fn gm_excisor_gains(x: *mut GmExcisor, gains: *mut f32) -> c_int;
    /// periodogram, median, mask and gains from n device samples: enqueued on `stream`, no host wait
    pub fn gm_excisor_adapt_dev(x: *mut GmExcisor, d_in: *const c_void, fmt: c_int, n: usize, stream: *mut c_void) -> c_int;
    pub fn gm_excisor_psd(x: *mut GmExcisor, p: *mut f32, median: *mut f32, n_flagged: *mut u32, n_zeroed: *mut u32) -> c_int;
    pub fn gm_excisor_stats(x: *mut GmExcisor, inputs: *mut u64, outputs: *mut u64, blanked: *mut u64) -> c_int;
    pub fn gm_excisor_process_dev(x: *mut GmExcisor, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void,
                                  out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_excisor_process(x: *mut GmExcisor, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32,
                              out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn gm_excisor_synchronize(x: *mut GmExcisor) -> c_int;
    /// block-adapt mode: host-only argument rules and defaults; on (cfg) / off (null); the counters; the capture of process_dev
    pub fn gm_excisor_block_plan(cfg: *const GmExcisorBlockCfg, threshold_factor: *mut f32, guard_bins: *mut u32) -> c_int;
    pub fn gm_excisor_set_block_adapt(x: *mut GmExcisor, cfg: *const GmExcisorBlockCfg) -> c_int;
    pub fn gm_excisor_block_stats(x: *mut GmExcisor, blocks: *mut u64, blocks_flagged: *mut u64, bins_flagged: *mut u64,
                                  bins_zeroed: *mut u64) -> c_int;
    pub fn gm_excisor_block_capture(x: *mut GmExcisor, d_power: *mut f32, d_mask: *mut u8, cap_blocks: usize) -> c_int;
    /// gm_frontend_write_ring_resampled with the excisor between the front-end and the resampler; `r` may be null
    pub fn gm_frontend_write_ring_conditioned(f: *mut GmFrontend, x: *mut GmExcisor, r: *mut GmResampler, ring: *mut GmRing,
                                              samples: *const c_void, n_samples: usize, fmt: c_int, n_out_total: *mut u64) -> c_int;

    /// real-IF int8 down-conversion to complex baseband: blank, an exact integer NCO, the resampler's polyphase filter
    pub fn gm_ddc_plan(cfg: *const GmDdcCfg, inputs_so_far: u64, n_in: u64, up_reduced: *mut u32, down_reduced: *mut u32,
                       taps: *mut u32, n_phases: *mut u32, phase_inc: *mut u64, n_out: *mut u64) -> c_int;
    pub fn gm_ddc_create(cfg: *const GmDdcCfg, out: *mut *mut GmDdc) -> c_int;
    pub fn gm_ddc_destroy(d: *mut GmDdc) -> c_int;
    pub fn gm_ddc_reset(d: *mut GmDdc, input_index: u64) -> c_int;
    pub fn gm_ddc_stats(d: *mut GmDdc, inputs: *mut u64, outputs: *mut u64, blanked: *mut u64) -> c_int;
    pub fn gm_ddc_synchronize(d: *mut GmDdc) -> c_int;
    pub fn gm_ddc_tables(d: *mut GmDdc, table: *mut f32, whi: *mut Complex32, wlo: *mut Complex32) -> c_int;
    pub fn gm_ddc_process_dev(d: *mut GmDdc, d_in: *const c_void, n_in: usize, d_out: *mut c_void, out_cap: usize,
                              n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_ddc_process(d: *mut GmDdc, input: *const i8, n_in: usize, out: *mut Complex32, out_cap: usize,
                          n_out: *mut usize) -> c_int;
    /// gm_frontend_write_ring_conditioned with the down-converter in the front-end's place; `x` and `r` may each be null
    pub fn gm_ddc_write_ring(d: *mut GmDdc, x: *mut GmExcisor, r: *mut GmResampler, ring: *mut GmRing, samples: *const i8,
                             n_samples: usize, n_out_total: *mut u64) -> c_int;

    /// polyphase filter bank: M sub-bands of one c32 / int8-IQ stream, each a c32 stream at fs / D; d_out is [C][out_stride]
    pub fn gm_channelizer_plan(cfg: *const GmChannelizerCfg, inputs_so_far: u64, n_in: u64, n_out_channels: *mut u32,
                               taps_per_branch: *mut u32, n_taps: *mut u32, n_out: *mut u64) -> c_int;
    pub fn gm_channelizer_design(cfg: *const GmChannelizerCfg, taps: *mut f32) -> c_int;
    pub fn gm_channelizer_create(cfg: *const GmChannelizerCfg, out: *mut *mut GmChannelizer) -> c_int;
    pub fn gm_channelizer_destroy(c: *mut GmChannelizer) -> c_int;
    pub fn gm_channelizer_reset(c: *mut GmChannelizer, input_index: u64) -> c_int;
    pub fn gm_channelizer_taps(c: *mut GmChannelizer, taps: *mut f32) -> c_int;
    pub fn gm_channelizer_stats(c: *mut GmChannelizer, inputs: *mut u64, outputs: *mut u64, blanked: *mut u64) -> c_int;
    pub fn gm_channelizer_process_dev(c: *mut GmChannelizer, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void,
                                      out_stride: usize, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_channelizer_process(c: *mut GmChannelizer, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32,
                                  out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn gm_channelizer_synchronize(c: *mut GmChannelizer) -> c_int;
    /// the GLONASS L1OF ranging code: 511 chips, +1 for logic 0
    pub fn gm_glonass_code(out_chips: *mut i8) -> c_int;

    /// adaptive spatial nulling: A interleaved antennas -> one c32 stream, the weights of a block from its own covariance; every
    /// count is in TIME samples
    pub fn gm_nuller_plan(cfg: *const GmNullerCfg, inputs_so_far: u64, n_in: u64, block: *mut u32, loading: *mut f32,
                          n_out: *mut u64) -> c_int;
    pub fn gm_nuller_create(cfg: *const GmNullerCfg, out: *mut *mut GmNuller) -> c_int;
    pub fn gm_nuller_destroy(n: *mut GmNuller) -> c_int;
    pub fn gm_nuller_reset(n: *mut GmNuller, input_index: u64) -> c_int;
    pub fn gm_nuller_stats(n: *mut GmNuller, inputs: *mut u64, outputs: *mut u64, blocks: *mut u64) -> c_int;
    pub fn gm_nuller_synchronize(n: *mut GmNuller) -> c_int;
    /// static mode: A fixed weights for every later block; null: back to the adaptive rule
    pub fn gm_nuller_set_weights(n: *mut GmNuller, w: *const Complex32) -> c_int;
    /// device buffers [cap_blocks][A][A] and [cap_blocks][A] that every later gm_nuller_process_dev fills from word 0
    pub fn gm_nuller_capture(n: *mut GmNuller, d_r: *mut c_void, d_w: *mut c_void, cap_blocks: usize) -> c_int;
    pub fn gm_nuller_process_dev(n: *mut GmNuller, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void, out_cap: usize,
                                 n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_nuller_process(n: *mut GmNuller, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32, out_cap: usize,
                             n_out: *mut usize, r: *mut Complex32, w: *mut Complex32, cap_blocks: usize) -> c_int;

    /// space-time adaptive nulling: the nuller's stream with L taps in time behind every antenna, M = A L weights a block from the
    /// exact Gram matrix of its stacked samples z[t][l A + a] = x_a[t - l]; every count is in TIME samples
    pub fn gm_stap_plan(cfg: *const GmStapCfg, inputs_so_far: u64, n_in: u64, block: *mut u32, loading: *mut f32,
                        n_out: *mut u64) -> c_int;
    pub fn gm_stap_create(cfg: *const GmStapCfg, out: *mut *mut GmStap) -> c_int;
    pub fn gm_stap_destroy(n: *mut GmStap) -> c_int;
    pub fn gm_stap_reset(n: *mut GmStap, input_index: u64) -> c_int;
    pub fn gm_stap_stats(n: *mut GmStap, inputs: *mut u64, outputs: *mut u64, blocks: *mut u64, fallback_blocks: *mut u64) -> c_int;
    pub fn gm_stap_synchronize(n: *mut GmStap) -> c_int;
    /// static mode: M fixed weights [L][A] for every later block; null: back to the adaptive rule
    pub fn gm_stap_set_weights(n: *mut GmStap, w: *const Complex32) -> c_int;
    /// device buffers [cap_blocks][M][M] and [cap_blocks][M] that every later gm_stap_process_dev fills from word 0
    pub fn gm_stap_capture(n: *mut GmStap, d_r: *mut c_void, d_w: *mut c_void, cap_blocks: usize) -> c_int;
    pub fn gm_stap_process_dev(n: *mut GmStap, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void, out_cap: usize,
                               n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_stap_process(n: *mut GmStap, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32, out_cap: usize,
                           n_out: *mut usize, r: *mut Complex32, w: *mut Complex32, cap_blocks: usize) -> c_int;

    /// one beam per constraint row from ONE Gram matrix and ONE factor a block: beam p's words are those of a gm_stap with
    /// steering = row p; planar output, beam p at d_out + p * out_stride; every count is in TIME samples, n_out per beam
    pub fn gm_beamformer_plan(cfg: *const GmBeamformerCfg, inputs_so_far: u64, n_in: u64, block: *mut u32, loading: *mut f32,
                              n_out: *mut u64) -> c_int;
    pub fn gm_beamformer_create(cfg: *const GmBeamformerCfg, out: *mut *mut GmBeamformer) -> c_int;
    pub fn gm_beamformer_destroy(h: *mut GmBeamformer) -> c_int;
    pub fn gm_beamformer_reset(h: *mut GmBeamformer, input_index: u64) -> c_int;
    /// fallbacks: P words, one per beam
    pub fn gm_beamformer_stats(h: *mut GmBeamformer, inputs: *mut u64, outputs: *mut u64, blocks: *mut u64, fallbacks: *mut u64) -> c_int;
    pub fn gm_beamformer_synchronize(h: *mut GmBeamformer) -> c_int;
    /// beam `beam`'s new row of M words for every block a later call finishes; synchronous
    pub fn gm_beamformer_set_steering(h: *mut GmBeamformer, beam: u32, s: *const Complex32) -> c_int;
    pub fn gm_beamformer_set_steering_dev(h: *mut GmBeamformer, first_beam: u32, n_rows: u32, d_rows: *const c_void, d_info: *const c_void,
                                          min_ratio: f32, d_installed: *mut c_void, stream: *mut c_void) -> c_int;
    /// static mode: P M fixed weights [P][L][A] for every later block (synchronous); null: back to the adaptive rule
    pub fn gm_beamformer_set_weights(h: *mut GmBeamformer, w: *const Complex32) -> c_int;
    /// device buffers [cap_blocks][M][M] and [cap_blocks][P][M] that every later gm_beamformer_process_dev fills from word 0
    pub fn gm_beamformer_capture(h: *mut GmBeamformer, d_r: *mut c_void, d_w: *mut c_void, cap_blocks: usize) -> c_int;
    pub fn gm_beamformer_process_dev(h: *mut GmBeamformer, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void,
                                     out_stride: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_beamformer_process(h: *mut GmBeamformer, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32,
                                 out_stride: usize, n_out: *mut usize, r: *mut Complex32, w: *mut Complex32, cap_blocks: usize) -> c_int;
    /// several constraints on one beam: beam p carries Q_p rows and responses, C^H w_p = f at the least output power; ONE Gram matrix
    /// and ONE factor a block; planar output, beam p at d_out + p * out_stride; every count is in TIME samples, n_out per beam
    pub fn gm_lcmv_plan(cfg: *const GmLcmvCfg, inputs_so_far: u64, n_in: u64, block: *mut u32, loading: *mut f32, n_out: *mut u64) -> c_int;
    pub fn gm_lcmv_create(cfg: *const GmLcmvCfg, out: *mut *mut GmLcmv) -> c_int;
    pub fn gm_lcmv_destroy(h: *mut GmLcmv) -> c_int;
    pub fn gm_lcmv_reset(h: *mut GmLcmv, input_index: u64) -> c_int;
    /// fallbacks: P words, one per beam
    pub fn gm_lcmv_stats(h: *mut GmLcmv, inputs: *mut u64, outputs: *mut u64, blocks: *mut u64, fallbacks: *mut u64) -> c_int;
    pub fn gm_lcmv_synchronize(h: *mut GmLcmv) -> c_int;
    /// beam `beam`'s new rows [n_rows][M] and responses [n_rows] for every block a later call finishes; synchronous
    pub fn gm_lcmv_set_constraints(h: *mut GmLcmv, beam: u32, n_rows: u32, rows: *const Complex32, response: *const Complex32) -> c_int;
    /// static mode: P M fixed weights [P][L][A] for every later block (synchronous); null: back to the adaptive rule
    pub fn gm_lcmv_set_weights(h: *mut GmLcmv, w: *const Complex32) -> c_int;
    /// device buffers [cap_blocks][M][M] and [cap_blocks][P][M] that every later gm_lcmv_process_dev fills from word 0
    pub fn gm_lcmv_capture(h: *mut GmLcmv, d_r: *mut c_void, d_w: *mut c_void, cap_blocks: usize) -> c_int;
    pub fn gm_lcmv_process_dev(h: *mut GmLcmv, d_in: *const c_void, fmt: c_int, n_in: usize, d_out: *mut c_void, out_stride: usize,
                               n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gm_lcmv_process(h: *mut GmLcmv, input: *const c_void, fmt: c_int, n_in: usize, out: *mut Complex32, out_stride: usize,
                           n_out: *mut usize, r: *mut Complex32, w: *mut Complex32, cap_blocks: usize) -> c_int;
    // do_tracking.rs:118-158, 311-327
    pub fn gm_trk_create(cfg: *const GmTrkCfg, out: *mut *mut GmTrk) -> c_int;
    pub fn gm_trk_destroy(t: *mut GmTrk) -> c_int;
    pub fn gm_trk_start(t: *mut GmTrk, ch: u32, r: *const GmAcqResult) -> c_int;
    pub fn gm_trk_reset(t: *mut GmTrk, ch: u32) -> c_int;
    pub fn gm_trk_get_state(t: *mut GmTrk, ch: u32, out: *mut GmTrkState) -> c_int;
    pub fn gm_trk_set_state(t: *mut GmTrk, ch: u32, state: *const GmTrkState) -> c_int;
    // do_tracking.rs:274-277, :52-71
    pub fn gm_trk_get_ca_chip(t: *mut GmTrk, ch: u32, phase: f32, chip: *mut f32) -> c_int;
    pub fn gm_loop_filter_new(noise_bw: f32, damping: f32, gain: f32, tau1: *mut f32, tau2: *mut f32) -> c_int;
    pub fn gm_loop_filter_update(tau1: f32, tau2: f32, d_err: f32, err: f32, dt: f32) -> f32;
    // do_tracking.rs:231-272, :183-210 on caller samples; :351-371 batched over the ring
    pub fn gm_trk_correlate(t: *mut GmTrk, ch: u32, s: *const Complex32, n: usize, out: *mut GmTrkOut) -> c_int;
    pub fn gm_trk_do_work(t: *mut GmTrk, ch: u32, s: *const Complex32, n: usize, out: *mut GmTrkOut,
                          lost: *mut u8, lost_prn: *mut u8) -> c_int;
    pub fn gm_trk_update_all(t: *mut GmTrk, ring: *mut GmRing, max_epochs: u32, outs: *mut GmTrkOut,
                             processed: *mut u8, lost: *mut u8, epochs_done: *mut u32) -> c_int;
    /// the same passes ordered on the DEVICE behind what the ring's writer has enqueued (the Condvar wait of :392-406 without a host wait)
    pub fn gm_trk_update_all_async(t: *mut GmTrk, ring: *mut GmRing, max_epochs: u32, ticket: *mut u64) -> c_int;
    /// states (ABI 7): the channel records as they stood behind THAT call's passes; a collect that fails has consumed the ticket
    pub fn gm_trk_collect(t: *mut GmTrk, ticket: u64, wait: c_int, outs: *mut GmTrkOut, processed: *mut u8, lost: *mut u8,
                          states: *mut GmTrkState, epochs_done: *mut u32, ready: *mut c_int) -> c_int;
    /// every channel's record in one synchronisation + one copy; `which`: NULL = all, else per-channel flags
    pub fn gm_trk_get_states(t: *mut GmTrk, out: *mut GmTrkState) -> c_int;
    pub fn gm_trk_set_states(t: *mut GmTrk, states: *const GmTrkState, which: *const u8) -> c_int;
    /// the correlator bank at tracked states: T taps x F carrier offsets of one code period per record, nothing advanced
    /// (states null: the handle's own channels, n_states = n_channels; out: [n_states][F][T]; done: [n_states] or null)
    pub fn gm_trk_bank_plan(trk: *const GmTrkCfg, cfg: *const GmTrkBankCfg, n_states: u32, out: *mut GmTrkBankPlanOut) -> c_int;
    pub fn gm_trk_bank(t: *mut GmTrk, ring: *mut GmRing, states: *const GmTrkState, n_states: u32, cfg: *const GmTrkBankCfg,
                       out: *mut Complex32, done: *mut u8) -> c_int;
    pub fn gm_trk_bank_samples(t: *mut GmTrk, state: *const GmTrkState, s: *const Complex32, n: usize, cfg: *const GmTrkBankCfg,
                               out: *mut Complex32) -> c_int;
    /// per-antenna prompts at tracked states: one code period of an interleaved array stream on the device (n_time time samples from
    /// absolute time first_index, fmt 0 = c32 or 1 = int8 IQ, written before the call) against the tracker's replica per record, every
    /// antenna and tap delay at once, nothing advanced (states null: the handle's own channels, n_states = n_channels;
    /// z: [n_states][L][A], host, the word order gm_array_row_solve takes; done: [n_states] or null)
    pub fn gm_trk_array_plan(trk: *const GmTrkCfg, cfg: *const GmTrkArrayCfg, n_states: u32, out: *mut GmTrkArrayPlanOut) -> c_int;
    pub fn gm_trk_array_prompts(t: *mut GmTrk, d_samples: *const c_void, fmt: c_int, first_index: u64, n_time: u64,
                                states: *const GmTrkState, n_states: u32, cfg: *const GmTrkArrayCfg, z: *mut Complex32,
                                done: *mut u8) -> c_int;
    /// the same words into device buffers (d_z [n_states][L][A], d_done [n_states]), asynchronous on `stream` (null: the handle's own);
    /// states is required and read before the call returns
    pub fn gm_trk_array_prompts_dev(t: *mut GmTrk, d_samples: *const c_void, fmt: c_int, first_index: u64, n_time: u64,
                                    states: *const GmTrkState, n_states: u32, cfg: *const GmTrkArrayCfg, d_z: *mut c_void,
                                    d_done: *mut c_void, stream: *mut c_void) -> c_int;
    // plane ring (additive entries, ABI stays 9; bindings only): n_planes rings of c32 on one time axis with one head, written from
    // device memory (plane p's samples at d_planes + p * in_stride words: what gm_beamformer / gm_lcmv / gm_channelizer process_dev
    // leave), ordered on the device against its readers; plan is host only
    pub fn gm_plane_ring_plan(n_planes: u32, plane_size: u64, bytes: *mut u64) -> c_int;
    pub fn gm_plane_ring_create(n_planes: u32, plane_size: u64, out: *mut *mut GmPlaneRing) -> c_int;
    pub fn gm_plane_ring_destroy(pr: *mut GmPlaneRing) -> c_int;
    pub fn gm_plane_ring_info(pr: *mut GmPlaneRing, n_planes: *mut u32, plane_size: *mut u64, bytes: *mut u64, d_base: *mut *mut c_void) -> c_int;
    pub fn gm_plane_ring_write_dev(pr: *mut GmPlaneRing, d_planes: *const c_void, in_stride: usize, n: usize, stream: *mut c_void) -> c_int;
    pub fn gm_plane_ring_write(pr: *mut GmPlaneRing, planes: *const Complex32, in_stride: usize, n: usize) -> c_int;
    pub fn gm_plane_ring_get_head(pr: *mut GmPlaneRing, head: *mut u64) -> c_int;
    pub fn gm_plane_ring_copy_to_slice(pr: *mut GmPlaneRing, plane: u32, start: u64, dest: *mut Complex32, n: usize) -> c_int;
    pub fn gm_plane_ring_synchronize(pr: *mut GmPlaneRing) -> c_int;
    // tracking on planes: gm_trk_update_all's contract on a plane ring, channel c on plane planes[c] (null: all 0); every other entry
    // ignores the map; a strict_sum_order handle is refused; plan is host only
    pub fn gm_trk_planes_plan(trk: *const GmTrkCfg, n_planes: u32, planes: *const u32, max_epochs: u32, out: *mut GmTrkPlanesPlanOut) -> c_int;
    pub fn gm_trk_set_channel_planes(t: *mut GmTrk, planes: *const u32) -> c_int;
    pub fn gm_trk_get_channel_planes(t: *mut GmTrk, planes: *mut u32) -> c_int;
    pub fn gm_trk_update_planes(t: *mut GmTrk, pr: *mut GmPlaneRing, max_epochs: u32, outs: *mut GmTrkOut, processed: *mut u8,
                                lost: *mut u8, epochs_done: *mut u32) -> c_int;
    pub fn gm_trk_update_planes_dev(t: *mut GmTrk, pr: *mut GmPlaneRing, epochs: u32) -> c_int;
    // fft.rs:5-56
    pub fn gm_fft_c2c_f32(n: usize, dir: c_int, inout: *mut Complex32, batch: usize) -> c_int;
    pub fn gm_fft_power_spectrum_f32(n: usize, inout: *mut Complex32, power: *mut f32) -> c_int;
    pub fn gm_rfft_f32(n: usize, input: *const f32, out: *mut Complex32) -> c_int;
    // multi-GPU (nothing to replace in the reference; rayon's fan-out :302-313 becomes one process per GPU)
    pub fn gm_acq_search_dev(a: *mut GmAcq, d_samples: *const c_void, fmt: c_int, d_metrics: *mut c_void) -> c_int;
    pub fn gm_comm_get_unique_id(id: *mut u8 /* [128] */) -> c_int;
    pub fn gm_comm_init(nranks: c_int, rank: c_int, id: *const u8, out: *mut *mut GmComm) -> c_int;
    pub fn gm_comm_destroy(c: *mut GmComm) -> c_int;
    pub fn gm_acq_allgather_metrics(a: *mut GmAcq, c: *mut GmComm, d_local: *const c_void, d_all: *mut c_void) -> c_int;
    pub fn gm_acq_allgather_metrics_async(a: *mut GmAcq, c: *mut GmComm, d_local: *const c_void, d_all: *mut c_void) -> c_int;
    pub fn gm_comm_wait(c: *mut GmComm, hip_stream: *mut c_void) -> c_int;
    pub fn gm_comm_allgather_words(c: *mut GmComm, d_local: *const c_void, d_all: *mut c_void, words: usize, hip_stream: *mut c_void) -> c_int;
    pub fn gm_grid_assemble_dev(d_gathered: *const c_void, nranks: u32, p_max: u32, n_bins: u32, d_row_map: *const u32,
                                n_rows: u32, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn gm_acq_decide_planes_dev(d_max: *const f32, d_argmax: *const u32, d_sum: *const f32, n_prn: u32, n_bins: u32,
                                    d_prn_ids: *const u8, d_table_freq: *const f32, fft_size: u32, fs: f32, code_rate: f32,
                                    threshold: f32, decision_mode: c_int, local_tail: u64, d_results: *mut GmAcqResult,
                                    d_found: *mut u8, hip_stream: *mut c_void) -> c_int;
    pub fn gm_acq_decide_dev(a: *mut GmAcq, d_metrics: *const c_void, n_prn: u32, prn_ids: *const u8, local_tail: u64) -> c_int;
    pub fn gm_acq_fetch_results(a: *mut GmAcq, n_prn: u32, results: *mut GmAcqResult, found: *mut u8) -> c_int;
    /// back-to-back dwells: the decision rides inside the next search's first kernel
    pub fn gm_acq_set_deferred_decision(a: *mut GmAcq, on: c_int) -> c_int;
    /// back-to-back dwells: stage F of the next dwell beside the current stage C (pays at N = 16368)
    pub fn gm_acq_prepare_dev(a: *mut GmAcq, d_samples: *const c_void, fmt: c_int, ready_stream: *mut c_void, token: *mut u64) -> c_int;
    pub fn gm_acq_search_prepared_dev(a: *mut GmAcq, token: u64, d_metrics: *mut c_void) -> c_int;
    pub fn gm_acq_drop_prepared(a: *mut GmAcq) -> c_int;
}

/// status -> the last error text of the library (for panics that mirror the reference's)
pub fn last_error() -> String {
    unsafe { std::ffi::CStr::from_ptr(gm_last_error()).to_string_lossy().into_owned() }
}
