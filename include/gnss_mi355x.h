/*
 * gnss_mi355x.h — C ABI of the MI355X-native acquisition + tracking hot path.
 *
 * Drop-in boundary for the acquisition / tracking channel API of kewei/gnss-sdr-rs.  The reference
 * has no FFI for this path (its API is Rust: SURVEY.md §8b); every entry point below names the
 * reference item (file:line, relative to the reference checkout) it replaces, and INTEGRATION.md
 * shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; no exceptions cross the boundary
 *   - every function returns a gm_status (0 = GM_OK, < 0 = error); absence (`Option::None`) is
 *     reported through `found[]` flags, never through the status
 *   - handles are opaque and thread-compatible: one thread per handle at a time (the reference
 *     hands one `&mut` worker/channel to each rayon task)
 *   - host pointers unless the name ends in `_dev`; `_dev` pointers are HIP device pointers on the
 *     handle's device and the call is asynchronous on the handle's stream
 *   - STREAMS: every stream the library creates is NON-BLOCKING (hipStreamNonBlocking).  Work on the NULL stream (hipMemset,
 *     hipMemcpy of device memory, a launch without a stream) is NOT ordered against the library's work in either direction.  A
 *     device buffer handed to a `_dev` entry must be READY on the stream the handle works on: pass the producer's stream with
 *     gm_acq_set_stream / gm_trk_set_stream (the entry then runs behind the producer in stream order, and what it writes is ready
 *     on that stream), or synchronise the producer first.  gm_acq_prepare_dev takes the producer's stream per call
 *     (`ready_stream`).  The reference copies its 10 ms out of the ring and THEN searches them (do_acquisition.rs:297-313): the
 *     stream order is that sequence.  INTEGRATION.md §3.3; tests/test_gpu_acquisition.py::test_caller_stream_orders_...
 *     The streaming stage handles (gm_frontend, gm_resampler, gm_excisor, gm_ddc, gm_channelizer, gm_nuller, gm_stap, gm_beamformer) take the
 *     producer's stream per call, as the `stream` argument of their `_dev` entries: the call runs behind what the caller has queued there, its
 *     outputs and the handle's history are ready on that stream, and the handle's own queries, reset, host-buffer entry and ring
 *     writers wait for it (gm_frontend's wait for the handle's own stream only); tests/test_gpu_caller_streams.py.
 *   - arithmetic type: f32 everywhere, as in the reference (num_complex::Complex32 = {f32 re, im})
 *   - the compute path is HIP on gfx950 only; there is NO CPU fallback — without a usable device
 *     every compute entry returns GM_ERR_NO_DEVICE
 */
#ifndef GNSS_MI355X_H
#define GNSS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_ABI_VERSION 9   /* 9: gm_acq_cfg.coherent_periods, gm_acq_coherent_phasors; still 9, additive (no struct changed: a caller
                              detects the feature by the symbol): the edge search — gm_acq_edge_dwell_periods,
                              gm_acq_set_edge_search, gm_acq_edge_metrics, gm_acq_edge_choice, gm_acq_result_offsets;
                              and the code-drift compensation — gm_acq_set_code_drift, gm_acq_code_drift_plan,
                              gm_acq_dwell_samples, gm_acq_code_drift_starts, gm_acq_code_drift_phasors;
                              and the fine Doppler from per-period prompts — gm_acq_refine_doppler, gm_acq_refine_plan;
                              and the lag window x fine Doppler at known cells — gm_acq_local_search, gm_acq_local_plan;
                              and subtracting found satellites from a dwell — gm_acq_cancel, gm_acq_cancel_plan;
                              and the correlator bank at tracked states — gm_trk_bank_plan, gm_trk_bank, gm_trk_bank_samples;
                              and per-antenna prompts of an array stream at tracked states — gm_trk_array_plan, gm_trk_array_prompts;
                              8: gm_acq_cfg.any_length, gm_acq_plan_info;
                              7: gm_trk_collect hands over the channel states, gm_trk_get_states / gm_trk_set_states,
                              gm_ring_get_enqueued_head (round 6); 6: gm_acq_prepare_dev returns a token (round 5) */

typedef enum {
    GM_OK = 0,
    GM_ERR_INVALID_ARG = -1,   /* null pointer, bad size, prn out of range ... (the reference panics) */
    GM_ERR_UNSUPPORTED_N = -2, /* no in-LDS FFT plan for this fft_size (see gm_fft_supported_sizes) */
    GM_ERR_NO_DEVICE = -3,     /* no HIP device / gm_init not called */
    GM_ERR_HIP = -4,           /* a HIP runtime call failed; gm_last_error() has the text */
    GM_ERR_OUT_OF_RANGE = -5,  /* slice/index out of range (the reference panics: index out of bounds) */
    GM_ERR_ALIGNMENT = -6,     /* fft_size % 8 != 0: the reference's SIMD tails (doppler_shift.rs:26,
                                  do_acquisition.rs:230-234) would leave stale / uncounted elements */
    GM_ERR_NOMEM = -7,
    GM_ERR_UNSUPPORTED = -8    /* optional component absent (RCCL for the gm_comm_* entries) */
} gm_status;

/* num_complex::Complex32 */
typedef struct { float re, im; } gm_c32;

/* ------------------------------------------------------------------ library / device */
int gm_abi_version(void);
/* Select the HIP device for subsequently created handles (one process per GPU). */
int gm_init(int device);
int gm_device_count(int *count);
const char *gm_last_error(void);
const char *gm_status_string(int status);

/* ------------------------------------------------------------------ constants / code table
 * GPS_CA_CODE_32_PRN (src/constants/gps_ca_constants.rs:1-1346): row r <-> PRN r+1, chips +-1. */
int gm_ca_code_row(int row, int8_t out_chips[1023]);
/* BeiDou B1I ranging code of PRN 1..37 (BDS-SIS-ICD-B1I: 11-stage Gold code, 2046 chips at 2.046 Mcps; +1 <-> logic 0).
 * Not in the reference (its README names BeiDou, its code has GPS only): provided for BASELINE configs[3]'s grid, to be
 * passed as gm_acq_cfg.codes.  n_chips = 2046 for the ICD's code; 2047 yields the untruncated period. */
int gm_b1i_code(uint32_t prn, int8_t *out_chips, uint32_t n_chips);
/* The GLONASS L1OF ranging code (GLONASS ICD L1/L2: 511 chips at 511 kcps, the same for every satellite; +1 <-> logic 0, as in
 * gm_b1i_code).  Nine stages s1 .. s9, all ones at the start; each clock the output is s7, then s5 xor s9 is shifted into s1.  The
 * period is 511; the first 24 logic chips are 111111100000111101111100 and 256 of the 511 are ones.  The satellites differ in their
 * carriers (FDMA: k = -7 .. 6 at 1602 MHz + k 562.5 kHz), which a gm_channelizer separates; pass the code as gm_acq_cfg.codes. */
int gm_glonass_code(int8_t out_chips[511]);
/* generate_ca_code_samples(prn, code_rate, f_sampling) (src/utilities/ca_code.rs:12-27).
 * *n_out = round(fs/(code_rate/1023)); writes min(n, cap) samples.  GM_ERR_OUT_OF_RANGE where the
 * reference would panic (prn not in 1..=32, chip index reaching 1023). */
int gm_generate_ca_code_samples(uint8_t prn, float code_rate, float f_sampling, int8_t *out, size_t cap,
                                size_t *n_out);

/* ------------------------------------------------------------------ Doppler wipe-off
 * DopplerShiftTable::new(f_if, doppler_freq_hz, fs, num_samples) (src/acquisition/doppler_shift.rs:10-22).
 * Host-side (glibc cosf/sinf, exactly the reference's arithmetic); *doppler_freq_hz_out receives the
 * stored field (= f_if + doppler, :20). */
int gm_doppler_table_new(float f_if, float doppler_freq_hz, float fs, size_t num_samples,
                         float *doppler_freq_hz_out, gm_c32 *table_out);
/* apply_doppler_shift(samples, table, output) (doppler_shift.rs:25-58) on the GPU.
 * Writes only the first 4*floor(n/4) outputs, like the reference. */
int gm_apply_doppler_shift(const gm_c32 *samples, const gm_c32 *table, gm_c32 *output, size_t n);

/* ------------------------------------------------------------------ FFT<T> / RealFFT<T> (src/fft.rs:5-56)
 * Unnormalised complex FFT, in place, `batch` contiguous transforms of length n.
 * dir: 0 forward (FFT::execute), 1 inverse.  n: one of gm_fft_supported_sizes() (one in-LDS transform), or ANY other
 * length up to 8192 (Bluestein on the smallest power-of-two plan >= 2n - 1; the reference's FFT<T> is generic over n). */
int gm_fft_c2c_f32(size_t n, int dir, gm_c32 *inout, size_t batch);
/* FFT::power_spectrum (src/fft.rs:27-29): transforms `inout` in place and writes |X|^2. */
int gm_fft_power_spectrum_f32(size_t n, gm_c32 *inout, float *power);
/* RealFFT::execute (src/fft.rs:45-49): n real inputs -> n/2+1 bins. */
int gm_rfft_f32(size_t n, const float *in, gm_c32 *out);
/* Sizes with an in-LDS plan; returns how many were written (<= cap). */
int gm_fft_supported_sizes(uint32_t *sizes, int cap);

/* ------------------------------------------------------------------ Acquisition
 * AcquisitionResult (src/acquisition/do_acquisition.rs:93-116) + the winning table index. */
typedef struct {
    uint8_t prn;
    uint64_t code_phase_samples;
    float code_phase_chips;
    float carrier_freq;        /* DopplerShiftTable.doppler_freq_hz of the winning bin = IF + Doppler */
    float fs;
    float mag_relative;        /* raw accumulated peak power (do_acquisition.rs:219) */
    uint64_t sample_global_index;
    int32_t doppler_bin;       /* extra: index into the table list */
} gm_acq_result;

typedef enum { GM_FMT_C32 = 0, GM_FMT_I8_IQ = 1, GM_FMT_I8_REAL = 2 } gm_sample_format;

typedef struct {
    float fs;                  /* freq_sampling_hz */
    float f_if;                /* used only when `tables` is NULL */
    uint32_t fft_size;         /* samples per code period (do_acquisition.rs:249-251): one of gm_fft_supported_sizes()
                                  (fused in-LDS kernels), or Q x {16000, 8000, 8192, 6000, 5000, 4000}, Q in {2,3,4,5,6,8}
                                  (e.g. 32000 for a 4 ms code at 8 Msps, 25000 for GPS at 25 Msps: composite path,
                                  transforms decimated in time, no intermediate plane in HBM); with any_length = 1 any
                                  multiple of 8 in [1024, 262144] (see any_length, gm_acq_plan_info) */
    uint32_t n_integrations;   /* LONG_SAMPLES_LENGTH = 10 (:23) */
    uint32_t n_bins;           /* Doppler bins; reference: 14000/500+1 = 29 (:248) */
    const float *doppler_hz;   /* [n_bins] offsets from f_if, ascending as the reference iterates */
    const gm_c32 *tables;      /* optional [n_bins][fft_size] caller-built DopplerShiftTable.table */
    const float *table_freq;   /* optional [n_bins] DopplerShiftTable.doppler_freq_hz (with `tables`) */
    uint32_t n_prn;            /* workers; reference: PRN_SEARCH_ACQUISITION_TOTAL = 32 (:22) */
    const uint8_t *prn_ids;    /* [n_prn] PRN of each worker (1..=32 when `codes` is NULL) */
    const int8_t *codes;       /* optional [n_prn][code_len] +-1 chips for non-GPS code families */
    uint32_t code_len;         /* chips per period of `codes` (ignored when NULL: 1023) */
    float code_rate;           /* chips/s of `codes` (ignored when NULL: 1.023e6) */
    float threshold;           /* is_good_satellite ratio, 7.0 (:237); 0 -> 7.0 */
    int32_t decision_mode;     /* GM_DECIDE_REFERENCE (0): first ascending bin whose running best passes the ratio test
                                  (the reference's early exit, :211-222).  GM_DECIDE_BEST_BIN (1): strongest bin of the
                                  whole grid, reported if IT passes the ratio test — not the reference's behaviour; for
                                  callers that hand the carrier to a PLL (a strong signal passes the test 1-2 kHz early) */
    int32_t strict_sum_order;  /* 0: the plane sum of is_good_satellite (:229-235) is a per-lane + shuffle-tree sum (within
                                  ~2e-6 of the reference's, FFT rounding aside).  1: summed in the reference's own order —
                                  eight running f32 sums over chunks_exact(8), then reduce_sum from -0.0 — and the
                                  integrations accumulated strictly in sequence (no grid-tail split); costs ~4 us per
                                  (worker, bin) workgroup.  Composite sizes (Q x a base plan) as well since ABI 6: their kernels
                                  then also store the accumulated power planes (n_prn * n_bins * fft_size * 4 bytes of device
                                  memory) and a second kernel sums each plane in that order. */
    int32_t reference_products; /* 0: `result_buf[i] *= conj(code_fft[i])` (:184-186) and `norm_sqr()` (:190-192) use two fused
                                  multiply-adds each (one rounding fewer per component; 4 instead of 6 instructions per
                                  element).  1: formed as num-complex forms them — every product and every sum rounded on its
                                  own (re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re; re*re + im*im) — so that the only
                                  arithmetic on the path that differs from the reference's is the FFT itself (rustfft's plan
                                  cannot be restated here).  ~3 % slower.  In-LDS sizes only.  (ABI 5) */
    int32_t any_length;        /* 0 (default): only the sizes above — every other fft_size is GM_ERR_UNSUPPORTED_N.
                                  1: also every fft_size with fft_size % 8 == 0 and 1024 <= fft_size <= 262144 (the reference
                                  plans any length), on the long path: L = Q x Nb, Q in [1, 32], Nb one of
                                  {16384, 16000, 10000, 8192, 8000, 4096, 2048}; L = fft_size where such a factorisation exists
                                  (GM_ACQ_FORM_LONG, e.g. 50000 = 5 x 10000, 200000 = 20 x 10000), else the smallest L >= 2 x fft_size
                                  (GM_ACQ_FORM_LONG_PADDED: the circular correlation through a zero-padded periodic extension —
                                  same correlation values, FFT rounding aside, about twice the work per sample).  Sizes the other
                                  paths serve keep them (bit-identical words).  reference_products = 1 on the long path:
                                  GM_ERR_INVALID_ARG; strict_sum_order is supported.  gm_acq_plan_info tells which path a size
                                  takes.  (ABI 8) */
    uint32_t coherent_periods; /* K: code periods integrated coherently.  0 or 1 (default): today's search — every period of the
                                  dwell is correlated and squared on its own, the n_integrations power planes are added.
                                  2 .. 32: a dwell is K x n_integrations consecutive periods, M = n_integrations groups of K.
                                  Group m is folded per Doppler bin d before the carrier mix,
                                      y[n] = sum_k rho[d][k] x[(m K + k) fft_size + n],  rho[d][k] = exp(-j 2 pi f_d k fft_size / fs),
                                  f_d = the bin's table_freq: the table's phasor continued to sample k fft_size, so the carrier
                                  phase runs on across the K periods (rho: f64 with the phase reduced to one cycle, rounded to f32;
                                  gm_acq_coherent_phasors returns them).  The fold runs in f32 with k ascending, every product and
                                  sum rounded on its own (num-complex's arithmetic).  Everything after it is today's search on y:
                                  same metric words, same decisions, same gm_acq_result meaning.  Every path, sample format, code
                                  family, strict_sum_order, decision mode and reference_products (where accepted) works.  Every
                                  entry that takes a dwell takes K x n_integrations x fft_size samples; gm_acq_finer_doppler uses
                                  (K M - 1) x fft_size of them.  > 32: GM_ERR_INVALID_ARG.
                                  Data bits and secondary (NH) codes are NOT wiped off: a sign change inside a group cancels part
                                  of it.  Space the Doppler bins at most 1 / (2 K T_code) apart.
                                  Thresholds: after the fold a noise cell's accumulated power is Gamma(M) distributed whatever K
                                  is, so the ratio test's false-alarm rate per cell is Q(M, t M) = exp(-t M) sum_{i<M} (t M)^i / i!
                                  for threshold t.  The default 7 assumes many non-coherent sums: at M = 1 it gives e^-7 per cell
                                  (several false alarms per 8000-cell plane).  Choose t from the grid's cell count instead
                                  (acquisition.detection_threshold in the Python package).  (ABI 9) */
} gm_acq_cfg;
typedef enum { GM_DECIDE_REFERENCE = 0, GM_DECIDE_BEST_BIN = 1 } gm_decision_mode;

typedef struct gm_acq gm_acq;

/* How gm_acq_create would run an fft_size (host only, no device needed, like gm_fft_supported_sizes). */
typedef enum {
    GM_ACQ_FORM_LDS = 0,          /* one in-LDS transform (gm_fft_supported_sizes): base = transform_len = fft_size, q = 1 */
    GM_ACQ_FORM_COMPOSITE = 1,    /* q x base, q in {2,3,4,5,6,8}, transform_len = fft_size */
    GM_ACQ_FORM_LONG = 2,         /* any_length: q x base, q in [1, 32], transform_len = fft_size */
    GM_ACQ_FORM_LONG_PADDED = 3   /* any_length: q x base = transform_len >= 2 x fft_size */
} gm_acq_form;
typedef struct {
    int32_t form;                 /* gm_acq_form */
    uint32_t base;                /* the base in-LDS plan length */
    uint32_t q;                   /* the factor: transform_len = q x base */
    uint32_t transform_len;
} gm_acq_plan;
/* The status gm_acq_create returns for this fft_size and any_length (GM_ERR_INVALID_ARG for 0, GM_ERR_ALIGNMENT for
 * fft_size % 8 != 0, GM_ERR_UNSUPPORTED_N for a size no path serves); on GM_OK `out` (may be NULL) describes the path.
 * gm_acq_create makes its choice through this same rule.  (ABI 8) */
int gm_acq_plan_info(uint32_t fft_size, int32_t any_length, gm_acq_plan *out);

/* = building the Doppler tables (:252-262) + AcquisitionWorker::new for every PRN (:268-271):
 * code replicas resampled, their forward FFTs computed on the GPU, plans/twiddles uploaded. */
int gm_acq_create(const gm_acq_cfg *cfg, gm_acq **out);
int gm_acq_destroy(gm_acq *a);

/* The batched equivalent of `workers.par_iter_mut()...search_satellite(...)` (:302-313, :158-226).
 *   samples  : coherent_periods*n_integrations*fft_size samples in `fmt` (coherent_periods 0 counts as 1, everywhere below)
 *   prn_mask : bit i set <-> worker i searched (the (mask >> (prn-1)) & 1 test for the default list)
 *   results[i], found[i] for every worker i (found = 0 <-> None).
 * Identical outcome to the reference loop: ascending-Doppler running best, first bin passing
 * is_good_satellite wins (early exit), argmax = first strict maximum. */
int gm_acq_search(gm_acq *a, const void *samples, size_t n_samples, int fmt, uint64_t local_tail,
                  uint64_t prn_mask, gm_acq_result *results, uint8_t *found);
int gm_acq_search_c32(gm_acq *a, const gm_c32 *samples, size_t n_samples, uint64_t local_tail,
                      uint64_t prn_mask, gm_acq_result *results, uint8_t *found);
int gm_acq_search_i8(gm_acq *a, const int8_t *iq_interleaved, size_t n_samples, uint64_t local_tail,
                     uint64_t prn_mask, gm_acq_result *results, uint8_t *found);

/* run()'s snapshot + fan-out (do_acquisition.rs:297-313) against the device ring mirror: searches the
 * coherent_periods*n_integrations*fft_size samples ending at the ring's head (device-to-device, wrap-aware); *local_tail_out =
 * head - K*M*N.  GM_ERR_OUT_OF_RANGE while head < K*M*N (the reference skips the round, :299). */
typedef struct gm_ring gm_ring;
int gm_acq_search_ring(gm_acq *a, gm_ring *ring, uint64_t prn_mask, gm_acq_result *results, uint8_t *found,
                       uint64_t *local_tail_out);

/* Fine-Doppler refinement after detection (finer_doppler, src/acquisition/acquisition_bk.rs:215-302 —
 * a legacy file outside the reference's module tree): for every found[p], the snapshot of the LAST search on this handle
 * (still in HBM) is code-stripped from results[p].code_phase_samples over (coherent_periods*num_integrations-1)*fft_size samples
 * (:240-272; the mean is taken over all K*M*N),
 * mean-removed (:236-237), zero-padded to 8*next_pow2 (:249) and transformed; the first index of the maximum |X| (:276-283)
 * gives fine_freq_hz[p] = (idx*fs)/fft_size (:251-253), i.e. IF + Doppler to fs/fft_size (7.6 Hz at 8 Msps, 10 ms).
 * Indices above fft_size/2 are reported as negative frequencies (the legacy indexes out of bounds there, :285-288, and
 * multiplies by (-1)^is_complex, :298-299: neither is reproduced).  Entries of not-found PRNs are left untouched.
 * Any output pointer may be NULL.  Synchronous.  GM_ERR_UNSUPPORTED_N if the long FFT does not factor into two in-LDS plans:
 * 8*next_pow2((K*M-1)*N) must lie in 2^16 .. 2^24, else GM_ERR_UNSUPPORTED_N (K = coherent_periods, M = num_integrations, N = fft_size).
 * A found result's code_phase_samples is a code phase: below fft_size, else GM_ERR_OUT_OF_RANGE (checked for every found result
 * before any pass runs, so a refused call fills no output).
 * gm_acq_refine_doppler (below, after the code-drift entries) is the estimator that follows the coherent, edge and drift handles. */
int gm_acq_finer_doppler(gm_acq *a, const gm_acq_result *results, const uint8_t *found, uint32_t n_prn,
                         float *fine_freq_hz, uint64_t *peak_index, float *peak_mag, uint64_t *fft_size);

/* Device-resident form: samples already in HBM (coherent_periods*n_integrations*fft_size of them); kernels are enqueued
 * on the handle's stream and the call returns without synchronising.  d_metrics (optional, may be NULL -> internal buffer) receives
 * 3*n_prn*n_bins 32-bit words: max f32 [P][D], argmax u32 [P][D], sum f32 [P][D]. */
int gm_acq_search_dev(gm_acq *a, const void *d_samples, int fmt, void *d_metrics);
/* Which workers the device-resident form searches (bit i <-> worker i); default: all. */
int gm_acq_set_prn_mask(gm_acq *a, uint64_t prn_mask);
/* ---- multi-GPU exchange (nothing distributed exists in the reference: do_acquisition.rs:302-313
 * fans the PRNs out over rayon threads of one host).  One process per GPU; PRNs are sharded in contiguous blocks of
 * n_prn per rank.  gm_comm_get_unique_id on rank 0, the 128 bytes travel out of band (file, socket, MPI, the host
 * application's own channel), gm_comm_init on every rank after gm_init(device).  RCCL (librccl.so.1) is bound at the
 * first call; GM_ERR_UNSUPPORTED if it is not installed. */
#define GM_COMM_ID_BYTES 128
typedef struct gm_comm gm_comm;
int gm_comm_get_unique_id(uint8_t id[GM_COMM_ID_BYTES]);
int gm_comm_init(int nranks, int rank, const uint8_t id[GM_COMM_ID_BYTES], gm_comm **out);
int gm_comm_destroy(gm_comm *c);
int gm_comm_info(gm_comm *c, int *nranks, int *rank);
/* The path's one exchange step, enqueued on the handle's stream (no host synchronisation): all-gather this rank's
 * metrics block d_local ([3][P][D] words as written by gm_acq_search_dev; NULL -> the handle's internal block) from
 * every rank and regroup into d_all = [3][nranks*P][D] (rank-major worker order), the layout gm_acq_decide_dev
 * takes with n_prn = nranks*P.  Every rank obtains the same block, so every rank's decision is identical. */
int gm_acq_allgather_metrics(gm_acq *a, gm_comm *c, const void *d_local, void *d_all);
/* Overlapped form: the all-gather + regroup are ordered behind everything enqueued so far on the handle's stream but run
 * on the communicator's own stream, so the next dwell's kernels need not wait for the collective; gm_comm_wait makes
 * hip_stream wait (on the device, no host synchronisation) for the last such exchange before d_all is consumed.  The
 * two buffers must not be reused before that wait. */
int gm_acq_allgather_metrics_async(gm_acq *a, gm_comm *c, const void *d_local, void *d_all);
int gm_comm_wait(gm_comm *c, void *hip_stream);
/* The same exchange for a grid that mixes transform sizes (BASELINE configs[3]: GPS + Galileo-E1 geometry + BeiDou B1I
 * codes in one family-major list; a rank's contiguous block may span two families, i.e. two gm_acq handles): all-gather
 * of `words` 32-bit words per rank, d_all = [nranks][words], enqueued on hip_stream (NULL: the default stream). */
int gm_comm_allgather_words(gm_comm *c, const void *d_local, void *d_all, size_t words, void *hip_stream);
/* Gathered padded blocks [nranks][3][p_max][n_bins] -> ONE family-major grid d_out = [3][n_rows][n_bins]:
 * d_row_map[i] = rank * p_max + row of the block that holds code i of the family-major list (device, [n_rows]).
 * Replaces the per-PRN fan-in of do_acquisition.rs:302-313 for the sharded grid; pure data movement. */
int gm_grid_assemble_dev(const void *d_gathered, uint32_t nranks, uint32_t p_max, uint32_t n_bins,
                         const uint32_t *d_row_map, uint32_t n_rows, void *d_out, void *hip_stream);
/* gm_acq_decide_dev without a handle: the reference's decision (do_acquisition.rs:195-238) for `n_prn` codes of ONE
 * family from device-resident planes (each [n_prn][n_bins]; e.g. a family's rows inside gm_grid_assemble_dev's output),
 * d_prn_ids / d_table_freq device arrays, results into caller-owned device arrays.  decision_mode: gm_decision_mode.
 * Asynchronous on hip_stream.
 * Defaults, the ones of gm_acq_cfg and gm_acq_decide_host: threshold == 0 -> 7.0; code_rate <= 0 (or not a number) -> the
 * C/A rate 1.023e6.
 * n_bins <= GM_ACQ_DECIDE_MAX_BINS: one workgroup stages a code's 3 * n_bins words (12 bytes per bin) in the 64 KB of
 * dynamic LDS it may ask for.  Above: GM_ERR_OUT_OF_RANGE, nothing launched, nothing written. */
#define GM_ACQ_DECIDE_MAX_BINS 5461u   /* 65536 / 12 */
int gm_acq_decide_planes_dev(const float *d_max, const uint32_t *d_argmax, const float *d_sum, uint32_t n_prn,
                             uint32_t n_bins, const uint8_t *d_prn_ids, const float *d_table_freq, uint32_t fft_size,
                             float fs, float code_rate, float threshold, int decision_mode, uint64_t local_tail,
                             gm_acq_result *d_results, uint8_t *d_found, void *hip_stream);

/* Replay the reference's decision (running best + ratio test + early exit) on the GPU from a metrics
 * block laid out as above for `n_prn` workers (e.g. an all-gathered one).  prn_ids: host [n_prn].
 * Asynchronous; results land in an internal device buffer read back by gm_acq_fetch_results.
 * Threshold and code rate are the handle's (gm_acq_cfg, its defaults applied at gm_acq_create: threshold 0 -> 7.0, code_rate
 * <= 0 -> the C/A rate).  A handle of more than GM_ACQ_DECIDE_MAX_BINS Doppler bins: GM_ERR_OUT_OF_RANGE, nothing launched
 * (gm_acq_search and gm_acq_search_ring, which decide through this entry, return the same). */
int gm_acq_decide_dev(gm_acq *a, const void *d_metrics, uint32_t n_prn, const uint8_t *prn_ids,
                      uint64_t local_tail);
int gm_acq_fetch_results(gm_acq *a, uint32_t n_prn, gm_acq_result *results, uint8_t *found); /* syncs */
/* The same decision replay on host-resident metrics ([n_prn][n_bins] planes), no device involved.  threshold == 0 -> 7.0;
 * code_rate <= 0 (or not a number) -> the C/A rate 1.023e6, as in gm_acq_decide_planes_dev.  A sequential scan: no limit on
 * n_bins. */
int gm_acq_decide_host(const float *max, const uint32_t *argmax, const float *sum, const float *table_freq,
                       uint32_t n_prn, uint32_t n_bins, const uint8_t *prn_ids, uint32_t fft_size, float fs,
                       float code_rate, float threshold, uint64_t local_tail, gm_acq_result *results,
                       uint8_t *found);
int gm_acq_synchronize(gm_acq *a);
/* Back-to-back dwells (a receiver that searches dwell after dwell): with `on`, a gm_acq_decide_dev on the metrics block the
 * LAST gm_acq_search_dev wrote is not launched on its own but kept, and runs inside the first kernel of the NEXT
 * gm_acq_search_dev (extra workgroups beside the forward transforms, one launch and one kernel boundary fewer per dwell), or
 * at the next gm_acq_synchronize / gm_acq_fetch_results / gm_acq_decide_dev / gm_acq_set_stream, whichever comes first.
 * Until then that metrics block must stay as the search left it; results are the same either way.  Off by default
 * (in-LDS transform sizes with n_bins <= 64 and coherent_periods <= 1 only; other handles — coherent ones included — accept the
 * call and decide at once as before). */
int gm_acq_set_deferred_decision(gm_acq *a, int on);
/* Stage F (carrier mix + forward transforms) of the NEXT dwell ahead of time: runs on a stream of the handle's own into a second
 * spectrum buffer, beside whatever the handle's stream is doing, as soon as that buffer is free (the stage C that last read it
 * has ended).  The preparation is a SNAPSHOT of d_samples — the counterpart of the reference copying its 10 ms out of the ring
 * before it searches them (do_acquisition.rs:297-301) — and is named by the generation number written to *token (never 0), NOT by
 * the address: gm_acq_search_prepared_dev(a, token, d_metrics) launches stage C on those spectra, and nothing else ever uses
 * them (d_samples: coherent_periods*n_integrations*fft_size samples).  gm_acq_search_dev always transforms the samples its own argument holds at that moment, whatever was prepared from the
 * same address before (ABI 5 matched a following search by pointer and format: a caller that refilled the buffer in between —
 * any ring-backed receiver — silently got the old samples' spectra).
 *   ready_stream: a HIP stream (or NULL).  Non-NULL: the samples are complete once the work queued on that stream SO FAR has run
 *     (an asynchronous copy, a front-end kernel): the library records an event there and stage F waits for it.  NULL: d_samples
 *     already holds the samples when the call is made (host-time contract, e.g. a published part of a device ring).
 *   Either way d_samples must stay unchanged until stage F has read it: until the search that consumes the token has been
 *     synchronised, or gm_acq_synchronize after gm_acq_drop_prepared.
 *   One preparation is outstanding at a time: a second gm_acq_prepare_dev replaces the first (its token becomes stale),
 *     gm_acq_drop_prepared forgets it; a stale / consumed / unknown token makes gm_acq_search_prepared_dev return
 *     GM_ERR_INVALID_ARG and launch nothing.  Plain searches in between leave the preparation intact.
 * Call order for dwell after dwell: search_prepared(k), prepare(k + 1), decide(k).  Pays where stage C leaves CUs idle in its last
 * round — N = 16368: 32 PRN x 29 bins are 3.6 rounds of one workgroup per CU and stage F fits into the rest; not at N = 8000, whose
 * last round is already filled.  Same metric words as the plain search.  The first call allocates the second spectrum buffer
 * (n_bins * n_integrations * fft_size * 8 bytes), the stream and three events — all of them or, on failure, none;
 * gm_acq_destroy releases them.  Composite sizes prepare nothing: they issue a token all the same and run the whole search at
 * gm_acq_search_prepared_dev from d_samples as it is THEN — behind the event recorded on `ready_stream` at prepare time (ABI 7: the
 * ordering promise holds on every size). */
int gm_acq_prepare_dev(gm_acq *a, const void *d_samples, int fmt, void *ready_stream, uint64_t *token);
int gm_acq_search_prepared_dev(gm_acq *a, uint64_t token, void *d_metrics);
int gm_acq_drop_prepared(gm_acq *a);
/* Use an existing HIP stream (e.g. torch's current stream, or the stream that fills the sample buffer) instead of the handle's
 * own: every later entry of the handle is enqueued there, i.e. BEHIND what the caller has queued on it and in front of what the
 * caller queues next — the way to order a `_dev` entry against the producer of its samples and the consumer of its metrics without
 * a synchronisation (see STREAMS at the top).  The caller keeps the stream alive until the handle is destroyed or given another. */
int gm_acq_set_stream(gm_acq *a, void *hip_stream);

/* Per-(worker, bin) planes of the last search: max, first-argmax, sum of the accumulated power
 * plane ([n_prn][n_bins] each; any pointer may be NULL).  For parity tests and the all-gather. */
int gm_acq_metrics(gm_acq *a, float *max, uint32_t *argmax, float *sum);
/* ca_code_samples_fft of worker i (AcquisitionWorker field, :126): fft_size bins. */
int gm_acq_code_fft(gm_acq *a, uint32_t worker, gm_c32 *out);
/* The table list in use: [n_bins][fft_size] and [n_bins] (either may be NULL). */
int gm_acq_tables(gm_acq *a, gm_c32 *tables, float *table_freq);
/* The coherent fold's phasor words [n_bins][coherent_periods] exactly as the device uses them (gm_acq_cfg.coherent_periods);
 * at coherent_periods 0 or 1 the one word per bin is (1, 0).  (ABI 9) */
int gm_acq_coherent_phasors(gm_acq *a, gm_c32 *out);
/* ---- Edge search on a coherent handle (coherent_periods = K >= 2): a third search axis beside PRN and Doppler — H hypotheses
 * about where the groups of K periods start, each with a secondary code's signs applied inside the group.  For GPS C/A with K = 20
 * (one data bit) the hypothesis whose groups start on the bit edge keeps the whole bit; for a signal with a secondary code (BeiDou
 * B1I's NH20, any tiered code of up to 32 periods) the aligned hypothesis wipes the code off, which is what makes K > 1 usable there.
 *   offsets   : H period offsets, 1 <= H <= 32, each in [0, 63], strictly ascending
 *   secondary : K entries of +1 / -1, or NULL (all +1)
 * A dwell is (K*M + offsets[H-1]) * fft_size samples.  Hypothesis h is the coherent search on the samples from period offsets[h]
 * on with secondary[k] * rho[d][k] in place of rho[d][k] in the fold,
 *     y_{h,d,m}[n] = sum_k secondary[k] rho[d][k] x[(offsets[h] + m K + k) fft_size + n],
 * in the fold's own arithmetic (k ascending, every product and sum rounded on its own; the multiplication by +-1 is exact).  Every
 * hypothesis yields the usual three planes: the full block is [3][P][H][D] (gm_acq_edge_metrics).  A reduction then picks, for every
 * (worker, bin) cell, the hypothesis with the largest max — on equal values the lowest h — and writes its three words into the
 * ordinary [3][P][D] metrics block and h into a choice plane [P][D] (gm_acq_edge_choice).  From there on nothing changes:
 * gm_acq_decide_dev / _host, both decision modes, the all-gather entries, gm_acq_metrics (the reduced planes) and
 * gm_acq_fetch_results see today's layout, gm_acq_result keeps its meaning (whole periods do not move the code phase;
 * sample_global_index = local_tail + code phase, relative to the dwell's first sample).  gm_acq_coherent_phasors is unchanged and does
 * not show the row.
 * While it is on: gm_acq_search*, gm_acq_search_dev, gm_acq_prepare_dev count (K*M + offsets[H-1]) * fft_size samples and
 * gm_acq_search_ring reports local_tail = head - that; gm_acq_prepare_dev behaves as on composite sizes (a token, the ordering
 * promise, the whole search at gm_acq_search_prepared_dev); gm_acq_set_deferred_decision is accepted and decides at once;
 * gm_acq_finer_doppler strips the code from the winning hypothesis's offset o* on — (K*M-1) * fft_size samples from
 * o* * fft_size + code_phase, the mean over the K*M periods from o* on.
 * Stage F runs one grid over H * D * M transforms and stage C one launch over P * H * D items (acq_stage_f_variants.h).
 * Device memory while it is on, beside the handle's own (T = gm_acq_plan_info's transform_len, N = fft_size):
 *     8 H D M T  (spectra)  +  12 P H D + 4 P D + 4 H  (metric words, choice, offsets)  +  8 offsets[H-1] N  (the internal sample
 *     buffer of the host / ring entries, when it has to grow)
 *     + 8 H D M N  on composite sizes whose base plan has no storage-order table  + 12 P H D q  on any-length sizes
 *     + 4 P H D N  with strict_sum_order on composite and any-length sizes (the stored power planes).
 * gm_acq_set_edge_search allocates it; GM_ERR_NOMEM if that fails, with the handle (and an earlier edge search) as it was.
 * GM_ERR_INVALID_ARG for K < 2, H > 32, an offset above 63, offsets that do not ascend strictly, a row entry other than +-1.  It runs
 * a pending deferred decision and drops an outstanding preparation.  n_offsets = 0 switches the search off: the handle as it was,
 * bit for bit.
 * Thresholds: the reduction takes the largest of H cells, so the false-alarm count grows with the cells searched — take
 * detection_threshold(M, n_cells * H, pfa) (acquisition.detection_threshold in the Python package) instead of (M, n_cells, pfa). */
/* host only, no device: checks the arguments as gm_acq_set_edge_search does; *dwell_periods = K*M + offsets[n_offsets-1]
 * (n_offsets = 0: K*M, coherent_periods 0 counting as 1) */
int gm_acq_edge_dwell_periods(uint32_t coherent_periods, uint32_t n_integrations, uint32_t n_offsets,
                              const uint32_t *offsets, const int8_t *secondary, uint64_t *dwell_periods);
int gm_acq_set_edge_search(gm_acq *a, uint32_t n_offsets, const uint32_t *offsets, const int8_t *secondary);
/* The planes of every hypothesis of the last search: [n_prn][H][n_bins] each, any pointer may be NULL.  Synchronises. */
int gm_acq_edge_metrics(gm_acq *a, float *max, uint32_t *argmax, float *sum);
/* The hypothesis index each (worker, bin) cell of the last search chose: [n_prn][n_bins]. */
int gm_acq_edge_choice(gm_acq *a, uint32_t *hypothesis);
/* For every found[p] the offset, in periods, of the hypothesis the winning bin (results[p].doppler_bin) of worker p chose in the
 * last search; entries of not-found workers are left untouched.  n_prn <= the handle's workers. */
int gm_acq_result_offsets(gm_acq *a, const gm_acq_result *results, const uint8_t *found, uint32_t n_prn,
                          uint32_t *offset_periods);
/* ---- Code-drift compensation: every code period of the dwell read from where it really starts.  All of the above counts period p of
 * a dwell from sample p * fft_size.  The true code period T is rarely fft_size samples: at fs = 16.3676 MHz a C/A period is 16367.6
 * samples against fft_size = 16368 (0.4 samples per period), and a Doppler of f_d shortens every period by 1 / (1 + f_d / f_carrier)
 * (3.2 chips per second at 5 kHz on L1).  Over a long dwell the code slides against the replica, the peak smears and moves.
 *   period_samples[d] : the true code period in samples as Doppler bin d sees it, f64, |T_d - fft_size| <= 8 (the nearest multiple
 *                       of 8 is within 4 of any period); n_bins must be the handle's.  n_bins = 0 or NULL: off, bit for bit.
 * Let R = K*M + offsets[H-1] be the dwell's periods (K = coherent_periods, 0 counting as 1; no edge search: R = K*M).  On the host,
 * in f64,
 *     s[d][p] = (uint64) floor(p * T_d + 0.5),   p = 0 .. R-1,
 * and period k of group m of hypothesis h in bin d is the fft_size samples from s[d][o_h + m K + k] on — the real samples at another
 * place: no circular shift, no phase ramp.  A dwell is max_d s[d][R-1] + fft_size samples (gm_acq_dwell_samples), fewer or more than
 * without the compensation, for every entry that takes one: gm_acq_search*, gm_acq_search_dev, gm_acq_prepare_dev, gm_acq_search_ring
 * (local_tail = head - that).
 * K >= 2: the fold's phasors run to where the period really starts,
 *     rho[h][d][m][k] = exp(-j 2 pi f_d (s[d][o_h+mK+k] - s[d][o_h+mK]) / fs),   f_d: the bin's table_freq,
 * formed as gm_acq_coherent_phasors' words are (f64, the phase reduced to one cycle, rounded to f32), the secondary row's sign applied
 * to them as without the compensation, and the fold's arithmetic is unchanged (k ascending, every product and sum rounded on its own).
 * K <= 1: no fold and no product — the words are those of a plain search of the gathered samples x'[m N + n] = x[s[d][m] + n].
 * With every T_d = fft_size the starts, the dwell, the phasor words and every metric word are those of the handle without it.
 * It works on every handle (every form gm_acq_plan_info reports, every sample format, code family, decision mode, strict_sum_order,
 * reference_products where the handle accepts it, the edge search on or off); gm_acq_set_edge_search and gm_acq_set_code_drift may
 * be called in either order, each plans the dwell again.  Stage C, the reduction over the hypotheses, the decision, the all-gather
 * entries and every [D][M][.] buffer stay as they are (acq_stage_f_variants.h holds the three stage-F kernels).
 * Results: s[d][0] = 0 and |s[d][o] - o T_d| <= 0.5, so code_phase_samples is the code phase at the dwell's first sample to within
 * half a sample; sample_global_index keeps its definition.  gm_acq_coherent_phasors is unchanged.
 * gm_acq_finer_doppler is unchanged and NOT compensated: it strips the code over contiguous samples (K*M periods of fft_size from
 * the winning offset on); GM_ERR_OUT_OF_RANGE where the compensated dwell ends before them.
 * While it is on gm_acq_prepare_dev behaves as on composite sizes (a token, the ordering promise, the whole search at
 * gm_acq_search_prepared_dev) and gm_acq_set_deferred_decision is accepted and decides at once.
 * Device memory while it is on, beside the handle's own and the edge search's:
 *     8 D R  (the starts)  +  8 H D M K  (the phasor words; H = 1 without an edge search)
 *     + 8 (dwell - what the internal sample buffer holds already)  when that buffer has to grow (it never holds less than the dwell
 *       without the compensation, so switching the compensation off needs no memory).
 * Everything new is allocated before anything old is released: GM_ERR_NOMEM leaves the handle (and an earlier compensation) as it
 * was, GM_ERR_INVALID_ARG (a T_d off by more than 8 or not a number, a wrong n_bins) as well.  The setter runs a pending deferred
 * decision and drops an outstanding preparation.  A handle on which it was never called, or was switched off, launches exactly the
 * kernels it launched before.  (ABI 9, additive: a caller detects the feature by the symbol) */
int gm_acq_set_code_drift(gm_acq *a, uint32_t n_bins, const double *period_samples);
/* host only, no device: checks the arguments as gm_acq_set_code_drift does (fft_size a multiple of 8); starts [n_bins][n_periods]
 * (may be NULL) and *dwell_samples = max_d starts[d][n_periods-1] + fft_size */
int gm_acq_code_drift_plan(uint32_t fft_size, uint32_t n_periods, uint32_t n_bins, const double *period_samples,
                           uint64_t *starts, uint64_t *dwell_samples);
/* Samples one dwell of this handle takes now, given coherent_periods, n_integrations, the edge search and the code drift. */
int gm_acq_dwell_samples(gm_acq *a, uint64_t *out);
/* The period starts in use: [n_bins][R].  GM_ERR_INVALID_ARG while the compensation is off. */
int gm_acq_code_drift_starts(gm_acq *a, uint64_t *out);
/* Hypothesis h's phasor words [n_bins][n_integrations][K] as they sit in device memory (h = 0 without an edge search; the secondary
 * row's signs are applied on the way into the fold and do not show here; (1, 0) throughout at K <= 1, where they are not used). */
int gm_acq_code_drift_phasors(gm_acq *a, uint32_t h, gm_c32 *out);
/* ---- Fine Doppler from per-period prompts: the search's own detection statistic on a fine frequency grid around the winning bin, built
 * from the pieces the search used — valid wherever the search is (coherent_periods 0 .. 32, the edge search and its secondary row, the
 * code-drift compensation, every form gm_acq_plan_info reports, every sample format).  For a found worker w with d =
 * results[w].doppler_bin and cp = results[w].code_phase_samples let o be the offset in periods its cell chose (gm_acq_result_offsets; 0
 * without an edge search), s[d][.] the period starts in use (p * fft_size without the compensation), tab[d] the handle's mix table,
 * c_w the handle's resampled replica, f_c = table_freq[d], N = fft_size.
 *   Prompts, i = 0 .. R_u-1:   z[i] = sum_{n<N} x[s[d][o+i] + n] * tab[d][n] * c_w[(n - cp) mod N]
 *     the circular correlation value at lag cp of period o+i alone: only samples the search read.  f32; the sample-table product is
 *     formed as in stage F; the N terms are added in a fixed order (no floating-point atomics): two calls give the same words.
 *   Groups.  K >= 2: the search's own — J = K, G = n_integrations, R_u = K*G, signs sigma_k = the edge search's secondary row (all +1
 *     without one); span_periods must be 0 or K.  K <= 1: J = span_periods (0 -> n_integrations), G = floor(n_integrations / J),
 *     R_u = G*J, sigma = +1.  An effective J < 2 (one period carries no frequency information) or G < 1: GM_ERR_INVALID_ARG.
 *   Grid.  Z = n_freq points, odd, 3 .. 4097 (0 -> 257); delta_j = (j - (Z-1)/2) * step, step = half_span / ((Z-1)/2).  half_span_hz
 *     0 -> half the distance from f_c to the farther neighbouring bin's table_freq, at most fs / (2N); a one-bin handle:
 *     fs / (2 N max(K,1)).  A given value above fs / (2N) (per-period prompts alias there), negative or not a number:
 *     GM_ERR_INVALID_ARG.
 *   Statistic.   S[j] = N^2 * sum_{g<G} | sum_{k<J} sigma_k * w_{g,k}(delta_j) * z[gJ+k] |^2,
 *                w_{g,k}(delta) = exp(-j 2 pi frac((f_c + delta) * (s[d][o+gJ+k] - s[d][o+gJ]) / fs))
 *     the cycles formed and reduced to one cycle in f64 (as the coherent and drift phasor words are), f32 sine / cosine after that.
 *     The N^2 puts S in gm_acq_metrics' units: at K >= 2 S at delta = 0 is the accumulated peak power of cell (w, d), FFT rounding
 *     aside (at K <= 1 that power is N^2 * sum_i |z[i]|^2 over the n_integrations periods).
 *   Peak.  peak_index = the first index of the maximum; delta_hz = delta_peak plus a three-point parabolic offset (host, f64);
 *     at_edge = 1 when the peak is at j = 0 or Z-1: no interpolation then, and the caller should widen the span.
 * Cost: R_u * N sample, table and replica reads per satellite (one 256-lane workgroup per (period, satellite)), no long FFT. */
typedef struct { uint32_t span_periods; uint32_t n_freq; float half_span_hz; } gm_acq_refine_cfg;   /* zeros: defaults */
typedef struct {
    double   carrier_hz;      /* table_freq[d] + delta_hz, f64: an f32 resolves 0.5 Hz at 4 MHz */
    float    delta_hz, step_hz, half_span_hz;
    float    peak_power, center_power;          /* S[peak_index], S[(Z-1)/2] */
    uint32_t peak_index, at_edge;
    uint32_t doppler_bin, offset_periods, span_periods, n_groups, n_freq;
} gm_acq_refine_out;
/* Works like gm_acq_finer_doppler: on the snapshot of the LAST search on this handle (gm_acq_search, _search_dev,
 * _search_prepared_dev, _search_ring), on the handle's stream, synchronous; entries of not-found workers are left untouched (out,
 * prompts and spectrum alike).  It runs a pending deferred decision first and changes no metric, choice or result word.
 *   out      : [n_prn]
 *   prompts  : [n_prn][R_u] or NULL;  spectrum : [n_prn][Z] or NULL  (R_u and Z: gm_acq_refine_plan)
 * GM_ERR_INVALID_ARG: a null handle (no device is touched), results, found or out; no search yet on this handle (or none since the last
 * gm_acq_set_edge_search / gm_acq_set_code_drift); n_prn above the handle's workers; a found entry's doppler_bin outside the bins or
 * code phase >= fft_size; the span / n_freq / half-span rules above.  All found flags zero: GM_OK, nothing written.
 * Device memory: one block of about n_found * (16 R_u + 4 Z + 40) bytes, built at the first call and grown when a call needs more — the new
 * block is allocated before the old one goes (GM_ERR_NOMEM leaves the handle as it was); gm_acq_destroy releases it.
 * (ABI 9, additive: a caller detects the feature by the symbol) */
int gm_acq_refine_doppler(gm_acq *a, const gm_acq_result *results, const uint8_t *found, uint32_t n_prn,
                          const gm_acq_refine_cfg *cfg /* NULL: defaults */, gm_acq_refine_out *out /* [n_prn] */,
                          gm_c32 *prompts /* [n_prn][R_u] or NULL */, float *spectrum /* [n_prn][Z] or NULL */);
/* host only, no device: the argument rules and what a call would use for `bin` (any output pointer may be NULL) */
int gm_acq_refine_plan(uint32_t coherent_periods, uint32_t n_integrations, const gm_acq_refine_cfg *cfg, float fs,
                       uint32_t fft_size, uint32_t n_bins, const float *table_freq, uint32_t bin,
                       uint32_t *span_periods, uint32_t *n_groups, uint32_t *n_freq, double *half_span_hz, double *step_hz);
/* ---- Lag window x fine Doppler at known cells: gm_acq_refine_doppler's statistic on W = 2L + 1 code phases around a predicted one, for
 * a receiver that already knows roughly where a satellite is (reacquisition after a loss of lock; probing found cells again on the next
 * dwell; a code phase finer than one sample for the hand-over) — without the P x H x D transforms of a search.
 * A candidate c names worker w, bin d, the window's centre cp and an offset o in periods: with an edge search any o <= the last offset
 * (it need not be one of the searched offsets: a predicted edge is fine), without one o = 0.  L = lag_half_window, 0 .. 64, W <= N.
 *   Lags, l = 0 .. W-1:        lambda_l = (cp + l - L) mod N
 *   Prompts, i = 0 .. R_u-1:   z[l][i] = sum_{n<N} x[s[d][o+i] + n] * tab[d][n] * c_w[(n - lambda_l) mod N]
 *     gm_acq_refine_doppler's prompts at lag lambda_l.  All W lags of a (period, candidate) come from ONE pass over the samples: every
 *     sample and table word is read once and the sample-table product is formed once, as stage F forms it.  Sums are added in a fixed
 *     order (no floating-point atomics): a candidate's words depend on the candidate, the samples and cfg alone, not on what else is
 *     in the call and not on repetition.
 *   Groups, signs, grid and statistic: gm_acq_refine_doppler's (above), unchanged and per lag,
 *     S[l][j] = N^2 * sum_{g<G} | sum_{k<J} sigma_k * w_{g,k}(delta_j) * z[l][gJ+k] |^2;  J, G, Z, half_span: gm_acq_refine_plan's rules.
 *   Peak.  (l*, j*) = the first index of the maximum of S in (l, j) order; code_phase_samples = lambda_{l*}; delta_hz and carrier_hz by
 *     gm_acq_refine_doppler's three-point parabola along j in row l*; freq_at_edge = 1 when j* is 0 or Z-1 (no interpolation then).
 *   Fine code phase (host, f64), defined when 0 < l* < W-1; otherwise lag_at_edge = 1 and code_phase_fine = code_phase_samples.  With
 *     a-, a0, a+ = sqrt(S[l*-1][j*]), sqrt(S[l*][j*]), sqrt(S[l*+1][j*]):  frac = (a+ - a-) / (2 (a0 - min(a-, a+))), the exact vertex of
 *     a symmetric triangle through three samples, clamped to +-0.5, 0 where the denominator is not positive; lambda = lambda_{l*} + frac.
 *     Without the code-drift compensation code_phase_fine = lambda mod N.  With it the period starts are known, so the rounding of the
 *     starts and the blend of two signal periods inside one read are both taken out:
 *       ebar = mean_i (s[d][o+i] - (o+i) T_d) over the R_u periods used;
 *       the lambda samples in front of the lag belong to the previous signal period, which ends N - T_d samples before the replica
 *       says it does: subtract (lambda / N)(N - T_d);
 *       code_phase_fine = (lambda + ebar - (lambda / N)(N - T_d)) mod N      (samples into the dwell, of the code's start)
 *     The estimate needs the chip edges to fall on varying sample phases: at an integer number of samples per chip with no drift the
 *     correlation is flat within a sample and the sub-sample part is unobservable (frac then only reflects noise).
 *   Floor.  floor_power = the mean of S[l][j] over all j and over the n_floor lags whose circular distance (mod N) from l* is at least
 *     ceil(fs / code_rate) + 1 samples (one chip and a sample: outside the correlation triangle); n_floor = 0 -> floor_power = 0.
 *     The library makes NO detection decision.  A caller can compare peak_power / floor_power, or peak_power against the last
 *     search's sum / N of the cell (gm_acq_metrics: the plane's mean); the W * Z values are strongly correlated along j (the grid
 *     oversamples the dwell's frequency resolution), so they are far fewer than W * Z independent trials.
 * Samples.  d_samples NULL: the snapshot of the LAST search on the handle — gm_acq_refine_doppler's rules (no search yet, or none since
 * the last gm_acq_set_edge_search / gm_acq_set_code_drift: GM_ERR_INVALID_ARG); fmt is ignored.  Non-NULL: a device pointer to
 * gm_acq_dwell_samples samples in format fmt, ready on the handle's stream — any dwell, for instance a later one; it is only read and
 * does NOT become the snapshot (a following gm_acq_refine_doppler / gm_acq_finer_doppler still sees the last search's samples).
 * Synchronous, on the handle's stream; runs a pending deferred decision first; changes no metric, choice or result word.
 *   out : [n_cands];  prompts : [n_cands][W][R_u] or NULL;  surface : [n_cands][W][Z] or NULL   (gm_acq_local_plan gives W, R_u, Z)
 * GM_ERR_INVALID_ARG, all checked before anything runs or is written: a null handle (no device is touched), cands or out; worker >=
 * the handle's workers; doppler_bin outside the bins; code_phase_samples >= fft_size; an offset outside the rule above;
 * lag_half_window > 64 or 2 * lag_half_window + 1 > fft_size; the span / n_freq / half-span rules of gm_acq_refine_plan; fmt not a
 * format (d_samples non-NULL).  n_cands = 0: GM_OK, nothing is written.
 * Device memory: one block of about n_cands * (W * (8 R_u + 4 Z + 16) + 8 R_u + 80) bytes, built at the first call and grown when a call
 * needs more — the new block is allocated before the old one goes (GM_ERR_NOMEM leaves the handle as it was); gm_acq_destroy releases it.
 * Cost: R_u * N sample and table reads and R_u * N * W multiply-adds per candidate (one 256-lane workgroup per (period, candidate)).
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct { uint32_t worker; int32_t doppler_bin; uint32_t code_phase_samples; uint32_t offset_periods; } gm_acq_cand;
typedef struct { uint32_t lag_half_window; uint32_t span_periods; uint32_t n_freq; float half_span_hz; } gm_acq_local_cfg; /* zeros: defaults */
typedef struct {                      /* 88 bytes (84 and the padding to the doubles' alignment) */
    double   carrier_hz;              /* table_freq[d] + delta_hz */
    double   code_phase_fine;         /* samples, [0, fft_size) */
    float    delta_hz, step_hz, half_span_hz;
    float    peak_power, floor_power; /* S[l*][j*]; the mean over the far lags */
    uint32_t peak_lag_index, peak_freq_index;   /* l*, j* */
    uint32_t code_phase_samples;      /* lambda_{l*} */
    uint32_t lag_at_edge, freq_at_edge, n_floor;
    uint32_t doppler_bin, offset_periods, span_periods, n_groups, n_freq, n_lags;
} gm_acq_local_out;
int gm_acq_local_search(gm_acq *a, const void *d_samples /* NULL: the last search's snapshot */, int fmt, const gm_acq_cand *cands,
                        uint32_t n_cands, const gm_acq_local_cfg *cfg /* NULL: defaults */, gm_acq_local_out *out /* [n_cands] */,
                        gm_c32 *prompts /* [n_cands][W][R_u] or NULL */, float *surface /* [n_cands][W][Z] or NULL */);
/* host only, no device: gm_acq_refine_plan's rules (the same host code) plus the lag rules; n_lags = W (any output pointer may be NULL) */
int gm_acq_local_plan(uint32_t coherent_periods, uint32_t n_integrations, const gm_acq_local_cfg *cfg, float fs, uint32_t fft_size,
                      uint32_t n_bins, const float *table_freq, uint32_t bin, uint32_t *n_lags, uint32_t *span_periods,
                      uint32_t *n_groups, uint32_t *n_freq, double *half_span_hz, double *step_hz);
/* ---- Beam rows from the array's own correlations.  A gm_beamformer handle (below) wants one constraint row [L][A] per satellite, and a real
 * receiver knows neither its array's geometry nor its cable phases.  Once a search behind the e_0 beam has found a satellite, its row can
 * be estimated from the array stream itself: correlate EVERY antenna and EVERY tap delay with the satellite's replica at the found cell
 * (gm_acq_array_prompts: one vector z_i of M = A L words per code period, in which the satellite is 30 dB up and has rank one), whiten
 * the z_i with the Gram matrix the beamformer already captures, take the principal eigenvector and un-whiten it (gm_array_row_solve).
 * Data bits cancel in z z^H; the array response, the cable phases and the code's autocorrelation across the taps are in the estimate.
 * A spatial-only estimate (A words in tap 0 of an L > 1 handle) and an estimate without the whitening both fail on the jammed scenes of
 * tests/array_probe_model.py: the prompts must be space-time and R must be the beamformer's own [M][M] matrix.
 *
 * gm_acq_array_prompts.  d_samples is ONE interleaved stream of A antennas, gm_nuller's / gm_stap's / gm_beamformer's layout: x_a[t] is
 * element t * A + a, t a TIME sample; a device pointer to gm_acq_dwell_samples(handle) time samples of A elements each, ready on the
 * handle's stream, GM_FMT_C32 or GM_FMT_I8_IQ (GM_FMT_I8_REAL is refused; int8 -128 is -128.0f), aligned to its ELEMENT size only (8
 * or 2 bytes: A = 3 int8 puts period starts on odd 2-byte boundaries).  It is only read and does not become the snapshot.
 * N = fft_size, A = n_antennas in 2 .. 8, L = taps in 1 .. 8, A L <= 32 (gm_stap's limits), R_u = max(1, coherent_periods) *
 * n_integrations.  For candidate c = (worker w, bin d, code phase cp, offset o: gm_acq_local_search's candidate and its rules, an edge
 * search allowing any o up to its last offset, else o = 0), period i < R_u, tap l < L, antenna a < A:
 *     ref[n]        = tab[d][n] * c_w[(n - cp) mod N]        the handle's mix table (gm_acq_tables) and sampled replica; c_w is +-1,
 *                                                            so both components of ref are exact
 *     z[c][i][l][a] = sum_{n<N} x_a[s[d][o+i] + n - l] * ref[n]
 *   s[d][.] are the handle's period starts in TIME samples, exactly as gm_acq_refine_doppler and gm_acq_local_search take them:
 *   (o + i) N without the code-drift compensation, gm_acq_code_drift_starts' table with it.  A time index below 0 reads as ZERO (and
 *   the word in front of the buffer is not touched): gm_stap's zero halo at the start of a stream, so with s = 0 tap l's sum misses its
 *   first l terms exactly as gm_stap's stacked samples do.  A dwell cut from the MIDDLE of a stream therefore differs from gm_stap's
 *   snapshots in the first L - 1 time samples of period 0 only; every later period reads its L - 1 predecessors from the dwell.
 *   At L = 1, z[c][i][0][a] is gm_acq_local_search's prompt (lag_half_window = 0) of antenna a's de-interleaved stream, up to the order
 *   of the sum.
 *   THE ORDER, f32.  With u = n - l the time sample relative to s, u in [-(L-1), N): lane j of 256 owns the time samples u = -(L-1) + j,
 *   -(L-1) + j + 256, ... (< N, and s + u >= 0), takes them in ascending u, and for each, l ascending and a ascending inside, adds the
 *   term of ref[u + l] (terms with u + l outside [0, N) are skipped: ref is zero there) into its own sum of (l, a), from +0, as
 *       re = fmaf(x.re, ref.re, re);  re = fmaf(-x.im, ref.im, re);  im = fmaf(x.re, ref.im, im);  im = fmaf(x.im, ref.re, im).
 *   Then S[j] = S[j] + S[j + d] for d = 32, 16, 8, 4, 2, 1 inside each group of 64 lanes, the group's sum being its S[0]; then
 *   z = ((G0 + G1) + G2) + G3 over the four groups.  No floating-point atomics: a candidate's words depend on the candidate and the
 *   samples alone, not on what else is in the call, not on the pointer's alignment and not on repetition.  Each component passes
 *   through at most 2 ceil((N + L - 1) / 256) + 9 roundings, so a word is within about (N / 128 + 12) 2^-24 sum_n |x_a[s + n - l]| of the
 *   exact sum.
 *   Synchronous, on the handle's stream, like gm_acq_local_search; runs a pending deferred decision first; changes no metric, choice,
 *   result or snapshot word.  z is a HOST array [n_cands][R_u][L][A] (gm_acq_array_plan gives R_u and R_u L A).
 *   GM_ERR_INVALID_ARG, all checked before anything runs or is written: a null handle (no device is touched), d_samples, cands or z; fmt
 *   not GM_FMT_C32 or GM_FMT_I8_IQ; A, L or A L outside the limits; n_cands > 1024; gm_acq_local_search's candidate rules (worker,
 *   doppler_bin, code_phase_samples, offset_periods).  n_cands = 0: GM_OK, nothing is written.
 *   Kernel (csrc/acq_array.hip): one 256-lane workgroup per (period, candidate); every time sample of [s - (L-1), s + N) and every table
 *   word is read once; a tile's 1024 ref words plus the L - 1 halo sit in LDS; a lane keeps its M complex sums in registers; a time
 *   sample's A words are loaded together with the widest loads (up to 16 bytes) its address allows, element by element where not.
 *   Device memory: one block of n_cands * (8 R_u L A + 16) bytes, built at the first call and grown when a call needs more — the new
 *   block is allocated before the old one goes (GM_ERR_NOMEM leaves the handle as it was); gm_acq_destroy releases it.
 *   Cost: R_u (N + L - 1) A element reads and R_u N table reads per candidate, 4 R_u N A L multiply-adds.
 *
 * gm_array_row_solve.  Host only, f64, no device.  z: n prompt vectors of m words ([n][m]; for one candidate of gm_acq_array_prompts
 * n = R_u, m = L A, as written).  R: n_blocks matrices [m][m] as gm_stap_capture / gm_beamformer_capture write them, or NULL: the
 * identity (n_blocks is ignored).  loading: 0 -> 1e-4, else in [1e-6, 1].
 *   1. Rs = the sum of the blocks in ascending order; only the UPPER triangle (p <= q) is read, the lower is its conjugate, the
 *      diagonal's imaginary part is taken as 0.
 *   2. tr = sum_p Re Rs[p][p] (p ascending);  Rl = Rs + loading * (tr / m) * I.
 *   3. Cholesky, Rl = C C^H, C lower triangular with a real positive diagonal.
 *   4. zt_i = C^-1 z_i;  Q = sum_i zt_i zt_i^H (i ascending).
 *   5. lambda1 >= lambda2: the two largest eigenvalues of Q, v the unit eigenvector of lambda1 (cyclic Hermitian Jacobi until the
 *      off-diagonal energy is below 1e-30 of the whole; lambda2 is reported as 0 where it comes out negative).
 *   6. s = C v.
 *   7. s is rotated so that its word of largest modulus, at ref_index (the lowest index on ties), is real and positive.
 *   8. s is scaled so that s^H s = m.
 *   9. Each word is rounded once to f32: row[0 .. m).
 *   v is defined up to a phase, which step 7 fixes; the row is as well defined as lambda1 is separated from lambda2.
 *   info: lambda1, lambda2, ref_index.  THE LIBRARY DECIDES NOTHING: a caller reads lambda1 / lambda2 as the quality of the estimate
 *   (the satellite's rank-one term over the largest whitened residual).
 *   GM_ERR_INVALID_ARG with row and info untouched: m outside 2 .. 32; n = 0; a NULL z, row or info; R non-NULL with n_blocks = 0; a z
 *   or R word read that is not finite; loading outside its range or not a number; tr <= 0 or not finite; a Cholesky pivot that is not
 *   positive and finite; lambda1 not greater than 0.
 *
 * The sequence: gm_beamformer with the row e_0 and gm_beamformer_capture; gm_acq_search_dev on plane 0; gm_acq_array_prompts at the
 * found cells on the beamformer's own input; gm_array_row_solve per cell with the captured R; gm_beamformer_set_steering, or a new
 * handle with the rows.
 * Not built: per-antenna prompts from the tracker (the array form of gm_trk_bank); a loop that re-steers by itself; ring writers; any
 * detection or quality decision; wiring into receiver_harness.cpp or bench.py.
 * (Since then the first item has been built: gm_trk_array_prompts, "Per-antenna prompts at tracked states" below.)
 * (And the second, as far as a library that decides nothing can build it: "Re-steering on the device" below, the three entries
 * gm_trk_array_prompts_dev, gm_array_rows_solve_dev and gm_beamformer_set_steering_dev that put one update on a stream with no host wait.)
 * (ABI 9, additive: a caller detects the feature by the symbol) */
/* 24 bytes.  reserved: gm_array_row_solve writes 0; gm_array_rows_solve_dev writes the row's STATUS there (0: solved; 1 .. 6: see
 * "Re-steering on the device") */
typedef struct { double lambda1, lambda2; uint32_t ref_index; uint32_t reserved; } gm_array_row_info;
int gm_acq_array_prompts(gm_acq *a, const void *d_samples, int fmt, uint32_t n_antennas, uint32_t taps, const gm_acq_cand *cands,
                         uint32_t n_cands, gm_c32 *z /* [n_cands][R_u][L][A], host */);
/* host only, no device: the limits on A, L and A L, coherent_periods <= 32 and n_integrations >= 1 (and R_u L A below 2^32);
 * *periods = R_u, *words_per_cand = R_u L A (either may be NULL) */
int gm_acq_array_plan(uint32_t coherent_periods, uint32_t n_integrations, uint32_t n_antennas, uint32_t taps, uint32_t *periods,
                      uint32_t *words_per_cand);
int gm_array_row_solve(uint32_t m, uint32_t n, const gm_c32 *z /* [n][m] */, const gm_c32 *R /* [n_blocks][m][m] or NULL */,
                       size_t n_blocks, float loading /* 0 -> 1e-4; else [1e-6, 1] */, gm_c32 *row /* [m] */, gm_array_row_info *info);
/* ---- Re-steering on the device.  A receiver that follows its satellites across the sky, or past a moving jammer, refreshes its beam
 * rows every few code periods.  With the entries above that is three host waits an update: gm_trk_array_prompts delivers to the host,
 * gm_array_row_solve is host f64 one row a call, gm_beamformer_set_steering drains the handle once per beam.  The three entries here
 * enqueue and return; with gm_beamformer_process_dev on the same stream the whole update sits behind the block it belongs to:
 *     states from gm_trk_collect (no synchronisation) -> gm_trk_array_prompts_dev into slot e of a history of prompts
 *     every few epochs: gm_array_rows_solve_dev (history, the captured R) -> gm_beamformer_set_steering_dev -> the next process_dev
 * THE LIBRARY DECIDES NOTHING but what the caller's min_ratio says: when to re-steer and how much history are the caller's.
 *
 * gm_trk_array_prompts_dev ("Per-antenna prompts at tracked states" below states the words): gm_trk_array_prompts' two kernels, rules,
 * order of refusals and skipped records, the result in DEVICE buffers, asynchronously on `stream` (NULL: the handle's own).  d_z
 * [n_states][L][A] c32 and d_done [n_states] u8 are word for word what the synchronous entry returns for the same arguments.
 *   states is a HOST array, read before the call returns; NULL is GM_ERR_INVALID_ARG (the handle's own channels live on the device
 *   and reading them needs a wait: take the states from gm_trk_collect).  A NULL d_z or d_done, and a d_z lying over the sample
 *   buffer, are refused likewise; a refused call enqueues nothing.
 *   The handle's per-call device block is shared with the synchronous entry, and calls of the two entries on one handle take effect in
 *   the order issued: a call that goes to a stream other than the last array call's first waits ON THE HOST for that call (the
 *   streaming stages' rule); growing the block waits for what is in flight before the old block goes.  A caller that keeps one stream
 *   and one shape never waits.  The records travel through pinned host blocks of the handle's (one allocation at the first call; at most 16 calls
 *   ahead of the stream: the 17th waits for the oldest copy).
 *
 * gm_array_rows_solve_dev: steps 1 to 9 of gm_array_row_solve above for n_rows rows in one launch, f64, on `stream` (NULL: the null
 * stream; there is no handle).  Vector i of row p is the m words at d_z + p * row_stride + i * vec_stride (c32 words): the defaults
 * (0, 0 -> n m and m) are gm_acq_array_prompts' [n_cands][R_u][m]; a history [n][P][m] of gm_trk_array_prompts_dev calls, one per
 * epoch, is row_stride = m, vec_stride = P m.  A skipped record's zeros add nothing to Q.  d_R: n_blocks captured matrices shared by
 * all rows, or NULL with n_blocks = 0: the identity.  Only the upper triangles are read; the blocks are summed in ascending order, so
 * Rs, C and Q are gm_array_row_solve's bit for bit.  The eigenproblem is a PARALLEL-ORDER cyclic Jacobi: the m indices (and an idle
 * one where m is odd) are paired by a round-robin tournament, player m' - 1 fixed, step r of m' - 1 pairing (r, m' - 1) and
 * ((r + k) mod (m' - 1), (r - k) mod (m' - 1)); the pairs of a step are disjoint, each pair's rotation is formed by
 * gm_array_row_solve's formulas from the current Q, the column rotations of Q and V are applied, then the row rotations of Q.  The
 * stopping rule is the host's (off-diagonal energy below 1e-30 of the whole, at most 64 sweeps).  This is a different but fixed
 * rotation order: lambda1, lambda2 and the row equal the host entry's up to f64 rounding, not bit for bit.
 *   STATUS.  What gm_array_row_solve refuses after looking at the data is here a per-row status in d_info[p].reserved, the first that
 *   applies: 1 a z word of the row is not finite; 2 a word of R that is read is not finite; 3 tr is not positive and finite; 4 a
 *   Cholesky pivot is not positive and finite; 5 lambda1 is not greater than 0; 6 the row came out zero or not finite.  Such a row
 *   gets all-zero words, lambda1 = lambda2 = 0 and ref_index = 0; the other rows of the call are not affected, bit for bit.
 *   A row's words depend on that row's vectors, R and the cfg alone: not on n_rows, not on the row's place in the call, not on
 *   repetition.  No floating-point atomics.
 *   gm_array_solve_plan (host only, no device) states every argument rule: m in 2 .. 32, n in 1 .. 4096, n_rows in 1 .. 1024,
 *   n_blocks at most 2^20, the strides both 0 or both at least m (and at most 2^40), loading 0 or in [1e-6, 1], reserved 0; and the
 *   extents in c32 words: *z_words = (n_rows - 1) row_stride + (n - 1) vec_stride + m read at d_z, *R_words = n_blocks m m read at
 *   d_R, *row_words = n_rows m written at d_rows (n_rows gm_array_row_info at d_info).  Any of the three may be NULL.
 *   gm_array_rows_solve_dev checks through the same function, then: a NULL d_z, d_rows or d_info; d_R NULL exactly where n_blocks
 *   is 0.  GM_ERR_INVALID_ARG, before anything is launched, nothing touched.
 *   Kernel (csrc/array_solve.hip): one 256-lane workgroup a row, no word between workgroups, no spin wait, every loop bounded by a
 *   checked argument or the 64 sweeps; Rs / C, Q and V stay in LDS in f64 (50688 bytes).  With 16 or fewer rows most of the device
 *   idles on purpose: a latency path beside the streaming kernels.
 *
 * gm_beamformer_set_steering_dev (the beamformer's section below states what a steering row is): a small kernel on `stream` (NULL:
 * the handle's own) copies row p of d_rows [n_rows][M] into the steering words of beam first_beam + p where every word of the row is
 * finite, the row is not all zero (gm_beamformer_set_steering's rules) and, with d_info, the row's status is 0 and lambda1 >=
 * min_ratio * lambda2 (min_ratio: the caller's policy; 0: no gate).  Otherwise the beam keeps its row.  d_installed[p] (or NULL) is
 * 1 or 0 accordingly.  Ordered like a process_dev call: it applies to every block finished by a call issued later, blocks of earlier
 * calls keep the old words; no host wait but the streaming stages' when `stream` differs from the last call's.
 * gm_beamformer_capture's w words show the effect.  GM_ERR_INVALID_ARG, nothing enqueued: a NULL handle or d_rows; n_rows = 0;
 * first_beam + n_rows > n_beams; min_ratio negative or not finite.
 * (ABI 9, additive: a caller detects the feature by the symbols) */
typedef struct {
    uint32_t m, n, n_rows, n_blocks;   /* m = L A in 2..32; n vectors a row, 1..4096; n_rows 1..1024; n_blocks 0 (R = identity) .. 2^20 */
    uint64_t row_stride, vec_stride;   /* c32 words between rows / between a row's vectors in d_z; 0, 0 -> n m and m ([n_rows][n][m]) */
    float    loading;                  /* gm_array_row_solve's: 0 -> 1e-4, else [1e-6, 1] */
    uint32_t reserved[5];              /* 0 */
} gm_array_solve_cfg;                  /* 56 bytes */
int gm_array_solve_plan(const gm_array_solve_cfg *cfg, uint64_t *z_words, uint64_t *R_words, uint64_t *row_words);
int gm_array_rows_solve_dev(const gm_array_solve_cfg *cfg, const void *d_z, const void *d_R /* [n_blocks][m][m] c32 or NULL */,
                            void *d_rows /* [n_rows][m] c32 */, void *d_info /* [n_rows] gm_array_row_info */, void *stream);
/* ---- Subtracting found satellites from a dwell.  C/A codes isolate about 24 dB: a strong satellite's cross-correlation peaks stand
 * above a satellite 24 dB weaker in every other PRN's plane.  gm_acq_cancel writes the dwell with the named satellites' signals
 * subtracted, as c32, into a second device buffer, which every search entry takes as a dwell.  The expected sequence is: search,
 * gm_acq_local_search on the found cells, gm_acq_cancel, search again on the output.  The library makes NO detection decision.
 * D = gm_acq_dwell_samples of the handle, N = fft_size, L = code_len, c_w = worker w's raw chips (cfg.codes, or the C/A row of
 * prn_ids[w]).  A candidate names worker w, f = carrier_hz (IF + Doppler: gm_acq_local_out.carrier_hz), cp = code_phase (samples into
 * the dwell, of the code's start, in [0, N): gm_acq_local_out.code_phase_fine) and T = period_samples, the signal's TRUE code period
 * (0: N; else within 8 of N).  The replica must be built from the fine values and the true period: an integer code phase leaves about
 * 11 dB of cancellation, T = N on a signal 0.4 sample a period off about 1 dB.
 *   Segments (host, f64): q0 = -ceil(cp / T);  o_k = cp + double(q0 + k) * T;  b_k = clamp(ceil(o_k), 0, D);  segment k is the samples
 *     b_k <= n < b_{k+1}, k = 0 .. Q-1, with Q the least count with o_Q >= D and b_Q = D;  n_k = b_{k+1} - b_k.  A segment is one code
 *     period of the SIGNAL; the first and the last are partial, and the last may be empty (then a_k = 0).  gm_acq_cancel_plan returns
 *     Q and b_0 .. b_Q.
 *   Replica at sample n of segment k.  Host constants in f64: cpl = L / T, fq = f / fs.  Device, per sample, in f64:
 *     e = double(n) - o_k;  idx = min(L - 1, (uint32) floor(e * cpl));  cyc = double(n) * fq;
 *     then turn = float(2.0 * (cyc - floor(cyc))),  (c, s) = (cospif(turn), sinpif(turn)),  r[n] = c_w[idx] * (c + j s)
 *     — the cycles reduced to one in f64, then the f32 sine / cosine, as gm_acq_refine_doppler forms its phasors.
 *   Amplitudes, one per segment, ALL taken from the input:  a_k = (sum_{n in segment k} x[n] * conj(r[n])) / n_k, an f32 sum in a
 *     fixed order (no floating-point atomics: two calls give the same words).  One complex amplitude per code period is a projection:
 *     data bits, a secondary code and slow phase drift need no model.  Taking every amplitude from the input is PARALLEL cancellation:
 *     the cross terms between cancelled satellites (about -24 dB) are left in; a caller may run the entry again on its output.
 *   Output.  GM_FMT_C32 and GM_FMT_I8_IQ: y[n] = x[n] - sum_c a_{c,k_c(n)} r_c[n], the candidates subtracted in ascending index;
 *     GM_FMT_I8_REAL: the term is 2 Re(a r) and the imaginary part of y is exactly 0 (a real dwell holds half the signal's power:
 *     the amplitudes are 3 dB noisier).  Every product and sum is rounded on its own.  n_cands = 0: y is x converted to c32, GM_OK.
 *   out[c] (host, f64, from the amplitude words): n_segments = Q, first_samples = n_0, last_samples = n_{Q-1}, removed_energy =
 *     sum_k n_k |a_k|^2, amp_rms = sqrt(removed_energy / D), worker echoed.  amps[c][k] = a_k for k < Q (the rest is not written).
 * Samples.  d_samples NULL: the snapshot of the LAST search on the handle, under gm_acq_local_search's rules (no search yet, or none
 * since the last gm_acq_set_edge_search / gm_acq_set_code_drift: GM_ERR_INVALID_ARG); fmt is ignored.  Non-NULL: any dwell of D samples
 * in format fmt, ready on the handle's stream; it is only read and does NOT become the snapshot.  d_out: D c32 samples of device
 * memory, aligned to 8 bytes (16 for 16-byte stores).  d_out == the c32 input itself is allowed and runs in place (every lane reads
 * its x[n] and writes its y[n] itself, after the amplitude kernel has ended); if that buffer is the snapshot, later
 * gm_acq_refine_doppler / gm_acq_local_search / gm_acq_finer_doppler calls see the CANCELLED samples.  Any other overlap of the two
 * ranges is GM_ERR_INVALID_ARG.
 * Synchronous, on the handle's stream; runs a pending deferred decision first; changes no metric, choice or result word.
 * GM_ERR_INVALID_ARG, all checked before anything runs or is written: a null handle (no device is touched), a null cands with
 * n_cands > 0, a null or misaligned d_out; n_cands > 64; worker >= the handle's workers (the same worker twice is allowed: multipath);
 * reserved != 0; cp outside [0, N) or not a number; T not 0 and (|T - N| > 8 or not a number); f not a number or |f| >= fs; fmt not
 * a format (d_samples non-NULL); the snapshot rules; the overlap rule; amps_stride below the largest Q (amps non-NULL).
 * gm_acq_cancel_plan also refuses fft_size < 16, dwell_samples = 0, above 2^40 or above 2^24 code periods, and bounds_cap < Q + 1
 * while bounds is non-NULL.
 * Device memory: one block of about n_cands * (Q + 1) * 24 bytes (o, b and a) plus 48 bytes a candidate, built at the first call and
 * grown when a call needs more — the new block is allocated before the old one goes (GM_ERR_NOMEM leaves the handle as it was) — and
 * the raw chips [P][L] as bytes, uploaded once; gm_acq_destroy releases both.
 * Cost: n_cands + 1 reads of the dwell and one c32 write; per sample and candidate a chip index and a turn in f64 and one sine / cosine.
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct { uint32_t worker, reserved; double carrier_hz, code_phase, period_samples; } gm_acq_cancel_cand;   /* 32 bytes */
typedef struct { double removed_energy; float amp_rms; uint32_t n_segments, first_samples, last_samples, worker, reserved; } gm_acq_cancel_out; /* 32 bytes */
int gm_acq_cancel(gm_acq *a, const void *d_samples /* NULL: the last search's snapshot */, int fmt,
                  const gm_acq_cancel_cand *cands, uint32_t n_cands, void *d_out /* device, c32 [dwell] */,
                  gm_acq_cancel_out *out /* [n_cands] or NULL */, gm_c32 *amps /* [n_cands][amps_stride] or NULL */, uint32_t amps_stride);
/* host only, no device: the segment rule above for one candidate on a dwell of dwell_samples samples (n_segments may be NULL) */
int gm_acq_cancel_plan(uint64_t dwell_samples, uint32_t fft_size, double code_phase, double period_samples,
                       uint32_t *n_segments, uint64_t *bounds /* [bounds_cap] or NULL */, uint32_t bounds_cap);
/* Kernel timing of the last gm_acq_search*_dev call, measured with HIP events on the handle's
 * stream: ms_mix_fft (stage F), ms_corr (stage C, the dominant kernel), ms_decide.  Enable first: on = 1 times every
 * search, on = k > 1 every k-th (an event record costs about 2 us of stream time; four per timed search), 0 disables. */
int gm_acq_enable_timing(gm_acq *a, int on);
int gm_acq_last_timing(gm_acq *a, float *ms_mix_fft, float *ms_corr, float *ms_decide);
/* Averages over every gm_acq_search_dev call since timing was enabled (the last 512 at most). */
int gm_acq_timing_summary(gm_acq *a, uint32_t *launches, float *avg_ms_mix_fft, float *avg_ms_corr);

/* Diagnostic (not in the reference): out == NULL arms, then out = [n_integrations][8][8] int64 shader-clock stamps
 * of workgroup 0's waves at the phase boundaries of each transform of the last search.  The stamped kernels are compiled into a
 * DIAGNOSTIC build of the library only (-DGM_DIAG_STAMPS): the product library returns GM_ERR_UNSUPPORTED and launches nothing. */
int gm_acq_debug_stamps(gm_acq *a, long long *out);

/* Diagnostic (not in the reference; an additive export, the ABI number stays): how the handle's LAST stage-C launch dealt its
 * workgroups onto (worker, Doppler bin, integration) items: the very numbers the launcher computed and passed to the kernel, recorded at
 * the launch and not computed again here.  path GM_CORR_PATH_NONE (all fields 0): no search with a selected worker has run yet.
 * In-LDS paths: blocks b and b + 8 share an XCD; XCD x takes `share` slots of the item list by `map_mode` (0 equal contiguous shares,
 * 1 whole bins, 2 whole bins and evenly split leftovers, >= 16 the diagnostic tiled walk (cb << 4) | rows_max); the slots from
 * `split_from` on are cut into `split_k` parts of one integration each (`split_items` of them per XCD); grid = 8 * (split_from +
 * split_items * split_k) workgroups.  cut: GM_CORR_CUT_*; why: for GM_CORR_CUT_NONE the first rule that forbade the cut.
 * Composite paths: 8 * slots workgroups walk equal shares in blocks of cb workers x rows_max bins (cb 0: in list order).
 * Long path: the (worker, bin) list in long_slabs slabs of long_slab items.  Fields of the other paths are 0. */
#define GM_CORR_PATH_NONE 0
#define GM_CORR_PATH_LDS 1            /* acq_corr_kernel */
#define GM_CORR_PATH_LDS_WS31 2       /* acq_corr_ws31_kernel */
#define GM_CORR_PATH_COMP 3           /* comp_corr_kernel */
#define GM_CORR_PATH_COMP_WS 4        /* comp_corr_ws_kernel */
#define GM_CORR_PATH_LONG 5           /* launch_long_corr */
#define GM_CORR_CUT_NONE 0
#define GM_CORR_CUT_ALL 1             /* the grid fits the resident slots: every item is cut */
#define GM_CORR_CUT_TAIL 2            /* several rounds: the last items of every XCD */
#define GM_CORR_WHY_CUT 0             /* (the grid is cut) */
#define GM_CORR_WHY_M1 1              /* one integration */
#define GM_CORR_WHY_STRICT 2          /* strict_sum_order */
#define GM_CORR_WHY_OFF 3             /* no scratch on this handle or plan, or a diagnostic switch */
#define GM_CORR_WHY_SHARE 4           /* one round of more items per XCD than there are tickets */
#define GM_CORR_WHY_MAX_K 5           /* more than 16 integrations */
#define GM_CORR_WHY_SCRATCH 6         /* every item would be cut and the handle's scratch does not hold their planes */
#define GM_CORR_WHY_ONE_WG_ROUNDS 7   /* a plan of one workgroup per CU on a grid of several rounds */
#define GM_CORR_WHY_CLAMPED 8         /* the scratch holds not even one item's planes per XCD */
typedef struct gm_acq_corr_grid_info {
    int32_t path;                                            /* GM_CORR_PATH_* */
    int32_t n_workers, n_bins, n_int;                        /* of the launch: the masked worker list, H * D bins in an edge search */
    int32_t wg_per_cu, split_planes;                         /* in-LDS: what the decision started from */
    int32_t map_mode, share, slots, split_from, split_k, split_items, grid, cut, why;
    int32_t cb, rows_max;                                    /* composite (slots, grid: as above) */
    uint32_t long_slab, long_slabs;
} gm_acq_corr_grid_info;
int gm_acq_debug_corr_grid(gm_acq *a, gm_acq_corr_grid_info *out);

/* AcquisitionManager (do_acquisition.rs:39-74): mode 0 ColdStart / 1 WarmStart / 2 SteadyState. */
int gm_acq_manager_mode_for(size_t tracked_count);
int gm_acq_manager_pacing_and_list(int mode, uint32_t active_prn_mask, uint64_t *interval_ms, uint32_t *mask);

/* ------------------------------------------------------------------ MulticastRingBuffer device mirror
 * (src/utilities/multicast_ring_buffer.rs:36-130): power-of-two ring of Complex32 addressed by the
 * absolute sample index `head`; the mirror keeps the same bytes in HBM for the tracking kernels. */
int gm_ring_create(size_t buf_size, gm_ring **out);                      /* ::new :46-61 */
int gm_ring_destroy(gm_ring *r);
int gm_ring_write_samples(gm_ring *r, const gm_c32 *samples, size_t n);  /* :66-101 */
int gm_ring_get_head(gm_ring *r, uint64_t *head);                        /* :103-105 */
int gm_ring_copy_to_slice(gm_ring *r, uint64_t start, gm_c32 *dest, size_t n); /* :107-129 */
/* write_samples that does not block the producer on the H2D copy: pinned staging + the ring's own copy stream; `head`
 * advances only after the samples have landed in HBM.  gm_ring_flush waits for all of it.  The head is published by PULL
 * (ABI 6): gm_ring_get_head, gm_ring_wait_head and every stage entry that snapshots the ring first retire the blocks whose copies
 * (and front-end kernels) have completed; nothing runs on the copy stream but copies and kernels (a host callback there — round 4 —
 * held the stream, i.e. the next block, until the runtime's callback thread woke up: milliseconds, now and then). */
int gm_ring_write_samples_async(gm_ring *r, const gm_c32 *samples, size_t n);
int gm_ring_flush(gm_ring *r);
/* What the asynchronous writer has ENQUEUED so far (>= gm_ring_get_head, which counts what has landed): the head that
 * gm_trk_update_all_async's passes are gated on, i.e. what a stage driver that never waits for the copies plans its pass count
 * from.  Equal to the head for a ring that is written synchronously.  ABI 7. */
int gm_ring_get_enqueued_head(gm_ring *r, uint64_t *head);
/* The notifier/Condvar of the reference ring (:42-43, :94-98) as used by do_tracking::run (do_tracking.rs:392-406):
 * sleep until head >= required_idx (wrapping signed comparison) or timeout_ms elapsed; *reached = 1 / 0. */
int gm_ring_wait_head(gm_ring *r, uint64_t required_idx, uint32_t timeout_ms, int *reached);

/* ------------------------------------------------------------------ Digital front-end
 * rf::frontend::DigitalFrontend (src/rf/frontend.rs:6-62): DC removal (DcRemoverSimd, src/rf/dc_remove.rs:10-29:
 * eight one-pole IIR lanes per component, alpha = 0.001) + LUT NCO down-mix (NcoLut, src/rf/nco_lut.rs:17-42: 2048
 * entries, f32 phase accumulator `% 2048`) + mix_simd (:8-15), bit-exact with the reference's f32 evaluation order.
 * Only whole chunks of 8 samples are processed (chunks_exact_mut(16), :35); a tail passes through unprocessed.
 * fs_out is stored only, as in the reference (frontend.rs keeps output_sample_rate as a dead field): the front-end returns fs_in
 * samples, and the rate is converted by a gm_resampler, declared below. */
typedef struct gm_frontend gm_frontend;
int gm_frontend_create(float f_if, float fs_in, float fs_out, gm_frontend **out);     /* ::new :19-30 */
int gm_frontend_destroy(gm_frontend *f);
/* NcoLut tables and phase_step (nco_lut.rs:25-34); any pointer may be NULL */
int gm_frontend_lut(gm_frontend *f, float lut_re[2048], float lut_im[2048], float *phase_step);
int gm_frontend_get_state(gm_frontend *f, float *phase_accumulator, float bias_re[8], float bias_im[8]);
int gm_frontend_set_state(gm_frontend *f, float phase_accumulator, const float bias_re[8], const float bias_im[8]);
/* process_block(&mut [f32]) :33-62 — host buffer of interleaved I/Q, in place (H2D + kernel + D2H, synchronous) */
int gm_frontend_process_block(gm_frontend *f, float *raw_floats, size_t n_floats);
/* device-resident form: d_in (GM_FMT_C32 or GM_FMT_I8_IQ) -> d_out (c32; may alias d_in for c32), asynchronous on
 * `stream` (a hipStream_t, NULL -> the handle's own stream; gm_frontend_synchronize waits for that one) */
int gm_frontend_process_dev(gm_frontend *f, const void *d_in, int fmt, void *d_out, size_t n_samples, void *stream);
/* n_streams independent streams (antennas, bands) in one launch, one workgroup each: fes[i] processes d_in[i] -> d_out[i]
 * (n_samples each); every front-end keeps its own state and NCO step; a handle may appear once per call.
 * The launch goes out on `stream` (NULL -> fes[0]'s own) and is not waited for; the call itself WAITS ON THE HOST for what is
 * queued on `stream` in front of it, once, while the streams' descriptors travel to the device. */
int gm_frontend_process_dev_batch(gm_frontend *const *fes, uint32_t n_streams, const void *const *d_in, int fmt,
                                  void *const *d_out, size_t n_samples, void *stream);
int gm_frontend_synchronize(gm_frontend *f);
/* rf_thread's block step (src/rf/rf_thread.rs:43-48: process_block, then shared_ring_buffer.write_samples) fused and
 * non-blocking: host samples (c32, or int8 IQ: 2 B/sample over PCIe, converted on the GPU) -> pinned staging -> front-end
 * kernel writing straight into the ring mirror; head advances when the block is in HBM (gm_ring_flush to wait).  Blocks of up
 * to 2^19 samples per copy + launch; the kernels run on a stream of the ring's own behind the copies (an event per staging slot). */
int gm_frontend_write_ring(gm_frontend *f, gm_ring *ring, const void *samples, size_t n_samples, int fmt);
/* Long blocks (>= 48 pipeline segments of 3840 samples, output not aliasing the input) run in the SPECULATIVE form since round 6: the
 * block is cut into up to 32 runs on as many workgroups, each starting from a GUESSED DC-remover state (the recurrence in exact arithmetic over the
 * 16 384 steps before its warm-up) that an 8 640-step warm-up lets fall onto the true f32 chain; a second kernel verifies run by run
 * that the state a run entered with is bit for bit the state its predecessor left, and does a run again — sequentially, from the right
 * state — where it is not.  The results are those of the sequential front-end, word for word, whatever the guesses were
 * (tests/test_gpu_frontend.py::test_speculative_blocks_are_exact spoils every one of them); 0.52 -> 0.15 ms per 2^19-sample block.
 * Diagnostic (not in the reference): *runs = how many runs the verification has had to repeat on this handle so far. */
int gm_frontend_debug_repairs(gm_frontend *f, uint32_t *runs);
/* Diagnostic (not in the reference; host counters, no device traffic): kernel launches on behalf of this handle since create, by the
 * form that ran: counts[0] the sequential kernel (no phase table, a phase set off the tabulated orbit, or a batch with such a member),
 * counts[1] the table form, counts[2] the speculative form.  A batch counts the launched form once for every member.
 * (tests/test_gpu_frontend_forms.py asserts with it that each form ran where it was meant to.) */
int gm_frontend_debug_forms(gm_frontend *f, uint32_t counts[3]);

/* ------------------------------------------------------------------ Rate conversion and pulse blanking
 * The two stages the reference's front-end names and leaves out (rf/frontend.rs: process_block ends with the comments
 * `// Pulse blanking, e.g., based on amplitude threshold)` and `// Resampling`).  A gm_resampler converts a stream of c32 or int8-IQ
 * samples at rate fs_in into c32 samples at fs_out = fs_in * up / down with a polyphase windowed-sinc filter, and can zero input
 * samples whose power exceeds a threshold first.  Every output is defined by ABSOLUTE sample indices alone: the words do not depend
 * on how the stream is cut into calls.
 *   Table (host, f64, each word rounded once to f32), layout [PHI + 1][T].  rho = min(1, up / down), fc = cutoff * rho,
 *     h(t) = fc * sinc(fc t) * I0(beta * sqrt(1 - (2t/T)^2)) / I0(beta)  for |t| <= T/2, else 0;   sinc(x) = sin(pi x) / (pi x)
 *     g[phi][j] = h(j - (T/2 - 1) - phi / PHI),  then every row divided by its own f64 sum: the DC gain is 1 at every phase.
 *   Output m = 0, 1, ...: position and phase from 64-bit integers only,
 *     pos = m * down,  i0 = pos div up,  r = pos mod up,  q = r * PHI,  phi = q div up,  alpha = float(double(q mod up) / double(up))
 *     c_j = fmaf(alpha, g[phi+1][j] - g[phi][j], g[phi][j])           (the difference rounded to f32 first)
 *     y[m] = sum_{j<T} c_j * xb[i0 - (T/2 - 1) + j]                   f32, one fmaf per component and tap, from +0, j ASCENDING
 *     xb = the input after blanking, zero before the stream's first sample.  The order of the T terms is a function of j alone, never
 *     of where the output falls in a tile, a workgroup or a call.  m = a * up + m' and the input count are decomposed so that no
 *     product exceeds 2^63: a stream stays correct past 2^32 samples (86 s at 50 Msps).
 *   Blanking (blank_threshold > 0): an input sample with re*re + im*im > thr*thr is replaced by (0, 0); f32, each product and the sum
 *     rounded on its own, strictly greater.  int8 samples are converted to f32 first (-128 is -128.0f).
 *   Timing.  Output m is the signal at input time m * down / up: the filter is centred and adds no timestamp delay.  Only availability
 *     lags: after A inputs in total, total_out(A) = max(0, ceil((A - T/2) * up / down)) outputs exist, and a call delivers
 *     total_out(A_after) - total_out(A_before).  The host computes the count with no synchronisation.
 *   State.  The handle keeps the last T blanked inputs in device memory, in two buffers used alternately (a call reads one while it
 *     writes the other), and the counters on the host; the blanked count is an integer in device memory.
 *   Kernel (csrc/resample_kernels.hip): one 256-lane workgroup per tile of outputs; the tile's inputs are converted and blanked once
 *     into LDS.  With n = floor((4096 - T - 1) * up / down) + 1, the most outputs whose inputs span at most 4096 LDS samples, a tile
 *     is 1024, 512 or 256 outputs (the largest of them not above n; a lane owns 4, 2 or 1), or n itself below 256.
 * Zeros in the config mean defaults.  (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t up, down;        /* fs_out = fs_in * up / down; reduced by their gcd inside; each 1 .. 2^24; 1/16 <= up/down <= 16 */
    uint32_t taps;            /* T, a multiple of 8 in 8 .. 256; 0 -> min(256, 32 * ceil(max(1, down/up))) */
    uint32_t n_phases;        /* PHI, a power of two 16 .. 1024; 0 -> 256 */
    float    cutoff;          /* (0, 1], of the narrower Nyquist band; 0 -> 0.9 */
    float    kaiser_beta;     /* [0, 20]; 0 -> 8.0 */
    float    blank_threshold; /* 0: off; > 0: an input sample with re^2 + im^2 > thr^2 (f32, each product and the sum rounded on its own) is replaced by (0, 0) */
    uint32_t reserved;        /* must be 0 */
} gm_resampler_cfg;
typedef struct gm_resampler gm_resampler;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG: a null cfg, up or down 0 or above 2^24, a ratio outside [1/16, 16],
 * taps not 0 and not a multiple of 8 in 8 .. 256, n_phases not 0 and not a power of two in 16 .. 1024, cutoff outside [0, 1], kaiser_beta
 * outside [0, 20], a negative blank_threshold, any of the three not a number, reserved != 0, inputs_so_far + n_in above 2^62) and, for
 * a stream that has taken inputs_so_far samples, the count n_in more deliver.  Any output pointer may be NULL. */
int gm_resampler_plan(const gm_resampler_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *up_reduced,
                      uint32_t *down_reduced, uint32_t *taps, uint32_t *n_phases, uint64_t *n_out);
/* host only, no device: the (PHI + 1) * T table words */
int gm_resampler_design(const gm_resampler_cfg *cfg, float *table);
int gm_resampler_create(const gm_resampler_cfg *cfg, gm_resampler **out);
int gm_resampler_destroy(gm_resampler *r);
/* Zeroes the history and the three counters; the stream continues as if input_index zero samples had gone before: the next input has
 * absolute index input_index, the next output absolute index total_out(input_index).  Synchronous.  input_index above 2^62:
 * GM_ERR_INVALID_ARG. */
int gm_resampler_reset(gm_resampler *r, uint64_t input_index);
/* the (PHI + 1) * T words the device uses (gm_resampler_design's) */
int gm_resampler_taps(gm_resampler *r, float *table);
/* inputs taken, outputs delivered and inputs blanked since gm_resampler_create or the last gm_resampler_reset (any pointer may be
 * NULL).  Each input is counted once.  Synchronises the handle's stream and the stream the last call ran on. */
int gm_resampler_stats(gm_resampler *r, uint64_t *inputs, uint64_t *outputs, uint64_t *blanked);
/* d_in (GM_FMT_C32 or GM_FMT_I8_IQ; GM_FMT_I8_REAL: GM_ERR_INVALID_ARG), n_in samples -> d_out (c32), *n_out of them (n_out may be
 * NULL).  Asynchronous on `stream` (a hipStream_t; NULL: the handle's own non-blocking stream); consecutive calls of a handle must be
 * ordered against each other (one stream, or the caller's events).  Every argument is checked before anything runs: out_cap below the
 * count is GM_ERR_OUT_OF_RANGE, d_out overlapping d_in GM_ERR_INVALID_ARG, each with nothing launched and the state unchanged.
 * n_in = 0: GM_OK, *n_out = 0. */
int gm_resampler_process_dev(gm_resampler *r, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_cap, size_t *n_out,
                             void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream) */
int gm_resampler_process(gm_resampler *r, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out);
int gm_resampler_synchronize(gm_resampler *r);
/* gm_frontend_write_ring with the rate conversion as one more step per block: the front-end kernel writes a linear device buffer owned
 * by the resampler, the resampler kernel writes its outputs into the ring at the writer's position (wrapping with the ring's mask), the
 * position advances by that block's output count and the block is published as gm_frontend_write_ring publishes it.  A block that
 * yields no output leaves the head where it was.  Ring indices then count OUTPUT samples: ring index m is input time m * down / up,
 * and gm_acq_result.sample_global_index of a search on this ring lives on that axis, at rate fs_out.  *n_out_total (may be NULL) =
 * the outputs this call enqueued.  GM_ERR_OUT_OF_RANGE when they exceed the ring; the resampler must not be in use elsewhere
 * meanwhile and should have been created at its absolute index 0 when the ring was empty.  gm_ring_flush waits for all of it. */
int gm_frontend_write_ring_resampled(gm_frontend *f, gm_resampler *r, gm_ring *ring, const void *samples, size_t n_samples, int fmt,
                                     uint64_t *n_out_total);

/* ------------------------------------------------------------------ Narrowband interference excision
 * Pulse blanking removes what is short in time and wide in frequency; a gm_excisor removes the reverse: a CW or narrowband carrier,
 * long in time and narrow in frequency, which no amplitude threshold catches.  c32 or int8-IQ samples in, c32 samples out at the same
 * rate and the same sample index (no timestamp delay).  It is a windowed overlap-add filter bank with a per-bin gain: 50 % overlap,
 * sine (square-root Hann) analysis and synthesis windows, perfect reconstruction when every gain is 1.  Everything is by ABSOLUTE
 * sample indices.
 *   Block length B in {256, 512, 1024, 2048, 4096}, half block H = B / 2.
 *   Windows (host, f64, each word rounded once to f32): analysis wa[i] = sin(pi i / B), synthesis ws[i] = sin(pi i / B) / B (the
 *     inverse transform's normalisation folded in): wa[i] ws[i] B + wa[i + H] ws[i + H] B = 1.
 *   Blanking (blank_threshold > 0), the resampler's rule word for word: an input sample with re*re + im*im > thr*thr is replaced by
 *     (0, 0); f32, each product and the sum rounded on its own, strictly greater; int8 samples are converted to f32 first.  It is
 *     applied to the input before anything else (a pulse smears over every bin of its block); blanked inputs are counted once each,
 *     with integer adds.
 *   Blocks.  Block b = 0, 1, ... covers absolute inputs [(b - 1) H, (b + 1) H); xb = the input after blanking, zero before the stream's
 *     first sample.  X_b = forward FFT of wa[i] * xb[(b - 1) H + i], unnormalised; Y_b[k] = g[k] * X_b[k], the f32 gain times each
 *     component; u_b = inverse FFT of Y_b, unnormalised.
 *   Output.  For n in segment s = n div H, i = n mod H:  y[n] = ws[i + H] * u_s[i + H] + ws[i] * u_{s+1}[i], each product rounded
 *     first, then the sum.  A block's words depend on its B inputs and the gains alone: y does not depend on how the stream is cut
 *     into calls, tiles or workgroups.
 *   Availability.  After A inputs in total, total_out(A) = H * max(0, A div H - 1) outputs exist, and a call delivers
 *     total_out(A_after) - total_out(A_before); the host computes the count with no synchronisation.  Output n is the filtered signal
 *     at input time n.  There is no flush entry: a caller that needs the tail appends B zeros.
 *   State.  The handle keeps the not yet retired blanked inputs (fewer than 3H) in device memory, in two buffers used alternately (a
 *     call reads one while it writes the other), and the counters on the host; the blanked count is an integer in device memory.
 *   Gains g[B], f32 in [0, 1], all ones at creation: gm_excisor_set_gains installs static notches or a taper; gm_excisor_adapt_dev
 *     sets them on the device from a Welch periodogram of the samples it is given (cut from index 0 of that buffer, independent of the
 *     stream state, blanked by the same rule), all enqueued with no host wait:
 *     1. Block j covers [j H, j H + B), J = (n - B) div H + 1 blocks; P[k] = sum_j |FFT(wa * block_j)[k]|^2, each |.|^2 as
 *        re*re + im*im with every operation rounded.  Fixed order: C = max(4, ceil(J / 512)) blocks a chunk; a chunk's partial sum
 *        adds its blocks with j ascending from +0, P adds the chunks' sums with the chunk index ascending from +0.  No
 *        floating-point atomics: two calls on the same input give the same words.
 *     2. med = the element of rank (B - 1) div 2 of P in ascending order.
 *     3. flag[k] = P[k] > factor * med (one f32 product, strictly greater); g[k] = 0 where any flag within guard_bins of k is set,
 *        the distance taken circularly, g[k] = 1 elsewhere.
 *     The library decides nothing else: no cap on the share of zeroed bins, no smoothing over time; the caller adapts when it wants
 *     to (J >= 32 blocks advised: with few blocks noise alone crosses factor 4).
 *   Kernel (csrc/excise_kernels.hip): one workgroup per tile of G consecutive segments runs blocks s0 .. s0 + G in turn on the in-LDS
 *     transforms of fft_core.h, the inverse on the plan with the forward plan's radices reversed so that the spectrum and the gain
 *     multiply stay in registers, and keeps a block's weighted second half on chip until the next block's first half exists.  G is
 *     not in the words.
 *   Block-adapt mode (gm_excisor_set_block_adapt): handle state, off at creation.  The static gains remove a carrier that stays in
 *     place; a sweeper, a hopper or a drifting harmonic needs a decision per block.  When the mode is on, for every block b (the blocks
 *     above, by absolute index), on chip between the two transforms, with no second pass over the samples and no host wait:
 *     1. Spectrum.  X_b as above (blanked, windowed, forward FFT, unnormalised); p[k] = re*re + im*im, f32, each product and the sum
 *        rounded on its own, as the periodogram forms it.
 *     2. Median.  med_b = the element of rank (B - 1) div 2 of p in ascending order, with the low 16 bits of its f32 word cleared.
 *        Non-negative floats order as their bit patterns, so med_b is the largest word v with 16 zero low bits and
 *        count(p < v) <= rank.  The truncation is part of the definition (it lowers the level by at most 2^-7 relative) and lets the
 *        selection run in 15 bit rounds where the full search takes 32.
 *     3. Flags and gain.  flag[k] = p[k] > factor * med_b (one f32 product, strictly greater); m_b[k] = 0 where any flag lies within
 *        guard_bins of k, circularly, 1 elsewhere; Y_b[k] = (g[k] * m_b[k]) * X_b[k]: the static gains stay in force and are
 *        multiplied in first, so a caller can keep a fixed notch.  With m_b all ones the words are those of the mode off.
 *     4. Output.  The inverse transform and the overlap-add exactly as above.
 *     5. m_b depends on the block's B inputs alone: as before, no word depends on how the stream is cut into calls, tiles or
 *        workgroups, and a block that two tiles or two calls both compute gets the same mask both times.
 *     6. Counters, integers in device memory, integer adds only: blocks, blocks_flagged (blocks with at least one flag), bins_flagged,
 *        bins_zeroed.  Block b is counted exactly once, when segment b - 1 is delivered; block 0 is never counted.  gm_excisor_reset
 *        zeroes them.
 *     7. With the mode off every word, counter and launch of the handle is as if the mode did not exist.
 *     A noise-only bin of one block is exponentially distributed: P(p > f * median) = 2^-f, so the default factor is 16 (1.6 % of
 *     noise-only blocks of B = 1024 carry a flag), not the periodogram's 4.  No cap on the share of zeroed bins and no smoothing
 *     between blocks: the library reports, the caller decides.
 * Zeros in the config mean defaults.  (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t block;            /* B: 256, 512, 1024, 2048 or 4096; 0 -> 1024 */
    uint32_t guard_bins;       /* 0 .. 16: bins zeroed on either side of a flagged one */
    float    threshold_factor; /* > 1; 0 -> 4.0: a bin is flagged when P[k] > factor * median */
    float    blank_threshold;  /* 0: off; > 0: an input sample with re^2 + im^2 > thr^2 is replaced by (0, 0) before anything else */
    uint32_t reserved[4];      /* must be 0 */
} gm_excisor_cfg;
typedef struct gm_excisor gm_excisor;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG: a null cfg, a block not in the list, guard_bins above 16, a
 * threshold_factor not 0 and <= 1 or not a number, a negative blank_threshold or not a number, reserved != 0, inputs_so_far + n_in above
 * 2^62), the resolved defaults and, for a stream that has taken inputs_so_far samples, the count n_in more deliver.  Any output
 * pointer may be NULL. */
int gm_excisor_plan(const gm_excisor_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *block, uint32_t *guard_bins,
                    float *threshold_factor, uint64_t *n_out);
/* host only, no device: the B analysis and the B synthesis window words (either pointer may be NULL, not both) */
int gm_excisor_windows(const gm_excisor_cfg *cfg, float *analysis, float *synthesis);
int gm_excisor_create(const gm_excisor_cfg *cfg, gm_excisor **out);
int gm_excisor_destroy(gm_excisor *x);
/* Zeroes the kept inputs and the three counters; the stream continues as if input_index zero samples had gone before.  The gains are
 * kept.  Synchronous.  input_index above 2^62: GM_ERR_INVALID_ARG. */
int gm_excisor_reset(gm_excisor *x, uint64_t input_index);
/* B host f32 values, each in [0, 1] (outside, or not a number: GM_ERR_INVALID_ARG, nothing changed).  Ordered on the handle's stream:
 * calls enqueued before it use the old gains, calls after it the new ones. */
int gm_excisor_set_gains(gm_excisor *x, const float *gains);
/* reads the B gains back (what gm_excisor_set_gains or gm_excisor_adapt_dev installed last).  Synchronises. */
int gm_excisor_gains(gm_excisor *x, float *gains);
/* the adaptive step on n samples at d_in (GM_FMT_C32 or GM_FMT_I8_IQ; n < B, n above 2^31, a null pointer or GM_FMT_I8_REAL:
 * GM_ERR_INVALID_ARG with nothing enqueued).  Asynchronous on `stream` (NULL: the handle's own); no host wait.  The stream state and
 * the counters are not touched.  It writes the gains: order it against the handle's other calls as they are ordered against each other
 * (one stream, or the caller's events); a gm_excisor_process_dev enqueued behind it on the same stream uses the new gains. */
int gm_excisor_adapt_dev(gm_excisor *x, const void *d_in, int fmt, size_t n, void *stream);
/* the last adapt's words: P[B], the median, the bins flagged and the bins zeroed (all 0 before the first adapt).  Synchronises.  Any
 * pointer may be NULL. */
int gm_excisor_psd(gm_excisor *x, float *P, float *median, uint32_t *n_flagged, uint32_t *n_zeroed);
/* d_in (GM_FMT_C32 or GM_FMT_I8_IQ; GM_FMT_I8_REAL: GM_ERR_INVALID_ARG), n_in samples -> d_out (c32), *n_out of them (n_out may be
 * NULL).  Asynchronous on `stream` (a hipStream_t; NULL: the handle's own non-blocking stream); consecutive calls of a handle must be
 * ordered against each other (one stream, or the caller's events).  Every argument is checked before anything runs: out_cap below the
 * count is GM_ERR_OUT_OF_RANGE, d_out overlapping d_in GM_ERR_INVALID_ARG, each with nothing launched and the state unchanged.
 * n_in = 0: GM_OK, *n_out = 0. */
int gm_excisor_process_dev(gm_excisor *x, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_cap, size_t *n_out,
                           void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream) */
int gm_excisor_process(gm_excisor *x, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out);
int gm_excisor_synchronize(gm_excisor *x);
/* inputs taken, outputs delivered and inputs blanked since gm_excisor_create or the last gm_excisor_reset (any pointer may be NULL).
 * Each input is counted once.  Synchronises the handle's stream and the stream the last call ran on. */
int gm_excisor_stats(gm_excisor *x, uint64_t *inputs, uint64_t *outputs, uint64_t *blanked);
/* Block-adapt mode (the definition above).  Zeros mean defaults. */
typedef struct {
    float    threshold_factor; /* > 1; 0 -> 16.0: a bin of a block is flagged when p[k] > factor * med_b */
    uint32_t guard_bins;       /* 0 .. 16: bins zeroed on either side of a flagged one */
    uint32_t reserved[6];      /* must be 0 */
} gm_excisor_block_cfg;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG: a null cfg, a threshold_factor not 0 and <= 1 or not a number,
 * guard_bins above 16, reserved != 0) and the resolved defaults.  Either output pointer may be NULL. */
int gm_excisor_block_plan(const gm_excisor_block_cfg *cfg, float *threshold_factor, uint32_t *guard_bins);
/* switches the mode on with cfg's settings (again: new settings), or off with cfg == NULL (which also disarms a capture).  Ordered
 * like gm_excisor_set_gains: calls enqueued before it run as they were enqueued, calls after it in the new mode.  A bad cfg is
 * GM_ERR_INVALID_ARG and changes nothing.  The counters are kept. */
int gm_excisor_set_block_adapt(gm_excisor *x, const gm_excisor_block_cfg *cfg);
/* the four counters since gm_excisor_create or the last gm_excisor_reset.  Synchronises.  Any pointer may be NULL. */
int gm_excisor_block_stats(gm_excisor *x, uint64_t *blocks, uint64_t *blocks_flagged, uint64_t *bins_flagged, uint64_t *bins_zeroed);
/* arms a capture into the caller's device buffers (both NULL: disarms it): every later gm_excisor_process_dev that delivers
 * n_seg >= 1 segments writes, for its blocks j = 0 .. n_seg in call order (block j of the call is the first block of segment j),
 * p as f32 d_power[j][B] and m as one byte a bin d_mask[j][B] (1: kept, 0: zeroed); either pointer alone may be NULL.  A call with
 * cap_blocks < n_seg + 1 is GM_ERR_OUT_OF_RANGE before anything runs.  Blocks that two tiles compute write the same words.  The
 * buffers must stay valid until the capture is disarmed and the handle synchronised.  The other entries (gm_excisor_process, the ring
 * paths) do not capture.  It needs the mode on: GM_ERR_INVALID_ARG otherwise.  What a test, or a caller's spectrum monitor, reads. */
int gm_excisor_block_capture(gm_excisor *x, float *d_power, uint8_t *d_mask, size_t cap_blocks);
/* gm_frontend_write_ring_resampled's block loop with the excisor between the front-end kernel and the resampler.  r may be NULL: the
 * excisor's outputs then go into the ring at the writer's position, wrapping, and ring indices count its outputs: ring index n is
 * input time n.  With r, ring indices count the resampler's outputs as in gm_frontend_write_ring_resampled.  The same publishing and
 * the same GM_ERR_OUT_OF_RANGE rule (the outputs of the call exceed the ring).  It does no adapt of its own.  *n_out_total (may be
 * NULL) = the outputs this call enqueued.  It calls the excisor through the handle: with the block-adapt mode on
 * (gm_excisor_set_block_adapt) every block gets its own mask and the counters run, with no other entry. */
int gm_frontend_write_ring_conditioned(gm_frontend *f, gm_excisor *x, gm_resampler *r, gm_ring *ring, const void *samples,
                                       size_t n_samples, int fmt, uint64_t *n_out_total);

/* ------------------------------------------------------------------ Real-IF down-conversion
 * The first block of a receiver for IF-sampled data: a gm_ddc takes GM_FMT_I8_REAL samples (one byte each) at fs_in, whose carrier
 * sits at an intermediate frequency, and delivers c32 samples at complex baseband at fs_out = fs_in * up / down: blank, multiply by
 * a complex NCO, then the rate converter's centred polyphase low-pass.  A real stream at fs carries fs / 2 of bandwidth: 16.3676 Msps
 * real at an IF of 4.1304 MHz becomes, with 20460 / 40919, 8.184 Msps complex with a C/A period of exactly 8184 samples.  It is the
 * stage to put in front of a gm_excisor, a gm_resampler or the ring when the capture is real: those take c32 or int8 IQ only.
 * Everything is defined by ABSOLUTE input indices: the words do not depend on how the stream is cut into calls, tiles or workgroups,
 * and stay right past 2^32 samples.
 *   Table: gm_resampler_design's words for the same up, down, taps, n_phases, cutoff and kaiser_beta (the same rules and defaults).
 *   NCO, in integers.  frac = mix - floor(mix) in f64 (mix = mix_cycles_per_sample = f_mix / fs_in, any finite value);
 *     inc = (uint64_t) floor(ldexp(frac, 64)), exact (a tiny negative mix whose frac rounds to 1 gives the wrapped value, inc = 0).
 *     Input n (absolute index) has phase Theta_n = (n * inc) mod 2^64, a wrapping 64-bit product, and k = Theta_n >> 40 (24 bits).  The
 *     truncation of the phase to 24 bits is part of the definition, not an error term.
 *     Two host-built tables of 4096 complex f32 words, each word the f64 value rounded once:
 *       Whi[h] = exp(-j 2 pi h / 4096),  Wlo[l] = exp(-j 2 pi l / 2^24)
 *     w[n] = Whi[k >> 12] * Wlo[k & 4095], formed in f32 with no fused operation, every product and sum rounded on its own:
 *       re = fl(fl(ar br) - fl(ai bi)),  im = fl(fl(ar bi) + fl(ai br))        (within 2^-22 of exp(-j 2 pi k / 2^24) for every k)
 *   Blanking (blank_threshold > 0): an input with x*x > thr*thr (f32, the int8 value converted first, strictly greater) is replaced by
 *     0 and counted once, with integer adds.
 *   Product: p[n] = (fl(xb[n] * re), fl(xb[n] * im)).  The filter rows have DC gain 1 and nothing is rescaled: a real carrier of
 *     amplitude A at f_mix + delta comes out as a complex tone of amplitude A / 2 at delta; its image at -(2 f_mix + delta) and the
 *     stream's DC, which lands at -f_mix, are what the low-pass removes.
 *   Output m: the rate converter's formula with p in xb's place — the same pos, i0, phi, alpha, the same
 *     c_j = fmaf(alpha, g[phi+1][j] - g[phi][j], g[phi][j]), and y[m] = sum_{j<T} c_j * p[i0 - (T/2 - 1) + j], one fmaf per component
 *     and tap, from +0, j ASCENDING; p is zero before the stream's first sample.  The same total_out(A) and per-call count, computed
 *     on the host with no synchronisation; output m is the baseband signal at input time m * down / up.
 *   State.  The handle keeps the last T blanked input BYTES in device memory, in two buffers used alternately, and the counters on the
 *     host.  The phase needs no state: it is a function of the absolute index.
 *   Kernel (csrc/ddc_kernels.hip): one 256-lane workgroup per tile of outputs, the rate converter's tiles; the tile's input span is read
 *     as bytes (16-byte loads where the address allows, single bytes at the head and the tail: the input may start at ANY byte address),
 *     blanked and multiplied by its phasor once, and kept in LDS as float pairs for the rate converter's tap loop.
 * Zeros in the filter fields mean defaults.  (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    double   mix_cycles_per_sample; /* f_mix / fs_in: the frequency brought to 0, in cycles per input sample; any finite value */
    uint32_t up, down;        /* as gm_resampler_cfg, field by field */
    uint32_t taps;
    uint32_t n_phases;
    float    cutoff;
    float    kaiser_beta;
    float    blank_threshold; /* 0: off; > 0: an input sample with x^2 > thr^2 (f32) is replaced by 0 */
    uint32_t reserved;        /* must be 0 */
} gm_ddc_cfg;
typedef struct gm_ddc gm_ddc;
/* host only, no device: gm_resampler_plan's argument rules for the fields they share, and GM_ERR_INVALID_ARG for a
 * mix_cycles_per_sample that is not finite; the reduced ratio, the defaults, *phase_inc = inc and, for a stream that has taken
 * inputs_so_far samples, the count n_in more deliver (gm_resampler_plan's for the same fields).  Any output pointer may be NULL. */
int gm_ddc_plan(const gm_ddc_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *up_reduced, uint32_t *down_reduced,
                uint32_t *taps, uint32_t *n_phases, uint64_t *phase_inc, uint64_t *n_out);
int gm_ddc_create(const gm_ddc_cfg *cfg, gm_ddc **out);
int gm_ddc_destroy(gm_ddc *d);
/* Zeroes the history and the three counters; the next input has absolute index input_index (its phase is input_index * inc), the next
 * output absolute index total_out(input_index).  Synchronous.  input_index above 2^62: GM_ERR_INVALID_ARG. */
int gm_ddc_reset(gm_ddc *d, uint64_t input_index);
/* inputs taken, outputs delivered and inputs blanked since gm_ddc_create or the last gm_ddc_reset (any pointer may be NULL).  Each
 * input is counted once.  Synchronises the handle's stream and the stream the last call ran on. */
int gm_ddc_stats(gm_ddc *d, uint64_t *inputs, uint64_t *outputs, uint64_t *blanked);
int gm_ddc_synchronize(gm_ddc *d);
/* the words the device uses: the (PHI + 1) * T filter words, and the 4096 words of Whi and of Wlo.  Any pointer may be NULL; the two
 * phasor tables are the same for every handle, so d may be NULL too when table is (host only, no device then). */
int gm_ddc_tables(gm_ddc *d, float *table, gm_c32 *whi, gm_c32 *wlo);
/* d_in (n_in bytes of GM_FMT_I8_REAL, starting at ANY byte address) -> d_out (c32), *n_out of them (n_out may be NULL).  Asynchronous
 * on `stream` (a hipStream_t; NULL: the handle's own non-blocking stream); consecutive calls of a handle must be ordered against each
 * other (one stream, or the caller's events).  Every argument is checked before anything runs: out_cap below the count is
 * GM_ERR_OUT_OF_RANGE, d_out overlapping d_in GM_ERR_INVALID_ARG, each with nothing launched and the state unchanged.  n_in = 0:
 * GM_OK, *n_out = 0. */
int gm_ddc_process_dev(gm_ddc *d, const void *d_in, size_t n_in, void *d_out, size_t out_cap, size_t *n_out, void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream) */
int gm_ddc_process(gm_ddc *d, const int8_t *in, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out);
/* gm_frontend_write_ring_conditioned's block loop with the down-converter in the front-end kernel's place, for host int8 real
 * samples, one byte each.  No gm_frontend takes part: the DC of a real stream lands at -f_mix and the low-pass removes it.  x and r may
 * each be NULL: down-converter, then the excisor if there is one, then the resampler if there is one; the last stage writes into the
 * ring at the writer's position, wrapping with the ring's mask, and ring indices count ITS outputs.  A block is the ring's staging
 * slot, as in the sibling entries (where up > down it is at most floor((2^19 - 1) * down / up) samples, so that a block's outputs fit
 * the linear buffers between the stages).  The same publishing and the same GM_ERR_OUT_OF_RANGE rule (the outputs of the call exceed
 * the ring: nothing is enqueued, no state moves).  *n_out_total (may be NULL) = the outputs this call enqueued.  The excisor is called
 * through its handle: its block-adapt mode (gm_excisor_set_block_adapt), when on, applies here too. */
int gm_ddc_write_ring(gm_ddc *d, gm_excisor *x, gm_resampler *r, gm_ring *ring, const int8_t *samples, size_t n_samples,
                      uint64_t *n_out_total);

/* ------------------------------------------------------------------ Polyphase filter bank: sub-bands of one stream
 * A gm_channelizer cuts a c32 or int8-IQ stream at fs into M sub-bands, each delivered as its own c32 stream at fs / D: one prototype
 * low-pass of L = M P taps and one M-point transform per output time, in place of M mixers and M filters.  It is what an FDMA
 * constellation needs (GLONASS L1OF: fourteen carriers 562.5 kHz apart in one capture, one code: gm_glonass_code) and what a wide
 * capture holding several signals needs before a search at a small fft_size.  Everything is defined by ABSOLUTE input indices: the
 * words do not depend on how the stream is cut into calls, tiles or workgroups, and stay right past 2^32 samples.
 *   Prototype filter, built on the host in f64, every word rounded once to f32:
 *     fc = cutoff / D;  h(t) = fc sinc(fc t) I0(beta sqrt(1 - (2t/L)^2)) / I0(beta) for |t| <= L/2, else 0;
 *     g[j] = h(j - (L/2 - 1)) for j = 0 .. L-1, divided by the f64 sum: DC gain 1.
 *   Channel k is centred at k fs / M; k >= M/2 means (k - M) fs / M.  Output m = 0, 1, ... of channel k:
 *     n0 = m D - (L/2 - 1)                                  (64-bit integers)
 *     u[r]  = sum_{p<P} g[r + pM] * xb[n0 + r + pM]         f32, one fmaf per component and tap from +0, p ASCENDING;  r = 0 .. M-1
 *     y_k[m] = sum_{r<M} u[r] * exp(-j 2 pi k (n0 + r) / M) = the M-point forward DFT of u, rotated by n0 mod M
 *     xb is the input after blanking (the resampler's rule: blank_threshold > 0 and re*re + im*im > thr*thr in f32, strictly greater,
 *     replaces the sample by 0 and counts it once), and zero before the stream's first sample; an int8 sample is converted to f32
 *     first (-128 is -128.0f).  The phase depends on (n0 + r) mod M only: exact at any absolute index, no NCO table.  The device forms
 *     the DFT with f32 butterflies and multiplies bin k by the f32 word of exp(-j 2 pi ((k n0) mod M) / M), each product and sum rounded
 *     on its own: within (P + 4 log2 M + 8) 2^-24 sum_j |g_j| |xb[n0 + j]| of the exact value.
 *   Timing.  The filter is centred: output m is the signal at input time m D, with no timestamp delay.  After A inputs
 *     total_out(A) = max(0, ceil((A - L/2) / D)) outputs exist per channel (gm_resampler's formula at 1/D); a call delivers the
 *     difference, computed on the host with no synchronisation.
 *   State.  The handle keeps the last L blanked inputs in device memory, in two buffers used alternately, and the counters on the host.
 *   Kernel (csrc/channelizer_kernels.hip): one 256-lane workgroup per tile of output times; the tile's input span, (tile - 1) D + L <=
 *     4096 samples (tile = min((4096 - L) / D + 1, 1024), rounded down to 512 or 256 above those), is read, converted and blanked once
 *     into a padded LDS image; a lane owns an output time, keeps the M branch sums in registers, transforms them there and stores the
 *     listed bins, so consecutive lanes store consecutive words of a plane.
 * Zeros in the filter fields mean defaults.  Not built: synthesis (the inverse bank).  (The C planes go into a plane ring: "Plane ring" and "Tracking on planes" below.)
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t n_channels;      /* M: 4, 8, 16, 32 or 64 */
    uint32_t decim;           /* D: 1 .. M; need not divide M */
    uint32_t taps_per_branch; /* P: 2 .. 32, L = M P taps in all; 0 -> 16 */
    float    cutoff;          /* (0, 1]: the pass band edge as a fraction of the output Nyquist frequency fs / (2 D); 0 -> 0.9 */
    float    kaiser_beta;     /* [0, 20]; 0 -> 8 */
    float    blank_threshold; /* 0: off; > 0: an input sample with re^2 + im^2 > thr^2 (f32) is replaced by 0, before the filter */
    uint32_t n_out_channels;  /* C <= M; 0 (with out_channels NULL): all M channels in order */
    uint32_t reserved;        /* must be 0 */
    const uint32_t *out_channels; /* [C] distinct indices 0 .. M-1 in any order: plane i of the output is channel out_channels[i].  Only
                                 the listed planes are computed to the end and stored.  Read during the call that takes the cfg only. */
} gm_channelizer_cfg;
typedef struct gm_channelizer gm_channelizer;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG for a value outside its range, a non-finite float, reserved != 0, a
 * channel index listed twice or outside 0 .. M-1, a list without a count or a count without a list, inputs_so_far + n_in above 2^62);
 * *n_out_channels = C, *taps_per_branch = P, *n_taps = L and, for a stream that has taken inputs_so_far samples, the count of outputs
 * per channel that n_in more deliver.  Any output pointer may be NULL. */
int gm_channelizer_plan(const gm_channelizer_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *n_out_channels,
                        uint32_t *taps_per_branch, uint32_t *n_taps, uint64_t *n_out);
/* host only, no device: the L words g[j] */
int gm_channelizer_design(const gm_channelizer_cfg *cfg, float *taps);
int gm_channelizer_create(const gm_channelizer_cfg *cfg, gm_channelizer **out);
int gm_channelizer_destroy(gm_channelizer *c);
/* Zeroes the history and the three counters; the next input has absolute index input_index, as if that many zeros had gone before, and
 * the next output absolute index total_out(input_index).  Synchronous.  input_index above 2^62: GM_ERR_INVALID_ARG. */
int gm_channelizer_reset(gm_channelizer *c, uint64_t input_index);
/* the L words the device uses (gm_channelizer_design's) */
int gm_channelizer_taps(gm_channelizer *c, float *taps);
/* inputs taken, outputs delivered PER CHANNEL and inputs blanked since gm_channelizer_create or the last gm_channelizer_reset (any
 * pointer may be NULL).  Each input is counted once.  Synchronises the handle's stream and the stream the last call ran on. */
int gm_channelizer_stats(gm_channelizer *c, uint64_t *inputs, uint64_t *outputs, uint64_t *blanked);
/* d_in (n_in samples of GM_FMT_C32 or GM_FMT_I8_IQ; GM_FMT_I8_REAL is refused: a real stream takes a gm_ddc in front) -> d_out, c32
 * [C][out_stride]: plane i holds this call's *n_out outputs of channel out_channels[i] as one contiguous stream, so a plane pointer
 * goes straight into gm_acq_search_dev; words of a plane behind *n_out are not touched (n_out may be NULL).  Asynchronous on `stream`
 * (a hipStream_t; NULL: the handle's own non-blocking stream); consecutive calls of a handle must be ordered against each other (one
 * stream, or the caller's events).  Every argument is checked before anything runs: out_cap below the count or out_stride below
 * out_cap is GM_ERR_OUT_OF_RANGE, the C * out_stride words at d_out overlapping d_in GM_ERR_INVALID_ARG, each with nothing launched and
 * the state unchanged.  n_in = 0: GM_OK, *n_out = 0.  At most 2^31 samples a call. */
int gm_channelizer_process_dev(gm_channelizer *c, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_stride, size_t out_cap,
                               size_t *n_out, void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream); out is [C][out_cap] */
int gm_channelizer_process(gm_channelizer *c, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out);
int gm_channelizer_synchronize(gm_channelizer *c);

/* ------------------------------------------------------------------ Adaptive spatial nulling of an antenna array
 * A gm_nuller takes A coherent antennas (2 .. 8) as ONE interleaved stream of GM_FMT_C32 or GM_FMT_I8_IQ elements — time sample n of
 * antenna a is element n * A + a, the layout a multi-channel SDR delivers — and combines them into one c32 stream at the same rate
 * and time index (no timestamp delay) with weights that put a null on whatever dominates the block's covariance: the wideband noise
 * jammer, long in time and as wide as the signal, that neither blanking nor a notch can touch.  Every count below is in TIME samples.
 * Everything is defined by ABSOLUTE indices: the words do not depend on how the stream is cut into calls, and two runs give the same
 * words.
 *   Blocks.  Block b covers the time samples [b B, (b+1) B); B is a power of two in 256 .. 16384.  After T time samples
 *     total_out(T) = B * (T div B) outputs exist; a call delivers the difference, computed on the host with no synchronisation.  The
 *     (converted) time samples of the unfinished block travel between calls in the handle's history buffers.  There is no flush: a
 *     caller that needs the tail appends zeros.
 *   Covariance, from the block's own samples, f32:  R[i][j] = sum_{t<B} x_i[bB + t] conj(x_j[bB + t])  for i <= j; an int8 sample is
 *     converted to f32 first (-128 is -128.0f).  The diagonal's imaginary part is 0 and R[j][i] = conj(R[i][j]).  THE ORDER: 256 lane
 *     sums S[l], l = 0 .. 255, each over t = l, l + 256, l + 512, ... ascending from +0 with, per t,
 *       re = fmaf(xi.re, xj.re, re);  re = fmaf(xi.im, xj.im, re);  im = fmaf(xi.im, xj.re, im);  im = fmaf(-xi.re, xj.im, im);
 *     then, within each group of 64 lanes, S[l] = S[l] + S[l + d] for d = 32, 16, 8, 4, 2, 1 (the group's sum W is its lane 0), then
 *     R = (W0 + W1) + (W2 + W3).  A function of the block-relative t alone; no floating-point atomics.  Within
 *     (B/256 + 12) 2^-24 sum_t |x_i| |x_j| of the exact sum.
 *   Weights, f64 from the f32 words of R:  tr = sum_i Re R[i][i] (i ascending);  Rl = R + loading * (tr / A) * I, loading being the
 *     f32 word widened;  u = Rl^-1 s;  w = u / (s^H u);  each component of w rounded once to f32.  The device solves by Cholesky,
 *     Rl = L L^H: z = L^-1 s, s^H u = z^H z (real by construction), u = L^-H z.  tr = 0 (an all-zero block): w = s / (s^H s).
 *     s is the caller's steering vector (A c32 words, not all zero): the response is held at 1 in its direction.  NULL means e_0 —
 *     power inversion with antenna 0 as the reference, and Re w[0] comes out as 1.0f.
 *   Output, f32:  y[bB + t] = sum_a conj(w[a]) x_a[bB + t], w the f32 words just rounded: from +0, a ASCENDING, per a
 *       re = fmaf(w.re, x.re, re);  re = fmaf(w.im, x.im, re);  im = fmaf(w.re, x.im, im);  im = fmaf(-w.im, x.re, im);
 *     within (A + 2) 2^-24 sum_a |w[a]| |x_a| of the exact value.
 *   Static mode.  gm_nuller_set_weights installs A fixed weights used for every block; the covariance pass is skipped; counts and
 *     block delivery are unchanged.
 *   Monitor.  gm_nuller_capture names device buffers that every later gm_nuller_process_dev fills with its blocks' R and w words.
 *   Kernel (csrc/nuller_kernels.hip): one 256-lane workgroup per block: the sums in registers, shuffles and LDS for the tree, the
 *     solve in wave 0 fully unrolled on A, a second read of the block (from L2) for y; a state kernel carries the unfinished block.
 * Not built: a ring writer with the nuller as head stage; wiring into receiver_harness.cpp; array calibration (taps in time are a
 * stage of their own, gm_stap below);
 * blanking inside the stage (its output goes into a gm_excisor or gm_resampler, which blank); any decision — the library reports R
 * and w, the caller judges.
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t n_antennas;      /* A: 2 .. 8 */
    uint32_t block;           /* B: a power of two in 256 .. 16384; 0 -> 1024 */
    float    loading;         /* [1e-6, 1]: diagonal loading as a fraction of the mean antenna power tr / A; 0 -> 1e-4 */
    uint32_t reserved;        /* must be 0 */
    const gm_c32 *steering;   /* [A] c32 words, finite, not all zero; NULL -> e_0.  Read during the call that takes the cfg only. */
} gm_nuller_cfg;
typedef struct gm_nuller gm_nuller;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG for an A, B or loading outside its range, a non-finite loading or
 * steering word, an all-zero steering, reserved != 0, inputs_so_far + n_in above 2^62); *block = B, *loading = the f32 word used and,
 * for a stream that has taken inputs_so_far time samples, the count of outputs that n_in more deliver.  Any output pointer may be
 * NULL. */
int gm_nuller_plan(const gm_nuller_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *block, float *loading, uint64_t *n_out);
int gm_nuller_create(const gm_nuller_cfg *cfg, gm_nuller **out);
int gm_nuller_destroy(gm_nuller *n);
/* Zeroes the history and the counters; the stream continues as if input_index zero time samples had gone before: the first block
 * delivered is block input_index div B, whose first input_index mod B samples are those zeros.  Keeps the weights mode and the
 * capture.  Synchronous.  input_index above 2^62: GM_ERR_INVALID_ARG. */
int gm_nuller_reset(gm_nuller *n, uint64_t input_index);
/* time samples taken, outputs delivered and blocks finished since gm_nuller_create or the last gm_nuller_reset, each counted once
 * (any pointer may be NULL).  Synchronises the handle's stream and the stream the last call ran on. */
int gm_nuller_stats(gm_nuller *n, uint64_t *inputs, uint64_t *outputs, uint64_t *blocks);
int gm_nuller_synchronize(gm_nuller *n);
/* w: A finite c32 words used for every later block (static mode: y = sum_a conj(w[a]) x_a, no covariance pass); NULL returns the
 * handle to the adaptive rule.  The words are copied during the call and travel with each later call's launch, so the change is
 * ordered with the handle's calls: every call made before it used the old rule, every later one uses the new. */
int gm_nuller_set_weights(gm_nuller *n, const gm_c32 *w);
/* Every later gm_nuller_process_dev writes its blocks' words to device memory, block k of the CALL at d_R + k A A (c32 [A][A], row
 * i column j = R[i][j]) and d_w + k A (c32 [A]), from word 0 on each call; a call that finishes more than cap_blocks blocks is
 * refused (GM_ERR_OUT_OF_RANGE) before anything runs.  In static mode only w is written.  d_R = d_w = NULL with cap_blocks = 0 ends
 * the capture; one pointer without the other, or pointers with cap_blocks = 0, is GM_ERR_INVALID_ARG. */
int gm_nuller_capture(gm_nuller *n, void *d_R, void *d_w, size_t cap_blocks);
/* d_in (n_in TIME samples, n_in * A elements of GM_FMT_C32 or GM_FMT_I8_IQ; GM_FMT_I8_REAL is refused) -> d_out, c32: this call's
 * *n_out outputs; words behind them are not touched (n_out may be NULL).  Asynchronous on `stream` (a hipStream_t; NULL: the handle's
 * own non-blocking stream); consecutive calls of a handle must be ordered against each other (one stream, or the caller's events).
 * Every argument is checked before anything runs: out_cap below the count is GM_ERR_OUT_OF_RANGE, as is a capture too small for the
 * call's blocks; d_out overlapping d_in, a NULL where a pointer is needed, more than 2^31 time samples in a call or a stream index
 * above 2^62 GM_ERR_INVALID_ARG; each with nothing launched and the state unchanged.  n_in = 0: GM_OK, *n_out = 0. */
int gm_nuller_process_dev(gm_nuller *n, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_cap, size_t *n_out, void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream).  R ([blocks][A][A]) and w ([blocks][A]) are host
 * buffers for the call's block words, each may be NULL; with either given, cap_blocks below the call's blocks is GM_ERR_OUT_OF_RANGE.
 * In static mode R is left untouched.  A device capture set by gm_nuller_capture is not written by this form. */
int gm_nuller_process(gm_nuller *n, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out, gm_c32 *R,
                      gm_c32 *w, size_t cap_blocks);

/* ------------------------------------------------------------------ Space-time adaptive nulling: taps on every antenna
 * A gm_stap is a gm_nuller with L taps in time (1 .. 8) behind each of the A antennas (2 .. 8), M = A L <= 32 weights in all: a
 * narrowband interferer then costs one temporal degree of freedom, not one of the A - 1 spatial ones.  The input is the nuller's: ONE
 * interleaved stream of GM_FMT_C32 or GM_FMT_I8_IQ elements, time sample n of antenna a being element n * A + a; the output one c32
 * stream at the same rate and time index (no timestamp delay).  Every count is in TIME samples; everything is defined by ABSOLUTE
 * indices: the words do not depend on how the stream is cut into calls, and two runs give the same words.
 *   Blocks.  Block b covers the time samples [b B, (b+1) B); B is a power of two in 256 .. 16384.  After T time samples
 *     total_out(T) = B * (T div B) outputs exist; a call delivers the difference, computed on the host with no synchronisation.  There
 *     is no flush.  The handle's history carries the (converted) time samples of the unfinished block and the L - 1 in front of it.
 *   Stacked sample.  z[t][l A + a] = x_a[t - l], t absolute, l = 0 .. L - 1; an int8 sample is converted to f32 first (-128 is
 *     -128.0f).  Samples before the stream's start are zeros, and after gm_stap_reset(input_index) so are those before input_index.
 *   Covariance, f32: the exact Gram matrix of the block's stacked samples (not a Toeplitz approximation),
 *       R[p][q] = sum_{t in [bB, (b+1)B)} z_p[t] conj(z_q[t]),
 *     Hermitian word for word, the diagonal's imaginary part +0.  THE ORDER, for p = l A + a <= q = (l + k) A + b, with u = t - l
 *     relative to the block's start and the term of u being x_a[u] conj(x_b[u - k]), accumulated as
 *       re = fmaf(xa.re, xb.re, re);  re = fmaf(xa.im, xb.im, re);  im = fmaf(xa.im, xb.re, im);  im = fmaf(-xa.re, xb.im, im):
 *     (1) the INTERIOR u in [0, B - L + 1), which all entries of a lag k and pair (a, b) share, in groups of 1024 (the last one
 *     shorter; one group where B <= 1024): per group 64 lane sums S[j], each over u = j, j + 64, j + 128, ... of the group ascending from
 *     +0, then S[j] = S[j] + S[j + d] for d = 32, 16, 8, 4, 2, 1, the group's sum being S[0]; the groups' sums are added in ascending
 *     order, from +0.  (2) Then the entry's own L - 1 edge terms, one by one: u = -l .. -1, then u = B - L + 1 .. B - l - 1.
 *     A function of the block-relative position alone; no floating-point atomics.  Each component goes through at most
 *     min(B, 1024) / 32 + 6 + B / 1024 + 2 (L - 1) roundings (68 at B = 16384, L = 8), so the entry is within
 *     sqrt(2) * 68 * 2^-24 = 5.8e-6 of sum_t |z_p| |z_q| of the exact sum.
 *   Weights, f64 from the f32 words of R:  tr = sum_p Re R[p][p] (p ascending);  Rl = R + loading * (tr / M) * I, loading being the f32
 *     word widened;  u = Rl^-1 s;  w = u / (s^H u);  each component of w rounded once to f32.  The device solves by Cholesky,
 *     Rl = C C^H (left-looking, columns ascending): z = C^-1 s, s^H u = z^H z, u = C^-H z.
 *     s is the caller's constraint vector, M c32 words [L][A], not all zero; NULL means e_0 (antenna 0 at tap 0: power inversion with
 *     no delay), and Re w[0] comes out as 1.0f.
 *   Fallback.  w = s / (s^H s) where tr = 0, or a Cholesky pivot (or z^H z) is not greater than 0 or not finite; the block is counted
 *     in fallback_blocks.  Finite input never produces a NaN.
 *   Output, f32:  y[t] = sum_l sum_a conj(w[l A + a]) x_a[t - l], w the f32 words just rounded: from +0, l ASCENDING, then a ascending,
 *       re = fmaf(w.re, x.re, re);  re = fmaf(w.im, x.im, re);  im = fmaf(w.re, x.im, im);  im = fmaf(-w.im, x.re, im);
 *     within (M + 2) 2^-24 sum |w| |z| of the exact value.  Block b's weights serve all B of its outputs, the taps that reach back into
 *     block b - 1 included.
 *   Static mode.  gm_stap_set_weights installs M fixed weights used for every block; no Gram matrix is formed.
 *   Monitor.  gm_stap_capture names device buffers that every later gm_stap_process_dev fills with its blocks' R and w words.
 *   Kernel (csrc/stap_kernels.hip): one 256-lane workgroup per block; the block passes through LDS in chunks of 256 + L - 1 samples;
 *     the four waves share the lags; the solve in LDS in f64; a second pass through the same chunks for y; a state kernel.
 * Limits (README, measured by tests/stap_model.py): ONE constraint shapes the signal's spectrum — at L = 2 a correlation peak can land
 * a sample off (gm_lcmv below holds the later taps to 0 with a constraint each); a reference on tap l0 delays the peak by l0
 * samples; a quantiser's clipping products are not low rank.
 * Not built: a ring writer with the stage at its head; wiring into receiver_harness.cpp; array calibration; any decision — the
 * library reports R, w and the fallback count, the caller judges.  (One beam per constraint is gm_beamformer below;
 * several constraints on ONE beam (LCMV) is gm_lcmv below it.)
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t n_antennas;      /* A: 2 .. 8 */
    uint32_t taps;            /* L: 1 .. 8, A L <= 32 */
    uint32_t block;           /* B: a power of two in 256 .. 16384; 0 -> 1024 */
    float    loading;         /* [1e-6, 1]: diagonal loading as a fraction of the mean stacked power tr / M; 0 -> 1e-4 */
    const gm_c32 *steering;   /* [L][A] c32 words, finite, not all zero; NULL -> e_0.  Read during the call that takes the cfg only. */
    uint64_t reserved;        /* must be 0 */
} gm_stap_cfg;
typedef struct gm_stap gm_stap;
/* host only, no device: the argument rules (GM_ERR_INVALID_ARG for an A, L, A L, B or loading outside its range, a non-finite loading
 * or steering word, an all-zero steering, reserved != 0, inputs_so_far + n_in above 2^62); *block = B, *loading = the f32 word used
 * and, for a stream that has taken inputs_so_far time samples, the count of outputs that n_in more deliver.  Any output pointer may
 * be NULL. */
int gm_stap_plan(const gm_stap_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *block, float *loading, uint64_t *n_out);
int gm_stap_create(const gm_stap_cfg *cfg, gm_stap **out);
int gm_stap_destroy(gm_stap *n);
/* Zeroes the history and the counters; the stream continues as if input_index zero time samples had gone before.  Keeps the weights
 * mode and the capture.  Synchronous.  input_index above 2^62: GM_ERR_INVALID_ARG. */
int gm_stap_reset(gm_stap *n, uint64_t input_index);
/* time samples taken, outputs delivered, blocks finished and blocks that took the fallback weights since gm_stap_create or the last
 * gm_stap_reset (any pointer may be NULL).  Synchronises the handle's stream and the stream the last call ran on. */
int gm_stap_stats(gm_stap *n, uint64_t *inputs, uint64_t *outputs, uint64_t *blocks, uint64_t *fallback_blocks);
int gm_stap_synchronize(gm_stap *n);
/* w: M finite c32 words [L][A] used for every later block (static mode); NULL returns the handle to the adaptive rule.  The words
 * are copied during the call and travel with each later call's launch. */
int gm_stap_set_weights(gm_stap *n, const gm_c32 *w);
/* Every later gm_stap_process_dev writes its blocks' words to device memory, block k of the CALL at d_R + k M M (c32 [M][M], row p
 * column q = R[p][q]) and d_w + k M (c32 [M]), from word 0 on each call; a call that finishes more than cap_blocks blocks is refused
 * (GM_ERR_OUT_OF_RANGE) before anything runs.  In static mode only w is written.  d_R = d_w = NULL with cap_blocks = 0 ends the
 * capture; one pointer without the other, or pointers with cap_blocks = 0, is GM_ERR_INVALID_ARG. */
int gm_stap_capture(gm_stap *n, void *d_R, void *d_w, size_t cap_blocks);
/* d_in (n_in TIME samples, n_in * A elements of GM_FMT_C32 or GM_FMT_I8_IQ; GM_FMT_I8_REAL is refused) -> d_out, c32: this call's
 * *n_out outputs; words behind them are not touched (n_out may be NULL).  Asynchronous on `stream` (a hipStream_t; NULL: the handle's
 * own non-blocking stream); consecutive calls of a handle must be ordered against each other.  Every argument is checked before
 * anything runs, with gm_nuller_process_dev's refusals; each with nothing launched and the state unchanged.  n_in = 0: GM_OK. */
int gm_stap_process_dev(gm_stap *n, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_cap, size_t *n_out, void *stream);
/* the synchronous host-buffer form (H2D, the kernels, D2H on the handle's stream).  R ([blocks][M][M]) and w ([blocks][M]) are host
 * buffers for the call's block words, each may be NULL; with either given, cap_blocks below the call's blocks is GM_ERR_OUT_OF_RANGE.
 * In static mode R is left untouched.  A device capture set by gm_stap_capture is not written by this form. */
int gm_stap_process(gm_stap *n, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_cap, size_t *n_out, gm_c32 *R,
                    gm_c32 *w, size_t cap_blocks);

/* ------------------------------------------------------------------ One beam per satellite from a shared covariance
 * A gm_beamformer is a gm_stap with P constraint vectors (1 .. 16) in place of one: a receiver with an array wants a beam per satellite
 * it tracks, plus a power-inversion beam to search in, and all of them share the block's Gram matrix and its Cholesky factor.  What a
 * beam costs beyond that is one more substitution and one more output pass over a block already staged on chip.
 *   Input and parameters.  gm_stap's: ONE interleaved stream of A antennas (2 .. 8), GM_FMT_C32 or GM_FMT_I8_IQ; L taps (1 .. 8),
 *     M = A L <= 32; B a power of two in 256 .. 16384 (0 -> 1024); loading in [1e-6, 1] (0 -> 1e-4).  Blocks, counts
 *     (total_out(T) = B * (T div B) PER BEAM), the history, gm_beamformer_reset and the zero halo are gm_stap's.
 *   Beams.  Beam p has its own constraint vector s_p: M c32 words [L][A], finite, not all zero.  `steering` is [P][L][A] and is
 *     required; a caller who wants power inversion passes e_0 as a row.
 *   Per block.  ONE Gram matrix R, gm_stap's, in gm_stap's stated order; ONE loaded matrix Rl and ONE factor Rl = C C^H.  Per beam:
 *     z_p = C^-1 s_p, u_p = C^-H z_p = Rl^-1 s_p, w_p = u_p / (z_p^H z_p), each component rounded once to f32, and
 *     y_p[t] = sum_l sum_a conj(w_p[l A + a]) x_a[t - l] in gm_stap's order.
 *   THE CONTRACT THAT FIXES EVERY WORD.  Beam p's R, w and y words and its fallback count are word for word those of a gm_stap created
 *     with the same A, L, B, loading and steering = s_p, fed the same stream.  So a beam's words depend neither on P nor on the other
 *     rows, nor on how the stream is cut into calls, nor on repetition.
 *   Fallback.  gm_stap's rule per beam: tr = 0 or a bad pivot sends every beam of the block to w_p = s_p / (s_p^H s_p); a z_p^H z_p
 *     that is not greater than 0 or not finite sends beam p alone.  The counters are per beam.
 *   Output, planar: beam p's stream is d_out + p * out_stride (c32 elements), so a plane goes straight into gm_acq_search_dev, an
 *     excisor or a resampler.  out_stride below the call's count is GM_ERR_OUT_OF_RANGE.  Words of a plane behind the count, and
 *     between planes, are not touched.
 *   Moving beams.  gm_beamformer_set_steering replaces one row, gm_beamformer_set_weights installs P M fixed weights (static mode, no
 *     Gram matrix).  Both apply to every block finished by a LATER call; blocks of earlier calls keep the old words.  The P M words
 *     (up to 4 KB each for s and w) live in device memory of the handle, and BOTH ENTRIES ARE SYNCHRONOUS: they first wait for every
 *     call of the handle in flight (on the handle's stream and on the stream the last call ran on), then copy, and return when the
 *     words are in place.  (A caller whose own stream is held back behind an event it has yet to record must not call them before.)
 *   Monitor.  gm_beamformer_capture names device buffers that every later gm_beamformer_process_dev fills with its blocks' R
 *     ([blocks][M][M]) and w ([blocks][P][M]) words.
 *   Kernel (csrc/beam_kernels.hip): gm_stap's workgroup per block with gm_stap's own code (csrc/stap_core.h) for the staging, the
 *     Gram matrix and the factorisation, the P rows riding below the matrix; the substitution eight beams at a time; the output pass
 *     four beams at a time from one read of the staged samples; gm_stap's state kernel.
 * Not built: a ring writer; wiring into receiver_harness.cpp; array calibration; deriving the rows from satellite directions; any
 * decision.  (Several constraints on one beam are gm_lcmv below.)
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t n_antennas;      /* A: 2 .. 8 */
    uint32_t taps;            /* L: 1 .. 8, A L <= 32 */
    uint32_t block;           /* B: a power of two in 256 .. 16384; 0 -> 1024 */
    float    loading;         /* [1e-6, 1]; 0 -> 1e-4 */
    uint32_t n_beams;         /* P: 1 .. 16 */
    uint32_t reserved32;      /* must be 0 */
    const gm_c32 *steering;   /* [P][L][A] c32 words, every row finite and not all zero; required.  Read during the call that takes the cfg only. */
    uint64_t reserved;        /* must be 0 */
} gm_beamformer_cfg;
typedef struct gm_beamformer gm_beamformer;
/* host only, no device: gm_stap_plan's rules, and GM_ERR_INVALID_ARG for P outside 1 .. 16, a NULL steering, a row that is not finite
 * or all zero, reserved32 != 0 or reserved != 0.  *n_out is the count PER BEAM.  Any output pointer may be NULL. */
int gm_beamformer_plan(const gm_beamformer_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *block, float *loading,
                       uint64_t *n_out);
int gm_beamformer_create(const gm_beamformer_cfg *cfg, gm_beamformer **out);
int gm_beamformer_destroy(gm_beamformer *h);
/* gm_stap_reset: zeroes the history and every counter; keeps the rows, the weights mode and the capture.  Synchronous. */
int gm_beamformer_reset(gm_beamformer *h, uint64_t input_index);
/* time samples taken, outputs delivered PER BEAM, blocks finished, and in fallbacks[p] (P words) the blocks whose beam p took the
 * fallback weights, since gm_beamformer_create or the last reset (any pointer may be NULL).  Synchronises like gm_stap_stats. */
int gm_beamformer_stats(gm_beamformer *h, uint64_t *inputs, uint64_t *outputs, uint64_t *blocks, uint64_t *fallbacks);
int gm_beamformer_synchronize(gm_beamformer *h);
/* s: the M words [L][A] of beam `beam`'s new row (finite, not all zero; beam >= P, a bad row or a NULL: GM_ERR_INVALID_ARG with
 * nothing changed).  Synchronous, see "Moving beams". */
int gm_beamformer_set_steering(gm_beamformer *h, uint32_t beam, const gm_c32 *s);
/* n_rows rows from DEVICE memory into beams first_beam .. first_beam + n_rows - 1, by a kernel on `stream` (NULL: the handle's own),
 * ordered like a process_dev call; no host wait.  "Re-steering on the device" above states the gate (d_info, min_ratio), d_installed
 * and the refusals. */
int gm_beamformer_set_steering_dev(gm_beamformer *h, uint32_t first_beam, uint32_t n_rows, const void *d_rows /* [n_rows][M] c32 */,
                                   const void *d_info /* [n_rows] gm_array_row_info or NULL */, float min_ratio,
                                   void *d_installed /* [n_rows] u8 or NULL */, void *stream);
/* w: P M finite c32 words [P][L][A] used for every later block (static mode); NULL returns the handle to the adaptive rule (and
 * waits for nothing).  Synchronous, see "Moving beams". */
int gm_beamformer_set_weights(gm_beamformer *h, const gm_c32 *w);
/* gm_stap_capture with block k of the CALL at d_R + k M M (c32 [M][M]) and d_w + k P M (c32 [P][M]).  In static mode only w is
 * written. */
int gm_beamformer_capture(gm_beamformer *h, void *d_R, void *d_w, size_t cap_blocks);
/* d_in (n_in TIME samples, n_in * A elements) -> beam p's *n_out outputs at d_out + p * out_stride (c32 elements).  Asynchronous on
 * `stream` like gm_stap_process_dev, with its refusals, all before anything runs and with state, outputs and captures untouched;
 * out_stride below the call's count is GM_ERR_OUT_OF_RANGE, and the overlap check against d_in covers
 * [d_out, d_out + (P - 1) out_stride + count).  n_in = 0: GM_OK. */
int gm_beamformer_process_dev(gm_beamformer *h, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_stride, size_t *n_out,
                              void *stream);
/* the synchronous host-buffer form; beam p's outputs at out + p * out_stride.  R ([blocks][M][M]) and w ([blocks][P][M]) are host
 * buffers for the call's block words, each may be NULL; with either given, cap_blocks below the call's blocks is GM_ERR_OUT_OF_RANGE.
 * In static mode R is left untouched.  A device capture set by gm_beamformer_capture is not written by this form. */
int gm_beamformer_process(gm_beamformer *h, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_stride, size_t *n_out,
                          gm_c32 *R, gm_c32 *w, size_t cap_blocks);

/* ------------------------------------------------------------------ Several constraints on one beam
 * A gm_lcmv is a gm_beamformer whose beam p carries Q_p constraint rows c_q and Q_p responses f_q in place of one row: the beam's
 * weights answer C^H w = f at the least output power.  Two uses (README, measured by tests/lcmv_model.py): a second row with the
 * response 0 removes a signal that power minimisation does not see because it lies below the noise (a spoofer, a repeater, a
 * strong reflection: its row is what gm_acq_array_prompts and gm_array_row_solve return for its cell); one row per tap (the
 * satellite's row on tap 0 answers 1, the same row on taps 1 .. L - 1 answers 0) keeps a space-time beam from skewing the
 * correlation triangle.  It is a handle of its own: gm_beamformer's words are unchanged.
 *   Shapes.  A is 2 .. 8, L is 1 .. 8, M = A L <= 32; B, loading, the formats (GM_FMT_C32, GM_FMT_I8_IQ), the interleaved input, the
 *     stacked sample z[t][l A + a] = x_a[t - l], blocks, counts (total_out(T) = B * (T div B) PER BEAM), the history, gm_lcmv_reset
 *     and the zero halo are gm_stap's.
 *   Beams.  P is 1 .. 16.  n_constraints[p] = Q_p is 1 .. 8 with Q_p <= M, and sum_p Q_p <= 16.  `constraints` holds [sum Q][M] c32
 *     words, each row laid out [L][A]; `response` holds [sum Q] c32 words; the rows of beam p are consecutive, beam 0's first.
 *   Weights.  Per block R, tr and Rl = R + loading (tr / M) I exactly as gm_stap forms them: R's words are gm_beamformer's bit for
 *     bit on the same input.  Then, in f64, with C the M x Q_p matrix whose columns are beam p's rows:
 *       1. Rl = Lc Lc^H (gm_stap's factor, ONE for all beams);   2. z_q = Lc^-1 c_q for every row of every beam, in that factor;
 *       3. G[q][r] = z_q^H z_r, the index ascending within each sum;   4. G = Lg Lg^H;   5. v = G^-1 f;
 *       6. t = sum_q z_q v_q, q ascending;   7. u = Lc^-H t;   8. w_p = u, each component rounded once to f32.
 *     So C^H w = f: w = Rl^-1 C (C^H Rl^-1 C)^-1 f.  The output is y = w^H z, so a signal whose stacked vector is c_q comes out with
 *     the gain conj(f_q).  At Q = 1 and f = 1 this is gm_beamformer's w, equal to rounding and NOT word for word (the division by
 *     z^H z comes before the last substitution here).
 *   Fallback.  ALL beams of a block fall back where tr = 0 or a pivot of Lc is not greater than 0 or not finite; beam p ALONE where a
 *     pivot of its Lg is not greater than 0 or not finite, or a word of u is not finite (as the f32 word it rounds to: a w above
 *     the f32 range would turn a zero sample into a NaN).  A beam that falls back takes its
 *     quiescent weights w0_p = C (C^H C)^-1 f (at Q = 1: f s / (s^H s)) and the block is counted for that beam.  The host computes
 *     w0 in f64 at gm_lcmv_create and at every gm_lcmv_set_constraints, rounds it once and keeps it on the device.  Finite input
 *     never produces a NaN.
 *   Output, static mode, monitor: gm_beamformer's.  P planes, beam p's stream at d_out + p * out_stride; pass 2's sums in gm_stap's
 *     order (l ascending, then a, one fmaf per real product); gm_lcmv_set_weights installs P M fixed weights (no Gram matrix);
 *     gm_lcmv_capture names device buffers for R ([blocks][M][M]) and w ([blocks][P][M]); gm_lcmv_stats gives the fallback counts
 *     per beam.
 *   A beam's words depend on its own rows and responses, R and the cfg alone: neither on P, nor on the other beams, nor on how the
 *     stream is cut into calls, nor on repetition.
 *   Moving beams.  gm_lcmv_set_constraints replaces the rows and responses of one beam (their number may change as long as the sum
 *     stays <= 16) for every block finished by a LATER call; SYNCHRONOUS, ordered as gm_beamformer_set_steering is.
 *   Kernel (csrc/lcmv_kernels.hip): gm_beamformer's workgroup per block with csrc/stap_core.h's staging, Gram matrix and factor, the
 *     rows of all beams riding below the matrix; then per beam, eight beams a round, the small Gram matrix (in the LDS words R leaves
 *     once it has gone to the capture), its Cholesky factor with f^H riding below it, and the two substitutions; gm_beamformer's
 *     output pass; gm_stap's state kernel.
 * Not built: a _dev form of gm_lcmv_set_constraints; choosing which cells are spoofers, or any other decision (the beams go into a plane ring: "Plane ring" below); wiring
 * into receiver_harness.cpp or bench.py; inequality or derivative constraints.
 * (ABI 9, additive: a caller detects the feature by the symbol) */
typedef struct {
    uint32_t n_antennas;      /* A: 2 .. 8 */
    uint32_t taps;            /* L: 1 .. 8, A L <= 32 */
    uint32_t block;           /* B: a power of two in 256 .. 16384; 0 -> 1024 */
    float    loading;         /* [1e-6, 1]; 0 -> 1e-4 */
    uint32_t n_beams;         /* P: 1 .. 16 */
    uint32_t reserved32;      /* must be 0 */
    const uint32_t *n_constraints; /* [P]: Q_p in 1 .. 8, Q_p <= A L, their sum <= 16; required */
    const gm_c32 *constraints;     /* [sum Q][L][A] c32 words, beam 0's rows first; required */
    const gm_c32 *response;   /* [sum Q] c32 words, in the rows' order; required.  All three are read during the call that takes the cfg only. */
    uint64_t reserved;        /* must be 0 */
} gm_lcmv_cfg;
typedef struct gm_lcmv gm_lcmv;
/* host only, no device: gm_beamformer_plan's rules (with n_constraints, constraints and response required in place of steering), and
 * GM_ERR_INVALID_ARG for a Q_p outside 1 .. 8 or above M; sum Q > 16; a row that is not finite or is all zero; a response word that
 * is not finite; rows of one beam that are linearly dependent (a Cholesky pivot of C^H C, columns ascending, not greater than 1e-10
 * times that row's squared norm, in f64); quiescent weights that are not finite in f32.  *n_out is the count PER BEAM.  Any output
 * pointer may be NULL. */
int gm_lcmv_plan(const gm_lcmv_cfg *cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t *block, float *loading, uint64_t *n_out);
int gm_lcmv_create(const gm_lcmv_cfg *cfg, gm_lcmv **out);
int gm_lcmv_destroy(gm_lcmv *h);
/* gm_stap_reset: zeroes the history and every counter; keeps the rows, the weights mode and the capture.  Synchronous. */
int gm_lcmv_reset(gm_lcmv *h, uint64_t input_index);
/* time samples taken, outputs delivered PER BEAM, blocks finished, and in fallbacks[p] (P words) the blocks whose beam p took its
 * quiescent weights, since gm_lcmv_create or the last reset (any pointer may be NULL).  Synchronises like gm_stap_stats. */
int gm_lcmv_stats(gm_lcmv *h, uint64_t *inputs, uint64_t *outputs, uint64_t *blocks, uint64_t *fallbacks);
int gm_lcmv_synchronize(gm_lcmv *h);
/* beam `beam`'s new rows ([n_rows][L][A]) and responses ([n_rows]), under gm_lcmv_plan's rules for one beam and for the sum; a
 * refusal (also beam >= P or a NULL) is GM_ERR_INVALID_ARG with nothing changed.  Synchronous, see "Moving beams". */
int gm_lcmv_set_constraints(gm_lcmv *h, uint32_t beam, uint32_t n_rows, const gm_c32 *rows, const gm_c32 *response);
/* w: P M finite c32 words [P][L][A] used for every later block (static mode); NULL returns the handle to the adaptive rule (and
 * waits for nothing).  Synchronous like gm_beamformer_set_weights. */
int gm_lcmv_set_weights(gm_lcmv *h, const gm_c32 *w);
/* gm_beamformer_capture: block k of the CALL at d_R + k M M (c32 [M][M]) and d_w + k P M (c32 [P][M]).  In static mode only w is
 * written. */
int gm_lcmv_capture(gm_lcmv *h, void *d_R, void *d_w, size_t cap_blocks);
/* gm_beamformer_process_dev: d_in (n_in TIME samples, n_in * A elements) -> beam p's *n_out outputs at d_out + p * out_stride (c32
 * elements).  Asynchronous on `stream` (NULL: the handle's own) under the streaming stages' rule, with gm_beamformer_process_dev's
 * refusals, all before anything runs and with state, outputs and captures untouched.  n_in = 0: GM_OK. */
int gm_lcmv_process_dev(gm_lcmv *h, const void *d_in, int fmt, size_t n_in, void *d_out, size_t out_stride, size_t *n_out, void *stream);
/* the synchronous host-buffer form, gm_beamformer_process's: beam p's outputs at out + p * out_stride; R ([blocks][M][M]) and w
 * ([blocks][P][M]) are host buffers for the call's block words, each may be NULL. */
int gm_lcmv_process(gm_lcmv *h, const void *in, int fmt, size_t n_in, gm_c32 *out, size_t out_stride, size_t *n_out, gm_c32 *R,
                    gm_c32 *w, size_t cap_blocks);

/* ------------------------------------------------------------------ Tracking
 * The evolving fields of TrackingChannel (src/tracking/do_tracking.rs:88-116). */
typedef struct {
    uint8_t prn;
    uint8_t active;            /* state == ChannelState::Tracking(prn) */
    uint8_t reserved[2];
    uint32_t lost_counter;
    uint64_t next_sample_index;
    uint64_t num_samples_per_code;
    float carrier_freq, carrier_phase, carrier_error, carrier_nco;
    float code_phase, code_error, code_nco, code_rate;
    float i_prompt, q_prompt;
} gm_trk_state;

/* Correlator outputs of one epoch: (i_p,q_p,i_e,q_e,i_l,q_l) = early_late_correlation() :231-272,
 * plus very-early / very-late for 5-arm configurations. */
typedef struct {
    float ip, qp, ie, qe, il, ql, ive, qve, ivl, qvl;
} gm_trk_out;

typedef enum { GM_CODE_INDEX_FAITHFUL = 0, GM_CODE_INDEX_FIXED = 1 } gm_code_index_mode;

typedef struct {
    float fs;
    uint32_t n_channels;       /* NUM_OF_CHANNELS = 15 (:18) */
    uint32_t n_arms;           /* 3 (E/P/L, reference) or 5 (VE/E/P/L/VL) */
    float early_late_space;    /* EARLY_LATE_SPACE = 0.5 chips (:28); 0 -> 0.5 */
    float very_early_late_space; /* 5-arm only; 0 -> 1.0 */
    int32_t code_index_mode;   /* FAITHFUL: get_ca_chip indexes row `prn` and saturates negative phases to
                                  chip 0 exactly like :274-277; FIXED: row prn-1, wrapping */
    int32_t boc11;             /* 1: multiply the chip by the BOC(1,1) sub-carrier sign (no reference code) */
    const int8_t *codes;       /* optional [n_codes][code_len] custom +-1 chips (NULL: GPS C/A table).  The tracking kernel keeps
                                  a channel's row in LDS as floats: 4 (code_len + 3) bytes, 12 code_len + 48 with boc11, beside
                                  ~2.6 KB of its own, within the device's LDS per workgroup.  gm_trk_create checks this against
                                  the kernel and the device it runs on and returns GM_ERR_OUT_OF_RANGE (the sizes in
                                  gm_last_error) for a code that does not fit; 10 230 chips without boc11 (41 KB) do. */
    uint32_t n_codes, code_len;
    float nominal_code_rate;   /* 0 -> 1.023e6 */
    /* loop constants (:16-27); 0 -> reference value */
    float pll_bw, pll_zeta, pll_gain, dll_bw, dll_zeta, dll_gain, pll_dt, dll_dt;
    float lock_threshold;      /* LOCK_THRESHOLD = 15 (:16) */
    uint32_t max_lost_epochs;  /* MAX_LOST_EPOCHS = 20 (:17) */
    int32_t strict_libm;       /* 1: the carrier's cos / sin (`phase.cos()`, `phase.sin()`, :234-235) are glibc 2.35's cosf / sinf
                                  restated on the device, bit for bit (csrc/gm_libm.h sincosf_glibc: f64 reduction + polynomial,
                                  one rounding) — every sample's products then equal the reference host's; 0 (default): the
                                  device's own < 1 ulp forms, which differ from glibc's in the last bit on a quarter of the
                                  samples.  ABI version 4. */
    int32_t strict_sum_order;  /* 1: the correlator sums are added sample by sample in f32, the reference's own order
                                  (`i_p += re * p_chip`, :256-262) — one serial wave per channel instead of the persistent
                                  kernel's tree (csrc/trk_kernels.hip trk_serial_sum_kernel; ~40x its time per epoch).  With
                                  strict_libm as well, every correlator sum and every word of the channel state equal the
                                  reference's bit for bit, free-running.  0 (default): tree sums, within 1e-5 of the
                                  envelope and closer to the exact sum.  ABI version 4. */
    int32_t share_device;      /* 1: a receiver — the persistent tracking kernel takes at most a QUARTER of the device's resident
                                  workgroup places (workgroups per channel chosen accordingly), so that the other stages' kernels
                                  (the digital front-end writing the ring needs a whole CU per stream, an acquisition dwell every
                                  CU it can get) run BESIDE a tracking launch instead of queueing behind its all-resident grid.
                                  0 (default): every place, the fastest epoch (a tracking-only load).  The split of a code period
                                  over a channel's workgroups follows the count: sums differ in the last bits between the two
                                  settings, inside the default mode's tolerance.  ABI version 6. */
} gm_trk_cfg;

typedef struct gm_trk gm_trk;

int gm_trk_create(const gm_trk_cfg *cfg, gm_trk **out);   /* TrackingManager::new :336-348 + Channel::new :118-146 */
int gm_trk_destroy(gm_trk *t);
/* TrackingChannel::start :148-154.  FIXED mode starts code_phase at 0 (sample_global_index is already the code
 * start) and restores the nominal code_rate after a reset(); FAITHFUL copies code_phase_chips like the reference. */
int gm_trk_start(gm_trk *t, uint32_t ch, const gm_acq_result *r);
int gm_trk_reset(gm_trk *t, uint32_t ch);                              /* ::reset :311-327 */
int gm_trk_get_state(gm_trk *t, uint32_t ch, gm_trk_state *out);
int gm_trk_set_state(gm_trk *t, uint32_t ch, const gm_trk_state *in);
/* All n_channels records in ONE synchronisation + ONE copy (ABI 7) — what a manager that mirrors the channels' pub fields
 * (TrackingManager.channels, do_tracking.rs:329-333) calls once per pass instead of 2 x n_channels single-channel calls.
 * which: NULL = every channel, else [n_channels] flags — only flagged channels are written (the others keep the device's words). */
int gm_trk_get_states(gm_trk *t, gm_trk_state *out);
int gm_trk_set_states(gm_trk *t, const gm_trk_state *in, const uint8_t *which);
/* get_ca_chip(phase) :274-277 for channel ch (host-side table look-up with the configured mode). */
int gm_trk_get_ca_chip(gm_trk *t, uint32_t ch, float phase, float *chip);
/* LoopFilter::new / ::update (:52-71), host-side scalars. */
int gm_loop_filter_new(float noise_bw, float damping, float gain, float *tau1, float *tau2);
float gm_loop_filter_update(float tau1, float tau2, float d_err, float err, float dt);

/* early_late_correlation() :231-272 for one channel on caller-supplied samples
 * (n must equal the channel's num_samples_per_code): advances carrier_phase / code_phase and sets
 * i_prompt/q_prompt exactly like the reference; no loop filters, no lock logic. */
int gm_trk_correlate(gm_trk *t, uint32_t ch, const gm_c32 *samples, size_t n, gm_trk_out *out);
/* do_work() :183-210 on caller-supplied samples (the reference's real-data test path, :734-739).
 * *lost = 1 <-> Some(TrackingMessage::SatelliteLost); *lost_prn = the prn the reference puts in the
 * message (0, because reset() runs first, :199-201). */
int gm_trk_do_work(gm_trk *t, uint32_t ch, const gm_c32 *samples, size_t n, gm_trk_out *out, uint8_t *lost,
                   uint8_t *lost_prn);
/* The batched equivalent of TrackingManager::process_channels' par_iter over active channels
 * (:364-371) repeated while data is available: up to `max_epochs` passes; in each pass every active
 * channel with head >= next_sample_index + num_samples_per_code runs update() :160-180 against the
 * device ring.  outs: [max_epochs][n_channels] (may be NULL); processed/lost: [max_epochs][n_channels]
 * flags (may be NULL).  *epochs_done = passes in which at least one channel ran. */
int gm_trk_update_all(gm_trk *t, gm_ring *ring, uint32_t max_epochs, gm_trk_out *outs, uint8_t *processed,
                      uint8_t *lost, uint32_t *epochs_done);
/* Asynchronous device-resident form for benchmarking: enqueues `epochs` passes, no host readback. */
int gm_trk_update_all_dev(gm_trk *t, gm_ring *ring, uint32_t epochs);
/* gm_trk_update_all without a host wait per block (ABI 6) — for a receiver loop that feeds block after block.  The reference's
 * tracking thread sleeps on the ring's Condvar until the head has passed what it needs (do_tracking.rs:392-406); here that wait
 * happens ON THE DEVICE: the passes are ordered behind everything the ring's asynchronous writer (gm_ring_write_samples_async /
 * gm_frontend_write_ring) has ENQUEUED so far, by an event on the ring's copy stream, and their data gate uses that enqueued
 * head — the host neither waits for the samples to land nor for the passes to run.  Results ([outs | processed | lost] as in
 * gm_trk_update_all) land in one of 8 pinned slots; *ticket (never 0) names the call.
 * gm_trk_collect(ticket, wait, ...): wait = 0 -> *ready = 0 and nothing else when the call has not finished; otherwise the results
 * are handed over (any of outs / processed / lost / states / epochs_done may be NULL), *ready = 1 and the slot is free again.
 * states (ABI 7): [n_channels] records as they stood when THIS call's passes had run (a snapshot taken on the device in stream
 * order, whatever has been enqueued behind it) — the pub fields a manager shows for that moment, without a synchronisation.  Tickets are
 * collected in any order; a call is refused (GM_ERR_OUT_OF_RANGE, nothing launched) while the ticket issued eight calls earlier —
 * whose slot it would take — has not been collected.  A collect that returns an ERROR (a HIP failure of the wait, an exchange
 * time-out reported by the kernel) has CONSUMED the ticket: its slot is free, its results are gone, a second collect of it is
 * GM_ERR_INVALID_ARG; wrappers drop their record of a ticket whenever the library returns an error for it.
 * Same channel states and sums as the synchronous entry, bit for bit (tests/test_gpu_pipeline.py). */
int gm_trk_update_all_async(gm_trk *t, gm_ring *ring, uint32_t max_epochs, uint64_t *ticket);
int gm_trk_collect(gm_trk *t, uint64_t ticket, int wait, gm_trk_out *outs, uint8_t *processed, uint8_t *lost, gm_trk_state *states,
                   uint32_t *epochs_done, int *ready);
int gm_trk_synchronize(gm_trk *t);
/* The handle's own stream is created at the device's HIGHEST priority: the tracking loop is the receiver's latency path (one short
 * launch per block of samples) and must not queue behind a front-end block or an acquisition dwell in flight on another stream.
 * gm_trk_set_stream replaces it with the caller's (whose priority is then the caller's choice). */
int gm_trk_set_stream(gm_trk *t, void *hip_stream);
/* Diagnostic (not in the reference): call with out == NULL to arm `cap` epochs of per-phase shader-clock stamps
 * of workgroup 0 in the persistent kernel, then with out = [cap][48] int64 after a launch to read them. */
int gm_trk_debug_stamps(gm_trk *t, uint32_t cap, long long *out);
int gm_trk_enable_timing(gm_trk *t, int on);
int gm_trk_last_timing(gm_trk *t, float *ms_correlate_total, uint32_t *launches);
/* Diagnostic (additive, ABI 9; not in the reference): the tracking loop's scalar device math, evaluated ON THE DEVICE for n caller-supplied
 * arguments, one per lane of 256-lane workgroups, by a kernel compiled with the tracking kernels (tests/test_gpu_device_math.py holds
 * the words against the host evaluation of csrc/gm_libm.h).  x, out0, out1: host arrays of n elements (n <= 2^24); results are raw
 * 32-bit words, 0 where an op has one result only.  p0 / p1 are uniform over the call; p2 is reserved.  RN(1/y) is formed on the host.
 *   op  out0 | out1                                                             parameters
 *    0  atanf_glibc(x)
 *    1  sincosf_glibc(x): sin | cos
 *    2  sincos_cw(x): sin | cos
 *    3  sincos_f32_via_f64(x): sin | cos
 *    4  div_const(x, y, RN(1/y)) | div_rn(x, y)                                 p0 = y
 *    5  fmod_bounded(x, y, RN(1/y))                                             p0 = y
 *    6  sqrt_rn(x)
 *    7  samples_per_code(fs, x, len) | samples_per_code(cfg, x), low 32 bits    p0 = fs, p1 = len
 *    8  spc_rate_bounds(fs, len, x): lo | hi                                    p0 = fs, p1 = len
 *    9  fmod_code<true>(x, len) | fmod_code<false>(x, len)                      p0 = len
 *   10  chip_index(x, len, FAITHFUL) | chip_index(x, len, FIXED)                p0 = len (an integer, 1..2^24)
 * GM_ERR_INVALID_ARG: a null array; GM_ERR_OUT_OF_RANGE: op, n, or a parameter an op reads that is not positive and finite;
 * GM_ERR_NO_DEVICE without a device. */
int gm_debug_math(int op, const float *x, size_t n, float p0, float p1, float p2, uint32_t *out0, uint32_t *out1);
/* Diagnostic (additive, ABI 9; not in the reference; a test entry): the four-step transform of length n1 * n2 with the factor pair NAMED,
 * in place on `batch` host arrays of n1 * n2 values: the column kernel of n1's plan on a grid of n2 workgroups, then the row kernel of
 * n2's plan on a grid of n1 — the code gm_fft_c2c_f32 runs for a power of two above 16384, which reaches only the pair its own rule
 * picks (N2 = 256 up to 2^22 points; a row plan of 2048 or more first at 2^25).  tests/test_gpu_fft_paths.py runs every column and
 * row kernel through it at 2^16 .. 2^22 points.  n1 < n2 is accepted.  dir: 0 forward, otherwise inverse (not normalised).
 * GM_ERR_INVALID_ARG: a null array or batch == 0; GM_ERR_UNSUPPORTED_N: a factor that is not one of the power-of-two in-LDS plans
 * (256 .. 16384), decided before the array is read; GM_ERR_OUT_OF_RANGE: n1 * n2 * batch above 2^31; GM_ERR_NO_DEVICE without a device. */
int gm_debug_fft_four_step(uint32_t n1, uint32_t n2, int dir, gm_c32 *inout, size_t batch);

/* ------------------------------------------------------------------ Correlator bank at tracked states (additive, ABI 9)
 * T taps x F carrier offsets of one code period at caller-supplied tracking states, formed with the tracker's own per-sample
 * arithmetic: the correlation function around the prompt (more points than E/P/L), the prompt at carrier offsets around the NCO, a
 * look at a state a receiver is only considering — without copying the epoch out of the ring and without starting a channel.
 *
 * A *record* is a gm_trk_state: a copy of one of the handle's channels (gm_trk_get_states) or anything the caller made up; it need
 * not belong to a channel.  For record r the epoch is n = round(fs / (code_rate / code_len)) samples, the samples_per_code the
 * tracker uses, starting at next_sample_index (ring form); in the linear form it is the num_samples_per_code samples the caller
 * hands in, as gm_trk_correlate takes them.  With T taps tau_t (chips, f32) and F carrier offsets df_f (Hz, f32):
 *
 *     f_f      = fl(carrier_freq + df_f)
 *     phase_i  = carrier_phase + fl(fl(fl(2 pi) * f_f) * i) / fs         the tracker's expression (do_tracking.rs:233) with f_f for carrier_freq
 *     y_f[i]   = x[i] * (cos phase_i, -sin phase_i)                      num-complex order, as correlate_sample forms it
 *     c[i]     = (code_phase + i * (code_rate / fs)) mod code_len        as correlate_sample forms it
 *     out[r][f][t] = sum_{i < n} y_f[i] * chip(fl(c[i] + tau_t))
 *
 * chip() is get_ca_chip's look-up in the handle's code_index_mode (FAITHFUL saturates a negative phase to chip 0, FIXED wraps); with
 * boc11 the sub-carrier sign comes from fract(phase) < 0.5, as the arms take it.  The chips are the +-1 of gm_trk_cfg.codes.  The
 * division by fs and the sine and cosine are the forms gm_trk_correlate's kernel uses (the exact fast forms where the epoch allows
 * them, the f64-reduced sine and cosine, glibc's on a strict_libm handle).  strict_sum_order is IGNORED: the bank always sums as a
 * tree — each lane its samples in order, then lanes, waves and slices of 4096 samples in a fixed order, no floating-point atomics;
 * the slice count is ceil(n / 4096), a function of n alone, so a record's words depend neither on what else is in the call nor on
 * repetition.  At df = 0 and tau = 0, +el, -el (and +-vel) the per-sample products are gm_trk_correlate's own; the sums agree with
 * it, and with the persistent kernel's prompt (whose sine and cosine differ on about 1e-5 of arguments), within the tracking
 * tolerance of 1e-5 of the envelope, not bit for bit.  NOTHING IS ADVANCED: no record is written, no channel state, loop filter or
 * lock counter moves.
 *
 * Limits, all checked before anything runs (gm_trk_bank_plan holds them; the device entries call the same code): a null cfg, a null
 * taps_chips, a null offsets_hz with n_offsets > 0, a null out or handle: GM_ERR_INVALID_ARG; a tap or offset that is not finite:
 * GM_ERR_INVALID_ARG; n_taps outside 1 .. 64, n_offsets above 8, n_offsets * n_taps above 256, n_states outside 1 .. 1024, a |tau_t|
 * above 64 or not below code_len / 2, a |df_f| above fs / 2, a custom code of more than 16384 chips (the chip row shares the
 * workgroup's LDS with the slice's samples): GM_ERR_OUT_OF_RANGE.  Taps need not be sorted or distinct.  A refusal leaves the
 * outputs untouched.
 * A record is SKIPPED — done[r] = 0, its words zeros, the call still succeeds — when active == 0; when its code row is outside
 * [0, n_codes); when n == 0 or n >= 2^31; ring form only: while the head has not passed next_sample_index + n (the tracker's own
 * gate), or when the epoch's first sample has already been overwritten (head - next_sample_index > ring size; the tracker has no such
 * test, the bank needs one because callers hand it old states). */
typedef struct {
    uint32_t n_taps, n_offsets;    /* T; F (0 with offsets_hz NULL: the single offset 0) */
    const float *taps_chips;       /* [n_taps] */
    const float *offsets_hz;       /* [n_offsets] or NULL */
    uint32_t reserved[4];          /* zeros */
} gm_trk_bank_cfg;
typedef struct {
    uint32_t n_taps, n_offsets;    /* T and the effective F */
    uint64_t out_words;            /* n_states * F * T gm_c32 words */
    uint64_t samples;              /* n for gm_trk_cfg.nominal_code_rate (0 -> 1.023e6) and code_len (no codes: 1023) */
    uint32_t slices;               /* ceil(n / 4096); 0 where a record with this n would be skipped */
    uint32_t tap_groups;           /* workgroups per slice: ceil(T / 16) */
} gm_trk_bank_plan_out;
/* host only, no device: the argument rules above, and the sizes of a call.  Of `trk` it reads fs, codes / code_len (the chips per
 * period) and nominal_code_rate (the code_rate n is reported for).  out may be NULL. */
int gm_trk_bank_plan(const gm_trk_cfg *trk, const gm_trk_bank_cfg *cfg, uint32_t n_states, gm_trk_bank_plan_out *out);
/* The ring form.  Synchronous, on the handle's stream, with gm_trk_update_all's ordering against the ring's writer and its head (the
 * published one).  states NULL: the handle's own channels as they stand, n_states = n_channels.  out: [n_states][F][T]; done:
 * [n_states] or NULL. */
int gm_trk_bank(gm_trk *t, gm_ring *ring, const gm_trk_state *states, uint32_t n_states, const gm_trk_bank_cfg *cfg, gm_c32 *out,
                uint8_t *done);
/* The linear form: one record on caller-supplied samples.  n must equal state->num_samples_per_code (and be in 1 .. 2^31 - 1), the
 * rule of gm_trk_correlate: GM_ERR_OUT_OF_RANGE otherwise, and for a code row outside the table.  Like gm_trk_correlate it runs
 * whatever `active` says.  out: [F][T]. */
int gm_trk_bank_samples(gm_trk *t, const gm_trk_state *state, const gm_c32 *samples, size_t n, const gm_trk_bank_cfg *cfg, gm_c32 *out);

/* ------------------------------------------------------------------ Per-antenna prompts at tracked states (additive, ABI 9)
 * The array form of gm_trk_bank: one code period of an INTERLEAVED antenna-array stream correlated with the tracker's replica at
 * caller-supplied tracking states, every antenna and every tap delay at once — the [L][A] words gm_array_row_solve takes, refreshed
 * from a tracked channel instead of from a new search (the first item the section "Beam rows from the array's own correlations" above
 * lists as not built).  The tracker's state goes in and [L][A] words come out; nothing is advanced.
 *
 * A record is a gm_trk_state, as for gm_trk_bank: a copy of a channel or anything the caller made up.  For record r:
 *   n = round(fs / (code_rate / code_len)).
 *   s = next_sample_index, a 64-bit TIME index.
 *   tau = cfg->tap_chips.
 *   x_a[t] is element (t - first_index) * A + a of an interleaved device buffer.  The buffer holds n_time time samples from absolute
 *   time first_index, in the layout gm_nuller, gm_stap, gm_beamformer and gm_acq_array_prompts take.
 *
 *     phase_i = carrier_phase + fl(fl(fl(2 pi) * carrier_freq) * i) / fs        gm_trk_bank's expression at df = 0
 *     c[i]    = (code_phase + i * (code_rate / fs)) mod code_len                as correlate_sample forms it
 *     ref[i]  = (cos phase_i, -sin phase_i) * chip(fl(c[i] + tau))              chip = +-1 (x BOC sign): an exact sign flip
 *     z[r][l][a] = sum_{i < n} x_a[s + i - l] * ref[i]                          l < L, a < A
 *
 * Helpers: chip(), the division by fs and the sine and cosine are the helpers gm_trk_bank uses (the exact fast forms where the epoch
 * allows them, the f64-reduced sine and cosine), with glibc's forms on a strict_libm handle.
 * Product: the complex product is four explicit fmaf, in the order gm_acq_array_prompts writes them:
 *     re = fma(xr, rr, re);  re = fma(-xi, ri, re);  im = fma(xr, ri, im);  im = fma(xi, rr, im)
 * THE ORDER, f32.  strict_sum_order is IGNORED.  The sum is a tree, a function of n and L alone.  Seen from the samples, time sample
 * u = i - l (u in [-(L-1), n)) meets ref[u .. u + L - 1].  The time samples are cut into ceil(n / 4096) slices: slice k holds u in
 * [4096 k, 4096 (k + 1)) below n, and slice 0 holds the L - 1 halo samples u < 0 as well.  Within a slice lane j of 256 takes, in this
 * order, the halo sample u = j - (L-1) (slice 0 and j < L - 1 only), then u = 4096 k + j + 256 m for m = 0 .. 15; for each time sample
 * it adds the taps l = 0 .. L-1 (a halo sample: l = -u .. L-1), one product above per tap, into its own sum per (l, a).  The 64 lanes of a wave add by
 * the butterfly v += v[lane xor d], d = 32, 16, 8, 4, 2, 1; the four waves add in ascending order ((w0 + w1) + w2) + w3; the slices
 * add in ascending order.  There are no floating-point atomics.  A record's words therefore do not depend on what else is in the call,
 * on repetition, or on where the buffer starts.
 * Agreement with gm_trk_bank: at L = 1, antenna a's word agrees with gm_trk_bank on the de-interleaved antenna (T = 1 tap tau, F = 1)
 * within the tracking tolerance of 1e-5 of the envelope.  It is NOT bit for bit: the bank rounds x * w (two products and a difference
 * per component) before the chip and sums in another order; this entry multiplies the sample by the finished ref word inside the fma.
 * NOTHING IS ADVANCED: no record is written and no channel state, loop filter or lock counter moves.
 *
 * Time samples and the halo: a time index below 0 reads as ZERO (gm_stap's halo), which can happen only when s < L - 1.  A record is
 * SKIPPED — done[r] = 0, its words zeros, the call succeeds — when active == 0; when its code row is outside the table; when n is 0 or
 * >= 2^31; when s + n > first_index + n_time; when max(0, s - (L-1)) < first_index, that is, part of its halo lies in front of the
 * buffer.  The library never reads outside [d_samples, d_samples + n_time * A elements).
 *
 * Formats: GM_FMT_C32 or GM_FMT_I8_IQ, aligned to the element only (8 or 2 bytes); int8 -128 is -128.0f.  GM_FMT_I8_REAL is refused.
 * Limits, all checked before anything runs (gm_trk_array_plan holds those of cfg and n_states; the device entry calls the same code):
 * a NULL handle, d_samples, cfg or z, a tap_chips that is not finite, a format other than the two above, a reserved word that is not
 * zero, states NULL with n_states != n_channels: GM_ERR_INVALID_ARG; n_antennas outside 2 .. 8, taps outside 1 .. 8, n_antennas * taps
 * above 32, n_states outside 1 .. 1024, |tap_chips| above 64 or not below code_len / 2, a custom code of more than 16384 chips (the chip
 * row shares the workgroup's LDS with the slice's ref image), first_index + n_time not below 2^62: GM_ERR_OUT_OF_RANGE.  A refusal
 * leaves z and done untouched.
 * Out of scope: a loop that re-steers by itself; propagating a state over several epochs inside the call; carrier offsets or several
 * code taps per call; an array ring; a _dev / caller's-stream form; any detection or quality decision.
 * (Since then the _dev / caller's-stream form has been built, and with it the update that needs no host wait: gm_trk_array_prompts_dev,
 * "Re-steering on the device" above.) */
typedef struct {
    uint32_t n_antennas, taps;     /* A, L */
    float tap_chips;               /* tau, chips */
    uint32_t reserved[5];          /* zeros */
} gm_trk_array_cfg;
typedef struct {
    uint32_t words_per_record;     /* L * A */
    uint64_t out_words;            /* n_states * L * A gm_c32 words */
    uint64_t samples;              /* n for gm_trk_cfg.nominal_code_rate (0 -> 1.023e6) and code_len (no codes: 1023) */
    uint32_t slices;               /* ceil(n / 4096); 0 where a record with this n would be skipped */
} gm_trk_array_plan_out;
/* host only, no device: the argument rules above, and the sizes of a call.  Of `trk` it reads fs, codes / code_len (the chips per
 * period) and nominal_code_rate (the code_rate n is reported for).  out may be NULL. */
int gm_trk_array_plan(const gm_trk_cfg *trk, const gm_trk_array_cfg *cfg, uint32_t n_states, gm_trk_array_plan_out *out);
/* Synchronous, on the handle's stream.  The caller HAS FINISHED WRITING d_samples before the call (the library orders nothing against
 * the buffer's writer).  states NULL: the handle's own channels as they stand, n_states = n_channels.  z: [n_states][L][A], host
 * memory, the word order gm_array_row_solve takes; done: [n_states] or NULL. */
int gm_trk_array_prompts(gm_trk *t, const void *d_samples, int fmt, uint64_t first_index, uint64_t n_time, const gm_trk_state *states,
                         uint32_t n_states, const gm_trk_array_cfg *cfg, gm_c32 *z, uint8_t *done);
/* The same words into device buffers, asynchronously on `stream` (NULL: the handle's own); the samples are ready on that stream.
 * "Re-steering on the device" above states the contract: states is required (host, read before the call returns), d_z and d_done are
 * required, d_z may not lie over the samples. */
int gm_trk_array_prompts_dev(gm_trk *t, const void *d_samples, int fmt, uint64_t first_index, uint64_t n_time,
                             const gm_trk_state *states, uint32_t n_states, const gm_trk_array_cfg *cfg,
                             void *d_z /* [n_states][L][A] c32, device */, void *d_done /* [n_states] u8, device */, void *stream);

/* ------------------------------------------------------------------ Plane ring (additive, ABI 9)
 * P rings of c32 on ONE time axis with ONE head, written from DEVICE memory: what a stage that ends in planes [P][out_stride]
 * leaves (gm_beamformer_process_dev and gm_lcmv_process_dev: one beam per plane; gm_channelizer_process_dev: one sub-band per plane) goes
 * into it with one launch, and "Tracking on planes" below reads it, channel c on plane planes[c].  Sample i of plane p is word
 * p * plane_size + (i & (plane_size - 1)) of one allocation [P][plane_size], zeroed at create.
 *
 * gm_plane_ring_plan (host only, no device) holds the rules of create: n_planes in 1 .. 64, plane_size a power of two (at least 1),
 * n_planes * plane_size * 8 at most 2^34 bytes: GM_ERR_OUT_OF_RANGE otherwise, *bytes (may be NULL) untouched; *bytes = the allocation.
 * gm_plane_ring_create waits for the fill before it returns, for gm_ring_create's reason (its writers work on non-blocking streams).
 *
 * gm_plane_ring_write_dev appends n samples to EVERY plane: plane p's come from d_planes + p * in_stride (c32 words), the layout and the
 * *n_out the three stage entries above leave.  One launch of the library's own copy kernel (the wrap is handled inside it; 16-byte
 * accesses when d_planes is 16-byte aligned and in_stride, n, the write position and plane_size are even, else 8-byte ones), on `stream`
 * (NULL: the ring's own non-blocking stream), NO host synchronisation.  n = 0: GM_OK, nothing launched.  Refused before anything runs,
 * the head and the ring untouched: a null ring or d_planes: GM_ERR_INVALID_ARG; n > plane_size, in_stride < n, a source range
 * [d_planes, d_planes + (n_planes - 1) * in_stride + n) that overlaps the ring: GM_ERR_OUT_OF_RANGE.
 * gm_plane_ring_write is the synchronous form from a host buffer of the same layout (same refusals but the overlap).
 * There is ONE head (gm_plane_ring_get_head): the samples per plane whose writes have been ENQUEUED, not those that have landed.
 * gm_plane_ring_copy_to_slice orders itself behind the enqueued writes, copies n samples of `plane` from absolute index start (across
 * the wrap too) and synchronises; it refuses what gm_ring_copy_to_slice refuses (a null pointer: GM_ERR_INVALID_ARG; n > plane_size:
 * GM_ERR_OUT_OF_RANGE) and plane >= n_planes (GM_ERR_OUT_OF_RANGE).  gm_plane_ring_synchronize waits for every write and every reader
 * the library has enqueued on the ring.
 *
 * ORDERING, all on the device; ONE writer (one host thread at a time calls the write entries).  Every write records an event behind
 * itself; when the writer's stream changes between calls the new stream first waits for that event; every reader the library launches
 * on the ring (the tracking launches below, gm_plane_ring_copy_to_slice) waits for that event and then uses the enqueued head; every
 * tracking launch records an event of its own on the ring (one per reader stream), and the next write waits for all of them — a write
 * that wraps can never land on samples an earlier tracking launch is still reading.  What the library does NOT order: the producer of
 * d_planes (run it on `stream`, or make `stream` wait for it), and readers of the caller's own. */
typedef struct gm_plane_ring gm_plane_ring;
int gm_plane_ring_plan(uint32_t n_planes, uint64_t plane_size, uint64_t *bytes);
int gm_plane_ring_create(uint32_t n_planes, uint64_t plane_size, gm_plane_ring **out);
int gm_plane_ring_destroy(gm_plane_ring *pr);
/* any output may be NULL; *d_base = the device address of plane 0 (plane p at d_base + p * plane_size words) */
int gm_plane_ring_info(gm_plane_ring *pr, uint32_t *n_planes, uint64_t *plane_size, uint64_t *bytes, void **d_base);
int gm_plane_ring_write_dev(gm_plane_ring *pr, const void *d_planes, size_t in_stride, size_t n, void *stream);
int gm_plane_ring_write(gm_plane_ring *pr, const gm_c32 *planes, size_t in_stride, size_t n);
int gm_plane_ring_get_head(gm_plane_ring *pr, uint64_t *head);
int gm_plane_ring_copy_to_slice(gm_plane_ring *pr, uint32_t plane, uint64_t start, gm_c32 *dest, size_t n);
int gm_plane_ring_synchronize(gm_plane_ring *pr);

/* ------------------------------------------------------------------ Tracking on planes (additive, ABI 9)
 * gm_trk_update_all on a plane ring: channel c runs update() (do_tracking.rs:160-180) against plane planes[c] of the ring — satellite p
 * tracked on beam p, a GLONASS satellite on its sub-band — without a copy through the host.  The contract of gm_trk_update_planes is
 * gm_trk_update_all's, argument for argument (outs / processed / lost: [max_epochs][n_channels], each may be NULL; *epochs_done = the
 * passes in which at least one channel ran); the data gate of every pass is (int64)(head - (next_sample_index + n)) >= 0 with
 * n = round(fs / (code_rate / code_len)) and head the plane ring's ENQUEUED head, behind whose writes the launch is ordered on the
 * device; the results land in one pinned area, with one synchronisation.  gm_trk_update_planes_dev enqueues the passes only.
 *
 * The map (gm_trk_set_channel_planes; planes NULL: every channel on plane 0, which is also a new handle's map) is handle state,
 * installed stream-ordered on the handle's stream; gm_trk_get_channel_planes returns it.  EVERY OTHER ENTRY IGNORES IT: gm_trk_update_all
 * and its kin run the persistent kernel on a gm_ring exactly as before, word for word.
 *
 * The kernel (csrc/trk_planes.hip): one 256-lane workgroup per channel, no communication between workgroups, no spin wait, no atomics.
 * It loads the channel's state and chip row once, then per pass takes the gate, forms every per-sample product with the code of
 * gm_trk_correlate (the f64-reduced sine and cosine, glibc's on a strict_libm handle; the exact fast forms of the division by fs and of the
 * code phase where the epoch allows them), sums as a FIXED TREE — lane j its samples j, j + 256, ... in ascending order, the 64 lanes of a
 * wave by the butterfly v += v[lane xor d], d = 32, 16, 8, 4, 2, 1, the four waves in ascending order ((w0 + w1) + w2) + w3 — runs the
 * scalar epilogue of gm_trk_do_work on one lane (lock test, atan PLL, envelope DLL, loop filters, loss of lock and reset), writes the
 * pass's outs / processed / lost and goes on with the state on chip; the state is stored once, after the last pass.  A channel that is
 * inactive, whose code row is outside the table, whose n is 0 or >= 2^31 or whose gate fails writes processed = 0 and zeros for that pass.
 * Like the tracker and UNLIKE gm_trk_bank it makes no "already overwritten" test: keep plane_size above the samples a channel may lag.
 * A channel's words are a function of its state and its plane's samples ALONE: not of the other channels, the map, the number of planes,
 * where in the ring the epoch lies, repetition, or how a run of E passes is cut into calls.  The sums agree with gm_trk_update_all's
 * (another tree) within the tracking tolerance of 1e-5 of the envelope, not bit for bit.
 * The launches join the device's chain of tracking launches as the strict_sum_order path does: they wait for the device's previous
 * tracking launch and record behind themselves, so a persistent grid of another handle finds all its places free.
 *
 * Refused before anything runs, state, outputs and head untouched (gm_trk_planes_plan holds the rules that need no handle; the device
 * entries call the same code): a null handle, ring or trk cfg: GM_ERR_INVALID_ARG; a ring on another device: GM_ERR_INVALID_ARG;
 * max_epochs 0: GM_ERR_INVALID_ARG (gm_trk_update_all's answer), above 4095: GM_ERR_OUT_OF_RANGE; n_planes outside 1 .. 64:
 * GM_ERR_OUT_OF_RANGE; a map entry at or above the ring's n_planes: GM_ERR_OUT_OF_RANGE, the message names the channel; a custom code of
 * more than 16384 chips: GM_ERR_OUT_OF_RANGE; a strict_sum_order handle: GM_ERR_INVALID_ARG — THE SEQUENTIAL-SUM PARITY PATH ON PLANES IS NOT
 * BUILT, and ignoring the switch would break that handle's bit-for-bit promise.  strict_libm, both code-index modes, boc11, three and
 * five arms and custom codes all work.
 * Out of scope: a ticketed (_async / collect) form; strict_sum_order; stage entries that write a plane ring by themselves; gm_trk_bank and
 * gm_trk_array_prompts on a plane ring; int8 planes; a loop that re-steers by itself. */
typedef struct {
    uint32_t workgroups;           /* one per channel: n_channels */
    uint32_t threads;              /* 256 */
    uint32_t chip_row_bytes;       /* the workgroup's dynamic LDS: code_len int8 chips (no codes: 1023) */
    uint32_t planes_used;          /* distinct planes the map names */
    uint64_t samples;              /* n for gm_trk_cfg.nominal_code_rate (0 -> 1.023e6) and code_len */
    uint32_t samples_per_lane;     /* ceil(n / 256); 0 where a channel with this n would not run */
    uint32_t reserved;             /* 0 */
    uint64_t result_bytes;         /* the call's device result block: max_epochs * n_channels * 43 bytes, rounded up to 4 */
} gm_trk_planes_plan_out;          /* 40 bytes */
/* host only, no device.  Of `trk` it reads fs, n_channels, n_arms, codes / n_codes / code_len, nominal_code_rate and strict_sum_order.
 * planes: [n_channels] or NULL (all 0).  out may be NULL; a refusal leaves it untouched. */
int gm_trk_planes_plan(const gm_trk_cfg *trk, uint32_t n_planes, const uint32_t *planes, uint32_t max_epochs, gm_trk_planes_plan_out *out);
int gm_trk_set_channel_planes(gm_trk *t, const uint32_t *planes /* [n_channels], NULL: all 0 */);
int gm_trk_get_channel_planes(gm_trk *t, uint32_t *planes /* [n_channels] */);
int gm_trk_update_planes(gm_trk *t, gm_plane_ring *pr, uint32_t max_epochs, gm_trk_out *outs, uint8_t *processed, uint8_t *lost,
                         uint32_t *epochs_done);
int gm_trk_update_planes_dev(gm_trk *t, gm_plane_ring *pr, uint32_t epochs);

/* ------------------------------------------------------------------ Bit sync + nav-bit accumulation
 * src/decoding.rs:8,40-227 (legacy file outside the reference's module tree): 20-bin histogram of prompt-I sign
 * changes (check_bit_sync :164-182, threshold 30), 20 ms accumulation into +-1 bits (bit_accumulation :184-214),
 * 8-bit preamble correlation (check_preamble_syn :216-227).  Host-side integer work, no device needed.
 * GM_NAV_FAITHFUL keeps the file's bugs (bits only emitted when frame_sync_ind == 0, :203-205; preamble tested only at
 * exactly 8 collected bits, :131-135); GM_NAV_FIXED wraps the bit boundary modulo 20 and slides the 8-bit window.
 * The subframe decoding of :147-160,229-257 panics as written (todo!(), indexing an empty Vec) and is not provided. */
enum { GM_NAV_FAITHFUL = 0, GM_NAV_FIXED = 1 };
typedef struct gm_nav_sync gm_nav_sync;
typedef struct {
    uint8_t flag_bit_sync, flag_frame_sync, sync_sw;   /* sync_sw: this epoch completed a bit */
    int8_t bit;                                        /* the completed bit (+1/-1), 0 otherwise */
    int8_t polarity;                                   /* preamble polarity (-1 until frame sync, like ::new :85) */
    uint32_t frame_sync_ind;                           /* ms offset of the bit edge */
    uint64_t n_frame_bits;
    float i_p;                                         /* running 20 ms accumulator */
    uint64_t sf_cnt, sf_start_biti, tow_expected_ind;
} gm_nav_status;
int gm_nav_sync_create(int mode, gm_nav_sync **out);                                       /* NavSyncStatus::new :68-100 */
int gm_nav_sync_destroy(gm_nav_sync *s);
/* nav_decoding's per-epoch step (:102-145) for epoch number `cnt` (1 ms each) with the channel's previous and current
 * prompt I (TrackingResult.old_i_prompt / i_prompt) */
int gm_nav_sync_update(gm_nav_sync *s, float old_i_prompt, float i_prompt, uint64_t cnt, uint64_t buff_loc,
                       gm_nav_status *out);
/* The same step for n consecutive epochs cnt0 .. cnt0 + n - 1 of one channel: i_prompt[k * stride] is epoch k's prompt I, the
 * previous one of epoch 0 is old_i_prompt0 (a caller that drives 15 channels x 1000 epochs per second through a foreign-function
 * boundary makes one call per channel and block instead of one per epoch).  *out = the status after the last epoch;
 * *first_bit_sync / *first_frame_sync (may be NULL) = the index k of the epoch at which the flag first became set in THIS call,
 * -1 if it did not.  n = 0: nothing happens, *out is left as it is. */
int gm_nav_sync_update_many(gm_nav_sync *s, float old_i_prompt0, const float *i_prompt, size_t stride, size_t n, uint64_t cnt0,
                            uint64_t buff_loc, gm_nav_status *out, int64_t *first_bit_sync, int64_t *first_frame_sync);
int gm_nav_sync_frame_bits(gm_nav_sync *s, int8_t *bits, size_t cap, size_t *n);
int gm_nav_sync_histogram(gm_nav_sync *s, uint64_t hist[20]);
/* parity_check (:259-352) on 32 symbols in +-1 form [D29*, D30*, d1..d24, D25..D30]: *ok = all six products match;
 * *ref_sum_zero (may be NULL) = the reference's own criterion, the i8 sum of the six differences is zero (:348-350) */
int gm_nav_parity_check(const int8_t bits[32], int *ok, int *ref_sum_zero);

#ifdef __cplusplus
}
#endif
#endif /* GNSS_MI355X_H */
