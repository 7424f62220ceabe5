// gm_internal.h — shared declarations between the kernel translation units and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gnss_mi355x.h"
#include "fft_core.h"
#include "trk_persist_plan.h"
#include "acq_corr_grid.h"

namespace gm {

// Fine Doppler (finer_doppler, acquisition_bk.rs:215-302): the zero-padded long FFT of the code-stripped
// snapshot as a four-step N1 x N2 transform built from two in-LDS plans; never materialised: the column pass reads the
// samples (strip + zero-pad fused), the row pass reduces |X|^2 to {max, first index} per row.
struct FineArgs {
    const void* samples; int fmt;          // the snapshot of the last search (M*N samples)
    const float* mean;                     // device {re, im}
    const int8_t* chips; uint32_t code_len; float code_rate, fs;   // [P][code_len]
    const uint32_t* sat_worker;            // [S] worker index of each satellite to refine
    const uint32_t* sat_code_phase;        // [S]
    uint32_t size_use, N1, N2;             // fft_size = N1 * N2
    cf* B;                                 // [S][N2][N1] intermediate (columns transformed, twiddled)
    const cf *tw1, *tw2;                   // forward base twiddles of plan N1 / plan N2
    float* rowmax; uint32_t* rowarg;       // [S][N1]
};

// gm_acq_cfg.coherent_periods: the most code periods one coherent group folds (gm_acq_create refuses more; stage F's LDS holds the phasors)
constexpr int GM_COHERENT_MAX = 32;

// Stage F of a coherent handle (gm_acq_cfg.coherent_periods = K >= 2), of its edge search (gm_acq_set_edge_search) and of a handle with
// code-drift compensation (gm_acq_set_code_drift): one argument block for the three families and the three forms
// (acq_stage_f_variants.h).  The dwell's M groups of K periods are folded with phasor words before the carrier mix; the output is laid
// out [H * n_bins][n_int][.], i.e. what stage C takes with H * n_bins bins.
//   coherent: group m is periods m K .. m K + K - 1 of N samples, rho is [n_bins][K] (gm_acq_coherent_phasors); H = 1, the rest null / 0
//   edge:     H hypotheses, each the coherent stage F on the samples from period offsets[h] on, the secondary row's signs in the fold
//   drift:    period k of group m of hypothesis h in bin d is the N samples from starts[d][offsets[h] + m K + k] on, rho is
//             [H][n_bins][n_int][K] (gm_acq_code_drift_phasors); offsets == null: one hypothesis at offset 0 (H = 1); K = 1: no fold
struct StageFArgs {
    const void* samples; int fmt;          // the dwell (coherent: K * M * N samples; edge: + offsets[H - 1] * N; drift: gm_acq_dwell_samples)
    const uint64_t* starts; uint32_t R;    // drift: device [n_bins][R] period starts (64-bit element offsets)
    const cf* rho; uint32_t K;             // device phasor words
    const uint32_t* offsets; uint32_t H;   // device [H], ascending period offsets
    uint32_t neg;                          // bit k set: secondary[k] = -1
    const cf* tables; const cf* tw_fwd;    // the Doppler tables [n_bins][N]; the forward plan's base twiddles
    cf* out;                               // in-LDS: the spectra; composite / long: the forward sub-transforms A
    uint32_t n_bins, n_int;                // the handle's own D and M: items = H * n_bins * n_int
    uint32_t Q, N, lim;                    // composite / long: Q; long: N and the signal's extension (N native, 2N padded)
    uint32_t* clear_tickets;               // in-LDS: the tail split's tickets, cleared on the way (PlanOps::mix_fft)
    const uint16_t* order;                 // in-LDS / composite: the storage order table (PlanOps::fill_order), may be null
};
// the launcher of a family (its loader: CohLoad, EdgeLoad, DriftLoad) for a form and its base plan length — in-LDS sizes: the size
// itself; composite and long: the base — or null: no such plan
typedef void (*StageFLaunch)(hipStream_t, const StageFArgs&);
enum { STAGE_F_MIX, STAGE_F_COMP, STAGE_F_LONG };
struct CohLoad; struct EdgeLoad; struct DriftLoad;
template <class Load> StageFLaunch find_stage_f(int form, int n);
// full [3][P][H][D] -> met [3][P][D] + choice [P][D] for the listed workers: per cell the hypothesis with the largest max, lowest h on ties
void launch_edge_reduce(hipStream_t, const uint32_t* full, uint32_t* met, uint32_t* choice, const uint32_t* worker_list,
                        uint32_t n_workers, uint32_t P, uint32_t H, uint32_t D);

// Fine Doppler from per-period prompts (gm_acq_refine_doppler, acq_refine.hip): the despreading kernel on grid (R_u, n_sats), then
// the scan over the Z grid points per satellite.  Nothing here depends on the handle's stage-C form.
struct RefineSat { uint32_t worker, code_phase, bin, offset; };   // offset: the periods the satellite's cell chose (0 without an edge search)
struct RefineArgs {
    const void* samples; int fmt;          // the snapshot of the last search
    const uint64_t* starts; uint32_t R;    // device [n_bins][R] period starts, or null: period p starts at p N
    const cf* tables;                      // the mix tables [n_bins][N]
    const int8_t* code_samples;            // the resampled replicas [P][N], natural order
    const RefineSat* sats; uint32_t n_sats;
    uint32_t N, R_u, J, G, Z;              // R_u = G * J prompts per satellite; Z grid points
    uint32_t neg;                          // bit k set: sigma_k = -1
    cf* z;                                 // [n_sats][R_u] prompts
    const double* t;                       // [n_sats][R_u] (s[o + g J + k] - s[o + g J]) / fs, seconds
    const double *fc, *step;               // [n_sats] table_freq of the bin; grid step in Hz
    float* spectrum;                       // [n_sats][Z]
    float* peak_val; uint32_t* peak_idx;   // [n_sats] first index of the maximum
};
void launch_refine(hipStream_t, const RefineArgs&);

// Lag window x fine Doppler at known cells (gm_acq_local_search, acq_local.hip): the despreading kernel on grid (R_u, n_cands) serves
// all W = 2L + 1 lags of a (period, candidate) from one pass over the samples, the scan runs on grid (W, n_cands), the pick per
// candidate.  A candidate is a RefineSat whose code_phase is the window's centre.
struct LocalPick {
    double floor_sum;                      // sum of S over all j of the n_floor rows at least `guard` lags from the peak
    float s0, s_jm, s_jp, s_lm, s_lp, s_c; // S at the peak, its neighbours along j and along l (0 past a rim), S[l*][(Z-1)/2]
    uint32_t l, j, n_floor;                // the first maximum in (l, j) order
};
struct LocalArgs {
    const void* samples; int fmt;          // the snapshot of the last search, or the caller's dwell
    const uint64_t* starts; uint32_t R;    // as RefineArgs
    const cf* tables;
    const int8_t* code_samples;
    const RefineSat* cands; uint32_t n_cands;
    uint32_t N, R_u, J, G, Z, L;           // L = lag_half_window (<= 64, 2L + 1 <= N)
    uint32_t neg, guard;                   // bit k set: sigma_k = -1; the floor's least circular distance in lags
    cf* z;                                 // [n_cands][W][R_u] prompts
    const double* t;                       // [n_cands][R_u]
    const double *fc, *step;               // [n_cands]
    float* surface;                        // [n_cands][W][Z]
    float* row_val; uint32_t* row_idx; double* row_sum;   // [n_cands][W] first maximum and sum of every row
    LocalPick* picks;                      // [n_cands]
};
void launch_local(hipStream_t, const LocalArgs&);

// Space-time prompts of an antenna array at known cells (gm_acq_array_prompts, acq_array.hip): one kernel on grid (R_u, n_cands), every
// time sample of [s - (L - 1), s + N) read once with its A words, against ref[n] = tab[d][n] c_w[(n - cp) mod N].  A candidate is a
// RefineSat.  gnss_mi355x.h states the definition and the summation order.
struct ArrayArgs {
    const void* samples; int fmt;          // the caller's interleaved dwell: time sample t, antenna a at element t A + a (c32 or int8 IQ)
    const uint64_t* starts; uint32_t R;    // as RefineArgs (in TIME samples)
    const cf* tables;
    const int8_t* code_samples;
    const RefineSat* cands; uint32_t n_cands;
    uint32_t N, R_u, A, L;                 // A in 2 .. 8, L in 1 .. 8, A L <= 32
    cf* z;                                 // [n_cands][R_u][L][A]
};
void launch_array(hipStream_t, const ArrayArgs&);

// Subtracting found satellites from a dwell (gm_acq_cancel, acq_cancel.hip): the amplitude kernel on grid (q_max, n_cands) sums one
// signal code period of one candidate per workgroup, the subtraction is one pass over the dwell.  The tables are [n_cands][stride],
// stride >= q_max + 1: o and b hold Q + 1 entries of a candidate, amps Q.
struct CancelCand {
    double cpl, fq;                        // L / T chips per sample; f / fs cycles per sample
    double cp, inv_T;                      // for the segment guess floor((n - cp) / T) - q0 only: the b table decides
    uint32_t worker, L, Q;                 // L = code_len
    int32_t q0;                            // -ceil(cp / T)
};
struct CancelArgs {
    const void* samples; int fmt;          // the snapshot of the last search, or the caller's dwell
    uint64_t D;                            // samples of the dwell
    const CancelCand* cands; uint32_t n_cands, q_max, stride;
    const double* o;                       // [n_cands][stride] segment origins o_k
    const uint64_t* b;                     // [n_cands][stride] segment bounds b_k (b_0 = 0, b_Q = D)
    const int8_t* chips;                   // [P][L] raw chips
    cf* amps;                              // [n_cands][stride]
    cf* out;                               // [D]; may be `samples` when fmt is c32
};
void launch_cancel(hipStream_t, const CancelArgs&);

// One entry per shipped transform size: launchers for the kernels instantiated on that plan.
struct DecideArgs;
struct PlanOps {
    int n;             // transform length
    int threads;       // workgroup size
    int tw_total;      // base-twiddle table entries (per direction)
    int lds_bytes;     // static LDS per workgroup of the correlation kernel
    int split_slab;    // floats of one partial power plane of the tail split (0: this plan cannot split)
    int code_paired;   // 1: corr() takes the code spectra in the paired layout (pair_codes), 0: in natural order
    void (*fill_tw)(cf* tw, bool inverse);
    // order[p] = the spectrum element index stored at position p of a stored spectrum, for sizes whose correlation plan reads its
    // input in a permuted order (prime-factor / hybrid plans); returns the table length (0: natural or merely paired order,
    // no table).  order == nullptr: just the length.
    int (*fill_order)(uint16_t* order);
    // stage F: carrier mix (apply_doppler_shift, doppler_shift.rs:25-58) fused into the forward FFT
    // (do_acquisition.rs:177-182).  One workgroup per (doppler bin, ms block); shared by all PRNs.
    // clear_tickets (may be null): the tail split's ticket counters, zeroed by the first workgroup for the corr() launch
    // that follows on the same stream (saves that launch its own hipMemsetAsync: ~8 us per dwell)
    // dec (may be null): a decision deferred by gm_acq_decide_dev — the PREVIOUS dwell's — runs as dec->n_prn trailing workgroups
    void (*mix_fft)(hipStream_t, const void* samples, int fmt, const cf* tables, const cf* tw_fwd,
                    cf* spectra, int n_bins, int n_int, uint32_t* clear_tickets, const uint16_t* order, const DecideArgs* dec);
    // stage C (spectra and code_fft in the PAIRED layout): x conj(code spectrum) -> inverse FFT -> |.|^2 accumulated over the integrations ->
    // {max, first argmax, sum} per (worker, bin)  (do_acquisition.rs:184-202, 229-235)
    void (*corr)(hipStream_t, const cf* spectra, const cf* code_fft, const cf* tw_inv, float* mmax,
                 uint32_t* margmax, float* msum, const uint32_t* worker_list, int n_workers, int n_bins,
                 int n_int, float* split_scratch, int split_planes, uint32_t* split_counter, int strict_sum, int tickets_cleared,
                 int ref_mul, gm_acq_corr_grid_info* rec);   // rec (may be null): the grid of this launch as decided (gm_acq_debug_corr_grid);   // ref_mul: gm_acq_cfg.reference_products;   // split_planes: power planes the scratch holds (<= GM_CORR_SPLIT_MAX_SLABS); tickets_cleared: mix_fft(.., split_counter) ran just before on this stream
    // AcquisitionWorker::new's replica spectrum (do_acquisition.rs:132-138)
    void (*code_fft)(hipStream_t, const int8_t* code_samples, const cf* tw_fwd, cf* code_fft, int n_codes);
    // the same spectra re-stored in the paired layout stage C reads (PairLayout in acq_kernels.hip); stage F writes its
    // spectra in that layout directly
    void (*pair_codes)(hipStream_t, const cf* natural, cf* paired, int n_codes);
    // FFT<T>::execute (fft.rs:21-25) on `batch` contiguous transforms
    void (*fft_batch)(hipStream_t, cf* data, const cf* tw, int inverse, int batch);
    // four-step long FFT passes (power-of-two plans only, else null): this plan as N1 (columns) / as N2 (rows)
    void (*fine_cols)(hipStream_t, const FineArgs&, int n_sats);
    void (*fine_rows)(hipStream_t, const FineArgs&, int n_sats);
    int fine_rows_per_wg;   // rows of the row pass one workgroup takes (its results: N1 / this per satellite)
    // long power-of-two FFT, four-step (power-of-two plans only, else null): columns x -> B[n2][k1] (twiddled), rows B -> X natural
    void (*big_cols)(hipStream_t, const cf* x, cf* B, const cf* tw, uint32_t n2, int inverse);
    void (*big_rows)(hipStream_t, const cf* B, cf* X, const cf* tw, uint32_t n1, int inverse);
    // stage F's forward transform may run on a plan of its own (MixPlanOf, acq_device.h): ITS base-twiddle table is what mix_fft takes
    int tw_total_mix;
    void (*fill_tw_mix)(cf* tw, bool inverse);
    // the inverse base-twiddle table of acq_corr_kernel, built for ITS plan (CorrPlanOf, acq_device.h: a plain plan of other radices
    // than the registered one since round 6, e.g. N = 8192; empty for prime-factor and hybrid correlation plans)
    int tw_total_corr;
    void (*fill_tw_corr)(cf* tw);
};
// mean of the snapshot (finer_doppler :236) and the final per-satellite reduction over the rows
void launch_fine_mean(hipStream_t, const void* samples, int fmt, uint32_t n, float* d_mean);
void launch_fine_final(hipStream_t, const float* rowmax, const uint32_t* rowarg, uint32_t n_rows, int n_sats,
                       float* peak_pow, uint32_t* peak_idx);
// tail split of the correlation grid: GM_CORR_SPLIT_MAX_K, GM_CORR_SPLIT_MAX_SLABS, GM_CORR_SPLIT_MAX_ITEMS and the whole decision
// (tile map, cut, grid; composite blocks; long slabs) are in acq_corr_grid.h (host-portable)
// Diagnostic overrides (item maps, tail split, workgroups per channel ...: tools/README.md).  The library reads NO environment
// variable unless the process was started with GM_DIAGNOSTICS=1: a receiver that links this library must not change kernels
// because its environment happens to carry a GM_* name.  diag_int returns `dflt` when diagnostics are off or `name` is unset.
int diag_int(const char* name, int dflt);
const PlanOps* find_plan(int n);
int list_plans(uint32_t* sizes, int cap);

// diagnostic: device buffer [n_int][8 waves][8 phases] of s_memtime stamps written by workgroup 0 of acq_corr_kernel
void set_corr_stamps(long long* d_ptr);
bool corr_stamps_built();          // false in the product library (the stamped kernels are compiled under -DGM_DIAG_STAMPS only)

// composite transform sizes N = Q * Nb (acq_composite.hip): decimated in time, the inverse fused with the power reduction
struct CompOps {
    int nb, q;         // base in-LDS plan length and the factor: N = q * nb
    // forward step 1: Q in-LDS transforms per item over the decimated inputs (signal: carrier mix fused; codes: int8 chips)
    // order (may be null): the base plan's PlanOps::fill_order table -> A leaves in storage order (permuted correlation plans)
    void (*fwd_sub)(hipStream_t, const void* samples, int fmt, const cf* tables, const int8_t* code_samples,
                    const cf* tw_fwd, cf* A, uint32_t n_items, uint32_t n_int, const uint16_t* order);
    // forward step 2: twiddle + Q-point DFTs -> natural block order; paired != 0 stores each block in the paired layout
    void (*fwd_post)(hipStream_t, const cf* A, cf* X, uint32_t n_items, int paired, const uint16_t* order);
    // inverse, fused: {max, first argmax, sum} per (worker, bin) straight from the spectra
    // planes (null normally; gm_acq_cfg.strict_sum_order): [n_workers_total * n_bins][N] floats — the kernel also stores every accumulated
    // power value at its natural index, for launch_plane_strict_sum
    void (*corr)(hipStream_t, const cf* spectra, const cf* code_paired, const cf* twn, const cf* tw_inv, float* mmax,
                 uint32_t* margmax, float* msum, const uint32_t* worker_list, int n_workers, int n_bins, int n_int, float* planes,
                 gm_acq_corr_grid_info* rec);   // rec (may be null): as PlanOps::corr
    void (*fill_twn)(cf* out);   // host: [q][nb] inverse twiddles W_N^{-n1 k2} in the paired position of k2
    // once per handle: comb[p][n1][k1][pos] = conj(code_paired[p][k1][pos]) * W_Q^{-n1 k1} * twn[n1][pos], the whole code-side
    // factor of sub-transform n1 (the codes are static, so corr multiplies a spectrum value by ONE table entry)
    void (*comb)(hipStream_t, const cf* code_paired, const cf* twn, cf* comb, uint32_t n_codes);
    // the stored order of a block of Nb spectrum elements on THIS path (its plan may differ from the fused kernels': CompPlanOf):
    // order table as PlanOps::fill_order, and natural -> stored re-layout of n_blocks blocks
    int (*fill_order)(uint16_t* order);
    void (*relayout)(hipStream_t, const cf* natural, cf* stored, int n_blocks);
    // base plans with an order table: forward step 2 folded into the table — comb2[p][n1][n1'][pos] such that a sub-transform's input is
    // sum_n1' A[n1'][pos] * comb2[n1][n1'][pos] on the forward sub-transforms A as fwd_sub leaves them (no fwd_post per dwell)
    void (*fold_post)(hipStream_t, const cf* comb, const uint16_t* order, cf* comb2, uint32_t n_codes);
};
const CompOps* find_comp(uint32_t n);
// strict_sum_order on the composite path: msum[o] = is_good_satellite's eight-lane ordered sum (do_acquisition.rs:229-235) of plane o,
// for the planes of the listed workers (o = worker * n_bins + bin)
void launch_plane_strict_sum(hipStream_t, const float* planes, float* msum, const uint32_t* worker_list, int n_workers, int n_bins, uint32_t N);

// any-length sizes (gm_acq_cfg.any_length, acq_long.hip): L = Q * nb with Q in [1, 32] at run time, native (L = N) or padded (L >= 2N)
struct LongOps {
    int nb;            // base in-LDS plan length
    // F1: Q in-LDS transforms of length nb per item over the decimated length-L inputs; element n < lim is sample n mod N (signal:
    // carrier mix fused; codes: int8 chips), the rest zero.  A[item][n1][k2], natural order
    void (*fwd_sub)(hipStream_t, const void* samples, int fmt, const cf* tables, const int8_t* code_samples, const cf* tw_fwd,
                    cf* A, uint32_t n_items, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int);
    // C2: items [item0, item0 + n_slab) of the bin-major (bin, worker) list, one workgroup per (item, n1) -> partials [item][n1]
    void (*corr_inv)(hipStream_t, const cf* Z, const cf* tw_inv, float* pmax, uint32_t* parg, float* psum, float* planes,
                     const uint32_t* worker_list, uint32_t n_workers, uint32_t n_bins, uint32_t item0, uint32_t n_slab, uint32_t Q,
                     uint32_t N, uint32_t n_int, float scale);
};
// the base plans, largest first
const LongOps* long_bases(int* n);
// F2: twiddle + Q-point DFT across n1, in place -> natural order (nothing for Q = 1)
void launch_long_fwd_post(hipStream_t, cf* X, uint32_t n_items, uint32_t Q, uint32_t Nb);
struct LongCorrArgs {
    const cf* spectra;                     // [n_bins][n_int][L] natural
    const cf* code_fft;                    // [codes][L] natural (not conjugated)
    const cf* tw_inv;                      // the base plan's inverse twiddles
    cf* Z;                                 // [slab_items][n_int][L]
    float *pmax, *psum; uint32_t* parg;    // partials [n_workers * n_bins][Q]
    float *mmax, *msum; uint32_t* margmax; // metric words, o = worker * n_bins + bin
    float* planes;                         // strict_sum_order: [codes * n_bins][N], else null
    const uint32_t* worker_list;
    uint32_t n_workers, n_bins, n_int, Q, Nb, N, slab_items;
    float scale;                           // (N / L)^2
};
// C1 + C2 per slab, then C3
void launch_long_corr(hipStream_t, const LongOps*, const LongCorrArgs&, gm_acq_corr_grid_info* rec = nullptr);   // rec: as PlanOps::corr

// elementwise apply_doppler_shift (doppler_shift.rs:25-58)
void launch_apply_doppler(hipStream_t, const cf* s, const cf* t, cf* out, size_t n);
// |X|^2 (fft.rs:27-29)
void launch_power(hipStream_t, const cf* x, float* p, size_t n);

// decision replay (do_acquisition.rs:195-225 + 229-238) from per-(worker,bin) metrics
struct DecideArgs {
    const float* mmax; const uint32_t* margmax; const float* msum;  // [n_prn][n_bins]
    const float* table_freq;                                        // [n_bins]
    const uint8_t* prn_ids;                                         // [n_prn]
    uint64_t mask_lo;                                               // worker i searched <-> bit i (i < 64), else all
    int n_prn, n_bins, fft_size;
    float fs, threshold, code_rate;
    int best_bin_mode;                                              // 0: reference early exit, 1: strongest bin
    uint64_t local_tail;
    gm_acq_result* results; uint8_t* found;                         // [n_prn]
};
void launch_decide(hipStream_t, const DecideArgs&);

// ---------------------------------------------------------------- tracking
// TrkDevCfg, fill_trk_derived and the persistent kernel's geometry and launch plan: trk_persist_plan.h (host-portable)
enum { TRK_MODE_CORRELATE = 0, TRK_MODE_DO_WORK = 1 };
// sample source: ring (mask = size-1, absolute index = next_sample_index + i) or linear (mask = ~0, base 0)
struct TrkSrc {
    const cf* base; uint64_t mask; uint64_t head; int linear;   // linear: index i directly, no head test
    int only_channel;                                           // >= 0: run just this channel (unit entries)
};
void launch_trk_epoch(hipStream_t, const TrkDevCfg&, const int8_t* d_codes, gm_trk_state* d_states,
                      const TrkSrc&, int slices, float* d_partials, uint8_t* d_ready, int mode,
                      gm_trk_out* d_outs, uint8_t* d_processed, uint8_t* d_lost, uint8_t* d_lost_prn,
                      float* d_terms = nullptr, size_t terms_cap = 0, int* d_error = nullptr);   // (strict_sum_order: per-sample product streams)

void launch_trk_results_to_host(hipStream_t, const void* d_src, void* h_dst_pinned, size_t bytes, const void* d_src2 = nullptr, void* h_dst2_pinned = nullptr,
                                size_t bytes2 = 0);
// gm_debug_math: one lane per argument through the tracking loop's scalar helpers (trk_kernels.hip); inv = RN(1 / divisor) of ops 4, 5, 7
void launch_trk_debug_math(hipStream_t, int op, const float* d_x, uint32_t n, float p0, float p1, float inv, uint32_t* d_out0, uint32_t* d_out1);
// What gm_trk_create asks the device about the instantiation(s) this configuration can launch: residency per CU (occupancy API with
// the config's dynamic LDS, capped at TRK_PERSIST_WG_PER_CU), the static LDS read from the code object (the larger where two
// instantiations are possible) and the most LDS the device gives a workgroup.
struct TrkPersistProbe { TrkPersistDevice dev; size_t static_lds, lds_limit; };
hipError_t trk_persist_probe(const TrkDevCfg&, const TrkPersistKnobs&, int device, TrkPersistProbe*);
// persistent multi-epoch tracking (one launch = `epochs` passes over all channels): what changes from call to call
struct TrkPersistCall {
    const int8_t* codes; gm_trk_state* states;
    const cf* ring; uint64_t mask, head;
    int epochs; uint32_t tag_base;
    unsigned long long* xchg;
    gm_trk_out* outs; uint8_t *processed, *lost, *lost_prn;
    int *error, *error_dev;
    long long* stamps; size_t stamps_words;      // diagnostic (may be null), and the words allocated behind it
};
void launch_trk_persistent(hipStream_t, const TrkDevCfg&, const TrkPersistPlan&, const TrkPersistCall&);

// gm_trk_bank / gm_trk_bank_samples (trk_bank.hip, a section of trk_kernels.hip): taps x carrier offsets at caller-supplied records.
// The host decides which records run (gnss_mi355x.h lists what skips one) and hands the kernel n, the slice count ceil(n / 4096) and
// the record's first partial; nothing of a record is written.
constexpr int GM_TRK_BANK_MAX_TAPS = 64, GM_TRK_BANK_MAX_OFFSETS = 8, GM_TRK_BANK_MAX_WORDS = 256, GM_TRK_BANK_MAX_STATES = 1024;
constexpr uint32_t GM_TRK_BANK_SLICE = 4096;
struct TrkBankRec { gm_trk_state st; uint32_t n, slices, poff, run; };   // poff: index of the record's first slice among the call's partials
struct TrkBankArgs {
    const TrkBankRec* recs;      // [n_records]
    const float* taps;           // [T] chips
    const float* offs;           // [F] Hz
    int T, F;
    const cf* base; uint64_t mask; int linear;      // the samples, as TrkSrc names them
    float* partials;             // [sum of slices][F][T] complex
};
int trk_bank_tap_group(int n_taps);     // taps per workgroup: the smallest of 1, 4, 8, 16 that holds min(T, 16)
void launch_trk_bank(hipStream_t, const TrkDevCfg&, const int8_t* d_codes, const TrkBankArgs&, int n_records, uint32_t max_slices,
                     gm_c32* d_out, uint8_t* d_done);

// gm_trk_array_prompts (trk_array.hip, a section of trk_kernels.hip): per-antenna, per-tap prompts of an interleaved array stream at
// caller-supplied records.  The host decides which records run (gnss_mi355x.h lists what skips one: among them any record whose time
// samples [max(0, s - (L-1)), s + n) do not lie inside the buffer) and hands the kernel n, the slice count ceil(n / 4096) and the
// record's first partial in a TrkBankRec; nothing of a record is written.
constexpr int GM_TRK_ARRAY_MIN_ANTENNAS = 2, GM_TRK_ARRAY_MAX_ANTENNAS = 8, GM_TRK_ARRAY_MAX_TAPS = 8, GM_TRK_ARRAY_MAX_WORDS = 32,
              GM_TRK_ARRAY_MAX_STATES = 1024;
constexpr uint32_t GM_TRK_ARRAY_SLICE = 4096;
struct TrkArrayArgs {
    const TrkBankRec* recs;      // [n_records]
    const void* samples;         // time sample first_index of the interleaved stream, fmt's elements
    uint64_t first_index;
    int fmt, A, L;               // GM_FMT_C32 or GM_FMT_I8_IQ
    float tau;                   // the code tap, chips
    cf* partials;                // [sum of slices][L][A]
};
void launch_trk_array(hipStream_t, const TrkDevCfg&, const int8_t* d_codes, const TrkArrayArgs&, int n_records, uint32_t max_slices,
                      gm_c32* d_z, uint8_t* d_done);

// gm_plane_ring_write_dev and gm_trk_update_planes (trk_planes.hip, a section of trk_kernels.hip).  The host has checked every limit
// (gm_plane_ring_plan, gm_trk_planes_plan, the map against the ring) and every pointer.
struct PlaneRingWriteArgs {
    const cf* src; cf* ring;                 // plane p: src + p * in_stride -> ring + p * plane_size
    uint64_t in_stride, plane_size;          // c32 words; plane_size a power of two
    uint64_t start, n;                       // the write position masked with plane_size - 1; samples per plane, <= plane_size
    uint32_t n_planes; int wide;             // wide: src 16-byte aligned and in_stride, n, start, plane_size even
};
void launch_plane_ring_write(hipStream_t, const PlaneRingWriteArgs&);
struct TrkPlanesArgs {
    TrkDevCfg cfg;
    const int8_t* codes; gm_trk_state* states;
    const uint32_t* map;                     // [n_channels] plane of channel c, each below n_planes
    const cf* ring; uint64_t plane_size, mask, head;   // [n_planes][plane_size]; mask = plane_size - 1; the enqueued head
    uint32_t n_planes; int epochs;
    gm_trk_out* outs; uint8_t *processed, *lost, *lost_prn;   // [epochs][n_channels] (may be null)
};
void launch_trk_planes(hipStream_t, const TrkPlanesArgs&);

// ---------------------------------------------------------------- digital front-end (fe_kernels.hip)
struct FeState { float phase_accumulator; float bias_re[8]; float bias_im[8]; };   // NcoLut.phase_accumulator, DcRemoverSimd.bias_*
struct FrontendArgs {
    struct Stream {
        const void* in;            // n_samples of c32 or int8 IQ (device)
        void* out;                 // c32 destination: linear buffer (out_mask = ~0) or ring base (out_mask = size-1)
        uint64_t out_start, out_mask;
        size_t n_samples;
        FeState* state;
        float phase_step;          // NcoLut.phase_step of this stream's front-end
        int fast_fmod;             // |phase_step| < 2048: fmodf reduces to one exact conditional add/subtract
        // tabulated NCO phase orbit (fast kernel; null: the sequential phase chain of frontend_kernel)
        const float* ph_table;     // |phase_accumulator| / 2048 before step k of the orbit that starts at phase 0
        uint32_t tab_len;          // entries: transient mu + period lambda' (lambda' = the period repeated to >= FE_FAST_SEG)
        uint32_t tab_lambda;       // lambda'
        uint32_t tab_pos;          // table index of this call's first sample (< tab_len)
        uint32_t tab_pos_end;      // table index after this call's last processed sample
        float tab_scale;           // +-2048: sign of phase_step
    };
    const Stream* streams;         // device array, one entry (and one workgroup) per stream
    Stream one;                    // used when streams == nullptr (single-stream launches need no upload)
    const float* lut;              // [2][2048]: lut_re, lut_im (nco_lut.rs:28-32), built on the host with glibc cosf/sinf
    float alpha, con;
    // speculative form (launch_frontend_spec): the block of `one` on spec_k workgroups; spec_buf = [spec_k][32] floats (the state run s
    // entered with / left with) + one word (repairs, diagnostic)
    int spec_k = 0, spec_poison = 0, spec_warm = 0;      // spec_warm: warm-up pipeline segments (0: the kernel's default, 18)
    float* spec_buf = nullptr;
    unsigned int* spec_repairs = nullptr;   // runs the walk has had to repeat (diagnostic counter)
};
void launch_frontend_spec(hipStream_t, const FrontendArgs&, int fmt);
void launch_frontend(hipStream_t, const FrontendArgs&, int n_streams, int fmt);
// every stream carries a phase table: the pipelined kernel (DC chains on one wave, everything else data-parallel)
void launch_frontend_fast(hipStream_t, const FrontendArgs&, int n_streams, int fmt);
constexpr int FE_SPEC_K_MAX = 64;     // most workgroups (runs) per block in the speculative form: the record block's size (32 are used)
constexpr int FE_FAST_SEG = 3840;      // samples per pipeline segment of the fast kernel: 480 chain steps = 120 quads x 8 SIMD
                                       // lanes = 960 stage-C items = one per helper lane (the table period is padded to >= this)

// ---------------------------------------------------------------- rate conversion and pulse blanking (resample_kernels.hip)
// gnss_mi355x.h states the definition.  One call = one launch of the output kernel (a workgroup per tile of `tile_out` outputs) and one
// of the state kernel (the next history, the blanked count).  The host hands over the call's first output index as m0 = a0 * up + mr0
// and the absolute index of the call's first input; the kernel forms every position from 64-bit integers.
constexpr int RS_SPAN_MAX = 4096;          // LDS samples of a tile's input span; tile_out is chosen so that the span fits (resample_tile_out)
constexpr int RS_TILE_MAX = 1024;          // 256 lanes x 4 outputs; a lane owns 4, 2 or 1 outputs (tiles of 1024, 512, <= 256)
struct ResampleArgs {
    const void* in; uint64_t n_in;         // this call's inputs (c32 or int8 IQ)
    const cf* hist_in; cf* hist_out;       // [T] the last T blanked inputs before / after this call (two buffers, used alternately)
    const float* table;                    // [PHI + 1][T]
    uint32_t T, PHI, up, down;
    uint64_t a0, mr0;                      // the call's first output: m0 = a0 * up + mr0, mr0 < up
    uint64_t in_index;                     // absolute index of in[0]
    uint64_t n_out; uint32_t tile_out;
    cf* out; uint64_t out_start, out_mask; // linear buffer (out_mask = ~0) or ring base
    float thr2; int blank;                 // blank_threshold^2 (f32 product); blanking on
    unsigned long long* blanked;           // device counter, integer atomics only
};
inline uint32_t resample_tile_out(uint32_t T, uint32_t up, uint32_t down) {
    const uint64_t n = uint64_t(RS_SPAN_MAX - int(T) - 1) * up / down + 1;      // the most outputs whose inputs span <= RS_SPAN_MAX samples
    return n >= 1024 ? 1024u : n >= 512 ? 512u : n >= 256 ? 256u : uint32_t(n);
}
void launch_resample(hipStream_t, const ResampleArgs&, int fmt);

// ---------------------------------------------------------------- real-IF down-conversion (ddc_kernels.hip)
// gnss_mi355x.h states the definition.  The rate converter's call shape (the same positions and tap loop; the fields they read carry
// ResampleArgs' names), with int8 real samples in, the history kept as T blanked BYTES, and the NCO:
// input n has phase (n * inc) mod 2^64, whose top 24 bits index the two phasor tables.
constexpr int DDC_TABLE = 4096;            // words of each phasor table
struct DdcArgs {
    const int8_t* in; uint64_t n_in;       // this call's inputs, one byte each, at any byte address
    const int8_t* hist_in; int8_t* hist_out;   // [T] the last T blanked inputs before / after this call (two buffers, used alternately)
    const float* table;                    // [PHI + 1][T]
    const cf *whi, *wlo;                   // [DDC_TABLE] each: exp(-j 2 pi h / 2^12), exp(-j 2 pi l / 2^24)
    uint32_t T, PHI, up, down;
    uint64_t a0, mr0;                      // the call's first output: m0 = a0 * up + mr0, mr0 < up
    uint64_t in_index;                     // absolute index of in[0]
    uint64_t inc;                          // floor(frac(mix_cycles_per_sample) * 2^64)
    uint64_t n_out; uint32_t tile_out;
    cf* out; uint64_t out_start, out_mask; // linear buffer (out_mask = ~0) or ring base
    float thr2; int blank;                 // blank_threshold^2 (f32 product); blanking on
    unsigned long long* blanked;           // device counter, integer atomics only
};
void launch_ddc(hipStream_t, const DdcArgs&);

// ---------------------------------------------------------------- polyphase filter bank (channelizer_kernels.hip)
// gnss_mi355x.h states the definition.  One call = one launch of the output kernel (a workgroup per tile of `tile_out` output times) and
// one of the state kernel (the next history, the blanked count).  The host hands over the absolute index m0 of the call's first output
// time and that of the call's first input; the kernel forms every position from 64-bit integers.
constexpr int CH_SPAN_MAX = 4096;          // LDS samples of a tile's input span; tile_out is chosen so that (tile_out - 1) D + L fits
constexpr int CH_M_MAX = 64;
struct ChannelizerArgs {
    const void* in; uint64_t n_in;         // this call's inputs (c32 or int8 IQ)
    const cf* hist_in; cf* hist_out;       // [L] the last L blanked inputs before / after this call (two buffers, used alternately)
    const float* taps;                     // [L] the prototype filter
    const cf* rot;                         // [M] exp(-j 2 pi e / M)
    uint32_t M, D, P, L;
    uint64_t m0;                           // absolute index of the call's first output time
    uint64_t in_index;                     // absolute index of the call's first input
    uint64_t n_out; uint32_t tile_out;     // output times of the call; per workgroup
    uint32_t pad_shift;                    // LDS word of sample i of a tile: i + (i >> pad_shift); >= 5
    cf* out; uint64_t out_stride;          // [C][out_stride]
    int8_t plane_of[CH_M_MAX];             // the plane of channel k, -1: not listed
    float thr2; int blank;                 // blank_threshold^2 (f32 product); blanking on
    unsigned long long* blanked;           // device counter, integer atomics only
};
inline uint32_t channelizer_tile_out(uint32_t L, uint32_t D) {
    const uint32_t n = (uint32_t(CH_SPAN_MAX) - L) / D + 1;      // the most output times whose inputs span <= CH_SPAN_MAX samples (L <= 2048)
    return n >= 1024 ? 1024u : n >= 512 ? 512u : n >= 256 ? 256u : n;
}
void launch_channelizer(hipStream_t, const ChannelizerArgs&, int fmt);

// ---------------------------------------------------------------- adaptive spatial nulling of an antenna array (nuller_kernels.hip)
// gnss_mi355x.h states the definition.  One call = one launch of the block kernel (a workgroup per finished block of B time samples:
// covariance, weights, output) and one of the state kernel (the time samples of the unfinished block, carried to the next call).  Time
// sample v of the call's span is word v of the old history for v < pending, else time sample v - pending of the call's input.
constexpr int NL_A_MAX = 8;
struct NullerArgs {
    const void* in; uint64_t n_in;         // this call's TIME samples, each A interleaved elements (c32 or int8 IQ)
    const cf* hist_in; cf* hist_out;       // [B][A] the converted time samples of the unfinished block before / after this call
    uint32_t A, B;
    uint32_t pending, pending_out;         // time samples in hist_in (< B); in hist_out after this call (< B)
    uint64_t n_blocks;                     // blocks this call finishes
    cf* out;                               // [n_blocks * B]
    cf* cap_R; cf* cap_w;                  // [n_blocks][A][A], [n_blocks][A]; null: not captured
    float loading;
    int adaptive;                          // 0: the fixed weights `w` for every block, no covariance pass
    int in_wide;                           // `in` is aligned for the widest load of a time sample (nuller_in_align)
    cf s[NL_A_MAX];                        // the steering vector
    cf w[NL_A_MAX];                        // the fixed weights
};
// the widest power-of-two load (bytes, at most 16) that divides a time sample of A elements
inline uint32_t nuller_in_align(uint32_t A, int fmt) {
    const uint32_t bytes = A * (fmt == GM_FMT_C32 ? 8u : 2u);
    return bytes % 16 == 0 ? 16u : bytes % 8 == 0 ? 8u : bytes % 4 == 0 ? 4u : 2u;
}
void launch_nuller(hipStream_t, const NullerArgs&, int fmt);

// ---------------------------------------------------------------- space-time adaptive nulling, taps on every antenna (stap_kernels.hip)
// gnss_mi355x.h states the definition.  One call = one launch of the block kernel (a workgroup per finished block of B time samples: Gram
// matrix, weights, output) and one of the state kernel.  The call's span starts H = L - 1 time samples in front of the unfinished block:
// time sample v of the span is word v of the old history for v < H + pending, else time sample v - (H + pending) of the call's input.
constexpr int ST_L_MAX = 8;
constexpr int ST_M_MAX = 32;               // A L at most
struct StapArgs {
    const void* in; uint64_t n_in;         // this call's TIME samples, each A interleaved elements (c32 or int8 IQ)
    int fmt;                               // GM_FMT_C32 or GM_FMT_I8_IQ
    const cf* hist_in; cf* hist_out;       // [L - 1 + B][A] the converted time samples in front of and in the unfinished block, before / after
    uint32_t A, L, B;
    uint32_t pending, pending_out;         // time samples of the unfinished block in hist_in (< B); in hist_out after this call (< B)
    uint64_t n_blocks;                     // blocks this call finishes
    cf* out;                               // [n_blocks * B]
    cf* cap_R; cf* cap_w;                  // [n_blocks][M][M], [n_blocks][M]; null: not captured
    float loading;
    int adaptive;                          // 0: the fixed weights `w` for every block, no Gram matrix
    unsigned long long* fallbacks;         // device counter of the blocks that took w = s / (s^H s): integer atomics only
    cf s[ST_M_MAX];                        // the constraint vector [L][A]
    cf w[ST_M_MAX];                        // the fixed weights
};
void launch_stap(hipStream_t, const StapArgs&);
void launch_stap_state(hipStream_t, const StapArgs&);      // the state kernel alone

// ---------------------------------------------------------------- one beam per constraint row from a shared Gram matrix (beam_kernels.hip)
// gnss_mi355x.h states the definition.  gm_stap's call with P constraint rows: one launch of the block kernel (a workgroup per finished
// block: ONE Gram matrix and ONE factor, then per beam a substitution and an output plane) and one of gm_stap's state kernel.  The span,
// the history and the counts are gm_stap's.  The rows and the static weights are too many words for the argument block: device memory.
constexpr int BM_P_MAX = 16;
struct BeamArgs {
    const void* in; uint64_t n_in;         // this call's TIME samples, each A interleaved elements (c32 or int8 IQ)
    int fmt;                               // GM_FMT_C32 or GM_FMT_I8_IQ
    const cf* hist_in; cf* hist_out;       // gm_stap's history, before / after
    uint32_t A, L, B, P;
    uint32_t pending, pending_out;
    uint64_t n_blocks;                     // blocks this call finishes
    cf* out; uint64_t out_stride;          // beam p's plane: out + p * out_stride, [n_blocks * B] words of it written
    cf* cap_R; cf* cap_w;                  // [n_blocks][M][M], [n_blocks][P][M]; null: not captured
    float loading;
    int adaptive;                          // 0: the fixed weights `w` for every block, no Gram matrix
    unsigned long long* fallbacks;         // [P] device counters of the blocks whose beam p took s_p / (s_p^H s_p): integer atomics only
    const cf* s;                           // device [P][M]: the constraint rows, each [L][A]
    const cf* w;                           // device [P][M]: the fixed weights
};
void launch_beam(hipStream_t, const BeamArgs&);

// ---------------------------------------------------------------- several constraints on one beam (lcmv_kernels.hip)
// gnss_mi355x.h states the definition.  gm_beamformer's call where beam p carries nq[p] constraint rows and responses in place of one
// row: the rows of all beams (at most LC_Q_SUM, beam p's from row q0[p]) ride below the matrix in the ONE factor; per beam a small Gram
// matrix, its factor and two substitutions.  The span, the history, the counts and the state kernel are gm_stap's.
constexpr int LC_Q_MAX = 8;                // constraint rows of one beam at most
constexpr int LC_Q_SUM = 16;               // constraint rows of all beams at most: the rows st_factor carries below the matrix
struct LcmvArgs {
    const void* in; uint64_t n_in;         // this call's TIME samples, each A interleaved elements (c32 or int8 IQ)
    int fmt;                               // GM_FMT_C32 or GM_FMT_I8_IQ
    const cf* hist_in; cf* hist_out;       // gm_stap's history, before / after
    uint32_t A, L, B, P;
    uint32_t pending, pending_out;
    uint64_t n_blocks;                     // blocks this call finishes
    cf* out; uint64_t out_stride;          // beam p's plane: out + p * out_stride, [n_blocks * B] words of it written
    cf* cap_R; cf* cap_w;                  // [n_blocks][M][M], [n_blocks][P][M]; null: not captured
    float loading;
    int adaptive;                          // 0: the fixed weights `w` for every block, no Gram matrix
    unsigned long long* fallbacks;         // [P] device counters of the blocks whose beam p took its quiescent weights: integer atomics only
    const cf* c;                           // device [q_sum][M]: the constraint rows, each [L][A], beam p's nq[p] rows from row q0[p]
    const cf* f;                           // device [q_sum]: the responses, in the rows' order
    const cf* w0;                          // device [P][M]: the quiescent weights C (C^H C)^-1 f, the host's f64 rounded once
    const cf* w;                           // device [P][M]: the fixed weights
    uint32_t q_sum, q_max;                 // sum and maximum of nq[0 .. P - 1]
    uint8_t nq[BM_P_MAX], q0[BM_P_MAX];
};
void launch_lcmv(hipStream_t, const LcmvArgs&);

// ---------------------------------------------------------------- re-steering on the device (array_solve.hip)
// gm_array_rows_solve_dev: gm_array_row_solve's nine steps for n_rows rows, f64, one workgroup a row; the host has checked every limit
// (gm_array_solve_plan) and every pointer.  Vector i of row p: the m words at z + p * row_stride + i * vec_stride.
struct ArraySolveArgs {
    const cf* z;
    const cf* R;                           // [n_blocks][m][m], only the upper triangles are read; null: the identity
    cf* rows;                              // [n_rows][m]
    void* info;                            // [n_rows] gm_array_row_info, the status in `reserved`
    uint64_t row_stride, vec_stride;       // c32 words
    uint32_t m, n, n_rows, n_blocks;
    double load;                           // the resolved loading
};
void launch_array_solve(hipStream_t, const ArraySolveArgs&);
// gm_beamformer_set_steering_dev: row p of `rows` into s[first_beam + p] where it is finite, not all zero and passes the gate
struct BeamInstallArgs {
    const cf* rows;                        // [n_rows][M]
    const void* info;                      // [n_rows] gm_array_row_info or null
    cf* s;                                 // the handle's constraint rows [P][M]
    uint8_t* installed;                    // [n_rows] or null
    uint32_t M, first_beam, n_rows;
    float min_ratio;
};
void launch_beam_install(hipStream_t, const BeamInstallArgs&);

// ---------------------------------------------------------------- narrowband interference excision (excise_kernels.hip)
// gnss_mi355x.h states the definition.  One call = one launch of the output kernel (a workgroup per tile of G segments of H = B / 2
// outputs) and one of the state kernel (the next history of 3H blanked inputs, the blanked count).  The host hands over where the
// call's first block starts relative to the call's first input (rel0 <= 0, >= -3H + 1: the history covers it).
constexpr int EX_BLOCK_MAX = 4096;         // the largest block length B
constexpr int EX_TW_MAX = 512;             // words of one base-twiddle set (272 at B = 4096)
constexpr int EX_BSTAT_SLOTS = 64, EX_BSTAT_STRIDE = 16;   // block-adapt counter rows of 128 bytes: a cache line each
constexpr uint32_t EX_CHUNKS_MAX = 512;    // most partial sums of the periodogram: chunk length C = max(4, ceil(J / 512)) blocks
struct ExciseArgs {
    const void* in; uint64_t n_in;         // this call's inputs (c32 or int8 IQ)
    const cf* hist_in; cf* hist_out;       // [3H] the last 3H blanked inputs before / after this call (two buffers, used alternately)
    const float *wa, *ws, *gains;          // [B] each
    const cf *tw_fwd, *tw_inv;             // base twiddles: the plan of B forward, the plan with its radices reversed inverse
    uint32_t B;
    int64_t rel0;                          // first input of the call's first block minus the call's first input
    uint32_t n_seg, G;                     // segments this call delivers; segments per workgroup (not in the words)
    cf* out; uint64_t out_start, out_mask; // linear buffer (out_mask = ~0) or ring base
    float thr2; int blank;                 // blank_threshold^2 (f32 product); blanking on
    unsigned long long* blanked;           // device counter, integer atomics only
    // block-adapt mode (launch_excise picks the block-adapt instantiation of excise_kernel when block_adapt is set)
    int block_adapt; float bfactor; uint32_t bguard;
    unsigned long long* bstat;             // [EX_BSTAT_SLOTS][EX_BSTAT_STRIDE], {blocks, blocks flagged, bins flagged, bins zeroed} first in a
                                           // row: device counters, integer atomics only; workgroup w adds to row w mod EX_BSTAT_SLOTS, the host sums the rows
    float* cap_p; unsigned char* cap_m;    // the capture: [n_seg + 1][B] power words / mask bytes of the call's blocks; either may be null
};
struct ExcisePsdArgs {
    const void* in;                        // the samples given, from their index 0
    const float* wa; const cf* tw_fwd;
    uint32_t B;
    uint64_t J; uint32_t C, n_chunks;      // blocks, blocks per chunk, chunks (= workgroups)
    float* partial;                        // [n_chunks][B]
    float thr2; int blank;
};
struct ExciseMaskArgs {
    const float* partial; uint32_t n_chunks, B;
    float factor; uint32_t guard;
    float* P; float* gains;                // [B] each
    uint32_t* stat;                        // {the median's word, bins flagged, bins zeroed}
};
inline uint32_t excise_tile_segments(uint32_t n_seg) {      // enough workgroups to fill the device on a 2^19-sample call, fewer repeated blocks on longer ones
    const uint32_t g = n_seg / 1024;
    return g < 1 ? 1u : (g > 8 ? 8u : g);
}
int excise_twiddles(uint32_t B, cf* fwd, cf* inv, int* n_fwd, int* n_inv);
void launch_excise(hipStream_t, const ExciseArgs&, int fmt);
void launch_excise_adapt(hipStream_t, const ExcisePsdArgs&, const ExciseMaskArgs&, int fmt);

}  // namespace gm
