// gnss_sdr.hpp — C++ host-side mirror of the reference crate's acquisition / tracking API over the C ABI
// (include/gnss_mi355x.h).  Header-only; link with libgnss_mi355x.so.  Type and method names follow the
// reference (file:line in the comments) so call sites port one to one; errors the reference turns into panics
// become gnss::Panic exceptions HERE (above the ABI — nothing unwinds across it).
#pragma once
#include <array>
#include <atomic>
#include <chrono>
#include <complex>
#include <algorithm>
#include <deque>
#include <functional>
#include <memory>
#include <map>
#include <mutex>
#include <thread>
#include <cstdint>
#include <cmath>
#include <limits>
#include <optional>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gnss_mi355x.h"

namespace gnss {

using Complex32 = std::complex<float>;   // num_complex::Complex32, layout-compatible with gm_c32

struct Panic : std::runtime_error {
    int status;
    Panic(int st, const std::string& where)
        : std::runtime_error(where + ": " + gm_status_string(st) + " (" + gm_last_error() + ")"), status(st) {}
};
inline void check(int st, const char* where) { if (st != GM_OK) throw Panic(st, where); }
inline void init(int device = 0) { check(gm_init(device), "gm_init"); }

// ---- utilities::ca_code (src/utilities/ca_code.rs:12-27)
inline std::vector<int8_t> generate_ca_code_samples(uint8_t prn, float code_rate, float f_sampling) {
    size_t n = 0;
    check(gm_generate_ca_code_samples(prn, code_rate, f_sampling, nullptr, 0, &n), "generate_ca_code_samples");
    std::vector<int8_t> v(n);
    check(gm_generate_ca_code_samples(prn, code_rate, f_sampling, v.data(), v.size(), &n), "generate_ca_code_samples");
    return v;
}

// ---- acquisition::doppler_shift (src/acquisition/doppler_shift.rs:5-58)
struct DopplerShiftTable {
    float doppler_freq_hz = 0.f;          // = f_if + doppler (:20)
    std::vector<Complex32> table;
    DopplerShiftTable(float f_if, float doppler_freq_hz_, float fs, size_t num_samples) : table(num_samples) {
        check(gm_doppler_table_new(f_if, doppler_freq_hz_, fs, num_samples, &doppler_freq_hz,
                                   reinterpret_cast<gm_c32*>(table.data())), "DopplerShiftTable::new");
    }
};
inline void apply_doppler_shift(const std::vector<Complex32>& samples, const DopplerShiftTable& t,
                                std::vector<Complex32>& output) {
    check(gm_apply_doppler_shift(reinterpret_cast<const gm_c32*>(samples.data()),
                                 reinterpret_cast<const gm_c32*>(t.table.data()),
                                 reinterpret_cast<gm_c32*>(output.data()), samples.size()), "apply_doppler_shift");
}

// ---- acquisition::do_acquisition (src/acquisition/do_acquisition.rs)
constexpr uint8_t PRN_SEARCH_ACQUISITION_TOTAL = 32;   // :22
using AcquisitionResult = gm_acq_result;                // :93-116 (+ doppler_bin)

enum class SearchMode { ColdStart = 0, WarmStart = 1, SteadyState = 2 };   // :33-37
class AcquisitionManager {                                                 // :39-74
    SearchMode mode_ = SearchMode::ColdStart;
public:
    SearchMode mode() const { return mode_; }
    void update_mode(size_t trked_acount) { mode_ = SearchMode(gm_acq_manager_mode_for(trked_acount)); }
    std::pair<uint64_t, uint32_t> get_pacing_and_list(const std::set<uint8_t>& active_prns) const {
        uint32_t am = 0;
        for (uint8_t p : active_prns) am |= 1u << (p - 1);
        uint64_t iv = 0; uint32_t mask = 0;
        check(gm_acq_manager_pacing_and_list(int(mode_), am, &iv, &mask), "get_pacing_and_list");
        return {iv, mask};
    }
};

// All workers of one acquisition stage in one handle: the batched replacement of
// `workers.par_iter_mut()...search_satellite(...)` (:268-271, :302-313).
class AcquisitionEngine {
    gm_acq* h_ = nullptr;
    uint32_t n_prn_ = 0, coherent_periods_ = 1, n_integrations_ = 0;     // (what gm_acq_array_plan sizes array_prompts' words from)
public:
    AcquisitionEngine(float fs, float f_if, uint32_t fft_size, const std::vector<float>& doppler_hz,
                      const std::vector<uint8_t>& prn_ids, uint32_t n_integrations = 10, float threshold = 7.0f,
                      int decision_mode = GM_DECIDE_REFERENCE, bool any_length = false, uint32_t coherent_periods = 1) {
        gm_acq_cfg c{};
        c.decision_mode = decision_mode;
        c.any_length = any_length ? 1 : 0;      // every fft_size % 8 == 0 in [1024, 2^18] (gm_acq_cfg.any_length)
        c.coherent_periods = coherent_periods;  // K periods folded coherently: a dwell is K * n_integrations periods (gm_acq_cfg.coherent_periods)
        c.fs = fs; c.f_if = f_if; c.fft_size = fft_size; c.n_integrations = n_integrations;
        c.n_bins = uint32_t(doppler_hz.size()); c.doppler_hz = doppler_hz.data();
        c.n_prn = uint32_t(prn_ids.size()); c.prn_ids = prn_ids.data(); c.threshold = threshold;
        n_prn_ = c.n_prn; coherent_periods_ = c.coherent_periods; n_integrations_ = c.n_integrations;
        check(gm_acq_create(&c, &h_), "AcquisitionEngine::new");
    }
    // caller-built tables, as search_satellite receives them (:160-161)
    AcquisitionEngine(float fs, uint32_t fft_size, const std::vector<DopplerShiftTable>& tables,
                      const std::vector<uint8_t>& prn_ids, uint32_t n_integrations, bool any_length = false) {
        std::vector<gm_c32> flat(tables.size() * size_t(fft_size));
        std::vector<float> freq(tables.size());
        for (size_t d = 0; d < tables.size(); ++d) {
            if (tables[d].table.size() < fft_size) throw Panic(GM_ERR_OUT_OF_RANGE, "DopplerShiftTable shorter than fft_size");
            for (uint32_t i = 0; i < fft_size; ++i) flat[d * fft_size + i] = {tables[d].table[i].real(), tables[d].table[i].imag()};
            freq[d] = tables[d].doppler_freq_hz;
        }
        gm_acq_cfg c{};
        c.fs = fs; c.fft_size = fft_size; c.n_integrations = n_integrations; c.n_bins = uint32_t(tables.size());
        c.tables = flat.data(); c.table_freq = freq.data(); c.n_prn = uint32_t(prn_ids.size()); c.prn_ids = prn_ids.data();
        c.any_length = any_length ? 1 : 0;
        n_prn_ = c.n_prn; coherent_periods_ = c.coherent_periods; n_integrations_ = c.n_integrations;
        check(gm_acq_create(&c, &h_), "AcquisitionEngine::new");
    }
    ~AcquisitionEngine() { gm_acq_destroy(h_); }
    AcquisitionEngine(const AcquisitionEngine&) = delete;
    AcquisitionEngine& operator=(const AcquisitionEngine&) = delete;
    gm_acq* handle() const { return h_; }

    std::vector<std::optional<AcquisitionResult>> search(const std::vector<Complex32>& samples_chunk, uint64_t local_tail,
                                                         uint64_t prn_mask = ~0ull) {
        std::vector<gm_acq_result> r(n_prn_);
        std::vector<uint8_t> f(n_prn_);
        check(gm_acq_search_c32(h_, reinterpret_cast<const gm_c32*>(samples_chunk.data()), samples_chunk.size(), local_tail,
                                prn_mask, r.data(), f.data()), "search_satellite");
        std::vector<std::optional<AcquisitionResult>> out(n_prn_);
        for (uint32_t i = 0; i < n_prn_; ++i) if (f[i]) out[i] = r[i];
        return out;
    }
    // run()'s snapshot + fan-out against the device ring (:297-313); nullopt while head < M*N (:299)
    std::optional<std::vector<std::optional<AcquisitionResult>>> search_ring(gm_ring* ring, uint64_t prn_mask = ~0ull,
                                                                             uint64_t* local_tail = nullptr) {
        std::vector<gm_acq_result> r(n_prn_);
        std::vector<uint8_t> f(n_prn_);
        const int st = gm_acq_search_ring(h_, ring, prn_mask, r.data(), f.data(), local_tail);
        if (st == GM_ERR_OUT_OF_RANGE) return std::nullopt;
        check(st, "search_ring");
        std::vector<std::optional<AcquisitionResult>> out(n_prn_);
        for (uint32_t i = 0; i < n_prn_; ++i) if (f[i]) out[i] = r[i];
        return out;
    }
    // finer_doppler (acquisition_bk.rs:215-302) on the snapshot of the last search: refined carrier (IF + Doppler) of
    // every found result, to a fraction of the coarse bin; entries of not-found workers are left as NaN
    std::vector<float> finer_doppler(const std::vector<std::optional<AcquisitionResult>>& results) {
        std::vector<gm_acq_result> r(results.size());
        std::vector<uint8_t> f(results.size(), 0);
        for (size_t i = 0; i < results.size(); ++i) if (results[i]) { r[i] = *results[i]; f[i] = 1; }
        std::vector<float> freq(results.size(), std::numeric_limits<float>::quiet_NaN());
        check(gm_acq_finer_doppler(h_, r.data(), f.data(), uint32_t(results.size()), freq.data(), nullptr, nullptr, nullptr),
              "finer_doppler");
        return freq;
    }
    // Fine Doppler from per-period prompts (gm_acq_refine_doppler) on the snapshot of the last search: the search's own statistic on a
    // fine grid around every found result's bin — valid with coherent groups, the edge search and the code drift, where finer_doppler
    // is not.  cfg zeros are the defaults.  Entries of not-found workers are nullopt; carrier_hz is the refined IF + Doppler.
    std::vector<std::optional<gm_acq_refine_out>> refine_doppler(const std::vector<std::optional<AcquisitionResult>>& results,
                                                                 const gm_acq_refine_cfg& cfg = {}) {
        std::vector<gm_acq_result> r(results.size());
        std::vector<uint8_t> f(results.size(), 0);
        for (size_t i = 0; i < results.size(); ++i) if (results[i]) { r[i] = *results[i]; f[i] = 1; }
        std::vector<gm_acq_refine_out> o(results.size());
        check(gm_acq_refine_doppler(h_, r.data(), f.data(), uint32_t(results.size()), &cfg, o.data(), nullptr, nullptr), "refine_doppler");
        std::vector<std::optional<gm_acq_refine_out>> out(results.size());
        for (size_t i = 0; i < results.size(); ++i) if (f[i]) out[i] = o[i];
        return out;
    }
    // Lag window x fine Doppler at known cells (gm_acq_local_search): refine_doppler's statistic on 2 * cfg.lag_half_window + 1 code
    // phases around every candidate's, from one pass over the samples — on the snapshot of the last search (d_samples null) or on any
    // dwell of dwell_samples() samples in device memory (read only; it does not become the snapshot).  No detection decision is made.
    std::vector<gm_acq_local_out> local_search(const std::vector<gm_acq_cand>& cands, const gm_acq_local_cfg& cfg = {},
                                               const void* d_samples = nullptr, int fmt = GM_FMT_C32) {
        const gm_acq_cand spare{};              // an empty list still hands over pointers: the library refuses null ones before it looks at the count
        std::vector<gm_acq_local_out> out(std::max<size_t>(cands.size(), 1));
        check(gm_acq_local_search(h_, d_samples, fmt, cands.empty() ? &spare : cands.data(), uint32_t(cands.size()), &cfg, out.data(), nullptr, nullptr), "local_search");
        out.resize(cands.size());
        return out;
    }
    // Space-time prompts of an antenna array at known cells (gm_acq_array_prompts): every antenna and tap delay of the interleaved
    // stream at d_samples (dwell_samples() TIME samples of n_antennas elements, read only) against each candidate's replica ->
    // [cands][R_u][taps][n_antennas] words, R_u from gm_acq_array_plan.  solve_row turns a candidate's words into a constraint row.
    std::vector<gm_c32> array_prompts(const std::vector<gm_acq_cand>& cands, const void* d_samples, uint32_t n_antennas, uint32_t taps = 1,
                                      int fmt = GM_FMT_C32, uint32_t* periods = nullptr) {
        uint32_t r = 0, words = 0;
        check(gm_acq_array_plan(coherent_periods_, n_integrations_, n_antennas, taps, &r, &words), "array_plan");
        std::vector<gm_c32> z(std::max<size_t>(cands.size(), 1) * words);
        const gm_acq_cand spare{};              // (as in local_search: no candidates is not a null pointer)
        check(gm_acq_array_prompts(h_, d_samples, fmt, n_antennas, taps, cands.empty() ? &spare : cands.data(), uint32_t(cands.size()), z.data()), "array_prompts");
        z.resize(cands.size() * words);
        if (periods) *periods = r;
        return z;
    }
    // Subtracting found satellites from a dwell (gm_acq_cancel): one amplitude per signal code period and candidate is estimated from
    // the input (the snapshot of the last search when d_samples is null, else any dwell of dwell_samples() samples, read only) and
    // the dwell minus the replicas is written as c32 to d_out, which every search entry takes as a dwell (d_out may be the c32 input
    // itself).  Candidates carry local_search's carrier_hz and code_phase_fine and the signal's true code period.  No detection
    // decision is made.
    std::vector<gm_acq_cancel_out> cancel(const std::vector<gm_acq_cancel_cand>& cands, void* d_out, const void* d_samples = nullptr,
                                          int fmt = GM_FMT_C32) {
        std::vector<gm_acq_cancel_out> out(cands.size());
        check(gm_acq_cancel(h_, d_samples, fmt, cands.data(), uint32_t(cands.size()), d_out, out.data(), nullptr, 0), "cancel");
        return out;
    }
    // The edge search of a coherent handle (gm_acq_set_edge_search): H ascending period offsets (each 0..63, H <= 32) and an optional
    // secondary row of coherent_periods entries +-1 (empty: all +1); no offsets switch it off.  While it is on a dwell is
    // (K * n_integrations + offsets.back()) * fft_size samples.
    void set_edge_search(const std::vector<uint32_t>& offsets, const std::vector<int8_t>& secondary = {}) {
        check(gm_acq_set_edge_search(h_, uint32_t(offsets.size()), offsets.empty() ? nullptr : offsets.data(),
                                     secondary.empty() ? nullptr : secondary.data()), "set_edge_search");
    }
    // Code-drift compensation (gm_acq_set_code_drift): the true code period in samples per Doppler bin (each within 8 of fft_size); period
    // p of the dwell then starts at floor(p * T_d + 0.5) in bin d and a dwell is dwell_samples() long.  An empty vector switches it off.
    void set_code_drift(const std::vector<double>& period_samples) {
        check(gm_acq_set_code_drift(h_, uint32_t(period_samples.size()), period_samples.empty() ? nullptr : period_samples.data()), "set_code_drift");
    }
    // samples one dwell takes now, given coherent_periods, n_integrations, the edge search and the code drift (gm_acq_dwell_samples)
    uint64_t dwell_samples() {
        uint64_t n = 0;
        check(gm_acq_dwell_samples(h_, &n), "dwell_samples");
        return n;
    }
    // for every found result of the last search the offset, in periods, of the hypothesis its winning bin chose (others: 0)
    std::vector<uint32_t> edge_offset_periods(const std::vector<std::optional<AcquisitionResult>>& results) {
        std::vector<gm_acq_result> r(results.size());
        std::vector<uint8_t> f(results.size(), 0);
        for (size_t i = 0; i < results.size(); ++i) if (results[i]) { r[i] = *results[i]; f[i] = 1; }
        std::vector<uint32_t> off(results.size(), 0u);
        check(gm_acq_result_offsets(h_, r.data(), f.data(), uint32_t(results.size()), off.data()), "edge_offset_periods");
        return off;
    }
    std::vector<std::optional<AcquisitionResult>> search_i8(const std::vector<int8_t>& iq_interleaved, uint64_t local_tail,
                                                            uint64_t prn_mask = ~0ull) {
        std::vector<gm_acq_result> r(n_prn_);
        std::vector<uint8_t> f(n_prn_);
        check(gm_acq_search_i8(h_, iq_interleaved.data(), iq_interleaved.size() / 2, local_tail, prn_mask, r.data(), f.data()),
              "search_satellite");
        std::vector<std::optional<AcquisitionResult>> out(n_prn_);
        for (uint32_t i = 0; i < n_prn_; ++i) if (f[i]) out[i] = r[i];
        return out;
    }
};

// A constraint row from one cell's prompt vectors (gm_array_row_solve, host only): z is [n][m] (a candidate's words of
// AcquisitionEngine::array_prompts: n = R_u, m = taps * n_antennas), R the captured Gram blocks [n_blocks][m][m] of a Stap or a
// Beamformer (empty: the identity), loading 0 -> 1e-4.  -> the row [m]; info->lambda1 / info->lambda2 is the estimate's quality, which
// the caller judges.
inline std::vector<gm_c32> solve_row(uint32_t m, const std::vector<gm_c32>& z, const std::vector<gm_c32>& R = {}, float loading = 0.0f,
                                     gm_array_row_info* info = nullptr) {
    std::vector<gm_c32> row(m);
    gm_array_row_info local{};
    check(gm_array_row_solve(m, m ? uint32_t(z.size() / m) : 0u, z.data(), R.empty() ? nullptr : R.data(),
                             m ? R.size() / (size_t(m) * m) : 0, loading, row.data(), info ? info : &local), "solve_row");
    return row;
}

// Re-steering on the device.  solve_plan (gm_array_solve_plan, host only): the argument rules of solve_rows_dev and the c32 words it
// reads at d_z and d_R and writes at d_rows.  solve_rows_dev (gm_array_rows_solve_dev): solve_row for cfg.n_rows rows in one launch,
// asynchronous on `stream` (null: the null stream); vector i of row p at d_z + p * row_stride + i * vec_stride words (0, 0: the dense
// [n_rows][n][m]); d_R null with n_blocks = 0: the identity; d_info[p].reserved is row p's status, 0: solved.
struct SolveExtents { uint64_t z_words, R_words, row_words; };
inline SolveExtents solve_plan(const gm_array_solve_cfg& cfg) {
    SolveExtents e{};
    check(gm_array_solve_plan(&cfg, &e.z_words, &e.R_words, &e.row_words), "solve_plan");
    return e;
}
inline void solve_rows_dev(const gm_array_solve_cfg& cfg, const void* d_z, const void* d_R, void* d_rows, void* d_info, void* stream = nullptr) {
    check(gm_array_rows_solve_dev(&cfg, d_z, d_R, d_rows, d_info, stream), "solve_rows_dev");
}

// AcquisitionWorker::new(prn, fft_size, freq_sampling_hz) / search_satellite (:130-226): one PRN per object.
class AcquisitionWorker {
    uint8_t prn_; uint32_t fft_size_; float fs_;
    std::unique_ptr<AcquisitionEngine> eng_;
    const void* key_ = nullptr; size_t key_n_ = 0, key_m_ = 0;
public:
    AcquisitionWorker(uint8_t prn, size_t fft_size, float freq_sampling_hz) : prn_(prn), fft_size_(uint32_t(fft_size)), fs_(freq_sampling_hz) {
        if (prn < 1 || prn > 32) throw Panic(GM_ERR_OUT_OF_RANGE, "GPS_CA_CODE_32_PRN[prn - 1]");
    }
    std::optional<AcquisitionResult> search_satellite(const std::vector<Complex32>& samples_chunk,
                                                      const std::vector<DopplerShiftTable>& doppler_table, size_t local_tail,
                                                      size_t num_integrations) {
        if (!eng_ || key_ != doppler_table.data() || key_n_ != doppler_table.size() || key_m_ != num_integrations) {
            // any_length: the reference plans an FFT of whatever fft_size is (:130-143)
            eng_ = std::make_unique<AcquisitionEngine>(fs_, fft_size_, doppler_table, std::vector<uint8_t>{prn_}, uint32_t(num_integrations), true);
            key_ = doppler_table.data(); key_n_ = doppler_table.size(); key_m_ = num_integrations;
        }
        return eng_->search(samples_chunk, local_tail)[0];
    }
};

// ---- utilities::multicast_ring_buffer (device mirror, :36-130)
class MulticastRingBuffer {
    gm_ring* h_ = nullptr;
public:
    explicit MulticastRingBuffer(size_t buf_size) { check(gm_ring_create(buf_size, &h_), "MulticastRingBuffer::new"); }
    ~MulticastRingBuffer() { gm_ring_destroy(h_); }
    MulticastRingBuffer(const MulticastRingBuffer&) = delete;
    gm_ring* handle() const { return h_; }
    void write_samples(const std::vector<Complex32>& s) { check(gm_ring_write_samples(h_, reinterpret_cast<const gm_c32*>(s.data()), s.size()), "write_samples"); }
    // producer side that never waits for the H2D copy (pinned staging, head published when the data is in HBM)
    void write_samples_async(const Complex32* s, size_t n) { check(gm_ring_write_samples_async(h_, reinterpret_cast<const gm_c32*>(s), n), "write_samples_async"); }
    void flush() { check(gm_ring_flush(h_), "flush"); }
    // notifier / condvar (:42-43): true once head >= required_idx
    bool wait_head(uint64_t required_idx, uint32_t timeout_ms) const { int r = 0; check(gm_ring_wait_head(h_, required_idx, timeout_ms, &r), "wait_head"); return r != 0; }
    uint64_t get_head() const { uint64_t h = 0; check(gm_ring_get_head(h_, &h), "get_head"); return h; }
    // what the asynchronous writer has ENQUEUED (>= get_head()): the head process_channels_async's passes are gated on
    uint64_t get_enqueued_head() const { uint64_t h = 0; check(gm_ring_get_enqueued_head(h_, &h), "get_enqueued_head"); return h; }
    void copy_to_slice(uint64_t start, std::vector<Complex32>& dest) const {
        check(gm_ring_copy_to_slice(h_, start, reinterpret_cast<gm_c32*>(dest.data()), dest.size()), "copy_to_slice");
    }
};

// ---- gm_plane_ring: n_planes rings on one time axis with one head, written from device memory (what Beamformer / Lcmv / Channelizer
// process_dev leave in their planes) and read by TrackingManager::update_planes, channel c on plane planes[c]
class PlaneRing {
    gm_plane_ring* h_ = nullptr;
public:
    PlaneRing(uint32_t n_planes, uint64_t plane_size) { check(gm_plane_ring_create(n_planes, plane_size, &h_), "PlaneRing::new"); }
    ~PlaneRing() { gm_plane_ring_destroy(h_); }
    PlaneRing(const PlaneRing&) = delete;
    gm_plane_ring* handle() const { return h_; }
    // gm_plane_ring_plan (host only): the rules of the shape -> the bytes of the one allocation
    static uint64_t plan(uint32_t n_planes, uint64_t plane_size) { uint64_t b = 0; check(gm_plane_ring_plan(n_planes, plane_size, &b), "PlaneRing::plan"); return b; }
    uint32_t n_planes() const { uint32_t p = 0; check(gm_plane_ring_info(h_, &p, nullptr, nullptr, nullptr), "PlaneRing::n_planes"); return p; }
    uint64_t plane_size() const { uint64_t s = 0; check(gm_plane_ring_info(h_, nullptr, &s, nullptr, nullptr), "PlaneRing::plane_size"); return s; }
    void* device_base() const { void* d = nullptr; check(gm_plane_ring_info(h_, nullptr, nullptr, nullptr, &d), "PlaneRing::device_base"); return d; }
    // n samples to every plane from device memory (plane p's at d_planes + p * in_stride words): one copy launch on `stream` (null: the
    // ring's own), no host synchronisation
    void write_dev(const void* d_planes, size_t in_stride, size_t n, void* stream = nullptr) {
        check(gm_plane_ring_write_dev(h_, d_planes, in_stride, n, stream), "PlaneRing::write_dev");
    }
    // the synchronous form from a host buffer of the same layout
    void write(const Complex32* planes, size_t in_stride, size_t n) { check(gm_plane_ring_write(h_, reinterpret_cast<const gm_c32*>(planes), in_stride, n), "PlaneRing::write"); }
    uint64_t get_head() const { uint64_t h = 0; check(gm_plane_ring_get_head(h_, &h), "PlaneRing::get_head"); return h; }
    void copy_to_slice(uint32_t plane, uint64_t start, std::vector<Complex32>& dest) const {
        check(gm_plane_ring_copy_to_slice(h_, plane, start, reinterpret_cast<gm_c32*>(dest.data()), dest.size()), "PlaneRing::copy_to_slice");
    }
    void synchronize() { check(gm_plane_ring_synchronize(h_), "PlaneRing::synchronize"); }
};

// ---- rate conversion and pulse blanking (gm_resampler): the two stages rf/frontend.rs names in comments and leaves out.
// fs_out = fs_in * up / down; every output is defined by absolute sample indices, so the words do not depend on the block cuts.
class Resampler {
    gm_resampler* h_ = nullptr;
public:
    explicit Resampler(const gm_resampler_cfg& cfg) { check(gm_resampler_create(&cfg, &h_), "Resampler::new"); }
    Resampler(uint32_t up, uint32_t down, float blank_threshold = 0.0f) {     // every other setting at its default
        gm_resampler_cfg cfg{};
        cfg.up = up; cfg.down = down; cfg.blank_threshold = blank_threshold;
        check(gm_resampler_create(&cfg, &h_), "Resampler::new");
    }
    ~Resampler() { gm_resampler_destroy(h_); }
    Resampler(const Resampler&) = delete;
    gm_resampler* handle() const { return h_; }
    // the synchronous host-buffer forms: this call's outputs
    std::vector<Complex32> process(const std::vector<Complex32>& block) { return run(block.data(), block.size(), GM_FMT_C32); }
    std::vector<Complex32> process_i8(const int8_t* iq, size_t n) { return run(iq, n, GM_FMT_I8_IQ); }
    // device pointers, asynchronous on `stream` (nullptr: the handle's own); returns the number of outputs written
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_resampler_process_dev(h_, d_in, fmt, n_in, d_out, out_cap, &n, stream), "Resampler::process_dev");
        return n;
    }
    void reset(uint64_t input_index = 0) { check(gm_resampler_reset(h_, input_index), "Resampler::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) const { check(gm_resampler_stats(h_, inputs, outputs, blanked), "Resampler::stats"); }
    void taps(float* table) const { check(gm_resampler_taps(h_, table), "Resampler::taps"); }      // (n_phases + 1) * taps words
    void synchronize() { check(gm_resampler_synchronize(h_), "Resampler::synchronize"); }
private:
    std::vector<Complex32> run(const void* in, size_t n, int fmt) {
        size_t got = 0;
        std::vector<Complex32> out(n * 16 + 1);                             // a call never delivers more than n * up / down + 1, up / down <= 16
        check(gm_resampler_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(out.data()), out.size(), &got), "Resampler::process");
        out.resize(got);
        return out;
    }
};

// ---- narrowband interference excision (gm_excisor): a 50 % overlap-add filter bank with sine windows and a per-bin gain, and a
// device-side adaptive step that sets the gains from a Welch periodogram.  Same rate, same sample index; every output is defined by
// absolute sample indices, so the words do not depend on the block cuts.
class Excisor {
    gm_excisor* h_ = nullptr;
    uint32_t block_ = 0;
public:
    explicit Excisor(const gm_excisor_cfg& cfg) { init(cfg); }
    explicit Excisor(uint32_t block = 0, uint32_t guard_bins = 0, float blank_threshold = 0.0f) {   // every other setting at its default
        gm_excisor_cfg cfg{};
        cfg.block = block; cfg.guard_bins = guard_bins; cfg.blank_threshold = blank_threshold;
        init(cfg);
    }
    ~Excisor() { gm_excisor_destroy(h_); }
    Excisor(const Excisor&) = delete;
    gm_excisor* handle() const { return h_; }
    uint32_t block() const { return block_; }
    // the synchronous host-buffer forms: this call's outputs
    std::vector<Complex32> process(const std::vector<Complex32>& block) { return run(block.data(), block.size(), GM_FMT_C32); }
    std::vector<Complex32> process_i8(const int8_t* iq, size_t n) { return run(iq, n, GM_FMT_I8_IQ); }
    // device pointers, asynchronous on `stream` (nullptr: the handle's own); returns the number of outputs written
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_excisor_process_dev(h_, d_in, fmt, n_in, d_out, out_cap, &n, stream), "Excisor::process_dev");
        return n;
    }
    // periodogram, median, mask and gains from n device samples, enqueued with no host wait
    void adapt_dev(const void* d_in, int fmt, size_t n, void* stream = nullptr) { check(gm_excisor_adapt_dev(h_, d_in, fmt, n, stream), "Excisor::adapt_dev"); }
    void set_gains(const std::vector<float>& gains) {
        if (gains.size() != block_) check(GM_ERR_INVALID_ARG, "Excisor::set_gains (one gain per bin)");
        check(gm_excisor_set_gains(h_, gains.data()), "Excisor::set_gains");
    }
    std::vector<float> gains() const { std::vector<float> g(block_); check(gm_excisor_gains(h_, g.data()), "Excisor::gains"); return g; }
    // the last adapt's periodogram; median, flagged and zeroed may be null
    std::vector<float> psd(float* median = nullptr, uint32_t* n_flagged = nullptr, uint32_t* n_zeroed = nullptr) const {
        std::vector<float> P(block_);
        check(gm_excisor_psd(h_, P.data(), median, n_flagged, n_zeroed), "Excisor::psd");
        return P;
    }
    // block-adapt mode: a mask per block, decided on the device between the two transforms (threshold_factor 0: 16); off at creation
    void set_block_adapt(float threshold_factor = 0.0f, uint32_t guard_bins = 0) {
        gm_excisor_block_cfg cfg{};
        cfg.threshold_factor = threshold_factor; cfg.guard_bins = guard_bins;
        check(gm_excisor_set_block_adapt(h_, &cfg), "Excisor::set_block_adapt");
    }
    void clear_block_adapt() { check(gm_excisor_set_block_adapt(h_, nullptr), "Excisor::clear_block_adapt"); }
    // its counters since the creation or the last reset (any pointer may be null); synchronises
    void block_stats(uint64_t* blocks, uint64_t* blocks_flagged, uint64_t* bins_flagged, uint64_t* bins_zeroed) const {
        check(gm_excisor_block_stats(h_, blocks, blocks_flagged, bins_flagged, bins_zeroed), "Excisor::block_stats");
    }
    // arms a capture of the power words [cap_blocks][block] and masks [cap_blocks][block] of every later process_dev (both null: disarms)
    void block_capture(float* d_power, uint8_t* d_mask, size_t cap_blocks) {
        check(gm_excisor_block_capture(h_, d_power, d_mask, cap_blocks), "Excisor::block_capture");
    }
    void reset(uint64_t input_index = 0) { check(gm_excisor_reset(h_, input_index), "Excisor::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) const { check(gm_excisor_stats(h_, inputs, outputs, blanked), "Excisor::stats"); }
    void synchronize() { check(gm_excisor_synchronize(h_), "Excisor::synchronize"); }
private:
    void init(const gm_excisor_cfg& cfg) {
        check(gm_excisor_plan(&cfg, 0, 0, &block_, nullptr, nullptr, nullptr), "Excisor::new");
        check(gm_excisor_create(&cfg, &h_), "Excisor::new");
    }
    std::vector<Complex32> run(const void* in, size_t n, int fmt) {
        size_t got = 0;
        std::vector<Complex32> out(n + block_);                             // a call never delivers more than n + H
        check(gm_excisor_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(out.data()), out.size(), &got), "Excisor::process");
        out.resize(got);
        return out;
    }
};

// ---- real-IF down-conversion (gm_ddc): int8 real samples at an intermediate frequency -> complex baseband at fs_in * up / down: blank,
// an exact integer NCO, the resampler's centred polyphase filter.  Every output is defined by absolute sample indices.  The stage to
// put in front of an Excisor, a Resampler or the ring when the capture is real.
class Ddc {
    gm_ddc* h_ = nullptr;
public:
    explicit Ddc(const gm_ddc_cfg& cfg) { check(gm_ddc_create(&cfg, &h_), "Ddc::new"); }
    Ddc(double mix_cycles_per_sample, uint32_t up, uint32_t down, float blank_threshold = 0.0f) {     // every other setting at its default
        gm_ddc_cfg cfg{};
        cfg.mix_cycles_per_sample = mix_cycles_per_sample; cfg.up = up; cfg.down = down; cfg.blank_threshold = blank_threshold;
        check(gm_ddc_create(&cfg, &h_), "Ddc::new");
    }
    ~Ddc() { gm_ddc_destroy(h_); }
    Ddc(const Ddc&) = delete;
    gm_ddc* handle() const { return h_; }
    // host only: the reduced ratio, the defaults, the NCO's phase increment and a call's output count
    static uint64_t plan(const gm_ddc_cfg& cfg, uint64_t inputs_so_far, uint64_t n_in, uint64_t* phase_inc = nullptr) {
        uint64_t n = 0;
        check(gm_ddc_plan(&cfg, inputs_so_far, n_in, nullptr, nullptr, nullptr, nullptr, phase_inc, &n), "Ddc::plan");
        return n;
    }
    // the synchronous host-buffer form: this call's outputs
    std::vector<Complex32> process(const int8_t* real, size_t n) {
        size_t got = 0;
        std::vector<Complex32> out(n * 16 + 1);                             // a call never delivers more than n * up / down + 1, up / down <= 16
        check(gm_ddc_process(h_, real, n, reinterpret_cast<gm_c32*>(out.data()), out.size(), &got), "Ddc::process");
        out.resize(got);
        return out;
    }
    // device pointers (d_in at any byte address), asynchronous on `stream` (nullptr: the handle's own); returns the number of outputs written
    size_t process_dev(const void* d_in, size_t n_in, void* d_out, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_ddc_process_dev(h_, d_in, n_in, d_out, out_cap, &n, stream), "Ddc::process_dev");
        return n;
    }
    // the block step of a real capture: down-converter, then the excisor and the resampler if given, into the ring; ring indices count
    // the last stage's outputs; returns the outputs enqueued
    uint64_t write_ring(MulticastRingBuffer& ring, const int8_t* real, size_t n, Excisor* excisor = nullptr, Resampler* resampler = nullptr) {
        uint64_t total = 0;
        check(gm_ddc_write_ring(h_, excisor ? excisor->handle() : nullptr, resampler ? resampler->handle() : nullptr, ring.handle(), real, n, &total), "Ddc::write_ring");
        return total;
    }
    void reset(uint64_t input_index = 0) { check(gm_ddc_reset(h_, input_index), "Ddc::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) const { check(gm_ddc_stats(h_, inputs, outputs, blanked), "Ddc::stats"); }
    // the (n_phases + 1) * taps filter words and the 4096 + 4096 phasor words; any pointer may be null
    void tables(float* table, Complex32* whi, Complex32* wlo) const { check(gm_ddc_tables(h_, table, reinterpret_cast<gm_c32*>(whi), reinterpret_cast<gm_c32*>(wlo)), "Ddc::tables"); }
    void synchronize() { check(gm_ddc_synchronize(h_), "Ddc::synchronize"); }
};

// ---- polyphase filter bank (gm_channelizer): M sub-bands of one complex stream, each its own Complex32 stream at fs / D; channel k is
// centred at k fs / M.  Every output is defined by absolute sample indices.  With glonass_code() the front of a GLONASS L1OF search:
// fourteen FDMA carriers of one capture, one plane each, a plane pointer going straight into Acquisition's device search.
class Channelizer {
    gm_channelizer* h_ = nullptr;
    uint32_t planes_ = 0, decim_ = 1;
public:
    // channels empty: all n_channels in order; every other setting at its default unless given in a cfg
    Channelizer(uint32_t n_channels, uint32_t decim, const std::vector<uint32_t>& channels = {}, float blank_threshold = 0.0f) {
        gm_channelizer_cfg cfg{};
        cfg.n_channels = n_channels; cfg.decim = decim; cfg.blank_threshold = blank_threshold;
        cfg.n_out_channels = uint32_t(channels.size()); cfg.out_channels = channels.empty() ? nullptr : channels.data();
        init(cfg);
    }
    explicit Channelizer(const gm_channelizer_cfg& cfg) { init(cfg); }
    ~Channelizer() { gm_channelizer_destroy(h_); }
    Channelizer(const Channelizer&) = delete;
    gm_channelizer* handle() const { return h_; }
    uint32_t planes() const { return planes_; }
    // the L1OF ranging code, 511 chips (+1 for logic 0), and the channel indices of its carriers k = -7 .. 6 in a bank of n_channels
    static std::vector<int8_t> glonass_code() {
        std::vector<int8_t> chips(511);
        check(gm_glonass_code(chips.data()), "Channelizer::glonass_code");
        return chips;
    }
    static std::vector<uint32_t> glonass_channels(uint32_t n_channels) {
        std::vector<uint32_t> ch;
        for (int k = -7; k <= 6; ++k) ch.push_back(uint32_t((k + int(n_channels)) % int(n_channels)));
        return ch;
    }
    // the synchronous host-buffer form: this call's outputs, [planes][*n_out] behind each other
    std::vector<Complex32> process(const void* in, int fmt, size_t n, size_t* n_out) {
        const size_t cap = n / decim_ + 2;                                  // a call never delivers more than n / D + 1
        std::vector<Complex32> out(size_t(planes_) * cap), packed;
        size_t got = 0;
        check(gm_channelizer_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(out.data()), cap, &got), "Channelizer::process");
        for (uint32_t i = 0; i < planes_; ++i) packed.insert(packed.end(), out.begin() + i * cap, out.begin() + i * cap + got);
        if (n_out) *n_out = got;
        return packed;
    }
    // device pointers, d_out [planes][out_stride]; asynchronous on `stream` (nullptr: the handle's own); returns the outputs written per plane
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_channelizer_process_dev(h_, d_in, fmt, n_in, d_out, out_stride, out_cap, &n, stream), "Channelizer::process_dev");
        return n;
    }
    void reset(uint64_t input_index = 0) { check(gm_channelizer_reset(h_, input_index), "Channelizer::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) const { check(gm_channelizer_stats(h_, inputs, outputs, blanked), "Channelizer::stats"); }
    std::vector<float> taps() const {
        std::vector<float> g(n_taps_);
        check(gm_channelizer_taps(h_, g.data()), "Channelizer::taps");
        return g;
    }
    void synchronize() { check(gm_channelizer_synchronize(h_), "Channelizer::synchronize"); }
private:
    uint32_t n_taps_ = 0;
    void init(const gm_channelizer_cfg& cfg) {
        check(gm_channelizer_plan(&cfg, 0, 0, &planes_, nullptr, &n_taps_, nullptr), "Channelizer::new");
        decim_ = cfg.decim;
        check(gm_channelizer_create(&cfg, &h_), "Channelizer::new");
    }
};

// ---- adaptive spatial nulling (gm_nuller): A coherent antennas interleaved time sample by time sample in one stream, one Complex32
// stream out at the same rate; per block of B time samples the weights come from the block's own covariance (a null on whatever
// dominates it, the response held at 1 towards the steering vector; none: antenna 0 as the reference).  All counts are time samples.
class Nuller {
    gm_nuller* h_ = nullptr;
    uint32_t antennas_ = 0, block_ = 0;
public:
    // block 0: 1024; loading 0: 1e-4; steering empty: e_0
    explicit Nuller(uint32_t n_antennas, uint32_t block = 0, float loading = 0.0f, const std::vector<Complex32>& steering = {}) {
        gm_nuller_cfg cfg{};
        cfg.n_antennas = n_antennas; cfg.block = block; cfg.loading = loading;
        if (!steering.empty() && steering.size() != n_antennas) check(GM_ERR_INVALID_ARG, "Nuller::new (steering: n_antennas words)");
        cfg.steering = steering.empty() ? nullptr : reinterpret_cast<const gm_c32*>(steering.data());
        check(gm_nuller_plan(&cfg, 0, 0, &block_, nullptr, nullptr), "Nuller::new");
        antennas_ = n_antennas;
        check(gm_nuller_create(&cfg, &h_), "Nuller::new");
    }
    ~Nuller() { gm_nuller_destroy(h_); }
    Nuller(const Nuller&) = delete;
    gm_nuller* handle() const { return h_; }
    uint32_t antennas() const { return antennas_; }
    uint32_t block() const { return block_; }
    // the synchronous host-buffer form: n time samples (n * antennas elements) -> this call's outputs; R ([blocks][A][A]) and w
    // ([blocks][A]) receive the words each of the call's blocks was combined with, where given
    std::vector<Complex32> process(const void* in, int fmt, size_t n, std::vector<Complex32>* R = nullptr, std::vector<Complex32>* w = nullptr) {
        const size_t cap = n + block_, nb = cap / block_;
        std::vector<Complex32> out(cap);
        if (R) R->assign(nb * antennas_ * antennas_, Complex32{});
        if (w) w->assign(nb * antennas_, Complex32{});
        size_t got = 0;
        check(gm_nuller_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(out.data()), cap, &got,
                                R ? reinterpret_cast<gm_c32*>(R->data()) : nullptr, w ? reinterpret_cast<gm_c32*>(w->data()) : nullptr, nb),
              "Nuller::process");
        out.resize(got);
        if (R) R->resize(got / block_ * antennas_ * antennas_);
        if (w) w->resize(got / block_ * antennas_);
        return out;
    }
    // device pointers; asynchronous on `stream` (nullptr: the handle's own); returns the outputs written
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_nuller_process_dev(h_, d_in, fmt, n_in, d_out, out_cap, &n, stream), "Nuller::process_dev");
        return n;
    }
    // fixed weights for every later block (static mode); empty: back to the adaptive rule
    void set_weights(const std::vector<Complex32>& w) {
        if (!w.empty() && w.size() != antennas_) check(GM_ERR_INVALID_ARG, "Nuller::set_weights (n_antennas words)");
        check(gm_nuller_set_weights(h_, w.empty() ? nullptr : reinterpret_cast<const gm_c32*>(w.data())), "Nuller::set_weights");
    }
    // device buffers [cap_blocks][A][A] and [cap_blocks][A] that every later process_dev fills from word 0; nulls and 0 end it
    void capture(void* d_R, void* d_w, size_t cap_blocks) { check(gm_nuller_capture(h_, d_R, d_w, cap_blocks), "Nuller::capture"); }
    void reset(uint64_t input_index = 0) { check(gm_nuller_reset(h_, input_index), "Nuller::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blocks) const { check(gm_nuller_stats(h_, inputs, outputs, blocks), "Nuller::stats"); }
    void synchronize() { check(gm_nuller_synchronize(h_), "Nuller::synchronize"); }
};

// ---- space-time adaptive nulling (gm_stap): the nuller's interleaved stream with `taps` taps in time behind every antenna; per block
// of B time samples the M = antennas * taps weights come from the exact Gram matrix of the block's stacked samples, so that a narrowband
// interferer costs a temporal degree of freedom, not a spatial one.  Steering and weights are laid out [taps][antennas].
class Stap {
    gm_stap* h_ = nullptr;
    uint32_t antennas_ = 0, taps_ = 0, block_ = 0;
public:
    // block 0: 1024; loading 0: 1e-4; steering empty: e_0 (antenna 0 at tap 0)
    Stap(uint32_t n_antennas, uint32_t taps, uint32_t block = 0, float loading = 0.0f, const std::vector<Complex32>& steering = {}) {
        gm_stap_cfg cfg{};
        cfg.n_antennas = n_antennas; cfg.taps = taps; cfg.block = block; cfg.loading = loading;
        if (!steering.empty() && steering.size() != size_t(n_antennas) * taps) check(GM_ERR_INVALID_ARG, "Stap::new (steering: taps * n_antennas words)");
        cfg.steering = steering.empty() ? nullptr : reinterpret_cast<const gm_c32*>(steering.data());
        check(gm_stap_plan(&cfg, 0, 0, &block_, nullptr, nullptr), "Stap::new");
        antennas_ = n_antennas; taps_ = taps;
        check(gm_stap_create(&cfg, &h_), "Stap::new");
    }
    ~Stap() { gm_stap_destroy(h_); }
    Stap(const Stap&) = delete;
    gm_stap* handle() const { return h_; }
    uint32_t antennas() const { return antennas_; }
    uint32_t taps() const { return taps_; }
    uint32_t weights() const { return antennas_ * taps_; }
    uint32_t block() const { return block_; }
    // the synchronous host-buffer form: n time samples (n * antennas elements) -> this call's outputs; R ([blocks][M][M]) and w
    // ([blocks][M]) receive the words each of the call's blocks was combined with, where given
    std::vector<Complex32> process(const void* in, int fmt, size_t n, std::vector<Complex32>* R = nullptr, std::vector<Complex32>* w = nullptr) {
        const size_t cap = n + block_, nb = cap / block_, M = weights();
        std::vector<Complex32> out(cap);
        if (R) R->assign(nb * M * M, Complex32{});
        if (w) w->assign(nb * M, Complex32{});
        size_t got = 0;
        check(gm_stap_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(out.data()), cap, &got,
                              R ? reinterpret_cast<gm_c32*>(R->data()) : nullptr, w ? reinterpret_cast<gm_c32*>(w->data()) : nullptr, nb),
              "Stap::process");
        out.resize(got);
        if (R) R->resize(got / block_ * M * M);
        if (w) w->resize(got / block_ * M);
        return out;
    }
    // device pointers; asynchronous on `stream` (nullptr: the handle's own); returns the outputs written
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, void* stream = nullptr) {
        size_t n = 0;
        check(gm_stap_process_dev(h_, d_in, fmt, n_in, d_out, out_cap, &n, stream), "Stap::process_dev");
        return n;
    }
    // fixed weights for every later block (static mode); empty: back to the adaptive rule
    void set_weights(const std::vector<Complex32>& w) {
        if (!w.empty() && w.size() != weights()) check(GM_ERR_INVALID_ARG, "Stap::set_weights (taps * n_antennas words)");
        check(gm_stap_set_weights(h_, w.empty() ? nullptr : reinterpret_cast<const gm_c32*>(w.data())), "Stap::set_weights");
    }
    // device buffers [cap_blocks][M][M] and [cap_blocks][M] that every later process_dev fills from word 0; nulls and 0 end it
    void capture(void* d_R, void* d_w, size_t cap_blocks) { check(gm_stap_capture(h_, d_R, d_w, cap_blocks), "Stap::capture"); }
    void reset(uint64_t input_index = 0) { check(gm_stap_reset(h_, input_index), "Stap::reset"); }
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, uint64_t* fallback_blocks = nullptr) const {
        check(gm_stap_stats(h_, inputs, outputs, blocks, fallback_blocks), "Stap::stats");
    }
    void synchronize() { check(gm_stap_synchronize(h_), "Stap::synchronize"); }
};

// ---- one beam per satellite from a shared covariance (gm_beamformer): gm_stap's stream, P constraint rows, P output planes; beam p's
// words are those of a Stap with steering = row p
class Beamformer {
    gm_beamformer* h_ = nullptr;
    uint32_t antennas_ = 0, taps_ = 0, beams_ = 0, block_ = 0;
public:
    // steering: [beams][taps][n_antennas], beams = steering.size() / (taps * n_antennas) in 1 .. 16; block 0: 1024; loading 0: 1e-4
    Beamformer(uint32_t n_antennas, uint32_t taps, const std::vector<Complex32>& steering, uint32_t block = 0, float loading = 0.0f) {
        const size_t M = size_t(n_antennas) * taps;
        if (!M || steering.empty() || steering.size() % M) check(GM_ERR_INVALID_ARG, "Beamformer::new (steering: rows of taps * n_antennas words)");
        gm_beamformer_cfg cfg{};
        cfg.n_antennas = n_antennas; cfg.taps = taps; cfg.block = block; cfg.loading = loading;
        cfg.n_beams = uint32_t(steering.size() / M);
        cfg.steering = reinterpret_cast<const gm_c32*>(steering.data());
        check(gm_beamformer_plan(&cfg, 0, 0, &block_, nullptr, nullptr), "Beamformer::new");
        antennas_ = n_antennas; taps_ = taps; beams_ = cfg.n_beams;
        check(gm_beamformer_create(&cfg, &h_), "Beamformer::new");
    }
    ~Beamformer() { gm_beamformer_destroy(h_); }
    Beamformer(const Beamformer&) = delete;
    gm_beamformer* handle() const { return h_; }
    uint32_t antennas() const { return antennas_; }
    uint32_t taps() const { return taps_; }
    uint32_t weights() const { return antennas_ * taps_; }
    uint32_t beams() const { return beams_; }
    uint32_t block() const { return block_; }
    // the synchronous host-buffer form: n time samples -> [beams][*n_out] outputs, plane after plane; R ([blocks][M][M]) and w
    // ([blocks][beams][M]) receive the words each of the call's blocks was combined with, where given
    std::vector<Complex32> process(const void* in, int fmt, size_t n, size_t* n_out = nullptr, std::vector<Complex32>* R = nullptr,
                                   std::vector<Complex32>* w = nullptr) {
        const size_t cap = n + block_, nb = cap / block_, M = weights();
        std::vector<Complex32> planes(cap * beams_);
        if (R) R->assign(nb * M * M, Complex32{});
        if (w) w->assign(nb * beams_ * M, Complex32{});
        size_t got = 0;
        check(gm_beamformer_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(planes.data()), cap, &got,
                                    R ? reinterpret_cast<gm_c32*>(R->data()) : nullptr, w ? reinterpret_cast<gm_c32*>(w->data()) : nullptr, nb),
              "Beamformer::process");
        std::vector<Complex32> out(got * beams_);
        for (uint32_t p = 0; p < beams_; ++p) std::copy(planes.begin() + p * cap, planes.begin() + p * cap + got, out.begin() + p * got);
        if (n_out) *n_out = got;
        if (R) R->resize(got / block_ * M * M);
        if (w) w->resize(got / block_ * beams_ * M);
        return out;
    }
    // device pointers, beam p's plane at d_out + p * out_stride (c32 elements); asynchronous on `stream` (nullptr: the handle's own);
    // returns the outputs written per beam
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, void* stream = nullptr) {
        size_t n = 0;
        check(gm_beamformer_process_dev(h_, d_in, fmt, n_in, d_out, out_stride, &n, stream), "Beamformer::process_dev");
        return n;
    }
    // beam `beam`'s new row for every block a later call finishes (synchronous)
    void set_steering(uint32_t beam, const std::vector<Complex32>& s) {
        if (s.size() != weights()) check(GM_ERR_INVALID_ARG, "Beamformer::set_steering (taps * n_antennas words)");
        check(gm_beamformer_set_steering(h_, beam, reinterpret_cast<const gm_c32*>(s.data())), "Beamformer::set_steering");
    }
    // gm_beamformer_set_steering_dev: n_rows rows [n_rows][M] in DEVICE memory (solve_rows_dev's) into beams first_beam .., by a kernel on
    // `stream` (null: the handle's own), ordered like a process_dev call, no host wait.  A row is installed where it is finite, not all
    // zero and, with d_info, has status 0 and lambda1 >= min_ratio * lambda2; d_installed: [n_rows] bytes on the device or null
    void set_steering_dev(uint32_t first_beam, uint32_t n_rows, const void* d_rows, const void* d_info = nullptr, float min_ratio = 0.0f,
                          void* d_installed = nullptr, void* stream = nullptr) {
        check(gm_beamformer_set_steering_dev(h_, first_beam, n_rows, d_rows, d_info, min_ratio, d_installed, stream), "Beamformer::set_steering_dev");
    }
    // fixed weights [beams][M] for every later block (static mode, synchronous); empty: back to the adaptive rule
    void set_weights(const std::vector<Complex32>& w) {
        if (!w.empty() && w.size() != size_t(beams_) * weights()) check(GM_ERR_INVALID_ARG, "Beamformer::set_weights (beams * taps * n_antennas words)");
        check(gm_beamformer_set_weights(h_, w.empty() ? nullptr : reinterpret_cast<const gm_c32*>(w.data())), "Beamformer::set_weights");
    }
    // device buffers [cap_blocks][M][M] and [cap_blocks][beams][M] that every later process_dev fills from word 0; nulls and 0 end it
    void capture(void* d_R, void* d_w, size_t cap_blocks) { check(gm_beamformer_capture(h_, d_R, d_w, cap_blocks), "Beamformer::capture"); }
    void reset(uint64_t input_index = 0) { check(gm_beamformer_reset(h_, input_index), "Beamformer::reset"); }
    // fallbacks: one count per beam
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, std::vector<uint64_t>* fallbacks = nullptr) const {
        if (fallbacks) fallbacks->assign(beams_, 0);
        check(gm_beamformer_stats(h_, inputs, outputs, blocks, fallbacks ? fallbacks->data() : nullptr), "Beamformer::stats");
    }
    void synchronize() { check(gm_beamformer_synchronize(h_), "Beamformer::synchronize"); }
};

// ---- several constraints on one beam (gm_lcmv): the beamformer's stream and planes, where beam p carries Q_p constraint rows and
// responses in place of one row: C^H w_p = f at the least output power, a signal along row q comes out with the gain conj(f_q)
class Lcmv {
    gm_lcmv* h_ = nullptr;
    uint32_t antennas_ = 0, taps_ = 0, beams_ = 0, block_ = 0;
public:
    // one beam's constraints: rows [Q][taps][n_antennas] and f [Q]
    struct Beam { std::vector<Complex32> rows, f; };
    // beams: 1 .. 16 of them, Q in 1 .. 8 each and at most 16 rows together; block 0: 1024; loading 0: 1e-4
    Lcmv(uint32_t n_antennas, uint32_t taps, const std::vector<Beam>& beams, uint32_t block = 0, float loading = 0.0f) {
        const size_t M = size_t(n_antennas) * taps;
        std::vector<uint32_t> q;
        std::vector<Complex32> rows, f;
        for (const Beam& b : beams) {
            if (!M || b.f.empty() || b.rows.size() != b.f.size() * M) check(GM_ERR_INVALID_ARG, "Lcmv::new (a beam: Q rows of taps * n_antennas words, Q responses)");
            q.push_back(uint32_t(b.f.size()));
            rows.insert(rows.end(), b.rows.begin(), b.rows.end());
            f.insert(f.end(), b.f.begin(), b.f.end());
        }
        gm_lcmv_cfg cfg{};
        cfg.n_antennas = n_antennas; cfg.taps = taps; cfg.block = block; cfg.loading = loading;
        cfg.n_beams = uint32_t(beams.size());
        cfg.n_constraints = q.data();
        cfg.constraints = reinterpret_cast<const gm_c32*>(rows.data());
        cfg.response = reinterpret_cast<const gm_c32*>(f.data());
        check(gm_lcmv_plan(&cfg, 0, 0, &block_, nullptr, nullptr), "Lcmv::new");
        antennas_ = n_antennas; taps_ = taps; beams_ = cfg.n_beams;
        check(gm_lcmv_create(&cfg, &h_), "Lcmv::new");
    }
    ~Lcmv() { gm_lcmv_destroy(h_); }
    Lcmv(const Lcmv&) = delete;
    gm_lcmv* handle() const { return h_; }
    uint32_t antennas() const { return antennas_; }
    uint32_t taps() const { return taps_; }
    uint32_t weights() const { return antennas_ * taps_; }
    uint32_t beams() const { return beams_; }
    uint32_t block() const { return block_; }
    // the synchronous host-buffer form: n time samples -> [beams][*n_out] outputs, plane after plane; R ([blocks][M][M]) and w
    // ([blocks][beams][M]) receive the words each of the call's blocks was combined with, where given
    std::vector<Complex32> process(const void* in, int fmt, size_t n, size_t* n_out = nullptr, std::vector<Complex32>* R = nullptr,
                                   std::vector<Complex32>* w = nullptr) {
        const size_t cap = n + block_, nb = cap / block_, M = weights();
        std::vector<Complex32> planes(cap * beams_);
        if (R) R->assign(nb * M * M, Complex32{});
        if (w) w->assign(nb * beams_ * M, Complex32{});
        size_t got = 0;
        check(gm_lcmv_process(h_, in, fmt, n, reinterpret_cast<gm_c32*>(planes.data()), cap, &got,
                              R ? reinterpret_cast<gm_c32*>(R->data()) : nullptr, w ? reinterpret_cast<gm_c32*>(w->data()) : nullptr, nb),
              "Lcmv::process");
        std::vector<Complex32> out(got * beams_);
        for (uint32_t p = 0; p < beams_; ++p) std::copy(planes.begin() + p * cap, planes.begin() + p * cap + got, out.begin() + p * got);
        if (n_out) *n_out = got;
        if (R) R->resize(got / block_ * M * M);
        if (w) w->resize(got / block_ * beams_ * M);
        return out;
    }
    // device pointers, beam p's plane at d_out + p * out_stride (c32 elements); asynchronous on `stream` (nullptr: the handle's own);
    // returns the outputs written per beam
    size_t process_dev(const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, void* stream = nullptr) {
        size_t n = 0;
        check(gm_lcmv_process_dev(h_, d_in, fmt, n_in, d_out, out_stride, &n, stream), "Lcmv::process_dev");
        return n;
    }
    // beam `beam`'s new rows and responses for every block a later call finishes (synchronous); their number may change
    void set_constraints(uint32_t beam, const Beam& b) {
        if (b.f.empty() || b.rows.size() != b.f.size() * weights()) check(GM_ERR_INVALID_ARG, "Lcmv::set_constraints (Q rows of taps * n_antennas words, Q responses)");
        check(gm_lcmv_set_constraints(h_, beam, uint32_t(b.f.size()), reinterpret_cast<const gm_c32*>(b.rows.data()),
                                      reinterpret_cast<const gm_c32*>(b.f.data())), "Lcmv::set_constraints");
    }
    // fixed weights [beams][M] for every later block (static mode, synchronous); empty: back to the adaptive rule
    void set_weights(const std::vector<Complex32>& w) {
        if (!w.empty() && w.size() != size_t(beams_) * weights()) check(GM_ERR_INVALID_ARG, "Lcmv::set_weights (beams * taps * n_antennas words)");
        check(gm_lcmv_set_weights(h_, w.empty() ? nullptr : reinterpret_cast<const gm_c32*>(w.data())), "Lcmv::set_weights");
    }
    // device buffers [cap_blocks][M][M] and [cap_blocks][beams][M] that every later process_dev fills from word 0; nulls and 0 end it
    void capture(void* d_R, void* d_w, size_t cap_blocks) { check(gm_lcmv_capture(h_, d_R, d_w, cap_blocks), "Lcmv::capture"); }
    void reset(uint64_t input_index = 0) { check(gm_lcmv_reset(h_, input_index), "Lcmv::reset"); }
    // fallbacks: one count per beam
    void stats(uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, std::vector<uint64_t>* fallbacks = nullptr) const {
        if (fallbacks) fallbacks->assign(beams_, 0);
        check(gm_lcmv_stats(h_, inputs, outputs, blocks, fallbacks ? fallbacks->data() : nullptr), "Lcmv::stats");
    }
    void synchronize() { check(gm_lcmv_synchronize(h_), "Lcmv::synchronize"); }
};

// ---- rf::frontend::DigitalFrontend (src/rf/frontend.rs:6-62)
class DigitalFrontend {
    gm_frontend* h_ = nullptr;
public:
    DigitalFrontend(float f_if, float fs_in, float fs_out) { check(gm_frontend_create(f_if, fs_in, fs_out, &h_), "DigitalFrontend::new"); }   // :19-30
    ~DigitalFrontend() { gm_frontend_destroy(h_); }
    DigitalFrontend(const DigitalFrontend&) = delete;
    void process_block(std::vector<float>& raw_floats) { check(gm_frontend_process_block(h_, raw_floats.data(), raw_floats.size()), "process_block"); }   // :33-62
    // rf_thread's block step (rf_thread.rs:43-48): process_block + write_samples, fused on the GPU, non-blocking
    void write_ring(MulticastRingBuffer& ring, const Complex32* block, size_t n) { check(gm_frontend_write_ring(h_, ring.handle(), block, n, GM_FMT_C32), "write_ring"); }
    void write_ring_i8(MulticastRingBuffer& ring, const int8_t* iq, size_t n) { check(gm_frontend_write_ring(h_, ring.handle(), iq, n, GM_FMT_I8_IQ), "write_ring"); }
    // the same block step with the rate conversion (and pulse blanking) between the front-end and the ring: ring indices then count
    // OUTPUT samples (ring index m is input time m * down / up); returns the outputs enqueued
    uint64_t write_ring(MulticastRingBuffer& ring, const Complex32* block, size_t n, Resampler& resampler) {
        uint64_t total = 0;
        check(gm_frontend_write_ring_resampled(h_, resampler.handle(), ring.handle(), block, n, GM_FMT_C32, &total), "write_ring");
        return total;
    }
    uint64_t write_ring_i8(MulticastRingBuffer& ring, const int8_t* iq, size_t n, Resampler& resampler) {
        uint64_t total = 0;
        check(gm_frontend_write_ring_resampled(h_, resampler.handle(), ring.handle(), iq, n, GM_FMT_I8_IQ, &total), "write_ring");
        return total;
    }
    // ... and with the excisor between the front-end and the resampler (resampler may be null: ring indices then count the excisor's
    // outputs, ring index n is input time n); returns the outputs enqueued
    uint64_t write_ring(MulticastRingBuffer& ring, const Complex32* block, size_t n, Excisor& excisor, Resampler* resampler = nullptr) {
        uint64_t total = 0;
        check(gm_frontend_write_ring_conditioned(h_, excisor.handle(), resampler ? resampler->handle() : nullptr, ring.handle(), block, n, GM_FMT_C32, &total), "write_ring");
        return total;
    }
    uint64_t write_ring_i8(MulticastRingBuffer& ring, const int8_t* iq, size_t n, Excisor& excisor, Resampler* resampler = nullptr) {
        uint64_t total = 0;
        check(gm_frontend_write_ring_conditioned(h_, excisor.handle(), resampler ? resampler->handle() : nullptr, ring.handle(), iq, n, GM_FMT_I8_IQ, &total), "write_ring");
        return total;
    }
    uint32_t debug_repairs() const { uint32_t n = 0; check(gm_frontend_debug_repairs(h_, &n), "debug_repairs"); return n; }   // runs of the speculative form done again
    std::array<uint32_t, 3> debug_forms() const { std::array<uint32_t, 3> c{}; check(gm_frontend_debug_forms(h_, c.data()), "debug_forms"); return c; }   // launches: sequential, table, speculative
};

// ---- decoding::NavSyncStatus + nav_decoding's per-epoch step up to frame sync (src/decoding.rs:40-227, legacy)
class NavSyncStatus {
    gm_nav_sync* h_ = nullptr;
public:
    explicit NavSyncStatus(int mode = GM_NAV_FAITHFUL) { check(gm_nav_sync_create(mode, &h_), "NavSyncStatus::new"); }
    ~NavSyncStatus() { gm_nav_sync_destroy(h_); }
    NavSyncStatus(const NavSyncStatus&) = delete;
    gm_nav_sync* handle() const { return h_; }
    gm_nav_status update(float old_i_prompt, float i_prompt, uint64_t cnt, uint64_t buff_loc = 0) {
        gm_nav_status st{};
        check(gm_nav_sync_update(h_, old_i_prompt, i_prompt, cnt, buff_loc, &st), "nav_decoding");
        return st;
    }
    std::vector<int8_t> frame_bits() const {
        size_t n = 0;
        check(gm_nav_sync_frame_bits(h_, nullptr, 0, &n), "frame_bits");
        std::vector<int8_t> b(n);
        if (n) check(gm_nav_sync_frame_bits(h_, b.data(), n, &n), "frame_bits");
        return b;
    }
};

// ---- tracking::do_tracking (src/tracking/do_tracking.rs)
struct LoopFilter {                                            // :52-71
    float tau1 = 0, tau2 = 0;
    LoopFilter(float noise_bw, float dumping_ratio, float gain) { check(gm_loop_filter_new(noise_bw, dumping_ratio, gain, &tau1, &tau2), "LoopFilter::new"); }
    float update(float d_err, float err, float dt) const { return gm_loop_filter_update(tau1, tau2, d_err, err, dt); }
};
enum class TrackingMessageKind { SatelliteLost, SatelliteLocked };   // :47-50
struct TrackingMessage { TrackingMessageKind kind; uint8_t prn; };
using CorrelatorOut = gm_trk_out;   // (i_p,q_p,i_e,q_e,i_l,q_l [,very early / very late])

class TrackingManager;              // TrackingManager::new (:336-348)
class TrackingChannel {             // a view of one channel of the manager's handle (:88-327)
    gm_trk* h_; uint32_t id_;
    friend class TrackingManager;
    TrackingChannel(gm_trk* h, uint32_t id) : h_(h), id_(id) {}
public:
    uint32_t id() const { return id_; }
    gm_trk_state state() const { gm_trk_state s; check(gm_trk_get_state(h_, id_, &s), "state"); return s; }
    void start(const AcquisitionResult& r) { check(gm_trk_start(h_, id_, &r), "TrackingChannel::start"); }      // :148-154
    bool is_active() const { return state().active != 0; }                                                       // :156-158
    void reset() { check(gm_trk_reset(h_, id_), "TrackingChannel::reset"); }                                     // :311-327
    float get_ca_chip(float phase) const { float c; check(gm_trk_get_ca_chip(h_, id_, phase, &c), "get_ca_chip"); return c; }   // :274-277
    CorrelatorOut early_late_correlation(const std::vector<Complex32>& data_samples) {                           // :231-272
        gm_trk_out o; check(gm_trk_correlate(h_, id_, reinterpret_cast<const gm_c32*>(data_samples.data()), data_samples.size(), &o), "early_late_correlation"); return o;
    }
    std::optional<TrackingMessage> do_work(const std::vector<Complex32>& data_samples, CorrelatorOut* out = nullptr) {   // :183-210
        gm_trk_out o; uint8_t lost = 0, prn = 0;
        check(gm_trk_do_work(h_, id_, reinterpret_cast<const gm_c32*>(data_samples.data()), data_samples.size(), &o, &lost, &prn), "do_work");
        if (out) *out = o;
        if (lost) return TrackingMessage{TrackingMessageKind::SatelliteLost, prn};
        return std::nullopt;
    }
    // gm_trk_bank_samples: taps (chips) x carrier offsets (Hz; empty: the single offset 0) on caller-supplied samples at this channel's
    // state as it stands, or at *at; nothing is advanced.  -> [F][T]
    std::vector<Complex32> bank(const std::vector<Complex32>& data_samples, const std::vector<float>& taps,
                                const std::vector<float>& offsets_hz = {}, const gm_trk_state* at = nullptr) {
        const gm_trk_state s = at ? *at : state();
        gm_trk_bank_cfg c{}; c.n_taps = uint32_t(taps.size()); c.n_offsets = uint32_t(offsets_hz.size());
        c.taps_chips = taps.data(); c.offsets_hz = offsets_hz.empty() ? nullptr : offsets_hz.data();
        std::vector<Complex32> out(taps.size() * (offsets_hz.empty() ? 1 : offsets_hz.size()));
        check(gm_trk_bank_samples(h_, &s, reinterpret_cast<const gm_c32*>(data_samples.data()), data_samples.size(), &c,
                                  reinterpret_cast<gm_c32*>(out.data())), "TrackingChannel::bank");
        return out;
    }
};

class TrackingManager {
    gm_trk* h_ = nullptr; uint32_t n_ = 0;
public:
    std::vector<TrackingChannel> channels;
    TrackingManager(float fs, uint32_t n_channels = 15, int code_index_mode = GM_CODE_INDEX_FAITHFUL, uint32_t n_arms = 3,
                    bool strict_libm = false, bool strict_sum_order = false, bool share_device = false) : n_(n_channels) {
        gm_trk_cfg c{}; c.fs = fs; c.n_channels = n_channels; c.n_arms = n_arms; c.code_index_mode = code_index_mode;
        c.strict_libm = strict_libm ? 1 : 0; c.strict_sum_order = strict_sum_order ? 1 : 0; c.share_device = share_device ? 1 : 0;
        check(gm_trk_create(&c, &h_), "TrackingManager::new");
        for (uint32_t i = 0; i < n_channels; ++i) channels.push_back(TrackingChannel(h_, i));
    }
    ~TrackingManager() { gm_trk_destroy(h_); }
    TrackingManager(const TrackingManager&) = delete;
    // process_channels' fan-out (:364-371), up to max_epochs passes; returns passes in which a channel ran
    uint32_t process_channels(MulticastRingBuffer& ring, uint32_t max_epochs, std::vector<CorrelatorOut>* outs = nullptr,
                              std::vector<uint8_t>* processed = nullptr, std::vector<uint8_t>* lost = nullptr) {
        const size_t n = size_t(max_epochs) * n_;
        if (outs) outs->resize(n);
        if (processed) processed->resize(n);
        if (lost) lost->resize(n);
        uint32_t done = 0;
        check(gm_trk_update_all(h_, ring.handle(), max_epochs, outs ? outs->data() : nullptr, processed ? processed->data() : nullptr,
                                lost ? lost->data() : nullptr, &done), "process_channels");
        return done;
    }
    // the same passes WITHOUT a host wait (ABI 6): ordered on the device behind everything the ring's asynchronous writer has enqueued
    // (the Condvar wait of do_tracking.rs:392-406 as an event on the ring's stream); the results are collected later, by ticket
    uint64_t process_channels_async(MulticastRingBuffer& ring, uint32_t max_epochs) {
        uint64_t ticket = 0;
        check(gm_trk_update_all_async(h_, ring.handle(), max_epochs, &ticket), "process_channels_async");
        pending_[ticket] = max_epochs;
        return ticket;
    }
    // false while the call is still running (wait = false); else the passes in which a channel ran through *done
    // states: the channel records as they stood behind THAT call's passes (a device-side snapshot in stream order)
    bool collect(uint64_t ticket, bool wait, uint32_t* done = nullptr, std::vector<CorrelatorOut>* outs = nullptr,
                 std::vector<uint8_t>* processed = nullptr, std::vector<uint8_t>* lost = nullptr,
                 std::vector<gm_trk_state>* states = nullptr) {
        const auto it = pending_.find(ticket);
        if (it == pending_.end()) throw Panic(GM_ERR_INVALID_ARG, "collect: no such ticket");
        const size_t n = size_t(it->second) * n_;
        if (outs) outs->resize(n);
        if (processed) processed->resize(n);
        if (lost) lost->resize(n);
        if (states) states->resize(n_);
        int ready = 0; uint32_t d = 0;
        const int rc = gm_trk_collect(h_, ticket, wait ? 1 : 0, outs ? outs->data() : nullptr, processed ? processed->data() : nullptr,
                                      lost ? lost->data() : nullptr, states ? states->data() : nullptr, &d, &ready);
        if (rc != GM_OK) { pending_.erase(it); check(rc, "collect"); }      // a failed collect has consumed the ticket (header)
        if (!ready) return false;
        pending_.erase(it);
        if (done) *done = d;
        return true;
    }
    size_t tickets_in_flight() const { return pending_.size(); }
    uint32_t n_channels() const { return n_; }
    uint32_t pass_count(uint64_t ticket) const { const auto it = pending_.find(ticket); return it == pending_.end() ? 0 : it->second; }
    // every channel's record in one synchronisation + one copy (ABI 7)
    std::vector<gm_trk_state> states() const { std::vector<gm_trk_state> s(n_); check(gm_trk_get_states(h_, s.data()), "states"); return s; }
    // gm_trk_bank: taps (chips) x carrier offsets (Hz; empty: the single offset 0) of one code period at tracking records, read from
    // the ring; nothing is advanced.  records NULL: the handle's own channels as they stand.  -> [R][F][T]; done: [R] flags, 0 for a
    // skipped record (whose words are zeros)
    std::vector<Complex32> bank(MulticastRingBuffer& ring, const std::vector<float>& taps, const std::vector<float>& offsets_hz = {},
                                const std::vector<gm_trk_state>* records = nullptr, std::vector<uint8_t>* done = nullptr) {
        const uint32_t r = records ? uint32_t(records->size()) : n_;
        gm_trk_bank_cfg c{}; c.n_taps = uint32_t(taps.size()); c.n_offsets = uint32_t(offsets_hz.size());
        c.taps_chips = taps.data(); c.offsets_hz = offsets_hz.empty() ? nullptr : offsets_hz.data();
        std::vector<Complex32> out(size_t(r) * taps.size() * (offsets_hz.empty() ? 1 : offsets_hz.size()));
        if (done) done->assign(r, 0);
        check(gm_trk_bank(h_, ring.handle(), records ? records->data() : nullptr, r, &c, reinterpret_cast<gm_c32*>(out.data()),
                          done ? done->data() : nullptr), "TrackingManager::bank");
        return out;
    }
    // gm_trk_bank_plan (host only): the argument rules and the sizes of a bank call for a tracking configuration
    static gm_trk_bank_plan_out bank_plan(const gm_trk_cfg& trk, const std::vector<float>& taps, const std::vector<float>& offsets_hz = {},
                                          uint32_t n_states = 1) {
        gm_trk_bank_cfg c{}; c.n_taps = uint32_t(taps.size()); c.n_offsets = uint32_t(offsets_hz.size());
        c.taps_chips = taps.data(); c.offsets_hz = offsets_hz.empty() ? nullptr : offsets_hz.data();
        gm_trk_bank_plan_out p{};
        check(gm_trk_bank_plan(&trk, &c, n_states, &p), "TrackingManager::bank_plan");
        return p;
    }
    // gm_trk_array_prompts: one code period of an interleaved array stream on the device (d_samples: time sample first_index, n_time
    // time samples of n_antennas elements of fmt, written before the call) against the tracker's replica at tracking records, every
    // antenna and tap delay at once; nothing is advanced.  records NULL: the handle's own channels as they stand.  -> [R][L][A], the
    // word order gm_array_row_solve takes; done: [R] flags, 0 for a skipped record (whose words are zeros)
    std::vector<Complex32> array_prompts(const void* d_samples, int fmt, uint64_t first_index, uint64_t n_time, uint32_t n_antennas,
                                         uint32_t taps = 1, float tap_chips = 0.0f, const std::vector<gm_trk_state>* records = nullptr,
                                         std::vector<uint8_t>* done = nullptr) {
        const uint32_t r = records ? uint32_t(records->size()) : n_;
        gm_trk_array_cfg c{}; c.n_antennas = n_antennas; c.taps = taps; c.tap_chips = tap_chips;
        std::vector<Complex32> z(size_t(r) * taps * n_antennas);
        if (done) done->assign(r, 0);
        check(gm_trk_array_prompts(h_, d_samples, fmt, first_index, n_time, records ? records->data() : nullptr, r, &c,
                                   reinterpret_cast<gm_c32*>(z.data()), done ? done->data() : nullptr), "TrackingManager::array_prompts");
        return z;
    }
    // gm_trk_array_prompts_dev: array_prompts' words into device buffers (d_z [R][L][A] c32, d_done [R] bytes), asynchronous on `stream`
    // (null: the handle's own), no host wait; the records are required (the states a collect handed over) and read before the return
    void array_prompts_dev(const void* d_samples, int fmt, uint64_t first_index, uint64_t n_time, uint32_t n_antennas, uint32_t taps,
                           float tap_chips, const std::vector<gm_trk_state>& records, void* d_z, void* d_done, void* stream = nullptr) {
        gm_trk_array_cfg c{}; c.n_antennas = n_antennas; c.taps = taps; c.tap_chips = tap_chips;
        check(gm_trk_array_prompts_dev(h_, d_samples, fmt, first_index, n_time, records.data(), uint32_t(records.size()), &c, d_z, d_done,
                                       stream), "TrackingManager::array_prompts_dev");
    }
    // gm_trk_array_plan (host only): the argument rules and the sizes of an array_prompts call for a tracking configuration
    static gm_trk_array_plan_out array_plan(const gm_trk_cfg& trk, uint32_t n_antennas, uint32_t taps = 1, float tap_chips = 0.0f,
                                            uint32_t n_states = 1) {
        gm_trk_array_cfg c{}; c.n_antennas = n_antennas; c.taps = taps; c.tap_chips = tap_chips;
        gm_trk_array_plan_out p{};
        check(gm_trk_array_plan(&trk, &c, n_states, &p), "TrackingManager::array_plan");
        return p;
    }
    // ---- tracking on planes: channel c on plane planes[c] of a PlaneRing (every other method ignores the map)
    // gm_trk_set_channel_planes (empty: every channel on plane 0), installed stream-ordered on the handle's stream
    void set_channel_planes(const std::vector<uint32_t>& planes = {}) {
        if (!planes.empty() && planes.size() != n_) throw Panic(GM_ERR_INVALID_ARG, "set_channel_planes: n_channels entries");
        check(gm_trk_set_channel_planes(h_, planes.empty() ? nullptr : planes.data()), "TrackingManager::set_channel_planes");
    }
    std::vector<uint32_t> channel_planes() const { std::vector<uint32_t> m(n_); check(gm_trk_get_channel_planes(h_, m.data()), "channel_planes"); return m; }
    // process_channels on the plane ring, gated on its ENQUEUED head; returns the passes in which a channel ran
    uint32_t update_planes(PlaneRing& ring, uint32_t max_epochs, std::vector<CorrelatorOut>* outs = nullptr,
                           std::vector<uint8_t>* processed = nullptr, std::vector<uint8_t>* lost = nullptr) {
        const size_t n = size_t(max_epochs) * n_;
        if (outs) outs->resize(n);
        if (processed) processed->resize(n);
        if (lost) lost->resize(n);
        uint32_t done = 0;
        check(gm_trk_update_planes(h_, ring.handle(), max_epochs, outs ? outs->data() : nullptr, processed ? processed->data() : nullptr,
                                   lost ? lost->data() : nullptr, &done), "TrackingManager::update_planes");
        return done;
    }
    // the same passes enqueued only, no host readback
    void update_planes_dev(PlaneRing& ring, uint32_t epochs) { check(gm_trk_update_planes_dev(h_, ring.handle(), epochs), "TrackingManager::update_planes_dev"); }
    // gm_trk_planes_plan (host only): the argument rules and the sizes of an update_planes call; planes empty: every channel on plane 0
    static gm_trk_planes_plan_out planes_plan(const gm_trk_cfg& trk, uint32_t n_planes, const std::vector<uint32_t>& planes = {},
                                              uint32_t max_epochs = 1) {
        if (!planes.empty() && planes.size() != trk.n_channels) throw Panic(GM_ERR_INVALID_ARG, "planes_plan: n_channels entries");
        gm_trk_planes_plan_out p{};
        check(gm_trk_planes_plan(&trk, n_planes, planes.empty() ? nullptr : planes.data(), max_epochs, &p), "TrackingManager::planes_plan");
        return p;
    }
private:
    std::map<uint64_t, uint32_t> pending_;      // ticket -> its pass count
};

// ---- the two stage drivers: do_acquisition::run (do_acquisition.rs:241-327) and
// do_tracking::run (do_tracking.rs:384-415), talking through the reference's two unbounded channels
// (main.rs:183-184).  The reference loops forever; here a StageControl stops the loops and can scale the pacing.
template <class T> class Channel {           // crossbeam_channel::unbounded()
    std::deque<T> q_;
    mutable std::mutex m_;
public:
    bool send(T v) { std::lock_guard<std::mutex> g(m_); q_.push_back(std::move(v)); return true; }
    std::optional<T> try_recv() {
        std::lock_guard<std::mutex> g(m_);
        if (q_.empty()) return std::nullopt;
        T v = std::move(q_.front()); q_.pop_front();
        return v;
    }
    size_t len() const { std::lock_guard<std::mutex> g(m_); return q_.size(); }
};

struct StageControl {
    std::atomic<bool> stop{false};
    double pacing_scale = 1.0;            // 1.0 = the reference's 500 / 1000 / 2000 ms search intervals (:59-63)
    std::atomic<uint64_t> acq_rounds{0}, trk_passes{0};
    // round 6: what a feeder that replays faster than real time needs for flow control, and what a harness reports
    std::atomic<uint64_t> trk_collected_head{0};   // ring head up to which the tracking stage's passes have run AND been collected
    std::atomic<uint64_t> channel_epochs{0};       // channel x code-period updates collected so far
    std::atomic<uint64_t> acq_ns{0}, fine_ns{0}, trk_ns{0}, hook_ns{0};   // wall clock spent inside the stages' calls
    std::atomic<bool> trk_finished{false};         // the tracking stage has collected its last call (its handles are torn down after this)
    std::atomic<int> stages_ready{0};              // + 1 by each stage once its handles exist (tables, code spectra, result slots): a
                                                   // replay that outruns real time starts its feeder when both stages are listening
};
inline uint64_t stage_ns(std::chrono::steady_clock::time_point t0) {
    return uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
}

struct AcquisitionRunOptions {            // the reference's compile-time constants (:20-23) as run-time values
    float freq_search_hz = 14e3f;         // FREQ_SEARCH_ACQUISITION_HZ
    float freq_step_hz = 500.0f;          // FREQ_SEARCH_STEP_HZ
    uint32_t long_samples_length = 10;    // LONG_SAMPLES_LENGTH (ms)
    int decision_mode = GM_DECIDE_REFERENCE;
    // The reference paces its rounds on the wall clock (:292-295), which IS signal time for a live source.  A replay that runs
    // faster (or slower) than real time keeps the reference's cadence per second of SIGNAL with this switch: the interval is
    // counted in samples of the ring's head.  first_round_signal_ms < 0: the reference's behaviour (the first round after one
    // interval, `last_run = Instant::now()` at :274); >= 0: the first round once that much signal is in the ring.
    bool pace_on_signal_time = false;
    double first_round_signal_ms = -1.0;
    // refine every hit's carrier (finer_doppler, acquisition_bk.rs:215-302) before it goes to tracking
    bool fine_doppler = false;
    // the same hand-over through gm_acq_refine_doppler (per-period prompts: follows coherent_periods, an edge search and a code-drift
    // compensation set on the engine); when set it replaces fine_doppler's carrier with carrier_hz
    bool refine_doppler = false;
    // gm_acq_cfg.coherent_periods: K code periods integrated coherently; a round then searches K * long_samples_length periods
    uint32_t coherent_periods = 1;
    std::function<void(uint64_t head, const std::vector<std::optional<AcquisitionResult>>&)> on_round;   // after every round (may be empty)
};

inline void run_acquisition(MulticastRingBuffer& multi_buffer, float freq_sampling_hz, float f_if,
                            Channel<AcquisitionResult>& to_tracking, Channel<TrackingMessage>& from_tracking,
                            StageControl& ctl, const AcquisitionRunOptions& opt = {}) {
    const size_t capacity = size_t(uint16_t(opt.freq_search_hz) / uint16_t(opt.freq_step_hz)) + 1;        // :248
    const uint32_t fft_size = uint32_t(std::lround(freq_sampling_hz / (1.023e6f / 1023.0f)));              // :249-251
    std::vector<float> doppler(capacity);
    for (size_t i = 0; i < capacity; ++i) doppler[i] = -opt.freq_search_hz / 2.0f + float(i) * opt.freq_step_hz;   // :253-255
    std::vector<uint8_t> prns(PRN_SEARCH_ACQUISITION_TOTAL);
    for (uint8_t p = 0; p < PRN_SEARCH_ACQUISITION_TOTAL; ++p) prns[p] = uint8_t(p + 1);
    AcquisitionEngine workers(freq_sampling_hz, f_if, fft_size, doppler, prns, opt.long_samples_length, 7.0f,
                              opt.decision_mode, true,       // any_length: fft_size = round(fs / 1 kHz), whatever fs is :252-271
                              opt.coherent_periods);
    std::set<uint8_t> active_prns;
    AcquisitionManager acq_manager;
    ctl.stages_ready++;
    auto last_run = std::chrono::steady_clock::now();
    const auto ms = [&](double v) { return std::chrono::duration<double, std::milli>(v * ctl.pacing_scale); };
    // signal-time pacing: the head (in samples) at which the next round is due
    const double samples_per_ms = double(freq_sampling_hz) * 1e-3;
    uint64_t next_due = opt.first_round_signal_ms >= 0.0 ? uint64_t(opt.first_round_signal_ms * samples_per_ms) : 0;
    bool first = true;
    while (!ctl.stop.load()) {
        while (auto msg = from_tracking.try_recv()) {                                                       // :278-287
            if (msg->kind == TrackingMessageKind::SatelliteLost) active_prns.erase(msg->prn);
            else active_prns.insert(msg->prn);
        }
        acq_manager.update_mode(active_prns.size());                                                        // :289
        auto [interval_ms, mask] = acq_manager.get_pacing_and_list(active_prns);                            // :290
        if (opt.pace_on_signal_time) {
            if (first && opt.first_round_signal_ms < 0.0) next_due = uint64_t(double(interval_ms) * ctl.pacing_scale * samples_per_ms);
            first = false;
            if (int64_t(multi_buffer.get_head() - next_due) < 0) {                                          // :292-295 in samples
                multi_buffer.wait_head(next_due, 2);         // the ring's Condvar, bounded so that `stop` is seen
                continue;
            }
        } else if (std::chrono::steady_clock::now() - last_run < ms(double(interval_ms))) {                 // :292-295
            std::this_thread::sleep_for(ms(50.0));
            continue;
        }
        uint64_t local_tail = 0;
        auto t0 = std::chrono::steady_clock::now();
        auto results = workers.search_ring(multi_buffer.handle(), uint64_t(mask), &local_tail);             // :297-313
        ctl.acq_ns += stage_ns(t0);
        if (!results) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); continue; }              // :324-326
        const uint64_t head_of_round = local_tail + uint64_t(opt.coherent_periods > 1 ? opt.coherent_periods : 1) *
                                                    uint64_t(opt.long_samples_length) * fft_size;
        if (opt.fine_doppler || opt.refine_doppler) {
            // hits on satellites that are tracked already go nowhere (:315-320 would hand them over again; the mask
            // normally excludes them) — refine only what is about to start a channel
            bool any = false;
            for (auto& r : *results) { if (r && active_prns.count(r->prn)) r.reset(); any = any || bool(r); }
            if (any) {
                t0 = std::chrono::steady_clock::now();
                if (opt.refine_doppler) {
                    const auto fine = workers.refine_doppler(*results);
                    for (size_t i = 0; i < results->size(); ++i)
                        if ((*results)[i] && fine[i] && std::isfinite(fine[i]->carrier_hz)) (*results)[i]->carrier_freq = float(fine[i]->carrier_hz);
                } else {
                    const std::vector<float> fine = workers.finer_doppler(*results);
                    for (size_t i = 0; i < results->size(); ++i)
                        if ((*results)[i] && std::isfinite(fine[i])) (*results)[i]->carrier_freq = fine[i];
                }
                ctl.fine_ns += stage_ns(t0);
            }
        }
        for (auto& r : *results)                                                                            // :315-320
            if (r && to_tracking.send(*r)) active_prns.insert(r->prn);
        if (opt.on_round) opt.on_round(head_of_round, *results);
        last_run = std::chrono::steady_clock::now();                                                        // :322
        // the NEXT interval is the one the manager gives for the satellites just handed over (as the loop head would compute it)
        acq_manager.update_mode(active_prns.size());
        next_due = head_of_round + uint64_t(double(acq_manager.get_pacing_and_list(active_prns).first) * ctl.pacing_scale * samples_per_ms);
        ctl.acq_rounds++;
    }
}

// What one collected call of the tracking stage hands to a consumer behind it (nav-bit accumulation, logging): the passes'
// correlator outputs and flags, [passes][n_channels], and the ring head the call was gated on.
struct EpochBlock {
    uint32_t passes = 0, n_channels = 0;
    uint64_t head = 0;
    const CorrelatorOut* outs = nullptr;
    const uint8_t* processed = nullptr;
    const uint8_t* lost = nullptr;
    const gm_trk_state* states = nullptr;       // [n_channels], as they stood behind this call's passes (NULL on the synchronous path)
    const uint8_t* channel_prn = nullptr;       // [n_channels] the PRN each channel was started with (0: never started)
};

struct TrackingRunOptions {
    int code_index_mode = GM_CODE_INDEX_FIXED;
    uint32_t n_channels = 15;                   // NUM_OF_CHANNELS (:18)
    // true (default): no host wait per block — process_channels is ENQUEUED behind whatever the ring's writer has enqueued
    // (gm_trk_update_all_async: the Condvar wait of :392-406 as an event on the ring's stream) and collected a block or two later;
    // false: the synchronous pass per loop turn (rounds 3-5)
    bool async_tickets = true;
    uint32_t max_in_flight = 6;                 // tickets not yet collected (the library holds 8 result slots)
    uint32_t max_passes_per_call = 256;         // the result slots are sized for this once, before the loop (they cannot grow under tickets in flight)
    bool share_device = true;                   // a receiver: leave CUs to the front-end and the acquisition dwell (gm_trk_cfg.share_device)
    bool drain_on_stop = true;                  // after `stop`: hand over pending acquisitions and run every whole code period the ring still holds
    std::function<void(const EpochBlock&)> on_epochs;      // every collected call (may be empty)
    std::vector<gm_trk_state>* final_states = nullptr;
};

namespace detail {
// passes needed so that every active channel reaches `head`: channels advance one code period per pass
inline uint32_t passes_to_head(const std::vector<gm_trk_state>& st, const std::vector<uint8_t>& busy, uint64_t head,
                               const std::vector<uint64_t>& covered) {
    uint64_t worst = 0;
    for (size_t c = 0; c < st.size(); ++c) {
        if (!busy[c] || !st[c].num_samples_per_code) continue;
        const uint64_t n = st[c].num_samples_per_code;
        uint64_t idx = st[c].next_sample_index;
        // passes already enqueued for this channel (not yet collected) take it to the last whole period before covered[c]
        if (int64_t(covered[c] - idx) > 0) idx += ((covered[c] - idx) / n) * n;
        if (int64_t(head - idx) > 0) worst = std::max<uint64_t>(worst, (head - idx) / n);
    }
    return uint32_t(std::min<uint64_t>(worst + 2, 4095));    // + 2: the period length moves by a sample now and then (code_rate)
}
}  // namespace detail

inline void run_tracking(MulticastRingBuffer& multi_ring_buf, Channel<AcquisitionResult>& acq_to_trk,
                         Channel<TrackingMessage>& trk_to_acq, float fs, StageControl& ctl, const TrackingRunOptions& opt) {
    const uint32_t n_channels = opt.n_channels;
    TrackingManager manager(fs, n_channels, opt.code_index_mode, 3, false, false, opt.share_device);        // :390
    std::vector<uint8_t> channel_prn(n_channels, 0), busy(n_channels, 0), lost, processed;
    std::vector<CorrelatorOut> outs;
    std::vector<gm_trk_state> states = manager.states(), snap;       // host view of the channels: exact whenever nothing is in flight
    struct Pending { uint64_t ticket, head, seq; };
    std::deque<Pending> tickets;
    uint64_t issued = 0;                                             // calls enqueued so far
    std::vector<uint64_t> start_seq(n_channels, 0);                  // `issued` when the channel was started: older snapshots predate it
    std::vector<uint64_t> covered(n_channels, 0);                    // the head up to which passes for this channel have been enqueued
    uint64_t planned_head = multi_ring_buf.get_enqueued_head();      // the head the most recent enqueued call was gated on
    ctl.trk_collected_head = planned_head;
    constexpr uint32_t LOOP_MS = 10;                                                                        // :29
    const bool want_outs = bool(opt.on_epochs);
    const uint32_t max_passes = std::max<uint32_t>(opt.max_passes_per_call, 3);
    if (opt.async_tickets)      // one empty call of the largest size: pinned result slots, copy path and events exist before the first block
        manager.collect(manager.process_channels_async(multi_ring_buf, max_passes), true);
    ctl.stages_ready++;

    // process_channels' first half (:352-362): hand new acquisitions to idle channels
    const auto take_acquisitions = [&] {
        while (auto msg = acq_to_trk.try_recv()) {
            for (uint32_t c = 0; c < n_channels; ++c) {
                if (busy[c]) continue;
                trk_to_acq.send(TrackingMessage{TrackingMessageKind::SatelliteLocked, msg->prn});
                manager.channels[c].start(*msg);       // (waits for the passes in flight: a hand-over, a few per minute)
                states[c] = manager.channels[c].state();
                busy[c] = 1; channel_prn[c] = msg->prn;
                start_seq[c] = issued; covered[c] = states[c].next_sample_index;
                break;
            }
        }
    };
    const auto report = [&](uint32_t passes, uint32_t done, uint64_t head, const gm_trk_state* st) {
        uint64_t ran = 0;
        for (uint32_t e = 0; e < passes; ++e)
            for (uint32_t c = 0; c < n_channels; ++c) {
                ran += processed[size_t(e) * n_channels + c];
                if (lost[size_t(e) * n_channels + c]) {
                    // the reference's message carries prn 0 (reset() runs first, :199-201); FIXED reports the real one
                    const uint8_t prn = opt.code_index_mode == GM_CODE_INDEX_FAITHFUL ? uint8_t(0) : channel_prn[c];
                    trk_to_acq.send(TrackingMessage{TrackingMessageKind::SatelliteLost, prn});
                    busy[c] = 0;
                }
            }
        ctl.trk_passes += done; ctl.channel_epochs += ran;
        if (opt.on_epochs) {
            const auto t0 = std::chrono::steady_clock::now();
            EpochBlock b; b.passes = passes; b.n_channels = n_channels; b.head = head; b.outs = outs.data();
            b.processed = processed.data(); b.lost = lost.data(); b.states = st; b.channel_prn = channel_prn.data();
            opt.on_epochs(b);
            ctl.hook_ns += stage_ns(t0);
        }
        ctl.trk_collected_head = head;
    };
    // collect what is ready (everything, waiting, when `all`); true if a call was collected
    const auto drain = [&](bool all) {
        bool got = false;
        while (!tickets.empty()) {
            const auto t0 = std::chrono::steady_clock::now();
            const uint32_t passes = manager.pass_count(tickets.front().ticket);
            uint32_t done = 0;
            const bool ready = manager.collect(tickets.front().ticket, all || tickets.size() >= opt.max_in_flight, &done,
                                               want_outs ? &outs : nullptr, &processed, &lost, &snap);
            ctl.trk_ns += stage_ns(t0);
            if (!ready) break;
            const uint64_t head = tickets.front().head, seq = tickets.front().seq;
            tickets.pop_front();
            // the collected snapshot is the truth for every channel that was not (re)started after that call was enqueued
            for (uint32_t c = 0; c < n_channels; ++c)
                if (seq >= start_seq[c]) states[c] = snap[c];
            report(passes, done, head, snap.data());
            got = true;
        }
        return got;
    };

    bool stopping = false;
    for (;;) {
        if (!stopping && ctl.stop.load()) { stopping = true; if (!opt.drain_on_stop) break; }
        take_acquisitions();
        bool any_active = false;
        for (uint32_t c = 0; c < n_channels; ++c) any_active = any_active || busy[c];
        bool progressed = false;
        if (opt.async_tickets) {
            const uint64_t head = multi_ring_buf.get_enqueued_head();
            if (any_active && tickets.size() < opt.max_in_flight) {
                const uint32_t passes = std::min(detail::passes_to_head(states, busy, head, covered), max_passes);
                if (passes > 2 || (stopping && tickets.empty())) {      // > 2: at least one whole code period is there for some channel
                    const auto t0 = std::chrono::steady_clock::now();
                    tickets.push_back(Pending{manager.process_channels_async(multi_ring_buf, passes), head, issued++});
                    ctl.trk_ns += stage_ns(t0);
                    planned_head = head;
                    for (uint32_t c = 0; c < n_channels; ++c) {         // how far this call takes each channel (all the way unless capped)
                        if (!busy[c] || !states[c].num_samples_per_code) continue;
                        const uint64_t n = states[c].num_samples_per_code;
                        uint64_t idx = states[c].next_sample_index;
                        if (int64_t(covered[c] - idx) > 0) idx += ((covered[c] - idx) / n) * n;
                        const uint64_t reach = idx + uint64_t(passes) * n;
                        covered[c] = int64_t(reach - head) < 0 ? reach : head;
                    }
                    progressed = true;
                }
            }
            const size_t before = tickets.size();
            const uint64_t passes_before = ctl.trk_passes.load();
            progressed = drain(stopping) || progressed;
            if (stopping) {
                // done when a drained call found nothing left to run and nothing new is waiting
                if (tickets.empty() && before && ctl.trk_passes.load() == passes_before && acq_to_trk.len() == 0) break;
                if (!any_active && acq_to_trk.len() == 0) break;
                continue;
            }
            if (!any_active) ctl.trk_collected_head = head;       // nothing to track: the feeder is not held back
        } else {
            // ... every active channel with a whole code period available runs update(), up to LOOP_MS passes, synchronously
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t head = multi_ring_buf.get_head();
            const uint32_t done = manager.process_channels(multi_ring_buf, LOOP_MS, want_outs ? &outs : nullptr, &processed, &lost);
            ctl.trk_ns += stage_ns(t0);
            report(LOOP_MS, done, head, nullptr);
            progressed = done != 0;
            if (stopping) { if (!done && acq_to_trk.len() == 0) break; continue; }
            if (!done) states = manager.states();                 // next_tracking_index (:373-381) needs the current records
        }
        if (!progressed && opt.async_tickets && !tickets.empty()) {
            // calls in flight: their completion and the writer's next ENQUEUED block are what this thread reacts to — neither moves
            // the published head's Condvar, so look again shortly (one ticket per writer block keeps the collected head a few
            // blocks behind the writer instead of a ticket's worth of blocks)
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        } else if (!progressed) {                                                       // Condvar wait (:392-406)
            uint64_t required_idx = 0; bool any = false;                                // next_tracking_index (:373-381)
            for (uint32_t c = 0; c < n_channels; ++c) {
                if (!busy[c] || !states[c].active) continue;
                uint64_t need = states[c].next_sample_index + states[c].num_samples_per_code;
                if (opt.async_tickets && int64_t(planned_head - need) >= 0) need = planned_head + states[c].num_samples_per_code;
                if (!any || int64_t(need - required_idx) < 0) required_idx = need;
                any = true;
            }
            if (any) multi_ring_buf.wait_head(required_idx, 1);     // bounded (1 ms) so that `stop` and new acquisitions are seen
            else std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    while (!tickets.empty()) drain(true);
    ctl.trk_finished = true;
    if (opt.final_states) *opt.final_states = manager.states();
}

// the signature of rounds 3-5 (tests/cpp/test_host_api.cpp): the default options, i.e. the ticket loop
inline void run_tracking(MulticastRingBuffer& multi_ring_buf, Channel<AcquisitionResult>& acq_to_trk,
                         Channel<TrackingMessage>& trk_to_acq, float fs, StageControl& ctl,
                         int code_index_mode = GM_CODE_INDEX_FIXED, uint32_t n_channels = 15,
                         std::vector<gm_trk_state>* final_states = nullptr) {
    TrackingRunOptions opt;
    opt.code_index_mode = code_index_mode; opt.n_channels = n_channels; opt.final_states = final_states;
    run_tracking(multi_ring_buf, acq_to_trk, trk_to_acq, fs, ctl, opt);
}

// ---- crate root FFT<T> / RealFFT<T> (src/fft.rs:5-56), T = f32
class FFT {
    size_t len_;
public:
    explicit FFT(size_t len) : len_(len) {}
    std::vector<Complex32> execute(std::vector<Complex32>& input) const {   // in place, returns a copy (:21-25)
        check(gm_fft_c2c_f32(len_, 0, reinterpret_cast<gm_c32*>(input.data()), input.size() / len_), "FFT::execute");
        return input;
    }
    std::vector<float> power_spectrum(std::vector<Complex32>& input) const {
        std::vector<float> p(len_);
        check(gm_fft_power_spectrum_f32(len_, reinterpret_cast<gm_c32*>(input.data()), p.data()), "FFT::power_spectrum");
        return p;
    }
};
class RealFFT {
    size_t len_;
public:
    explicit RealFFT(size_t len) : len_(len) {}
    std::vector<Complex32> execute(const std::vector<float>& input) const {
        std::vector<Complex32> out(len_ / 2 + 1);
        check(gm_rfft_f32(len_, input.data(), reinterpret_cast<gm_c32*>(out.data())), "RealFFT::execute");
        return out;
    }
};

}  // namespace gnss
