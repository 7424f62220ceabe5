// host_stages.cpp — runs the classes and methods of gnss-sdr-rs_amd/host/gnss_sdr.hpp that tests/cpp/test_host_api.cpp does not reach,
// one operation per process, so that tests/test_gpu_cpp_host_stages.py can hold every word a wrapper returns to the Python layer's.
//
//   host_stages [--cpu-only] <operation> <case file> <result file>
//
// The case file is little-endian binary written by the test: the operation's settings (uint32 / uint64 / float / double), then a step
// count and the steps, each a uint32 code, its arguments and its input arrays.  A code with bit 15 set is a step that must be refused:
// its gnss::Panic is caught there and its status recorded, and the steps go on (the handle must be as it was).  The result file is a
// list of records (uint32 tag length, tag, uint64 byte count, bytes), in the order the wrappers returned them.  Any other gnss::Panic
// ends the run in main: status and text go to the result file and the exit status is 3.  Only the C++ classes are called here — a
// gm_* call would bypass the wrapper under test.  Every buffer handed to a _dev method lies between two 64-byte guards of 0x5A.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include <hip/hip_runtime_api.h>

#include "gnss_sdr.hpp"

using gnss::Complex32;

namespace {

struct In {
    std::vector<uint8_t> b;
    size_t at = 0;
    void need(size_t n) const { if (at + n > b.size()) throw std::runtime_error("case file too short"); }
    template <class T> T get() { T v; need(sizeof v); std::memcpy(&v, b.data() + at, sizeof v); at += sizeof v; return v; }
    uint32_t u32() { return get<uint32_t>(); }
    uint64_t u64() { return get<uint64_t>(); }
    float f32() { return get<float>(); }
    double f64() { return get<double>(); }
    template <class T> std::vector<T> vec(size_t n) {
        need(n * sizeof(T));
        std::vector<T> v(n);
        if (n) std::memcpy(static_cast<void*>(v.data()), b.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

struct Out {
    FILE* f = nullptr;
    void rec(const std::string& tag, const void* p, size_t nbytes) {
        const uint32_t tl = uint32_t(tag.size());
        const uint64_t nb = nbytes;
        std::fwrite(&tl, 4, 1, f); std::fwrite(tag.data(), 1, tl, f); std::fwrite(&nb, 8, 1, f);
        if (nbytes) std::fwrite(p, 1, nbytes, f);
    }
    template <class T> void vec(const std::string& tag, const std::vector<T>& v) { rec(tag, v.data(), v.size() * sizeof(T)); }
    void u64(const std::string& tag, uint64_t v) { rec(tag, &v, 8); }
    void u32(const std::string& tag, uint32_t v) { rec(tag, &v, 4); }
    void i32(const std::string& tag, int32_t v) { rec(tag, &v, 4); }
    void f32(const std::string& tag, float v) { rec(tag, &v, 4); }
};

void hip_ok(hipError_t e, const char* what) { if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); }

constexpr size_t GUARD = 64;
// n bytes of device memory between two guards; payload and guards start as 0x5A
struct DevBuf {
    uint8_t* base = nullptr;
    size_t n = 0;
    explicit DevBuf(size_t nbytes, const void* src = nullptr) : n(nbytes) {
        hip_ok(hipMalloc(reinterpret_cast<void**>(&base), n + 2 * GUARD), "hipMalloc");
        hip_ok(hipMemset(base, 0x5A, n + 2 * GUARD), "hipMemset");
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        if (src && n) hip_ok(hipMemcpy(base + GUARD, src, n, hipMemcpyHostToDevice), "hipMemcpy");
    }
    DevBuf(const DevBuf&) = delete;
    ~DevBuf() { if (base) (void)hipFree(base); }
    void* p(size_t byte_offset = 0) const { return base + GUARD + byte_offset; }
    std::vector<uint8_t> image() const {
        std::vector<uint8_t> v(n);
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        if (n) hip_ok(hipMemcpy(v.data(), base + GUARD, n, hipMemcpyDeviceToHost), "hipMemcpy");
        return v;
    }
    bool intact() const {
        uint8_t g[2 * GUARD];
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_ok(hipMemcpy(g, base, GUARD, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipMemcpy(g + GUARD, base + GUARD + n, GUARD, hipMemcpyDeviceToHost), "hipMemcpy");
        for (uint8_t v : g) if (v != 0x5A) return false;
        return true;
    }
    void dump(Out& out, const std::string& tag) const { out.vec(tag, image()); out.u32(tag + ".guards", intact() ? 1u : 0u); }
};

// the steps of a case: f(code) reads ALL of a step's arguments before it calls a wrapper, so that a refused step leaves the cursor
// behind its arguments
template <class F> void steps(In& in, Out& out, F&& f) {
    const uint32_t n = in.u32();
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t code = in.u32();
        const bool refuse = (code & 0x8000u) != 0;
        code &= 0x7FFFu;
        if (!refuse) { f(code); continue; }
        int32_t st = 0;
        try { f(code); } catch (const gnss::Panic& p) { st = p.status; }
        out.i32("refused", st);
    }
}

size_t bps(int fmt) { return fmt == GM_FMT_C32 ? 8 : fmt == GM_FMT_I8_IQ ? 2 : 1; }

enum : uint32_t {
    PROCESS = 1, PROCESS_DEV = 2, RESET = 3, STATS = 4, TAPS = 5, SYNC = 6, WRITE_RING = 7, RING_READ = 8,
    SET_GAINS = 10, GAINS = 11, ADAPT_DEV = 12, PSD = 13, SET_BLOCK_ADAPT = 14, CLEAR_BLOCK_ADAPT = 15, BLOCK_STATS = 16, BLOCK_CAPTURE = 17,
    SET_WEIGHTS = 20, SET_STEERING = 21, SET_CONSTRAINTS = 22, CAPTURE = 23, STATS_PLAIN = 24,
};

template <class S> bool common_step(S& s, uint32_t code, In& in, Out& out) {
    if (code == RESET) { const uint64_t at = in.u64(); s.reset(at); return true; }
    if (code == SYNC) { s.synchronize(); return true; }
    if (code == STATS) {
        uint64_t v[3] = {0, 0, 0};
        s.stats(&v[0], &v[1], &v[2]);
        out.rec("stats", v, sizeof v);
        return true;
    }
    return false;
}

// process / process_i8 of the three single-stream stages
template <class S> void stream_process(S& s, In& in, Out& out) {
    const int fmt = int(in.u32());
    const uint64_t n = in.u64();
    if (fmt == GM_FMT_C32) {
        const std::vector<Complex32> x = in.vec<Complex32>(n);
        out.vec("y", s.process(x));
    } else {
        const std::vector<int8_t> x = in.vec<int8_t>(2 * n);
        out.vec("y", s.process_i8(x.data(), n));
    }
}
template <class S> void stream_process_dev(S& s, In& in, Out& out) {
    const int fmt = int(in.u32());
    const uint64_t n = in.u64(), cap = in.u64();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n * bps(fmt));
    DevBuf d_in(x.size(), x.data()), d_out(cap * 8);
    const size_t got = s.process_dev(d_in.p(), fmt, n, d_out.p(), cap);
    s.synchronize();
    out.u64("got", got);
    d_out.dump(out, "dev");
    out.u32("in.guards", d_in.intact() && d_in.image() == x ? 1u : 0u);
}

void op_resampler(In& in, Out& out) {
    gm_resampler_cfg c{};
    c.up = in.u32(); c.down = in.u32(); c.taps = in.u32(); c.n_phases = in.u32();
    c.cutoff = in.f32(); c.kaiser_beta = in.f32(); c.blank_threshold = in.f32();
    const bool short_form = in.u32() != 0;
    std::unique_ptr<gnss::Resampler> r(short_form ? new gnss::Resampler(c.up, c.down, c.blank_threshold) : new gnss::Resampler(c));
    steps(in, out, [&](uint32_t code) {
        if (common_step(*r, code, in, out)) return;
        if (code == PROCESS) return stream_process(*r, in, out);
        if (code == PROCESS_DEV) return stream_process_dev(*r, in, out);
        if (code == TAPS) { std::vector<float> t(in.u64()); r->taps(t.data()); return out.vec("taps", t); }
        throw std::runtime_error("resampler: unknown step");
    });
}

void op_excisor(In& in, Out& out) {
    gm_excisor_cfg c{};
    c.block = in.u32(); c.guard_bins = in.u32(); c.threshold_factor = in.f32(); c.blank_threshold = in.f32();
    const bool short_form = in.u32() != 0;
    std::unique_ptr<gnss::Excisor> e(short_form ? new gnss::Excisor(c.block, c.guard_bins, c.blank_threshold) : new gnss::Excisor(c));
    out.u32("block", e->block());
    std::unique_ptr<DevBuf> d_power, d_mask;
    steps(in, out, [&](uint32_t code) {
        if (common_step(*e, code, in, out)) return;
        if (code == PROCESS) return stream_process(*e, in, out);
        if (code == PROCESS_DEV) return stream_process_dev(*e, in, out);
        if (code == SET_GAINS) { const std::vector<float> g = in.vec<float>(in.u32()); return e->set_gains(g); }
        if (code == GAINS) return out.vec("gains", e->gains());
        if (code == ADAPT_DEV) {
            const int fmt = int(in.u32());
            const uint64_t n = in.u64();
            const std::vector<uint8_t> x = in.vec<uint8_t>(n * bps(fmt));
            DevBuf d_in(x.size(), x.data());
            e->adapt_dev(d_in.p(), fmt, n);
            e->synchronize();
            return out.u32("in.guards", d_in.intact() ? 1u : 0u);
        }
        if (code == PSD) {
            float median = -1.0f; uint32_t flagged = ~0u, zeroed = ~0u;
            out.vec("psd", e->psd(&median, &flagged, &zeroed));
            out.f32("median", median); out.u32("n_flagged", flagged); out.u32("n_zeroed", zeroed);
            return out.vec("psd.alone", e->psd());
        }
        if (code == SET_BLOCK_ADAPT) { const float f = in.f32(); const uint32_t g = in.u32(); return e->set_block_adapt(f, g); }
        if (code == CLEAR_BLOCK_ADAPT) return e->clear_block_adapt();
        if (code == BLOCK_STATS) {
            uint64_t v[4] = {0, 0, 0, 0};
            e->block_stats(&v[0], &v[1], &v[2], &v[3]);
            uint64_t only = 0;
            e->block_stats(nullptr, nullptr, &only, nullptr);
            out.rec("block_stats", v, sizeof v);
            return out.u64("bins_flagged.alone", only);
        }
        if (code == BLOCK_CAPTURE) {       // cap_blocks > 0: arms it on buffers of the driver's; 0: disarms and writes what they hold
            const uint64_t cap = in.u64();
            if (cap) {
                d_power.reset(new DevBuf(cap * e->block() * 4)); d_mask.reset(new DevBuf(cap * e->block()));
                return e->block_capture(static_cast<float*>(d_power->p()), static_cast<uint8_t*>(d_mask->p()), cap);
            }
            e->block_capture(nullptr, nullptr, 0);
            e->synchronize();
            d_power->dump(out, "power"); d_mask->dump(out, "mask");
            return;
        }
        throw std::runtime_error("excisor: unknown step");
    });
}

void op_ddc(In& in, Out& out) {
    gm_ddc_cfg c{};
    c.mix_cycles_per_sample = in.f64(); c.up = in.u32(); c.down = in.u32(); c.taps = in.u32(); c.n_phases = in.u32();
    c.cutoff = in.f32(); c.kaiser_beta = in.f32(); c.blank_threshold = in.f32();
    const bool short_form = in.u32() != 0;
    std::unique_ptr<gnss::Ddc> d(short_form ? new gnss::Ddc(c.mix_cycles_per_sample, c.up, c.down, c.blank_threshold) : new gnss::Ddc(c));
    steps(in, out, [&](uint32_t code) {
        if (common_step(*d, code, in, out)) return;
        if (code == PROCESS) {
            const uint64_t n = in.u64();
            const std::vector<int8_t> x = in.vec<int8_t>(n);
            return out.vec("y", d->process(x.data(), n));
        }
        if (code == PROCESS_DEV) {          // the input at any byte address
            const uint64_t n = in.u64(), cap = in.u64();
            const uint32_t offset = in.u32();
            std::vector<uint8_t> x(offset, 0);
            const std::vector<uint8_t> body = in.vec<uint8_t>(n);
            x.insert(x.end(), body.begin(), body.end());
            DevBuf d_in(x.size(), x.data()), d_out(cap * 8);
            const size_t got = d->process_dev(d_in.p(offset), n, d_out.p(), cap);
            d->synchronize();
            out.u64("got", got);
            d_out.dump(out, "dev");
            return out.u32("in.guards", d_in.intact() && d_in.image() == x ? 1u : 0u);
        }
        if (code == TAPS) {
            std::vector<float> t(in.u64()), alone(t.size());
            const uint64_t phasors = in.u64();
            std::vector<Complex32> whi(phasors), wlo(phasors), whi2(phasors);
            d->tables(t.data(), whi.data(), wlo.data());
            d->tables(alone.data(), nullptr, nullptr);
            d->tables(nullptr, whi2.data(), nullptr);
            out.vec("taps", t); out.vec("whi", whi); out.vec("wlo", wlo); out.vec("taps.alone", alone);
            return out.vec("whi.alone", whi2);
        }
        throw std::runtime_error("ddc: unknown step");
    });
}

void op_channelizer(In& in, Out& out) {
    gm_channelizer_cfg c{};
    c.n_channels = in.u32(); c.decim = in.u32(); c.taps_per_branch = in.u32();
    c.cutoff = in.f32(); c.kaiser_beta = in.f32(); c.blank_threshold = in.f32();
    const bool short_form = in.u32() != 0;
    const bool glonass = in.u32() != 0;         // the listed channels are Channelizer::glonass_channels(n_channels)
    std::vector<uint32_t> list = in.vec<uint32_t>(in.u32());
    if (glonass) list = gnss::Channelizer::glonass_channels(c.n_channels);
    c.n_out_channels = uint32_t(list.size()); c.out_channels = list.empty() ? nullptr : list.data();
    std::unique_ptr<gnss::Channelizer> ch(short_form ? new gnss::Channelizer(c.n_channels, c.decim, list, c.blank_threshold)
                                                     : new gnss::Channelizer(c));
    out.u32("planes", ch->planes());
    steps(in, out, [&](uint32_t code) {
        if (common_step(*ch, code, in, out)) return;
        if (code == PROCESS) {
            const int fmt = int(in.u32());
            const uint64_t n = in.u64();
            const std::vector<uint8_t> x = in.vec<uint8_t>(n * bps(fmt));
            size_t n_out = ~size_t(0);
            out.vec("y", ch->process(x.data(), fmt, n, &n_out));
            return out.u64("n_out", n_out);
        }
        if (code == PROCESS_DEV) {
            const int fmt = int(in.u32());
            const uint64_t n = in.u64(), stride = in.u64(), cap = in.u64();
            const std::vector<uint8_t> x = in.vec<uint8_t>(n * bps(fmt));
            DevBuf d_in(x.size(), x.data()), d_out(size_t(ch->planes()) * stride * 8);
            const size_t got = ch->process_dev(d_in.p(), fmt, n, d_out.p(), stride, cap);
            ch->synchronize();
            out.u64("got", got);
            d_out.dump(out, "dev");
            return out.u32("in.guards", d_in.intact() && d_in.image() == x ? 1u : 0u);
        }
        if (code == TAPS) return out.vec("taps", ch->taps());
        throw std::runtime_error("channelizer: unknown step");
    });
}

// ---- the array stages.  process: the flags say which of R and w are asked for; capture: cap_blocks > 0 arms it on buffers of the
// driver's, 0 disarms it and writes what they hold.
struct Captured {
    std::unique_ptr<DevBuf> R, w;
    template <class S> void step(S& s, In& in, Out& out, size_t R_words, size_t w_words) {
        const uint64_t cap = in.u64();
        if (cap) {
            R.reset(new DevBuf(cap * R_words * 8)); w.reset(new DevBuf(cap * w_words * 8));
            return s.capture(R->p(), w->p(), cap);
        }
        s.capture(nullptr, nullptr, 0);
        s.synchronize();
        R->dump(out, "cap.R"); w->dump(out, "cap.w");
    }
};

template <class S> void array_process(S& s, In& in, Out& out, uint32_t antennas) {     // Nuller, Stap: one stream out
    const int fmt = int(in.u32());
    const uint64_t n = in.u64();
    const uint32_t want = in.u32();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n * antennas * bps(fmt));
    std::vector<Complex32> R{Complex32(7, 7)}, w{Complex32(7, 7)};
    out.vec("y", s.process(x.data(), fmt, n, (want & 1) ? &R : nullptr, (want & 2) ? &w : nullptr));
    if (want & 1) out.vec("R", R);
    if (want & 2) out.vec("w", w);
}
template <class S> void array_process_dev(S& s, In& in, Out& out, uint32_t antennas) {
    const int fmt = int(in.u32());
    const uint64_t n = in.u64(), cap = in.u64();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n * antennas * bps(fmt));
    DevBuf d_in(x.size(), x.data()), d_out(cap * 8);
    const size_t got = s.process_dev(d_in.p(), fmt, n, d_out.p(), cap);
    s.synchronize();
    out.u64("got", got);
    d_out.dump(out, "dev");
    out.u32("in.guards", d_in.intact() && d_in.image() == x ? 1u : 0u);
}
template <class S> void beams_process(S& s, In& in, Out& out) {                         // Beamformer, Lcmv: a plane a beam
    const int fmt = int(in.u32());
    const uint64_t n = in.u64();
    const uint32_t want = in.u32();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n * s.antennas() * bps(fmt));
    std::vector<Complex32> R{Complex32(7, 7)}, w{Complex32(7, 7)};
    size_t n_out = ~size_t(0);
    out.vec("y", s.process(x.data(), fmt, n, (want & 4) ? &n_out : nullptr, (want & 1) ? &R : nullptr, (want & 2) ? &w : nullptr));
    if (want & 4) out.u64("n_out", n_out);
    if (want & 1) out.vec("R", R);
    if (want & 2) out.vec("w", w);
}
template <class S> void beams_process_dev(S& s, In& in, Out& out) {                     // planes `stride` words apart
    const int fmt = int(in.u32());
    const uint64_t n = in.u64(), stride = in.u64();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n * s.antennas() * bps(fmt));
    DevBuf d_in(x.size(), x.data()), d_out(size_t(s.beams()) * stride * 8);
    const size_t got = s.process_dev(d_in.p(), fmt, n, d_out.p(), stride);
    s.synchronize();
    out.u64("got", got);
    d_out.dump(out, "dev");
    out.u32("in.guards", d_in.intact() && d_in.image() == x ? 1u : 0u);
}
template <class S> void beams_stats(S& s, uint32_t code, Out& out) {
    uint64_t v[3] = {0, 0, 0};
    if (code == STATS_PLAIN) { s.stats(&v[0], &v[1], &v[2]); return out.rec("stats", v, sizeof v); }
    std::vector<uint64_t> fb{99};
    s.stats(&v[0], &v[1], &v[2], &fb);
    out.rec("stats", v, sizeof v);
    out.vec("fallbacks", fb);
}

void op_nuller(In& in, Out& out) {
    const uint32_t A = in.u32(), block = in.u32();
    const float loading = in.f32();
    const std::vector<Complex32> s = in.vec<Complex32>(in.u32());
    gnss::Nuller nl(A, block, loading, s);
    out.u32("block", nl.block()); out.u32("antennas", nl.antennas());
    Captured cap;
    steps(in, out, [&](uint32_t code) {
        if (common_step(nl, code, in, out)) return;
        if (code == PROCESS) return array_process(nl, in, out, A);
        if (code == PROCESS_DEV) return array_process_dev(nl, in, out, A);
        if (code == SET_WEIGHTS) { const std::vector<Complex32> w = in.vec<Complex32>(in.u32()); return nl.set_weights(w); }
        if (code == CAPTURE) return cap.step(nl, in, out, size_t(A) * A, A);
        throw std::runtime_error("nuller: unknown step");
    });
}

void op_stap(In& in, Out& out) {
    const uint32_t A = in.u32(), L = in.u32(), block = in.u32();
    const float loading = in.f32();
    const std::vector<Complex32> s = in.vec<Complex32>(in.u32());
    gnss::Stap st(A, L, block, loading, s);
    out.u32("block", st.block()); out.u32("weights", st.weights()); out.u32("antennas", st.antennas()); out.u32("taps", st.taps());
    const size_t M = st.weights();
    Captured cap;
    steps(in, out, [&](uint32_t code) {
        if (code == RESET || code == SYNC) { common_step(st, code, in, out); return; }
        if (code == STATS || code == STATS_PLAIN) {
            uint64_t v[4] = {0, 0, 0, 0};
            if (code == STATS) st.stats(&v[0], &v[1], &v[2], &v[3]); else st.stats(&v[0], &v[1], &v[2]);
            return out.rec("stats", v, code == STATS ? 32 : 24);
        }
        if (code == PROCESS) return array_process(st, in, out, A);
        if (code == PROCESS_DEV) return array_process_dev(st, in, out, A);
        if (code == SET_WEIGHTS) { const std::vector<Complex32> w = in.vec<Complex32>(in.u32()); return st.set_weights(w); }
        if (code == CAPTURE) return cap.step(st, in, out, M * M, M);
        throw std::runtime_error("stap: unknown step");
    });
}

void op_beamformer(In& in, Out& out) {
    const uint32_t A = in.u32(), L = in.u32(), block = in.u32();
    const float loading = in.f32();
    const std::vector<Complex32> s = in.vec<Complex32>(in.u32());
    gnss::Beamformer bf(A, L, s, block, loading);
    out.u32("block", bf.block()); out.u32("weights", bf.weights()); out.u32("beams", bf.beams());
    const size_t M = bf.weights(), P = bf.beams();
    Captured cap;
    steps(in, out, [&](uint32_t code) {
        if (code == RESET || code == SYNC) { common_step(bf, code, in, out); return; }
        if (code == STATS || code == STATS_PLAIN) return beams_stats(bf, code, out);
        if (code == PROCESS) return beams_process(bf, in, out);
        if (code == PROCESS_DEV) return beams_process_dev(bf, in, out);
        if (code == SET_WEIGHTS) { const std::vector<Complex32> w = in.vec<Complex32>(in.u32()); return bf.set_weights(w); }
        if (code == SET_STEERING) { const uint32_t beam = in.u32(); const std::vector<Complex32> r = in.vec<Complex32>(in.u32()); return bf.set_steering(beam, r); }
        if (code == CAPTURE) return cap.step(bf, in, out, M * M, P * M);
        throw std::runtime_error("beamformer: unknown step");
    });
}

gnss::Lcmv::Beam read_beam(In& in) {
    gnss::Lcmv::Beam b;
    b.rows = in.vec<Complex32>(in.u32());
    b.f = in.vec<Complex32>(in.u32());
    return b;
}

void op_lcmv(In& in, Out& out) {
    const uint32_t A = in.u32(), L = in.u32(), block = in.u32();
    const float loading = in.f32();
    std::vector<gnss::Lcmv::Beam> beams(in.u32());
    for (auto& b : beams) b = read_beam(in);
    gnss::Lcmv lc(A, L, beams, block, loading);
    out.u32("block", lc.block()); out.u32("weights", lc.weights()); out.u32("beams", lc.beams());
    const size_t M = lc.weights(), P = lc.beams();
    Captured cap;
    steps(in, out, [&](uint32_t code) {
        if (code == RESET || code == SYNC) { common_step(lc, code, in, out); return; }
        if (code == STATS || code == STATS_PLAIN) return beams_stats(lc, code, out);
        if (code == PROCESS) return beams_process(lc, in, out);
        if (code == PROCESS_DEV) return beams_process_dev(lc, in, out);
        if (code == SET_WEIGHTS) { const std::vector<Complex32> w = in.vec<Complex32>(in.u32()); return lc.set_weights(w); }
        if (code == SET_CONSTRAINTS) { const uint32_t beam = in.u32(); const gnss::Lcmv::Beam b = read_beam(in); return lc.set_constraints(beam, b); }
        if (code == CAPTURE) return cap.step(lc, in, out, M * M, P * M);
        throw std::runtime_error("lcmv: unknown step");
    });
}

// ---- the ring writers: Ddc::write_ring and the resampled and conditioned DigitalFrontend::write_ring / write_ring_i8 overloads
void op_ring(In& in, Out& out) {
    gnss::MulticastRingBuffer ring(in.u64());
    const uint32_t source = in.u32();           // 0: a Ddc, 1: a DigitalFrontend
    std::unique_ptr<gnss::Ddc> ddc;
    std::unique_ptr<gnss::DigitalFrontend> fe;
    if (source == 0) {
        const double mix = in.f64(); const uint32_t up = in.u32(), down = in.u32(); const float blank = in.f32();
        ddc.reset(new gnss::Ddc(mix, up, down, blank));
    } else {
        const float f_if = in.f32(), fs_in = in.f32(), fs_out = in.f32();
        fe.reset(new gnss::DigitalFrontend(f_if, fs_in, fs_out));
    }
    std::unique_ptr<gnss::Excisor> ex;
    std::unique_ptr<gnss::Resampler> rs;
    if (const uint32_t block = in.u32()) {
        ex.reset(new gnss::Excisor(block));
        ex->set_gains(in.vec<float>(block));
    }
    const uint32_t up = in.u32(), down = in.u32();
    if (up) rs.reset(new gnss::Resampler(up, down));
    steps(in, out, [&](uint32_t code) {
        if (code == WRITE_RING) {
            const int fmt = int(in.u32());
            const uint64_t n = in.u64();
            const std::vector<uint8_t> x = in.vec<uint8_t>(n * bps(fmt));
            uint64_t total = 0;
            if (ddc) total = ddc->write_ring(ring, reinterpret_cast<const int8_t*>(x.data()), n, ex.get(), rs.get());
            else if (fmt == GM_FMT_C32 && ex) total = fe->write_ring(ring, reinterpret_cast<const Complex32*>(x.data()), n, *ex, rs.get());
            else if (fmt == GM_FMT_C32) total = fe->write_ring(ring, reinterpret_cast<const Complex32*>(x.data()), n, *rs);
            else if (ex) total = fe->write_ring_i8(ring, reinterpret_cast<const int8_t*>(x.data()), n, *ex, rs.get());
            else total = fe->write_ring_i8(ring, reinterpret_cast<const int8_t*>(x.data()), n, *rs);
            out.u64("total", total);
            return out.u64("enqueued", ring.get_enqueued_head());
        }
        if (code == RING_READ) {
            const uint64_t start = in.u64(), n = in.u64();
            ring.flush();
            out.u64("head", ring.get_head());
            std::vector<Complex32> words(n);
            ring.copy_to_slice(start, words);
            return out.vec("ring", words);
        }
        if (code == STATS) {
            uint64_t v[9] = {0};
            if (ddc) ddc->stats(&v[0], &v[1], &v[2]);
            if (ex) ex->stats(&v[3], &v[4], &v[5]);
            if (rs) rs->stats(&v[6], &v[7], &v[8]);
            return out.rec("stats", v, sizeof v);
        }
        throw std::runtime_error("ring: unknown step");
    });
}

// ---- re-steering on the device: R captured from a Stap, solve_plan, solve_rows_dev without and with R, and Beamformer::set_steering_dev
// without d_info and with it under a min_ratio; a process call behind each install shows which rows the beams use
void op_resteer(In& in, Out& out) {
    const uint32_t A = in.u32(), L = in.u32(), block = in.u32(), n = in.u32();
    const float loading = in.f32(), min_ratio = in.f32();
    const std::vector<Complex32> steering = in.vec<Complex32>(in.u32());
    const std::vector<uint8_t> z = in.vec<uint8_t>(in.u64() * 8), x = in.vec<uint8_t>(in.u64() * 8);
    const uint32_t M = A * L, P = uint32_t(steering.size() / M);
    const size_t n_time = x.size() / 8 / A, half = n_time / 2;
    DevBuf d_x(x.size(), x.data()), d_z(z.size(), z.data());
    DevBuf d_R(2 * size_t(M) * M * 8), d_w(2 * size_t(M) * 8), d_y(n_time * 8 + size_t(block) * 8);
    {
        gnss::Stap st(A, L, block);
        st.capture(d_R.p(), d_w.p(), 2);
        out.u64("stap.got", st.process_dev(d_x.p(), GM_FMT_C32, half, d_y.p(), half + block));
        st.synchronize();
        st.capture(nullptr, nullptr, 0);
        d_R.dump(out, "R");
    }
    gm_array_solve_cfg c{};
    c.m = M; c.n = n; c.n_rows = P; c.loading = loading;
    DevBuf rows0(size_t(P) * M * 8), info0(size_t(P) * sizeof(gm_array_row_info)), rows1(size_t(P) * M * 8), info1(size_t(P) * sizeof(gm_array_row_info));
    gnss::SolveExtents e = gnss::solve_plan(c);
    gnss::solve_rows_dev(c, d_z.p(), nullptr, rows0.p(), info0.p());
    c.n_blocks = 2;
    const gnss::SolveExtents e2 = gnss::solve_plan(c);
    const uint64_t ext[6] = {e.z_words, e.R_words, e.row_words, e2.z_words, e2.R_words, e2.row_words};
    out.rec("extents", ext, sizeof ext);
    gnss::solve_rows_dev(c, d_z.p(), d_R.p(), rows1.p(), info1.p(), nullptr);
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    rows0.dump(out, "rows0"); info0.dump(out, "info0"); rows1.dump(out, "rows1"); info1.dump(out, "info1");
    gnss::Beamformer bf(A, L, steering, block);
    const uint8_t* tail = x.data() + half * A * 8;
    const auto run = [&](const char* tag) {
        std::vector<Complex32> R, w;
        size_t n_out = 0;
        out.vec(std::string(tag) + ".y", bf.process(tail, GM_FMT_C32, n_time - half, &n_out, &R, &w));
        out.u64(std::string(tag) + ".n_out", n_out);
        out.vec(std::string(tag) + ".w", w);
        bf.reset(0);
    };
    run("before");
    DevBuf installed(P), gated(P);
    bf.set_steering_dev(0, P, rows1.p());                                   // every default: no info, no gate, no flags
    run("plain");
    bf.set_steering_dev(0, P, rows1.p(), nullptr, 0.0f, installed.p());
    bf.synchronize();
    installed.dump(out, "installed");
    bf.set_steering_dev(0, P, rows0.p(), info0.p(), min_ratio, gated.p(), nullptr);
    bf.synchronize();
    gated.dump(out, "gated");
    run("gated");
    out.u32("in.guards", d_x.intact() && d_z.intact() && d_x.image() == x && d_z.image() == z ? 1u : 0u);
}

// ---- AcquisitionEngine beyond search / finer_doppler, and the constraint rows solved from its array_prompts words
struct AcqWords { uint64_t prn, code_phase_samples; float code_phase_chips, carrier_freq, fs, mag_relative; uint64_t sample_global_index; int32_t doppler_bin; uint32_t found; };
using AcqResults = std::vector<std::optional<gnss::AcquisitionResult>>;
void put_results(Out& out, const std::string& tag, const AcqResults& r) {
    std::vector<AcqWords> w(r.size());
    for (size_t i = 0; i < r.size(); ++i) {
        std::memset(static_cast<void*>(&w[i]), 0, sizeof w[i]);
        if (!r[i]) continue;
        w[i].prn = r[i]->prn; w[i].code_phase_samples = r[i]->code_phase_samples; w[i].code_phase_chips = r[i]->code_phase_chips;
        w[i].carrier_freq = r[i]->carrier_freq; w[i].fs = r[i]->fs; w[i].mag_relative = r[i]->mag_relative;
        w[i].sample_global_index = r[i]->sample_global_index; w[i].doppler_bin = r[i]->doppler_bin; w[i].found = 1;
    }
    out.vec(tag, w);
}
// the first `keep` bytes of every struct: what lies behind them is padding or a reserved word
template <class T> void put_structs(Out& out, const std::string& tag, const std::vector<T>& v, size_t keep) {
    std::vector<uint8_t> b;
    for (const T& e : v) { const uint8_t* p = reinterpret_cast<const uint8_t*>(&e); b.insert(b.end(), p, p + keep); }
    out.vec(tag, b);
}

void op_acquisition(In& in, Out& out) {
    const float fs = in.f32(), f_if = in.f32();
    const uint32_t N = in.u32();
    const std::vector<float> doppler = in.vec<float>(in.u32());
    const std::vector<uint8_t> prns = in.vec<uint8_t>(in.u32());
    const uint32_t M = in.u32();
    const float threshold = in.f32();
    const uint32_t K = in.u32(), from_tables = in.u32();
    std::unique_ptr<gnss::AcquisitionEngine> eng;
    if (from_tables) {
        std::vector<gnss::DopplerShiftTable> tables;
        for (float d : doppler) tables.emplace_back(f_if, d, fs, size_t(N));
        eng.reset(new gnss::AcquisitionEngine(fs, N, tables, prns, M, true));
    } else {
        eng.reset(new gnss::AcquisitionEngine(fs, f_if, N, doppler, prns, M, threshold, GM_DECIDE_REFERENCE, true, K));
    }
    AcqResults last;
    std::vector<gm_c32> z;                     // the last array_prompts words
    uint32_t z_cands = 0, z_periods = 0, z_m = 0;
    const auto read_dwell = [&](std::unique_ptr<DevBuf>& d, int& fmt, std::vector<uint8_t>& x, uint32_t width) {
        const uint32_t on_device = in.u32();
        fmt = int(in.u32());
        x = in.vec<uint8_t>(in.u64() * width * bps(fmt));
        if (on_device) d.reset(new DevBuf(x.size(), x.data()));
    };
    steps(in, out, [&](uint32_t code) {
        if (code == 1) {                        // search / search_i8
            const int fmt = int(in.u32());
            const uint64_t n = in.u64(), tail = in.u64(), mask = in.u64();
            if (fmt == GM_FMT_C32) { const std::vector<Complex32> x = in.vec<Complex32>(n); last = eng->search(x, tail, mask); }
            else { const std::vector<int8_t> x = in.vec<int8_t>(2 * n); last = eng->search_i8(x, tail, mask); }
            return put_results(out, "results", last);
        }
        if (code == 3) {                        // refine_doppler, with entry `drop` taken as not found
            gm_acq_refine_cfg c{};
            c.span_periods = in.u32(); c.n_freq = in.u32(); c.half_span_hz = in.f32();
            const uint32_t drop = in.u32();
            AcqResults r = last;
            if (drop < r.size()) r[drop].reset();
            const auto o = c.span_periods || c.n_freq || c.half_span_hz != 0.0f ? eng->refine_doppler(r, c) : eng->refine_doppler(r);
            std::vector<uint8_t> found;
            std::vector<gm_acq_refine_out> v;
            for (const auto& e : o) { found.push_back(e ? 1 : 0); if (e) v.push_back(*e); }
            out.vec("refine.found", found);
            return put_structs(out, "refine", v, sizeof(gm_acq_refine_out));
        }
        if (code == 4) {                        // local_search on the snapshot or on a device dwell
            const std::vector<gm_acq_cand> cands = in.vec<gm_acq_cand>(in.u32());
            gm_acq_local_cfg c{};
            c.lag_half_window = in.u32(); c.span_periods = in.u32(); c.n_freq = in.u32(); c.half_span_hz = in.f32();
            std::unique_ptr<DevBuf> d; int fmt = 0; std::vector<uint8_t> x;
            read_dwell(d, fmt, x, 1);
            put_structs(out, "local", d ? eng->local_search(cands, c, d->p(), fmt) : eng->local_search(cands, c), 84);
            return out.u32("in.guards", !d || (d->intact() && d->image() == x) ? 1u : 0u);
        }
        if (code == 5) {                        // array_prompts
            const std::vector<gm_acq_cand> cands = in.vec<gm_acq_cand>(in.u32());
            const uint32_t A = in.u32(), L = in.u32();
            std::unique_ptr<DevBuf> d; int fmt = 0; std::vector<uint8_t> x;
            read_dwell(d, fmt, x, A);
            uint32_t periods = 0;
            z = eng->array_prompts(cands, d->p(), A, L, fmt, &periods);
            z_cands = uint32_t(cands.size()); z_periods = periods; z_m = A * L;
            out.vec("z", z); out.u32("periods", periods);
            return out.u32("in.guards", d->intact() && d->image() == x ? 1u : 0u);
        }
        if (code == 6) {                        // cancel into a device buffer of dwell_samples() words
            const std::vector<gm_acq_cancel_cand> cands = in.vec<gm_acq_cancel_cand>(in.u32());
            std::unique_ptr<DevBuf> d; int fmt = 0; std::vector<uint8_t> x;
            read_dwell(d, fmt, x, 1);
            DevBuf d_out(size_t(eng->dwell_samples()) * 8);
            put_structs(out, "cancel", d ? eng->cancel(cands, d_out.p(), d->p(), fmt) : eng->cancel(cands, d_out.p()), 28);
            d_out.dump(out, "cancel.out");
            return out.u32("in.guards", !d || (d->intact() && d->image() == x) ? 1u : 0u);
        }
        if (code == 7) {
            const std::vector<uint32_t> off = in.vec<uint32_t>(in.u32());
            const std::vector<int8_t> sec = in.vec<int8_t>(in.u32());
            return sec.empty() ? eng->set_edge_search(off) : eng->set_edge_search(off, sec);
        }
        if (code == 8) { const std::vector<double> t = in.vec<double>(in.u32()); return eng->set_code_drift(t); }
        if (code == 9) return out.u64("dwell_samples", eng->dwell_samples());
        if (code == 10) return out.vec("edge_offset_periods", eng->edge_offset_periods(last));
        if (code == 11) {                       // the last array_prompts words -> solve_row per candidate and solve_rows_dev for all of them
            const float loading = in.f32();
            const size_t words = size_t(z_periods) * z_m;
            for (uint32_t c = 0; c < z_cands; ++c) {
                gm_array_row_info info{};
                out.vec("row", gnss::solve_row(z_m, std::vector<gm_c32>(z.begin() + c * words, z.begin() + (c + 1) * words), {}, loading, &info));
                out.rec("lambda", &info.lambda1, 16); out.u32("ref_index", info.ref_index);
            }
            gm_array_solve_cfg cfg{};
            cfg.m = z_m; cfg.n = z_periods; cfg.n_rows = z_cands; cfg.loading = loading;
            DevBuf d_z(z.size() * 8, z.data()), rows(size_t(z_cands) * z_m * 8), info(size_t(z_cands) * sizeof(gm_array_row_info));
            gnss::solve_rows_dev(cfg, d_z.p(), nullptr, rows.p(), info.p());
            hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
            rows.dump(out, "rows"); info.dump(out, "info");
            return out.u32("in.guards", d_z.intact() ? 1u : 0u);
        }
        throw std::runtime_error("acquisition: unknown step");
    });
}

// ---- TrackingManager::bank, array_prompts and array_prompts_dev
void op_tracking(In& in, Out& out) {
    const float fs = in.f32();
    const uint32_t n_channels = in.u32();
    const int mode = int(in.u32());
    gnss::MulticastRingBuffer ring(in.u64());
    ring.write_samples(in.vec<Complex32>(in.u64()));
    const int fmt = int(in.u32());
    const uint64_t n_time = in.u64();
    const uint32_t A = in.u32();
    const std::vector<uint8_t> x = in.vec<uint8_t>(n_time * A * bps(fmt));
    DevBuf d_x(x.size(), x.data());
    gnss::TrackingManager mgr(fs, n_channels, mode);
    const auto read_records = [&](std::vector<gm_trk_state>& recs) {
        const uint32_t given = in.u32();
        recs = in.vec<gm_trk_state>(in.u32());
        return given != 0;
    };
    steps(in, out, [&](uint32_t code) {
        if (code == 1) {                        // start a channel
            const uint32_t ch = in.u32();
            const AcqWords w = in.get<AcqWords>();
            gnss::AcquisitionResult r{};
            r.prn = uint8_t(w.prn); r.code_phase_samples = w.code_phase_samples; r.code_phase_chips = w.code_phase_chips;
            r.carrier_freq = w.carrier_freq; r.fs = w.fs; r.mag_relative = w.mag_relative; r.sample_global_index = w.sample_global_index;
            r.doppler_bin = w.doppler_bin;
            return mgr.channels[ch].start(r);
        }
        if (code == 2) {                        // bank
            const std::vector<float> taps = in.vec<float>(in.u32()), offs = in.vec<float>(in.u32());
            std::vector<gm_trk_state> recs;
            const bool given = read_records(recs);
            const bool want_done = in.u32() != 0;
            std::vector<uint8_t> done{9};
            out.vec("bank", offs.empty() && !given && !want_done ? mgr.bank(ring, taps) : mgr.bank(ring, taps, offs, given ? &recs : nullptr, want_done ? &done : nullptr));
            if (want_done) out.vec("done", done);
            return;
        }
        if (code == 3 || code == 4) {           // array_prompts / array_prompts_dev
            const uint64_t first = in.u64(), n = in.u64();
            const uint32_t L = in.u32();
            const float tau = in.f32();
            std::vector<gm_trk_state> recs;
            const bool given = read_records(recs);
            const bool want_done = in.u32() != 0;
            if (code == 3) {
                std::vector<uint8_t> done{9};
                out.vec("z", mgr.array_prompts(d_x.p(), fmt, first, n, A, L, tau, given ? &recs : nullptr, want_done ? &done : nullptr));
                if (want_done) out.vec("done", done);
            } else {
                DevBuf d_z(recs.size() * L * A * 8), d_done(recs.size());
                mgr.array_prompts_dev(d_x.p(), fmt, first, n, A, L, tau, recs, d_z.p(), d_done.p());
                hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
                d_z.dump(out, "z.dev"); d_done.dump(out, "done.dev");
            }
            return out.u32("in.guards", d_x.intact() && d_x.image() == x ? 1u : 0u);
        }
        throw std::runtime_error("tracking: unknown step");
    });
}

void op_fft(In& in, Out& out) {
    const uint64_t len = in.u64();
    const uint32_t batch = in.u32();
    std::vector<Complex32> x = in.vec<Complex32>(len * batch), one = in.vec<Complex32>(len);
    const std::vector<float> real = in.vec<float>(len);
    gnss::FFT fft(len);
    out.vec("execute", fft.execute(x));
    out.vec("execute.in_place", x);
    out.vec("power_spectrum", fft.power_spectrum(one));
    out.vec("rfft", gnss::RealFFT(len).execute(real));
}

// ---- host only
void op_plans(In& in, Out& out) {
    steps(in, out, [&](uint32_t code) {
        if (code == 1) {                    // Ddc::plan
            gm_ddc_cfg c{};
            c.mix_cycles_per_sample = in.f64(); c.up = in.u32(); c.down = in.u32(); c.taps = in.u32(); c.n_phases = in.u32();
            c.cutoff = in.f32(); c.kaiser_beta = in.f32(); c.blank_threshold = in.f32();
            const uint64_t so_far = in.u64(), n_in = in.u64();
            uint64_t inc = 0;
            const uint64_t n = gnss::Ddc::plan(c, so_far, n_in, &inc);
            out.u64("n_out", n); out.u64("phase_inc", inc);
            return out.u64("n_out.alone", gnss::Ddc::plan(c, so_far, n_in));
        }
        gm_trk_cfg trk{};
        std::vector<int8_t> dummy;
        const auto read_trk = [&] {
            trk.fs = in.f32(); trk.n_channels = 1; trk.nominal_code_rate = in.f32();
            if (const uint32_t code_len = in.u32()) {
                dummy.assign(code_len, 1);
                trk.codes = dummy.data(); trk.n_codes = 1; trk.code_len = code_len;
            }
        };
        if (code == 2) {                    // TrackingManager::bank_plan
            read_trk();
            const std::vector<float> taps = in.vec<float>(in.u32()), offsets = in.vec<float>(in.u32());
            const uint32_t n_states = in.u32();
            const gm_trk_bank_plan_out p = gnss::TrackingManager::bank_plan(trk, taps, offsets, n_states);
            const uint64_t v[6] = {p.n_taps, p.n_offsets, p.out_words, p.samples, p.slices, p.tap_groups};
            return out.rec("bank_plan", v, sizeof v);
        }
        if (code == 3) {                    // TrackingManager::array_plan
            read_trk();
            const uint32_t A = in.u32(), L = in.u32(); const float tap_chips = in.f32(); const uint32_t n_states = in.u32();
            const gm_trk_array_plan_out p = gnss::TrackingManager::array_plan(trk, A, L, tap_chips, n_states);
            const uint64_t v[4] = {p.words_per_record, p.out_words, p.samples, p.slices};
            return out.rec("array_plan", v, sizeof v);
        }
        if (code == 4) {                    // solve_plan
            gm_array_solve_cfg c{};
            c.m = in.u32(); c.n = in.u32(); c.n_rows = in.u32(); c.n_blocks = in.u32();
            c.row_stride = in.u64(); c.vec_stride = in.u64(); c.loading = in.f32();
            const gnss::SolveExtents e = gnss::solve_plan(c);
            const uint64_t v[3] = {e.z_words, e.R_words, e.row_words};
            return out.rec("solve_plan", v, sizeof v);
        }
        throw std::runtime_error("plans: unknown step");
    });
}

void op_solve_row(In& in, Out& out) {
    steps(in, out, [&](uint32_t) {
        const uint32_t m = in.u32();
        const std::vector<gm_c32> z = in.vec<gm_c32>(in.u64()), R = in.vec<gm_c32>(in.u64());
        const float loading = in.f32();
        const bool with_info = in.u32() != 0;
        gm_array_row_info info{};
        const std::vector<gm_c32> row = with_info ? gnss::solve_row(m, z, R, loading, &info) : gnss::solve_row(m, z, R, loading);
        out.vec("row", row);
        if (with_info) { out.rec("lambda", &info.lambda1, 16); out.u32("ref_index", info.ref_index); }
    });
}

void op_glonass(In& in, Out& out) {
    out.vec("code", gnss::Channelizer::glonass_code());
    const uint32_t n = in.u32();
    for (uint32_t i = 0; i < n; ++i) out.vec("channels", gnss::Channelizer::glonass_channels(in.u32()));
}

// one constructor that the library's plan must refuse (host only: the plan runs before the device is touched); the Panic ends in main
void op_refuse(In& in, Out& out) {
    const uint32_t cls = in.u32();
    const uint32_t a = in.u32(), b = in.u32(), c = in.u32(), d = in.u32();
    const std::vector<Complex32> words = in.vec<Complex32>(in.u32());
    switch (cls) {
    case 0: { gnss::Resampler x(a, b); break; }
    case 1: { gnss::Excisor x(a, b); break; }
    case 2: { gnss::Ddc x(0.25, a, b); break; }
    case 3: { gnss::Channelizer x(a, b); break; }
    case 4: { gnss::Nuller x(a, b, 0.0f, words); break; }
    case 5: { gnss::Stap x(a, b, c, 0.0f, words); break; }
    case 6: { gnss::Beamformer x(a, b, words, c); break; }
    case 7: {
        std::vector<gnss::Lcmv::Beam> beams(d);
        for (auto& beam : beams) { beam.rows = words; beam.f.assign((a && b) ? words.size() / (size_t(a) * b) : 0, Complex32(1, 0)); }
        gnss::Lcmv x(a, b, beams, c);
        break;
    }
    default: throw std::runtime_error("refuse: unknown class");
    }
    out.u32("constructed", 1);
}

struct Op { const char* name; void (*run)(In&, Out&); bool needs_device; };
const Op OPS[] = {
    {"resampler", op_resampler, true}, {"excisor", op_excisor, true}, {"ddc", op_ddc, true}, {"channelizer", op_channelizer, true},
    {"nuller", op_nuller, true}, {"stap", op_stap, true}, {"beamformer", op_beamformer, true}, {"lcmv", op_lcmv, true},
    {"ring", op_ring, true}, {"fft", op_fft, true}, {"resteer", op_resteer, true}, {"acquisition", op_acquisition, true}, {"tracking", op_tracking, true},
    {"plans", op_plans, false}, {"solve_row", op_solve_row, false}, {"glonass", op_glonass, false}, {"refuse", op_refuse, false},
};

}  // namespace

int main(int argc, char** argv) {
    bool cpu_only = false;
    std::vector<std::string> args;
    for (int i = 1; i < argc; ++i) { if (std::string(argv[i]) == "--cpu-only") cpu_only = true; else args.push_back(argv[i]); }
    if (args.size() != 3) { std::fprintf(stderr, "usage: host_stages [--cpu-only] <operation> <case file> <result file>\n"); return 2; }
    const Op* op = nullptr;
    for (const Op& o : OPS) if (args[0] == o.name) op = &o;
    if (!op) { std::fprintf(stderr, "host_stages: unknown operation %s\n", args[0].c_str()); return 2; }
    if (cpu_only && op->needs_device) { std::fprintf(stderr, "host_stages: %s needs a device\n", op->name); return 2; }
    In in;
    {
        std::ifstream f(args[1], std::ios::binary);
        if (!f) { std::fprintf(stderr, "host_stages: cannot read %s\n", args[1].c_str()); return 2; }
        in.b.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    Out out;
    out.f = std::fopen(args[2].c_str(), "wb");
    if (!out.f) { std::fprintf(stderr, "host_stages: cannot write %s\n", args[2].c_str()); return 2; }
    int rc = 0;
    try {
        if (!cpu_only) gnss::init(0);
        op->run(in, out);
        if (in.at != in.b.size()) throw std::runtime_error("case file longer than the operation reads");
        out.u32("end", 1);
    } catch (const gnss::Panic& p) {
        out.i32("panic", p.status);
        out.rec("panic.text", p.what(), std::strlen(p.what()));
        rc = 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "host_stages: %s\n", e.what());
        rc = 4;
    }
    std::fclose(out.f);
    return rc;
}
