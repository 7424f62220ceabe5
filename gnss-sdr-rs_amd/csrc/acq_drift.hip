// acq_drift.hip — stage F of a handle with code-drift compensation (gm_acq_set_code_drift): every code period of the dwell is read
// from where it really starts.
//
// Period p of the dwell, as Doppler bin d sees it, starts at sample s[d][p] = floor(p T_d + 0.5) (T_d: the bin's true code period in
// samples; the host plans the starts in f64).  Period k of group m of hypothesis h is the N samples from s[d][o_h + m K + k] on:
//     y_{h,d,m}[n] = sum_k sec[k] rho[h][d][m][k] x[s[d][o_h + m K + k] + n]
// with the phasor words continued to the real starts, rho = exp(-j 2 pi f_d (s[d][o_h+mK+k] - s[d][o_h+mK]) / fs).  These are the real
// samples at another place: no circular shift and no phase ramp.  K = 1 is the samples themselves (no fold, no product), so the words
// of a K = 1 handle are those of a plain search of the gathered samples.
//
// The three stage-F kernels are copies of acq_edge.hip's with DriftLoad in place of EdgeLoad, in a translation unit of their own for
// the reason given in acq_coherent.hip: every other code object stays exactly as it was.  One kernel per form serves K = 1 and K >= 2,
// the edge search on or off (offsets == null: one hypothesis at offset 0).  The spectra leave as [H D][M][.], so stage C and the
// reduction over the hypotheses run unchanged.
#include "acq_device.h"

namespace gm {

// the composite path's base plans run their correlation on these plans (as in acq_composite.hip): they fix the stored order
template <> struct CompPlanOf<Plan16368> { using type = AsPlain<Plan16368>; };
template <> struct CompPlanOf<Plan8184> { using type = AsPlain<Plan8184>; };
template <> struct CompPlanOf<Plan8192> { using type = Plan8192; };
#ifdef GM_COMP_PLAIN_16000
template <> struct CompPlanOf<Plan16000> { using type = Plan16000; };
#endif

namespace {

// Stage F's loader for one (h, d, m) item.  stage(): lane k copies period k's start (a 64-bit element offset) and its phasor word,
// with the secondary row's sign (bit k of neg set: -1, a negation: exact), into LDS; one barrier orders both before the first pass-0
// load.  The start words are uniform over the workgroup: they are read back through readfirstlane, so that the address of period k is
// a scalar base plus the lane's n.
struct DriftLoad {
    const void* samples; int fmt;
    uint32_t K; cf* rho_s; uint32_t* start_s;      // start_s: [K] {lo, hi}
    // starts_g: s[d][o_h + m K ..], rho_g: rho[h][d][m][..]
    __device__ __forceinline__ void stage(const uint64_t* __restrict__ starts_g, const cf* __restrict__ rho_g, uint32_t neg, int tid) const {
        if (uint32_t(tid) < K) {
            const uint64_t s = starts_g[tid];
            start_s[2 * tid] = uint32_t(s);
            start_s[2 * tid + 1] = uint32_t(s >> 32);
            const cf r = rho_g[tid];
            rho_s[tid] = ((neg >> tid) & 1u) ? cf_make(-r.x, -r.y) : r;
        }
        __syncthreads();
    }
    __device__ __forceinline__ size_t start(uint32_t k) const {
        const uint32_t lo = __builtin_amdgcn_readfirstlane(start_s[2 * k]), hi = __builtin_amdgcn_readfirstlane(start_s[2 * k + 1]);
        return size_t(lo) | (size_t(hi) << 32);
    }
    // element n of the item's folded period (fold_sample's arithmetic, acq_device.h: k ascending, every product and sum rounded on its own)
    __device__ __forceinline__ cf operator()(size_t n) const {
        cf s = load_sample(samples, fmt, start(0) + n);
        if (K == 1) return s;                      // the samples themselves: no product with (1, 0)
        cf r = rho_s[0];
        cf acc = cf_make(r.x * s.x - r.y * s.y, r.x * s.y + r.y * s.x);
        for (uint32_t k = 1; k < K; ++k) {
            s = load_sample(samples, fmt, start(k) + n);
            r = rho_s[k];
            acc = cf_make(acc.x + (r.x * s.x - r.y * s.y), acc.y + (r.x * s.y + r.y * s.x));
        }
        return acc;
    }
};

// ------------------------------------------------------------------------------------ in-LDS sizes (acq_mix_fft_kernel)
// one workgroup per (v, m), v = h D + d; no trailing decision workgroups (a drift handle decides at once)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void acq_mix_fft_drift_kernel(const void* __restrict__ samples, int fmt,
                                                                const uint64_t* __restrict__ starts, uint32_t R,
                                                                const cf* __restrict__ rho, uint32_t K,
                                                                const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                const cf* __restrict__ tables,
                                                                const cf* __restrict__ tw_fwd,
                                                                cf* __restrict__ spectra, int n_int,
                                                                uint32_t* __restrict__ clear_tickets,
                                                                const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    using CP = typename CorrPlanOf<PLX>::type;
    static_assert(PL::N == PLX::N, "the mix plan keeps the size");
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the starts");
    constexpr bool PERMUTED = CorrMode<CP>::PERMUTED;
    constexpr int STAGE = PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    __shared__ uint32_t start_s[2 * GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    const uint32_t v = blockIdx.x / uint32_t(n_int), m = blockIdx.x - v * uint32_t(n_int);   // virtual bin v = h D + d
    const uint32_t h = v / D, d = v - h * D;
    if (clear_tickets && blockIdx.x == 0)        // the tail split's tickets, as acq_mix_fft_kernel clears them
        for (int i = tid; i < GM_CORR_SPLIT_MAX_ITEMS; i += PL::T) clear_tickets[i] = 0u;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t o = offsets ? offsets[h] : 0u;
    const DriftLoad load{samples, fmt, K, rho_s, start_s};
    load.stage(starts + size_t(d) * R + o + size_t(m) * K, rho + size_t(blockIdx.x) * K, neg, tid);
    const cf* tab = tables + size_t(d) * PL::N;
    cf* dst = spectra + size_t(blockIdx.x) * PL::N;   // [v][m][k]
    constexpr int NB0 = PL::NB(0);
    auto in = [&](int it, int r) {
        const int idx = (tid + it * PL::T) + r * NB0;
        const cf s = load(size_t(idx));                                // group m folded over its K periods, each from its own start
        const cf t = tab[idx];
        // multiply_simd_block (doppler_shift.rs:43-58): a*c + (b*d*(-1)), a*d + (b*c*(+1))
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);
    };
    if constexpr (!PERMUTED) {
        constexpr int NBL = PL::NB(PL::NP - 1);
        lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[PairLayout<CP>::pos((tid + it * PL::T) + r * NBL)] = val; }, lds, tw, tid);
    } else {
        // permuted storage order: staged through LDS and stored position by position, as acq_mix_fft_kernel does
        constexpr int NBL = PL::NB(PL::NP - 1);
        {
            cf v0[PL::IT0][PL::R0];
            Fft<PL, false>::pass0_stage1(v0, in, tid);
            __syncthreads();
            Fft<PL, false>::pass0_stage2(v0, lds, tid);
        }
        __syncthreads();
        MiddlePasses<PL, false, 1>::run(lds, tw, tid);
        cf vl[PL::ITL][PL::RL];
        Fft<PL, false>::last_stage1(vl, lds, tw, tid);
        __syncthreads();
        Fft<PL, false>::last_stage2(vl, [&](int it, int r, cf val) {
            const int k = (tid + it * PL::T) + r * NBL;
            lds[k + (k >> 5)] = val; }, tid);
        __syncthreads();
        static_assert(PL::N % 2 == 0, "N must be even");
        for (int g = tid; g < PL::N / 2; g += PL::T) {
            const uint32_t w = reinterpret_cast<const uint32_t*>(order)[g];
            const int k0 = int(w & 0xffffu), k1 = int(w >> 16);
            const cf v0 = lds[k0 + (k0 >> 5)], v1 = lds[k1 + (k1 >> 5)];
            reinterpret_cast<float4*>(dst)[g] = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    }
}

// ------------------------------------------------------------------------------------ composite sizes (comp_fwd_sub_kernel)
// grid n_items * Q: item = (v, m), v = h D + d, n1 = blockIdx % Q; A[item][n1][k2] (order != null: storage order, staged through LDS)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void comp_fwd_sub_drift_kernel(const void* __restrict__ samples, int fmt,
                                                                 const uint64_t* __restrict__ starts, uint32_t R,
                                                                 const cf* __restrict__ rho, uint32_t K,
                                                                 const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                 const cf* __restrict__ tables,
                                                                 const cf* __restrict__ tw_fwd, cf* __restrict__ A,
                                                                 uint32_t Q, uint32_t n_int, const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the starts");
    constexpr int STAGE = CorrMode<typename CompPlanOf<PLX>::type>::PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    __shared__ uint32_t start_s[2 * GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x % Q;
    const size_t N = size_t(Q) * PL::N;
    const uint32_t v = item / n_int, m = item % n_int, h = v / D, d = v - h * D;
    const uint32_t o = offsets ? offsets[h] : 0u;
    const DriftLoad load{samples, fmt, K, rho_s, start_s};
    load.stage(starts + size_t(d) * R + o + size_t(m) * K, rho + size_t(item) * K, neg, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const size_t n = size_t(Q) * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        const cf s = load(n);                                                  // group m folded over its K periods
        const cf t = tables[size_t(d) * N + n];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    if (!STAGE || !order) {
        lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
    } else {
        {
            cf v0[PL::IT0][PL::R0];
            Fft<PL, false>::pass0_stage1(v0, in, tid);
            __syncthreads();
            Fft<PL, false>::pass0_stage2(v0, lds, tid);
        }
        __syncthreads();
        MiddlePasses<PL, false, 1>::run(lds, tw, tid);
        cf vl[PL::ITL][PL::RL];
        Fft<PL, false>::last_stage1(vl, lds, tw, tid);
        __syncthreads();
        Fft<PL, false>::last_stage2(vl, [&](int it, int r, cf val) {
            const int k = (tid + it * PL::T) + r * NBL;
            lds[k + (k >> 5)] = val; }, tid);
        __syncthreads();
        for (int p = tid; p < PL::N; p += PL::T) {
            const int k = order[p];
            dst[p] = lds[k + (k >> 5)];
        }
    }
}

// ------------------------------------------------------------------------------------ any-length sizes (long_fwd_sub_kernel)
// grid n_items * Q; element n = Q*n2 + n1 of the length-L sequence: folded sample n mod N for n < lim, else 0 — the mod-N wrap and the
// zero padding apply to the folded sequence.  A[item][n1][k2], natural order
template <class PL>
__global__ __launch_bounds__(PL::T) void long_fwd_sub_drift_kernel(const void* __restrict__ samples, int fmt,
                                                                  const uint64_t* __restrict__ starts, uint32_t R,
                                                                  const cf* __restrict__ rho, uint32_t K,
                                                                  const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                  const cf* __restrict__ tables, const cf* __restrict__ tw_fwd,
                                                                  cf* __restrict__ A, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the starts");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    __shared__ uint32_t start_s[2 * GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x - item * Q;
    const uint32_t v = item / n_int, m = item - v * n_int, h = v / D, d = v - h * D;
    const uint32_t o = offsets ? offsets[h] : 0u;
    const DriftLoad load{samples, fmt, K, rho_s, start_s};
    load.stage(starts + size_t(d) * R + o + size_t(m) * K, rho + size_t(item) * K, neg, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const uint32_t n = Q * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        if (n >= lim) return cf_make(0.0f, 0.0f);
        const uint32_t i = n < N ? n : n - N;
        const cf s = load(size_t(i));                                          // group m folded over its K periods
        const cf t = tables[size_t(d) * N + i];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
}

}  // namespace

// ------------------------------------------------------------------------------------ launchers
template <class PL> static void launch_mix_fft_drift(hipStream_t st, const DriftArgs& a) {
    hipLaunchKernelGGL(acq_mix_fft_drift_kernel<PL>, dim3(a.H * a.n_bins * a.n_int), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt,
                       a.starts, a.R, a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, int(a.n_int), a.clear_tickets, a.order);
}
template <class PL> static void launch_comp_fwd_sub_drift(hipStream_t st, const DriftArgs& a) {
    hipLaunchKernelGGL(comp_fwd_sub_drift_kernel<PL>, dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt,
                       a.starts, a.R, a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.n_int, a.order);
}
template <class PL> static void launch_long_fwd_sub_drift(hipStream_t st, const DriftArgs& a) {
    hipLaunchKernelGGL(long_fwd_sub_drift_kernel<PL>, dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(PL::T), 0, st, a.samples, a.fmt, a.starts, a.R,
                       a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.N, a.lim, a.n_int);
}

// the in-LDS plans, the composite bases and the long bases, looked up by base length as in acq_edge.hip: the plan tables of the other
// units stay as they are
DriftLaunch find_drift_mix_fft(int n) {
#define GM_DRIFT_MIX(PL) if (n == PL::N) return &launch_mix_fft_drift<PL>;
    GM_FOR_EACH_PLAN(GM_DRIFT_MIX)
    return nullptr;
}
DriftLaunch find_drift_comp_fwd_sub(int nb) {
#define GM_DRIFT_COMP(PL) if (nb == PL::N) return &launch_comp_fwd_sub_drift<PL>;
    GM_DRIFT_COMP(Plan16384) GM_DRIFT_COMP(Plan16368) GM_DRIFT_COMP(Plan16000) GM_DRIFT_COMP(Plan8000) GM_DRIFT_COMP(Plan8192) GM_DRIFT_COMP(Plan8184)
    GM_DRIFT_COMP(Plan6000) GM_DRIFT_COMP(Plan5000) GM_DRIFT_COMP(Plan4000)
    return nullptr;
}
DriftLaunch find_drift_long_fwd_sub(int nb) {
#define GM_DRIFT_LONG(PL) if (nb == PL::N) return &launch_long_fwd_sub_drift<PL>;
    GM_DRIFT_LONG(Plan16384) GM_DRIFT_LONG(Plan16000) GM_DRIFT_LONG(Plan10000) GM_DRIFT_LONG(Plan8192) GM_DRIFT_LONG(Plan8000) GM_DRIFT_LONG(Plan4096)
    GM_DRIFT_LONG(Plan2048)
    return nullptr;
}

}  // namespace gm
