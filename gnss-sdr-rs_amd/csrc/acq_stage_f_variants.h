// acq_stage_f_variants.h — stage F of the coherent, the edge-search and the code-drift handles: one kernel body per form (in-LDS sizes,
// composite bases, any-length bases), parameterised on how pass 0 gets one input sample.
//
// The bodies are stage F's K = 1 kernels (acq_mix_fft_kernel, comp_fwd_sub_kernel, long_fwd_sub_kernel) with a loader `Load` in pass
// 0's input.  A loader is constructed once per workgroup from the kernel's arguments, the item's place (h, d, m, item), the period
// length and the workgroup's LDS words; the constructor stages what the item needs into LDS and issues the one barrier that orders it
// before the first pass-0 load.  load(n) is element n of the item's input.  Two constants say what the grid looks like:
//     Load::HYP     the grid has a hypothesis axis: item = (v, m) with the virtual bin v = h D + d; else item = (d, m) and h = 0
//     Load::STARTS  the loader wants 2 * GM_COHERENT_MAX words of LDS for the periods' starts (else none are declared)
//
//     CohLoad    (gm_acq_cfg.coherent_periods = K >= 2)  y_{d,m}[n]   = sum_k rho[d][k] x[(m K + k) N + n]
//     EdgeLoad   (gm_acq_set_edge_search)                y_{h,d,m}[n] = sum_k sec[k] rho[d][k] x[(o_h + m K + k) N + n]
//     DriftLoad  (gm_acq_set_code_drift)                 y_{h,d,m}[n] = sum_k sec[k] rho[h][d][m][k] x[s[d][o_h + m K + k] + n]
//
// The spectra leave as [D][M][.] or [H D][M][.], so stage C, the decision and the reduction over the hypotheses run unchanged.  The
// K = 1 kernels keep their own bodies in their own units (a second instantiation of one body THERE changed the inlining, and with it
// the registers, of the K = 1 kernels of 16000); the variants among themselves share these (profiles/stage_f_variants_kernel_stats.txt).
// The replicas (code_samples) never come here: they are not folded.
#pragma once
#include "acq_device.h"

namespace gm {

// the composite path's base plans run their correlation on these plans (as in acq_composite.hip): they fix the stored order
template <> struct CompPlanOf<Plan16368> { using type = AsPlain<Plan16368>; };
template <> struct CompPlanOf<Plan8184> { using type = AsPlain<Plan8184>; };
template <> struct CompPlanOf<Plan8192> { using type = Plan8192; };
#ifdef GM_COMP_PLAIN_16000
template <> struct CompPlanOf<Plan16000> { using type = Plan16000; };
#endif

// Coherent fold: y[n] = sum_k rho[k] x[idx + k stride].  k ascends, and every product and every sum is rounded on its own as
// num-complex forms them (the sources build with -ffp-contract=off: no fma here), so the host restates the fold exactly.
// 64-bit element offsets: K M N samples of 8 bytes can pass 4 GiB.
__device__ __forceinline__ cf fold_sample(const void* samples, int fmt, size_t idx, size_t stride, uint32_t K, const cf* rho) {
    cf s = load_sample(samples, fmt, idx), r = rho[0];
    cf acc = cf_make(r.x * s.x - r.y * s.y, r.x * s.y + r.y * s.x);
    for (uint32_t k = 1; k < K; ++k) {
        s = load_sample(samples, fmt, idx + size_t(k) * stride);
        r = rho[k];
        acc = cf_make(acc.x + (r.x * s.x - r.y * s.y), acc.y + (r.x * s.y + r.y * s.x));
    }
    return acc;
}

// what a loader reads of the kernel's arguments, gathered inside the kernel (the kernels themselves keep plain __restrict__ pointers)
struct FoldIn {
    const void* samples; int fmt;
    const uint64_t* starts; uint32_t R;    // DriftLoad: s[n_bins][R]
    const cf* rho; uint32_t K;             // [D][K]; DriftLoad: [H][D][M][K]
    const uint32_t* offsets; uint32_t neg; // [H] period offsets (DriftLoad: may be null, one hypothesis at 0); bit k set: sec[k] = -1
};
// the item's place in the grid
struct FoldItem { uint32_t h, d, m, item; };

// group m of K consecutive periods of N samples, folded with bin d's K phasor words
struct CohLoad {
    static constexpr bool HYP = false, STARTS = false;
    const void* samples; int fmt; uint32_t K; const cf* rho_s; size_t base, N;
    __device__ __forceinline__ CohLoad(const FoldIn& a, FoldItem w, size_t N_, cf* rho_s_, uint32_t*, int tid)
        : samples(a.samples), fmt(a.fmt), K(a.K), rho_s(rho_s_), base(size_t(w.m) * a.K * N_), N(N_) {
        if (uint32_t(tid) < K) rho_s_[tid] = a.rho[size_t(w.d) * K + tid];
        __syncthreads();
    }
    __device__ __forceinline__ cf operator()(size_t n) const { return fold_sample(samples, fmt, base + n, N, K, rho_s); }
};

// CohLoad for hypothesis h: the dwell from period o_h on, the secondary row's signs applied to bin d's phasor words on their way into
// LDS (a negation: exact)
struct EdgeLoad {
    static constexpr bool HYP = true, STARTS = false;
    const void* samples; int fmt; uint32_t K; const cf* rho_s; size_t base, N;
    __device__ __forceinline__ EdgeLoad(const FoldIn& a, FoldItem w, size_t N_, cf* rho_s_, uint32_t*, int tid)
        : samples(a.samples), fmt(a.fmt), K(a.K), rho_s(rho_s_), base(size_t(a.offsets[w.h]) * N_ + size_t(w.m) * a.K * N_), N(N_) {
        if (uint32_t(tid) < K) {
            const cf r = a.rho[size_t(w.d) * K + tid];
            rho_s_[tid] = ((a.neg >> tid) & 1u) ? cf_make(-r.x, -r.y) : r;
        }
        __syncthreads();
    }
    __device__ __forceinline__ cf operator()(size_t n) const { return fold_sample(samples, fmt, base + n, N, K, rho_s); }
};

// every period from where it really starts: lane k copies period k's start (a 64-bit element offset) and its phasor word, with the
// secondary row's sign, into LDS.  The start words are uniform over the workgroup: they are read back through readfirstlane, so that
// the address of period k is a scalar base plus the lane's n.  These are the real samples at another place: no circular shift and no
// phase ramp.  K = 1 is the samples themselves (no fold, no product), so its words are those of a plain search of the gathered samples.
struct DriftLoad {
    static constexpr bool HYP = true, STARTS = true;
    const void* samples; int fmt; uint32_t K; const cf* rho_s; const uint32_t* start_s;      // start_s: [K] {lo, hi}
    __device__ __forceinline__ DriftLoad(const FoldIn& a, FoldItem w, size_t, cf* rho_s_, uint32_t* start_s_, int tid)
        : samples(a.samples), fmt(a.fmt), K(a.K), rho_s(rho_s_), start_s(start_s_) {
        const uint32_t o = a.offsets ? a.offsets[w.h] : 0u;
        const uint64_t* __restrict__ starts_g = a.starts + size_t(w.d) * a.R + o + size_t(w.m) * K;   // s[d][o_h + m K ..]
        const cf* __restrict__ rho_g = a.rho + size_t(w.item) * K;                                   // rho[h][d][m][..]
        if (uint32_t(tid) < K) {
            const uint64_t s = starts_g[tid];
            start_s_[2 * tid] = uint32_t(s);
            start_s_[2 * tid + 1] = uint32_t(s >> 32);
            const cf r = rho_g[tid];
            rho_s_[tid] = ((a.neg >> tid) & 1u) ? cf_make(-r.x, -r.y) : r;
        }
        __syncthreads();
    }
    __device__ __forceinline__ size_t start(uint32_t k) const {
        const uint32_t lo = __builtin_amdgcn_readfirstlane(start_s[2 * k]), hi = __builtin_amdgcn_readfirstlane(start_s[2 * k + 1]);
        return size_t(lo) | (size_t(hi) << 32);
    }
    // fold_sample's arithmetic: k ascending, every product and sum rounded on its own
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

namespace {

// item -> (h, d, m): item = (v, m), v = h D + d with a hypothesis axis, else item = (d, m)
template <class Load> __device__ __forceinline__ FoldItem fold_item(uint32_t item, uint32_t n_int, uint32_t D) {
    const uint32_t v = item / n_int, m = item - v * n_int;
    if constexpr (Load::HYP) {
        const uint32_t h = v / D;
        return FoldItem{h, v - h * D, m, item};
    } else {
        return FoldItem{0u, v, m, item};
    }
}

// Permuted storage orders: the transform of `in` is staged through LDS (element k at k + (k >> 5)) and stored position by position,
// order[p] being the element stored at p — as acq_mix_fft_kernel (PAIRS: two positions per lane, one 16-byte store) and
// comp_fwd_sub_kernel do
template <class PL, bool PAIRS, class In>
__device__ __forceinline__ void store_permuted(In in, cf* __restrict__ dst, const uint16_t* __restrict__ order, cf* lds, const cf* tw, int tid) {
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
    if constexpr (PAIRS) {
        static_assert(PL::N % 2 == 0, "N must be even");
        for (int g = tid; g < PL::N / 2; g += PL::T) {
            const uint32_t o = reinterpret_cast<const uint32_t*>(order)[g];
            const int k0 = int(o & 0xffffu), k1 = int(o >> 16);
            const cf v0 = lds[k0 + (k0 >> 5)], v1 = lds[k1 + (k1 >> 5)];
            reinterpret_cast<float4*>(dst)[g] = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    } else {
        for (int p = tid; p < PL::N; p += PL::T) {
            const int k = order[p];
            dst[p] = lds[k + (k >> 5)];
        }
    }
}

#define GM_FOLD_LDS(Load)                                                        \
    __shared__ cf rho_s[GM_COHERENT_MAX];                                        \
    uint32_t* start_s = nullptr;                                                 \
    if constexpr (Load::STARTS) {                                                \
        __shared__ uint32_t start_words[2 * GM_COHERENT_MAX];                    \
        start_s = start_words;                                                   \
    }

// ------------------------------------------------------------------------------------ in-LDS sizes (acq_mix_fft_kernel)
// one workgroup per item; no trailing decision workgroups (these handles decide at once, gm_acq_set_deferred_decision)
template <class PLX, class Load>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void acq_mix_fft_fold_kernel(const void* __restrict__ samples, int fmt,
                                                                const uint64_t* __restrict__ starts, uint32_t R,
                                                                const cf* __restrict__ rho, uint32_t K,
                                                                const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                const cf* __restrict__ tables,
                                                                const cf* __restrict__ tw_fwd,
                                                                cf* __restrict__ spectra, uint32_t n_int,
                                                                uint32_t* __restrict__ clear_tickets,
                                                                const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    using CP = typename CorrPlanOf<PLX>::type;
    static_assert(PL::N == PLX::N, "the mix plan keeps the size");
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the phasor words and the starts");
    constexpr bool PERMUTED = CorrMode<CP>::PERMUTED;
    constexpr int STAGE = PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    GM_FOLD_LDS(Load)
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    const FoldItem w = fold_item<Load>(blockIdx.x, n_int, D);
    if (clear_tickets && blockIdx.x == 0)        // the tail split's tickets, as acq_mix_fft_kernel clears them
        for (int i = tid; i < GM_CORR_SPLIT_MAX_ITEMS; i += PL::T) clear_tickets[i] = 0u;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const Load load(FoldIn{samples, fmt, starts, R, rho, K, offsets, neg}, w, size_t(PL::N), rho_s, start_s, tid);
    const cf* tab = tables + size_t(w.d) * PL::N;
    cf* dst = spectra + size_t(blockIdx.x) * PL::N;   // [v][m][k]
    constexpr int NB0 = PL::NB(0);
    auto in = [&](int it, int r) {
        const int idx = (tid + it * PL::T) + r * NB0;
        const cf s = load(size_t(idx));
        const cf t = tab[idx];
        // multiply_simd_block (doppler_shift.rs:43-58): a*c + (b*d*(-1)), a*d + (b*c*(+1))
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);
    };
    if constexpr (!PERMUTED) {
        constexpr int NBL = PL::NB(PL::NP - 1);
        lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[PairLayout<CP>::pos((tid + it * PL::T) + r * NBL)] = val; }, lds, tw, tid);
    } else {
        store_permuted<PL, true>(in, dst, order, lds, tw, tid);
    }
}

// ------------------------------------------------------------------------------------ composite sizes (comp_fwd_sub_kernel)
// grid n_items * Q: n1 = blockIdx % Q; A[item][n1][k2] (order != null: storage order, staged through LDS)
template <class PLX, class Load>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void comp_fwd_sub_fold_kernel(const void* __restrict__ samples, int fmt,
                                                                 const uint64_t* __restrict__ starts, uint32_t R,
                                                                 const cf* __restrict__ rho, uint32_t K,
                                                                 const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                 const cf* __restrict__ tables,
                                                                 const cf* __restrict__ tw_fwd, cf* __restrict__ A,
                                                                 uint32_t Q, uint32_t n_int, const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the phasor words and the starts");
    constexpr int STAGE = CorrMode<typename CompPlanOf<PLX>::type>::PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    GM_FOLD_LDS(Load)
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x % Q;
    const size_t N = size_t(Q) * PL::N;
    const FoldItem w = fold_item<Load>(item, n_int, D);
    const Load load(FoldIn{samples, fmt, starts, R, rho, K, offsets, neg}, w, N, rho_s, start_s, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const size_t n = size_t(Q) * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        const cf s = load(n);
        const cf t = tables[size_t(w.d) * N + n];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    if (!STAGE || !order) {
        lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
    } else {
        store_permuted<PL, false>(in, dst, order, lds, tw, tid);
    }
}

// ------------------------------------------------------------------------------------ any-length sizes (long_fwd_sub_kernel)
// grid n_items * Q; element n = Q*n2 + n1 of the length-L sequence: folded sample n mod N for n < lim, else 0 — the mod-N wrap and the
// zero padding apply to the folded sequence.  A[item][n1][k2], natural order
template <class PL, class Load>
__global__ __launch_bounds__(PL::T) void long_fwd_sub_fold_kernel(const void* __restrict__ samples, int fmt,
                                                                 const uint64_t* __restrict__ starts, uint32_t R,
                                                                 const cf* __restrict__ rho, uint32_t K,
                                                                 const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                 const cf* __restrict__ tables, const cf* __restrict__ tw_fwd,
                                                                 cf* __restrict__ A, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    static_assert(PL::T >= GM_COHERENT_MAX, "one lane per period stages the phasor words and the starts");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    GM_FOLD_LDS(Load)
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x - item * Q;
    const FoldItem w = fold_item<Load>(item, n_int, D);
    const Load load(FoldIn{samples, fmt, starts, R, rho, K, offsets, neg}, w, size_t(N), rho_s, start_s, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const uint32_t n = Q * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        if (n >= lim) return cf_make(0.0f, 0.0f);
        const uint32_t i = n < N ? n : n - N;
        const cf s = load(size_t(i));
        const cf t = tables[size_t(w.d) * N + i];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
}
#undef GM_FOLD_LDS

// ------------------------------------------------------------------------------------ launchers: one per form
template <class PL, class Load> void launch_mix_fft_fold(hipStream_t st, const StageFArgs& a) {
    hipLaunchKernelGGL((acq_mix_fft_fold_kernel<PL, Load>), dim3(a.H * a.n_bins * a.n_int), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples,
                       a.fmt, a.starts, a.R, a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.n_int, a.clear_tickets, a.order);
}
template <class PL, class Load> void launch_comp_fwd_sub_fold(hipStream_t st, const StageFArgs& a) {
    hipLaunchKernelGGL((comp_fwd_sub_fold_kernel<PL, Load>), dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(MixPlanOf<PL>::type::T), 0, st,
                       a.samples, a.fmt, a.starts, a.R, a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.n_int, a.order);
}
template <class PL, class Load> void launch_long_fwd_sub_fold(hipStream_t st, const StageFArgs& a) {
    hipLaunchKernelGGL((long_fwd_sub_fold_kernel<PL, Load>), dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(PL::T), 0, st, a.samples, a.fmt,
                       a.starts, a.R, a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.N, a.lim, a.n_int);
}

// the composite bases (acq_composite.hip's g_comp, GM_COMP_ALL_Q's 4000 included) and the long bases (acq_long.hip's g_long); the
// in-LDS plans are GM_FOR_EACH_PLAN
#define GM_FOR_EACH_COMP_BASE(X) X(Plan16384) X(Plan16368) X(Plan16000) X(Plan8000) X(Plan8192) X(Plan8184) X(Plan6000) X(Plan5000) X(Plan4000)
#define GM_FOR_EACH_LONG_BASE(X) X(Plan16384) X(Plan16000) X(Plan10000) X(Plan8192) X(Plan8000) X(Plan4096) X(Plan2048)

}  // namespace

// the launcher of `form` (STAGE_F_MIX: n is the size; else the base plan's length) with loader Load; null: no such plan
template <class Load> StageFLaunch find_stage_f(int form, int n) {
#define GM_FOLD_MIX(PL) if (n == PL::N) return &launch_mix_fft_fold<PL, Load>;
#define GM_FOLD_COMP(PL) if (n == PL::N) return &launch_comp_fwd_sub_fold<PL, Load>;
#define GM_FOLD_LONG(PL) if (n == PL::N) return &launch_long_fwd_sub_fold<PL, Load>;
    if (form == STAGE_F_MIX) { GM_FOR_EACH_PLAN(GM_FOLD_MIX) }
    else if (form == STAGE_F_COMP) { GM_FOR_EACH_COMP_BASE(GM_FOLD_COMP) }
    else { GM_FOR_EACH_LONG_BASE(GM_FOLD_LONG) }
    return nullptr;
#undef GM_FOLD_MIX
#undef GM_FOLD_COMP
#undef GM_FOLD_LONG
}

}  // namespace gm
