// acq_coherent.hip — stage F of a coherent handle (gm_acq_cfg.coherent_periods = K >= 2): coherent integration over K code periods.
//
// A dwell of K * M periods of N samples forms M groups of K.  For Doppler bin d and group m the workgroup folds the group's periods with
// the bin's phasor words before the carrier mix (CohLoad, acq_device.h),
//     y[n] = sum_k rho[d][k] x[(m K + k) N + n],   rho[d][k] = exp(-j 2 pi f_d k N / fs),
// and then does what today's stage F does with period m: mix with table d, forward transform, store the spectrum [d][m][.].  Stage C,
// the decision and every buffer sized D * M * N are unchanged.  Against a sum of K spectra in the frequency domain the fold costs K times
// the pass-0 loads and no extra transform.
//
// The three kernels are copies of stage F's K = 1 kernels (acq_mix_fft_kernel, comp_fwd_sub_kernel, long_fwd_sub_kernel) with the fold in
// pass 0's input, kept in a translation unit of their own: the K = 1 kernels' sources and code objects stay exactly as they were (two
// instantiations of one body in the same unit changed the inlining, and with it the registers, of the K = 1 kernels of 16000).
// The replicas (code_samples) never come here: they are not folded.
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

// ------------------------------------------------------------------------------------ in-LDS sizes (acq_mix_fft_kernel)
// one workgroup per (d, m); no trailing decision workgroups (a coherent handle decides at once, gm_acq_set_deferred_decision)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void acq_mix_fft_coh_kernel(const void* __restrict__ samples, int fmt,
                                                                const cf* __restrict__ rho, uint32_t K,
                                                                const cf* __restrict__ tables,
                                                                const cf* __restrict__ tw_fwd,
                                                                cf* __restrict__ spectra, int n_int,
                                                                uint32_t* __restrict__ clear_tickets,
                                                                const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    using CP = typename CorrPlanOf<PLX>::type;
    static_assert(PL::N == PLX::N, "the mix plan keeps the size");
    constexpr bool PERMUTED = CorrMode<CP>::PERMUTED;
    constexpr int STAGE = PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    const int d = blockIdx.x / n_int, m = blockIdx.x % n_int;
    if (clear_tickets && blockIdx.x == 0)        // the tail split's tickets, as acq_mix_fft_kernel clears them
        for (int i = tid; i < GM_CORR_SPLIT_MAX_ITEMS; i += PL::T) clear_tickets[i] = 0u;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const CohLoad load{samples, fmt, rho, K, rho_s};
    load.stage(uint32_t(d), tid);
    const cf* tab = tables + size_t(d) * PL::N;
    cf* dst = spectra + size_t(blockIdx.x) * PL::N;   // [d][m][k]
    constexpr int NB0 = PL::NB(0);
    auto in = [&](int it, int r) {
        const int idx = (tid + it * PL::T) + r * NB0;
        const cf s = load(size_t(m), size_t(PL::N), size_t(idx));      // group m folded over its K periods
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
            const uint32_t o = reinterpret_cast<const uint32_t*>(order)[g];
            const int k0 = int(o & 0xffffu), k1 = int(o >> 16);
            const cf v0 = lds[k0 + (k0 >> 5)], v1 = lds[k1 + (k1 >> 5)];
            reinterpret_cast<float4*>(dst)[g] = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    }
}

// ------------------------------------------------------------------------------------ composite sizes (comp_fwd_sub_kernel)
// grid n_items * Q: item = (d, m), n1 = blockIdx % Q; A[item][n1][k2] (order != null: storage order, staged through LDS)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void comp_fwd_sub_coh_kernel(const void* __restrict__ samples, int fmt,
                                                                 const cf* __restrict__ rho, uint32_t K,
                                                                 const cf* __restrict__ tables,
                                                                 const cf* __restrict__ tw_fwd, cf* __restrict__ A,
                                                                 uint32_t Q, uint32_t n_int, const uint16_t* __restrict__ order) {
    using PL = typename MixPlanOf<PLX>::type;
    constexpr int STAGE = CorrMode<typename CompPlanOf<PLX>::type>::PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x % Q;
    const size_t N = size_t(Q) * PL::N;
    const uint32_t d = item / n_int, m = item % n_int;
    const CohLoad load{samples, fmt, rho, K, rho_s};
    load.stage(d, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const size_t n = size_t(Q) * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        const cf s = load(size_t(m), N, n);                                    // group m folded over its K periods
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
__global__ __launch_bounds__(PL::T) void long_fwd_sub_coh_kernel(const void* __restrict__ samples, int fmt, const cf* __restrict__ rho,
                                                                 uint32_t K, const cf* __restrict__ tables, const cf* __restrict__ tw_fwd,
                                                                 cf* __restrict__ A, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x - item * Q;
    const uint32_t d = item / n_int, m = item - d * n_int;
    const CohLoad load{samples, fmt, rho, K, rho_s};
    load.stage(d, tid);
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const uint32_t n = Q * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        if (n >= lim) return cf_make(0.0f, 0.0f);
        const uint32_t i = n < N ? n : n - N;
        const cf s = load(size_t(m), size_t(N), size_t(i));                    // group m folded over its K periods
        const cf t = tables[size_t(d) * N + i];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
}

}  // namespace

// ------------------------------------------------------------------------------------ launchers (PlanOps / CompOps / LongOps)
template <class PL> void launch_mix_fft_coh(hipStream_t st, const CohArgs& a) {
    hipLaunchKernelGGL(acq_mix_fft_coh_kernel<PL>, dim3(a.n_bins * a.n_int), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt, a.rho,
                       a.K, a.tables, a.tw_fwd, a.out, int(a.n_int), a.clear_tickets, a.order);
}
template <class PL> void launch_comp_fwd_sub_coh(hipStream_t st, const CohArgs& a) {
    hipLaunchKernelGGL(comp_fwd_sub_coh_kernel<PL>, dim3(a.n_bins * a.n_int * a.Q), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt,
                       a.rho, a.K, a.tables, a.tw_fwd, a.out, a.Q, a.n_int, a.order);
}
template <class PL> void launch_long_fwd_sub_coh(hipStream_t st, const CohArgs& a) {
    hipLaunchKernelGGL(long_fwd_sub_coh_kernel<PL>, dim3(a.n_bins * a.n_int * a.Q), dim3(PL::T), 0, st, a.samples, a.fmt, a.rho, a.K,
                       a.tables, a.tw_fwd, a.out, a.Q, a.N, a.lim, a.n_int);
}

// the in-LDS plans, the composite bases (acq_composite.hip's g_comp, GM_COMP_ALL_Q's 4000 included) and the long bases (acq_long.hip)
#define GM_COH_MIX(PL) template void launch_mix_fft_coh<PL>(hipStream_t, const CohArgs&);
GM_FOR_EACH_PLAN(GM_COH_MIX)
#define GM_COH_COMP(PL) template void launch_comp_fwd_sub_coh<PL>(hipStream_t, const CohArgs&);
GM_COH_COMP(Plan16384) GM_COH_COMP(Plan16368) GM_COH_COMP(Plan16000) GM_COH_COMP(Plan8000) GM_COH_COMP(Plan8192) GM_COH_COMP(Plan8184)
GM_COH_COMP(Plan6000) GM_COH_COMP(Plan5000) GM_COH_COMP(Plan4000)
#define GM_COH_LONG(PL) template void launch_long_fwd_sub_coh<PL>(hipStream_t, const CohArgs&);
GM_COH_LONG(Plan16384) GM_COH_LONG(Plan16000) GM_COH_LONG(Plan10000) GM_COH_LONG(Plan8192) GM_COH_LONG(Plan8000) GM_COH_LONG(Plan4096)
GM_COH_LONG(Plan2048)

}  // namespace gm
