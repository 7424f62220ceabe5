// acq_edge.hip — stage F of a coherent handle's edge search (gm_acq_set_edge_search) and the reduction over its hypotheses.
//
// Hypothesis h of H is the coherent search (acq_coherent.hip) on the samples from period o_h on, with the secondary row's signs in
// the fold:  y_{h,d,m}[n] = sum_k s[k] rho[d][k] x[(o_h + m K + k) N + n].  The grid grows by H: a virtual bin is v = h D + d, the
// sample base moves on by o_h N elements (64-bit), bin d's table and phasor words serve every h, and the phasor words are staged into
// LDS as s[k] * rho[d][k] (a negation: exact).  The spectra leave as [H D][M][.], so stage C runs unchanged with n_bins = H D into a
// [3][P][H][D] block, and acq_edge_reduce_kernel picks a hypothesis per (worker, bin) cell.
//
// The three stage-F kernels are copies of acq_coherent.hip's with these changes, in a translation unit of their own for the reason
// given there: the K = 1 and the plain coherent code objects stay exactly as they were.
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

// CohLoad (acq_device.h) for hypothesis h: the dwell from element base = o_h N on; stage() applies the secondary row's signs (bit k of
// neg set: s[k] = -1) to bin d's K phasor words on their way into LDS
struct EdgeLoad {
    const void* samples; int fmt;
    const cf* rho_g; uint32_t K; cf* rho_s;
    size_t base; uint32_t neg;
    __device__ __forceinline__ void stage(uint32_t d, int tid) const {
        if (uint32_t(tid) < K) {
            const cf r = rho_g[size_t(d) * K + tid];
            rho_s[tid] = ((neg >> tid) & 1u) ? cf_make(-r.x, -r.y) : r;
        }
        __syncthreads();
    }
    __device__ __forceinline__ cf operator()(size_t m, size_t N, size_t n) const {
        return fold_sample(samples, fmt, base + m * K * N + n, N, K, rho_s);
    }
};

// ------------------------------------------------------------------------------------ in-LDS sizes (acq_mix_fft_kernel)
// one workgroup per (v, m), v = h D + d; no trailing decision workgroups (a coherent handle decides at once)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void acq_mix_fft_edge_kernel(const void* __restrict__ samples, int fmt,
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
    constexpr bool PERMUTED = CorrMode<CP>::PERMUTED;
    constexpr int STAGE = PERMUTED ? PL::N + PL::N / 32 + 1 : 0;
    constexpr int LDS_N = PL::LDS_ELEMS + PL::TW_TOTAL > STAGE ? PL::LDS_ELEMS + PL::TW_TOTAL : STAGE;
    __shared__ cf lds[LDS_N];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    const uint32_t v = blockIdx.x / uint32_t(n_int), m = blockIdx.x - v * uint32_t(n_int);   // virtual bin v = h D + d
    const uint32_t h = v / D, d = v - h * D;
    if (clear_tickets && blockIdx.x == 0)        // the tail split's tickets, as acq_mix_fft_kernel clears them
        for (int i = tid; i < GM_CORR_SPLIT_MAX_ITEMS; i += PL::T) clear_tickets[i] = 0u;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const EdgeLoad load{samples, fmt, rho, K, rho_s, size_t(offsets[h]) * PL::N, neg};
    load.stage(d, tid);
    const cf* tab = tables + size_t(d) * PL::N;
    cf* dst = spectra + size_t(blockIdx.x) * PL::N;   // [v][m][k]
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
// grid n_items * Q: item = (v, m), v = h D + d, n1 = blockIdx % Q; A[item][n1][k2] (order != null: storage order, staged through LDS)
template <class PLX>
__global__ __launch_bounds__(MixPlanOf<PLX>::type::T) void comp_fwd_sub_edge_kernel(const void* __restrict__ samples, int fmt,
                                                                 const cf* __restrict__ rho, uint32_t K,
                                                                 const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
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
    const uint32_t v = item / n_int, m = item % n_int, h = v / D, d = v - h * D;
    const EdgeLoad load{samples, fmt, rho, K, rho_s, size_t(offsets[h]) * N, neg};
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
__global__ __launch_bounds__(PL::T) void long_fwd_sub_edge_kernel(const void* __restrict__ samples, int fmt, const cf* __restrict__ rho,
                                                                 uint32_t K, const uint32_t* __restrict__ offsets, uint32_t neg, uint32_t D,
                                                                 const cf* __restrict__ tables, const cf* __restrict__ tw_fwd,
                                                                 cf* __restrict__ A, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    __shared__ cf rho_s[GM_COHERENT_MAX];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x - item * Q;
    const uint32_t v = item / n_int, m = item - v * n_int, h = v / D, d = v - h * D;
    const EdgeLoad load{samples, fmt, rho, K, rho_s, size_t(offsets[h]) * N, neg};
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

// ------------------------------------------------------------------------------------ launchers
template <class PL> static void launch_mix_fft_edge(hipStream_t st, const EdgeArgs& a) {
    hipLaunchKernelGGL(acq_mix_fft_edge_kernel<PL>, dim3(a.H * a.n_bins * a.n_int), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt, a.rho,
                       a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, int(a.n_int), a.clear_tickets, a.order);
}
template <class PL> static void launch_comp_fwd_sub_edge(hipStream_t st, const EdgeArgs& a) {
    hipLaunchKernelGGL(comp_fwd_sub_edge_kernel<PL>, dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(MixPlanOf<PL>::type::T), 0, st, a.samples, a.fmt,
                       a.rho, a.K, a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.n_int, a.order);
}
template <class PL> static void launch_long_fwd_sub_edge(hipStream_t st, const EdgeArgs& a) {
    hipLaunchKernelGGL(long_fwd_sub_edge_kernel<PL>, dim3(a.H * a.n_bins * a.n_int * a.Q), dim3(PL::T), 0, st, a.samples, a.fmt, a.rho, a.K,
                       a.offsets, a.neg, a.n_bins, a.tables, a.tw_fwd, a.out, a.Q, a.N, a.lim, a.n_int);
}

// the in-LDS plans, the composite bases (acq_composite.hip's g_comp, GM_COMP_ALL_Q's 4000 included) and the long bases (acq_long.hip):
// looked up by base length, so that the plan tables of the other units stay as they are
EdgeLaunch find_edge_mix_fft(int n) {
#define GM_EDGE_MIX(PL) if (n == PL::N) return &launch_mix_fft_edge<PL>;
    GM_FOR_EACH_PLAN(GM_EDGE_MIX)
    return nullptr;
}
EdgeLaunch find_edge_comp_fwd_sub(int nb) {
#define GM_EDGE_COMP(PL) if (nb == PL::N) return &launch_comp_fwd_sub_edge<PL>;
    GM_EDGE_COMP(Plan16384) GM_EDGE_COMP(Plan16368) GM_EDGE_COMP(Plan16000) GM_EDGE_COMP(Plan8000) GM_EDGE_COMP(Plan8192) GM_EDGE_COMP(Plan8184)
    GM_EDGE_COMP(Plan6000) GM_EDGE_COMP(Plan5000) GM_EDGE_COMP(Plan4000)
    return nullptr;
}
EdgeLaunch find_edge_long_fwd_sub(int nb) {
#define GM_EDGE_LONG(PL) if (nb == PL::N) return &launch_long_fwd_sub_edge<PL>;
    GM_EDGE_LONG(Plan16384) GM_EDGE_LONG(Plan16000) GM_EDGE_LONG(Plan10000) GM_EDGE_LONG(Plan8192) GM_EDGE_LONG(Plan8000) GM_EDGE_LONG(Plan4096)
    GM_EDGE_LONG(Plan2048)
    return nullptr;
}

// ------------------------------------------------------------------------------------ the reduction over the hypotheses
// [3][P][H][D] -> [3][P][D] + choice [P][D]: one lane per (listed worker, bin) cell.  The hypothesis with the largest max wins, on equal
// values the lowest h (a strict comparison with h ascending); its three words are copied as they are.  Rows of workers that are not
// listed stay untouched, as stage C leaves them.
__global__ __launch_bounds__(256) void acq_edge_reduce_kernel(const uint32_t* __restrict__ full, uint32_t* __restrict__ met,
                                                              uint32_t* __restrict__ choice, const uint32_t* __restrict__ worker_list,
                                                              uint32_t n_workers, uint32_t P, uint32_t H, uint32_t D) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_workers * D) return;
    const uint32_t w = g / D, d = g - w * D, p = worker_list[w];
    const size_t PHD = size_t(P) * H * D, PD = size_t(P) * D;
    const size_t b = size_t(p) * H * D + d;
    uint32_t bh = 0;
    float bv = __uint_as_float(full[b]);
    for (uint32_t h = 1; h < H; ++h) {
        const float v = __uint_as_float(full[b + size_t(h) * D]);
        if (v > bv) { bv = v; bh = h; }
    }
    const size_t src = b + size_t(bh) * D, dst = size_t(p) * D + d;
    met[dst] = full[src];
    met[PD + dst] = full[PHD + src];
    met[2 * PD + dst] = full[2 * PHD + src];
    choice[dst] = bh;
}

void launch_edge_reduce(hipStream_t st, const uint32_t* full, uint32_t* met, uint32_t* choice, const uint32_t* worker_list,
                        uint32_t n_workers, uint32_t P, uint32_t H, uint32_t D) {
    if (!n_workers || !D) return;
    hipLaunchKernelGGL(acq_edge_reduce_kernel, dim3((n_workers * D + 255) / 256), dim3(256), 0, st, full, met, choice, worker_list,
                       n_workers, P, H, D);
}

}  // namespace gm
