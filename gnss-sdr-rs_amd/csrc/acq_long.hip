// acq_long.hip — acquisition at any fft_size N % 8 == 0 in [1024, 2^18] (gm_acq_cfg.any_length): the lengths that neither the
// in-LDS plans (acq_kernels.hip) nor the composites Q x base with Q in {2..8} (acq_composite.hip) serve.
//
// The transform length is L = Q * Nb, Nb one of the base plans below and Q a RUNTIME factor in [1, 32] (one kernel per base, not
// per (base, Q) pair):
//   native  (GM_ACQ_FORM_LONG)         L = N (50000 = 5 x 10000, 200000 = 20 x 10000, 61440 = 15 x 4096);
//   padded  (GM_ACQ_FORM_LONG_PADDED)  L >= 2N: the circular correlation of length N through a zero-padded periodic extension,
//     x'[n] = mix(x)[n mod N] for n < 2N, 0 up to L;  c'[n] = c[n] for n < N, 0 up to L;
//     IFFT_L(FFT_L(x') conj(FFT_L(c')))[tau] = (L/N) y_ref[tau] for tau < N  (n + tau < 2N <= L: no wrap inside the sum),
//     so only tau < N is kept and every power value is scaled by (N/L)^2.
// Decimated in time like the composites, n = Q*n2 + n1 and k = k1*Nb + k2:
//   forward  F1 long_fwd_sub_kernel   Q in-LDS transforms of length Nb per item over the decimated inputs (mix, mod-N wrap and
//                                      zero padding fused into the loads);
//            F2 long_fwd_post_kernel  twiddle W_L^{n1 k2} + Q-point DFT across n1, in place -> natural order (skipped for Q = 1).
//   inverse  per slab of (worker, bin) items, the slab's intermediate Z sized to stay well inside the Infinity Cache:
//            C1 long_corr_pre_kernel  Y = X conj(C) over k1, inverse Q-point DFT across k1, twiddle W_L^{-n1 k2} -> Z[item][m][n1][k2];
//            C2 long_corr_inv_kernel  one workgroup per (item, n1): in-LDS inverse of length Nb per integration, |y|^2 accumulated
//                                      over the integrations in registers, reduced over tau = Q*n2 + n1 < N to a partial
//                                      {max, first argmax, sum} (strict_sum_order: the power plane is stored as well);
//            C3 long_combine_kernel   the Q partials -> the metric words the decision kernels read.
// Against re-reading the spectra per n1 as comp_corr_kernel does (2 Q L loads per item and integration, and a P Q L x 8 B code table:
// 1.15 GB at 200000 = 20 x 10000 with 36 codes), the slab form moves about 5 L x 8 B per item and integration.
#include "acq_device.h"

namespace gm {

namespace {
constexpr int LCT = 128;              // columns per workgroup of the Q-point DFT kernels (F2, C1)
constexpr uint32_t LQMAX = 32;

// e^{-+ 2 pi i t / n} for integer t in [0, n): the argument is formed from the exact integer phase
__device__ __forceinline__ cf long_root(uint32_t t, uint32_t n, bool inverse) {
    float sn, cs;
    sincospif(2.0f * (float(t) / float(n)), &sn, &cs);
    return cf_make(cs, inverse ? sn : -sn);
}

// ------------------------------------------------------------------------------------ F1
// grid n_items * Q: item = (d, m) for the signal (tables != null), or a code index (code_samples != null).  Input element
// n = Q*n2 + n1 of the length-L sequence: sample n mod N for n < lim (signal: lim = N native, 2N padded; codes: lim = N), else 0.
// A[item][n1][k2], natural order.
template <class PL>
__global__ __launch_bounds__(PL::T) void long_fwd_sub_kernel(const void* __restrict__ samples, int fmt, const cf* __restrict__ tables,
                                                             const int8_t* __restrict__ code_samples, const cf* __restrict__ tw_fwd,
                                                             cf* __restrict__ A, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_fwd, tid);
    const uint32_t item = blockIdx.x / Q, n1 = blockIdx.x - item * Q;
    const uint32_t d = item / n_int, m = item - d * n_int;
    cf* dst = A + size_t(blockIdx.x) * PL::N;
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    auto in = [&](int it, int r) {
        const uint32_t n = Q * uint32_t((tid + it * PL::T) + r * NB0) + n1;
        if (n >= lim) return cf_make(0.0f, 0.0f);
        const uint32_t i = n < N ? n : n - N;
        if (code_samples) return cf_make(float(code_samples[size_t(item) * N + i]), 0.0f);
        const cf s = load_sample(samples, fmt, size_t(m) * N + i);
        const cf t = tables[size_t(d) * N + i];
        return cf_make(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);           // multiply_simd_block
    };
    lds_transform<PL, false>(in, [&](int it, int r, cf val) { dst[(tid + it * PL::T) + r * NBL] = val; }, lds, tw, tid);
}

// ------------------------------------------------------------------------------------ F2
// grid (ceil(Nb / LCT), n_items), in place: X[item][k1][k2] = sum_n1 W_Q^{n1 k1} W_L^{n1 k2} A[item][n1][k2].  A lane owns column
// k2: it reads all Q values of its column before it writes any, so no other lane's data is touched.
__global__ __launch_bounds__(LCT) void long_fwd_post_kernel(cf* __restrict__ X, uint32_t Q, uint32_t Nb) {
    __shared__ cf a[LQMAX * LCT];
    __shared__ cf wq[LQMAX];
    const int tid = threadIdx.x;
    const uint32_t k2 = blockIdx.x * LCT + tid, L = Q * Nb;
    if (uint32_t(tid) < Q) wq[tid] = long_root(tid, Q, false);
    const bool on = k2 < Nb;
    cf* col = X + size_t(blockIdx.y) * L + k2;
    if (on)
        for (uint32_t n1 = 0; n1 < Q; ++n1)
            a[n1 * LCT + tid] = cf_mul(col[size_t(n1) * Nb], long_root(uint32_t((uint64_t(n1) * k2) % L), L, false));
    __syncthreads();
    if (!on) return;
    for (uint32_t k1 = 0; k1 < Q; ++k1) {
        cf acc = a[tid];
        uint32_t j = 0;
        for (uint32_t n1 = 1; n1 < Q; ++n1) {
            j += k1; if (j >= Q) j -= Q;                       // (n1 k1) mod Q
            acc = cf_add(acc, cf_mul(a[n1 * LCT + tid], wq[j]));
        }
        col[size_t(k1) * Nb] = acc;
    }
}

// ------------------------------------------------------------------------------------ C1
// grid (ceil(Nb / LCT), n_slab * n_int): item g = item0 + blockIdx.y / n_int of the bin-major list (g = d * n_workers + w).
// Z[s][m][n1][k2] = W_L^{-n1 k2} sum_k1 W_Q^{-n1 k1} X[d][m][k1][k2] conj(C[p][k1][k2])
__global__ __launch_bounds__(LCT) void long_corr_pre_kernel(const cf* __restrict__ X, const cf* __restrict__ C, cf* __restrict__ Z,
                                                            const uint32_t* __restrict__ worker_list, uint32_t n_workers, uint32_t item0,
                                                            uint32_t Q, uint32_t Nb, uint32_t n_int) {
    __shared__ cf y[LQMAX * LCT];
    __shared__ cf wq[LQMAX];
    const int tid = threadIdx.x;
    const uint32_t k2 = blockIdx.x * LCT + tid, L = Q * Nb;
    const uint32_t s = blockIdx.y / n_int, m = blockIdx.y - s * n_int, g = item0 + s;
    const uint32_t d = g / n_workers, p = worker_list[g - d * n_workers];
    if (uint32_t(tid) < Q) wq[tid] = long_root(tid, Q, true);
    const bool on = k2 < Nb;
    if (on) {
        const cf* xs = X + (size_t(d) * n_int + m) * L + k2;
        const cf* cs = C + size_t(p) * L + k2;
        for (uint32_t k1 = 0; k1 < Q; ++k1) {
            const cf c = cs[size_t(k1) * Nb];
            y[k1 * LCT + tid] = cf_mul(xs[size_t(k1) * Nb], cf_make(c.x, -c.y));
        }
    }
    __syncthreads();
    if (!on) return;
    cf* zs = Z + (size_t(s) * n_int + m) * L + k2;
    for (uint32_t n1 = 0; n1 < Q; ++n1) {
        cf acc = y[tid];
        uint32_t j = 0;
        for (uint32_t k1 = 1; k1 < Q; ++k1) {
            j += n1; if (j >= Q) j -= Q;                       // (n1 k1) mod Q
            acc = cf_add(acc, cf_mul(y[k1 * LCT + tid], wq[j]));
        }
        zs[size_t(n1) * Nb] = cf_mul(acc, long_root(uint32_t((uint64_t(n1) * k2) % L), L, true));
    }
}

// ------------------------------------------------------------------------------------ C2
// grid n_slab * Q: one workgroup per (item, n1).  Outputs of the sub-transform are y[Q n2 + n1]; tau = Q n2 + n1 >= N (padded form)
// is dropped.  Partials at [g * Q + n1].  planes (strict_sum_order): [(p * n_bins + d) * N + tau] = the scaled power.
template <class PL>
__global__ __launch_bounds__(PL::T) void long_corr_inv_kernel(const cf* __restrict__ Z, const cf* __restrict__ tw_inv,
                                                              float* __restrict__ pmax, uint32_t* __restrict__ parg, float* __restrict__ psum,
                                                              float* __restrict__ planes, const uint32_t* __restrict__ worker_list,
                                                              uint32_t n_workers, uint32_t n_bins, uint32_t item0, uint32_t Q, uint32_t N,
                                                              uint32_t n_int, float scale) {
    static_assert(!PL::COPRIME && !PL::HYBRID, "long-path bases: plain plans with twiddles");
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    cf* tw = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(tw, tw_inv, tid);
    constexpr int NB0 = PL::NB(0), NBL = PL::NB(PL::NP - 1);
    const uint32_t s = blockIdx.x / Q, n1 = blockIdx.x - s * Q, g = item0 + s;
    const size_t L = size_t(Q) * PL::N;
    float acc[PL::ITL][PL::RL];
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it)
#pragma unroll
        for (int r = 0; r < PL::RL; ++r) acc[it][r] = 0.0f;
    for (uint32_t m = 0; m < n_int; ++m) {
        const cf* src = Z + (size_t(s) * n_int + m) * L + size_t(n1) * PL::N;
        lds_transform<PL, true>([&](int it, int r) { return src[(tid + it * PL::T) + r * NB0]; },
                                [&](int it, int r, cf v) { acc[it][r] = acc[it][r] + (v.x * v.x + v.y * v.y); },
                                lds, tw, tid);
    }
    const uint32_t d = g / n_workers, p = worker_list[g - d * n_workers];
    float bv = 0.0f, sum = 0.0f;
    uint32_t bi = 0xffffffffu;
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it) {
        if (tid + it * PL::T < NBL) {
#pragma unroll
            for (int r = 0; r < PL::RL; ++r) {
                const uint32_t tau = Q * uint32_t((tid + it * PL::T) + r * NBL) + n1;
                if (tau < N) {
                    const float v = acc[it][r] * scale;
                    take_better(bv, bi, v, tau);
                    sum += v;
                    if (planes) planes[(size_t(p) * n_bins + d) * N + tau] = v;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const uint32_t oi = uint32_t(__shfl_xor(int(bi), off, 64));
        const float os = __shfl_xor(sum, off, 64);
        take_better(bv, bi, ov, oi);
        sum += os;
    }
    __syncthreads();   // everyone is done with the LDS transform buffer: reuse it as scratch
    float* sv = reinterpret_cast<float*>(lds);
    uint32_t* si = reinterpret_cast<uint32_t*>(lds) + 64;
    float* ss = reinterpret_cast<float*>(lds) + 128;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int NW = PL::T / 64;
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; ss[wave] = sum; }
    __syncthreads();
    if (tid == 0) {
        float fv = sv[0], fs = ss[0];
        uint32_t fi = si[0];
        for (int w = 1; w < NW; ++w) { take_better(fv, fi, sv[w], si[w]); fs += ss[w]; }
        const size_t o = size_t(g) * Q + n1;
        pmax[o] = fv; parg[o] = fi; psum[o] = fs;
    }
}

// ------------------------------------------------------------------------------------ C3
// one lane per item: the maximum of the partials, the smallest tau among those that attain it, the sum of the partials
__global__ __launch_bounds__(256) void long_combine_kernel(const float* __restrict__ pmax, const uint32_t* __restrict__ parg,
                                                           const float* __restrict__ psum, float* __restrict__ mmax,
                                                           uint32_t* __restrict__ margmax, float* __restrict__ msum,
                                                           const uint32_t* __restrict__ worker_list, uint32_t n_workers, uint32_t n_bins,
                                                           uint32_t Q, uint32_t n_items) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_items) return;
    const uint32_t d = g / n_workers, p = worker_list[g - d * n_workers];
    const size_t b = size_t(g) * Q;
    float bv = pmax[b], sum = psum[b];
    uint32_t bi = parg[b];
    for (uint32_t n1 = 1; n1 < Q; ++n1) {
        take_better(bv, bi, pmax[b + n1], parg[b + n1]);
        sum += psum[b + n1];
    }
    if (bi == 0xffffffffu) bi = 0;   // all-NaN / all-zero plane: the reference keeps (0.0, 0)
    const size_t o = size_t(p) * n_bins + d;
    mmax[o] = bv; margmax[o] = bi; msum[o] = sum;
}

template <class PL> struct LongLaunch {
    static void fwd_sub(hipStream_t st, const void* samples, int fmt, const cf* tables, const int8_t* code_samples, const cf* tw_fwd,
                        cf* A, uint32_t n_items, uint32_t Q, uint32_t N, uint32_t lim, uint32_t n_int) {
        hipLaunchKernelGGL(long_fwd_sub_kernel<PL>, dim3(n_items * Q), dim3(PL::T), 0, st, samples, fmt, tables, code_samples, tw_fwd, A,
                           Q, N, lim, n_int);
    }
    static void corr_inv(hipStream_t st, const cf* Z, const cf* tw_inv, float* pmax, uint32_t* parg, float* psum, float* planes,
                         const uint32_t* worker_list, uint32_t n_workers, uint32_t n_bins, uint32_t item0, uint32_t n_slab, uint32_t Q,
                         uint32_t N, uint32_t n_int, float scale) {
        hipLaunchKernelGGL(long_corr_inv_kernel<PL>, dim3(n_slab * Q), dim3(PL::T), 0, st, Z, tw_inv, pmax, parg, psum, planes,
                           worker_list, n_workers, n_bins, item0, Q, N, n_int, scale);
    }
    static constexpr LongOps ops() { return LongOps{PL::N, &fwd_sub, &corr_inv}; }
};
}  // namespace

// largest base first: the native form takes the largest Nb that divides N
static const LongOps g_long[] = {LongLaunch<Plan16384>::ops(), LongLaunch<Plan16000>::ops(), LongLaunch<Plan10000>::ops(),
                                 LongLaunch<Plan8192>::ops(), LongLaunch<Plan8000>::ops(), LongLaunch<Plan4096>::ops(),
                                 LongLaunch<Plan2048>::ops()};

const LongOps* long_bases(int* n) {
    *n = int(sizeof(g_long) / sizeof(g_long[0]));
    return g_long;
}

void launch_long_fwd_post(hipStream_t st, cf* X, uint32_t n_items, uint32_t Q, uint32_t Nb) {
    if (Q <= 1 || !n_items) return;
    hipLaunchKernelGGL(long_fwd_post_kernel, dim3((Nb + LCT - 1) / LCT, n_items), dim3(LCT), 0, st, X, Q, Nb);
}

void launch_long_corr(hipStream_t st, const LongOps* lo, const LongCorrArgs& a, gm_acq_corr_grid_info* rec) {
    const uint32_t items = a.n_workers * a.n_bins;
    if (!items) return;
    if (rec) {
        *rec = gm_acq_corr_grid_info{};
        rec->path = GM_CORR_PATH_LONG;
        rec->n_workers = int32_t(a.n_workers); rec->n_bins = int32_t(a.n_bins); rec->n_int = int32_t(a.n_int);
        rec->long_slab = a.slab_items;
    }
    for (uint32_t item0 = 0; item0 < items; item0 += a.slab_items) {
        const uint32_t n = items - item0 < a.slab_items ? items - item0 : a.slab_items;
        hipLaunchKernelGGL(long_corr_pre_kernel, dim3((a.Nb + LCT - 1) / LCT, n * a.n_int), dim3(LCT), 0, st, a.spectra, a.code_fft,
                           a.Z, a.worker_list, a.n_workers, item0, a.Q, a.Nb, a.n_int);
        lo->corr_inv(st, a.Z, a.tw_inv, a.pmax, a.parg, a.psum, a.planes, a.worker_list, a.n_workers, a.n_bins, item0, n, a.Q, a.N,
                     a.n_int, a.scale);
        if (rec) ++rec->long_slabs;      // counted where the slabs are launched
    }
    hipLaunchKernelGGL(long_combine_kernel, dim3((items + 255) / 256), dim3(256), 0, st, a.pmax, a.parg, a.psum, a.mmax, a.margmax,
                       a.msum, a.worker_list, a.n_workers, a.n_bins, a.Q, items);
}

}  // namespace gm
