// acq_cancel.hip — subtract found satellites from a dwell (gm_acq_cancel).
//
// A candidate's replica runs on the SIGNAL's own code periods (o_k = cp + (q0 + k) T, any real T within 8 of N), not on the handle's:
// segment k is the samples b_k <= n < b_{k+1} of the host-built table b, and inside it
//   r[n] = c_w[min(L - 1, floor((n - o_k) L / T))] * exp(j 2 pi frac(n f / fs))
// with the chip index and the cycles in f64 and the sine / cosine in f32 on the reduced turn, as acq_refine_scan_kernel forms them.
// Two kernels; neither knows the handle's stage-C form:
//   acq_cancel_amp_kernel       a[c][k] = (1 / n_k) sum_{n in segment k} x[n] conj(r_c[n]): one 256-lane workgroup per (segment, candidate)
//   acq_cancel_subtract_kernel  y[n] = x[n] - sum_c a[c][k_c(n)] r_c[n] (int8 real: 2 Re of the term, Im y = 0), candidates ascending, c32 out
// Both walk the dwell in chunks of eight samples that start on multiples of 8 of the DWELL (not of the segment), so a chunk is 16 bytes of
// int8 IQ, 8 of int8 real, 64 of c32, aligned wherever the dwell's first byte is, whatever sample a segment starts on; the samples of a
// chunk outside the segment are masked.  Only the dwell's last chunk can be short (a drift dwell is no multiple of 8): it is read and
// written sample by sample.
// Sums run in a fixed order (per-lane partial sums in ascending n, a wave64 shuffle tree, four LDS words added by one lane): no
// floating-point atomics, so two calls give the same words.  The unit builds with -ffp-contract=off like the rest.
#include "acq_device.h"
#include "acq_load8.h"

namespace gm {
namespace {

constexpr int CANCEL_T = 256;            // lanes per workgroup of both kernels
constexpr int CANCEL_CHUNK = 8;          // consecutive samples per lane and step

template <int FMT> constexpr int bytes_per_sample() { return FMT == GM_FMT_C32 ? 8 : (FMT == GM_FMT_I8_IQ ? 2 : 1); }

// the chunk of eight samples from n0 (a multiple of 8, n0 < D): whole chunks through load8, the dwell's short last chunk sample by
// sample with zeros behind the end
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void load_chunk(const char* samples, uint64_t n0, uint64_t D, float (&xr)[8], float (&xi)[8]) {
    if (n0 + CANCEL_CHUNK <= D) {
        load8<FMT, ALIGNED>(samples + n0 * uint64_t(bytes_per_sample<FMT>()), xr, xi);
    } else {
#pragma unroll
        for (int e = 0; e < CANCEL_CHUNK; ++e) {
            cf v = cf_make(0.0f, 0.0f);
            if (n0 + e < D) v = load_sample(samples, FMT, size_t(n0 + e));
            xr[e] = v.x; xi[e] = v.y;
        }
    }
}

// r[n] of a candidate inside the segment that starts at o (n >= o: e >= 0)
__device__ __forceinline__ void replica(const CancelCand& cc, const int8_t* __restrict__ chips, double o, uint64_t n, float& rr, float& ri) {
    const double e = double(n) - o;
    const uint32_t i = uint32_t(floor(e * cc.cpl));
    const uint32_t idx = i < cc.L - 1 ? i : cc.L - 1;
    const double cyc = double(n) * cc.fq;
    const float turn = float(2.0 * (cyc - floor(cyc)));
    const float ch = float(chips[idx]);
    rr = ch * cospif(turn);
    ri = ch * sinpif(turn);
}

template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(CANCEL_T) void acq_cancel_amp_kernel(const char* __restrict__ samples, uint64_t D,
                                                                  const CancelCand* __restrict__ cands, const double* __restrict__ o_tab,
                                                                  const uint64_t* __restrict__ b_tab, uint32_t stride,
                                                                  const int8_t* __restrict__ chips, cf* __restrict__ amps) {
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x, cand = blockIdx.y;
    const CancelCand cc = cands[cand];
    if (k >= cc.Q) return;                                       // (uniform: the grid is the largest Q of the call)
    const size_t row = size_t(cand) * stride;
    const uint64_t lo = b_tab[row + k], hi = b_tab[row + k + 1];
    if (hi <= lo) {                                              // an empty segment (the dwell ends on its first sample): a_k = 0
        if (tid == 0) amps[row + k] = cf_make(0.0f, 0.0f);
        return;
    }
    const double o = o_tab[row + k];
    const int8_t* cw = chips + size_t(cc.worker) * cc.L;
    float ar = 0.0f, ai = 0.0f;
    for (uint64_t n0 = (lo & ~uint64_t(7)) + uint64_t(tid) * CANCEL_CHUNK; n0 < hi; n0 += uint64_t(CANCEL_T) * CANCEL_CHUNK) {
        float xr[8], xi[8];
        load_chunk<FMT, ALIGNED>(samples, n0, D, xr, xi);
#pragma unroll
        for (int e = 0; e < CANCEL_CHUNK; ++e) {
            const uint64_t n = n0 + e;
            if (n >= lo && n < hi) {
                float rr, ri;
                replica(cc, cw, o, n, rr, ri);
                ar += xr[e] * rr + xi[e] * ri;                   // x conj(r)
                ai += xi[e] * rr - xr[e] * ri;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_down(ar, off, 64);
        ai += __shfl_down(ai, off, 64);
    }
    __shared__ float red[CANCEL_T / 64][2];
    if ((tid & 63) == 0) { red[tid >> 6][0] = ar; red[tid >> 6][1] = ai; }
    __syncthreads();
    if (tid == 0) {
        float re = red[0][0], im = red[0][1];
#pragma unroll
        for (int v = 1; v < CANCEL_T / 64; ++v) { re += red[v][0]; im += red[v][1]; }
        const float nk = float(hi - lo);                         // (n_k <= N + 9: exact)
        amps[row + k] = cf_make(re / nk, im / nk);
    }
}

// Lane g takes the chunk from 8 g.  Per candidate it finds the segment of the chunk's first sample — a guess from (n - cp) / T, corrected
// against the b table, which is the definition — and steps to the next segment where a later sample of the chunk has passed b_{k+1}.
// A lane reads its x[n] before it writes its y[n] and touches no other sample: d_out may be the c32 input (so `samples` and `out` are
// not declared restrict).
template <int FMT, bool ALIGNED, bool OUT_ALIGNED>
__global__ __launch_bounds__(CANCEL_T) void acq_cancel_subtract_kernel(const char* samples, uint64_t D,
                                                                       const CancelCand* __restrict__ cands, uint32_t n_cands,
                                                                       const double* __restrict__ o_tab, const uint64_t* __restrict__ b_tab,
                                                                       uint32_t stride, const int8_t* __restrict__ chips,
                                                                       const cf* __restrict__ amps, cf* out) {
    const uint64_t n0 = (uint64_t(blockIdx.x) * CANCEL_T + threadIdx.x) * CANCEL_CHUNK;
    if (n0 >= D) return;
    float yr[8], yi[8];
    load_chunk<FMT, ALIGNED>(samples, n0, D, yr, yi);
    const uint32_t cnt = D - n0 < CANCEL_CHUNK ? uint32_t(D - n0) : uint32_t(CANCEL_CHUNK);
    for (uint32_t c = 0; c < n_cands; ++c) {
        const CancelCand cc = cands[c];                          // (uniform over the grid)
        const size_t row = size_t(c) * stride;
        const uint64_t* b = b_tab + row;
        double g = floor((double(n0) - cc.cp) * cc.inv_T) - double(cc.q0);
        g = g < 0.0 ? 0.0 : g;
        uint32_t k = g < double(cc.Q - 1) ? uint32_t(g) : cc.Q - 1;
        while (k > 0 && n0 < b[k]) --k;                          // (b_0 = 0 <= n0 < D = b_Q: both walks end inside the table)
        while (k + 1 < cc.Q && n0 >= b[k + 1]) ++k;
        uint64_t next = b[k + 1];
        double o = o_tab[row + k];
        cf a = amps[row + k];
        const int8_t* cw = chips + size_t(cc.worker) * cc.L;
#pragma unroll
        for (int e = 0; e < CANCEL_CHUNK; ++e) {
            const uint64_t n = n0 + e;
            if (uint32_t(e) < cnt) {
                while (n >= next) {                              // (n < D = b_Q: k stays below Q)
                    ++k;
                    next = b[k + 1];
                    o = o_tab[row + k];
                    a = amps[row + k];
                }
                float rr, ri;
                replica(cc, cw, o, n, rr, ri);
                if constexpr (FMT == GM_FMT_I8_REAL) {
                    yr[e] = yr[e] - 2.0f * (a.x * rr - a.y * ri);                  // 2 Re(a r)
                } else {
                    yr[e] = yr[e] - (a.x * rr - a.y * ri);
                    yi[e] = yi[e] - (a.x * ri + a.y * rr);
                }
            }
        }
    }
    cf* yp = out + n0;
    if (OUT_ALIGNED && cnt == CANCEL_CHUNK) {
        float4* y4 = reinterpret_cast<float4*>(yp);
#pragma unroll
        for (int e = 0; e < 4; ++e) y4[e] = make_float4(yr[2 * e], yi[2 * e], yr[2 * e + 1], yi[2 * e + 1]);
    } else {
#pragma unroll
        for (int e = 0; e < CANCEL_CHUNK; ++e)
            if (uint32_t(e) < cnt) yp[e] = cf_make(yr[e], yi[e]);
    }
}

template <int FMT, bool ALIGNED> void launch_fmt(hipStream_t st, const CancelArgs& a) {
    const char* sp = static_cast<const char*>(a.samples);
    if (a.n_cands)
        hipLaunchKernelGGL((acq_cancel_amp_kernel<FMT, ALIGNED>), dim3(a.q_max, a.n_cands), dim3(CANCEL_T), 0, st, sp, a.D, a.cands, a.o,
                           a.b, a.stride, a.chips, a.amps);
    const uint32_t blocks = uint32_t((a.D + uint64_t(CANCEL_T) * CANCEL_CHUNK - 1) / (uint64_t(CANCEL_T) * CANCEL_CHUNK));
    if ((reinterpret_cast<uintptr_t>(a.out) & 15u) == 0)
        hipLaunchKernelGGL((acq_cancel_subtract_kernel<FMT, ALIGNED, true>), dim3(blocks), dim3(CANCEL_T), 0, st, sp, a.D, a.cands,
                           a.n_cands, a.o, a.b, a.stride, a.chips, a.amps, a.out);
    else
        hipLaunchKernelGGL((acq_cancel_subtract_kernel<FMT, ALIGNED, false>), dim3(blocks), dim3(CANCEL_T), 0, st, sp, a.D, a.cands,
                           a.n_cands, a.o, a.b, a.stride, a.chips, a.amps, a.out);
}

}  // namespace

void launch_cancel(hipStream_t st, const CancelArgs& a) {
    // a chunk starts a multiple of 8 samples into the dwell: its loads are aligned where the dwell's first byte is
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.samples);
    if (a.fmt == GM_FMT_C32) {
        if ((p & 15u) == 0) launch_fmt<GM_FMT_C32, true>(st, a); else launch_fmt<GM_FMT_C32, false>(st, a);
    } else if (a.fmt == GM_FMT_I8_IQ) {
        if ((p & 15u) == 0) launch_fmt<GM_FMT_I8_IQ, true>(st, a); else launch_fmt<GM_FMT_I8_IQ, false>(st, a);
    } else {
        if ((p & 7u) == 0) launch_fmt<GM_FMT_I8_REAL, true>(st, a); else launch_fmt<GM_FMT_I8_REAL, false>(st, a);
    }
}

}  // namespace gm
