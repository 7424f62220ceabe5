// acq_refine.hip — fine Doppler from per-period prompts (gm_acq_refine_doppler).
//
// Two kernels, neither of which knows the handle's stage-C form (the mix tables and the replicas are [.][N] in natural order on every
// form, padded-long handles included):
//   acq_despread_kernel     z[i] = sum_n x[s[d][o + i] + n] tab[d][n] c_w[(n - cp) mod N]: the circular correlation value at lag cp of
//                           period o + i alone, read from where the search read it.  One 256-lane workgroup per (period, satellite).
//   acq_refine_scan_kernel  S[j] = N^2 sum_g | sum_k sigma_k w_{g,k}(delta_j) z[g J + k] |^2 on the Z grid points, then the first index
//                           of the maximum.  One workgroup per satellite, lanes over j.
// Sums run in a fixed order (per-lane partial sums, a wave64 shuffle tree, four LDS words added by one lane): no floating-point atomics,
// so two calls give the same words.  The unit builds with -ffp-contract=off like the rest: the sample-table product rounds as stage F's.
#include "acq_device.h"
#include "acq_load8.h"

namespace gm {
namespace {

constexpr int REFINE_T = 256;            // lanes per workgroup of both kernels
constexpr int REFINE_CHUNK = 8;          // consecutive samples one lane takes per step (fft_size is a multiple of 8)

// one lane's share of the N-term sum: chunks tid, tid + 256, ... of eight samples, the terms of a chunk added in ascending n.
// The table row is 64 bytes per chunk (four 16-byte loads, the row and the chunk are 64-byte aligned); the rotated replica is two
// contiguous runs around cp: the eight chips from (n0 - cp) mod N on sit in two aligned 8-byte words of the row (N is a multiple of
// 8, so a word never straddles the wrap; the word after the last is the first).
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void despread_sum(const char* __restrict__ sp, const cf* __restrict__ tab, const int8_t* __restrict__ rep,
                                             uint32_t N, uint32_t cp, int tid, float& ar, float& ai) {
    constexpr int BPS = FMT == GM_FMT_C32 ? 8 : (FMT == GM_FMT_I8_IQ ? 2 : 1);
    for (uint32_t n0 = uint32_t(tid) * REFINE_CHUNK; n0 < N; n0 += REFINE_T * REFINE_CHUNK) {
        float xr[8], xi[8];
        load8<FMT, ALIGNED>(sp + size_t(n0) * BPS, xr, xi);
        const float4* t4 = reinterpret_cast<const float4*>(tab + n0);
        const uint32_t m0 = n0 >= cp ? n0 - cp : n0 + N - cp;
        const uint32_t a0 = m0 & ~7u, a1 = a0 + 8 == N ? 0u : a0 + 8, sh = (m0 & 7u) * 8;
        const unsigned long long lo = *reinterpret_cast<const unsigned long long*>(rep + a0);
        const unsigned long long hi = *reinterpret_cast<const unsigned long long*>(rep + a1);
        const unsigned long long c8 = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 t = t4[e];
            const float c0 = float(int8_t(c8 >> (16 * e))), c1 = float(int8_t(c8 >> (16 * e + 8)));
            // multiply_simd_block (doppler_shift.rs:43-58), as stage F forms it; the chip is +-1: that product is exact
            ar += (xr[2 * e] * t.x - xi[2 * e] * t.y) * c0;
            ai += (xr[2 * e] * t.y + xi[2 * e] * t.x) * c0;
            ar += (xr[2 * e + 1] * t.z - xi[2 * e + 1] * t.w) * c1;
            ai += (xr[2 * e + 1] * t.w + xi[2 * e + 1] * t.z) * c1;
        }
    }
}

__global__ __launch_bounds__(REFINE_T) void acq_despread_kernel(const void* __restrict__ samples, int fmt,
                                                                const uint64_t* __restrict__ starts, uint32_t R,
                                                                const cf* __restrict__ tables, const int8_t* __restrict__ code_samples,
                                                                const RefineSat* __restrict__ sats, uint32_t N, uint32_t R_u,
                                                                cf* __restrict__ z) {
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x, sat = blockIdx.y;
    const RefineSat w = sats[sat];
    // the period's start, a 64-bit element offset, uniform over the workgroup (as DriftLoad::start reads it): the address of sample n
    // is a scalar base plus the lane's n
    uint64_t s = starts ? starts[size_t(w.bin) * R + w.offset + i] : uint64_t(w.offset + i) * N;
    s = uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s))) | (uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s >> 32))) << 32);
    const uint32_t cp = __builtin_amdgcn_readfirstlane(w.code_phase);
    const cf* tab = tables + size_t(w.bin) * N;
    const int8_t* rep = code_samples + size_t(w.worker) * N;
    float ar = 0.0f, ai = 0.0f;
    if (fmt == GM_FMT_C32) {
        const char* sp = static_cast<const char*>(samples) + s * 8;
        if ((reinterpret_cast<uintptr_t>(sp) & 15u) == 0) despread_sum<GM_FMT_C32, true>(sp, tab, rep, N, cp, tid, ar, ai);
        else despread_sum<GM_FMT_C32, false>(sp, tab, rep, N, cp, tid, ar, ai);
    } else if (fmt == GM_FMT_I8_IQ) {
        const char* sp = static_cast<const char*>(samples) + s * 2;
        if ((reinterpret_cast<uintptr_t>(sp) & 15u) == 0) despread_sum<GM_FMT_I8_IQ, true>(sp, tab, rep, N, cp, tid, ar, ai);
        else despread_sum<GM_FMT_I8_IQ, false>(sp, tab, rep, N, cp, tid, ar, ai);
    } else {
        const char* sp = static_cast<const char*>(samples) + s;
        if ((reinterpret_cast<uintptr_t>(sp) & 7u) == 0) despread_sum<GM_FMT_I8_REAL, true>(sp, tab, rep, N, cp, tid, ar, ai);
        else despread_sum<GM_FMT_I8_REAL, false>(sp, tab, rep, N, cp, tid, ar, ai);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_down(ar, off, 64);
        ai += __shfl_down(ai, off, 64);
    }
    __shared__ float red[REFINE_T / 64][2];
    if ((tid & 63) == 0) { red[tid >> 6][0] = ar; red[tid >> 6][1] = ai; }
    __syncthreads();
    if (tid == 0) {
        float re = red[0][0], im = red[0][1];
#pragma unroll
        for (int v = 1; v < REFINE_T / 64; ++v) { re += red[v][0]; im += red[v][1]; }
        z[size_t(sat) * R_u + i] = cf_make(re, im);
    }
}

// STAGED: the satellite's R_u prompts and period times sit in LDS (R_u <= REFINE_STAGE_MAX: 16 KiB); else they are read from global
// memory each time (an L1 / L2 hit: every lane reads the same word)
constexpr uint32_t REFINE_STAGE_MAX = 1024;

template <bool STAGED>
__global__ __launch_bounds__(REFINE_T) void acq_refine_scan_kernel(const cf* __restrict__ z, const double* __restrict__ t,
                                                                   const double* __restrict__ fc, const double* __restrict__ step,
                                                                   uint32_t neg, uint32_t J, uint32_t G, uint32_t Z, float n2,
                                                                   float* __restrict__ spectrum, float* __restrict__ peak_val,
                                                                   uint32_t* __restrict__ peak_idx) {
    const int tid = threadIdx.x;
    const uint32_t sat = blockIdx.x, R_u = G * J;
    const cf* zp = z + size_t(sat) * R_u;
    const double* tp = t + size_t(sat) * R_u;
    __shared__ cf z_s[STAGED ? REFINE_STAGE_MAX : 1];
    __shared__ double t_s[STAGED ? REFINE_STAGE_MAX : 1];
    if constexpr (STAGED) {
        for (uint32_t i = tid; i < R_u; i += REFINE_T) { z_s[i] = zp[i]; t_s[i] = tp[i]; }
        __syncthreads();
    }
    const double f0 = fc[sat], st = step[sat];
    const int half = int(Z >> 1);
    float bv = -1.0f;
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t j = tid; j < Z; j += REFINE_T) {
        const double f = f0 + double(int(j) - half) * st;
        float tot = 0.0f;
        uint32_t idx = 0;
        for (uint32_t g = 0; g < G; ++g) {
            float are = 0.0f, aim = 0.0f;
            for (uint32_t k = 0; k < J; ++k, ++idx) {
                const double tk = STAGED ? t_s[idx] : tp[idx];
                const cf v = STAGED ? z_s[idx] : zp[idx];
                // the cycles in f64, reduced to one cycle before the angle (as the coherent and drift phasor words are formed)
                const double cyc = f * tk;
                const float turn = float(2.0 * (cyc - floor(cyc)));
                const float c = cospif(turn), s = sinpif(turn);           // w = exp(-j 2 pi frac) = (c, -s)
                const float pr = c * v.x + s * v.y, pi = c * v.y - s * v.x;
                if ((neg >> k) & 1u) { are -= pr; aim -= pi; }
                else { are += pr; aim += pi; }
            }
            tot += are * are + aim * aim;
        }
        const float S = tot * n2;
        spectrum[size_t(sat) * Z + j] = S;
        take_better(bv, bi, S, j);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(bv, off, 64);
        const uint32_t oi = __shfl_down(bi, off, 64);
        take_better(bv, bi, ov, oi);
    }
    __shared__ float rv[REFINE_T / 64];
    __shared__ uint32_t ri[REFINE_T / 64];
    if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < REFINE_T / 64; ++v) take_better(bv, bi, rv[v], ri[v]);
        peak_val[sat] = bv;
        peak_idx[sat] = bi;
    }
}

}  // namespace

void launch_refine(hipStream_t st, const RefineArgs& a) {
    hipLaunchKernelGGL(acq_despread_kernel, dim3(a.R_u, a.n_sats), dim3(REFINE_T), 0, st, a.samples, a.fmt, a.starts, a.R, a.tables,
                       a.code_samples, a.sats, a.N, a.R_u, a.z);
    const float n2 = float(double(a.N) * double(a.N));
    if (a.R_u <= REFINE_STAGE_MAX)
        hipLaunchKernelGGL(acq_refine_scan_kernel<true>, dim3(a.n_sats), dim3(REFINE_T), 0, st, a.z, a.t, a.fc, a.step, a.neg, a.J, a.G,
                           a.Z, n2, a.spectrum, a.peak_val, a.peak_idx);
    else
        hipLaunchKernelGGL(acq_refine_scan_kernel<false>, dim3(a.n_sats), dim3(REFINE_T), 0, st, a.z, a.t, a.fc, a.step, a.neg, a.J, a.G,
                           a.Z, n2, a.spectrum, a.peak_val, a.peak_idx);
}

}  // namespace gm
