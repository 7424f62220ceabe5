// acq_local.hip — lag window x fine Doppler at known cells (gm_acq_local_search).
//
// Three kernels; none knows the handle's stage-C form (the mix tables and the replicas are [.][N] in natural order on every form):
//   acq_local_despread_kernel  z[l][i] = sum_n x[s[d][o + i] + n] tab[d][n] c_w[(n - lambda_l) mod N] for ALL W = 2L + 1 lags
//                              lambda_l = (cp + l - L) mod N of one (period, candidate) from ONE pass over the samples: the period is
//                              cut into tiles of 2048 samples; a tile's sample x table products (formed once, as stage F forms them)
//                              and the tile's replica chips plus 2L sit in LDS; every lag's sum reads them from there.
//   acq_local_scan_kernel      S[l][j] of gm_acq_refine_doppler's statistic on the Z grid points of one (lag, candidate), the row's first
//                              maximum and the row's sum (f64).
//   acq_local_pick_kernel      per candidate: the first maximum in (l, j) order, its four neighbours and the floor's sum.
//
// The despreading workgroup (256 lanes) is nsl = 256 / P2 slices of P2 lanes, P2 = the power of two >= W within 8 .. 64.  A slice owns
// 2048 / nsl consecutive samples of every tile; lane ls of a slice owns the lags ls, ls + P2, ls + 2 P2 (< W; at most three: W <= 129)
// and adds its slice's terms in ascending n, tile after tile, into registers.  After the last tile the slices' partial sums meet in
// LDS and one lane per lag adds them in ascending slice order: a fixed order, no floating-point atomics, so a candidate's words depend on
// the candidate and the samples alone.
//
// LDS layout.  Element q of the product and chip arrays sits at word q + 4 (q >> 6): four pad words per 64 keep a lane's eight
// products 16-byte aligned (two 16-byte writes per array) and move slices, which start a multiple of 64 samples apart, four banks apart
// per 64 — the lanes of one slice read the SAME product word (a broadcast) and consecutive chip words, and the two to four slices of a
// 32-lane half then sit on different banks (ds_read_b32: bank = word mod 32 within a 32-lane half).
#include "acq_device.h"
#include "acq_load8.h"

namespace gm {
namespace {

constexpr int LOCAL_T = 256;                      // lanes per workgroup of the despreading and scan kernels
constexpr int LOCAL_TILE = LOCAL_T * 8;           // samples per tile: eight per lane
constexpr int LOCAL_LMAX = 64;                    // the largest lag_half_window
constexpr int LOCAL_WMAX = 2 * LOCAL_LMAX + 1;
constexpr int LOCAL_LB = 3;                       // lags per lane at most: ceil(129 / 64)

__host__ __device__ constexpr int lpad(int q) { return q + ((q >> 6) << 2); }
constexpr int LOCAL_PROD_WORDS = lpad(LOCAL_TILE - 1) + 1;                        // 2172
constexpr int LOCAL_CHIP_WORDS = lpad(LOCAL_TILE + 2 * LOCAL_LMAX - 1) + 1;       // 2308
constexpr int LOCAL_ACC_WORDS = 4 * LOCAL_WMAX;                                   // nsl * W <= 516 (P2 = 64: 4 slices of 129 lags)

// a tile's products x[n] tab[n] into LDS: lane tid forms samples n0 + 8 tid .. + 7 (multiply_simd_block, doppler_shift.rs:43-58, as
// stage F forms it; the unit builds with -ffp-contract=off)
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void stage_products(const char* __restrict__ sp, const cf* __restrict__ tab, uint32_t n0, uint32_t tl, int tid,
                                               float* __restrict__ pr_s, float* __restrict__ pi_s) {
    constexpr int BPS = FMT == GM_FMT_C32 ? 8 : (FMT == GM_FMT_I8_IQ ? 2 : 1);
    const uint32_t t0 = uint32_t(tid) * 8;
    if (t0 >= tl) return;                         // (tl is a multiple of 8: a lane's eight samples are inside the period or not at all)
    float xr[8], xi[8];
    load8<FMT, ALIGNED>(sp + size_t(n0 + t0) * BPS, xr, xi);
    const float4* t4 = reinterpret_cast<const float4*>(tab + n0 + t0);
    float pr[8], pi[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float4 t = t4[e];
        pr[2 * e] = xr[2 * e] * t.x - xi[2 * e] * t.y;
        pi[2 * e] = xr[2 * e] * t.y + xi[2 * e] * t.x;
        pr[2 * e + 1] = xr[2 * e + 1] * t.z - xi[2 * e + 1] * t.w;
        pi[2 * e + 1] = xr[2 * e + 1] * t.w + xi[2 * e + 1] * t.z;
    }
    float4* wr = reinterpret_cast<float4*>(pr_s + lpad(int(t0)));
    float4* wi = reinterpret_cast<float4*>(pi_s + lpad(int(t0)));
    wr[0] = make_float4(pr[0], pr[1], pr[2], pr[3]); wr[1] = make_float4(pr[4], pr[5], pr[6], pr[7]);
    wi[0] = make_float4(pi[0], pi[1], pi[2], pi[3]); wi[1] = make_float4(pi[4], pi[5], pi[6], pi[7]);
}

__global__ __launch_bounds__(LOCAL_T) void acq_local_despread_kernel(const void* __restrict__ samples, int fmt,
                                                                     const uint64_t* __restrict__ starts, uint32_t R,
                                                                     const cf* __restrict__ tables, const int8_t* __restrict__ code_samples,
                                                                     const RefineSat* __restrict__ cands, uint32_t N, uint32_t R_u,
                                                                     uint32_t L, uint32_t p2_log, cf* __restrict__ z) {
    __shared__ __attribute__((aligned(16))) float pr_s[LOCAL_PROD_WORDS];
    __shared__ __attribute__((aligned(16))) float pi_s[LOCAL_PROD_WORDS];
    __shared__ float r_s[LOCAL_CHIP_WORDS];
    __shared__ cf acc_s[LOCAL_ACC_WORDS];
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x, cand = blockIdx.y, W = 2 * L + 1;
    const RefineSat w = cands[cand];
    // the period's start, a 64-bit element offset, uniform over the workgroup (as acq_despread_kernel reads it)
    uint64_t s = starts ? starts[size_t(w.bin) * R + w.offset + i] : uint64_t(w.offset + i) * N;
    s = uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s))) | (uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s >> 32))) << 32);
    const uint32_t cp = __builtin_amdgcn_readfirstlane(w.code_phase);
    const cf* tab = tables + size_t(w.bin) * N;
    const int8_t* rep = code_samples + size_t(w.worker) * N;
    const int bps = fmt == GM_FMT_C32 ? 8 : (fmt == GM_FMT_I8_IQ ? 2 : 1);
    const char* sp = static_cast<const char*>(samples) + s * uint64_t(bps);
    const bool aligned = (reinterpret_cast<uintptr_t>(sp) & (fmt == GM_FMT_I8_REAL ? 7u : 15u)) == 0;

    // the lane's slice and lags
    const uint32_t P2 = 1u << p2_log, nsl = uint32_t(LOCAL_T) >> p2_log, seg = uint32_t(LOCAL_TILE) >> (8 - p2_log);
    const uint32_t slice = uint32_t(tid) >> p2_log, ls = uint32_t(tid) & (P2 - 1);
    const uint32_t nj = (W + P2 - 1) >> p2_log;                 // lags per lane, uniform: 1 .. 3
    int roff[LOCAL_LB];                                         // chip of sample t at lag l: r[t + 2L - l]
#pragma unroll
    for (int j = 0; j < LOCAL_LB; ++j) {
        const uint32_t l = ls + uint32_t(j) * P2;
        roff[j] = int(2 * L) - int(l < W ? l : W - 1);          // (a lane past the last lag repeats it; its sums are not stored)
    }
    float ar[LOCAL_LB] = {0.0f, 0.0f, 0.0f}, ai[LOCAL_LB] = {0.0f, 0.0f, 0.0f};
    // chip q of a tile from n0: c[(n0 - cp - L + q) mod N], q < tl + 2L
    const uint32_t shift = (cp + L) % N;                        // (cp < N, L < N)

    for (uint32_t n0 = 0; n0 < N; n0 += LOCAL_TILE) {
        const uint32_t tl = N - n0 < uint32_t(LOCAL_TILE) ? N - n0 : uint32_t(LOCAL_TILE);
        if (fmt == GM_FMT_C32) {
            if (aligned) stage_products<GM_FMT_C32, true>(sp, tab, n0, tl, tid, pr_s, pi_s);
            else stage_products<GM_FMT_C32, false>(sp, tab, n0, tl, tid, pr_s, pi_s);
        } else if (fmt == GM_FMT_I8_IQ) {
            if (aligned) stage_products<GM_FMT_I8_IQ, true>(sp, tab, n0, tl, tid, pr_s, pi_s);
            else stage_products<GM_FMT_I8_IQ, false>(sp, tab, n0, tl, tid, pr_s, pi_s);
        } else {
            if (aligned) stage_products<GM_FMT_I8_REAL, true>(sp, tab, n0, tl, tid, pr_s, pi_s);
            else stage_products<GM_FMT_I8_REAL, false>(sp, tab, n0, tl, tid, pr_s, pi_s);
        }
        const uint32_t base = (n0 % N + N - shift) % N, nq = tl + 2 * L;       // base < N, q < N + 2L < 2N
        for (uint32_t q = uint32_t(tid); q < nq; q += LOCAL_T) {
            uint32_t m = base + q;
            if (m >= N) m -= N;
            if (m >= N) m -= N;
            r_s[lpad(int(q))] = float(rep[m]);
        }
        __syncthreads();
        const uint32_t tb = slice * seg, te = tb + seg < tl ? tb + seg : tl;
        for (uint32_t t = tb; t < te; ++t) {
            const float a = pr_s[lpad(int(t))], b = pi_s[lpad(int(t))];
#pragma unroll
            for (int j = 0; j < LOCAL_LB; ++j)
                if (uint32_t(j) < nj) {
                    const float c = r_s[lpad(int(t) + roff[j])];               // +-1: the products are exact
                    ar[j] += a * c;
                    ai[j] += b * c;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < LOCAL_LB; ++j) {
        const uint32_t l = ls + uint32_t(j) * P2;
        if (l < W) acc_s[slice * W + l] = cf_make(ar[j], ai[j]);
    }
    __syncthreads();
    if (uint32_t(tid) < W) {
        float re = acc_s[tid].x, im = acc_s[tid].y;
        for (uint32_t v = 1; v < nsl; ++v) { re += acc_s[v * W + tid].x; im += acc_s[v * W + tid].y; }
        z[(size_t(cand) * W + tid) * R_u + i] = cf_make(re, im);
    }
}

// the prompts and period times of a (lag, candidate) sit in LDS where R_u <= LOCAL_STAGE_MAX (16 KiB); longer dwells read them from
// global memory (every lane reads the same word)
constexpr uint32_t LOCAL_STAGE_MAX = 1024;

__global__ __launch_bounds__(LOCAL_T) void acq_local_scan_kernel(const cf* __restrict__ z, const double* __restrict__ t,
                                                                 const double* __restrict__ fc, const double* __restrict__ step,
                                                                 uint32_t neg, uint32_t J, uint32_t G, uint32_t Z, float n2,
                                                                 float* __restrict__ surface, float* __restrict__ row_val,
                                                                 uint32_t* __restrict__ row_idx, double* __restrict__ row_sum) {
    const int tid = threadIdx.x;
    const uint32_t W = gridDim.x, l = blockIdx.x, cand = blockIdx.y, R_u = G * J;
    const size_t row = size_t(cand) * W + l;
    const cf* zp = z + row * R_u;
    const double* tp = t + size_t(cand) * R_u;
    __shared__ cf z_s[LOCAL_STAGE_MAX];
    __shared__ double t_s[LOCAL_STAGE_MAX];
    const bool staged = R_u <= LOCAL_STAGE_MAX;
    if (staged) {
        for (uint32_t i = tid; i < R_u; i += LOCAL_T) { z_s[i] = zp[i]; t_s[i] = tp[i]; }
        __syncthreads();
    }
    const double f0 = fc[cand], st = step[cand];
    const int half = int(Z >> 1);
    float bv = -1.0f;
    uint32_t bi = 0xFFFFFFFFu;
    double sum = 0.0;
    for (uint32_t j = tid; j < Z; j += LOCAL_T) {
        const double f = f0 + double(int(j) - half) * st;
        float tot = 0.0f;
        uint32_t idx = 0;
        for (uint32_t g = 0; g < G; ++g) {
            float are = 0.0f, aim = 0.0f;
            for (uint32_t k = 0; k < J; ++k, ++idx) {
                const double tk = staged ? t_s[idx] : tp[idx];
                const cf v = staged ? z_s[idx] : zp[idx];
                // acq_refine_scan_kernel's arithmetic: the cycles in f64, reduced to one cycle before the angle
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
        surface[row * Z + j] = S;
        sum += double(S);
        take_better(bv, bi, S, j);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(bv, off, 64);
        const uint32_t oi = __shfl_down(bi, off, 64);
        take_better(bv, bi, ov, oi);
        sum += __shfl_down(sum, off, 64);
    }
    __shared__ float rv[LOCAL_T / 64];
    __shared__ uint32_t ri[LOCAL_T / 64];
    __shared__ double rs[LOCAL_T / 64];
    if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; rs[tid >> 6] = sum; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < LOCAL_T / 64; ++v) { take_better(bv, bi, rv[v], ri[v]); sum += rs[v]; }
        row_val[row] = bv;
        row_idx[row] = bi;
        row_sum[row] = sum;
    }
}

// one lane per candidate: the W row maxima in ascending l (a later row wins only when strictly larger: the first maximum in (l, j)
// order), the peak's neighbours along j and along l, and the sum of the rows at least `guard` lags (circular, mod N) from the peak
__global__ void acq_local_pick_kernel(const float* __restrict__ surface, const float* __restrict__ row_val,
                                      const uint32_t* __restrict__ row_idx, const double* __restrict__ row_sum, uint32_t n_cands,
                                      uint32_t W, uint32_t Z, uint32_t N, uint32_t guard, LocalPick* __restrict__ picks) {
    const uint32_t cand = blockIdx.x * blockDim.x + threadIdx.x;
    if (cand >= n_cands) return;
    const size_t r0 = size_t(cand) * W;
    float bv = -1.0f;
    uint32_t bl = 0xFFFFFFFFu, bj = 0;
    for (uint32_t l = 0; l < W; ++l) {
        const uint32_t j = row_idx[r0 + l];
        const float v = row_val[r0 + l];
        if (j < Z && v > bv) { bv = v; bl = l; bj = j; }
    }
    if (bl >= W) { bl = W >> 1; bj = Z >> 1; }                 // (no comparable value at all, e.g. samples that are not numbers: the centre)
    const float* sp = surface + (r0 + bl) * Z;
    LocalPick p;
    p.l = bl; p.j = bj;
    p.s0 = sp[bj];
    p.s_jm = bj > 0 ? sp[bj - 1] : 0.0f;
    p.s_jp = bj + 1 < Z ? sp[bj + 1] : 0.0f;
    p.s_lm = bl > 0 ? surface[(r0 + bl - 1) * Z + bj] : 0.0f;
    p.s_lp = bl + 1 < W ? surface[(r0 + bl + 1) * Z + bj] : 0.0f;
    p.s_c = sp[Z >> 1];
    double fsum = 0.0;
    uint32_t nf = 0;
    for (uint32_t l = 0; l < W; ++l) {
        const uint32_t dl = l > bl ? l - bl : bl - l, dc = dl < N - dl ? dl : N - dl;
        if (dc >= guard) { fsum += row_sum[r0 + l]; ++nf; }
    }
    p.floor_sum = fsum;
    p.n_floor = nf;
    picks[cand] = p;
}

}  // namespace

void launch_local(hipStream_t st, const LocalArgs& a) {
    const uint32_t W = 2 * a.L + 1;
    uint32_t p2_log = 3;
    while ((1u << p2_log) < W && p2_log < 6) ++p2_log;
    hipLaunchKernelGGL(acq_local_despread_kernel, dim3(a.R_u, a.n_cands), dim3(LOCAL_T), 0, st, a.samples, a.fmt, a.starts, a.R, a.tables,
                       a.code_samples, a.cands, a.N, a.R_u, a.L, p2_log, a.z);
    const float n2 = float(double(a.N) * double(a.N));
    hipLaunchKernelGGL(acq_local_scan_kernel, dim3(W, a.n_cands), dim3(LOCAL_T), 0, st, a.z, a.t, a.fc, a.step, a.neg, a.J, a.G, a.Z, n2,
                       a.surface, a.row_val, a.row_idx, a.row_sum);
    hipLaunchKernelGGL(acq_local_pick_kernel, dim3((a.n_cands + 63) / 64), dim3(64), 0, st, a.surface, a.row_val, a.row_idx, a.row_sum,
                       a.n_cands, W, a.Z, a.N, a.guard, a.picks);
}

}  // namespace gm
