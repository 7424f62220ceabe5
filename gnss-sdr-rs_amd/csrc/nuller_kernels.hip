// nuller_kernels.hip — per-block adaptive spatial nulling of an antenna array (gm_nuller; gnss_mi355x.h states the definition): A
// antennas interleaved time sample by time sample in one stream, one c32 stream out, the weights of a block from the block's own
// covariance.
//
// nuller_kernel<A, FMT>: one 256-lane workgroup per finished block of B time samples.
//   Pass 1 (adaptive mode): lane l owns the time samples t = l, l + 256, ... of the block, ascending.  A time sample is A contiguous
//     elements, read with the widest load its size and the pointer allow (16 bytes for an even A of c32 and for A = 8 of int8), from
//     the history in front of the call's input where the block began in an earlier call.  The A (A + 1) / 2 sums of the upper triangle
//     live in registers: per time sample and entry (i <= j) re = fmaf(xi.re, xj.re, re), re = fmaf(xi.im, xj.im, re) and, off the
//     diagonal, im = fmaf(xi.im, xj.re, im), im = fmaf(-xi.re, xj.im, im), from +0.
//   Reduction: within a wave S[l] += S[l + d] for d = 32, 16, 8, 4, 2, 1 (shuffles), then (W0 + W1) + (W2 + W3) of the four waves'
//     sums through LDS.  A fixed tree of f32 adds: a function of the block-relative t alone, no floating-point atomics.
//   Solve: wave 0, every lane the same arithmetic in f64 from the f32 words of R: tr, the loaded matrix, its Cholesky factor L (row by
//     row, a reciprocal of each diagonal word), z = L^-1 s, d = z^H z (= s^H Rl^-1 s, real by construction), u = L^-H z, w = u / d, each
//     component rounded once to f32.  Every loop is unrolled on the template A: no register array is indexed by a run-time value.  Lane
//     0 leaves w (and, for a capture, R) in LDS.
//   Pass 2: every lane re-reads its time samples (from L2), forms y = sum_a conj(w[a]) x_a with one fmaf per real product, a ascending,
//     from +0, and stores it: consecutive lanes store consecutive 8-byte words.
//   An output's arithmetic is one fixed function of its block's samples, whatever call, cut or workgroup the block falls into.
// nuller_state_kernel<FMT>: the converted elements of the unfinished block, from the old history (a call that finishes no block) or
//   from this call's input, into the OTHER history buffer.
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf.
#include "gm_internal.h"

namespace gm {
namespace {
constexpr int NL_LANES = 256;

template <int A>
__device__ __forceinline__ void nl_load_c32(const cf* p, bool wide, float2 (&x)[A]) {
    if ((A % 2 == 0) && wide) {
        const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int k = 0; k < A / 2; ++k) {
            const float4 t = q[k];
            x[2 * k].x = t.x; x[2 * k].y = t.y; x[2 * k + 1].x = t.z; x[2 * k + 1].y = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < A; ++k) { const cf t = p[k]; x[k].x = t.x; x[k].y = t.y; }
    }
}

template <int A>
__device__ __forceinline__ void nl_load_i8(const char2* p, bool wide, float2 (&x)[A]) {
    constexpr int BYTES = 2 * A;
    constexpr int W = BYTES % 16 == 0 ? 16 : BYTES % 8 == 0 ? 8 : BYTES % 4 == 0 ? 4 : 2;
    char2 c[A];
    if (W > 2 && wide) __builtin_memcpy(c, __builtin_assume_aligned(p, W), BYTES);
    else {
#pragma unroll
        for (int k = 0; k < A; ++k) c[k] = p[k];
    }
#pragma unroll
    for (int k = 0; k < A; ++k) { x[k].x = float(c[k].x); x[k].y = float(c[k].y); }
}

// time sample v of the call's span: the history for v < pending, else the call's input
template <int A, int FMT>
__device__ __forceinline__ void nl_sample(const NullerArgs& a, uint64_t v, float2 (&x)[A]) {
    if (v < uint64_t(a.pending)) nl_load_c32<A>(a.hist_in + v * A, A % 2 == 0, x);
    else {
        const uint64_t u = v - uint64_t(a.pending);             // < n_in: the host counts only blocks whose samples all exist
        if (FMT == GM_FMT_C32) nl_load_c32<A>(reinterpret_cast<const cf*>(a.in) + u * A, a.in_wide != 0, x);
        else nl_load_i8<A>(reinterpret_cast<const char2*>(a.in) + u * A, a.in_wide != 0, x);
    }
}

__device__ __forceinline__ float nl_wave_sum(float v) {
    for (int d = 32; d; d >>= 1) v = v + __shfl_down(v, d, 64);
    return v;                                                    // lane 0 of the wave holds the tree's root
}

// w from the f32 words of R (upper triangle: re[idx], im[idx], idx running over i <= j row by row), in f64
template <int A>
__device__ __forceinline__ void nl_solve(const float (&re)[A * (A + 1) / 2], const float (&im)[A * (A + 1) / 2], const NullerArgs& a,
                                         float2 (&w)[A]) {
    double sr[A], si[A];
#pragma unroll
    for (int i = 0; i < A; ++i) { sr[i] = double(a.s[i].x); si[i] = double(a.s[i].y); }
    double mr[A][A], mi[A][A];                                   // the lower triangle of Rl, then of L
    double tr = 0.0;
    {
        int idx = 0;
#pragma unroll
        for (int i = 0; i < A; ++i) {
#pragma unroll
            for (int j = i; j < A; ++j) {
                mr[j][i] = double(re[idx]);
                mi[j][i] = i == j ? 0.0 : -double(im[idx]);      // Rl[j][i] = conj(R[i][j])
                if (i == j) tr += double(re[idx]);
                ++idx;
            }
        }
    }
    if (tr == 0.0) {                                             // an all-zero block: w = s / (s^H s)
        double d = 0.0;
#pragma unroll
        for (int i = 0; i < A; ++i) d += sr[i] * sr[i] + si[i] * si[i];
#pragma unroll
        for (int i = 0; i < A; ++i) { w[i].x = float(sr[i] / d); w[i].y = float(si[i] / d); }
        return;
    }
    const double load = double(a.loading) * (tr / double(A));
    double inv[A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double xr = mr[i][j] + (i == j ? load : 0.0), xi = mi[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {                        // - L[i][k] conj(L[j][k])
                xr -= mr[i][k] * mr[j][k] + mi[i][k] * mi[j][k];
                xi -= mi[i][k] * mr[j][k] - mr[i][k] * mi[j][k];
            }
            if (i == j) {
                const double d = sqrt(xr);
                mr[i][i] = d; mi[i][i] = 0.0; inv[i] = 1.0 / d;
            } else {
                mr[i][j] = xr * inv[j]; mi[i][j] = xi * inv[j];
            }
        }
    }
    double zr[A], zi[A], d = 0.0;
#pragma unroll
    for (int i = 0; i < A; ++i) {                                // z = L^-1 s
        double xr = sr[i], xi = si[i];
#pragma unroll
        for (int k = 0; k < i; ++k) {
            xr -= mr[i][k] * zr[k] - mi[i][k] * zi[k];
            xi -= mr[i][k] * zi[k] + mi[i][k] * zr[k];
        }
        zr[i] = xr * inv[i]; zi[i] = xi * inv[i];
        d += zr[i] * zr[i] + zi[i] * zi[i];
    }
    double ur[A], ui[A];
#pragma unroll
    for (int i = A - 1; i >= 0; --i) {                           // u = L^-H z
        double xr = zr[i], xi = zi[i];
#pragma unroll
        for (int k = i + 1; k < A; ++k) {                        // - conj(L[k][i]) u[k]
            xr -= mr[k][i] * ur[k] + mi[k][i] * ui[k];
            xi -= mr[k][i] * ui[k] - mi[k][i] * ur[k];
        }
        ur[i] = xr * inv[i]; ui[i] = xi * inv[i];
    }
#pragma unroll
    for (int i = 0; i < A; ++i) { w[i].x = float(ur[i] / d); w[i].y = float(ui[i] / d); }
}

template <int A, int FMT>
__global__ __launch_bounds__(NL_LANES) void nuller_kernel(NullerArgs a) {
    constexpr int T = A * (A + 1) / 2;
    __shared__ float s_part[4][2 * T];
    __shared__ float2 s_R[A * A];
    __shared__ float2 s_w[A];
    const int tid = threadIdx.x;
    const int B = int(a.B);
    const uint64_t v0 = uint64_t(blockIdx.x) * uint64_t(B);     // the block's first time sample in the call's span

    if (a.adaptive) {
        float re[T], im[T];
#pragma unroll
        for (int k = 0; k < T; ++k) { re[k] = 0.0f; im[k] = 0.0f; }
        for (int t = tid; t < B; t += NL_LANES) {
            float2 x[A];
            nl_sample<A, FMT>(a, v0 + uint64_t(t), x);
            int idx = 0;
#pragma unroll
            for (int i = 0; i < A; ++i) {
#pragma unroll
                for (int j = i; j < A; ++j) {
                    re[idx] = __builtin_fmaf(x[i].x, x[j].x, re[idx]);
                    re[idx] = __builtin_fmaf(x[i].y, x[j].y, re[idx]);
                    if (j > i) {
                        im[idx] = __builtin_fmaf(x[i].y, x[j].x, im[idx]);
                        im[idx] = __builtin_fmaf(-x[i].x, x[j].y, im[idx]);
                    }
                    ++idx;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const float r = nl_wave_sum(re[k]), i = nl_wave_sum(im[k]);
            if ((tid & 63) == 0) { s_part[tid >> 6][2 * k] = r; s_part[tid >> 6][2 * k + 1] = i; }
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                re[k] = (s_part[0][2 * k] + s_part[1][2 * k]) + (s_part[2][2 * k] + s_part[3][2 * k]);
                im[k] = (s_part[0][2 * k + 1] + s_part[1][2 * k + 1]) + (s_part[2][2 * k + 1] + s_part[3][2 * k + 1]);
            }
            float2 w[A];
            nl_solve<A>(re, im, a, w);
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < A; ++i) s_w[i] = w[i];
                int idx = 0;
#pragma unroll
                for (int i = 0; i < A; ++i) {
#pragma unroll
                    for (int j = i; j < A; ++j) {
                        float2 r; r.x = re[idx]; r.y = i == j ? 0.0f : im[idx];
                        s_R[i * A + j] = r;
                        if (j > i) { r.y = -r.y; s_R[j * A + i] = r; }
                        ++idx;
                    }
                }
            }
        }
    } else if (tid == 0) {
#pragma unroll
        for (int i = 0; i < A; ++i) { s_w[i].x = a.w[i].x; s_w[i].y = a.w[i].y; }
    }
    __syncthreads();

    if (a.cap_w && tid < A) reinterpret_cast<float2*>(a.cap_w)[uint64_t(blockIdx.x) * A + tid] = s_w[tid];
    if (a.adaptive && a.cap_R && tid < A * A) reinterpret_cast<float2*>(a.cap_R)[uint64_t(blockIdx.x) * (A * A) + tid] = s_R[tid];

    float2 w[A];
#pragma unroll
    for (int i = 0; i < A; ++i) w[i] = s_w[i];
    for (int t = tid; t < B; t += NL_LANES) {
        float2 x[A];
        nl_sample<A, FMT>(a, v0 + uint64_t(t), x);
        float2 y; y.x = 0.0f; y.y = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {                            // conj(w) x = (wr xr + wi xi) + j (wr xi - wi xr)
            y.x = __builtin_fmaf(w[i].x, x[i].x, y.x);
            y.x = __builtin_fmaf(w[i].y, x[i].y, y.x);
            y.y = __builtin_fmaf(w[i].x, x[i].y, y.y);
            y.y = __builtin_fmaf(-w[i].y, x[i].x, y.y);
        }
        reinterpret_cast<float2*>(a.out)[v0 + uint64_t(t)] = y;
    }
}

template <int FMT>
__global__ __launch_bounds__(NL_LANES) void nuller_state_kernel(NullerArgs a) {
    const uint64_t n = uint64_t(a.pending_out) * a.A;            // elements of the new history
    const uint64_t e = uint64_t(blockIdx.x) * NL_LANES + threadIdx.x;
    if (e >= n) return;
    const uint64_t k = a.n_blocks * uint64_t(a.B) * a.A + e;     // the same element in the call's span
    const uint64_t old = uint64_t(a.pending) * a.A;
    cf v;
    if (k < old) v = a.hist_in[k];                               // only where the call finishes no block
    else if (FMT == GM_FMT_C32) v = reinterpret_cast<const cf*>(a.in)[k - old];
    else {
        const char2 c = reinterpret_cast<const char2*>(a.in)[k - old];
        v = cf_make(float(c.x), float(c.y));
    }
    a.hist_out[e] = v;
}

template <int FMT>
void launch_blocks(hipStream_t s, const NullerArgs& a) {
    const unsigned g = unsigned(a.n_blocks);
    switch (a.A) {
        case 2: nuller_kernel<2, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        case 3: nuller_kernel<3, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        case 4: nuller_kernel<4, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        case 5: nuller_kernel<5, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        case 6: nuller_kernel<6, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        case 7: nuller_kernel<7, FMT><<<g, NL_LANES, 0, s>>>(a); break;
        default: nuller_kernel<8, FMT><<<g, NL_LANES, 0, s>>>(a); break;
    }
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, A in 2 .. 8, B a multiple of 256 (the caller has checked); n_in > 0
void launch_nuller(hipStream_t s, const NullerArgs& a, int fmt) {
    if (a.n_blocks) {
        if (fmt == GM_FMT_C32) launch_blocks<GM_FMT_C32>(s, a);
        else launch_blocks<GM_FMT_I8_IQ>(s, a);
    }
    const uint64_t n = uint64_t(a.pending_out) * a.A;
    if (n) {
        const unsigned g = unsigned((n + NL_LANES - 1) / NL_LANES);
        if (fmt == GM_FMT_C32) nuller_state_kernel<GM_FMT_C32><<<g, NL_LANES, 0, s>>>(a);
        else nuller_state_kernel<GM_FMT_I8_IQ><<<g, NL_LANES, 0, s>>>(a);
    }
}

}  // namespace gm
