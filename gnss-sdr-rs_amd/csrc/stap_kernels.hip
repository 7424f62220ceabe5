// stap_kernels.hip — per-block space-time adaptive nulling of an antenna array (gm_stap; gnss_mi355x.h states the definition): A antennas
// interleaved time sample by time sample in one stream, L taps in time on every antenna, one c32 stream out, the M = A L weights of a
// block from the Gram matrix of the block's stacked samples z[t][l A + a] = x_a[t - l].
//
// stap_kernel<A, NL>: one 256-lane workgroup per finished block of B time samples; NL = lags a wave carries (1: L <= 4, 2: L <= 8).
//   Staging: the block goes through LDS in chunks of 256 time samples plus the L - 1 in front of them, converted to f32, one row per
//     antenna (s_x[a][i]: consecutive lanes read consecutive 8-byte words).  Both passes read their samples from there.
//   Pass 1 (adaptive mode): entry ((l, a), (l + k, b)) of the Gram matrix is the lag-k sum of x_a[u] conj(x_b[u - k]) over u in
//     [bB - l, (b+1)B - l).  Wave v carries the lags k = v and v + 4 (those below L), all A x A pairs of each, over the INTERIOR
//     u in [bB, (b+1)B - L + 1) that every entry shares: lane j of the wave owns u = j, j + 64, j + 128, ... ascending, in registers,
//     four fmaf a pair and sample.  After every group of 1024 time samples (and at the block's end) the wave's 64 lane sums are added by
//     shuffles, S[j] += S[j + d] for d = 32, 16, 8, 4, 2, 1, and lane 0 adds the group's sum to the lag sum C[k][a][b] in LDS.
//   Assembly: every entry p <= q starts from its lag sum and adds its own L - 1 edge terms, the l head terms u = bB - l .. bB - 1 and
//     the L - 1 - l tail terms u = (b+1)B - L + 1 .. (b+1)B - l - 1, u ascending; the mirror entry is its conjugate, the diagonal's
//     imaginary part +0.  A fixed function of the block-relative position: no floating-point atomics.
//   Solve: in LDS, f64, from the f32 words of R.  Left-looking Cholesky, one column a barrier, lane i row i; row M is s^H, so that it
//     comes out as z^H = (L^-1 s)^H.  Every lane forms the pivot itself from row j (the same arithmetic, the same word), so the
//     fallback verdict is uniform.  Then d = z^H z, u = L^-H z column by column from the last, w = u / d rounded once.
//   Pass 2: lane i of a chunk forms y of time sample i from the staged rows, l ascending, a ascending, one fmaf per real product, w as
//     LDS broadcasts; consecutive lanes store consecutive 8-byte words.
// stap_state_kernel: the converted elements of the L - 1 samples in front of the unfinished block and of that block, from the old history
//   (a call that finishes no block) or from this call's input, into the OTHER history buffer.
// The staging, pass 1, the assembly and the factorisation are stap_core.h's, which beam_kernels.hip (gm_beamformer) includes too.
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf / __builtin_fma.
#include "stap_core.h"

namespace gm {
namespace {
template <int A, int NL>
__global__ __launch_bounds__(ST_LANES) void stap_kernel(StapArgs a) {
    __shared__ float2 s_x[A][ST_ROW];                            // the staged chunk: s_x[ant][i] = time sample chunk start - H + i
    __shared__ float2 s_edge[A][ST_EDGE];                        // [0, H): the H samples before the block; [H, 3H): its last 2H
    __shared__ float2 s_C[NL * 4][A][A];                         // the lag sums over the interior
    __shared__ float2 s_R[ST_M_MAX * ST_M_MAX];                  // the Gram matrix, f32 words, [M][M]
    __shared__ double s_Lr[ST_M_MAX + 1][ST_M_MAX], s_Li[ST_M_MAX + 1][ST_M_MAX];   // the Cholesky factor; row M: z^H
    __shared__ double s_inv[ST_M_MAX], s_ur[ST_M_MAX], s_ui[ST_M_MAX];
    __shared__ float2 s_w[ST_M_MAX];

    const int tid = threadIdx.x;
    const int B = int(a.B), L = int(a.L), H = L - 1, M = A * L;
    const int n_chunks = B / ST_CHUNK;
    const uint64_t old = (uint64_t(H) + a.pending) * A;          // elements of the span that lie in the history
    const uint64_t e0 = uint64_t(blockIdx.x) * uint64_t(B) * A;  // the span element of time sample (block start - H), antenna 0

    if (a.adaptive) {
        st_gram<A, NL>(a, s_x, s_edge, s_C, s_R, e0, old);

        // the weights, f64 from the f32 words; row M of the factor is s^H
        bool bad = st_factor(M, M + 1, a.loading, s_R, s_Lr, s_Li, s_inv, [&](int, int j) { return a.s[j]; });
        const int row = tid;
        double dd = 0.0;                                         // z^H z: s^H Rl^-1 s, real by construction
        for (int j = 0; j < M; ++j) { const double zr = s_Lr[M][j], zi = s_Li[M][j]; dd += zr * zr + zi * zi; }
        double rr = 0.0, ri = 0.0;                               // u = L^-H z, from the last column
        if (row < M) { rr = s_Lr[M][row]; ri = -s_Li[M][row]; }
        for (int k = M - 1; k >= 0; --k) {
            if (row == k) { s_ur[k] = rr * s_inv[k]; s_ui[k] = ri * s_inv[k]; }
            __syncthreads();
            if (row < k) {                                       // - conj(L[k][row]) u[k]
                const double lr = s_Lr[k][row], li = s_Li[k][row], ur = s_ur[k], ui = s_ui[k];
                rr -= lr * ur + li * ui;
                ri -= lr * ui - li * ur;
            }
        }
        if (!(dd > 0.0) || !(dd <= 1.7976931348623157e308)) bad = true;
        if (row < M) {
            float2 w;
            if (bad) {                                           // w = s / (s^H s)
                double ss = 0.0;
                for (int p = 0; p < M; ++p) ss += double(a.s[p].x) * double(a.s[p].x) + double(a.s[p].y) * double(a.s[p].y);
                w.x = float(double(a.s[row].x) / ss); w.y = float(double(a.s[row].y) / ss);
            } else {
                w.x = float(s_ur[row] / dd); w.y = float(s_ui[row] / dd);
            }
            s_w[row] = w;
        }
        if (bad && tid == 0) atomicAdd(a.fallbacks, 1ull);
    } else if (tid < M) {
        s_w[tid].x = a.w[tid].x; s_w[tid].y = a.w[tid].y;
    }
    __syncthreads();

    if (a.cap_w && tid < M) reinterpret_cast<float2*>(a.cap_w)[uint64_t(blockIdx.x) * M + tid] = s_w[tid];
    if (a.adaptive && a.cap_R)
        for (int e = tid; e < M * M; e += ST_LANES) reinterpret_cast<float2*>(a.cap_R)[uint64_t(blockIdx.x) * (M * M) + e] = s_R[e];

    for (int c = 0; c < n_chunks; ++c) {
        if (!(c == 0 && n_chunks == 1 && a.adaptive)) {          // a block of one chunk is still staged from pass 1
            __syncthreads();
            st_stage<A>(a, s_x, e0, old, c);
            __syncthreads();
        }
        float2 y; y.x = 0.0f; y.y = 0.0f;
        for (int l = 0; l < L; ++l) {
#pragma unroll
            for (int k = 0; k < A; ++k) {                        // conj(w) x = (wr xr + wi xi) + j (wr xi - wi xr)
                const float2 w = s_w[l * A + k], x = s_x[k][tid + H - l];
                y.x = __builtin_fmaf(w.x, x.x, y.x);
                y.x = __builtin_fmaf(w.y, x.y, y.x);
                y.y = __builtin_fmaf(w.x, x.y, y.y);
                y.y = __builtin_fmaf(-w.y, x.x, y.y);
            }
        }
        reinterpret_cast<float2*>(a.out)[uint64_t(blockIdx.x) * uint64_t(B) + uint64_t(c) * ST_CHUNK + tid] = y;
    }
}

__global__ __launch_bounds__(ST_LANES) void stap_state_kernel(StapArgs a) {
    const uint64_t H = a.L - 1;
    const uint64_t n = (H + a.pending_out) * a.A;                // elements of the new history
    const uint64_t e = uint64_t(blockIdx.x) * ST_LANES + threadIdx.x;
    if (e >= n) return;
    const float2 v = st_element(a, a.n_blocks * uint64_t(a.B) * a.A + e, (H + a.pending) * a.A);
    a.hist_out[e] = cf_make(v.x, v.y);
}

template <int A>
void launch_blocks(hipStream_t s, const StapArgs& a) {
    const unsigned g = unsigned(a.n_blocks);
    if (a.L <= 4) stap_kernel<A, 1><<<g, ST_LANES, 0, s>>>(a);
    else if constexpr (A <= 6) stap_kernel<A, 2><<<g, ST_LANES, 0, s>>>(a);         // A L <= 32: more than four taps only at A <= 6
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, A in 2 .. 8, L in 1 .. 8, A L <= 32, B a multiple of 256 (the caller has checked); n_in > 0
void launch_stap(hipStream_t s, const StapArgs& a) {
    if (a.n_blocks) {
        switch (a.A) {
            case 2: launch_blocks<2>(s, a); break;
            case 3: launch_blocks<3>(s, a); break;
            case 4: launch_blocks<4>(s, a); break;
            case 5: launch_blocks<5>(s, a); break;
            case 6: launch_blocks<6>(s, a); break;
            case 7: launch_blocks<7>(s, a); break;
            default: launch_blocks<8>(s, a); break;
        }
    }
    launch_stap_state(s, a);
}

// the state kernel alone (gm_beamformer's call ends with it too); reads in, fmt, hist_in, hist_out, A, L, B, pending, pending_out, n_blocks
void launch_stap_state(hipStream_t s, const StapArgs& a) {
    const uint64_t n = (uint64_t(a.L) - 1 + a.pending_out) * a.A;
    if (n) stap_state_kernel<<<unsigned((n + ST_LANES - 1) / ST_LANES), ST_LANES, 0, s>>>(a);
}

}  // namespace gm
