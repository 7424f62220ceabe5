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
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf / __builtin_fma.
#include "gm_internal.h"

namespace gm {
namespace {
constexpr int ST_LANES = 256;
constexpr int ST_CHUNK = 256;                                    // time samples staged at once
constexpr int ST_GROUP = 1024;                                   // time samples between two reductions of the lane sums
constexpr int ST_ROW = ST_CHUNK + ST_L_MAX - 1;                  // words of one antenna's staged row

__device__ __forceinline__ float st_wave_sum(float v) {
    for (int d = 32; d; d >>= 1) v = v + __shfl_down(v, d, 64);
    return v;                                                    // lane 0 of the wave holds the tree's root
}

// element e (= time sample * A + antenna) of the call's span: the history for the first (H + pending) time samples, else the call's input
__device__ __forceinline__ float2 st_element(const StapArgs& a, uint64_t e, uint64_t old) {
    float2 r;
    if (e < old) { const cf t = a.hist_in[e]; r.x = t.x; r.y = t.y; }
    else if (a.fmt == GM_FMT_C32) { const cf t = reinterpret_cast<const cf*>(a.in)[e - old]; r.x = t.x; r.y = t.y; }
    else { const char2 c = reinterpret_cast<const char2*>(a.in)[e - old]; r.x = float(c.x); r.y = float(c.y); }
    return r;
}

template <int A, int NL>
__global__ __launch_bounds__(ST_LANES) void stap_kernel(StapArgs a) {
    __shared__ float2 s_x[A][ST_ROW];                            // the staged chunk: s_x[ant][i] = time sample chunk start - H + i
    __shared__ float2 s_edge[A][3 * (ST_L_MAX - 1)];             // [0, H): the H samples before the block; [H, 3H): its last 2H
    __shared__ float2 s_C[NL * 4][A][A];                         // the lag sums over the interior
    __shared__ float2 s_R[ST_M_MAX * ST_M_MAX];                  // the Gram matrix, f32 words, [M][M]
    __shared__ double s_Lr[ST_M_MAX + 1][ST_M_MAX], s_Li[ST_M_MAX + 1][ST_M_MAX];   // the Cholesky factor; row M: z^H
    __shared__ double s_inv[ST_M_MAX], s_ur[ST_M_MAX], s_ui[ST_M_MAX];
    __shared__ float2 s_w[ST_M_MAX];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = int(a.B), L = int(a.L), H = L - 1, M = A * L;
    const int n_chunks = B / ST_CHUNK;
    const uint64_t old = (uint64_t(H) + a.pending) * A;          // elements of the span that lie in the history
    const uint64_t e0 = uint64_t(blockIdx.x) * uint64_t(B) * A;  // the span element of time sample (block start - H), antenna 0

    // chunk c into LDS (every lane; the caller puts the barriers around it)
    auto stage = [&](int c) {
        const uint64_t base = e0 + uint64_t(c) * ST_CHUNK * A;
        const int n = (ST_CHUNK + H) * A;
        for (int e = tid; e < n; e += ST_LANES) s_x[e % A][e / A] = st_element(a, base + uint64_t(e), old);
    };

    if (a.adaptive) {
        for (int e = tid; e < NL * 4 * A * A; e += ST_LANES) (&s_C[0][0][0])[e] = make_float2(0.0f, 0.0f);
        float re[NL][A][A], im[NL][A][A];
#pragma unroll
        for (int n = 0; n < NL; ++n)
#pragma unroll
            for (int i = 0; i < A; ++i)
#pragma unroll
                for (int j = 0; j < A; ++j) { re[n][i][j] = 0.0f; im[n][i][j] = 0.0f; }

        for (int c = 0; c < n_chunks; ++c) {
            __syncthreads();                                     // the chunk before has been read
            stage(c);
            __syncthreads();
            if (c == 0)
                for (int e = tid; e < H * A; e += ST_LANES) s_edge[e % A][e / A] = s_x[e % A][e / A];
            if (c == n_chunks - 1)
                for (int e = tid; e < 2 * H * A; e += ST_LANES) s_edge[e % A][H + e / A] = s_x[e % A][ST_CHUNK + H - 2 * H + e / A];
            if (wave < L) {
                const int end = B - H - c * ST_CHUNK;            // interior samples of this chunk: local i < end
                for (int i = lane; i < ST_CHUNK && i < end; i += 64) {
                    float2 x[A];
#pragma unroll
                    for (int k = 0; k < A; ++k) x[k] = s_x[k][i + H];
#pragma unroll
                    for (int n = 0; n < NL; ++n) {
                        const int lag = wave + 4 * n;
                        if (lag < L) {
                            float2 z[A];
#pragma unroll
                            for (int k = 0; k < A; ++k) z[k] = s_x[k][i + H - lag];
#pragma unroll
                            for (int p = 0; p < A; ++p) {
#pragma unroll
                                for (int q = 0; q < A; ++q) {
                                    re[n][p][q] = __builtin_fmaf(x[p].x, z[q].x, re[n][p][q]);
                                    re[n][p][q] = __builtin_fmaf(x[p].y, z[q].y, re[n][p][q]);
                                    im[n][p][q] = __builtin_fmaf(x[p].y, z[q].x, im[n][p][q]);
                                    im[n][p][q] = __builtin_fmaf(-x[p].x, z[q].y, im[n][p][q]);
                                }
                            }
                        }
                    }
                }
                if ((c + 1) % (ST_GROUP / ST_CHUNK) == 0 || c == n_chunks - 1) {     // the group's lane sums into the lag sums
#pragma unroll
                    for (int n = 0; n < NL; ++n) {
                        const int lag = wave + 4 * n;
                        if (lag < L) {
#pragma unroll
                            for (int p = 0; p < A; ++p) {
#pragma unroll
                                for (int q = 0; q < A; ++q) {
                                    const float r = st_wave_sum(re[n][p][q]), i = st_wave_sum(im[n][p][q]);
                                    if (lane == 0) { float2 t = s_C[lag][p][q]; t.x = t.x + r; t.y = t.y + i; s_C[lag][p][q] = t; }
                                    re[n][p][q] = 0.0f; im[n][p][q] = 0.0f;
                                }
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();

        // the Gram matrix: the lag sum plus the entry's own edge terms
        for (int e = tid; e < M * M; e += ST_LANES) {
            const int p = e / M, q = e % M;
            if (p > q) continue;
            const int l = p / A, ant = p % A, k = q / A - l, bnt = q % A;
            float2 r = s_C[k][ant][bnt];
            for (int t = 0; t < H; ++t) {
                // head terms u = -l .. -1 (s_edge word u + H), then tail terms u = B - H .. B - l - 1 (s_edge word H + u - (B - 2H))
                const int iu = t < l ? H - l + t : 2 * H + (t - l);
                const float2 xa = s_edge[ant][iu], xb = s_edge[bnt][iu - k];
                r.x = __builtin_fmaf(xa.x, xb.x, r.x);
                r.x = __builtin_fmaf(xa.y, xb.y, r.x);
                r.y = __builtin_fmaf(xa.y, xb.x, r.y);
                r.y = __builtin_fmaf(-xa.x, xb.y, r.y);
            }
            if (p == q) r.y = 0.0f;
            s_R[p * M + q] = r;
            if (p != q) { r.y = -r.y; s_R[q * M + p] = r; }
        }
        __syncthreads();

        // the weights, f64 from the f32 words
        double tr = 0.0;
        for (int p = 0; p < M; ++p) tr += double(s_R[p * M + p].x);
        const double load = double(a.loading) * (tr / double(M));
        bool bad = tr == 0.0;
        const int row = tid;                                     // rows 0 .. M - 1 of Rl, row M = s^H
        for (int j = 0; j < M; ++j) {
            double pj = double(s_R[j * M + j].x) + load;
            double xr = 0.0, xi = 0.0;
            if (row >= j && row <= M) {
                if (row < M) { xr = double(s_R[row * M + j].x) + (row == j ? load : 0.0); xi = row == j ? 0.0 : double(s_R[row * M + j].y); }
                else { xr = double(a.s[j].x); xi = -double(a.s[j].y); }
            }
            for (int k = 0; k < j; ++k) {
                const double jr = s_Lr[j][k], ji = s_Li[j][k];
                pj = __builtin_fma(-jr, jr, pj);
                pj = __builtin_fma(-ji, ji, pj);
                if (row > j && row <= M) {                       // - L[row][k] conj(L[j][k])
                    const double ir = s_Lr[row][k], ii = s_Li[row][k];
                    xr -= ir * jr + ii * ji;
                    xi -= ii * jr - ir * ji;
                }
            }
            if (!(pj > 0.0) || !(pj <= 1.7976931348623157e308)) bad = true;
            const double d = sqrt(pj), inv = 1.0 / d;
            if (row == j) { s_Lr[j][j] = d; s_Li[j][j] = 0.0; s_inv[j] = inv; }
            else if (row > j && row <= M) { s_Lr[row][j] = xr * inv; s_Li[row][j] = xi * inv; }
            __syncthreads();
        }
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
            stage(c);
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
    const uint64_t n = (uint64_t(a.L) - 1 + a.pending_out) * a.A;
    if (n) stap_state_kernel<<<unsigned((n + ST_LANES - 1) / ST_LANES), ST_LANES, 0, s>>>(a);
}

}  // namespace gm
