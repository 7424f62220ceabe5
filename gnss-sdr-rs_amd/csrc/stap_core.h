// stap_core.h — what stap_kernel (stap_kernels.hip, gm_stap) and beam_kernel (beam_kernels.hip, gm_beamformer) share, so that a beam's
// words are a gm_stap's by construction: the staging of a chunk, pass 1 and the assembly of the Gram matrix, and the left-looking
// Cholesky factorisation with the constraint rows riding below the matrix.  stap_kernels.hip describes each step.  `Args` is StapArgs or
// BeamArgs: the fields read here (in, fmt, hist_in, B, L, pending, loading) mean the same in both.
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf / __builtin_fma.
#pragma once
#include "gm_internal.h"

namespace gm {
namespace {
constexpr int ST_LANES = 256;
constexpr int ST_CHUNK = 256;                                    // time samples staged at once
constexpr int ST_GROUP = 1024;                                   // time samples between two reductions of the lane sums
constexpr int ST_ROW = ST_CHUNK + ST_L_MAX - 1;                  // words of one antenna's staged row
constexpr int ST_EDGE = 3 * (ST_L_MAX - 1);                      // words of one antenna's edge row

__device__ __forceinline__ float st_wave_sum(float v) {
    for (int d = 32; d; d >>= 1) v = v + __shfl_down(v, d, 64);
    return v;                                                    // lane 0 of the wave holds the tree's root
}

// element e (= time sample * A + antenna) of the call's span: the history for the first (H + pending) time samples, else the call's input
template <class Args>
__device__ __forceinline__ float2 st_element(const Args& a, uint64_t e, uint64_t old) {
    float2 r;
    if (e < old) { const cf t = a.hist_in[e]; r.x = t.x; r.y = t.y; }
    else if (a.fmt == GM_FMT_C32) { const cf t = reinterpret_cast<const cf*>(a.in)[e - old]; r.x = t.x; r.y = t.y; }
    else { const char2 c = reinterpret_cast<const char2*>(a.in)[e - old]; r.x = float(c.x); r.y = float(c.y); }
    return r;
}

// chunk c of the workgroup's block into LDS (every lane; the caller puts the barriers around it): s_x[ant][i] = time sample
// chunk start - H + i.  e0: the span element of time sample (block start - H), antenna 0; old: elements of the span in the history
template <int A, class Args>
__device__ __forceinline__ void st_stage(const Args& a, float2 (*s_x)[ST_ROW], uint64_t e0, uint64_t old, int c) {
    const int tid = threadIdx.x, H = int(a.L) - 1;
    const uint64_t base = e0 + uint64_t(c) * ST_CHUNK * A;
    const int n = (ST_CHUNK + H) * A;
    for (int e = tid; e < n; e += ST_LANES) s_x[e % A][e / A] = st_element(a, base + uint64_t(e), old);
}

// Pass 1 and the assembly: the f32 words of the block's Gram matrix into s_R[M][M], behind a barrier.  Leaves the block's last chunk
// staged in s_x.  s_edge: [0, H) the H samples before the block, [H, 3H) its last 2H; s_C: the lag sums over the interior.
template <int A, int NL, class Args>
__device__ __forceinline__ void st_gram(const Args& a, float2 (*s_x)[ST_ROW], float2 (*s_edge)[ST_EDGE], float2 (*s_C)[A][A], float2* s_R,
                                        uint64_t e0, uint64_t old) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = int(a.B), L = int(a.L), H = L - 1, M = A * L;
    const int n_chunks = B / ST_CHUNK;

    for (int e = tid; e < NL * 4 * A * A; e += ST_LANES) (&s_C[0][0][0])[e] = make_float2(0.0f, 0.0f);
    float re[NL][A][A], im[NL][A][A];
#pragma unroll
    for (int n = 0; n < NL; ++n)
#pragma unroll
        for (int i = 0; i < A; ++i)
#pragma unroll
            for (int j = 0; j < A; ++j) { re[n][i][j] = 0.0f; im[n][i][j] = 0.0f; }

    for (int c = 0; c < n_chunks; ++c) {
        __syncthreads();                                         // the chunk before has been read
        st_stage<A>(a, s_x, e0, old, c);
        __syncthreads();
        if (c == 0)
            for (int e = tid; e < H * A; e += ST_LANES) s_edge[e % A][e / A] = s_x[e % A][e / A];
        if (c == n_chunks - 1)
            for (int e = tid; e < 2 * H * A; e += ST_LANES) s_edge[e % A][H + e / A] = s_x[e % A][ST_CHUNK + H - 2 * H + e / A];
        if (wave < L) {
            const int end = B - H - c * ST_CHUNK;                // interior samples of this chunk: local i < end
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
}

// The factorisation, f64 from the f32 words of R: left-looking Cholesky of the loaded matrix, one column a barrier, lane i row i.  Rows
// M .. rows - 1 are the constraint rows s_p^H (s_at(p, j) = word j of s_p), so that row M + p comes out as z_p^H = (L^-1 s_p)^H.  Every
// lane forms the pivot itself from row j (the same arithmetic, the same word), so the verdict returned (tr = 0 or a bad pivot) is
// uniform.  s_inv[j] = 1 / L[j][j].  Ends behind a barrier.
template <class S>
__device__ __forceinline__ bool st_factor(int M, int rows, float loading, const float2* s_R, double (*s_Lr)[ST_M_MAX], double (*s_Li)[ST_M_MAX],
                                          double* s_inv, S&& s_at) {
    double tr = 0.0;
    for (int p = 0; p < M; ++p) tr += double(s_R[p * M + p].x);
    const double load = double(loading) * (tr / double(M));
    bool bad = tr == 0.0;
    const int row = threadIdx.x;
    for (int j = 0; j < M; ++j) {
        double pj = double(s_R[j * M + j].x) + load;
        double xr = 0.0, xi = 0.0;
        if (row >= j && row < rows) {
            if (row < M) { xr = double(s_R[row * M + j].x) + (row == j ? load : 0.0); xi = row == j ? 0.0 : double(s_R[row * M + j].y); }
            else { const auto s = s_at(row - M, j); xr = double(s.x); xi = -double(s.y); }
        }
        for (int k = 0; k < j; ++k) {
            const double jr = s_Lr[j][k], ji = s_Li[j][k];
            pj = __builtin_fma(-jr, jr, pj);
            pj = __builtin_fma(-ji, ji, pj);
            if (row > j && row < rows) {                         // - L[row][k] conj(L[j][k])
                const double ir = s_Lr[row][k], ii = s_Li[row][k];
                xr -= ir * jr + ii * ji;
                xi -= ii * jr - ir * ji;
            }
        }
        if (!(pj > 0.0) || !(pj <= 1.7976931348623157e308)) bad = true;
        const double d = sqrt(pj), inv = 1.0 / d;
        if (row == j) { s_Lr[j][j] = d; s_Li[j][j] = 0.0; s_inv[j] = inv; }
        else if (row > j && row < rows) { s_Lr[row][j] = xr * inv; s_Li[row][j] = xi * inv; }
        __syncthreads();
    }
    return bad;
}
}  // namespace
}  // namespace gm
