// beam_kernels.hip — one beam per constraint row from ONE Gram matrix of an antenna array's block (gm_beamformer; gnss_mi355x.h states
// the definition): gm_stap's input, blocks, history and arithmetic, P constraint rows s_p of M = A L words, P output planes.  Beam p's
// words are those of a gm_stap with steering = s_p, word for word: the staging, pass 1, the assembly of R and the factorisation are
// stap_core.h's, the same code stap_kernel runs, and what is restated here (the substitution, the fallback, pass 2's sums) keeps
// stap_kernel's operations in stap_kernel's order.
//
// beam_kernel<A, NL>: one 256-lane workgroup per finished block of B time samples; NL = lags a wave carries (1: L <= 4, 2: L <= 8).  P is
//   a run-time value: twelve instantiations, as for stap_kernel.
//   The rows s_p go into s_w first (the weights replace them beam by beam once the factor stands).
//   Pass 1, assembly: st_gram.  ONE matrix.
//   Factor: st_factor with P constraint rows below the matrix, a lane a row: row M + p comes out as z_p^H = (L^-1 s_p)^H.  ONE factor.
//   Substitution: lane (slot, row) = (tid / 32, tid % 32) carries row `row` of beam p = 8 r + slot in round r (two rounds at P = 16):
//     d_p = z_p^H z_p, u_p = L^-H z_p column by column from the last, w_p = u_p / d_p rounded once, into s_w[p].
//   Fallback: tr = 0 or a bad pivot (uniform over the workgroup) sends every beam to s_p / (s_p^H s_p), a bad d_p beam p alone; the lane
//     of row 0 of a beam that fell back adds one to the beam's counter (integer atomic).  The fallback reads s_p from device memory.
//   Pass 2: per staged chunk lane i owns time sample i; beams in groups of four, four y accumulators in registers, x read from LDS once
//     per (l, a) and group, w as LDS broadcasts; consecutive lanes store consecutive 8-byte words of plane p.
// LDS at the largest shapes: the staged chunk (16.8 KB at A = 8), the edges (1.3 KB), the lag sums (2 KB), R (8 KB), the factor with 16
//   rows below it in f64 twice (24 KB), reciprocals (0.25 KB), u of one round of eight beams (4 KB), s / w (4 KB): 61.4 KB at (8, 1),
//   under the 64 KB of a static allocation.  One workgroup a CU there.
// The state kernel is gm_stap's (launch_stap_state).
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf / __builtin_fma.
#include "stap_core.h"

namespace gm {
namespace {
constexpr int BM_SLOTS = ST_LANES / ST_M_MAX;                    // beams a substitution round carries

template <int A, int NL>
__global__ __launch_bounds__(ST_LANES) void beam_kernel(BeamArgs a) {
    __shared__ float2 s_x[A][ST_ROW];                            // the staged chunk: s_x[ant][i] = time sample chunk start - H + i
    __shared__ float2 s_edge[A][ST_EDGE];                        // [0, H): the H samples before the block; [H, 3H): its last 2H
    __shared__ float2 s_C[NL * 4][A][A];                         // the lag sums over the interior
    __shared__ float2 s_R[ST_M_MAX * ST_M_MAX];                  // the Gram matrix, f32 words, [M][M]
    __shared__ double s_Lr[ST_M_MAX + BM_P_MAX][ST_M_MAX], s_Li[ST_M_MAX + BM_P_MAX][ST_M_MAX];   // the factor; row M + p: z_p^H
    __shared__ double s_inv[ST_M_MAX], s_ur[BM_SLOTS][ST_M_MAX], s_ui[BM_SLOTS][ST_M_MAX];
    __shared__ float2 s_w[BM_P_MAX][ST_M_MAX];                   // the rows s_p until the factor stands, then the weights

    const int tid = threadIdx.x;
    const int B = int(a.B), L = int(a.L), H = L - 1, M = A * L, P = int(a.P);
    const int n_chunks = B / ST_CHUNK;
    const uint64_t old = (uint64_t(H) + a.pending) * A;          // elements of the span that lie in the history
    const uint64_t e0 = uint64_t(blockIdx.x) * uint64_t(B) * A;  // the span element of time sample (block start - H), antenna 0

    if (a.adaptive) {
        for (int e = tid; e < P * M; e += ST_LANES) { const cf s = a.s[e]; s_w[e / M][e % M] = make_float2(s.x, s.y); }
        st_gram<A, NL>(a, s_x, s_edge, s_C, s_R, e0, old);       // (its barriers stand between the rows' stores and their readers)

        const bool bad_block = st_factor(M, M + P, a.loading, s_R, s_Lr, s_Li, s_inv, [&](int p, int j) { return s_w[p][j]; });
        const int slot = tid / ST_M_MAX, row = tid % ST_M_MAX;
        for (int p0 = 0; p0 < P; p0 += BM_SLOTS) {
            const int p = p0 + slot;
            const bool live = p < P && row < M;
            const int zrow = M + (p < P ? p : 0);
            double dd = 0.0;                                     // z_p^H z_p: s_p^H Rl^-1 s_p, real by construction
            for (int j = 0; j < M; ++j) { const double zr = s_Lr[zrow][j], zi = s_Li[zrow][j]; dd += zr * zr + zi * zi; }
            double rr = 0.0, ri = 0.0;                           // u_p = L^-H z_p, from the last column
            if (live) { rr = s_Lr[zrow][row]; ri = -s_Li[zrow][row]; }
            for (int k = M - 1; k >= 0; --k) {
                if (live && row == k) { s_ur[slot][k] = rr * s_inv[k]; s_ui[slot][k] = ri * s_inv[k]; }
                __syncthreads();
                if (live && row < k) {                           // - conj(L[k][row]) u[k]
                    const double lr = s_Lr[k][row], li = s_Li[k][row], ur = s_ur[slot][k], ui = s_ui[slot][k];
                    rr -= lr * ur + li * ui;
                    ri -= lr * ui - li * ur;
                }
            }
            const bool bad = bad_block || !(dd > 0.0) || !(dd <= 1.7976931348623157e308);
            if (live) {
                float2 w;
                if (bad) {                                       // w_p = s_p / (s_p^H s_p)
                    const cf* s = a.s + p * M;
                    double ss = 0.0;
                    for (int q = 0; q < M; ++q) ss += double(s[q].x) * double(s[q].x) + double(s[q].y) * double(s[q].y);
                    w.x = float(double(s[row].x) / ss); w.y = float(double(s[row].y) / ss);
                } else {
                    w.x = float(s_ur[slot][row] / dd); w.y = float(s_ui[slot][row] / dd);
                }
                s_w[p][row] = w;
                if (bad && row == 0) atomicAdd(a.fallbacks + p, 1ull);
            }
            __syncthreads();                                     // the round's u words have been read
        }
    } else {
        for (int e = tid; e < P * M; e += ST_LANES) { const cf w = a.w[e]; s_w[e / M][e % M] = make_float2(w.x, w.y); }
    }
    __syncthreads();

    if (a.cap_w)
        for (int e = tid; e < P * M; e += ST_LANES) reinterpret_cast<float2*>(a.cap_w)[uint64_t(blockIdx.x) * (P * M) + e] = s_w[e / M][e % M];
    if (a.adaptive && a.cap_R)
        for (int e = tid; e < M * M; e += ST_LANES) reinterpret_cast<float2*>(a.cap_R)[uint64_t(blockIdx.x) * (M * M) + e] = s_R[e];

    float2* out = reinterpret_cast<float2*>(a.out) + uint64_t(blockIdx.x) * uint64_t(B) + tid;
    for (int c = 0; c < n_chunks; ++c) {
        if (!(c == 0 && n_chunks == 1 && a.adaptive)) {          // a block of one chunk is still staged from pass 1
            __syncthreads();
            st_stage<A>(a, s_x, e0, old, c);
            __syncthreads();
        }
        for (int g = 0; g < P; g += 4) {                         // beams g .. g + 3 (those past P - 1 repeat beam P - 1 and are not stored)
            int wq[4];                                           // the beams' rows of s_w
            float2 y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { wq[q] = g + q < P ? g + q : P - 1; y[q].x = 0.0f; y[q].y = 0.0f; }
            for (int l = 0; l < L; ++l) {
#pragma unroll
                for (int k = 0; k < A; ++k) {                    // conj(w) x = (wr xr + wi xi) + j (wr xi - wi xr)
                    const float2 x = s_x[k][tid + H - l];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float2 w = s_w[wq[q]][l * A + k];
                        y[q].x = __builtin_fmaf(w.x, x.x, y[q].x);
                        y[q].x = __builtin_fmaf(w.y, x.y, y[q].x);
                        y[q].y = __builtin_fmaf(w.x, x.y, y[q].y);
                        y[q].y = __builtin_fmaf(-w.y, x.x, y[q].y);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g + q < P) out[uint64_t(g + q) * a.out_stride + uint64_t(c) * ST_CHUNK] = y[q];
        }
    }
}

template <int A>
void launch_blocks(hipStream_t s, const BeamArgs& a) {
    const unsigned g = unsigned(a.n_blocks);
    if (a.L <= 4) beam_kernel<A, 1><<<g, ST_LANES, 0, s>>>(a);
    else if constexpr (A <= 6) beam_kernel<A, 2><<<g, ST_LANES, 0, s>>>(a);         // A L <= 32: more than four taps only at A <= 6
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, A in 2 .. 8, L in 1 .. 8, A L <= 32, P in 1 .. 16, B a multiple of 256, out_stride >= n_blocks B (the
// caller has checked); n_in > 0
void launch_beam(hipStream_t s, const BeamArgs& a) {
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
    StapArgs st{};                                               // gm_stap's state kernel: the L - 1 samples and the unfinished block
    st.in = a.in; st.n_in = a.n_in; st.fmt = a.fmt;
    st.hist_in = a.hist_in; st.hist_out = a.hist_out;
    st.A = a.A; st.L = a.L; st.B = a.B;
    st.pending = a.pending; st.pending_out = a.pending_out; st.n_blocks = a.n_blocks;
    launch_stap_state(s, st);
}

}  // namespace gm
