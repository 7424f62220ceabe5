// lcmv_kernels.hip — several constraints on one beam of an antenna array (gm_lcmv; gnss_mi355x.h states the definition): gm_beamformer's
// input, blocks, history and Gram matrix, where beam p carries Q_p constraint rows c_q of M = A L words and Q_p responses f_q in place of
// one row, and its weights answer C^H w = f at the least output power: w = Rl^-1 C (C^H Rl^-1 C)^-1 f.  The staging, pass 1, the assembly
// of R and the factorisation are stap_core.h's, the same code stap_kernel and beam_kernel run, so R's words are theirs bit for bit.
//
// lcmv_kernel<A, NL>: one 256-lane workgroup per finished block of B time samples; NL = lags a wave carries (1: L <= 4, 2: L <= 8).  P and
//   the Q_p are run-time values: twelve instantiations, as for beam_kernel.
//   The rows of all beams (q_sum <= 16, beam p's from row q0[p]) go into s_w first (the weights replace them once the factor stands).
//   Pass 1, assembly: st_gram.  ONE matrix.
//   Factor: st_factor with q_sum rows below the matrix, a lane a row: row M + q comes out as z_q^H = (Lc^-1 c_q)^H.  ONE factor.
//   R goes to the capture here: its LDS words then hold the small Gram matrices (s_G), so that the kernel stays under 64 KB.
//   Per beam, lane (slot, row) = (tid / 32, tid % 32), beam p = 8 r + slot in round r (two rounds at P > 8), all f64:
//     G[q][r] = z_q^H z_r (the lower triangle, two entries a lane, the index ascending within each sum);
//     G = Lg Lg^H left-looking, a lane a row, one column a barrier, the row f^H riding below it so that it comes out as y^H = (Lg^-1 f)^H
//       (lane Q; its words live in s_v); every lane forms the pivot itself, so the beam's verdict is uniform over its lanes;
//     v = Lg^-H y column by column from the last;  t = sum_q z_q v_q, q ascending, a lane a row of t;
//     u = Lc^-H t column by column from the last, as in beam_kernel;  w_p = u rounded once, into s_w[p].
//   Fallback: tr = 0 or a bad pivot of Lc (uniform over the workgroup) sends every beam to its quiescent weights w0_p (device memory,
//     the host's f64), a bad pivot of Lg or a word of u that does not round to a finite f32 beam p alone; the lane of row 0 of a beam
//     that fell back adds one to the beam's counter (integer atomic).
//   Pass 2: beam_kernel's — per staged chunk lane i owns time sample i; beams in groups of four, x read from LDS once per (l, a) and
//     group, w as LDS broadcasts; l ascending, then a, one fmaf per real product.
// Loops over the columns of G run to q_max, the largest Q_p of the call, with the beam's own Q_p as a predicate: a barrier count that is
//   uniform, and words that depend on the beam's own rows alone.
// LDS beside beam_kernel's: v (1 KB), 1 / Lg[j][j] (0.5 KB), the responses and the verdicts (0.2 KB): 63.2 KB at (8, 1).
// The state kernel is gm_stap's (launch_stap_state).
// Compiled with -ffp-contract=off: every fused operation is written as __builtin_fmaf / __builtin_fma.
#include "stap_core.h"

namespace gm {
namespace {
constexpr int LC_SLOTS = ST_LANES / ST_M_MAX;                    // beams a round carries
static_assert(LC_SLOTS * LC_Q_MAX * LC_Q_MAX * 2 * sizeof(double) <= ST_M_MAX * ST_M_MAX * sizeof(float2), "s_G lies over s_R");
static_assert(LC_Q_MAX < ST_M_MAX && LC_Q_MAX * LC_Q_MAX == 2 * ST_M_MAX, "a lane a row of G and f^H, two entries of G a lane");

__device__ __forceinline__ bool lc_bad(double v) { return !(v > 0.0) || !(v <= 1.7976931348623157e308); }
__device__ __forceinline__ bool lc_finite(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }

template <int A, int NL>
__global__ __launch_bounds__(ST_LANES) void lcmv_kernel(LcmvArgs a) {
    __shared__ float2 s_x[A][ST_ROW];                            // the staged chunk: s_x[ant][i] = time sample chunk start - H + i
    __shared__ float2 s_edge[A][ST_EDGE];                        // [0, H): the H samples before the block; [H, 3H): its last 2H
    __shared__ float2 s_C[NL * 4][A][A];                         // the lag sums over the interior
    __shared__ float2 s_R[ST_M_MAX * ST_M_MAX];                  // the Gram matrix, f32 words, [M][M]; after the factor: s_G
    __shared__ double s_Lr[ST_M_MAX + LC_Q_SUM][ST_M_MAX], s_Li[ST_M_MAX + LC_Q_SUM][ST_M_MAX];   // the factor; row M + q: z_q^H
    __shared__ double s_inv[ST_M_MAX], s_ur[LC_SLOTS][ST_M_MAX], s_ui[LC_SLOTS][ST_M_MAX];
    __shared__ double s_vr[LC_SLOTS][LC_Q_MAX], s_vi[LC_SLOTS][LC_Q_MAX], s_ginv[LC_SLOTS][LC_Q_MAX];
    __shared__ float2 s_w[BM_P_MAX][ST_M_MAX];                   // the constraint rows until the factor stands, then the weights
    __shared__ float2 s_f[LC_Q_SUM];                             // the responses
    __shared__ int s_bad[LC_SLOTS];                              // a word of u of the slot's beam does not round to a finite f32

    const int tid = threadIdx.x;
    const int B = int(a.B), L = int(a.L), H = L - 1, M = A * L, P = int(a.P);
    const int n_chunks = B / ST_CHUNK;
    const uint64_t old = (uint64_t(H) + a.pending) * A;          // elements of the span that lie in the history
    const uint64_t e0 = uint64_t(blockIdx.x) * uint64_t(B) * A;  // the span element of time sample (block start - H), antenna 0

    if (a.adaptive) {
        const int QS = int(a.q_sum), QM = int(a.q_max);
        for (int e = tid; e < QS * M; e += ST_LANES) { const cf c = a.c[e]; s_w[e / M][e % M] = make_float2(c.x, c.y); }
        if (tid < QS) { const cf f = a.f[tid]; s_f[tid] = make_float2(f.x, f.y); }
        st_gram<A, NL>(a, s_x, s_edge, s_C, s_R, e0, old);       // (its barriers stand between the rows' stores and their readers)

        const bool bad_block = st_factor(M, M + QS, a.loading, s_R, s_Lr, s_Li, s_inv, [&](int q, int j) { return s_w[q][j]; });
        if (a.cap_R)
            for (int e = tid; e < M * M; e += ST_LANES) reinterpret_cast<float2*>(a.cap_R)[uint64_t(blockIdx.x) * (M * M) + e] = s_R[e];
        __syncthreads();                                         // R has been read: its words are s_G from here
        const int slot = tid / ST_M_MAX, row = tid % ST_M_MAX;
        double (*s_Gr)[LC_Q_MAX] = reinterpret_cast<double (*)[LC_Q_MAX]>(s_R) + slot * 2 * LC_Q_MAX;      // [q][r] of the slot's beam
        double (*s_Gi)[LC_Q_MAX] = s_Gr + LC_Q_MAX;
        for (int p0 = 0; p0 < P; p0 += LC_SLOTS) {
            const int p = p0 + slot;
            const int Q = p < P ? int(a.nq[p]) : 0;              // a slot with no beam: no lane of it does anything but the barriers
            const int zrow = M + (p < P ? int(a.q0[p]) : 0);     // row zrow + q of the factor: z_q^H
            const bool live = Q > 0 && row < M;
            if (row == 0) s_bad[slot] = 0;

            // G[q][r] = z_q^H z_r, q >= r: sum_j a_q[j] conj(a_r[j]) with a_q = row zrow + q of the factor
            for (int e = row; e < LC_Q_MAX * LC_Q_MAX; e += ST_M_MAX) {
                const int q = e / LC_Q_MAX, r = e % LC_Q_MAX;
                if (q < Q && r <= q) {
                    double gr = 0.0, gi = 0.0;
                    for (int j = 0; j < M; ++j) {
                        const double qr = s_Lr[zrow + q][j], qi = s_Li[zrow + q][j], rr = s_Lr[zrow + r][j], ri = s_Li[zrow + r][j];
                        gr += qr * rr + qi * ri;
                        gi += qi * rr - qr * ri;
                    }
                    s_Gr[q][r] = gr; s_Gi[q][r] = q == r ? 0.0 : gi;
                }
            }
            __syncthreads();

            // G = Lg Lg^H in place below the diagonal (the diagonal keeps G's words, 1 / Lg[j][j] goes to s_ginv); lane Q: the row f^H
            bool bad_beam = false;
            for (int j = 0; j < QM; ++j) {
                if (j < Q) {
                    double pj = s_Gr[j][j];
                    double xr = 0.0, xi = 0.0;
                    if (row > j && row < Q) { xr = s_Gr[row][j]; xi = s_Gi[row][j]; }
                    else if (row == Q) { const float2 f = s_f[zrow - M + j]; xr = double(f.x); xi = -double(f.y); }
                    for (int k = 0; k < j; ++k) {
                        const double jr = s_Gr[j][k], ji = s_Gi[j][k];
                        pj = __builtin_fma(-jr, jr, pj);
                        pj = __builtin_fma(-ji, ji, pj);
                        if (row > j && row <= Q) {               // - Lg[row][k] conj(Lg[j][k])
                            const double ir = row < Q ? s_Gr[row][k] : s_vr[slot][k], ii = row < Q ? s_Gi[row][k] : s_vi[slot][k];
                            xr -= ir * jr + ii * ji;
                            xi -= ii * jr - ir * ji;
                        }
                    }
                    if (lc_bad(pj)) bad_beam = true;
                    const double inv = 1.0 / sqrt(pj);
                    if (row == j) s_ginv[slot][j] = inv;
                    else if (row > j && row < Q) { s_Gr[row][j] = xr * inv; s_Gi[row][j] = xi * inv; }
                    else if (row == Q) { s_vr[slot][j] = xr * inv; s_vi[slot][j] = xi * inv; }       // conj(y[j])
                }
                __syncthreads();
            }

            // v = Lg^-H y, from the last column; lane `row` < Q carries v[row]
            double rr = 0.0, ri = 0.0;
            if (row < Q) { rr = s_vr[slot][row]; ri = -s_vi[slot][row]; }
            __syncthreads();                                     // y has been read: its words are v from here
            for (int k = QM - 1; k >= 0; --k) {
                if (k < Q && row == k) { s_vr[slot][k] = rr * s_ginv[slot][k]; s_vi[slot][k] = ri * s_ginv[slot][k]; }
                __syncthreads();
                if (k < Q && row < k) {                          // - conj(Lg[k][row]) v[k]
                    const double lr = s_Gr[k][row], li = s_Gi[k][row], vr = s_vr[slot][k], vi = s_vi[slot][k];
                    rr -= lr * vr + li * vi;
                    ri -= lr * vi - li * vr;
                }
            }

            // t = sum_q z_q v_q (z_q[row] = conj of the factor's word), then u = Lc^-H t from the last column
            rr = 0.0; ri = 0.0;
            if (live)
                for (int q = 0; q < Q; ++q) {
                    const double zr = s_Lr[zrow + q][row], zi = -s_Li[zrow + q][row], vr = s_vr[slot][q], vi = s_vi[slot][q];
                    rr += zr * vr - zi * vi;
                    ri += zr * vi + zi * vr;
                }
            double ur = 0.0, ui = 0.0;
            for (int k = M - 1; k >= 0; --k) {
                if (live && row == k) { ur = rr * s_inv[k]; ui = ri * s_inv[k]; s_ur[slot][k] = ur; s_ui[slot][k] = ui; }
                __syncthreads();
                if (live && row < k) {                           // - conj(Lc[k][row]) u[k]
                    const double lr = s_Lr[k][row], li = s_Li[k][row], kr = s_ur[slot][k], ki = s_ui[slot][k];
                    rr -= lr * kr + li * ki;
                    ri -= lr * ki - li * kr;
                }
            }
            if (live && !(lc_finite(float(ur)) && lc_finite(float(ui)))) s_bad[slot] = 1;   // the word as it would be stored
            __syncthreads();
            const bool bad = bad_block || bad_beam || s_bad[slot] != 0;
            if (live) {
                float2 w;
                if (bad) { const cf q = a.w0[p * M + row]; w.x = q.x; w.y = q.y; }
                else { w.x = float(ur); w.y = float(ui); }
                s_w[p][row] = w;
                if (bad && row == 0) atomicAdd(a.fallbacks + p, 1ull);
            }
            __syncthreads();                                     // the round's words have been read
        }
    } else {
        for (int e = tid; e < P * M; e += ST_LANES) { const cf w = a.w[e]; s_w[e / M][e % M] = make_float2(w.x, w.y); }
    }
    __syncthreads();

    if (a.cap_w)
        for (int e = tid; e < P * M; e += ST_LANES) reinterpret_cast<float2*>(a.cap_w)[uint64_t(blockIdx.x) * (P * M) + e] = s_w[e / M][e % M];

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
void launch_blocks(hipStream_t s, const LcmvArgs& a) {
    const unsigned g = unsigned(a.n_blocks);
    if (a.L <= 4) lcmv_kernel<A, 1><<<g, ST_LANES, 0, s>>>(a);
    else if constexpr (A <= 6) lcmv_kernel<A, 2><<<g, ST_LANES, 0, s>>>(a);         // A L <= 32: more than four taps only at A <= 6
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, A in 2 .. 8, L in 1 .. 8, A L <= 32, P in 1 .. 16, nq[p] in 1 .. 8 and <= A L, q0[p] the sum of the nq
// before p, q_sum <= 16, q_max the largest, B a multiple of 256, out_stride >= n_blocks B (the caller has checked); n_in > 0
void launch_lcmv(hipStream_t s, const LcmvArgs& a) {
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
