// array_solve.hip — gm_array_rows_solve_dev: the nine steps of gm_array_row_solve (gnss_mi355x.h states them) for many rows at once on
// the device, f64, one 256-lane workgroup a row; and gm_beamformer_set_steering_dev's install kernel (gfx950, wave64;
// -ffp-contract=off: every operation below rounds once, as the host entry's does).
//
// A workgroup owns ONE row from its first load to its last store: no word travels between workgroups, nothing spins, there are no
// floating-point atomics, and every loop is bounded by an argument the host has checked (n_blocks, n, m) or by a constant (64 sweeps).
// Every branch around a barrier is taken by the whole workgroup: the statuses and the sweep's verdict are formed by every lane from the
// same LDS words with the same arithmetic.  THE INVARIANT that makes "the same words" true: an LDS word that lanes of several waves read
// to decide a branch is written only behind a barrier that all of those reads precede.  So each stage has a flag word of its own (s_bad_z,
// s_bad_R, both cleared before the first barrier), the sweep's partial sums s_red are rewritten only behind the barrier at the top of
// the next sweep, a barrier stands behind the sweep loop, and step 6 keeps s in words of its own (s_s).
//
// LDS, f64, re and im planes apart, rows AS_LD = 33 doubles apart (lanes that walk a column fall on different banks, as st_factor's
// s_Lr / s_Li do): image 0 holds Rs (upper triangle) and then C in place (lower triangle and diagonal: column j of the factorisation
// reads Rs[j][i], i > j, which no column writes), image 1 Q, image 2 first a batch of whitened vectors and then V.  3 x 2 x 32 x 33 x 8
// = 50688 bytes, whatever m.
//
//   z check  every word of the row's n vectors is read once (lanes stride the words of a vector): status 1
//   1        lanes own upper-triangle entries, blocks ascending, += double(word): status 2.  Rs is gm_array_row_solve's bit for bit
//   2        tr by every lane, p ascending: status 3
//   3        left-looking Cholesky as st_factor runs it (stap_core.h): a column a barrier, lane i row i, every lane forms the pivot
//            itself so the verdict is uniform: status 4.  The arithmetic is gm_array_row_solve's (a - (x y + u v), then / d), not
//            st_factor's fused one, so C is the host's bit for bit as well
//   4        batches of nb = min(256, stride) vectors: staged as doubles zt[k][v] (v fastest, rows `stride` = (1056 / m) made odd
//            apart), lane v substitutes its vector in place, then lanes own (p, q) entries of Q and add the batch's terms, i ascending.
//            Q is the host's bit for bit
//   5        parallel-order cyclic Jacobi: mp = m rounded up to even players, player mp - 1 fixed, step r pairs (r, mp - 1) and
//            ((r + k) mod (mp - 1), (r - k) mod (mp - 1)) for k = 1 .. mp / 2 - 1; a pair with a player >= m idles (odd m).  Lane k
//            forms its pair's (c, s e^{j phi}) by hermitian_jacobi's formulas from the current Q; behind a barrier the column
//            rotations of Q and V, behind another the row rotations of Q and the exact zeros; mp - 1 steps a sweep.  Before each sweep
//            lane p sums row p's energies, every lane adds the m partial sums in ascending p: stop below 1e-30 of the whole, or after
//            64 sweeps: status 5 where lambda1 is not positive
//   6 .. 9   the first wave: lane p forms s[p] = sum_{k <= p} C[p][k] V[k][i1], every lane of it scans the moduli in ascending p
//            (status 6), lane p rounds word p
// A row with a status gets zero words and a zero info but for the status; the other rows never see it.
#include "gm_internal.h"

namespace gm {
namespace {
constexpr int AS_LANES = 256;
constexpr int AS_LD = 33;                                    // doubles between two rows of an image
constexpr int AS_PLANE = ST_M_MAX * AS_LD;                   // doubles of one plane of an image

struct AsInfo { double lambda1, lambda2; uint32_t ref_index, status; };      // gm_array_row_info's 24 bytes
static_assert(sizeof(AsInfo) == sizeof(gm_array_row_info), "gm_array_row_info");

__device__ __forceinline__ bool as_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }
__device__ __forceinline__ bool as_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }

// X[:, p] <- c X[:, p] - conj(se) X[:, q];  X[:, q] <- se X[:, p] + c X[:, q], at row k (hermitian_jacobi's `cols`)
__device__ __forceinline__ void as_col_rot(double* Xr, double* Xi, int k, int p, int q, double c, double ser, double sei) {
    const double pr = Xr[k * AS_LD + p], pi = Xi[k * AS_LD + p], qr = Xr[k * AS_LD + q], qi = Xi[k * AS_LD + q];
    Xr[k * AS_LD + p] = c * pr - (ser * qr + sei * qi);
    Xi[k * AS_LD + p] = c * pi - (ser * qi - sei * qr);
    Xr[k * AS_LD + q] = ser * pr - sei * pi + c * qr;
    Xi[k * AS_LD + q] = ser * pi + sei * pr + c * qi;
}

__global__ __launch_bounds__(AS_LANES) void array_solve_kernel(const ArraySolveArgs a) {
    __shared__ double s_img[3][2][AS_PLANE];
    __shared__ double s_red[2][ST_M_MAX];                    // the sweep's row energies
    __shared__ double s_s[2][ST_M_MAX];                      // s = C v (its own words: no stage rewrites what another may still read)
    __shared__ double s_c[ST_M_MAX / 2], s_ser[ST_M_MAX / 2], s_sei[ST_M_MAX / 2];
    __shared__ int s_p[ST_M_MAX / 2], s_q[ST_M_MAX / 2];
    __shared__ int s_bad_z, s_bad_R;                         // a flag word a stage: a stage's writers never meet another stage's readers

    const int tid = threadIdx.x, m = int(a.m);
    const uint32_t row = blockIdx.x;
    double* const Cr = s_img[0][0]; double* const Ci = s_img[0][1];
    double* const Qr = s_img[1][0]; double* const Qi = s_img[1][1];
    double* const Vr = s_img[2][0]; double* const Vi = s_img[2][1];
    const cf* const z = a.z + uint64_t(row) * a.row_stride;
    int status = 0;
    double lambda1 = 0.0, lambda2 = 0.0;
    int i1 = 0;

    if (tid == 0) { s_bad_z = 0; s_bad_R = 0; }
    __syncthreads();

    // ---- the row's vectors are finite
    {
        bool bad = false;
        const uint64_t words = uint64_t(a.n) * uint64_t(m);
        for (uint64_t e = tid; e < words; e += AS_LANES) {
            const cf v = z[(e / m) * a.vec_stride + (e % m)];
            bad = bad || !as_finite(v.x) || !as_finite(v.y);
        }
        if (bad) s_bad_z = 1;                                // (every writer writes the same word)
        __syncthreads();
        if (s_bad_z) status = 1;
    }

    // ---- 1. Rs
    if (!status) {
        bool bad = false;
        for (int e = tid; e < m * m; e += AS_LANES) {
            const int p = e / m, q = e % m;
            double re = 0.0, im = 0.0;
            if (p <= q && a.R) {
                const cf* w = a.R + size_t(p) * m + q;
                for (uint32_t b = 0; b < a.n_blocks; ++b, w += size_t(m) * m) {
                    const cf v = *w;
                    bad = bad || !as_finite(v.x) || !as_finite(v.y);
                    re += double(v.x);
                    if (p != q) im += double(v.y);
                }
            } else if (p == q) {
                re = 1.0;
            }
            Cr[p * AS_LD + q] = re; Ci[p * AS_LD + q] = im;
        }
        if (bad) s_bad_R = 1;
        __syncthreads();
        if (s_bad_R) status = 2;
    }

    // ---- 2. the loading
    double dl = 0.0;
    if (!status) {
        double tr = 0.0;
        for (int p = 0; p < m; ++p) tr += Cr[p * AS_LD + p];
        if (!(tr > 0.0) || !as_finite(tr)) status = 3;
        dl = a.load * (tr / double(m));
    }

    // ---- 3. Cholesky in place: C[i][j], i >= j, over the lower triangle; Rl[i][j] = conj(Rs[j][i])
    if (!status) {
        for (int j = 0; j < m; ++j) {
            double pj = Cr[j * AS_LD + j] + dl;
            for (int k = 0; k < j; ++k) pj -= Cr[j * AS_LD + k] * Cr[j * AS_LD + k] + Ci[j * AS_LD + k] * Ci[j * AS_LD + k];
            if (!(pj > 0.0) || !as_finite(pj)) { status = 4; break; }        // (the same words in every lane: uniform)
            const double d = sqrt(pj);
            if (tid > j && tid < m) {
                double xr = Cr[j * AS_LD + tid], xi = -Ci[j * AS_LD + tid];
                for (int k = 0; k < j; ++k) {                // - C[i][k] conj(C[j][k])
                    const double ir = Cr[tid * AS_LD + k], ii = Ci[tid * AS_LD + k], jr = Cr[j * AS_LD + k], ji = Ci[j * AS_LD + k];
                    xr -= ir * jr + ii * ji;
                    xi -= ii * jr - ir * ji;
                }
                Cr[tid * AS_LD + j] = xr / d; Ci[tid * AS_LD + j] = xi / d;
            }
            __syncthreads();                                 // every lane has formed pivot j before its diagonal word changes
            if (tid == j) { Cr[j * AS_LD + j] = d; Ci[j * AS_LD + j] = 0.0; }
            __syncthreads();
        }
    }

    // ---- 4. zt_i = C^-1 z_i, Q = sum_i zt_i zt_i^H
    if (!status) {
        int stride = AS_PLANE / m;
        if (!(stride & 1)) --stride;
        const int nb = stride < AS_LANES ? stride : AS_LANES;
        double* const Tr = Vr; double* const Ti = Vi;        // zt[k][v] at k * stride + v
        for (int e = tid; e < m * m; e += AS_LANES) { Qr[(e / m) * AS_LD + e % m] = 0.0; Qi[(e / m) * AS_LD + e % m] = 0.0; }
        for (uint32_t i0 = 0; i0 < a.n; i0 += uint32_t(nb)) {
            const int cnt = a.n - i0 < uint32_t(nb) ? int(a.n - i0) : nb;
            __syncthreads();                                 // the batch before has been summed
            for (int e = tid; e < cnt * m; e += AS_LANES) {
                const int v = e / m, k = e % m;
                const cf w = z[uint64_t(i0 + uint32_t(v)) * a.vec_stride + uint32_t(k)];
                Tr[k * stride + v] = double(w.x); Ti[k * stride + v] = double(w.y);
            }
            __syncthreads();
            if (tid < cnt) {
                for (int p = 0; p < m; ++p) {
                    double xr = Tr[p * stride + tid], xi = Ti[p * stride + tid];
                    for (int k = 0; k < p; ++k) {
                        const double cr = Cr[p * AS_LD + k], ci = Ci[p * AS_LD + k], tr = Tr[k * stride + tid], ti = Ti[k * stride + tid];
                        xr -= cr * tr - ci * ti;
                        xi -= cr * ti + ci * tr;
                    }
                    const double d = Cr[p * AS_LD + p];
                    Tr[p * stride + tid] = xr / d; Ti[p * stride + tid] = xi / d;
                }
            }
            __syncthreads();
            for (int e = tid; e < m * m; e += AS_LANES) {
                const int p = e / m, q = e % m;
                double re = Qr[p * AS_LD + q], im = Qi[p * AS_LD + q];
                for (int v = 0; v < cnt; ++v) {              // zt[p] conj(zt[q])
                    const double pr = Tr[p * stride + v], pi = Ti[p * stride + v], qr = Tr[q * stride + v], qi = Ti[q * stride + v];
                    re += pr * qr + pi * qi;
                    im += pi * qr - pr * qi;
                }
                Qr[p * AS_LD + q] = re; Qi[p * AS_LD + q] = im;
            }
        }
        __syncthreads();
    }

    // ---- 5. the eigenproblem
    if (!status) {
        for (int e = tid; e < m * m; e += AS_LANES) { Vr[(e / m) * AS_LD + e % m] = e / m == e % m ? 1.0 : 0.0; Vi[(e / m) * AS_LD + e % m] = 0.0; }
        const int mp = (m + 1) & ~1, half = mp / 2, ring = mp - 1;
        for (int sweep = 0; sweep < 64; ++sweep) {
            __syncthreads();
            if (tid < m) {
                double off = 0.0, all = 0.0;
                for (int q = 0; q < m; ++q) {
                    const double e = Qr[tid * AS_LD + q] * Qr[tid * AS_LD + q] + Qi[tid * AS_LD + q] * Qi[tid * AS_LD + q];
                    all += e;
                    if (q != tid) off += e;
                }
                s_red[0][tid] = off; s_red[1][tid] = all;
            }
            __syncthreads();
            double off = 0.0, all = 0.0;
            for (int p = 0; p < m; ++p) { off += s_red[0][p]; all += s_red[1][p]; }
            if (!(off > 1e-30 * all)) break;                 // (uniform: the same words in the same order in every lane)
            for (int r = 0; r < ring; ++r) {
                if (tid < half) {
                    int x = tid == 0 ? r : (r + tid) % ring, y = tid == 0 ? ring : (r - tid + ring) % ring;
                    const int p = x < y ? x : y, q = x < y ? y : x;
                    int pp = -1;
                    if (q < m) {
                        const double br = Qr[p * AS_LD + q], bi = Qi[p * AS_LD + q];
                        const double g = hypot(br, bi);
                        if (g != 0.0) {
                            const double app = Qr[p * AS_LD + p], aqq = Qr[q * AS_LD + q];
                            const double tau = (aqq - app) / (2.0 * g);
                            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(tau) + sqrt(1.0 + tau * tau));
                            const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                            s_c[tid] = c; s_ser[tid] = s * (br / g); s_sei[tid] = s * (bi / g);
                            pp = p;
                        }
                    }
                    s_p[tid] = pp; s_q[tid] = q;
                }
                __syncthreads();
                for (int e = tid; e < 2 * half * m; e += AS_LANES) {         // columns of Q, then of V
                    const int img = e / (half * m), pr = (e / m) % half, k = e % m;
                    const int p = s_p[pr];
                    if (p >= 0) as_col_rot(img ? Vr : Qr, img ? Vi : Qi, k, p, s_q[pr], s_c[pr], s_ser[pr], s_sei[pr]);
                }
                __syncthreads();
                for (int e = tid; e < half * m; e += AS_LANES) {             // rows of Q (J^H from the left)
                    const int pr = e / m, k = e % m;
                    const int p = s_p[pr], q = s_q[pr];
                    if (p < 0) continue;
                    const double c = s_c[pr], ser = s_ser[pr], sei = s_sei[pr];
                    const double xr = Qr[p * AS_LD + k], xi = Qi[p * AS_LD + k], yr = Qr[q * AS_LD + k], yi = Qi[q * AS_LD + k];
                    double npr = c * xr - (ser * yr - sei * yi), npi = c * xi - (ser * yi + sei * yr);
                    double nqr = ser * xr + sei * xi + c * yr, nqi = ser * xi - sei * xr + c * yi;
                    if (k == p) { npi = 0.0; nqr = 0.0; nqi = 0.0; }
                    if (k == q) { npr = 0.0; npi = 0.0; nqi = 0.0; }
                    Qr[p * AS_LD + k] = npr; Qi[p * AS_LD + k] = npi;
                    Qr[q * AS_LD + k] = nqr; Qi[q * AS_LD + k] = nqi;
                }
                __syncthreads();
            }
        }
        __syncthreads();                                     // every wave has formed the last verdict and left the loop
        for (int p = 1; p < m; ++p)
            if (Qr[p * AS_LD + p] > Qr[i1 * AS_LD + i1]) i1 = p;
        lambda1 = Qr[i1 * AS_LD + i1];
        lambda2 = -1.0;
        for (int p = 0; p < m; ++p)
            if (p != i1 && Qr[p * AS_LD + p] > lambda2) lambda2 = Qr[p * AS_LD + p];
        if (lambda2 < 0.0) lambda2 = 0.0;
        if (!(lambda1 > 0.0) || !as_finite(lambda1)) status = 5;
    }

    // ---- 6. s = C v;  7. the word of largest modulus real and positive;  8. s^H s = m;  9. one rounding to f32
    cf word = cf_make(0.0f, 0.0f);
    int ref = 0;
    if (!status) {
        if (tid < m) {
            double xr = 0.0, xi = 0.0;
            for (int k = 0; k <= tid; ++k) {
                const double cr = Cr[tid * AS_LD + k], ci = Ci[tid * AS_LD + k], vr = Vr[k * AS_LD + i1], vi = Vi[k * AS_LD + i1];
                xr += cr * vr - ci * vi;
                xi += cr * vi + ci * vr;
            }
            s_s[0][tid] = xr; s_s[1][tid] = xi;
        }
        __syncthreads();
        double best = -1.0, e = 0.0;
        for (int p = 0; p < m; ++p) {
            const double a2 = s_s[0][p] * s_s[0][p] + s_s[1][p] * s_s[1][p];
            e += a2;
            if (a2 > best) { best = a2; ref = p; }
        }
        if (!(best > 0.0) || !as_finite(e)) status = 6;
        else if (tid < m) {
            const double g = sqrt(best), scale = sqrt(double(m) / e);
            const double rr = s_s[0][ref] / g, ri = -s_s[1][ref] / g;
            const double sr = s_s[0][tid], si = s_s[1][tid];
            word.x = float((sr * rr - si * ri) * scale);
            word.y = tid == ref ? 0.0f : float((sr * ri + si * rr) * scale);
        }
    }

    if (tid < m) a.rows[uint64_t(row) * m + tid] = status ? cf_make(0.0f, 0.0f) : word;
    if (tid == 0) {
        AsInfo o;
        o.lambda1 = status ? 0.0 : lambda1; o.lambda2 = status ? 0.0 : lambda2;
        o.ref_index = status ? 0u : uint32_t(ref); o.status = uint32_t(status);
        reinterpret_cast<AsInfo*>(a.info)[row] = o;
    }
}

// gm_beamformer_set_steering_dev: one 64-lane workgroup a row; M <= 32 words, lane k word k
__global__ __launch_bounds__(64) void beam_install_kernel(const BeamInstallArgs a) {
    const int tid = threadIdx.x, M = int(a.M);
    const uint32_t p = blockIdx.x;
    cf w = cf_make(0.0f, 0.0f);
    if (tid < M) w = a.rows[size_t(p) * M + tid];
    const bool fin = as_finite(w.x) && as_finite(w.y), any = w.x != 0.0f || w.y != 0.0f;
    bool ok = __ballot(!fin) == 0ull && __ballot(any) != 0ull;
    if (ok && a.info) {
        const AsInfo o = reinterpret_cast<const AsInfo*>(a.info)[p];
        ok = o.status == 0u && o.lambda1 >= double(a.min_ratio) * o.lambda2;
    }
    if (ok && tid < M) a.s[size_t(a.first_beam + p) * M + tid] = w;
    if (a.installed && tid == 0) a.installed[p] = ok ? 1 : 0;
}
}  // namespace

void launch_array_solve(hipStream_t st, const ArraySolveArgs& a) {
    hipLaunchKernelGGL(array_solve_kernel, dim3(a.n_rows), dim3(AS_LANES), 0, st, a);
}
void launch_beam_install(hipStream_t st, const BeamInstallArgs& a) {
    hipLaunchKernelGGL(beam_install_kernel, dim3(a.n_rows), dim3(64), 0, st, a);
}
}  // namespace gm
