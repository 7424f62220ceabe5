// acq_array.hip — space-time prompts of an antenna array at known cells (gm_acq_array_prompts).
//
// One kernel, one 256-lane workgroup per (period, candidate):
//   z[l][a] = sum_{n<N} x_a[s + n - l] ref[n],   ref[n] = tab[d][n] c_w[(n - cp) mod N],   x_a[t] = element t A + a of the stream.
// Seen from the samples: time sample u = n - l (relative to the period start s, u in [-(L-1), N)) meets ref[u .. u + L - 1], so a lane
// that owns WHOLE time samples loads a time sample's A words once and feeds all M = L A sums from them.  The period is cut into tiles of
// 1024 time samples from u = -(L-1) on; lane j owns u0 + j, u0 + j + 256, ... of a tile and takes them in ascending u.  A tile's ref
// words sit in LDS at position p <-> ref[u0 + p], p < 1024 + L - 1, zero outside [0, N): the first L - 1 positions are the last L - 1 of
// the tile before (copied LDS to LDS, so every table word is read from memory once), the rest is formed from the table and the replica.
// Two LDS images alternate, so one barrier a tile is enough: a tile's image is written while the tile before is still being read.
//
// After the last tile: a wave's 64 sums by a fixed butterfly (d = 32 .. 1), then the four waves through LDS in ascending order.  No
// floating-point atomics.  gnss_mi355x.h states the order word for word.
//
// Loads.  A time sample is TS = A * 8 (c32) or A * 2 (int8 IQ) bytes.  V = the widest power of two <= 16 that divides TS; where the
// period's first byte is a multiple of V (uniform over the workgroup) a time sample is TS / V loads of V bytes, else A element loads
// (the stream is aligned to its element size only, and a code-drift start is any time sample).  Both paths form the same floats.
//
// Instantiations: <FMT, A, LC>, LC the class of L (1, 2, 4, or the most taps A allows: 8, 8, 8, 6, 5, 4, 4 for A = 2 .. 8) — the tap
// loop runs to LC with a uniform test against L, so the accumulators stay in registers.  Compiled with -ffp-contract=off: every fused
// operation is written as __builtin_fmaf.
#include "gm_internal.h"

namespace gm {
namespace {

constexpr int AR_T = 256;                         // lanes per workgroup
constexpr int AR_PER = 4;                         // time samples per lane and tile
constexpr int AR_TILE = AR_T * AR_PER;            // time samples per tile
constexpr int AR_HALO = ST_L_MAX - 1;
constexpr int AR_REF_WORDS = AR_TILE + AR_HALO;

typedef unsigned int ar_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int ar_u32x4 __attribute__((ext_vector_type(4)));

constexpr int ar_ts_bytes(int fmt, int A) { return A * (fmt == GM_FMT_C32 ? 8 : 2); }
constexpr int ar_widest(int ts) { return ts % 16 == 0 ? 16 : ts % 8 == 0 ? 8 : ts % 4 == 0 ? 4 : 2; }

// the A words of the time sample at byte address p: WIDE — loads of ar_widest(TS) bytes, p a multiple of it; else element loads
template <int FMT, int A, bool WIDE> __device__ __forceinline__ void ar_load(const char* p, float (&xr)[A], float (&xi)[A]) {
    constexpr int TS = ar_ts_bytes(FMT, A), V = ar_widest(TS);
    if constexpr (FMT == GM_FMT_C32) {
        if constexpr (WIDE && V == 16) {
            const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
            for (int e = 0; e < A / 2; ++e) {
                const float4 v = q[e];
                xr[2 * e] = v.x; xi[2 * e] = v.y; xr[2 * e + 1] = v.z; xi[2 * e + 1] = v.w;
            }
        } else {                                  // (V = 8 is the element itself)
            const cf* q = reinterpret_cast<const cf*>(p);
#pragma unroll
            for (int e = 0; e < A; ++e) { const cf v = q[e]; xr[e] = v.x; xi[e] = v.y; }
        }
    } else {
        if constexpr (WIDE && V >= 4) {
            uint32_t w[TS / 4];
            if constexpr (V == 16) {
                const ar_u32x4 v = *reinterpret_cast<const ar_u32x4*>(p);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else if constexpr (V == 8) {
                const ar_u32x2 v = *reinterpret_cast<const ar_u32x2*>(p);
                w[0] = v.x; w[1] = v.y;
            } else {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int e = 0; e < TS / 4; ++e) w[e] = q[e];
            }
#pragma unroll
            for (int e = 0; e < A; ++e) {
                const uint32_t h = w[e >> 1] >> (16 * (e & 1));
                xr[e] = float(int8_t(h)); xi[e] = float(int8_t(h >> 8));
            }
        } else {
            const char2* q = reinterpret_cast<const char2*>(p);
#pragma unroll
            for (int e = 0; e < A; ++e) { const char2 v = q[e]; xr[e] = float(v.x); xi[e] = float(v.y); }
        }
    }
}

// the lane's AR_PER time samples of one tile, in ascending u: u = u0 + tid + 256 j.  lo, hi: the time samples that exist, lo <= u < hi
template <int FMT, int A, int LC, bool WIDE>
__device__ __forceinline__ void ar_tile(const char* sp, int64_t u0, int64_t lo, int64_t hi, int L, int tid, const cf* __restrict__ ref,
                                        float (&ar)[LC][A], float (&ai)[LC][A]) {
    constexpr int TS = ar_ts_bytes(FMT, A);
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) {
        const int p = tid + AR_T * j;
        const int64_t u = u0 + p;
        if (u < lo || u >= hi) continue;
        float xr[A], xi[A];
        ar_load<FMT, A, WIDE>(sp + u * TS, xr, xi);
#pragma unroll
        for (int l = 0; l < LC; ++l) {
            if (l < L) {
                const cf r = ref[p + l];
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    ar[l][a] = __builtin_fmaf(xr[a], r.x, ar[l][a]);
                    ar[l][a] = __builtin_fmaf(-xi[a], r.y, ar[l][a]);
                    ai[l][a] = __builtin_fmaf(xr[a], r.y, ai[l][a]);
                    ai[l][a] = __builtin_fmaf(xi[a], r.x, ai[l][a]);
                }
            }
        }
    }
}

template <int FMT, int A, int LC>
__global__ __launch_bounds__(AR_T) void acq_array_prompts_kernel(const void* __restrict__ samples, const uint64_t* __restrict__ starts,
                                                                 uint32_t R, const cf* __restrict__ tables,
                                                                 const int8_t* __restrict__ code_samples,
                                                                 const RefineSat* __restrict__ cands, uint32_t N, uint32_t R_u, uint32_t L,
                                                                 cf* __restrict__ z) {
    static_assert(A * LC <= 2 * ST_M_MAX && LC <= ST_L_MAX, "no such class");
    __shared__ cf ref_s[2][AR_REF_WORDS];
    __shared__ cf part_s[AR_T / 64][ST_M_MAX];
    constexpr int TS = ar_ts_bytes(FMT, A), V = ar_widest(TS);
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x, cand = blockIdx.y;
    const RefineSat w = cands[cand];
    // the period's start, a 64-bit TIME sample index, uniform over the workgroup (as acq_local_despread_kernel reads it)
    uint64_t s = starts ? starts[size_t(w.bin) * R + w.offset + i] : uint64_t(w.offset + i) * N;
    s = uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s))) | (uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(s >> 32))) << 32);
    const uint32_t cp = __builtin_amdgcn_readfirstlane(w.code_phase);
    const cf* tab = tables + size_t(w.bin) * N;
    const int8_t* rep = code_samples + size_t(w.worker) * N;
    const char* sp = static_cast<const char*>(samples) + s * uint64_t(TS);
    const bool wide = (reinterpret_cast<uintptr_t>(sp) & uintptr_t(V - 1)) == 0;
    const int H = int(L) - 1;
    // the time samples that exist: u >= -H, and not in front of the stream (s + u >= 0)
    const int64_t lo = s < uint64_t(H) ? -int64_t(s) : -int64_t(H), hi = int64_t(N);

    float ar[LC][A], ai[LC][A];
#pragma unroll
    for (int l = 0; l < LC; ++l)
#pragma unroll
        for (int a = 0; a < A; ++a) { ar[l][a] = 0.0f; ai[l][a] = 0.0f; }

    const uint32_t n_tiles = (N + uint32_t(H) + AR_TILE - 1) / AR_TILE;
    for (uint32_t k = 0; k < n_tiles; ++k) {
        cf* ref = ref_s[k & 1];
        const cf* prev = ref_s[(k & 1) ^ 1];
        // position p <-> ref[u0 + p], u0 = k TILE - H: the halo from the image before, then the table words n = k TILE + q
        if (tid < H) ref[tid] = k ? prev[AR_TILE + tid] : cf_make(0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < AR_PER; ++j) {
            const uint32_t q = uint32_t(tid) + AR_T * j, n = k * AR_TILE + q;
            cf v = cf_make(0.0f, 0.0f);
            if (n < N) {
                const cf t = tab[n];
                const uint32_t m = n >= cp ? n - cp : n + N - cp;      // (n - cp) mod N: cp < N
                const float c = float(rep[m]);                          // +-1: the products are exact
                v = cf_make(t.x * c, t.y * c);
            }
            ref[H + q] = v;
        }
        __syncthreads();
        const int64_t u0 = int64_t(k) * AR_TILE - H;
        if (wide) ar_tile<FMT, A, LC, true>(sp, u0, lo, hi, int(L), tid, ref, ar, ai);
        else ar_tile<FMT, A, LC, false>(sp, u0, lo, hi, int(L), tid, ref, ar, ai);
    }

    // a wave's sums by the fixed butterfly, then the four waves in ascending order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        if (l < int(L)) {
#pragma unroll
            for (int a = 0; a < A; ++a) {
                float re = ar[l][a], im = ai[l][a];
#pragma unroll
                for (int d = 32; d; d >>= 1) { re = re + __shfl_down(re, d, 64); im = im + __shfl_down(im, d, 64); }
                if (lane == 0) part_s[wave][l * A + a] = cf_make(re, im);
            }
        }
    }
    __syncthreads();
    const uint32_t M = L * A;
    if (uint32_t(tid) < M) {
        float re = part_s[0][tid].x, im = part_s[0][tid].y;
#pragma unroll
        for (int v = 1; v < AR_T / 64; ++v) { re = re + part_s[v][tid].x; im = im + part_s[v][tid].y; }
        z[(size_t(cand) * R_u + i) * M + tid] = cf_make(re, im);
    }
}

template <int FMT, int A, int LC> void ar_launch(hipStream_t st, const ArrayArgs& a) {
    hipLaunchKernelGGL((acq_array_prompts_kernel<FMT, A, LC>), dim3(a.R_u, a.n_cands), dim3(AR_T), 0, st, a.samples, a.starts, a.R, a.tables,
                       a.code_samples, a.cands, a.N, a.R_u, a.L, a.z);
}
// LMAX = the most taps A allows (A L <= 32, L <= 8): the widest class of A
template <int FMT, int A> void ar_launch_a(hipStream_t st, const ArrayArgs& a) {
    constexpr int LMAX = ST_M_MAX / A < ST_L_MAX ? ST_M_MAX / A : ST_L_MAX;
    if (a.L <= 1) ar_launch<FMT, A, 1>(st, a);
    else if (a.L <= 2) ar_launch<FMT, A, 2>(st, a);
    else if (a.L <= 4) ar_launch<FMT, A, 4>(st, a);
    else if constexpr (LMAX > 4) ar_launch<FMT, A, LMAX>(st, a);
}
template <int FMT> void ar_launch_fmt(hipStream_t st, const ArrayArgs& a) {
    switch (a.A) {
        case 2: ar_launch_a<FMT, 2>(st, a); break;
        case 3: ar_launch_a<FMT, 3>(st, a); break;
        case 4: ar_launch_a<FMT, 4>(st, a); break;
        case 5: ar_launch_a<FMT, 5>(st, a); break;
        case 6: ar_launch_a<FMT, 6>(st, a); break;
        case 7: ar_launch_a<FMT, 7>(st, a); break;
        case 8: ar_launch_a<FMT, 8>(st, a); break;
        default: break;                           // (the entry has refused it)
    }
}

}  // namespace

void launch_array(hipStream_t st, const ArrayArgs& a) {
    if (a.fmt == GM_FMT_C32) ar_launch_fmt<GM_FMT_C32>(st, a);
    else ar_launch_fmt<GM_FMT_I8_IQ>(st, a);
}

}  // namespace gm
