// trk_array.hip — gm_trk_array_prompts: per-antenna, per-tap prompts of an interleaved array stream at tracked states (gfx950, wave64;
// DESIGN 4.3b).
//
// A SECTION of trk_kernels.hip, included at the end of its namespace behind trk_bank.hip (it is not a translation unit of its own): the
// replica is formed with the tracker's own helpers — EpochConsts / epoch_consts, fast_code_ok / fast_car_ok, fmod_code, chip_index,
// div_by_fs and the sincos forms — which live in that file, and none of the kernels above is touched by it.  include/gnss_mi355x.h
// states the definition:
//
//   phase_i = carrier_phase + fl(fl(fl(2 pi) carrier_freq) i) / fs,  c[i] = (code_phase + i (code_rate / fs)) mod code_len,
//   ref[i] = (cos phase_i, -sin phase_i) chip(fl(c[i] + tau)),  z[r][l][a] = sum_{i < n} x_a[s + i - l] ref[i],  x_a[t] = element
//   (t - first_index) A + a of the stream.
//
// Seen from the samples (as acq_array.hip sees them): time sample u = i - l (relative to the record's start s, u in [-(L-1), n)) meets
// ref[u .. u + L - 1], so a lane that owns WHOLE time samples loads a time sample's A words once and feeds all L A sums from them.
//
//   trk_array_kernel<FMT, A, LC> : grid (slices, records), 256 lanes.  Slice k owns the time samples u in [4096 k, 4096 (k + 1)) below n;
//       slice 0 owns the L - 1 halo samples u in [-(L-1), 0) as well, so the slice count is ceil(n / 4096).  The record's chip row sits
//       in LDS beside the slice's ref image, position p <-> ref[4096 k + p], p < 4096 + L - 1, zero from n on: each word is formed ONCE —
//       one sincos, one chip look-up, one sign (a chip is +-1 x the BOC sub-carrier sign: an exact sign flip).  The slices split the time
//       samples, not the ref indices, so the L - 1 ref words behind a slice's end are formed again by the next slice; no sample is loaded
//       twice.  Lane j takes, in this order: the halo sample u = j - (L-1) (slice 0, j < L - 1), then u = 4096 k + j + 256 m, m = 0 .. 15.
//       Per-lane sums -> the wave's 64 by a fixed butterfly (xor 32 .. 1) -> the four waves through LDS in ascending order -> one partial
//       per (record, slice, l, a).
//   trk_array_sum_kernel : one workgroup per record adds the slices in ascending order, writes zeros for a skipped record, and `done`.
//
// Nothing is shared between records and the slice count is a function of n alone: a record's words depend neither on what else is in the
// call, nor on repetition, nor on where the buffer starts.  No floating-point atomics.  Nothing is written but the partials and the outputs.
//
// Loads: acq_array.hip's rule.  A time sample is TS = A * 8 (c32) or A * 2 (int8 IQ) bytes, V = the widest power of two <= 16 that divides
// TS; where the record's first byte is a multiple of V (uniform over the workgroup) a time sample is TS / V loads of V bytes, else A
// element loads.  Both paths form the same floats.
// Bounds: the host (gm_trk_array_prompts, gm_api.hip) runs a record only if [max(0, s - (L-1)), s + n) lies inside the buffer; the kernel
// reads the time samples s + u with max(-(L-1), -s) <= u < n and nothing else.  A chip index lies in [0, code_len) for the bank's reason
// (|c[i]| < code_len, |tau| < code_len / 2).
// Every fused operation is written as __builtin_fmaf (the file is compiled with -ffp-contract=off).

constexpr int TA_T = 256;                                   // lanes per workgroup
constexpr int TA_SLICE = int(GM_TRK_ARRAY_SLICE);           // time samples per workgroup
constexpr int TA_PER = TA_SLICE / TA_T;                     // time samples per lane (besides a halo sample)
constexpr int TA_REF_WORDS = TA_SLICE + GM_TRK_ARRAY_MAX_TAPS - 1;

typedef unsigned int ta_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int ta_u32x4 __attribute__((ext_vector_type(4)));

constexpr int ta_ts_bytes(int fmt, int A) { return A * (fmt == GM_FMT_C32 ? 8 : 2); }
constexpr int ta_widest(int ts) { return ts % 16 == 0 ? 16 : ts % 8 == 0 ? 8 : ts % 4 == 0 ? 4 : 2; }

// the A words of the time sample at byte address p: WIDE — loads of ta_widest(TS) bytes, p a multiple of it; else element loads
template <int FMT, int A, bool WIDE> __device__ __forceinline__ void ta_load(const char* p, float (&xr)[A], float (&xi)[A]) {
    constexpr int TS = ta_ts_bytes(FMT, A), V = ta_widest(TS);
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
                const ta_u32x4 v = *reinterpret_cast<const ta_u32x4*>(p);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else if constexpr (V == 8) {
                const ta_u32x2 v = *reinterpret_cast<const ta_u32x2*>(p);
                w[0] = v.x; w[1] = v.y;
            } else {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int e = 0; e < TS / 4; ++e) w[e] = q[e];
            }
#pragma unroll
            for (int e = 0; e < A; ++e) {
                const uint32_t h = w[e >> 1] >> (16 * (e & 1));
                xr[e] = float(int8_t(h)); xi[e] = float(int8_t(h >> 8));      // -128 is -128.0f
            }
        } else {
            const char2* q = reinterpret_cast<const char2*>(p);
#pragma unroll
            for (int e = 0; e < A; ++e) { const char2 v = q[e]; xr[e] = float(v.x); xi[e] = float(v.y); }
        }
    }
}

// the slice's ref image: position p <-> ref[i0 + p], zero from n on
template <bool FASTC>
__device__ __forceinline__ void ta_ref_image(const EpochConsts& ec, const int8_t* chips, float tau, uint32_t i0, uint32_t n, int words,
                                             cf* __restrict__ ref) {
    const bool fast = FASTC && fast_car_ok(ec, float(n));                      // = fast_code_range of the epoch, as the bank takes it
    for (int p = threadIdx.x; p < words; p += TA_T) {
        const uint32_t i = i0 + uint32_t(p);                                   // n < 2^31 and i0 < n: no wrap
        cf v = cf_make(0.0f, 0.0f);
        if (i < n) {
            const float w = ec.two_pi_f * float(i);
            const float phase = ec.carrier_phase + (fast ? div_by_fs(w, ec.fs, ec.inv_fs) : __fdiv_rn(w, ec.fs));
            float sn, cs;
            if (ec.strict) sincosf_glibc(phase, sn, cs);
            else sincos_f32_via_f64(phase, sn, cs);
            const float chip_idx = fmod_code<FASTC>(ec.code_phase + float(i) * ec.step, ec.lenf);      // as correlate_sample forms it
            const float ph = chip_idx + tau;
            uint32_t neg = chips[chip_index(ph, ec.len, ec.mode)] < 0 ? 1u : 0u;
            if (ec.boc11) neg ^= (ph - floorf(ph)) < 0.5f ? 0u : 1u;           // BOC(1,1): -1 on the second half chip, as the arms take it
            const uint32_t s = neg << 31;
            v = cf_make(__uint_as_float(__float_as_uint(cs) ^ s), __uint_as_float(__float_as_uint(-sn) ^ s));      // (cos, -sin) x +-1
        }
        ref[p] = v;
    }
}

// one time sample into the lane's sums: taps l0 <= l < L meet ref[q + l]
template <int A, int LC>
__device__ __forceinline__ void ta_feed(const float (&xr)[A], const float (&xi)[A], const cf* __restrict__ ref, int q, int l0, int L,
                                        float (&ar)[LC][A], float (&ai)[LC][A]) {
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        if (l >= l0 && l < L) {
            const cf r = ref[q + l];
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

// the lane's time samples of the slice in ascending u; sp: the byte address of time sample u = 0; lo: the first time sample that exists
template <int FMT, int A, int LC, bool WIDE>
__device__ __forceinline__ void ta_slice(const char* sp, uint32_t slice, int64_t lo, uint32_t n, int L, int tid, const cf* __restrict__ ref,
                                         float (&ar)[LC][A], float (&ai)[LC][A]) {
    constexpr int TS = ta_ts_bytes(FMT, A);
    const int H = L - 1;
    if (slice == 0 && tid < H) {                  // the halo: u = tid - H < 0 meets ref[u + l] for l >= -u
        const int u = tid - H;
        if (int64_t(u) >= lo) {
            float xr[A], xi[A];
            ta_load<FMT, A, WIDE>(sp + int64_t(u) * TS, xr, xi);
            ta_feed<A, LC>(xr, xi, ref, u, -u, L, ar, ai);
        }
    }
    const uint32_t i0 = slice * uint32_t(TA_SLICE);
#pragma unroll 2
    for (int j = 0; j < TA_PER; ++j) {
        const int p = tid + TA_T * j;
        const uint32_t u = i0 + uint32_t(p);
        if (u < n) {
            float xr[A], xi[A];
            ta_load<FMT, A, WIDE>(sp + int64_t(u) * TS, xr, xi);
            ta_feed<A, LC>(xr, xi, ref, p, 0, L, ar, ai);
        }
    }
}

template <int FMT, int A, int LC>
__global__ __launch_bounds__(TA_T) void trk_array_kernel(TrkDevCfg cfg, const int8_t* __restrict__ codes, TrkArrayArgs a) {
    static_assert(A * LC <= GM_TRK_ARRAY_MAX_WORDS && LC <= GM_TRK_ARRAY_MAX_TAPS, "no such class");
    const TrkBankRec rec = a.recs[blockIdx.y];
    if (!rec.run || blockIdx.x >= rec.slices) return;           // uniform over the workgroup
    extern __shared__ int8_t chips[];                           // code_len chips of this record's row (row checked on the host)
    __shared__ cf ref_s[TA_REF_WORDS];
    __shared__ cf part_s[TA_T / 64][GM_TRK_ARRAY_MAX_WORDS];
    constexpr int TS = ta_ts_bytes(FMT, A), V = ta_widest(TS);
    const int tid = threadIdx.x, L = a.L, H = L - 1;
    const uint32_t slice = blockIdx.x, n = rec.n;
    const int8_t* crow = codes + size_t(code_row(cfg, rec.st)) * cfg.code_len;
    for (int i = tid; i < cfg.code_len; i += TA_T) chips[i] = crow[i];
    __syncthreads();
    const EpochConsts ec = epoch_consts(cfg, rec.st);
    const uint32_t i0 = slice * uint32_t(TA_SLICE);
    if (fast_code_ok(ec, n)) ta_ref_image<true>(ec, chips, a.tau, i0, n, TA_SLICE + H, ref_s);
    else ta_ref_image<false>(ec, chips, a.tau, i0, n, TA_SLICE + H, ref_s);
    __syncthreads();

    // the record's start, a 64-bit TIME sample index, uniform over the workgroup; the host has checked s >= first_index
    const uint64_t s = rec.st.next_sample_index;
    const char* sp = static_cast<const char*>(a.samples) + (s - a.first_index) * uint64_t(TS);
    const bool wide = (reinterpret_cast<uintptr_t>(sp) & uintptr_t(V - 1)) == 0;
    const int64_t lo = s < uint64_t(H) ? -int64_t(s) : -int64_t(H);      // a time index below 0 reads as zero

    float ar[LC][A], ai[LC][A];
#pragma unroll
    for (int l = 0; l < LC; ++l)
#pragma unroll
        for (int e = 0; e < A; ++e) { ar[l][e] = 0.0f; ai[l][e] = 0.0f; }
    if (wide) ta_slice<FMT, A, LC, true>(sp, slice, lo, n, L, tid, ref_s, ar, ai);
    else ta_slice<FMT, A, LC, false>(sp, slice, lo, n, L, tid, ref_s, ar, ai);

    // a wave's sums by the fixed butterfly, then the four waves in ascending order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        if (l < L) {
#pragma unroll
            for (int e = 0; e < A; ++e) {
                float re = ar[l][e], im = ai[l][e];
#pragma unroll
                for (int d = 32; d; d >>= 1) { re = re + __shfl_xor(re, d, 64); im = im + __shfl_xor(im, d, 64); }
                if (lane == 0) part_s[wave][l * A + e] = cf_make(re, im);
            }
        }
    }
    __syncthreads();
    const int M = L * A;
    if (tid < M) {
        float re = part_s[0][tid].x, im = part_s[0][tid].y;
#pragma unroll
        for (int v = 1; v < TA_T / 64; ++v) { re = re + part_s[v][tid].x; im = im + part_s[v][tid].y; }
        a.partials[(size_t(rec.poff) + slice) * size_t(M) + tid] = cf_make(re, im);
    }
}

__global__ __launch_bounds__(64) void trk_array_sum_kernel(TrkArrayArgs a, cf* __restrict__ z, uint8_t* __restrict__ done) {
    const TrkBankRec rec = a.recs[blockIdx.x];
    const int M = a.L * a.A, w = threadIdx.x;
    if (w < M) {
        float re = 0.0f, im = 0.0f;
        if (rec.run) {
            const cf* p = a.partials + size_t(rec.poff) * size_t(M);
            re = p[w].x; im = p[w].y;
            for (uint32_t sl = 1; sl < rec.slices; ++sl) { re = re + p[size_t(sl) * M + w].x; im = im + p[size_t(sl) * M + w].y; }   // ascending slices
        }
        z[size_t(blockIdx.x) * M + w] = cf_make(re, im);
    }
    if (w == 0) done[blockIdx.x] = rec.run ? 1 : 0;
}

template <int FMT, int A, int LC>
void ta_launch(hipStream_t st, const TrkDevCfg& cfg, const int8_t* d_codes, const TrkArrayArgs& a, int n_records, uint32_t max_slices) {
    hipLaunchKernelGGL((trk_array_kernel<FMT, A, LC>), dim3(max_slices, n_records), dim3(TA_T), size_t(cfg.code_len), st, cfg, d_codes, a);
}
// LMAX = the most taps A allows (A L <= 32, L <= 8): the widest class of A
template <int FMT, int A>
void ta_launch_a(hipStream_t st, const TrkDevCfg& cfg, const int8_t* d_codes, const TrkArrayArgs& a, int n_records, uint32_t max_slices) {
    constexpr int LMAX = GM_TRK_ARRAY_MAX_WORDS / A < GM_TRK_ARRAY_MAX_TAPS ? GM_TRK_ARRAY_MAX_WORDS / A : GM_TRK_ARRAY_MAX_TAPS;
    if (a.L <= 1) ta_launch<FMT, A, 1>(st, cfg, d_codes, a, n_records, max_slices);
    else if (a.L <= 2) ta_launch<FMT, A, 2>(st, cfg, d_codes, a, n_records, max_slices);
    else if (a.L <= 4) ta_launch<FMT, A, 4>(st, cfg, d_codes, a, n_records, max_slices);
    else if constexpr (LMAX > 4) ta_launch<FMT, A, LMAX>(st, cfg, d_codes, a, n_records, max_slices);
}
template <int FMT>
void ta_launch_fmt(hipStream_t st, const TrkDevCfg& cfg, const int8_t* d_codes, const TrkArrayArgs& a, int n_records, uint32_t max_slices) {
    switch (a.A) {
        case 2: ta_launch_a<FMT, 2>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 3: ta_launch_a<FMT, 3>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 4: ta_launch_a<FMT, 4>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 5: ta_launch_a<FMT, 5>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 6: ta_launch_a<FMT, 6>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 7: ta_launch_a<FMT, 7>(st, cfg, d_codes, a, n_records, max_slices); break;
        case 8: ta_launch_a<FMT, 8>(st, cfg, d_codes, a, n_records, max_slices); break;
        default: break;                           // (the entry has refused it)
    }
}

void launch_trk_array(hipStream_t st, const TrkDevCfg& cfg, const int8_t* d_codes, const TrkArrayArgs& a, int n_records, uint32_t max_slices,
                      gm_c32* d_z, uint8_t* d_done) {
    if (max_slices) {           // (no record runs: the sum kernel writes the zeros)
        if (a.fmt == GM_FMT_C32) ta_launch_fmt<GM_FMT_C32>(st, cfg, d_codes, a, n_records, max_slices);
        else ta_launch_fmt<GM_FMT_I8_IQ>(st, cfg, d_codes, a, n_records, max_slices);
    }
    hipLaunchKernelGGL(trk_array_sum_kernel, dim3(n_records), dim3(64), 0, st, a, reinterpret_cast<cf*>(d_z), d_done);
}
