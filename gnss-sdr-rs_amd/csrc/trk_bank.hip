// trk_bank.hip — gm_trk_bank / gm_trk_bank_samples: a tap x carrier-offset correlator bank at tracked states (gfx950, wave64).
//
// A SECTION of trk_kernels.hip, included at the end of its namespace (it is not a translation unit of its own): the bank forms its
// samples with the tracker's own helpers — EpochConsts / epoch_consts, fast_code_ok / fast_car_ok (the two halves of
// fast_code_range), fmod_code, chip_index, div_by_fs and the sincos forms of trk_correlate_kernel — which live in that file, and
// none of the kernels above is touched by it.  include/gnss_mi355x.h states the definition:
//
//   f_f = fl(carrier_freq + df_f),  phase_i = carrier_phase + fl(fl(fl(2 pi) f_f) i) / fs,  y_f[i] = x[i] (cos phase_i, -sin phase_i),
//   c[i] = (code_phase + i (code_rate / fs)) mod code_len,  out[r][f][t] = sum_{i < n} y_f[i] chip(fl(c[i] + tau_t))
//
//   trk_bank_kernel<TG> : grid (slices of 4096 samples, records, tap groups of TG <= 16 taps), 256 lanes.  The record's chip row sits in
//       LDS.  A lane owns 16 samples of the slice (i = 4096 slice + 256 k + lane): it reads each ONCE from memory, forms c[i]
//       ONCE and looks every tap of the group up ONCE — a chip is +-1 (x the BOC sub-carrier sign), so what a look-up yields is a sign,
//       and the TG signs of a sample are 16 bits; sample and signs wait in LDS places of the lane's own (40 KB per workgroup).  Then, per carrier offset, y_f[i] is formed once per sample and added
//       into the group's 2 TG sums with the sign bit applied: y x (+-1) is exact, so acc + (+-y) is what gm_trk_correlate's
//       fma(y, chip, acc) adds, bit for bit.  Per-lane sums in sample order -> wave butterfly -> the four waves through LDS in a
//       fixed order -> one partial per (record, slice, offset, tap).  Taps beyond the group go to further workgroups on grid.z, which
//       read the same samples again (from L2).
//   trk_bank_sum_kernel : one workgroup per record adds the slices in ascending order, writes zeros for a skipped record, and `done`.
//
// The slice count of a record is ceil(n / 4096), a function of n alone, and nothing is shared between records: a record's words depend
// neither on what else is in the call nor on repetition.  No atomics.  Nothing is written but the partials and the outputs.
// Bounds: the host (trk_bank_run, gm_api.hip) decides which records run and hands n, the slice count and the partial offset over
// in TrkBankRec; ring indices are masked, linear indices are tested against n; a chip index lies in [0, code_len) because |c[i]| <
// code_len (fmod_code, or not a number: index 0) and |tau| < code_len / 2 (gm_trk_bank_plan), which is what chip_index's single
// wrap needs.

constexpr int TRK_BANK_SLICE = int(GM_TRK_BANK_SLICE);   // samples per workgroup (4096): 256 lanes x TRK_BANK_NS
constexpr int TRK_BANK_NS = TRK_BANK_SLICE / 256;    // samples a lane keeps in registers

// the TG sign bits of one sample: bit j set <-> chip(fl(c + tau[j])) is negative
template <int TG, bool FASTC>
__device__ __forceinline__ uint32_t bank_signs(const EpochConsts& c, const int8_t* chips, uint32_t i, const float (&tau)[TG]) {
    const float chip_idx = fmod_code<FASTC>(c.code_phase + float(i) * c.step, c.lenf);      // as correlate_sample forms it
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < TG; ++j) {
        const float p = chip_idx + tau[j];
        uint32_t neg = chips[chip_index(p, c.len, c.mode)] < 0 ? 1u : 0u;
        if (c.boc11) neg ^= (p - floorf(p)) < 0.5f ? 0u : 1u;       // BOC(1,1): -1 on the second half chip, as the arms take it
        m |= neg << j;
    }
    return m;
}

template <int TG, bool FASTC>
__device__ __forceinline__ void trk_bank_body(const TrkDevCfg& cfg, const TrkBankArgs& a, const TrkBankRec& rec, const EpochConsts& ec,
                                              const int8_t* chips, cf* xs, uint16_t* sgs, float (&wsum)[GM_TRK_BANK_MAX_OFFSETS][4][2 * TG]) {
    constexpr int NV = 2 * TG;
    const int tid = threadIdx.x, slice = blockIdx.x, t0 = int(blockIdx.z) * TG;
    const uint32_t n = rec.n;
    float tau[TG];
#pragma unroll
    for (int j = 0; j < TG; ++j) tau[j] = t0 + j < a.T ? a.taps[t0 + j] : 0.0f;

    // the lane's samples and their sign words, once, into the lane's own LDS places (k * 256 + lane: no two lanes share one, so no
    // barrier stands between this loop and the next).  Held in registers instead, the 16 samples had to be 16 unrolled copies of both
    // loops, which the scheduler interleaved into 436 (TG = 8) and 512 registers + scratch (TG = 16).
    const uint32_t i0 = uint32_t(slice) * uint32_t(TRK_BANK_SLICE) + uint32_t(tid);      // n < 2^31: no wrap
    const uint64_t base = a.linear ? 0 : rec.st.next_sample_index;
#pragma unroll 1
    for (int k = 0; k < TRK_BANK_NS; ++k) {
        const uint32_t i = i0 + 256u * uint32_t(k);
        cf x = cf_make(0.0f, 0.0f);
        if (i < n) x = a.base[(base + i) & a.mask];
        xs[k * 256 + tid] = x;
        sgs[k * 256 + tid] = uint16_t(bank_signs<TG, FASTC>(ec, chips, i, tau));
    }

    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll 1
    for (int f = 0; f < a.F; ++f) {
        EpochConsts ef = ec;
        ef.two_pi_f = 2.0f * GM_PI_F * (rec.st.carrier_freq + a.offs[f]);      // (2.0*PI) * f_f
        const bool fast = FASTC && fast_car_ok(ef, float(n));                  // = fast_code_range of the epoch at f_f
        float acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.0f;
#pragma unroll 2
        for (int k = 0; k < TRK_BANK_NS; ++k) {
            const uint32_t i = i0 + 256u * uint32_t(k);
            const cf x = xs[k * 256 + tid];
            const uint32_t sg = sgs[k * 256 + tid];
            const float w = ef.two_pi_f * float(i);
            const float phase = ef.carrier_phase + (fast ? div_by_fs(w, ef.fs, ef.inv_fs) : __fdiv_rn(w, ef.fs));
            float sn, cs;
            if (ef.strict) sincosf_glibc(phase, sn, cs);
            else sincos_f32_via_f64(phase, sn, cs);
            const float wc = cs, ws = -sn;                          // Complex32::new(cos_p, -sin)
            float yr = x.x * wc - x.y * ws;                         // num-complex Mul
            float yi = x.x * ws + x.y * wc;
            if (!(i < n)) { yr = 0.0f; yi = 0.0f; }                 // past the epoch's end: nothing is added
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                const uint32_t s = (sg >> j) << 31;
                acc[2 * j] += __uint_as_float(__float_as_uint(yr) ^ s);
                acc[2 * j + 1] += __uint_as_float(__float_as_uint(yi) ^ s);
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[v] += __shfl_xor(acc[v], off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) wsum[f][wave][v] = acc[v];
        }
    }
    __syncthreads();
    // F * NV <= 8 * 32 = 256 words: one per lane
    float* pout = a.partials + (size_t(rec.poff) + size_t(slice)) * size_t(a.F) * size_t(a.T) * 2;
    for (int o = tid; o < a.F * NV; o += 256) {
        const int f = o / NV, v = o % NV, t = t0 + (v >> 1);
        if (t < a.T) pout[(size_t(f) * a.T + t) * 2 + (v & 1)] = ((wsum[f][0][v] + wsum[f][1][v]) + wsum[f][2][v]) + wsum[f][3][v];
    }
}

template <int TG>
__global__ __launch_bounds__(256) void trk_bank_kernel(TrkDevCfg cfg, const int8_t* __restrict__ codes, TrkBankArgs a) {
    const TrkBankRec rec = a.recs[blockIdx.y];
    if (!rec.run || blockIdx.x >= rec.slices) return;           // uniform over the workgroup
    extern __shared__ int8_t chips[];   // code_len chips of this record's row (row checked on the host)
    __shared__ cf xs[TRK_BANK_SLICE];                           // the slice's samples, [k][lane]
    __shared__ uint16_t sgs[TRK_BANK_SLICE];                    // and their TG sign bits
    __shared__ float wsum[GM_TRK_BANK_MAX_OFFSETS][4][2 * TG];  // [offset][wave][sum]
    const int8_t* crow = codes + size_t(code_row(cfg, rec.st)) * cfg.code_len;
    for (int i = threadIdx.x; i < cfg.code_len; i += 256) chips[i] = crow[i];
    __syncthreads();
    const EpochConsts ec = epoch_consts(cfg, rec.st);
    if (fast_code_ok(ec, rec.n)) trk_bank_body<TG, true>(cfg, a, rec, ec, chips, xs, sgs, wsum);
    else trk_bank_body<TG, false>(cfg, a, rec, ec, chips, xs, sgs, wsum);
}

__global__ __launch_bounds__(256) void trk_bank_sum_kernel(TrkBankArgs a, float* __restrict__ out, uint8_t* __restrict__ done) {
    const TrkBankRec rec = a.recs[blockIdx.x];
    const size_t W = size_t(a.F) * size_t(a.T) * 2;
    const float* p = a.partials + size_t(rec.poff) * W;
    for (size_t w = threadIdx.x; w < W; w += 256) {
        float s = 0.0f;
        if (rec.run) {
            s = p[w];
            for (uint32_t sl = 1; sl < rec.slices; ++sl) s += p[size_t(sl) * W + w];      // ascending slices
        }
        out[size_t(blockIdx.x) * W + w] = s;
    }
    if (threadIdx.x == 0) done[blockIdx.x] = rec.run ? 1 : 0;
}

int trk_bank_tap_group(int n_taps) { return n_taps <= 1 ? 1 : n_taps <= 4 ? 4 : n_taps <= 8 ? 8 : 16; }

void launch_trk_bank(hipStream_t st, const TrkDevCfg& cfg, const int8_t* d_codes, const TrkBankArgs& a, int n_records,
                     uint32_t max_slices, gm_c32* d_out, uint8_t* d_done) {
    const int tg = trk_bank_tap_group(a.T);
    const dim3 grid(max_slices, n_records, (a.T + tg - 1) / tg);
    const size_t lds = size_t(cfg.code_len);
    if (max_slices) {           // (no record runs: the sum kernel writes the zeros)
        switch (tg) {
            case 1: hipLaunchKernelGGL(trk_bank_kernel<1>, grid, dim3(256), lds, st, cfg, d_codes, a); break;
            case 4: hipLaunchKernelGGL(trk_bank_kernel<4>, grid, dim3(256), lds, st, cfg, d_codes, a); break;
            case 8: hipLaunchKernelGGL(trk_bank_kernel<8>, grid, dim3(256), lds, st, cfg, d_codes, a); break;
            default: hipLaunchKernelGGL(trk_bank_kernel<16>, grid, dim3(256), lds, st, cfg, d_codes, a); break;
        }
    }
    hipLaunchKernelGGL(trk_bank_sum_kernel, dim3(n_records), dim3(256), 0, st, a, reinterpret_cast<float*>(d_out), d_done);
}
