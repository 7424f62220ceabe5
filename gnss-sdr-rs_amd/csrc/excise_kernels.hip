// excise_kernels.hip — FFT-domain narrowband interference excision (gm_excisor; gnss_mi355x.h states the definition): a 50 % overlap-add
// filter bank with sine windows and a per-bin gain, on fft_core.h's in-LDS transforms of B = 256 .. 4096.
//
// excise_kernel: one workgroup of Plan::T lanes per tile of G consecutive output segments (half blocks).  It runs blocks s0 .. s0 + G in
//   turn: the forward transform on the plan of B, whose pass-0 loads convert, blank and window the inputs (from the call's input or, in
//   front of it, from the history buffer); the gain multiply on the forward's last-pass registers (lane b holds bins b + r * NB(last));
//   the inverse on the plan with the radices REVERSED, whose pass-0 inputs are exactly those registers — the spectrum never goes
//   through LDS or memory.  The inverse's last pass leaves lane b with samples b + q * NB'(last): q and q + RL/2 are i and i + H, so a
//   lane keeps the weighted second half of a block in registers and adds it to the weighted first half of the next block: a segment is
//   stored once both terms exist.  G + 1 transform pairs for G segments.  A block's words depend on its B inputs and the gains alone,
//   so neither G nor the cut of the stream into calls shows in the words.  LDS: one transform image + both twiddle sets (39 KB at
//   B = 4096: two workgroups a CU and more); the image's layout and its padding are fft_core.h's.  Windows and gains come from L2.
//   The block-adapt instantiation (ExciseArgs::block_adapt) decides a 0 / 1 mask per block between the two transforms, on the same
//   registers: power words, a truncated rank selection across the workgroup (15 counting rounds), the flags as a bit image in
//   LDS, the guard widening, integer counters; the mask multiplies the static gain.  The other instantiation is the kernel as it was.
// excise_state_kernel: workgroup 0 writes the next history (the last 3H blanked inputs) into the OTHER history buffer; with blanking on,
//   all workgroups count the blanked inputs of the call, each input once, with integer adds only.
// excise_psd_kernel: the forward half alone; workgroup c accumulates |X|^2 of blocks c C .. c C + C - 1, C = max(4, ceil(J / 512)), (j ascending, from +0) in registers
//   and stores its partial sums.  excise_mask_kernel (one workgroup): adds the partial sums with c ascending, finds the element of rank
//   (B - 1) div 2 by a bitwise search over the words (32 counting steps of one barrier each, the words in registers: non-negative
//   floats order as their bit patterns), flags
//   P[k] > factor * med, widens the flags by the guard (circular) and writes the gains and the counts.  No floating-point atomics.
// Compiled with -ffp-contract=off: every product and sum below rounds on its own; the transforms call __builtin_fmaf explicitly.
#include "acq_device.h"
#include "excise_core.h"

namespace gm {

namespace {
template <int FMT>
__device__ __forceinline__ cf ex_load(const void* in, uint64_t i, float thr2, int blank, bool& blanked) {
    cf v;
    if (FMT == GM_FMT_C32) v = reinterpret_cast<const cf*>(in)[i];
    else {   // GM_FMT_I8_IQ
        const char2 c = reinterpret_cast<const char2*>(in)[i];
        v.x = float(c.x); v.y = float(c.y);
    }
    blanked = false;
    if (blank) {
        const float p = v.x * v.x + v.y * v.y;
        if (p > thr2) { v.x = 0.0f; v.y = 0.0f; blanked = true; }
    }
    return v;
}

// the forward transform of one block; in(i) yields windowed input i; the outputs stay in registers: X[it][r] is bin (tid + it T) + r NB(last)
template <class PL, class In>
__device__ __forceinline__ void ex_forward(cf (&X)[PL::ITL][PL::RL], In&& in, cf* lds, const cf* twf, int tid) {
    constexpr int NB0 = PL::NB(0);
    {
        cf v0[PL::IT0][PL::R0];
        Fft<PL, false>::pass0_stage1(v0, [&](int it, int r) { return in((tid + it * PL::T) + r * NB0); }, tid);
        __syncthreads();                                    // the image's last readers (the previous transform) are done
        Fft<PL, false>::pass0_stage2(v0, lds, tid);
    }
    __syncthreads();
    MiddlePasses<PL, false, 1>::run(lds, twf, tid);
    cf vl[PL::ITL][PL::RL];
    Fft<PL, false>::last_stage1(vl, lds, twf, tid);
    Fft<PL, false>::last_stage2(vl, [&](int it, int q, cf val) { X[it][q] = val; }, tid);
}

// The sum of v over the wave's 64 lanes, in every lane: the row-shift / row-broadcast DPP ladder (partial sums of 4, 8 and 16 lanes within
// a row of 16, then rows 0 + 1 and 2 + 3, then both halves), whose total lands in lane 63.  Lanes a step does not write add 0.
// Integers: the order of the adds is not in the result.
__device__ __forceinline__ uint32_t ex_wave_sum(uint32_t v) {
    const int v0 = int(v);
    int t = v0 + __builtin_amdgcn_update_dpp(0, v0, 0x111, 0xf, 0xf, false)      // row_shr:1
               + __builtin_amdgcn_update_dpp(0, v0, 0x112, 0xf, 0xf, false)      // row_shr:2
               + __builtin_amdgcn_update_dpp(0, v0, 0x113, 0xf, 0xf, false);     // row_shr:3
    t += __builtin_amdgcn_update_dpp(0, t, 0x114, 0xf, 0xe, false);              // row_shr:4, banks 1 .. 3
    t += __builtin_amdgcn_update_dpp(0, t, 0x118, 0xf, 0xc, false);              // row_shr:8, banks 2 and 3: lane 15 of a row holds the row
    t += __builtin_amdgcn_update_dpp(0, t, 0x142, 0xa, 0xf, false);              // row_bcast:15 into rows 1 and 3
    t += __builtin_amdgcn_update_dpp(0, t, 0x143, 0xc, 0xf, false);              // row_bcast:31 into rows 2 and 3: lane 63 holds the wave
    return uint32_t(__builtin_amdgcn_readlane(t, 63));
}

// The block-adapt decision of one block, on the forward's last-pass registers (gnss_mi355x.h, "Block-adapt mode"; the rule's lane-local
// parts are excise_core.h's).  -> zero[it], bit r set where bin (tid + it T) + r NBL is zeroed (m = 0).  Lanes with a butterfly b >= NBL hold no bins.
//   1. p = re*re + im*im of the lane's bins, kept as words.
//   2. 15 rounds over bits 30 .. 16: a lane counts its own words below the candidate, ex_wave_sum adds the lanes; where more than one
//      wave holds bins (B >= 2048) the waves' counts go through one of two LDS rows in turn, so a round costs one barrier (as in
//      excise_mask_kernel).  Measured on a 2^19-sample call (B = 1024 / 4096, the whole step, mode off 0.0144 / 0.0254 ms): a ballot
//      and a scalar popcount per word and round 0.0351 / 0.0445 ms, of which the rounds were 0.0125 / 0.0120 ms; three bits a round
//      with 7 such ballots per word 0.0509 / 0.0659 ms — the ballots, not the exchange, were the cost; the count in the lanes with
//      one wave sum a round 0.0289 / 0.0424 ms, which is what is built.  LDS integer histograms were not measured.
//   3. The flags go into LDS as a bit image (a ballot is 64 — or NBL — consecutive bins of one r), with a word per wave that says
//      whether it flagged; one barrier; every lane widens its own bins by the guard from three words of the image.
// The LDS rows are written again only behind the barriers of the inverse transform that follows.  any_flag is the block's (the same in
// every lane); lane_nf and lane_nz are THIS LANE's flagged and zeroed bins: the kernel adds them up over its tile and sums the lanes once.
template <class PL>
struct ExBlockLds {
    static constexpr int W = (PL::T + 63) / 64;
    uint32_t bits[PL::N / 32];
    uint32_t round[2][W];
    uint32_t any[W];
};

template <class PL>
__device__ __forceinline__ void ex_block_decide(uint32_t (&zero)[PL::ITL], const cf (&X)[PL::ITL][PL::RL], float factor, int guard,
                                                float* cap_p, unsigned char* cap_m, bool& any_flag, uint32_t& lane_nf, uint32_t& lane_nz,
                                                int tid) {
    __shared__ ExBlockLds<PL> s;                                          // (only the block-adapt instantiations have it)
    constexpr int B = PL::N, T = PL::T, NBL = PL::NB(PL::NP - 1), W = ExBlockLds<PL>::W;
    constexpr int VW = (NBL + 63) / 64;                                   // the waves that hold bins
    constexpr int NV = NBL < 64 ? NBL : 64;                               // valid lanes of a ballot: bins b0 + r NBL .. + NV - 1
    static_assert(NV % 16 == 0 && (NBL % 64 == 0 || PL::ITL == 1), "a ballot is a run of 16-bit pieces of the bit image");
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t w[PL::ITL][PL::RL];
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it)
#pragma unroll
        for (int r = 0; r < PL::RL; ++r) {
            const float p = ex_power(X[it][r]);
            w[it][r] = ex_word(p);
            if (cap_p && tid + it * T < NBL) cap_p[(tid + it * T) + r * NBL] = p;
        }
    const uint32_t rank = uint32_t(B - 1) / 2;
    uint32_t med = 0;
    for (int bit = EX_SEL_TOP_BIT; bit >= EX_SEL_LOW_BIT; --bit) {
        const uint32_t cand = ex_sel_cand(med, bit);
        uint32_t cnt = 0;
#pragma unroll
        for (int it = 0; it < PL::ITL; ++it)
#pragma unroll
            for (int r = 0; r < PL::RL; ++r) cnt += tid + it * T < NBL && ex_sel_below(w[it][r], cand) ? 1u : 0u;
        uint32_t total = ex_wave_sum(cnt);
        if (VW > 1) {                                                     // (one wave holds every bin up to B = 1024)
            uint32_t* row = s.round[bit & 1];
            if (lane == 0) row[wave] = total;
            __syncthreads();
            total = 0;
#pragma unroll
            for (int v = 0; v < VW; ++v) total += row[v];
        }
        med = ex_sel_step(med, cand, total, rank);
    }
    const float medf = ex_float(med);
    uint16_t* bits16 = reinterpret_cast<uint16_t*>(s.bits);               // little-endian: piece c of the image is bits 16 c .. 16 c + 15
    lane_nf = 0;
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it) {
        const int b0 = (tid - lane) + it * T;                             // the wave's first butterfly
#pragma unroll
        for (int r = 0; r < PL::RL; ++r) {
            const bool f = tid + it * T < NBL && ex_flag(ex_float(w[it][r]), factor, medf);
            const unsigned long long bal = __ballot(f);
            lane_nf += f ? 1u : 0u;
            if (b0 < NBL && lane < NV / 16) bits16[(b0 + r * NBL) / 16 + lane] = uint16_t(bal >> (16 * lane));
        }
    }
    const bool wave_any = __ballot(lane_nf != 0) != 0;
    if (lane == 0) s.any[wave] = wave_any ? 1u : 0u;
    __syncthreads();
    uint32_t n_any = 0;
#pragma unroll
    for (int v = 0; v < W; ++v) n_any += s.any[v];
    any_flag = n_any != 0;
    lane_nz = 0;
    static_assert(PL::RL <= 32, "a lane's zeroed bins fit one word");
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it) {
        zero[it] = 0;
#pragma unroll
        for (int r = 0; r < PL::RL; ++r) {
            const int b = tid + it * T, k = b + r * NBL;
            const bool z = b < NBL && any_flag && ex_zeroed(s.bits, k, guard, B);
            lane_nz += z ? 1u : 0u;
            zero[it] |= z ? 1u << r : 0u;
            if (cap_m && b < NBL) cap_m[k] = z ? 0 : 1;
        }
    }
}

template <class PL, int FMT, bool ADAPT>
__global__ __launch_bounds__(PL::T) void excise_kernel(ExciseArgs a) {
    using MAP = ExciseMap<PL>;                                             // excise_core.h: the index maps, checked on the CPU
    using RP = typename MAP::RP;
    constexpr int H = MAP::H, T = MAP::T, NBL = MAP::NBL, RNBL = MAP::RNBL, RRL = MAP::RRL, HQ = MAP::HQ, LE = MAP::LDS_ELEMS;
    __shared__ cf lds[LE + PL::TW_TOTAL + RP::TW_TOTAL];
    uint32_t c_blocks = 0, c_bflag = 0, c_flag = 0, c_zero = 0;             // the tile's counts: blocks (the same in every lane), this lane's bins
    cf* twf = lds + LE;
    cf* twi = twf + PL::TW_TOTAL;
    const int tid = threadIdx.x;
    load_twiddles<PL>(twf, a.tw_fwd, tid);
    load_twiddles<RP>(twi, a.tw_inv, tid);
    const uint32_t s0 = blockIdx.x * a.G;
    const uint32_t s1 = s0 + a.G < a.n_seg ? s0 + a.G : a.n_seg;           // segments s0 .. s1 - 1 of the call: blocks s0 .. s1
    const int64_t hist_len = 3 * H;
    cf prev[RP::ITL][HQ];                                                  // ws[i + H] * u[i + H] of the block before
    for (uint32_t j = s0; j <= s1; ++j) {
        const int64_t base = a.rel0 + int64_t(j) * H;                      // the block's first input, relative to the call's first (negative: history)
        cf X[PL::ITL][PL::RL];
        ex_forward<PL>(X, [&](int i) {
            const int64_t rel = base + i;
            cf v = cf_make(0.0f, 0.0f);
            if (rel < 0) {
                const int64_t h = hist_len + rel;                          // history word 3H - 1 is the input just before the call
                if (h >= 0) v = a.hist_in[h];
            } else if (uint64_t(rel) < a.n_in) {
                bool b;
                v = ex_load<FMT>(a.in, uint64_t(rel), a.thr2, a.blank, b);
            }
            const float w = a.wa[i];
            return cf_make(w * v.x, w * v.y);
        }, lds, twf, tid);
        uint32_t zero[PL::ITL];
        if constexpr (ADAPT) {
            bool any_flag;
            uint32_t lane_nf, lane_nz;
            ex_block_decide<PL>(zero, X, a.bfactor, int(a.bguard), a.cap_p ? a.cap_p + size_t(j) * PL::N : nullptr,
                                a.cap_m ? a.cap_m + size_t(j) * PL::N : nullptr, any_flag, lane_nf, lane_nz, tid);
            if (j > s0) {                                                  // block j is counted with segment j - 1, which this tile delivers
                c_flag += lane_nf; c_zero += lane_nz;
                c_blocks += 1; c_bflag += any_flag ? 1 : 0;
            }
        }
        cf u[RP::ITL][RRL];
        {
            cf v0[RP::IT0][RP::R0];
            Fft<RP, true>::pass0_stage1(v0, [&](int it, int r) {
                float g = a.gains[(tid + it * T) + r * NBL];
                if constexpr (ADAPT) g = g * ((zero[it] >> r) & 1u ? 0.0f : 1.0f);     // (g * m_b) first
                return cf_make(g * X[it][r].x, g * X[it][r].y);
            }, tid);
            __syncthreads();                                               // every lane has read the forward's last image
            Fft<RP, true>::pass0_stage2(v0, lds, tid);
        }
        __syncthreads();
        MiddlePasses<RP, true, 1>::run(lds, twi, tid);
        {
            cf vl[RP::ITL][RRL];
            Fft<RP, true>::last_stage1(vl, lds, twi, tid);
            Fft<RP, true>::last_stage2(vl, [&](int it, int q, cf val) { u[it][q] = val; }, tid);
        }
#pragma unroll
        for (int it = 0; it < RP::ITL; ++it) {
            const int b = tid + it * T;
            if (b < RNBL) {
#pragma unroll
                for (int q = 0; q < HQ; ++q) {
                    const int i = b + q * RNBL;                            // < H
                    if (j > s0) {
                        const float w = a.ws[i];
                        cf y;
                        y.x = prev[it][q].x + w * u[it][q].x;
                        y.y = prev[it][q].y + w * u[it][q].y;
                        a.out[(a.out_start + uint64_t(j - 1) * H + i) & a.out_mask] = y;
                    }
                    const float w2 = a.ws[i + H];
                    prev[it][q] = cf_make(w2 * u[it][q + HQ].x, w2 * u[it][q + HQ].y);
                }
            }
        }
    }
    if constexpr (ADAPT) {
        // integer adds only: any order gives the same counts.  One set of adds per workgroup, into the counter row of its slot: every
        // workgroup adding to ONE cache line cost several times the transforms (measured), the rows spread the adds over 64 lines
        __shared__ uint32_t s_cnt[2][(T + 63) / 64];
        const uint32_t wave_flag = ex_wave_sum(c_flag), wave_zero = ex_wave_sum(c_zero);
        if ((tid & 63) == 0) { s_cnt[0][tid >> 6] = wave_flag; s_cnt[1][tid >> 6] = wave_zero; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long n_flag = 0, n_zero = 0;
#pragma unroll
            for (int v = 0; v < (T + 63) / 64; ++v) { n_flag += s_cnt[0][v]; n_zero += s_cnt[1][v]; }
            unsigned long long* row = a.bstat + size_t(blockIdx.x % EX_BSTAT_SLOTS) * EX_BSTAT_STRIDE;
            if (c_blocks) atomicAdd(row + 0, (unsigned long long)c_blocks);
            if (c_bflag) atomicAdd(row + 1, (unsigned long long)c_bflag);
            if (n_flag) atomicAdd(row + 2, n_flag);
            if (n_zero) atomicAdd(row + 3, n_zero);
        }
    }
}

constexpr int EX_STATE_LANES = 256;

template <int FMT>
__global__ __launch_bounds__(EX_STATE_LANES) void excise_state_kernel(ExciseArgs a) {
    const int tid = threadIdx.x;
    const uint64_t L = 3ull * (a.B / 2);
    if (a.blank) {
        unsigned long long cnt = 0;
        const uint64_t stride = uint64_t(gridDim.x) * EX_STATE_LANES;
        for (uint64_t i = uint64_t(blockIdx.x) * EX_STATE_LANES + tid; i < a.n_in; i += stride) {
            bool b;
            (void)ex_load<FMT>(a.in, i, a.thr2, a.blank, b);
            cnt += b ? 1ull : 0ull;
        }
        for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if ((tid & 63) == 0 && cnt) atomicAdd(a.blanked, cnt);
    }
    if (blockIdx.x == 0) {
        for (uint64_t w = tid; w < L; w += EX_STATE_LANES) {
            const uint64_t k = w + a.n_in;                    // word w of the new history is word w + n_in of (old history | input)
            cf v;
            if (k < L) v = a.hist_in[k];
            else {
                bool b;
                v = ex_load<FMT>(a.in, k - L, a.thr2, a.blank, b);
            }
            a.hist_out[w] = v;
        }
    }
}

template <class PL, int FMT>
__global__ __launch_bounds__(PL::T) void excise_psd_kernel(ExcisePsdArgs a) {
    constexpr int N = PL::N, H = N / 2, T = PL::T, NBL = PL::NB(PL::NP - 1);
    __shared__ cf lds[PL::LDS_ELEMS + PL::TW_TOTAL];
    cf* twf = lds + PL::LDS_ELEMS;
    const int tid = threadIdx.x;
    load_twiddles<PL>(twf, a.tw_fwd, tid);
    const uint64_t j0 = uint64_t(blockIdx.x) * a.C;
    const uint64_t j1 = j0 + a.C < a.J ? j0 + a.C : a.J;
    float acc[PL::ITL][PL::RL];
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it)
#pragma unroll
        for (int r = 0; r < PL::RL; ++r) acc[it][r] = 0.0f;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t base = j * H;                                       // base + i < J H + H <= n
        cf X[PL::ITL][PL::RL];
        ex_forward<PL>(X, [&](int i) {
            bool b;
            const cf v = ex_load<FMT>(a.in, base + uint64_t(i), a.thr2, a.blank, b);
            const float w = a.wa[i];
            return cf_make(w * v.x, w * v.y);
        }, lds, twf, tid);
#pragma unroll
        for (int it = 0; it < PL::ITL; ++it)
#pragma unroll
            for (int r = 0; r < PL::RL; ++r) acc[it][r] = acc[it][r] + (X[it][r].x * X[it][r].x + X[it][r].y * X[it][r].y);
    }
    float* dst = a.partial + size_t(blockIdx.x) * N;
#pragma unroll
    for (int it = 0; it < PL::ITL; ++it) {
        const int b = tid + it * T;
        if (b < NBL) {
#pragma unroll
            for (int r = 0; r < PL::RL; ++r) dst[b + r * NBL] = acc[it][r];
        }
    }
}

constexpr int EX_MASK_LANES = 1024, EX_MASK_WAVES = EX_MASK_LANES / 64, EX_MASK_PER = EX_BLOCK_MAX / EX_MASK_LANES;

// the sum of v over the workgroup's lanes, in every lane (integers: any order gives the same words)
__device__ __forceinline__ unsigned ex_block_sum(unsigned v, unsigned* s_part, int tid) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();                                         // the last use's readers are done
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < EX_MASK_WAVES; ++w) t += s_part[w];
    return t;
}

// lane l owns bins l + e * 1024, e < 4 (those below B): its words stay in registers through the 32 rounds of the search
__global__ __launch_bounds__(EX_MASK_LANES) void excise_mask_kernel(ExciseMaskArgs a) {
    __shared__ unsigned char s_flag[EX_BLOCK_MAX];
    __shared__ unsigned s_part[EX_MASK_WAVES];
    __shared__ unsigned s_round[2][EX_MASK_WAVES];
    const int tid = threadIdx.x;
    const int B = int(a.B);
    float p[EX_MASK_PER];
#pragma unroll
    for (int e = 0; e < EX_MASK_PER; ++e) {
        const int k = tid + e * EX_MASK_LANES;
        float s = 0.0f;
        if (k < B) {
            const float* src = a.partial + k;
#pragma unroll 8
            for (uint32_t c = 0; c < a.n_chunks; ++c) s = s + src[size_t(c) * B];      // c ascending, from +0
            a.P[k] = s;
        }
        p[e] = s;
    }
    // the element of rank (B - 1) div 2: the largest word v with count(P < v) <= rank.  A wave's count comes from its ballots; the
    // waves' counts go through one of two LDS rows in turn, so a round needs one barrier (a wave can write row r & 1 again only
    // behind the barrier of round r + 1, which every wave reaches after it has read that row in round r)
    const unsigned rank = unsigned(B - 1) / 2;
    unsigned med_bits = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = med_bits | (1u << bit);
        unsigned cnt = 0;
#pragma unroll
        for (int e = 0; e < EX_MASK_PER; ++e) {
            const bool below = tid + e * EX_MASK_LANES < B && __float_as_uint(p[e]) < cand;
            cnt += unsigned(__popcll(__ballot(below)));
        }
        unsigned* row = s_round[bit & 1];
        if ((tid & 63) == 0) row[tid >> 6] = cnt;
        __syncthreads();
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < EX_MASK_WAVES; ++w) total += row[w];
        if (total <= rank) med_bits = cand;
    }
    const float med = __uint_as_float(med_bits);
    const float level = a.factor * med;
    unsigned n_flag = 0;
#pragma unroll
    for (int e = 0; e < EX_MASK_PER; ++e) {
        const int k = tid + e * EX_MASK_LANES;
        if (k < B) {
            const bool f = p[e] > level;
            s_flag[k] = f ? 1 : 0;
            n_flag += f ? 1u : 0u;
        }
    }
    n_flag = ex_block_sum(n_flag, s_part, tid);              // (its barriers also publish s_flag)
    const int guard = int(a.guard);
    unsigned n_zero = 0;
#pragma unroll
    for (int e = 0; e < EX_MASK_PER; ++e) {
        const int k = tid + e * EX_MASK_LANES;
        if (k < B) {
            bool z = false;
            for (int d = -guard; d <= guard; ++d) z = z || s_flag[(k + d + B) & (B - 1)];
            a.gains[k] = z ? 0.0f : 1.0f;
            n_zero += z ? 1u : 0u;
        }
    }
    n_zero = ex_block_sum(n_zero, s_part, tid);
    if (tid == 0) {
        a.stat[0] = med_bits;
        a.stat[1] = n_flag;
        a.stat[2] = n_zero;
    }
}

template <class PL>
void launch_excise_plan(hipStream_t s, const ExciseArgs& a, int fmt) {
    const unsigned tiles = (a.n_seg + a.G - 1) / a.G;
    if (a.block_adapt) {
        if (fmt == GM_FMT_C32) excise_kernel<PL, GM_FMT_C32, true><<<tiles, PL::T, 0, s>>>(a);
        else excise_kernel<PL, GM_FMT_I8_IQ, true><<<tiles, PL::T, 0, s>>>(a);
    } else if (fmt == GM_FMT_C32) excise_kernel<PL, GM_FMT_C32, false><<<tiles, PL::T, 0, s>>>(a);
    else excise_kernel<PL, GM_FMT_I8_IQ, false><<<tiles, PL::T, 0, s>>>(a);
}
template <class PL>
void launch_psd_plan(hipStream_t s, const ExcisePsdArgs& a, int fmt) {
    if (fmt == GM_FMT_C32) excise_psd_kernel<PL, GM_FMT_C32><<<a.n_chunks, PL::T, 0, s>>>(a);
    else excise_psd_kernel<PL, GM_FMT_I8_IQ><<<a.n_chunks, PL::T, 0, s>>>(a);
}
template <class PL>
int fill_both(cf* fwd, cf* inv, int* n_fwd, int* n_inv) {
    using RP = typename RevPlan<PL>::type;
    static_assert(PL::TW_TOTAL <= EX_TW_MAX && RP::TW_TOTAL <= EX_TW_MAX, "twiddle sets fit the handle's buffers");
    fill_twiddles<PL>(fwd, false, [](double x) { return ::cos(x); }, [](double x) { return ::sin(x); });
    fill_twiddles<RP>(inv, true, [](double x) { return ::cos(x); }, [](double x) { return ::sin(x); });
    *n_fwd = PL::TW_TOTAL; *n_inv = RP::TW_TOTAL;
    return 0;
}
}  // namespace

#define EX_DISPATCH(B, CALL)                  \
    switch (B) {                              \
        case 256: CALL(Plan256); break;       \
        case 512: CALL(Plan512); break;       \
        case 1024: CALL(Plan1024); break;     \
        case 2048: CALL(Plan2048); break;     \
        case 4096: CALL(Plan4096); break;     \
        default: break;                       \
    }

// the forward base twiddles of the plan of B and the inverse ones of the plan with its radices reversed (at most EX_TW_MAX words each)
int excise_twiddles(uint32_t B, cf* fwd, cf* inv, int* n_fwd, int* n_inv) {
    int rc = -1;
#define EX_CALL(PL) rc = fill_both<PL>(fwd, inv, n_fwd, n_inv)
    EX_DISPATCH(B, EX_CALL)
#undef EX_CALL
    return rc;
}

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, B one of the five sizes (the caller has checked); n_in > 0
void launch_excise(hipStream_t s, const ExciseArgs& a, int fmt) {
    if (a.n_seg) {
#define EX_CALL(PL) launch_excise_plan<PL>(s, a, fmt)
        EX_DISPATCH(a.B, EX_CALL)
#undef EX_CALL
    }
    // the count reads every input once: a workgroup per 2048 inputs, at most 1024 of them; without blanking one workgroup (the history)
    uint64_t blocks = a.blank ? (a.n_in + 2047) / 2048 : 1;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    if (fmt == GM_FMT_C32) excise_state_kernel<GM_FMT_C32><<<unsigned(blocks), EX_STATE_LANES, 0, s>>>(a);
    else excise_state_kernel<GM_FMT_I8_IQ><<<unsigned(blocks), EX_STATE_LANES, 0, s>>>(a);
}

void launch_excise_adapt(hipStream_t s, const ExcisePsdArgs& p, const ExciseMaskArgs& m, int fmt) {
#define EX_CALL(PL) launch_psd_plan<PL>(s, p, fmt)
    EX_DISPATCH(p.B, EX_CALL)
#undef EX_CALL
    excise_mask_kernel<<<1, EX_MASK_LANES, 0, s>>>(m);
}

}  // namespace gm
