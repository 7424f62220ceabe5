// ddc_kernels.hip — real-IF int8 down-conversion to complex baseband (gm_ddc; gnss_mi355x.h states the definition): blank, mix by an
// exact integer NCO, then the rate converter's centred polyphase filter (the same positions, the same tap loop).
//
// ddc_kernel: one 256-lane workgroup per tile of outputs, tiles sized by resample_tile_out.  The tile's input span (at most RS_SPAN_MAX
//   bytes) goes into LDS as bytes first: 16-byte loads over the part of the call's input that allows them (the input may start at any
//   byte address: up to 15 head bytes and 15 tail bytes are single loads, and the LDS image is shifted so that the 16-byte stores are
//   aligned too), single bytes from the history in front of the call, zeros before the stream.  Then lane l takes span samples l,
//   l + 256, ...: adjacent lanes read adjacent LDS bytes and write adjacent float pairs.  Each sample is blanked and multiplied by its
//   phasor ONCE: sample n of the stream has phase (n * inc) mod 2^64, formed as (n0 + l) * inc + k * (256 * inc) in wrapping 64-bit
//   integers — the same value whatever the tile, since the arithmetic is that of a ring — and the phasor is the product of two table
//   words, each operation rounded on its own (-ffp-contract=off).  The two 32 KB tables are gathered from L2: a tile does 4096
//   lookups in each, so staging a table in LDS would read as many bytes as the lookups it serves and halve the resident workgroups.
// ddc_state_kernel: workgroup 0 writes the next history (the last T blanked input BYTES: from this call's input, or carried forward
//   when the call is shorter than T) into the OTHER history buffer; with blanking on, all workgroups count the blanked inputs of the
//   call, each input once, with integer adds only.  The phase needs no state: it is a function of the absolute index.
#include "gm_internal.h"

namespace gm {

namespace {
constexpr int RS_LANES = 256;

// ---- the rate converter's positions and tap loop (resample_kernels.hip), restated: the same integers, the same operations in
// the same order.  (Sharing them through a header changed resample_kernel's register allocation, 88 -> 98 VGPRs in the blended
// four-output form, below its five waves per SIMD; the rate converter's file is left as it is.)
// output k of the call (absolute index m = a0 * up + mr0 + k): its first-tap anchor i0 relative to the call's first input, the table
// row and the blend weight.  m' * down < 2^48 and r * PHI < 2^34: no product reaches 2^63.
__device__ __forceinline__ void rs_pos(const DdcArgs& a, uint64_t k, int64_t& rel, uint32_t& phi, float& alpha) {
    const uint64_t t = a.mr0 + k;
    const uint64_t aa = a.a0 + t / a.up, mp = t % a.up;
    const uint64_t p = mp * a.down;
    const uint64_t i0 = aa * a.down + p / a.up;
    const uint64_t q = (p % a.up) * a.PHI;
    phi = uint32_t(q / a.up);
    alpha = float(double(q % a.up) / double(a.up));
    rel = int64_t(i0 - a.in_index);
}

// the tile's first input relative to the call's first (negative: history) and how many inputs it spans (<= RS_SPAN_MAX by
// resample_tile_out); the tile is outputs k0 .. kend - 1 of the call
__device__ __forceinline__ void rs_tile_span(const DdcArgs& a, uint64_t k0, uint64_t kend, int64_t& lo, int& span) {
    const int half = int(a.T) / 2;
    int64_t rel_first, rel_last;
    uint32_t ph; float al;
    rs_pos(a, k0, rel_first, ph, al);
    rs_pos(a, kend - 1, rel_last, ph, al);
    lo = rel_first - (half - 1);
    const int64_t span64 = rel_last + half - lo + 1;
    span = int(span64 < int64_t(RS_SPAN_MAX) ? span64 : int64_t(RS_SPAN_MAX));
}

// lane tid's OPL outputs (tile outputs tid, tid + 256, ...: adjacent lanes store adjacent words) from the span in s_x: T dependent fused
// multiply-adds per output and component, j ascending, from +0; table rows by 16-byte loads; BLEND = false: the second row is not read
template <bool BLEND, int OPL>
__device__ __forceinline__ void rs_tile_outputs(const DdcArgs& a, const float2* s_x, int64_t lo, uint64_t k0, uint64_t kend, int tid) {
    const int T = int(a.T), half = T / 2;
    int xo[OPL];
    const float4* g[OPL];
    float al[OPL];
    bool ok[OPL];
#pragma unroll
    for (int o = 0; o < OPL; ++o) {
        const uint64_t k = k0 + uint64_t(tid) + uint64_t(o) * RS_LANES;
        ok[o] = k < kend;
        xo[o] = 0; al[o] = 0.0f; g[o] = reinterpret_cast<const float4*>(a.table);
        if (ok[o]) {
            int64_t rel; uint32_t phi;
            rs_pos(a, k, rel, phi, al[o]);
            int x = int(rel - (half - 1) - lo);
            x = x < 0 ? 0 : (x > RS_SPAN_MAX - T ? RS_SPAN_MAX - T : x);      // in [0, span - T] by construction; the clamp keeps LDS reads in bounds whatever happens
            xo[o] = x;
            g[o] = reinterpret_cast<const float4*>(a.table + size_t(phi) * T);
        }
    }
    float2 acc[OPL];
#pragma unroll
    for (int o = 0; o < OPL; ++o) { acc[o].x = 0.0f; acc[o].y = 0.0f; }
    const int T4 = T / 4;
#pragma unroll 2
    for (int j4 = 0; j4 < T4; ++j4) {
#pragma unroll
        for (int o = 0; o < OPL; ++o) {
            float4 c = g[o][j4];
            if (BLEND) {
                const float4 g1 = g[o][T4 + j4];
                c.x = __builtin_fmaf(al[o], g1.x - c.x, c.x);
                c.y = __builtin_fmaf(al[o], g1.y - c.y, c.y);
                c.z = __builtin_fmaf(al[o], g1.z - c.z, c.z);
                c.w = __builtin_fmaf(al[o], g1.w - c.w, c.w);
            }
            const float2* x = s_x + xo[o] + 4 * j4;
            const float2 x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
            acc[o].x = __builtin_fmaf(c.x, x0.x, acc[o].x); acc[o].y = __builtin_fmaf(c.x, x0.y, acc[o].y);
            acc[o].x = __builtin_fmaf(c.y, x1.x, acc[o].x); acc[o].y = __builtin_fmaf(c.y, x1.y, acc[o].y);
            acc[o].x = __builtin_fmaf(c.z, x2.x, acc[o].x); acc[o].y = __builtin_fmaf(c.z, x2.y, acc[o].y);
            acc[o].x = __builtin_fmaf(c.w, x3.x, acc[o].x); acc[o].y = __builtin_fmaf(c.w, x3.y, acc[o].y);
        }
    }
#pragma unroll
    for (int o = 0; o < OPL; ++o) {
        if (ok[o]) {
            const uint64_t k = k0 + uint64_t(tid) + uint64_t(o) * RS_LANES;
            reinterpret_cast<float2*>(a.out)[(a.out_start + k) & a.out_mask] = acc[o];
        }
    }
}

// ---- the down-converter
__device__ __forceinline__ float ddc_blank(const DdcArgs& a, int8_t raw, bool& blanked) {
    float x = float(raw);
    blanked = false;
    if (a.blank && x * x > a.thr2) { x = 0.0f; blanked = true; }
    return x;
}

template <bool BLEND, int OPL>
__global__ __launch_bounds__(RS_LANES) void ddc_kernel(DdcArgs a) {
    __shared__ __attribute__((aligned(16))) float2 s_x[RS_SPAN_MAX];
    __shared__ __attribute__((aligned(16))) int8_t s_raw[RS_SPAN_MAX + 16];
    const int tid = threadIdx.x;
    const int T = int(a.T);
    const uint64_t k0 = uint64_t(blockIdx.x) * a.tile_out;
    const uint64_t kend = k0 + a.tile_out < a.n_out ? k0 + a.tile_out : a.n_out;
    int64_t lo;                                              // the tile's first input, relative to the call's first (negative: history)
    int span;
    rs_tile_span(a, k0, kend, lo, span);

    // span samples [i0, i1) lie in the call's input, from byte address pb on: head single bytes, nbody 16-byte words, the rest single bytes
    const int i0 = lo < 0 ? int(-lo < int64_t(span) ? -lo : int64_t(span)) : 0;
    const int64_t end64 = int64_t(a.n_in) - lo;
    int i1 = end64 < int64_t(span) ? int(end64) : span;
    i1 = i1 < i0 ? i0 : i1;
    const int len = i1 - i0;
    const int8_t* pb = a.in + (lo + i0);
    const int to16 = int((16u - unsigned(reinterpret_cast<uintptr_t>(pb) & 15u)) & 15u);
    const int head = to16 < len ? to16 : len;
    const int nbody = (len - head) / 16;
    const int b0 = i0 + head, b1 = b0 + 16 * nbody;
    const int sh = (16 - (b0 & 15)) & 15;                    // s_raw[sh + i] holds span sample i: sh + b0 is a multiple of 16
    for (int i = tid; i < span; i += RS_LANES) {
        if (i >= b0 && i < b1) continue;
        const int64_t s = lo + i;
        int8_t v = 0;
        if (s < 0) {
            const int64_t h = int64_t(T) + s;                // history byte T - 1 is the input just before the call
            if (h >= 0) v = a.hist_in[h];
        } else if (uint64_t(s) < a.n_in) v = a.in[s];
        s_raw[sh + i] = v;
    }
    for (int w = tid; w < nbody; w += RS_LANES)
        *reinterpret_cast<uint4*>(s_raw + sh + b0 + 16 * w) = *reinterpret_cast<const uint4*>(pb + head + 16 * w);
    __syncthreads();

    const uint64_t n0 = a.in_index + uint64_t(lo);           // absolute index of span sample 0 (wraps below the stream's start, where the samples are zero)
    uint64_t th = (n0 + uint64_t(tid)) * a.inc;
    const uint64_t step = a.inc * uint64_t(RS_LANES);
    const float2* whi = reinterpret_cast<const float2*>(a.whi);
    const float2* wlo = reinterpret_cast<const float2*>(a.wlo);
    for (int i = tid; i < span; i += RS_LANES, th += step) {
        bool b;
        const float x = ddc_blank(a, s_raw[sh + i], b);      // a history byte is blanked already: 0 stays 0
        const uint32_t k = uint32_t(th >> 40);
        const float2 wa = whi[k >> 12], wb = wlo[k & 4095u];
        const float re = wa.x * wb.x - wa.y * wb.y;          // each product and sum rounded on its own
        const float im = wa.x * wb.y + wa.y * wb.x;
        float2 p; p.x = x * re; p.y = x * im;
        s_x[i] = p;
    }
    __syncthreads();

    rs_tile_outputs<BLEND, OPL>(a, s_x, lo, k0, kend, tid);
}

__global__ __launch_bounds__(RS_LANES) void ddc_state_kernel(DdcArgs a) {
    const int tid = threadIdx.x;
    const int T = int(a.T);
    if (a.blank) {
        unsigned long long cnt = 0;
        const uint64_t stride = uint64_t(gridDim.x) * RS_LANES;
        for (uint64_t i = uint64_t(blockIdx.x) * RS_LANES + tid; i < a.n_in; i += stride) {
            bool b;
            (void)ddc_blank(a, a.in[i], b);
            cnt += b ? 1ull : 0ull;
        }
        for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if ((tid & 63) == 0 && cnt) atomicAdd(a.blanked, cnt);
    }
    if (blockIdx.x == 0 && tid < T) {
        const uint64_t k = uint64_t(tid) + a.n_in;            // byte tid of the new history is byte tid + n_in of (old history | input)
        int8_t v;
        if (k < uint64_t(T)) v = a.hist_in[k];
        else {
            bool b;
            v = a.in[k - uint64_t(T)];
            (void)ddc_blank(a, v, b);
            if (b) v = 0;
        }
        a.hist_out[tid] = v;
    }
}

template <bool BLEND>
void launch_out(hipStream_t s, const DdcArgs& a) {
    const unsigned tiles = unsigned((a.n_out + a.tile_out - 1) / a.tile_out);
    if (a.tile_out > 512) ddc_kernel<BLEND, 4><<<tiles, RS_LANES, 0, s>>>(a);
    else if (a.tile_out > 256) ddc_kernel<BLEND, 2><<<tiles, RS_LANES, 0, s>>>(a);
    else ddc_kernel<BLEND, 1><<<tiles, RS_LANES, 0, s>>>(a);
}
}  // namespace

// n_in > 0 (the caller has checked every argument)
void launch_ddc(hipStream_t s, const DdcArgs& a) {
    if (a.n_out) {
        if (a.PHI % a.up != 0) launch_out<true>(s, a); else launch_out<false>(s, a);
    }
    // the count reads every input once: a workgroup per 2048 inputs, at most 1024 of them; without blanking one workgroup (the history)
    uint64_t blocks = a.blank ? (a.n_in + 2047) / 2048 : 1;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    ddc_state_kernel<<<unsigned(blocks), RS_LANES, 0, s>>>(a);
}

}  // namespace gm
