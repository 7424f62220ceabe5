// resample_kernels.hip — polyphase rate conversion and pulse blanking (gm_resampler; gnss_mi355x.h states the definition): the two
// stages rf::frontend::DigitalFrontend::process_block names in comments and leaves out (src/rf/frontend.rs).
//
// resample_kernel: one 256-lane workgroup per tile of outputs.  The tile's input span (tile * down / up + T samples, at most
//   RS_SPAN_MAX by the choice of the tile) is converted and blanked ONCE into LDS as float pairs — from the call's input, or, in front
//   of it, from the history buffer — so every input leaves HBM once plus the halo.  A lane owns OPL = 4, 2 or 1 outputs (lane l: tile
//   outputs l, l + 256, ...: adjacent lanes store adjacent words), whose T dependent fused multiply-adds run side by side.  Table rows
//   are fetched with 16-byte loads (rows are T * 4 bytes, T a multiple of 8: every row is 32-byte aligned); the table is at most 1 MB
//   and stays in L2.  BLEND = false when `up` divides PHI: alpha is then exactly 0 for every output, fmaf(0, d, g) = g, and the second
//   row is not fetched — the same words (a zero coefficient's sign cannot reach the sum: it starts at +0 and never becomes -0).
//   The T terms are added with j ascending for every output, whatever tile, lane or call it falls into.
// resample_state_kernel: workgroup 0 writes the next history (the last T blanked inputs: from this call's input, or carried forward
//   from the old history when the call is shorter than T) into the OTHER history buffer; with blanking on, all workgroups count the
//   blanked inputs of the call, each input once, with integer adds only.
// Compiled with -ffp-contract=off: re*re + im*im rounds three times, every fused operation is written as __builtin_fmaf.
#include "gm_internal.h"

namespace gm {

namespace {
constexpr int RS_LANES = 256;

template <int FMT>
__device__ __forceinline__ float2 rs_load(const ResampleArgs& a, uint64_t i, bool& blanked) {
    float2 v;
    if (FMT == GM_FMT_C32) v = reinterpret_cast<const float2*>(a.in)[i];
    else {   // GM_FMT_I8_IQ
        const char2 c = reinterpret_cast<const char2*>(a.in)[i];
        v.x = float(c.x); v.y = float(c.y);
    }
    blanked = false;
    if (a.blank) {
        const float p = v.x * v.x + v.y * v.y;
        if (p > a.thr2) { v.x = 0.0f; v.y = 0.0f; blanked = true; }
    }
    return v;
}

// output k of the call (absolute index m = a0 * up + mr0 + k): its first-tap anchor i0 relative to the call's first input, the table
// row and the blend weight.  m' * down < 2^48 and r * PHI < 2^34: no product reaches 2^63.
__device__ __forceinline__ void rs_pos(const ResampleArgs& a, uint64_t k, int64_t& rel, uint32_t& phi, float& alpha) {
    const uint64_t t = a.mr0 + k;
    const uint64_t aa = a.a0 + t / a.up, mp = t % a.up;
    const uint64_t p = mp * a.down;
    const uint64_t i0 = aa * a.down + p / a.up;
    const uint64_t q = (p % a.up) * a.PHI;
    phi = uint32_t(q / a.up);
    alpha = float(double(q % a.up) / double(a.up));
    rel = int64_t(i0 - a.in_index);
}

template <int FMT, bool BLEND, int OPL>
__global__ __launch_bounds__(RS_LANES) void resample_kernel(ResampleArgs a) {
    __shared__ __attribute__((aligned(16))) float2 s_x[RS_SPAN_MAX];
    const int tid = threadIdx.x;
    const int T = int(a.T), half = T / 2;
    const uint64_t k0 = uint64_t(blockIdx.x) * a.tile_out;
    const uint64_t kend = k0 + a.tile_out < a.n_out ? k0 + a.tile_out : a.n_out;
    int64_t rel_first, rel_last;
    {
        uint32_t ph; float al;
        rs_pos(a, k0, rel_first, ph, al);
        rs_pos(a, kend - 1, rel_last, ph, al);
    }
    const int64_t lo = rel_first - (half - 1);               // the tile's first input, relative to the call's first (negative: history)
    const int64_t span64 = rel_last + half - lo + 1;         // <= RS_SPAN_MAX by resample_tile_out
    const int span = int(span64 < int64_t(RS_SPAN_MAX) ? span64 : int64_t(RS_SPAN_MAX));
    for (int i = tid; i < span; i += RS_LANES) {
        const int64_t s = lo + i;
        float2 v; v.x = 0.0f; v.y = 0.0f;
        if (s < 0) {
            const int64_t h = int64_t(T) + s;                // history word T - 1 is the input just before the call
            if (h >= 0) v = reinterpret_cast<const float2*>(a.hist_in)[h];
        } else if (uint64_t(s) < a.n_in) {
            bool b;
            v = rs_load<FMT>(a, uint64_t(s), b);
        }
        s_x[i] = v;
    }
    __syncthreads();

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

template <int FMT>
__global__ __launch_bounds__(RS_LANES) void resample_state_kernel(ResampleArgs a) {
    const int tid = threadIdx.x;
    const int T = int(a.T);
    if (a.blank) {
        unsigned long long cnt = 0;
        const uint64_t stride = uint64_t(gridDim.x) * RS_LANES;
        for (uint64_t i = uint64_t(blockIdx.x) * RS_LANES + tid; i < a.n_in; i += stride) {
            bool b;
            (void)rs_load<FMT>(a, i, b);
            cnt += b ? 1ull : 0ull;
        }
        for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if ((tid & 63) == 0 && cnt) atomicAdd(a.blanked, cnt);
    }
    if (blockIdx.x == 0 && tid < T) {
        const uint64_t k = uint64_t(tid) + a.n_in;            // word tid of the new history is word tid + n_in of (old history | input)
        float2 v;
        if (k < uint64_t(T)) v = reinterpret_cast<const float2*>(a.hist_in)[k];
        else {
            bool b;
            v = rs_load<FMT>(a, k - uint64_t(T), b);
        }
        reinterpret_cast<float2*>(a.hist_out)[tid] = v;
    }
}

template <int FMT, bool BLEND>
void launch_out(hipStream_t s, const ResampleArgs& a) {
    const unsigned tiles = unsigned((a.n_out + a.tile_out - 1) / a.tile_out);
    if (a.tile_out > 512) resample_kernel<FMT, BLEND, 4><<<tiles, RS_LANES, 0, s>>>(a);
    else if (a.tile_out > 256) resample_kernel<FMT, BLEND, 2><<<tiles, RS_LANES, 0, s>>>(a);
    else resample_kernel<FMT, BLEND, 1><<<tiles, RS_LANES, 0, s>>>(a);
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ (the caller has checked); n_in > 0
void launch_resample(hipStream_t s, const ResampleArgs& a, int fmt) {
    const bool blend = a.PHI % a.up != 0;
    if (a.n_out) {
        if (fmt == GM_FMT_C32) { if (blend) launch_out<GM_FMT_C32, true>(s, a); else launch_out<GM_FMT_C32, false>(s, a); }
        else { if (blend) launch_out<GM_FMT_I8_IQ, true>(s, a); else launch_out<GM_FMT_I8_IQ, false>(s, a); }
    }
    // the count reads every input once: a workgroup per 2048 inputs, at most 1024 of them; without blanking one workgroup (the history)
    uint64_t blocks = a.blank ? (a.n_in + 2047) / 2048 : 1;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    if (fmt == GM_FMT_C32) resample_state_kernel<GM_FMT_C32><<<unsigned(blocks), RS_LANES, 0, s>>>(a);
    else resample_state_kernel<GM_FMT_I8_IQ><<<unsigned(blocks), RS_LANES, 0, s>>>(a);
}

}  // namespace gm
