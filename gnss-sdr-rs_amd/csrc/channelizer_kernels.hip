// channelizer_kernels.hip — the polyphase filter bank (gm_channelizer; gnss_mi355x.h states the definition): M sub-bands of one complex
// stream, each at rate fs / D, from one prototype filter of L = M P taps and one M-point transform per output time.
//
// channelizer_kernel<M, FMT>: one 256-lane workgroup per tile of output times.  The tile's input span ((tile - 1) D + L samples, at most
//   CH_SPAN_MAX by the choice of the tile) is converted and blanked ONCE into LDS as float pairs — from the call's input, or, in front of
//   it, from the history buffer.  A lane owns the output times l, l + 256, ... of the tile (adjacent lanes store adjacent words of a
//   plane).  Per output time: the M branch sums u[r] = sum_p g[r + pM] xb[n0 + r + pM] live in registers (r unrolled, p the run-time
//   loop, ascending: one fmaf per component and tap from +0; the coefficient's address is the same in every lane, a scalar load), the
//   M-point forward DFT runs on them in registers with fft_core.h's butterflies (compile-time twiddles), and each LISTED bin k is
//   multiplied by W^{k n0} — word (k (n0 mod M)) mod M of the host's M-word table, kept in LDS — and stored to its plane.  `plane_of` is
//   read with a compile-time k: no register is indexed by a run-time value.
//   LDS banks: neighbouring lanes read samples D apart (8 D bytes), so sample i sits at word i + (i >> pad_shift): with pad_shift = 5
//   (6 at D = 64) the 32 lanes of a read group fall on 32 different 8-byte bank pairs for D = 2^a, and odd D needs no help.
//   An output time's arithmetic is one fixed function of its L inputs and of n0 mod M, whatever tile, lane or call it falls into.
// channelizer_state_kernel: workgroup 0 writes the next history (the last L blanked inputs: from this call's input, or carried forward
//   from the old history when the call is shorter than L) into the OTHER history buffer; with blanking on, all workgroups count the
//   blanked inputs of the call, each input once, with integer adds only.
// Compiled with -ffp-contract=off: re*re + im*im rounds three times, every fused operation is written as __builtin_fmaf.
#include "gm_internal.h"

namespace gm {

template <bool INV> struct Dft<64, INV> { static GM_HD void run(cf (&u)[64]) { DftCT<8, 8, INV>::run(u); } };

namespace {
constexpr int CH_LANES = 256;
constexpr int CH_LDS = CH_SPAN_MAX + (CH_SPAN_MAX >> 5);     // the padded sample image

template <int FMT>
__device__ __forceinline__ float2 ch_load(const ChannelizerArgs& a, uint64_t i, bool& blanked) {
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

template <int M, int K>
__device__ __forceinline__ void ch_store(const ChannelizerArgs& a, const cf (&u)[M], const cf* s_rot, int q, uint64_t k) {
    if constexpr (K < M) {
        const int pl = a.plane_of[K];
        if (pl >= 0) {
            const cf w = s_rot[(K * q) & (M - 1)];
            float2 y;
            y.x = u[K].x * w.x - u[K].y * w.y;
            y.y = u[K].x * w.y + u[K].y * w.x;
            reinterpret_cast<float2*>(a.out)[uint64_t(pl) * a.out_stride + k] = y;
        }
        ch_store<M, K + 1>(a, u, s_rot, q, k);
    }
}

template <int M, int FMT>
__global__ __launch_bounds__(CH_LANES) void channelizer_kernel(ChannelizerArgs a) {
    __shared__ __attribute__((aligned(16))) float2 s_x[CH_LDS];
    __shared__ cf s_rot[M];
    const int tid = threadIdx.x;
    const int L = int(a.L), D = int(a.D), P = int(a.P), sh = int(a.pad_shift);
    const uint64_t k0 = uint64_t(blockIdx.x) * a.tile_out;
    const uint64_t kend = k0 + a.tile_out < a.n_out ? k0 + a.tile_out : a.n_out;
    const int ntile = int(kend - k0);                                            // 1 .. tile_out
    const int64_t n0_first = int64_t((a.m0 + k0) * uint64_t(D)) - int64_t(L / 2 - 1);   // absolute index of the tile's first input
    const int64_t lo = n0_first - int64_t(a.in_index);                           // the same, relative to the call's first (negative: history)
    const int span_want = (ntile - 1) * D + L;                                   // <= CH_SPAN_MAX by channelizer_tile_out
    const int span = span_want < CH_SPAN_MAX ? span_want : CH_SPAN_MAX;
    for (int i = tid; i < span; i += CH_LANES) {
        const int64_t s = lo + i;
        float2 v; v.x = 0.0f; v.y = 0.0f;
        if (s < 0) {
            const int64_t h = int64_t(L) + s;                                    // history word L - 1 is the input just before the call
            if (h >= 0) v = reinterpret_cast<const float2*>(a.hist_in)[h];
        } else if (uint64_t(s) < a.n_in) {
            bool b;
            v = ch_load<FMT>(a, uint64_t(s), b);
        }
        s_x[i + (i >> sh)] = v;
    }
    if (tid < M) s_rot[tid] = a.rot[tid];
    __syncthreads();

    for (int o = tid; o < ntile; o += CH_LANES) {
        int base = o * D;
        base = base > CH_SPAN_MAX - L ? CH_SPAN_MAX - L : base;                  // in [0, span - L] by construction; the clamp keeps LDS reads in bounds whatever happens
        cf u[M];
#pragma unroll
        for (int r = 0; r < M; ++r) u[r] = cf_make(0.0f, 0.0f);
        for (int p = 0; p < P; ++p) {
            const float* g = a.taps + p * M;
            const int xb = base + p * M;
#pragma unroll
            for (int r = 0; r < M; ++r) {
                const int i = xb + r;
                const float2 x = s_x[i + (i >> sh)];
                const float c = g[r];
                u[r].x = __builtin_fmaf(c, x.x, u[r].x);
                u[r].y = __builtin_fmaf(c, x.y, u[r].y);
            }
        }
        Dft<M, false>::run(u);
        const int q = int((n0_first + int64_t(o) * D) & int64_t(M - 1));         // n0 mod M, n0 of either sign
        ch_store<M, 0>(a, u, s_rot, q, k0 + uint64_t(o));
    }
}

template <int FMT>
__global__ __launch_bounds__(CH_LANES) void channelizer_state_kernel(ChannelizerArgs a) {
    const int tid = threadIdx.x;
    const int L = int(a.L);
    if (a.blank) {
        unsigned long long cnt = 0;
        const uint64_t stride = uint64_t(gridDim.x) * CH_LANES;
        for (uint64_t i = uint64_t(blockIdx.x) * CH_LANES + tid; i < a.n_in; i += stride) {
            bool b;
            (void)ch_load<FMT>(a, i, b);
            cnt += b ? 1ull : 0ull;
        }
        for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if ((tid & 63) == 0 && cnt) atomicAdd(a.blanked, cnt);
    }
    if (blockIdx.x == 0) {
        for (int t = tid; t < L; t += CH_LANES) {
            const uint64_t k = uint64_t(t) + a.n_in;          // word t of the new history is word t + n_in of (old history | input)
            float2 v;
            if (k < uint64_t(L)) v = reinterpret_cast<const float2*>(a.hist_in)[k];
            else {
                bool b;
                v = ch_load<FMT>(a, k - uint64_t(L), b);
            }
            reinterpret_cast<float2*>(a.hist_out)[t] = v;
        }
    }
}

template <int FMT>
void launch_out(hipStream_t s, const ChannelizerArgs& a) {
    const unsigned tiles = unsigned((a.n_out + a.tile_out - 1) / a.tile_out);
    switch (a.M) {
        case 4: channelizer_kernel<4, FMT><<<tiles, CH_LANES, 0, s>>>(a); break;
        case 8: channelizer_kernel<8, FMT><<<tiles, CH_LANES, 0, s>>>(a); break;
        case 16: channelizer_kernel<16, FMT><<<tiles, CH_LANES, 0, s>>>(a); break;
        case 32: channelizer_kernel<32, FMT><<<tiles, CH_LANES, 0, s>>>(a); break;
        default: channelizer_kernel<64, FMT><<<tiles, CH_LANES, 0, s>>>(a); break;
    }
}
}  // namespace

// fmt: GM_FMT_C32 or GM_FMT_I8_IQ, M one of 4 .. 64 (the caller has checked); n_in > 0
void launch_channelizer(hipStream_t s, const ChannelizerArgs& a, int fmt) {
    if (a.n_out) {
        if (fmt == GM_FMT_C32) launch_out<GM_FMT_C32>(s, a);
        else launch_out<GM_FMT_I8_IQ>(s, a);
    }
    // the count reads every input once: a workgroup per 2048 inputs, at most 1024 of them; without blanking one workgroup (the history)
    uint64_t blocks = a.blank ? (a.n_in + 2047) / 2048 : 1;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    if (fmt == GM_FMT_C32) channelizer_state_kernel<GM_FMT_C32><<<unsigned(blocks), CH_LANES, 0, s>>>(a);
    else channelizer_state_kernel<GM_FMT_I8_IQ><<<unsigned(blocks), CH_LANES, 0, s>>>(a);
}

}  // namespace gm
