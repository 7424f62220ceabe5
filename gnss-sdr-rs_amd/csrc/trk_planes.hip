// trk_planes.hip — gm_plane_ring's copy kernel and gm_trk_update_planes' tracking kernel (gfx950, wave64).
//
// A SECTION of trk_kernels.hip, included at the end of its namespace like trk_bank.hip and trk_array.hip (it is not a translation unit of
// its own): the tracking kernel forms its samples with correlate_sample<ARMS, FAST> and ends an epoch with epoch_epilogue<ARMS>, which
// live in that file, and none of the kernels above is touched by it.  include/gnss_mi355x.h states the contract of both.
//
//   plane_ring_write_kernel<WIDE> : grid (x, planes), 256 lanes.  Sample i of plane p goes from src[p * in_stride + i] to
//       ring[p * plane_size + ((start + i) & mask)].  WIDE: two samples (16 bytes) a lane and step; the host takes that form only when the
//       source is 16-byte aligned and in_stride, n, start and plane_size are even, so a pair is aligned on both sides and never straddles
//       the wrap.  Bounds: i < n <= plane_size, p < n_planes (the grid), the destination index is masked.
//   trk_planes_kernel<ARMS> : grid (channels), 256 lanes, one workgroup per channel and nothing shared between workgroups: no exchange, no
//       spin wait, no atomics.  What trk_correlate_kernel (one slice) + trk_update_kernel do per pass, for `epochs` passes with the state
//       kept on chip: gate, per-sample products by correlate_sample on plane[(next_sample_index + i) & mask], the fixed tree (lane j its
//       samples j, j + 256, ... in order; butterfly xor 32 .. 1; the four waves in ascending order), epoch_epilogue in DO_WORK mode on
//       lane 0, the pass's outs / processed / lost / lost_prn, the new state to all lanes through LDS.  The state is stored once, behind
//       the last pass.  Every condition the loop branches on is a function of the channel's state and the launch's arguments, the same in
//       all 256 lanes, so the barriers are met by all of them.
//       Bounds: the plane index is checked on the host against the ring (and clamped here), sample indices are masked with
//       plane_size - 1, the chip row is read only when 0 <= row < n_codes, chip indices lie in [0, code_len) (chip_index / chip_index_arm),
//       result words at [pass][channel] with pass < epochs, channel < n_channels (the grid).

template <bool WIDE>
__global__ __launch_bounds__(256) void plane_ring_write_kernel(const cf* __restrict__ src, cf* __restrict__ ring, uint64_t in_stride,
                                                               uint64_t plane_size, uint64_t start, uint64_t n) {
    const uint64_t p = blockIdx.y, mask = plane_size - 1;
    const cf* s = src + p * in_stride;
    cf* d = ring + p * plane_size;
    const uint64_t step = uint64_t(gridDim.x) * 256u;
    if constexpr (WIDE) {
        for (uint64_t j = uint64_t(blockIdx.x) * 256u + threadIdx.x; j < n / 2; j += step) {
            const float4 v = *reinterpret_cast<const float4*>(s + 2 * j);
            *reinterpret_cast<float4*>(d + ((start + 2 * j) & mask)) = v;
        }
    } else {
        for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n; i += step) d[(start + i) & mask] = s[i];
    }
}

void launch_plane_ring_write(hipStream_t st, const PlaneRingWriteArgs& a) {
    if (!a.n || !a.n_planes) return;
    const uint64_t units = a.wide ? a.n / 2 : a.n, wg = (units + 255) / 256;
    const dim3 grid(uint32_t(wg < 1024 ? wg : 1024), a.n_planes);
    if (a.wide) hipLaunchKernelGGL(plane_ring_write_kernel<true>, grid, dim3(256), 0, st, a.src, a.ring, a.in_stride, a.plane_size, a.start, a.n);
    else hipLaunchKernelGGL(plane_ring_write_kernel<false>, grid, dim3(256), 0, st, a.src, a.ring, a.in_stride, a.plane_size, a.start, a.n);
}

template <int ARMS>
__global__ __launch_bounds__(256) void trk_planes_kernel(TrkPlanesArgs a) {
    constexpr int NV = 2 * ARMS;
    const TrkDevCfg& cfg = a.cfg;
    const int ch = blockIdx.x, tid = threadIdx.x;
    extern __shared__ int8_t chips[];   // code_len chips of this channel's row
    __shared__ float wsum[4][NV];
    __shared__ gm_trk_state next_state;

    gm_trk_state st = a.states[ch];     // every lane holds the channel's state
    uint32_t pl = a.map[ch];
    if (pl >= a.n_planes) pl = 0;       // (the host has refused such a map)
    const cf* __restrict__ plane = a.ring + uint64_t(pl) * a.plane_size;

    // before the first pass: the chip row.  prn changes only in reset(), which also clears `active`: a channel that runs, runs on this row
    const int row = code_row(cfg, st);
    const bool row_ok = row >= 0 && row < cfg.n_codes;
    if (row_ok) {
        const int8_t* crow = a.codes + size_t(row) * cfg.code_len;
        for (int i = tid; i < cfg.code_len; i += 256) chips[i] = crow[i];
    }
    __syncthreads();

    bool any = false;
    for (int e = 0; e < a.epochs; ++e) {
        const size_t o = size_t(e) * size_t(cfg.n_channels) + size_t(ch);
        // update(): n = generate_ca_code_samples(..).len() (:165-166); (head - (next + n)) as isize >= 0 (:170-172)
        const uint64_t n = samples_per_code(cfg.fs, st.code_rate, cfg.code_len_f);
        const bool run = st.active && row_ok && code_row(cfg, st) == row && n > 0 && n < (1ull << 31) &&
                         (int64_t)(a.head - (st.next_sample_index + n)) >= 0;
        if (!run) {                     // what trk_correlate_kernel + trk_update_kernel leave for a channel that is not ready
            if (tid == 0) {
                float z[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) z[k] = 0.0f;
                if (a.outs) a.outs[o] = make_out<ARMS>(z);
                if (a.processed) a.processed[o] = 0;
                if (a.lost) a.lost[o] = 0;
                if (a.lost_prn) a.lost_prn[o] = 0;
            }
            continue;
        }
        st.num_samples_per_code = n;    // (:166)
        const EpochConsts ec = epoch_consts(cfg, st);
        float acc[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
        const uint64_t base = st.next_sample_index;
        const uint32_t n32 = uint32_t(n);
        if (fast_code_range(ec, n)) {
            for (uint32_t i = tid; i < n32; i += 256) correlate_sample<ARMS, true>(ec, chips, plane[(base + i) & a.mask], i, acc);
        } else {
            for (uint32_t i = tid; i < n32; i += 256) correlate_sample<ARMS, false>(ec, chips, plane[(base + i) & a.mask], i, acc);
        }
        // per-lane sums -> wavefront butterfly (64 lanes) -> the four waves through LDS, ascending
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
        }
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) wsum[wave][k] = acc[k];
        }
        __syncthreads();
        if (tid == 0) {
            float v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
            uint8_t lst = 0, lprn = 0;
            epoch_epilogue<ARMS>(cfg, st, v, n, TRK_MODE_DO_WORK, lst, lprn);
            if (a.outs) a.outs[o] = make_out<ARMS>(v);
            if (a.processed) a.processed[o] = 1;
            if (a.lost) a.lost[o] = lst;
            if (a.lost_prn) a.lost_prn[o] = lprn;
            next_state = st;
        }
        __syncthreads();
        st = next_state;                // read before the next pass's barrier, rewritten only behind it
        any = true;
    }
    if (any && tid == 0) a.states[ch] = st;
}

void launch_trk_planes(hipStream_t st, const TrkPlanesArgs& a) {
    const size_t lds = size_t(a.cfg.code_len);
    if (a.cfg.n_arms == 5) hipLaunchKernelGGL(trk_planes_kernel<5>, dim3(a.cfg.n_channels), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(trk_planes_kernel<3>, dim3(a.cfg.n_channels), dim3(256), lds, st, a);
}
