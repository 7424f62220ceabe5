// acq_stage_f_edge.hip — stage F of a coherent handle's edge search (gm_acq_set_edge_search): acq_stage_f_variants.h's three kernels with
// EdgeLoad, instantiated for every plan they can run on, and the reduction over the hypotheses.
// The three families share one source and take a unit each: in one unit they were the longest job of the build.  None of them shares
// a unit with the K = 1 kernels, whose sources and code objects stay exactly as they are.
#include "acq_stage_f_variants.h"

namespace gm {

template StageFLaunch find_stage_f<EdgeLoad>(int, int);

// ------------------------------------------------------------------------------------ the reduction over the hypotheses
// [3][P][H][D] -> [3][P][D] + choice [P][D]: one lane per (listed worker, bin) cell.  The hypothesis with the largest max wins, on equal
// values the lowest h (a strict comparison with h ascending); its three words are copied as they are.  Rows of workers that are not
// listed stay untouched, as stage C leaves them.
__global__ __launch_bounds__(256) void acq_edge_reduce_kernel(const uint32_t* __restrict__ full, uint32_t* __restrict__ met,
                                                              uint32_t* __restrict__ choice, const uint32_t* __restrict__ worker_list,
                                                              uint32_t n_workers, uint32_t P, uint32_t H, uint32_t D) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_workers * D) return;
    const uint32_t w = g / D, d = g - w * D, p = worker_list[w];
    const size_t PHD = size_t(P) * H * D, PD = size_t(P) * D;
    const size_t b = size_t(p) * H * D + d;
    uint32_t bh = 0;
    float bv = __uint_as_float(full[b]);
    for (uint32_t h = 1; h < H; ++h) {
        const float v = __uint_as_float(full[b + size_t(h) * D]);
        if (v > bv) { bv = v; bh = h; }
    }
    const size_t src = b + size_t(bh) * D, dst = size_t(p) * D + d;
    met[dst] = full[src];
    met[PD + dst] = full[PHD + src];
    met[2 * PD + dst] = full[2 * PHD + src];
    choice[dst] = bh;
}

void launch_edge_reduce(hipStream_t st, const uint32_t* full, uint32_t* met, uint32_t* choice, const uint32_t* worker_list,
                        uint32_t n_workers, uint32_t P, uint32_t H, uint32_t D) {
    if (!n_workers || !D) return;
    hipLaunchKernelGGL(acq_edge_reduce_kernel, dim3((n_workers * D + 255) / 256), dim3(256), 0, st, full, met, choice, worker_list,
                       n_workers, P, H, D);
}

}  // namespace gm
