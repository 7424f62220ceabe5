// acq_load8.h — eight consecutive samples of any format from any byte address, for the kernels that read a period from where the search
// read it (acq_refine.hip, acq_local.hip).
#pragma once
#include "acq_device.h"

namespace gm {

// eight consecutive samples from byte address `p` as separate real arrays — what load_sample (acq_device.h) forms, 16 bytes per load
// where ALIGNED says the address allows it (c32: four float4; int8 IQ: one uint4; int8 real: one uint2), element loads where not (a
// code-drift start is any sample, so an int8 period may begin on any byte)
template <int FMT, bool ALIGNED> __device__ __forceinline__ void load8(const char* p, float (&xr)[8], float (&xi)[8]) {
    if constexpr (FMT == GM_FMT_C32) {
        if constexpr (ALIGNED) {
            const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 v = q[e];
                xr[2 * e] = v.x; xi[2 * e] = v.y; xr[2 * e + 1] = v.z; xi[2 * e + 1] = v.w;
            }
        } else {
            const cf* q = reinterpret_cast<const cf*>(p);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const cf v = q[e]; xr[e] = v.x; xi[e] = v.y; }
        }
    } else if constexpr (FMT == GM_FMT_I8_IQ) {
        if constexpr (ALIGNED) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xr[2 * e] = float(int8_t(w[e])); xi[2 * e] = float(int8_t(w[e] >> 8));
                xr[2 * e + 1] = float(int8_t(w[e] >> 16)); xi[2 * e + 1] = float(int8_t(w[e] >> 24));
            }
        } else {
            const char2* q = reinterpret_cast<const char2*>(p);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const char2 v = q[e]; xr[e] = float(v.x); xi[e] = float(v.y); }
        }
    } else {
        if constexpr (ALIGNED) {
            const u32x2 v = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) { xr[e] = float(int8_t(v.x >> (8 * e))); xr[4 + e] = float(int8_t(v.y >> (8 * e))); }
        } else {
            const int8_t* q = reinterpret_cast<const int8_t*>(p);
#pragma unroll
            for (int e = 0; e < 8; ++e) xr[e] = float(q[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xi[e] = 0.0f;
    }
}

}  // namespace gm
