// tests/cpu/libm_host.cpp — the host side of tests/test_gpu_device_math.py: gnss-sdr-rs_amd/csrc/gm_libm.h evaluated by g++ (the
// header is host/device portable) next to the platform's own functions, under the op numbers of gm_debug_math (gnss_mi355x.h).
// Built at test time with the g++ line of tests/test_abi_and_host.py plus -fPIC -shared.
//   h0 / h1: the header's host evaluation, as raw words — what the device must reproduce bit for bit;
//   r0 / r1: the platform's answer (atanf, sinf / cosf, x / y, fmodf, sqrtf, spc_definition).
// Ops 3, 9 and 10 are device-only helpers of trk_kernels.hip (their references are written in the test): GM_HOST_NO_SUCH_OP.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "gm_libm.h"

namespace {
uint32_t low32(float v) { return v > 0.0f ? uint32_t(uint64_t(v)) : 0u; }      // samples_per_code's conversion
}

extern "C" int gm_host_math(int op, const float* x, size_t n, float p0, float p1, float p2, uint32_t* h0, uint32_t* h1, uint32_t* r0,
                            uint32_t* r1) {
    (void)p2;
    if (!x || !h0 || !h1 || !r0 || !r1) return -1;
    const float inv0 = 1.0f / p0;
    for (size_t i = 0; i < n; ++i) {
        const float v = x[i];
        float a = 0.0f, b = 0.0f;
        h0[i] = h1[i] = r0[i] = r1[i] = 0;
        switch (op) {
            case 0: h0[i] = gm::f32_bits(gm::atanf_glibc(v)); r0[i] = gm::f32_bits(atanf(v)); break;
            case 1:
                gm::sincosf_glibc(v, a, b);
                h0[i] = gm::f32_bits(a); h1[i] = gm::f32_bits(b);
                r0[i] = gm::f32_bits(sinf(v)); r1[i] = gm::f32_bits(cosf(v));
                break;
            case 2:
                gm::sincos_cw(v, a, b);
                h0[i] = gm::f32_bits(a); h1[i] = gm::f32_bits(b);
                r0[i] = gm::f32_bits(sinf(v)); r1[i] = gm::f32_bits(cosf(v));
                break;
            case 4:
                h0[i] = gm::f32_bits(gm::div_const(v, p0, inv0)); h1[i] = gm::f32_bits(gm::div_rn(v, p0));
                r0[i] = r1[i] = gm::f32_bits(v / p0);
                break;
            case 5: h0[i] = gm::f32_bits(gm::fmod_bounded(v, p0, inv0)); r0[i] = gm::f32_bits(fmodf(v, p0)); break;
            case 6: h0[i] = gm::f32_bits(gm::sqrt_rn(v)); r0[i] = gm::f32_bits(sqrtf(v)); break;
            case 7: h0[i] = h1[i] = r0[i] = r1[i] = low32(gm::spc_definition(p0, v, p1)); break;
            case 8: gm::spc_rate_bounds(p0, p1, v, a, b); h0[i] = gm::f32_bits(a); h1[i] = gm::f32_bits(b); break;
            default: return -2;
        }
    }
    return 0;
}
