// The in-kernel standard-normal stream of the sampling kernels: Philox4x32-10 keyed by the 64-bit seed, counter
// (lane, draw, 0, 'STGN'), two uniforms -> Box-Muller.  Which lane and draw a sample takes is sample_draw.hpp's
// business.  tests/philox_np.py is the host replay of this stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace stg {

namespace {

__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0,
                                             uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
}

// two independent standard normals for counter (lane, draw) under `seed` (Philox4x32-10 + Box-Muller)
__device__ __forceinline__ float2 philox_normal2(uint64_t seed, uint64_t lane, uint32_t draw) {
    uint32_t c0 = (uint32_t)lane, c1 = (uint32_t)(lane >> 32), c2 = draw, c3 = 0x5354474Eu;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);       // (0,1)
    const float u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u0));
    float s, c;
    sincosf(6.28318530717958647692f * u1, &s, &c);
    return make_float2(r * c, r * s);
}

}  // namespace

}  // namespace stg
