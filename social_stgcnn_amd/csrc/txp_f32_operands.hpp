// A operands (weights in VGPRs) of the TXP-CNN's implicit GEMMs on v_mfma_f32_16x16x4_f32: one register per K-step
// (tap, 4 channels), filled once per layer.  Shared by the wave-per-scene kernels (txp_wave.hip) and the
// workgroup-per-scene kernels (model_fwd.hip, model_bwd.hip).
#pragma once
#include "model_common.hpp"

namespace stg {

// A lane's weights of one (co, ci) pair are 9 consecutive floats (the taps): two 16-byte loads + one dword per pair
// instead of nine scattered dwords (every lane reads a different cache line, so the request count is what costs)
struct __attribute__((packed, aligned(4))) F4U {
    float v[4];
};
__device__ __forceinline__ void load_taps(const float *__restrict__ p, float (&t)[9]) {
    const F4U a = *reinterpret_cast<const F4U *>(p), b = *reinterpret_cast<const F4U *>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        t[i] = a.v[i];
        t[4 + i] = b.v[i];
    }
    t[8] = p[8];
}

// forward A operand: lane (co = l&15, kq = l>>4) of K-step (tap, j) holds W[co][4j+kq][tap]
template <int CINL>
__device__ __forceinline__ void load_w_fwd(const float *__restrict__ W, float (&wreg)[CINL * 9 / 4]) {
    const int lane = threadIdx.x & 63, co = lane & 15, kq = lane >> 4;
    const int cc = co < Cfg::P ? co : 0;              // rows 12..15 of the tile are zero
#pragma unroll
    for (int j = 0; j < CINL / 4; ++j) {
        float t[9];
        load_taps(W + (cc * CINL + 4 * j + kq) * 9, t);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) wreg[tap * (CINL / 4) + j] = co < Cfg::P ? t[tap] : 0.f;
    }
}

// input-gradient A operand: lane (ci = l&15, kq) of K-step (tap', j) holds W[4j+kq][ci][8 - tap']
template <int CINL>
__device__ __forceinline__ void load_w_bwd(const float *__restrict__ W, float (&wreg)[27]) {
    const int lane = threadIdx.x & 63, ci = lane & 15, kq = lane >> 4;
    const int cc = ci < CINL ? ci : 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float t[9];
        load_taps(W + ((4 * j + kq) * CINL + cc) * 9, t);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) wreg[tap * 3 + j] = ci < CINL ? t[8 - tap] : 0.f;
    }
}

}  // namespace stg
