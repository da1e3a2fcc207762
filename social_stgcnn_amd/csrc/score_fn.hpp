// score_fn: the values of a scored prediction, what the push-indexed and the time-indexed score kernels (score.hip,
// score_time.hip) share.  Device helpers without state, float32 as written (no fused
// multiply-add).
#pragma once
#include "common.hpp"

namespace stg {

// |p - t|, float32 as written
__device__ __forceinline__ float score_dist(float px, float py, float tx, float ty) {
#pragma clang fp contract(off)
    const float dx = px - tx, dy = py - ty;
    return sqrtf(dx * dx + dy * dy);
}

// d2 and nll of the offset (dx, dy) under the covariance (cxx, cxy, cyy), float32 as written.  The determinant is
// floored at 2^-15 of cxx*cyy: the float32 C_h (expf, tanhf, up to 32 summed steps) and the difference's own three
// roundings leave it an absolute error of up to 213 * 2^-24 cxx*cyy, so below the floor it is mostly noise (a
// saturated tanhf makes it 0 or negative); at the floor the relative error is below one half.  Above the floor every
// bit is what the plain difference gives
__device__ __forceinline__ void score_gauss(float dx, float dy, float cxx, float cxy, float cyy, float &d2, float &nll) {
#pragma clang fp contract(off)
    const float p = cxx * cyy;
    const float det = fmaxf(p - cxy * cxy, p * 0x1p-15f);
    d2 = (cyy * (dx * dx) - 2.f * cxy * dx * dy + cxx * (dy * dy)) / det;
    nll = 0.5f * d2 + 0.5f * (float)log((double)det) + 1.8378770664093453f;
}

}  // namespace stg
