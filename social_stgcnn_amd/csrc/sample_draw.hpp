// One sampled displacement of (scene n, pedestrian v, sample k, step t), for every kernel that turns V_pred (N,5,P,V)
// into the K sampled trajectories (bestofk_kernel, sample_traj_kernel, sample_risk_kernel): mean + chol(cov) eps, as
// MultivariateNormal(mean, cov).sample() draws it (test.py:59-71).  The kernels call these pieces and keep only their
// own mapping of lanes, stores and LDS, so the samples of one are the samples of the others (up to the multiply-adds
// the compiler fuses per kernel, ~2e-6).
#pragma once
#include "philox.hpp"

namespace stg {

namespace {

struct Chol2 {
    float l00, l10, l11;
};

// chol([[sx^2, rho sx sy], [rho sx sy, sy^2]]) in the order torch.linalg.cholesky evaluates it, with the radicand
// clamped at zero: where tanhf saturates (|raw| from about 9) the float32 difference sy^2 - l10^2 is rounding noise of
// either sign, and a negative one would make the draw and every later step of its running sum NaN.  A positive
// radicand keeps every bit; a clamped one samples on the degenerate line, which is the float64 statement to within
// the bound of DESIGN.md 2.4
__device__ __forceinline__ Chol2 draw_chol(float sx, float sy, float rho) {
    const float c01 = rho * sx * sy;
    const float l00 = sqrtf(sx * sx);
    const float l10 = c01 / l00;
    return {l00, l10, sqrtf(fmaxf(sy * sy - l10 * l10, 0.f))};
}
// q: the element (n, field 0, t, v) of V_pred, p_sf: its field stride
__device__ __forceinline__ Chol2 draw_chol(const float *q, int64_t p_sf) {
    return draw_chol(expf(q[2 * p_sf]), expf(q[3 * p_sf]), tanhf(q[4 * p_sf]));
}

// eps of the in-kernel stream: Philox lane n * V + v (V = the padded width), draw k * P + t.  A kernel whose own lane
// index is n * V + v passes it as `lane`
__device__ __forceinline__ float2 draw_normal2(uint64_t seed, int64_t lane, int k, int P, int t) {
    return philox_normal2(seed, (uint64_t)lane, (uint32_t)(k * P + t));
}
__device__ __forceinline__ float2 draw_normal2(uint64_t seed, int n, int V, int v, int k, int P, int t) {
    return draw_normal2(seed, (int64_t)n * V + v, k, P, t);
}

// the running sum of nodes_rel_to_nodes_abs (metrics.py:70-73)
__device__ __forceinline__ void draw_step(float &cx, float &cy, float mx, float my, const Chol2 &l, float2 e) {
    cx += mx + l.l00 * e.x;
    cy += my + (l.l10 * e.x + l.l11 * e.y);
}

}  // namespace

}  // namespace stg
