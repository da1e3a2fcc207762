// bestofk: the evaluation tail of test.test (test.py:59-123) with metrics.ade / fde / nodes_rel_to_nodes_abs
// (metrics.py:21-75) as ONE device op: per pedestrian, draw K trajectories from the predicted bivariate
// Gaussians (MultivariateNormal(mean, cov).sample() = mean + chol(cov) eps, test.py:59-71), integrate the
// displacements from the last observed position (test.py:89-91), and keep the smallest average / final
// displacement error against the ground truth (test.py:104-117).
//
// One lane per (scene, pedestrian); lanes run along v, so every load of V_pred, the targets and the noise is
// coalesced.  The whole K x P loop stays in registers: HBM traffic is V_pred + targets once (L2 serves the K
// re-reads) + the optional noise tensor.  Noise: either caller-provided standard normals (exact parity with a
// CPU sampler fed the same numbers) or an in-kernel Philox4x32-10 stream keyed by (seed; scene, ped, k, t).
#include "common.hpp"
#include "sample_draw.hpp"

namespace stg {

__global__ __launch_bounds__(256) void bestofk_kernel(
    const float *__restrict__ pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
    const float *__restrict__ target_rel, const float *__restrict__ obs_last,
    const int32_t *__restrict__ num_peds, const float *__restrict__ noise, uint64_t seed, int N, int P, int V,
    int K, float *__restrict__ ade, float *__restrict__ fde) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * V) return;
    const int n = (int)(idx / V), v = (int)(idx - (int64_t)n * V);
    int vi = num_peds ? num_peds[n] : V;
    vi = vi < 0 ? 0 : (vi > V ? V : vi);
    if (v >= vi) {                         // padded slot
        ade[idx] = 0.f;
        fde[idx] = 0.f;
        return;
    }
    const float *pn = pred + n * p_sn + v * p_sv;
    const float *tn = target_rel + ((int64_t)n * P * V + v) * 2;
    float ox = 0.f, oy = 0.f;
    if (obs_last) {
        ox = obs_last[idx * 2];
        oy = obs_last[idx * 2 + 1];
    }
    float best_a = INFINITY, best_f = INFINITY;
    const float inv_p = 1.0f / (float)P;
    for (int k = 0; k < K; ++k) {
        float cx = 0.f, cy = 0.f, gx = 0.f, gy = 0.f, acc = 0.f, last = 0.f;
        for (int t = 0; t < P; ++t) {
            const float *q = pn + t * p_sp;
            const float mx = q[0], my = q[p_sf];
            // (draw_chol(q, p_sf) with its arguments evaluated here: inside the helper the compiler moves the two expf
            // behind tanhf's branch and away from their loads, measured +1.2 % on this kernel's time)
            const Chol2 l = draw_chol(expf(q[2 * p_sf]), expf(q[3 * p_sf]), tanhf(q[4 * p_sf]));
            float2 e;
            if (noise)
                e = *reinterpret_cast<const float2 *>(noise + ((((int64_t)k * N + n) * P + t) * V + v) * 2);
            else
                e = draw_normal2(seed, idx, k, P, t);   // idx = n * V + v
            draw_step(cx, cy, mx, my, l, e);            // cumulative sum of sampled displacements (metrics.py:70-73)
            const float2 tg = *reinterpret_cast<const float2 *>(tn + (int64_t)t * V * 2);
            gx += tg.x;
            gy += tg.y;
            const float dx = (cx + ox) - (gx + ox), dy = (cy + oy) - (gy + oy);
            last = sqrtf(dx * dx + dy * dy);
            acc += last;
        }
        best_a = fminf(best_a, acc * inv_p);
        best_f = fminf(best_f, last);
    }
    ade[idx] = K > 0 ? best_a : 0.f;
    fde[idx] = K > 0 ? best_f : 0.f;
}

}  // namespace stg

extern "C" {

int stg_bestofk_eval(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                     const float *target_rel, const float *obs_last, const int32_t *num_peds, const float *noise,
                     uint64_t seed, int N, int P, int V, int K, float *ade, float *fde, void *stream) {
    STG_REQUIRE(N >= 0 && P > 0 && V > 0 && K >= 0, STG_EINVAL, "stg_bestofk_eval: bad sizes N=%d P=%d V=%d K=%d", N,
                P, V, K);
    if (N == 0) return STG_OK;
    STG_REQUIRE(pred && target_rel && ade && fde, STG_EINVAL, "stg_bestofk_eval: null pointer");
    const int64_t total = (int64_t)N * V;
    STG_REQUIRE(total < (1ll << 31) * 256, STG_EINVAL, "stg_bestofk_eval: N*V too large");
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(stg::bestofk_kernel, dim3((unsigned)blocks), dim3(256), 0, stg::as_stream(stream), pred, p_sn,
                       p_sf, p_sp, p_sv, target_rel, obs_last, num_peds, noise, seed, N, P, V, K, ade, fde);
    STG_LAUNCH_CHECK("stg_bestofk_eval");
    return STG_OK;
}

}  // extern "C"
