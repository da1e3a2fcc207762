// sample_traj: the sampling half of test.test (test.py:59-91) for a whole batch -- per pedestrian K trajectories
// drawn from the predicted bivariate Gaussians (MultivariateNormal(mean, cov).sample() = mean + chol(cov) eps) and
// integrated from the last observed position (metrics.nodes_rel_to_nodes_abs), plus the zero-noise trajectory.  What
// stg_bestofk_eval reduces to min-ADE / min-FDE in registers, this kernel writes out: raw_data_dict[step]['pred'].
//
// A write-bound stream (K x N x P x V x 2 floats out against N x 5 x P x V in, re-read K times from L2 / MALL), so the
// mapping is chosen for stores and parallelism: one lane per (k, scene, pedestrian group of PEDS), pedestrians
// fastest, k slowest.  Each time step a lane stores its PEDS x 2 floats of the row samples[k, n, t, :, :] (one float4
// for a pair), so a wave's store covers whole 128-byte lines of consecutive rows.  The draw is sample_draw.hpp's, as
// in bestofk_kernel, so best-of-K over `samples` is what stg_bestofk_eval reports for the same seed.
#include "common.hpp"
#include "sample_draw.hpp"

#include <type_traits>

namespace stg {

template <int PEDS>
__global__ __launch_bounds__(256) void sample_traj_kernel(
    const float *__restrict__ pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
    const float *__restrict__ obs_last, const int32_t *__restrict__ num_peds, const float *__restrict__ noise,
    uint64_t seed, const uint64_t *__restrict__ seed_dev, int N, int P, int V, int K, float *__restrict__ samples,
    float *__restrict__ mean) {
    using vec = typename std::conditional<PEDS == 2, float4, float2>::type;
    const int vg = V / PEDS;                                   // pedestrian groups per scene (host: V % PEDS == 0)
    const int64_t per_k = (int64_t)N * vg;
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= (K > 0 ? K : 1) * per_k) return;
    const int k = (int)(idx / per_k);
    const int64_t rem = idx - k * per_k;
    const int n = (int)(rem / vg);
    const int v0 = (int)(rem - (int64_t)n * vg) * PEDS;
    if (seed_dev) seed = *seed_dev;
    int vi = num_peds ? num_peds[n] : V;
    vi = vi < 0 ? 0 : (vi > V ? V : vi);
    const bool do_samp = k < K, do_mean = mean != nullptr && k == 0;

    float ox[PEDS], oy[PEDS], cx[PEDS], cy[PEDS], mx_s[PEDS], my_s[PEDS];
#pragma unroll
    for (int j = 0; j < PEDS; ++j) {
        const int64_t o = ((int64_t)n * V + v0 + j) * 2;
        ox[j] = obs_last && v0 + j < vi ? obs_last[o] : 0.f;
        oy[j] = obs_last && v0 + j < vi ? obs_last[o + 1] : 0.f;
        cx[j] = cy[j] = mx_s[j] = my_s[j] = 0.f;
    }
    float *srow = do_samp ? samples + (((int64_t)k * N + n) * P * V + v0) * 2 : nullptr;
    float *mrow = do_mean ? mean + ((int64_t)n * P * V + v0) * 2 : nullptr;
    const float *nrow = noise ? noise + (((int64_t)k * N + n) * P * V + v0) * 2 : nullptr;
    for (int t = 0; t < P; ++t) {
        alignas(8 * PEDS) float s_out[2 * PEDS], m_out[2 * PEDS], e_in[2 * PEDS];
        if (do_samp && noise) {
            const vec e = *reinterpret_cast<const vec *>(nrow + (int64_t)t * V * 2);
            *reinterpret_cast<vec *>(e_in) = e;
        }
#pragma unroll
        for (int j = 0; j < PEDS; ++j) {
            const int v = v0 + j;
            s_out[2 * j] = s_out[2 * j + 1] = m_out[2 * j] = m_out[2 * j + 1] = 0.f;      // padded slot: zeros
            if (v >= vi) continue;
            const float *q = pred + n * p_sn + v * p_sv + t * p_sp;
            const float mx = q[0], my = q[p_sf];
            if (do_samp) {
                const Chol2 l = draw_chol(q, p_sf);
                float2 e;
                if (noise)
                    e = make_float2(e_in[2 * j], e_in[2 * j + 1]);
                else
                    e = draw_normal2(seed, n, V, v, k, P, t);
                draw_step(cx[j], cy[j], mx, my, l, e);
                s_out[2 * j] = cx[j] + ox[j];
                s_out[2 * j + 1] = cy[j] + oy[j];
            }
            if (do_mean) {
                mx_s[j] += mx;
                my_s[j] += my;
                m_out[2 * j] = mx_s[j] + ox[j];
                m_out[2 * j + 1] = my_s[j] + oy[j];
            }
        }
        if (do_samp) *reinterpret_cast<vec *>(srow + (int64_t)t * V * 2) = *reinterpret_cast<const vec *>(s_out);
        if (do_mean) *reinterpret_cast<vec *>(mrow + (int64_t)t * V * 2) = *reinterpret_cast<const vec *>(m_out);
    }
}

}  // namespace stg

extern "C" {

int stg_sample_trajectories(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                            const float *obs_last, const int32_t *num_peds, const float *noise, uint64_t seed,
                            const uint64_t *seed_dev, int N, int P, int V, int K, float *samples, float *mean,
                            void *stream) {
    STG_REQUIRE(N >= 0 && P > 0 && V > 0 && K >= 0, STG_EINVAL,
                "stg_sample_trajectories: bad sizes N=%d P=%d V=%d K=%d", N, P, V, K);
    if (N == 0) return STG_OK;
    STG_REQUIRE(pred, STG_EINVAL, "stg_sample_trajectories: null pointer (pred)");
    STG_REQUIRE(samples || K == 0, STG_EINVAL, "stg_sample_trajectories: null pointer (samples with K=%d)", K);
    STG_REQUIRE(samples || mean, STG_EINVAL, "stg_sample_trajectories: null pointer (no output)");
    using stg::aligned;
    STG_REQUIRE(aligned(samples, 8) && aligned(mean, 8) && aligned(noise, 8) && aligned(obs_last, 8), STG_EINVAL,
                "stg_sample_trajectories: samples / mean / noise / obs_last must be 8-byte aligned");
    // a pair of pedestrians per lane (float4 stores) when the rows split into aligned pairs, else one (float2)
    int peds = (V % 2 == 0 && aligned(samples, 16) && aligned(mean, 16) && aligned(noise, 16)) ? 2 : 1;
    if (stg::diag_env("STG_SAMPLE_PEDS", 2) == 1) peds = 1;            // A/B switch of the diagnostic build only
    const int64_t total = (int64_t)(K > 0 ? K : 1) * N * (V / peds);
    STG_REQUIRE(total < (1ll << 31) * 256, STG_EINVAL, "stg_sample_trajectories: K*N*V too large");
    const int64_t blocks = (total + 255) / 256;
    if (peds == 2)
        hipLaunchKernelGGL(stg::sample_traj_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, stg::as_stream(stream),
                           pred, p_sn, p_sf, p_sp, p_sv, obs_last, num_peds, noise, seed, seed_dev, N, P, V, K,
                           samples, mean);
    else
        hipLaunchKernelGGL(stg::sample_traj_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stg::as_stream(stream),
                           pred, p_sn, p_sf, p_sp, p_sv, obs_last, num_peds, noise, seed, seed_dev, N, P, V, K,
                           samples, mean);
    STG_LAUNCH_CHECK("stg_sample_trajectories");
    return STG_OK;
}

}  // extern "C"
