/* stgcnn_hip_metrics.h -- distribution metrics of a batch of predictions against the ground truth: part of the C ABI of
 * libstgcnn_hip.so, included by stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and
 * status codes) and not meant to be included on its own.  The binding of this entry point is social_stgcnn_amd/_lib.py's
 * _SIGNATURES_METRICS; tests/test_dist_metrics_cpu.py holds the two copies against each other.                       */
#ifndef STGCNN_HIP_METRICS_H
#define STGCNN_HIP_METRICS_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N14  what stg_sample_trajectories leaves on the device, judged against the truth (an added entry point,
 *      the ABI version stays).  The sampler draws the steps independently and sums them, so the absolute position at
 *      horizon h is N(mean_h, C_h) with C_h = sum_{t<=h} [sx^2, rho sx sy, sy^2]_t: the record of the live score (N8).
 *   Inputs: v_pred (N,5,P,V) with strides, mean (N,P,V,2), samples (K,N,P,V,2) or NULL with K == 0, truth (N,P,V,2)
 *     absolute positions, num_peds int32[N] or NULL (every scene holds V).  All float32, DEVICE memory.
 *   Per element (N,P,V), float32 as written (no fused multiply-add), zero where v >= num_peds[n]:
 *     cov (N,P,V,3), optional (NULL: not written): C_h as N8 accumulates it (expf, tanhf, ascending t)
 *     d2, nll   N8's values of the offset mean - truth under C_h, the determinant floored at 2^-15 cxx cyy
 *     lam       the larger eigenvalue of C_h: 0.5 (cxx + cyy) + sqrtf(0.25 (cxx - cyy)^2 + cxy^2)
 *     kde_nll   (K >= 3) minus the log density at the truth of the Gaussian kernel density estimate of the K sampled
 *               positions at that horizon, bandwidth by Scott's rule: kernel covariance H = K^(-1/3) S, S the unbiased
 *               sample covariance about the sample mean (two passes); det H floored at 2^-15 hxx hyy; the density summed
 *               about the nearest sample (in the metric of H); the result clipped from above at kde_floor (NaN -> kde_floor)
 *   Per pedestrian (N,V), K >= 3: ade = min_k (sum_t |samples[k,t] - truth_t|) / P, fde = min_k |samples[k,P] - truth_P|:
 *     N8's traj_ade / traj_fde of a pedestrian matched at every horizon.  ade_ref, fde_ref float64 (N,V), optional (both
 *     or neither; NULL: not computed): the same two minima in the reference's own arithmetic (metrics.py:21-53 as
 *     predict.sample_test evaluates it): float32 differences and squares, a float64 root, a float64 sum in ascending t, / P.
 *   Per scene (N), K >= 3, c = num_peds[n]: jade = min_k (sum_v sum_t e[k,t,v]) / (c P), jfde = min_k (sum_v e[k,P,v]) / c,
 *     jbest int32 = the k of jade (the lowest on ties); 0, 0 and -1 for c == 0.  The sums over v are float32 in a fixed
 *     order (a lane holds one pedestrian, a wave's 64 by the xor butterfly 32 .. 1, the waves ascending): bitwise repeatable.
 *   One workgroup per scene, a lane per pedestrian, no atomics, no host synchronisation.  1 <= P <= STG_SCORE_MAX_P,
 *   1 <= V <= STG_SCORE_MAX_V, K == 0 or 3 <= K <= STG_SCORE_MAX_K: above a limit STG_EUNSUPPORTED; K of 1 or 2, bad
 *   sizes, NULL required pointers (the sample-based outputs with K >= 3), samples without K or K without samples, mean /
 *   samples / truth not 8-byte aligned: STG_EINVAL; both decided before any launch.  N == 0 is a no-op.               */
int stg_dist_metrics(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *mean,
                     const float *samples, const float *truth, const int32_t *num_peds, int N, int P, int V, int K,
                     float kde_floor, float *cov, float *d2, float *nll, float *lam, float *kde_nll, float *ade,
                     float *fde, float *jade, float *jfde, int32_t *jbest, double *ade_ref, double *fde_ref,
                     void *stream);

#endif /* STGCNN_HIP_METRICS_H */
