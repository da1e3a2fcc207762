// score_fn: what the push-indexed and the time-indexed score kernels (score.hip, score_time.hip) share (DESIGN.md 5.17,
// 5.25, 5.30): the values of a scored prediction, the record tables they advance, the trajectory values of a retiring
// row, the totals columns, the pieces of an enqueue and, on the host, the checks on the prediction.  Device helpers
// without state, float32 as written (no fused multiply-add); where the truth comes from, which wave takes which work and
// where the per-entry results go stay with the two kernels.
#pragma once
#include "common.hpp"

namespace stg {

constexpr int kScoreThreads = 256;
constexpr int kScoreWaves = kScoreThreads / kWave;
constexpr int kScoreCols = 5;                           // totals columns ahead of the coverage counts
constexpr int kScoreRow = kScoreCols + STG_SCORE_MAX_Q;

// The prediction as the chain leaves it: mean (NS,P,V,2), v_pred with strides, samples (K,NS,P,V,2), ids (NS,V)
struct ScorePred {
    const float *mean, *v_pred;
    int64_t p_sn, p_sf, p_sp, p_sv;
    const float *samples;
    const int64_t *ids;
    const int32_t *num_peds;
};

// One stream's record tables, a row r per record: mean (.,P,V,2), cov (.,P,V,3), samples (.,K,P,V,2) and the
// accumulators acc (.,K,V), acc_mean (.,V), steps (.,V); samples and acc are null with K = 0
struct ScoreRows {
    float *mean, *cov, *samples, *acc, *acc_mean;
    int32_t *steps;
    int P, V, K;
};

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

// Pedestrian v of record r scored at its step h against the truth (tx, ty): err, d2, nll, best (0 with K = 0), and the
// record's accumulators advance -- acc[k] += |samples[k,h] - truth|, acc_mean += err, steps += 1.  The row belongs to the
// calling wave: plain read-modify-writes
__device__ __forceinline__ void score_entry(const ScoreRows &t, int r, int h, int v, float tx, float ty, float &err,
                                            float &d2, float &nll, float &best) {
    const int P = t.P, V = t.V, K = t.K;
    const int64_t e = ((int64_t)r * P + (h - 1)) * V + v;
    const int x = r * V + v;
    const float2 mu = *reinterpret_cast<const float2 *>(t.mean + e * 2);
    err = score_dist(mu.x, mu.y, tx, ty);
    score_gauss(mu.x - tx, mu.y - ty, t.cov[e * 3], t.cov[e * 3 + 1], t.cov[e * 3 + 2], d2, nll);
    t.acc_mean[x] += err;
    t.steps[x] += 1;
    best = 0.f;
    if (K > 0) {
        float bmin = INFINITY;
        for (int k = 0; k < K; ++k) {
            const int64_t se = (((int64_t)r * K + k) * P + (h - 1)) * V + v;
            const float2 s = *reinterpret_cast<const float2 *>(t.samples + se * 2);
            const float d = score_dist(s.x, s.y, tx, ty);
            bmin = fminf(bmin, d);
            t.acc[((int64_t)r * K + k) * V + v] += d;
        }
        best = bmin;
    }
}

// Pedestrian v of the retiring record r: returns its steps, t_ade = min_k acc[k] / steps and t_adem = acc_mean / steps
// (0 without steps); with steps == P the trajectory enters the lane's five totals tp.  t_fde, t_fdem: best and err at
// h = P, which the caller holds
__device__ __forceinline__ int score_retire(const ScoreRows &t, int r, int v, float t_fde, float t_fdem, float &t_ade,
                                            float &t_adem, double (&tp)[5]) {
    const int x = r * t.V + v;
    const int sn = t.steps[x];
    t_ade = 0.f, t_adem = 0.f;
    if (sn > 0) {
        if (t.K > 0) {
            float amin = INFINITY;
            for (int k = 0; k < t.K; ++k) amin = fminf(amin, t.acc[((int64_t)r * t.K + k) * t.V + v]);
            t_ade = amin / (float)sn;
        }
        t_adem = t.acc_mean[x] / (float)sn;
    }
    if (sn == t.P) {
        tp[0] += 1.0;
        tp[1] += (double)t_ade;
        tp[2] += (double)t_fde;
        tp[3] += (double)t_adem;
        tp[4] += (double)t_fdem;
    }
    return sn;
}

// The totals columns of one matched entry: count, err, d2, nll, best and, for each of the Q thresholds, whether
// d2 <= thr_q.  kAdd: added to a lane's partial sums; otherwise stored over zeros ahead of a wave_sum
template <bool kAdd>
__device__ __forceinline__ void score_cols(double (&c)[kScoreRow], float err, float d2, float nll, float best,
                                           const float *thr, int Q) {
    const double x[kScoreCols] = {1.0, (double)err, (double)d2, (double)nll, (double)best};
#pragma unroll
    for (int i = 0; i < kScoreCols; ++i) c[i] = kAdd ? c[i] + x[i] : x[i];
#pragma unroll
    for (int q = 0; q < STG_SCORE_MAX_Q; ++q)
        if (q < Q && d2 <= thr[q]) c[kScoreCols + q] = kAdd ? c[kScoreCols + q] + 1.0 : 1.0;
}

// ---- enqueue: the prediction of stream b into record `row` ------------------------------------------------------------
// The covariance of one step: [sx^2, rho sx sy, sy^2] of the element q = (n, field 0, t, v) of V_pred with field stride
// p_sf, float32 as written (shared with calibrate.hip, which scales it)
__device__ __forceinline__ void score_sig(const float *q, int64_t p_sf, float &sxx, float &sxy, float &syy) {
#pragma clang fp contract(off)
    const float sx = expf(q[2 * p_sf]), sy = expf(q[3 * p_sf]), rho = tanhf(q[4 * p_sf]);
    sxx = sx * sx;
    sxy = rho * sx * sy;
    syy = sy * sy;
}

// One step of the running covariance: (cxx, cxy, cyy) += score_sig (shared with dist_metrics.hip)
__device__ __forceinline__ void score_cov_add(const float *q, int64_t p_sf, float &cxx, float &cxy, float &cyy) {
#pragma clang fp contract(off)
    float sxx, sxy, syy;
    score_sig(q, p_sf, sxx, sxy, syy);
    cxx += sxx;
    cxy += sxy;
    cyy += syy;
}

// The running covariance of column v: C_h = sum_{t<=h} [sx^2, rho sx sy, sy^2]_t, float32, ascending t.  A column that is
// not live (at or past num_peds) reads nothing and carries zeros
__device__ __forceinline__ void score_cov_column(const ScorePred &p, int b, const ScoreRows &t, int row, int v, bool live) {
#pragma clang fp contract(off)
    float cxx = 0.f, cxy = 0.f, cyy = 0.f;
    for (int s = 0; s < t.P; ++s) {
        float *c = t.cov + (((int64_t)row * t.P + s) * t.V + v) * 3;
        if (live) score_cov_add(p.v_pred + b * p.p_sn + v * p.p_sv + s * p.p_sp, p.p_sf, cxx, cxy, cyy);
        c[0] = cxx;
        c[1] = cxy;
        c[2] = cyy;
    }
}

// mean: the columns of the scene's npn pedestrians only (nothing reads a slot at or past num_peds, and a scene of 15 in
// a padding of 128 would otherwise move eight times the bytes).  also(y): the caller's own stores for entry y of the
// (rows,P,V) tables.  By all kScoreThreads threads
template <class Also>
__device__ __forceinline__ void score_copy_mean(const ScorePred &p, int b, const ScoreRows &t, int row, int npn, Also also) {
    const int P = t.P, V = t.V;
    const float2 *src = reinterpret_cast<const float2 *>(p.mean + (int64_t)b * P * V * 2);
    float2 *dst = reinterpret_cast<float2 *>(t.mean + (int64_t)row * P * V * 2);
    for (int e = threadIdx.x; e < P * npn; e += kScoreThreads) {
        const int s = e / npn, x = s * V + (e - s * npn);
        dst[x] = src[x];
        also((int64_t)row * P * V + x);
    }
}

// the K samples (K,NS,P,V,2), the same columns
__device__ __forceinline__ void score_copy_samples(const ScorePred &p, int NS, int b, const ScoreRows &t, int row, int npn) {
    const int P = t.P, K = t.K, pv = P * t.V;
#pragma unroll 4
    for (int e = threadIdx.x; e < K * P * npn; e += kScoreThreads) {
        const int r = e / npn, v = e - r * npn, k = r / P, x = (r - k * P) * t.V + v;               // r = k * P + s
        const float2 *src = reinterpret_cast<const float2 *>(p.samples + ((int64_t)k * NS + b) * pv * 2);
        float2 *dst = reinterpret_cast<float2 *>(t.samples + ((int64_t)row * K + k) * pv * 2);
        dst[x] = src[x];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// The checks every score entry point shares, behind its own check of the sizes: the prediction, thr, the state's sampled
// fields (`sampled`: all there; `sampled_names` for the message), the alignment of the float2 copies and the limits.
// Without samples nothing sample-based is scored: K becomes 0
static inline int score_pred_args(const char *what, ScorePred *p, const float *thr, const float *rec_mean,
                                  const float *rec_samples, bool sampled, const char *sampled_names, int NS, int P, int V,
                                  int *K, int Q) {
    if (!p->samples) *K = 0;
    STG_REQUIRE(p->mean && p->v_pred && p->ids && p->num_peds, STG_EINVAL,
                "%s: null pointer (mean / v_pred / ids / num_peds)", what);
    STG_REQUIRE(*K == 0 || sampled, STG_EINVAL, "%s: null pointer in the state (%s with K=%d)", what, sampled_names, *K);
    STG_REQUIRE(Q == 0 || thr, STG_EINVAL, "%s: null pointer (thr with Q=%d)", what, Q);
    STG_REQUIRE(aligned(p->mean, 8) && aligned(p->samples, 8) && aligned(rec_mean, 8) && aligned(rec_samples, 8),
                STG_EINVAL, "%s: mean / samples and their records must be 8-byte aligned", what);
    STG_REQUIRE(NS <= STG_TRACK_MAX_STREAMS, STG_EUNSUPPORTED, "%s: NS=%d above STG_TRACK_MAX_STREAMS=%d", what, NS,
                STG_TRACK_MAX_STREAMS);
    STG_REQUIRE(V <= STG_SCORE_MAX_V, STG_EUNSUPPORTED, "%s: V=%d above STG_SCORE_MAX_V=%d", what, V, STG_SCORE_MAX_V);
    STG_REQUIRE(*K <= STG_SCORE_MAX_K, STG_EUNSUPPORTED, "%s: K=%d above STG_SCORE_MAX_K=%d", what, *K, STG_SCORE_MAX_K);
    STG_REQUIRE(P <= STG_SCORE_MAX_P, STG_EUNSUPPORTED, "%s: P=%d above STG_SCORE_MAX_P=%d", what, P, STG_SCORE_MAX_P);
    STG_REQUIRE(Q <= STG_SCORE_MAX_Q, STG_EUNSUPPORTED, "%s: Q=%d above STG_SCORE_MAX_Q=%d", what, Q, STG_SCORE_MAX_Q);
    if (*K == 0) p->samples = nullptr;
    return STG_OK;
}

}  // namespace stg
