// dist_metrics: a batch of predictions judged against the ground truth on the device, beside stg_bestofk_eval (DESIGN.md
// 5.31): what best-of-K ADE / FDE cannot say -- whether the predicted Gaussians are calibrated, and whether a scene as a
// whole is predicted well.
//
// The sampler draws the steps independently and sums them (sample_draw.hpp), so the absolute position at horizon h is
// N(mean_h, C_h) with C_h = sum_{t<=h} [sx^2, rho sx sy, sy^2]_t: the record the live score keeps (score_fn.hpp), and the
// closed-form values here ARE its values -- score_cov_add and score_gauss, float32 as written -- so an offline figure and
// a live one are one measurement.
//
//   per element (N,P,V)   cov (optional), d2, nll, lam (the larger eigenvalue of C_h) from v_pred, mean and truth;
//                         kde_nll from the K sampled positions at that horizon: a Gaussian kernel density estimate with
//                         Scott's bandwidth (H = K^(-1/3) S, S the unbiased sample covariance, two passes so that it
//                         does not cancel), det H floored at 2^-15 hxx hyy as score_gauss floors its own (collinear
//                         samples stay finite), the K kernels summed about the nearest sample, the result clipped from
//                         above at kde_floor
//   per pedestrian (N,V)  ade, fde: best-of-K over the given samples (score_dist; min_k of the sum over t, then / P);
//                         optionally ade_ref, fde_ref (float64): the same minima in the arithmetic of the reference's
//                         metrics.ade / fde as predict.sample_test evaluates them on the host -- float32 differences and
//                         squares, a float64 root, a float64 sum over t in ascending t, / P -- so that an offline
//                         evaluation reports sample_test's own figures
//   per scene (N)         jade, jfde: min_k of the scene's summed error, / (c P) and / c; jbest the k of jade
//
// One workgroup per scene, a lane per pedestrian (V <= 256: 64 .. 256 threads, whole waves), so every load of
// samples[k,n,t,:] is contiguous in v and the sum over a scene's pedestrians stays inside the workgroup.  A pedestrian's
// K positions at one horizon are read four times (sample mean, covariance, nearest sample, density) and once more by the
// best-of-K loop; the 8 K V bytes of a horizon stay in the CU's L1 (5 KB at K 20, V 32), so nothing is staged in LDS and
// no register array is sized by K.
//
// The order of the scene sums, fixed: a lane holds ONE pedestrian's sum over t (ascending t); the 64 lanes of a wave are
// added by the xor butterfly 32, 16, .. 1 (the one the score totals use; every lane ends with the same bits); lane 0 of
// each wave leaves its sum in LDS and, behind one barrier, thread 0 adds the waves in ascending order and takes the
// minimum over k in ascending k (a strict <, so the lowest k wins a tie).  No atomics: two runs give the same bits.
// LDS: 2 KB static (K x 4 waves x 2 floats).
#include "score_fn.hpp"

namespace stg {

constexpr int kDistMaxWaves = STG_SCORE_MAX_V / kWave;
constexpr float kLog2Pi = 1.8378770664093453f;

struct DistArgs {
    const float *v_pred;
    int64_t p_sn, p_sf, p_sp, p_sv;
    const float *mean, *samples, *truth;
    const int32_t *num_peds;
    int N, P, V, K;
    float kde_floor, bw, log_k;                  // bw = K^(-1/3) / (K - 1): Scott's factor and the unbiased divisor
    float *cov, *d2, *nll, *lam, *kde_nll, *ade, *fde, *jade, *jfde;
    int32_t *jbest;
    double *ade_ref, *fde_ref;
};

// the sum over the 64 lanes in the order of wave_sum(double), in every lane; needs the whole wave
__device__ __forceinline__ float dist_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float2 ld2(const float *p) { return *reinterpret_cast<const float2 *>(p); }

// the squared distance of (dx, dy) in the metric of H, over the floored determinant
__device__ __forceinline__ float kde_q(float dx, float dy, float hxx, float hxy, float hyy, float det) {
#pragma clang fp contract(off)
    return (hyy * (dx * dx) - 2.f * hxy * dx * dy + hxx * (dy * dy)) / det;
}

// minus the log density at (tx, ty) of the KDE of the K positions s[k * ks], clipped at kde_floor
__device__ __forceinline__ float kde_nll_at(const float *s, int64_t ks, int K, float tx, float ty, float bw, float log_k,
                                            float kde_floor) {
#pragma clang fp contract(off)
    float sx = 0.f, sy = 0.f;
    for (int k = 0; k < K; ++k) {
        const float2 q = ld2(s + k * ks);
        sx += q.x;
        sy += q.y;
    }
    const float mx = sx / (float)K, my = sy / (float)K;
    float sxx = 0.f, sxy = 0.f, syy = 0.f;
    for (int k = 0; k < K; ++k) {
        const float2 q = ld2(s + k * ks);
        const float dx = q.x - mx, dy = q.y - my;
        sxx += dx * dx;
        sxy += dx * dy;
        syy += dy * dy;
    }
    const float hxx = bw * sxx, hxy = bw * sxy, hyy = bw * syy;
    const float p = hxx * hyy;
    const float det = fmaxf(p - hxy * hxy, p * 0x1p-15f);
    float qmin = INFINITY;
    for (int k = 0; k < K; ++k) {
        const float2 q = ld2(s + k * ks);
        qmin = fminf(qmin, kde_q(tx - q.x, ty - q.y, hxx, hxy, hyy, det));
    }
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float2 q = ld2(s + k * ks);
        acc += expf(-0.5f * (kde_q(tx - q.x, ty - q.y, hxx, hxy, hyy, det) - qmin));
    }
    const float val = 0.5f * qmin - logf(acc) + log_k + kLog2Pi + 0.5f * logf(det);
    return val < kde_floor ? val : kde_floor;                 // (a NaN -- all K samples in one point -- is clipped too)
}

__global__ __launch_bounds__(STG_SCORE_MAX_V) void dist_metrics_kernel(const DistArgs a) {
#pragma clang fp contract(off)
    __shared__ float part[STG_SCORE_MAX_K][kDistMaxWaves][2];
    const int n = blockIdx.x, v = threadIdx.x, lane = v & (kWave - 1), wave = v / kWave;
    const int waves = blockDim.x / kWave;
    const int N = a.N, P = a.P, V = a.V, K = a.K;
    int c = a.num_peds ? a.num_peds[n] : V;
    c = c < 0 ? 0 : (c > V ? V : c);
    const bool col = v < V, live = v < c;                     // a column of the outputs; a pedestrian of the scene
    const int64_t pv = (int64_t)P * V;
    const int64_t e0 = (int64_t)n * pv + v;                   // the element (n, 0, v)

    // 1. the closed form
    if (col) {
        float cxx = 0.f, cxy = 0.f, cyy = 0.f;
        for (int t = 0; t < P; ++t) {
            const int64_t e = e0 + (int64_t)t * V;
            float d2 = 0.f, nll = 0.f, lam = 0.f;
            if (live) {
                score_cov_add(a.v_pred + n * a.p_sn + v * a.p_sv + t * a.p_sp, a.p_sf, cxx, cxy, cyy);
                const float2 mu = ld2(a.mean + e * 2), tr = ld2(a.truth + e * 2);
                score_gauss(mu.x - tr.x, mu.y - tr.y, cxx, cxy, cyy, d2, nll);
                const float dd = cxx - cyy;
                lam = 0.5f * (cxx + cyy) + sqrtf(0.25f * (dd * dd) + cxy * cxy);
            }
            a.d2[e] = d2;
            a.nll[e] = nll;
            a.lam[e] = lam;
            if (a.cov) {
                a.cov[e * 3] = cxx;
                a.cov[e * 3 + 1] = cxy;
                a.cov[e * 3 + 2] = cyy;
            }
        }
    }
    if (K == 0) return;                                       // (uniform)

    // 2. the kernel density estimate, horizon by horizon
    const int64_t ks = (int64_t)N * pv * 2;                   // from sample k to sample k + 1
    if (col) {
        for (int t = 0; t < P; ++t) {
            const int64_t e = e0 + (int64_t)t * V;
            float val = 0.f;
            if (live) {
                const float2 tr = ld2(a.truth + e * 2);
                val = kde_nll_at(a.samples + e * 2, ks, K, tr.x, tr.y, a.bw, a.log_k, a.kde_floor);
            }
            a.kde_nll[e] = val;
        }
    }

    // 3. best-of-K per pedestrian and per scene: every thread of the workgroup walks the k loop (the butterfly needs
    //    whole waves); a lane without a pedestrian adds zeros
    float amin = INFINITY, fmin_ = INFINITY;
    double amin_ref = INFINITY, fmin_ref = INFINITY;
    const bool ref = a.ade_ref != nullptr;                    // (uniform)
    for (int k = 0; k < K; ++k) {
        float acc = 0.f, last = 0.f;
        double acc_ref = 0.0, last_ref = 0.0;
        if (live) {
            const float *s = a.samples + k * ks + e0 * 2;
            for (int t = 0; t < P; ++t) {
                const float2 q = ld2(s + (int64_t)t * V * 2), tr = ld2(a.truth + (e0 + (int64_t)t * V) * 2);
                last = score_dist(q.x, q.y, tr.x, tr.y);
                acc += last;
                if (ref) {
                    const float dx = q.x - tr.x, dy = q.y - tr.y;
                    last_ref = sqrt((double)(dx * dx + dy * dy));
                    acc_ref += last_ref;
                }
            }
        }
        amin = fminf(amin, acc);
        fmin_ = fminf(fmin_, last);
        amin_ref = fmin(amin_ref, acc_ref / (double)P);
        fmin_ref = fmin(fmin_ref, last_ref);
        const float sa = dist_wave_sum(acc), sl = dist_wave_sum(last);
        if (lane == 0) {
            part[k][wave][0] = sa;
            part[k][wave][1] = sl;
        }
    }
    if (col) {
        a.ade[(int64_t)n * V + v] = live ? amin / (float)P : 0.f;
        a.fde[(int64_t)n * V + v] = live ? fmin_ : 0.f;
        if (ref) {
            a.ade_ref[(int64_t)n * V + v] = live ? amin_ref : 0.0;
            a.fde_ref[(int64_t)n * V + v] = live ? fmin_ref : 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ja = INFINITY, jf = INFINITY;
        int jb = -1;
        for (int k = 0; k < K; ++k) {
            float sa = part[k][0][0], sl = part[k][0][1];
            for (int w = 1; w < waves; ++w) {
                sa += part[k][w][0];
                sl += part[k][w][1];
            }
            if (sa < ja) {
                ja = sa;
                jb = k;
            }
            jf = fminf(jf, sl);
        }
        a.jade[n] = c > 0 ? ja / (float)(c * P) : 0.f;
        a.jfde[n] = c > 0 ? jf / (float)c : 0.f;
        a.jbest[n] = c > 0 ? jb : -1;
    }
}

}  // namespace stg

extern "C" {

int stg_dist_metrics(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *mean,
                     const float *samples, const float *truth, const int32_t *num_peds, int N, int P, int V, int K,
                     float kde_floor, float *cov, float *d2, float *nll, float *lam, float *kde_nll, float *ade,
                     float *fde, float *jade, float *jfde, int32_t *jbest, double *ade_ref, double *fde_ref,
                     void *stream) {
    using stg::aligned;
    STG_REQUIRE(N >= 0 && P >= 1 && V >= 1 && K >= 0, STG_EINVAL, "stg_dist_metrics: bad sizes N=%d P=%d V=%d K=%d", N, P,
                V, K);
    STG_REQUIRE(K == 0 || K >= 3, STG_EINVAL,
                "stg_dist_metrics: K=%d (a sample covariance and its bandwidth need K >= 3; K = 0: no samples)", K);
    STG_REQUIRE(V <= STG_SCORE_MAX_V, STG_EUNSUPPORTED, "stg_dist_metrics: V=%d above STG_SCORE_MAX_V=%d", V,
                STG_SCORE_MAX_V);
    STG_REQUIRE(K <= STG_SCORE_MAX_K, STG_EUNSUPPORTED, "stg_dist_metrics: K=%d above STG_SCORE_MAX_K=%d", K,
                STG_SCORE_MAX_K);
    STG_REQUIRE(P <= STG_SCORE_MAX_P, STG_EUNSUPPORTED, "stg_dist_metrics: P=%d above STG_SCORE_MAX_P=%d", P,
                STG_SCORE_MAX_P);
    if (N == 0) return STG_OK;
    STG_REQUIRE(v_pred && mean && truth, STG_EINVAL, "stg_dist_metrics: null pointer (v_pred / mean / truth)");
    STG_REQUIRE(d2 && nll && lam, STG_EINVAL, "stg_dist_metrics: null pointer among the outputs (d2 / nll / lam)");
    STG_REQUIRE((K == 0) == (samples == nullptr), STG_EINVAL,
                "stg_dist_metrics: samples and K=%d do not go together (null samples with K = 0)", K);
    STG_REQUIRE(K == 0 || (kde_nll && ade && fde && jade && jfde && jbest), STG_EINVAL,
                "stg_dist_metrics: null pointer among the outputs (kde_nll / ade / fde / jade / jfde / jbest with K=%d)",
                K);
    STG_REQUIRE((ade_ref == nullptr) == (fde_ref == nullptr) && (K > 0 || !ade_ref), STG_EINVAL,
                "stg_dist_metrics: ade_ref and fde_ref go together, and with samples (K=%d)", K);
    STG_REQUIRE(aligned(mean, 8) && aligned(samples, 8) && aligned(truth, 8), STG_EINVAL,
                "stg_dist_metrics: mean / samples / truth must be 8-byte aligned");
    stg::DistArgs a{};
    a.v_pred = v_pred, a.p_sn = p_sn, a.p_sf = p_sf, a.p_sp = p_sp, a.p_sv = p_sv;
    a.mean = mean, a.samples = samples, a.truth = truth, a.num_peds = num_peds;
    a.N = N, a.P = P, a.V = V, a.K = K;
    a.kde_floor = kde_floor;
    if (K > 0) {
        a.bw = (float)(pow((double)K, -1.0 / 3.0) / (double)(K - 1));
        a.log_k = (float)log((double)K);
    }
    a.cov = cov, a.d2 = d2, a.nll = nll, a.lam = lam, a.kde_nll = kde_nll, a.ade = ade, a.fde = fde, a.jade = jade;
    a.jfde = jfde, a.jbest = jbest, a.ade_ref = ade_ref, a.fde_ref = fde_ref;
    const unsigned threads = (unsigned)((V + stg::kWave - 1) / stg::kWave * stg::kWave);
    hipLaunchKernelGGL(stg::dist_metrics_kernel, dim3((unsigned)N), dim3(threads), 0, stg::as_stream(stream), a);
    STG_LAUNCH_CHECK("stg_dist_metrics");
    return STG_OK;
}

}  // extern "C"
