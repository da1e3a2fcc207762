// associate_filter: unlabelled NOISY detections -> track ids on timestamped pushes, with a filtered track state
// (include/stgcnn_hip_assoc_filter.h N13).
//
//   stg_associate_filtered          ONE workgroup on a single stream's arrays
//   stg_associate_streams_filtered  one workgroup per stream on its slices of the (NS, ...) state, its own time and its
//                                   own clock; a stream not pushed returns before the first barrier, its state untouched
//
// The clock, the order test, the rounds and the lifetime are associate_time.hip's: the body is associate.hpp's
// associate_body, here with FilteredMotion.  A slot keeps a constant-velocity Kalman state: the filtered position and
// velocity per model step and the covariance trk_cov = {p00, p01, p11} of one axis, shared by both.  The prediction
// over k steps gives the innovation variance S, and the slot's squared gate min(n2 * S, gmax2) goes to LDS beside its
// predicted position (kSlotGate: 8 bytes more per slot, the only change of the image).  The rounds read that gate
// where the other rules choose between their two.  The predicted covariance and the gain are recomputed in the update
// from the state, as k is: nothing of them is kept in LDS.  Every expression is N13's, one IEEE operation at a time.
// Plain C++ stores, LDS atomics on integer words only, no scratch, no host synchronisation.
#include "associate.hpp"

namespace stg {

struct FilterRule {
    double r, qa, v0, n2, gmax2;
};

// the predicted covariance of one axis over k steps and the innovation variance (N13, 1.)
struct FilterAhead {
    double a00, a01, a11, S;
};
__device__ __forceinline__ FilterAhead filter_ahead(double p00, double p01, double p11, double k, double qa, double r) {
#pragma clang fp contract(off)
    FilterAhead f;
    const double w = qa * k;
    f.a11 = p11 + w;
    const double u = k * p11;
    const double wk = w * k;
    const double h = wk / 2.0;
    const double b = p01 + u;
    f.a01 = b + h;
    const double d = 2.0 * p01;
    const double e = d + u;
    const double g = k * e;
    const double wkk = wk * k;
    const double c = wkk / 3.0;
    const double a = p00 + g;
    f.a00 = a + c;
    f.S = f.a00 + r;
    return f;
}

// The filtered motion: the word is trk_t, as in TimedMotion; t_now is filled in on the device.
struct FilteredMotion {
    int64_t *trk_t;          // (C)
    double *trk_cov;         // (C,3) {p00, p01, p11}
    int64_t t_now, step, max_age;
    FilterRule f;
    using Word = int64_t;
    struct More {
        double vx, vy, p00, p01, p11;
    };
    static constexpr bool kSlotGate = true;
    __device__ __forceinline__ FilteredMotion at(int64_t b, int C, int64_t t) const {
        return {trk_t + b * C, trk_cov + b * C * 3, t, step, max_age, f};
    }
    __device__ __forceinline__ Word word(int s) const { return trk_t[s]; }
    __device__ __forceinline__ double steps(Word t) const {
#pragma clang fp contract(off)
        return (double)(t_now - t) / (double)step;
    }
    // the slot's squared gate (a free slot's is never read)
    __device__ __forceinline__ double gate(int s, double k) const {
#pragma clang fp contract(off)
        const FilterAhead a = filter_ahead(trk_cov[3 * s], trk_cov[3 * s + 1], trk_cov[3 * s + 2], k, f.qa, f.r);
        const double g = f.n2 * a.S;
        return g < f.gmax2 ? g : f.gmax2;
    }
    __device__ __forceinline__ More more(const AssocState &st, int s) const {
        return {st.trk_vel[2 * s], st.trk_vel[2 * s + 1], trk_cov[3 * s], trk_cov[3 * s + 1], trk_cov[3 * s + 2]};
    }
    __device__ __forceinline__ void update(const AssocState &st, int s, Word t, const More &m, double qx, double qy,
                                           double px, double py, double, double) const {
#pragma clang fp contract(off)
        const FilterAhead a = filter_ahead(m.p00, m.p01, m.p11, steps(t), f.qa, f.r);
        const double K0 = a.a00 / a.S, K1 = a.a01 / a.S;
        const double ex = px - qx, ey = py - qy;
        const double cx = K0 * ex, cy = K0 * ey;
        const double dx = K1 * ex, dy = K1 * ey;
        st.trk_pos[2 * s] = qx + cx;
        st.trk_pos[2 * s + 1] = qy + cy;
        st.trk_vel[2 * s] = m.vx + dx;
        st.trk_vel[2 * s + 1] = m.vy + dy;
        const double t00 = K0 * a.a00, t01 = K0 * a.a01, t11 = K1 * a.a01;
        trk_cov[3 * s] = a.a00 - t00;
        trk_cov[3 * s + 1] = a.a01 - t01;
        trk_cov[3 * s + 2] = a.a11 - t11;
        trk_t[s] = t_now;
    }
    __device__ __forceinline__ bool missed(int s, Word t) const {
        const bool gone = t_now - t > max_age;
        if (gone) {
            trk_t[s] = 0;
            trk_cov[3 * s] = trk_cov[3 * s + 1] = trk_cov[3 * s + 2] = 0.0;
        }
        return gone;
    }
    __device__ __forceinline__ void born(int s) const {
        trk_t[s] = t_now;
        trk_cov[3 * s] = f.r;
        trk_cov[3 * s + 1] = 0.0;
        trk_cov[3 * s + 2] = f.v0;
    }
};

__global__ __launch_bounds__(kAssocThreads) void associate_filtered_kernel(
    int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count,
    const int64_t *__restrict__ det_time, const int64_t *__restrict__ clock, int M_max, AssocState st, FilteredMotion mo,
    int C, double scale) {
    const DetectionsOut det{det_id, 1, det_xy, 2};
    const int count = det_count[0];
    const int64_t t_now = det_time[0];
    if (assoc_refused<kAssocThreads>(det, count, M_max, t_now, clock, st.assoc_flags)) return;
    associate_body<kAssocThreads>(det, count, M_max, st, mo.at(0, C, t_now), C, AssocGates{scale, 0.0, 0.0});
}

__global__ __launch_bounds__(kAssocStreamThreads) void associate_streams_filtered_kernel(
    DetectionsOut det, Tick tick, const int64_t *__restrict__ det_time, const int64_t *__restrict__ clock, int M_max,
    AssocState st, FilteredMotion mo, int C, double scale) {
    const int b = blockIdx.x;
    if (tick.pushed_at(b) == 0) return;                     // uniform over the block, ahead of the first barrier
    int lo;
    const int count = tick.range(b, lo);
    const int64_t t_now = det_time[b];
    const AssocState mine = st.of_stream(b, C);
    const DetectionsOut dets = det.from(lo);
    if (assoc_refused<kAssocStreamThreads>(dets, count, M_max, t_now, clock + 2 * (int64_t)b, mine.assoc_flags)) return;
    associate_body<kAssocStreamThreads>(dets, count, M_max, mine, mo.at(b, C, t_now), C, AssocGates{scale, 0.0, 0.0});
}

// the checks the two entry points share: sizes (above the limits: STG_EUNSUPPORTED), the rule, the pointers
static int assoc_filtered_args(const char *what, int M_max, int C, const FilterRule &f, int64_t step, int64_t max_age,
                               const void *det_id, const void *det_xy, const void *det_time, const void *clock,
                               const AssocState &st, const void *trk_t, const void *trk_cov) {
    constexpr double kMax = 1.7976931348623157e308;
    STG_REQUIRE(M_max >= 1 && C >= 1, STG_EINVAL, "%s: bad sizes M_max=%d C=%d", what, M_max, C);
    STG_REQUIRE(M_max <= STG_ASSOC_MAX_DETECTIONS && C <= STG_ASSOC_MAX_SLOTS, STG_EUNSUPPORTED,
                "%s: M_max=%d C=%d above the limits (%d, %d)", what, M_max, C, STG_ASSOC_MAX_DETECTIONS,
                STG_ASSOC_MAX_SLOTS);
    STG_REQUIRE(f.r > 0.0 && f.r <= kMax && f.qa >= 0.0 && f.qa <= kMax && f.v0 > 0.0 && f.v0 <= kMax && f.n2 > 0.0 &&
                    f.n2 <= kMax && f.gmax2 > 0.0 && f.gmax2 <= kMax,
                STG_EINVAL,
                "%s: squared parameters r=%g qa=%g v0=%g n2=%g gmax2=%g: finite, qa >= 0 and the others > 0 expected",
                what, f.r, f.qa, f.v0, f.n2, f.gmax2);
    STG_REQUIRE(step >= 1, STG_EINVAL, "%s: step=%lld ticks (at least 1)", what, (long long)step);
    STG_REQUIRE(step < ((int64_t)1 << 31), STG_EUNSUPPORTED, "%s: step=%lld must stay below 2^31", what,
                (long long)step);
    STG_REQUIRE(max_age >= 0 && max_age < ((int64_t)1 << 31), STG_EINVAL, "%s: max_age=%lld ticks not in [0, 2^31)",
                what, (long long)max_age);
    STG_REQUIRE(det_id && det_xy && det_time && clock && st.trk_id && st.trk_pos && st.trk_vel && trk_t && trk_cov &&
                    st.trk_hits && st.next_id && st.assoc_flags,
                STG_EINVAL, "%s: null pointer", what);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_associate_filtered(int64_t *det_id, const double *det_xy, const int32_t *det_count, const int64_t *det_time,
                           const int64_t *clock, int M_max, int64_t *trk_id, double *trk_pos, double *trk_vel,
                           int64_t *trk_t, double *trk_cov, int32_t *trk_hits, int64_t *next_id, int32_t *assoc_flags,
                           int C, double scale, double r, double qa, double v0, double n2, double gmax2, int64_t step,
                           int64_t max_age, void *stream) {
    const char *what = "stg_associate_filtered";
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    const stg::FilterRule f = {r, qa, v0, n2, gmax2};
    const int rc = stg::assoc_filtered_args(what, M_max, C, f, step, max_age, det_id, det_xy, det_time, clock, st, trk_t,
                                            trk_cov);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_count, STG_EINVAL, "%s: null pointer", what);
    return stg::launch({what, dim3(1), dim3(stg::kAssocThreads), stg::assoc_lds(C, M_max, true),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_filtered_kernel, det_id, det_xy, det_count, det_time, clock, M_max, st,
                       stg::FilteredMotion{trk_t, trk_cov, 0, step, max_age, f}, C, scale);
}

int stg_associate_streams_filtered(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                   int M_total, const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                   const int64_t *clock, int NS, int M_max, int64_t *trk_id, double *trk_pos,
                                   double *trk_vel, int64_t *trk_t, double *trk_cov, int32_t *trk_hits, int64_t *next_id,
                                   int32_t *assoc_flags, int C, double scale, double r, double qa, double v0, double n2,
                                   double gmax2, int64_t step, int64_t max_age, void *stream) {
    const char *what = "stg_associate_streams_filtered";
    int rc = stg::stream_args(what, NS, M_total, id_stride, xy_stride);
    if (rc != STG_OK) return rc;
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    const stg::FilterRule f = {r, qa, v0, n2, gmax2};
    rc = stg::assoc_filtered_args(what, M_max, C, f, step, max_age, det_id, det_xy, det_time, clock, st, trk_t, trk_cov);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_start && pushed, STG_EINVAL, "%s: null pointer", what);
    return stg::launch({what, dim3(NS), dim3(stg::kAssocStreamThreads), stg::assoc_lds(C, M_max, true),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_streams_filtered_kernel, stg::DetectionsOut{det_id, id_stride, det_xy, xy_stride},
                       stg::Tick{det_start, pushed, M_total}, det_time, clock, M_max, st,
                       stg::FilteredMotion{trk_t, trk_cov, 0, step, max_age, f}, C, scale);
}

}  // extern "C"
