// associate_time: unlabelled detections -> track ids on TIMESTAMPED pushes, the front end of the timed live push
// (include/stgcnn_hip_assoc_time.h N12).
//
//   stg_associate_timed          ONE workgroup on a single stream's arrays
//   stg_associate_streams_timed  one workgroup per stream on its slices of the (NS, ...) state, its own time and its
//                                own clock; a stream not pushed returns before the first barrier, its state untouched
//
// The rule, the rounds and the LDS image are those of associate.hip: the body is associate.hpp's associate_body, here
// with TimedMotion.  A slot remembers the TIME of its last match, trk_t, and the number of model steps since then is
// k = (double)(t_now - trk_t) / (double)step, one IEEE division; the velocity is the displacement per step.  k is
// computed where it is used, in the prediction and again in the update, from trk_t: nothing of it is kept in LDS.  A
// slot not matched is freed once t_now - trk_t > max_age and otherwise left alone.
//
// The launch runs ahead of the timed push and makes that push's own order test on the clock the push keeps (read only
// here): a push that is not after the stream's last accepted one changes nothing, gets ids of -1 and the flag
// STG_ASSOC_TIME_ORDER.  The test is uniform over the block and ahead of the first barrier.  Everything, the time
// included, is read from device memory when the kernel runs.  Plain C++ stores, LDS atomics on integer words only, no
// scratch, no host synchronisation.
#include "associate.hpp"

namespace stg {

// The timed motion: the word is trk_t, the time of the slot's last match.  t_now is filled in on the device.
struct TimedMotion {
    int64_t *trk_t;          // (C)
    int64_t t_now, step, max_age;
    using Word = int64_t;
    using More = AssocNoMore;
    static constexpr bool kSlotGate = false;
    __device__ __forceinline__ More more(const AssocState &, int) const { return {}; }
    __device__ __forceinline__ void update(const AssocState &st, int s, Word t, const More &, double, double, double px,
                                           double py, double ox, double oy) const {
        assoc_two_sample(st, s, steps(t), px, py, ox, oy);
        matched(s);
    }
    __device__ __forceinline__ TimedMotion at(int64_t b, int C, int64_t t) const {
        return {trk_t + b * C, t, step, max_age};
    }
    __device__ __forceinline__ Word word(int s) const { return trk_t[s]; }
    __device__ __forceinline__ double steps(Word t) const {
#pragma clang fp contract(off)
        return (double)(t_now - t) / (double)step;
    }
    __device__ __forceinline__ void matched(int s) const { trk_t[s] = t_now; }
    __device__ __forceinline__ bool missed(int s, Word t) const {
        const bool gone = t_now - t > max_age;
        if (gone) trk_t[s] = 0;
        return gone;
    }
    __device__ __forceinline__ void born(int s) const { trk_t[s] = t_now; }
};

__global__ __launch_bounds__(kAssocThreads) void associate_timed_kernel(
    int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count,
    const int64_t *__restrict__ det_time, const int64_t *__restrict__ clock, int M_max, AssocState st, TimedMotion mo,
    int C, AssocGates rule) {
    const DetectionsOut det{det_id, 1, det_xy, 2};
    const int count = det_count[0];
    const int64_t t_now = det_time[0];
    if (assoc_refused<kAssocThreads>(det, count, M_max, t_now, clock, st.assoc_flags)) return;
    associate_body<kAssocThreads>(det, count, M_max, st, mo.at(0, C, t_now), C, rule);
}

__global__ __launch_bounds__(kAssocStreamThreads) void associate_streams_timed_kernel(
    DetectionsOut det, Tick tick, const int64_t *__restrict__ det_time, const int64_t *__restrict__ clock, int M_max,
    AssocState st, TimedMotion mo, int C, AssocGates rule) {
    const int b = blockIdx.x;
    if (tick.pushed_at(b) == 0) return;                     // uniform over the block, ahead of the first barrier
    int lo;
    const int count = tick.range(b, lo);
    const int64_t t_now = det_time[b];
    const AssocState mine = st.of_stream(b, C);
    const DetectionsOut dets = det.from(lo);
    if (assoc_refused<kAssocStreamThreads>(dets, count, M_max, t_now, clock + 2 * (int64_t)b, mine.assoc_flags)) return;
    associate_body<kAssocStreamThreads>(dets, count, M_max, mine, mo.at(b, C, t_now), C, rule);
}

// the checks the two entry points share: sizes (above the limits: STG_EUNSUPPORTED), the rule, the pointers
static int assoc_timed_args(const char *what, int M_max, int C, double gate2, double gate_new2, int64_t step,
                            int64_t max_age, const void *det_id, const void *det_xy, const void *det_time,
                            const void *clock, const AssocState &st, const void *trk_t) {
    STG_REQUIRE(M_max >= 1 && C >= 1, STG_EINVAL, "%s: bad sizes M_max=%d C=%d", what, M_max, C);
    STG_REQUIRE(M_max <= STG_ASSOC_MAX_DETECTIONS && C <= STG_ASSOC_MAX_SLOTS, STG_EUNSUPPORTED,
                "%s: M_max=%d C=%d above the limits (%d, %d)", what, M_max, C, STG_ASSOC_MAX_DETECTIONS,
                STG_ASSOC_MAX_SLOTS);
    STG_REQUIRE(gate2 > 0.0 && gate2 <= 1.7976931348623157e308 && gate_new2 >= gate2 &&
                    gate_new2 <= 1.7976931348623157e308,
                STG_EINVAL, "%s: squared gates %g, %g: finite, gate2 > 0 and gate_new2 >= gate2 expected", what, gate2,
                gate_new2);
    STG_REQUIRE(step >= 1, STG_EINVAL, "%s: step=%lld ticks (at least 1)", what, (long long)step);
    STG_REQUIRE(step < ((int64_t)1 << 31), STG_EUNSUPPORTED, "%s: step=%lld must stay below 2^31", what,
                (long long)step);
    STG_REQUIRE(max_age >= 0 && max_age < ((int64_t)1 << 31), STG_EINVAL, "%s: max_age=%lld ticks not in [0, 2^31)",
                what, (long long)max_age);
    STG_REQUIRE(det_id && det_xy && det_time && clock && st.trk_id && st.trk_pos && st.trk_vel && trk_t &&
                    st.trk_hits && st.next_id && st.assoc_flags,
                STG_EINVAL, "%s: null pointer", what);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_associate_timed(int64_t *det_id, const double *det_xy, const int32_t *det_count, const int64_t *det_time,
                        const int64_t *clock, int M_max, int64_t *trk_id, double *trk_pos, double *trk_vel,
                        int64_t *trk_t, int32_t *trk_hits, int64_t *next_id, int32_t *assoc_flags, int C, double scale,
                        double gate2, double gate_new2, int64_t step, int64_t max_age, void *stream) {
    const char *what = "stg_associate_timed";
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    const int rc = stg::assoc_timed_args(what, M_max, C, gate2, gate_new2, step, max_age, det_id, det_xy, det_time,
                                         clock, st, trk_t);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_count, STG_EINVAL, "%s: null pointer", what);
    return stg::launch({what, dim3(1), dim3(stg::kAssocThreads), stg::assoc_lds(C, M_max), stg::as_stream(stream),
                        63 * 1024},
                       stg::associate_timed_kernel, det_id, det_xy, det_count, det_time, clock, M_max, st,
                       stg::TimedMotion{trk_t, 0, step, max_age}, C, stg::AssocGates{scale, gate2, gate_new2});
}

int stg_associate_streams_timed(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride, int M_total,
                                const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                const int64_t *clock, int NS, int M_max, int64_t *trk_id, double *trk_pos,
                                double *trk_vel, int64_t *trk_t, int32_t *trk_hits, int64_t *next_id,
                                int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int64_t step,
                                int64_t max_age, void *stream) {
    const char *what = "stg_associate_streams_timed";
    int rc = stg::stream_args(what, NS, M_total, id_stride, xy_stride);
    if (rc != STG_OK) return rc;
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    rc = stg::assoc_timed_args(what, M_max, C, gate2, gate_new2, step, max_age, det_id, det_xy, det_time, clock, st,
                               trk_t);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_start && pushed, STG_EINVAL, "%s: null pointer", what);
    return stg::launch({what, dim3(NS), dim3(stg::kAssocStreamThreads), stg::assoc_lds(C, M_max),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_streams_timed_kernel, stg::DetectionsOut{det_id, id_stride, det_xy, xy_stride},
                       stg::Tick{det_start, pushed, M_total}, det_time, clock, M_max, st,
                       stg::TimedMotion{trk_t, 0, step, max_age}, C, stg::AssocGates{scale, gate2, gate_new2});
}

}  // extern "C"
