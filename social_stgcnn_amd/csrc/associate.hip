// associate: unlabelled detections -> track ids on the device, the front end of the live pushes.
//
//   stg_associate          ONE workgroup on a single stream's arrays
//   stg_associate_streams  one workgroup per stream on its slices of the (NS, ...) state and its range of one packed
//                          tick; a stream not pushed returns before the first barrier, its state untouched
//
// The rule: a per-stream tracker with constant-velocity prediction and gated, globally greedy nearest-neighbour
// matching -- the candidates (cost <= the track's squared gate) taken in ascending (cost, track slot, detection) order,
// each accepted when its track and its detection are both still free.  The kernel reaches that matching in rounds:
// every free track remembers its best free detection, min (cost, j), every free detection its best free track,
// min (cost, s); a pair that is each other's best is accepted.  The smallest remaining candidate is always such a
// pair, so every round with a candidate left accepts at least one, and after min(live tracks, m) rounds nothing is
// left: that is the loop's bound.  A row or column is rescanned only when its remembered partner was taken, by a group
// of 8 lanes that split its partners and reduce (cost, index) by shuffles.
//
// Everything is read from device memory when the kernel runs (count, ranges, state), the ids are written into the
// caller's det_id array, which the push and score launches behind it read.  Plain C++ stores, LDS atomics on integer
// words only, no scratch, no host synchronisation.
//
// The body, associate_body, is a template over a motion policy in associate.hpp, shared with the timed kernels of
// associate_time.hip; here it runs with PushMotion: every push is one step, trk_miss counts the pushes since the match.
#include "associate.hpp"

namespace stg {


__global__ __launch_bounds__(kAssocThreads) void associate_kernel(
    int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count, int M_max,
    AssocState st, PushMotion mo, int C, AssocGates rule) {
    associate_body<kAssocThreads>({det_id, 1, det_xy, 2}, det_count[0], M_max, st, mo, C, rule);
}

__global__ __launch_bounds__(kAssocStreamThreads) void associate_streams_kernel(DetectionsOut det, Tick tick, int M_max,
                                                                                AssocState st, PushMotion mo, int C,
                                                                                AssocGates rule) {
    const int b = blockIdx.x;
    if (tick.pushed_at(b) == 0) return;                     // uniform over the block, ahead of the first barrier
    int lo;
    const int count = tick.range(b, lo);
    associate_body<kAssocStreamThreads>(det.from(lo), count, M_max, st.of_stream(b, C), mo.of_stream(b, C), C, rule);
}

// the checks the two entry points share: sizes (above the limits: STG_EUNSUPPORTED), the rule, the pointers
static int assoc_args(const char *what, int M_max, int C, double gate2, double gate_new2, int max_miss,
                      const void *det_id, const void *det_xy, const AssocState &st, const void *trk_miss) {
    STG_REQUIRE(M_max >= 1 && C >= 1, STG_EINVAL, "%s: bad sizes M_max=%d C=%d", what, M_max, C);
    STG_REQUIRE(M_max <= STG_ASSOC_MAX_DETECTIONS && C <= STG_ASSOC_MAX_SLOTS, STG_EUNSUPPORTED,
                "%s: M_max=%d C=%d above the limits (%d, %d)", what, M_max, C, STG_ASSOC_MAX_DETECTIONS,
                STG_ASSOC_MAX_SLOTS);
    STG_REQUIRE(gate2 > 0.0 && gate2 <= 1.7976931348623157e308 && gate_new2 >= gate2 &&
                    gate_new2 <= 1.7976931348623157e308,
                STG_EINVAL, "%s: squared gates %g, %g: finite, gate2 > 0 and gate_new2 >= gate2 expected", what, gate2,
                gate_new2);
    STG_REQUIRE(max_miss >= 0, STG_EINVAL, "%s: max_miss=%d (at least 0)", what, max_miss);
    STG_REQUIRE(det_id && det_xy && st.trk_id && st.trk_pos && st.trk_vel && trk_miss && st.trk_hits &&
                    st.next_id && st.assoc_flags,
                STG_EINVAL, "%s: null pointer", what);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_associate(int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, int64_t *trk_id,
                  double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                  int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                  void *stream) {
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    const int rc = stg::assoc_args("stg_associate", M_max, C, gate2, gate_new2, max_miss, det_id, det_xy, st, trk_miss);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_count, STG_EINVAL, "stg_associate: null pointer");
    return stg::launch({"stg_associate", dim3(1), dim3(stg::kAssocThreads), stg::assoc_lds(C, M_max),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_kernel, det_id, det_xy, det_count, M_max, st, stg::PushMotion{trk_miss, max_miss},
                       C, stg::AssocGates{scale, gate2, gate_new2});
}

int stg_associate_streams(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride, int M_total,
                          const int32_t *det_start, const int32_t *pushed, int NS, int M_max, int64_t *trk_id,
                          double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                          int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                          void *stream) {
    int rc = stg::stream_args("stg_associate_streams", NS, M_total, id_stride, xy_stride);
    if (rc != STG_OK) return rc;
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_hits, next_id, assoc_flags};
    rc = stg::assoc_args("stg_associate_streams", M_max, C, gate2, gate_new2, max_miss, det_id, det_xy, st, trk_miss);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_start && pushed, STG_EINVAL, "stg_associate_streams: null pointer");
    return stg::launch({"stg_associate_streams", dim3(NS), dim3(stg::kAssocStreamThreads), stg::assoc_lds(C, M_max),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_streams_kernel, stg::DetectionsOut{det_id, id_stride, det_xy, xy_stride},
                       stg::Tick{det_start, pushed, M_total}, M_max, st, stg::PushMotion{trk_miss, max_miss}, C,
                       stg::AssocGates{scale, gate2, gate_new2});
}

}  // extern "C"
