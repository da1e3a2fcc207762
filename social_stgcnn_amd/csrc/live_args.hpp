// live_args: the argument records of the live path (frames.hip, frames_time.hip, score.hip, score_time.hip,
// associate.hip, harvest.hip, harvest_time.hip): plain structs passed by value as kernel arguments
// in the place of runs of same-typed pointers.  THE ONE SLICING RULE: a record that lives in (NS, ...) arrays has an
// of_stream(b, ...) (the detections: from(lo)), the only place its per-stream strides are written; a body only ever
// sees its own stream's record.  On the host, stream_args is the one check of what the _streams entry points are told
// about their streams, timed_size_args the one check of the track rings' depth and the step.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace stg {

// Detections j = 0, 1, ...: (id[j * id_stride], xy[j * xy_stride], xy[j * xy_stride + 1]); a single stream's (M),
// (M,2) arrays are {det_id, 1, det_xy, 2}.  Id = int64_t for the kernel that writes the ids (associate.hip).
template <class Id>
struct DetectionsOf {
    Id *id;
    int64_t id_stride;
    const double *xy;
    int64_t xy_stride;

    __device__ __forceinline__ DetectionsOf from(int lo) const {          // the detections from the lo-th on
        return {id + lo * id_stride, id_stride, xy + lo * xy_stride, xy_stride};
    }
    __device__ __forceinline__ Id &id_at(int j) const { return id[j * id_stride]; }
    __device__ __forceinline__ double x(int j) const { return xy[j * xy_stride]; }
    __device__ __forceinline__ double y(int j) const { return xy[j * xy_stride + 1]; }
};
using Detections = DetectionsOf<const int64_t>;
using DetectionsOut = DetectionsOf<int64_t>;

// One packed tick of NS streams: stream b holds detections det_start[b] .. det_start[b+1]-1 and takes part when
// pushed[b] != 0.
struct Tick {
    const int32_t *det_start, *pushed;
    int M_total;

    __device__ __forceinline__ int pushed_at(int b) const { return pushed[b]; }
    // stream b's range clamped to [0, M_total): first, and the count
    __device__ __forceinline__ int range(int b, int &first) const {
        const int lo = det_start[b], hi = det_start[b + 1];
        first = lo < 0 ? 0 : (lo > M_total ? M_total : lo);
        return (hi < first ? first : (hi > M_total ? M_total : hi)) - first;
    }
};

// The sizes of a push: at most M_max detections (M2 = det_sort_n(M_max), filled in on the host), S slots, T_obs steps,
// scenes padded to V, positions rounded by scale.  The timed push adds R samples per slot, the step and max_dt in ticks.
struct PushDims { int M_max, M2, S, T_obs, V; double scale; };
struct TimedDims : PushDims { int R; int64_t step, max_dt; };

// The state of a push (frames.hip): slot_id (S), mask (S), ring (T_obs,S,2), head_flags (2)
struct TrackState {
    int64_t *slot_id; uint32_t *mask; double *ring; int32_t *head_flags;
    __device__ __forceinline__ TrackState of_stream(int64_t b, const PushDims &d) const {
        return {slot_id + b * d.S, mask + b * d.S, ring + b * d.T_obs * d.S * 2, head_flags + 2 * b};
    }
};

// ... of a timed push: slot_id (S), t_ring (S,R), xy_ring (S,R,2), slot_head (S,2) = {next write index, count} per slot,
// clock (2), head_flags (2).  kConst: the same state as the kernels behind the push read it (harvest_time.hip,
// score_time.hip; time_samples.hpp reads a slot's samples out of it): nothing of it is written.
template <bool kConst>
struct TimedStateOf {
    template <class T> using Ptr = std::conditional_t<kConst, const T, T> *;
    Ptr<int64_t> slot_id, t_ring; Ptr<double> xy_ring; Ptr<int32_t> slot_head; Ptr<int64_t> clock; Ptr<int32_t> head_flags;
    __device__ __forceinline__ TimedStateOf of_stream(int64_t b, int S, int R) const {
        return {slot_id + b * S,       t_ring + b * S * R, xy_ring + b * S * R * 2,
                slot_head + b * S * 2, clock + 2 * b,      head_flags + 2 * b};
    }
};
using TimedState = TimedStateOf<false>;
using TimedView = TimedStateOf<true>;

// The scene a push leaves: obs_abs (T_obs,V,2), out_ids (V), num_peds (1), seen (V; null in the strict pushes)
struct SceneOut {
    double *obs_abs; int64_t *out_ids; int32_t *num_peds, *seen;
    __device__ __forceinline__ SceneOut of_stream(int64_t b, int T_obs, int V) const {
        return {obs_abs + b * T_obs * V * 2, out_ids + b * V, num_peds + b, seen ? seen + b * V : nullptr};
    }
};

// ---- the window harvest (harvest.hip) ------------------------------------------------------------------
// The sizes of a harvest: S slots, the push's T_obs, windows of T_all steps, at least min_peds rows each
struct HarvestDims { int S, T_obs, T_all, min_peds; };

// The push's state as the harvest reads it, behind that push: nothing of it is written
struct TrackView {
    const int64_t *slot_id; const uint32_t *mask; const double *ring; const int32_t *head_flags;
    __device__ __forceinline__ TrackView of_stream(int64_t b, const HarvestDims &d) const {
        return {slot_id + b * d.S, mask + b * d.S, ring + b * d.T_obs * d.S * 2, head_flags + 2 * b};
    }
};

// The harvest's own history: word (S), ring (T_all,S,2), head (2) = {ring row of the last push, pushes since reset}
struct HarvestState {
    uint32_t *word; double *ring; int32_t *head;
    __device__ __forceinline__ HarvestState of_stream(int64_t b, const HarvestDims &d) const {
        return {word + b * d.S, ring + b * d.T_all * d.S * 2, head + 2 * b};
    }
};

// What a tick's launches hand each other, one int32 array: cand (NS,S) the candidates' slots in id order, count (NS)
// the rows of the stream's window (0: none), place (NS,2) = {first row in the log or -1, window index}
struct HarvestWork {
    int32_t *cand, *count, *place;
    static __host__ __device__ __forceinline__ HarvestWork carve(int32_t *work, int64_t NS, int S) {
        return {work, work + NS * S, work + NS * S + NS};
    }
    __device__ __forceinline__ HarvestWork of_stream(int64_t b, const HarvestDims &d) const {
        return {cand + b * d.S, count + b, place + 2 * b};
    }
};

// The log, one for all streams (no of_stream): rel_all (cap_rows,2,T_all), win_start (cap_windows + 1), win_tag
// (cap_windows,2), header (3) = {n_windows, n_rows, dropped_full}
struct HarvestLog {
    float *rel_all; int32_t *win_start, *win_tag, *header;
    int cap_windows, cap_rows;
};

// ---- the timed window harvest (harvest_time.hip) --------------------------------------------------------
// What the timed harvest adds to HarvestDims: R samples per slot, the push's scale, step, max_dt and settle in ticks
struct TimedHarvestDims { int R; double scale; int64_t step, max_dt, settle; };

// ---- host side ------------------------------------------------------------------------------------------------------
// What every _streams entry point checks of its streams, under its own name `what`: NS, M_total and the strides.  The
// entry points do not all answer alike, and each keeps its answer:
//   min_NS   1 for the pushes and the association; 0 for stg_score_push_streams, which returns STG_OK on NS == 0
//   limits   NS and M_total above their limits are STG_EINVAL here; not for stg_score_push_streams (false), which
//            answers STG_EUNSUPPORTED, behind the checks of its other arguments, and so makes those two checks itself
static inline int stream_args(const char *what, int NS, int M_total, int64_t id_stride, int64_t xy_stride,
                              int min_NS = 1, bool limits = true) {
    STG_REQUIRE(NS >= min_NS && M_total >= 0 && id_stride >= 1 && xy_stride >= 2 &&
                    (!limits || (NS <= STG_TRACK_MAX_STREAMS && M_total <= STG_TRACK_MAX_TOTAL_DETECTIONS)),
                STG_EINVAL, "%s: bad sizes NS=%d M_total=%d strides %lld/%lld", what, NS, M_total, (long long)id_stride,
                (long long)xy_stride);
    return STG_OK;
}

// What the timed push (frames_time.hip), the timed harvest (harvest_time.hip) and the timed score (score_time.hip) are
// told alike about the track rings and the step, under the entry point's name `what`, in the order of the push:
// R >= 2; R <= STG_TRACK_MAX_HISTORY (STG_EUNSUPPORTED); step >= 1; step and step * n below 2^31 (STG_EUNSUPPORTED),
// where n, called n_name in the message, is T_obs for the push and the harvest and P for the score.  The bounds that
// differ between the families stay with them: max_dt in [1, (T_obs - 1) * step] for the push and the harvest, the
// harvest's settle, max_dt in [1, 2^31) for the score.
static inline int timed_size_args(const char *what, int R, int64_t step, int n, const char *n_name) {
    STG_REQUIRE(R >= 2, STG_EINVAL, "%s: R=%d samples per track (at least 2)", what, R);
    STG_REQUIRE(R <= STG_TRACK_MAX_HISTORY, STG_EUNSUPPORTED, "%s: R=%d above STG_TRACK_MAX_HISTORY=%d", what, R,
                STG_TRACK_MAX_HISTORY);
    STG_REQUIRE(step >= 1, STG_EINVAL, "%s: step=%lld ticks (at least 1)", what, (long long)step);
    STG_REQUIRE(step < ((int64_t)1 << 31) && step * n < ((int64_t)1 << 31), STG_EUNSUPPORTED,
                "%s: step=%lld: step * %s must stay below 2^31", what, (long long)step, n_name);
    return STG_OK;
}

}  // namespace stg
