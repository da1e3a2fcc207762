// frames_time: the live push with TIME.  stg_track_push of frames.hip takes every push for one model
// step; here a push carries its time in integer ticks and the scene is built "as of now": each pedestrian's position at
// t_now - k * step, k = 0 .. T_obs-1, taken from the track's samples -- a sample at exactly that instant as it is, else
// the linear interpolation of the two samples that bracket it when they are at most max_dt apart.  An instant with
// neither is a missed step and goes through TrackRule (track_rule.hpp): membership by the presence bits, the fill of
// the missed steps from the observed ones.
//
//   stg_track_push_timed          ONE workgroup, the state of one stream: slot ids, per slot a ring of its newest R
//                                 samples (time, rounded position), {next write index, count} per slot, the clock
//   stg_track_push_streams_timed  one workgroup per stream on the (NS, ...) slices, as stg_track_push_streams_rule
//
// The sort and the slot assignment (assign_slots), the padding of a scene and the per-stream wrapper are those of every
// push (track_rule.hpp); a slot is live by its newest sample's age instead of a presence mask.  How a
// slot's samples are indexed, searched and interpolated is time_samples.hpp's, shared with the score and the harvest
// behind this push; the push keeps its own virtual last sample: tb = t_now, the position from the input.
// Everything is read from device memory when the kernel runs -- the time too -- so one captured graph serves every
// push.  Integer work, float64 arithmetic with IEEE operations as written, plain C++ stores, LDS atomics on integer
// words, no scratch, no host synchronisation.
#include "detections.hpp"
#include "track_rule.hpp"
#include "time_samples.hpp"

namespace stg {

constexpr int kFlagTimeOrder = STG_TRACK_TIME_ORDER;

// One timed push of one stream by one workgroup of kThreads threads at the time t_now; the arguments of
// track_push_body with the timed state and sizes (live_args.hpp) in the place of the plain ones.  Returns the flags.
// LDS layout (dynamic): sort keys (M2 x int64), sort indices (M2 x int32), det_slot, det_rank (M_max x int32 each),
// slot masks, free slots, slot heads, slot counts (S x 4 bytes each), found (M_max x T_obs bytes: the logical index of
// the sample at or below each observed instant, so the scene pass does not search again)
template <int kThreads>
__device__ __forceinline__ int track_push_timed_body(const Detections &det, int count, int64_t t_now,
                                                     const TimedState &st, const TimedDims &d, const TrackRule &rule,
                                                     const SceneOut &out) {
    const int M_max = d.M_max, M2 = d.M2, S = d.S, R = d.R, T_obs = d.T_obs, V = d.V;
    const double scale = d.scale;
    const int64_t step = d.step, max_dt = d.max_dt;
    int64_t *slot_id = st.slot_id, *t_ring = st.t_ring, *clock = st.clock, *out_ids = out.out_ids;
    double *xy_ring = st.xy_ring, *obs_abs = out.obs_abs;
    int32_t *slot_head = st.slot_head, *head_flags = st.head_flags, *seen = out.seen;
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + M2);
    int32_t *det_slot = kidx + M2;
    int32_t *det_rank = det_slot + M_max;
    uint32_t *smask = reinterpret_cast<uint32_t *>(det_rank + M_max);
    int32_t *free_list = reinterpret_cast<int32_t *>(smask + S);
    int32_t *shead = free_list + S;
    int32_t *scnt = shead + S;
    uint8_t *found = reinterpret_cast<uint8_t *>(scnt + S);
    __shared__ int wave_cnt[kThreads / kWave];
    __shared__ int flags;

    const int tid = threadIdx.x, nt = blockDim.x;
    const uint32_t full = T_obs >= 32 ? 0xffffffffu : (1u << T_obs) - 1u;
    const int64_t last = clock[0], pushes = clock[1];

    // 0. time must move forward (the first push takes any time): otherwise the empty scene and no change of state.
    //    Uniform over the block, ahead of every barrier.
    if (pushes > 0 && t_now <= last) {
        pad_scene(out, T_obs, V, 0);
        if (tid == 0) {
            out.num_peds[0] = 0;
            head_flags[1] = kFlagTimeOrder;
        }
        return kFlagTimeOrder;
    }

    int m = count;
    const bool truncated = m > M_max;
    m = m < 0 ? 0 : (m > M_max ? M_max : m);
    if (tid == 0) flags = truncated ? kFlagTruncated : 0;

    // 1. a slot whose newest sample is older than T_obs - 1 steps is free, its ring empty.  Load the detections into
    //    the sort buffer (padding keys sort last).
    const int64_t span = (int64_t)(T_obs - 1) * step;
    for (int s = tid; s < S; s += nt) {
        int h = slot_head[2 * s], c = slot_head[2 * s + 1];
        if (c > 0 && t_now - t_ring[(int64_t)s * R + ring_before(h, R)] > span) {
            h = c = 0;
            slot_id[s] = -1;
            slot_head[2 * s] = 0;
            slot_head[2 * s + 1] = 0;
        }
        smask[s] = 0;
        shead[s] = h;
        scnt[s] = c;
    }
    const int n2 = det_sort_n(m);                           // (<= M2)
    det_load(key, kidx, det, m, n2, tid, nt);
    for (int j = tid; j < m; j += nt) det_slot[j] = -1;
    __syncthreads();

    // 2-4. every detection gets its slot (assign_slots); a slot is live while its ring holds a sample
    assign_slots<kThreads>(key, kidx, det_slot, free_list, wave_cnt, &flags, m, n2, S, slot_id,
                           [&](int s) { return scnt[s] != 0; });

    // 5. record this push's sample (time, rounded position) at the slot's write index; the ring entry it overwrites is
    //    outside what the search below reads (n_old <= R - 1), so the two need no barrier between them
    for (int j = tid; j < m; j += nt) {
        const int s = det_slot[j];
        if (s < 0) continue;
        const int h = shead[s], c = scnt[s];
        const int64_t at = (int64_t)s * R + h;
        slot_id[s] = det.id_at(j);
        atomicOr(&smask[s], 1u);
        t_ring[at] = t_now;
        xy_ring[at * 2] = round_pos(det.x(j), scale);
        xy_ring[at * 2 + 1] = round_pos(det.y(j), scale);
        slot_head[2 * s] = h + 1 == R ? 0 : h + 1;
        slot_head[2 * s + 1] = c < R ? c + 1 : R;
    }

    // 6. one thread per (detection with a slot, earlier window step k): the search of the instant in the slot's times
    //    (time_samples.hpp).  Observed: a sample at the instant, or its neighbours at most max_dt apart.
    const int T1 = T_obs - 1;
    for (int e = tid; e < m * T1; e += nt) {
        const int j = e / T1, k = e % T1;
        const int s = det_slot[j];
        if (s < 0) continue;
        const int c = scnt[s], n_old = c < R - 1 ? c : R - 1, h = shead[s];
        const int64_t tau = t_now - (int64_t)(T1 - k) * step;
        const int64_t *tr = t_ring + (int64_t)s * R;
        const int i = last_at_or_before(tr, h, n_old, R, tau);
        if (i < 0) continue;
        const int64_t ta = tr[ring_at(h, n_old, i, R)];
        const int64_t tb = i + 1 < n_old ? tr[ring_at(h, n_old, i + 1, R)] : t_now;
        if (ta == tau || tb - ta <= max_dt) {
            atomicOr(&smask[s], 1u << (T1 - k));
            found[j * T_obs + k] = (uint8_t)i;
        }
    }
    __syncthreads();

    // 7. the scene: the rule's members in ascending id order (the sorted detections), the first V of them
    int c = 0, tot = 0;
    for (int p0 = 0; p0 < m; p0 += nt) {
        const int p = p0 + tid;
        const int j = p < m ? kidx[p] : 0;
        const int s = p < m ? det_slot[j] : -1;
        const bool in = s >= 0 && rule.member(smask[s]);
        const int r = block_rank<kThreads>(in, c, &tot, wave_cnt);
        if (p < m) det_rank[j] = in && r < V ? r : -1;
        if (in && r < V) {
            out_ids[r] = key[p];
            seen[r] = (int32_t)smask[s];
        }
        c += tot;
    }
    if (c > V && tid == 0) atomicOr(&flags, kFlagTooMany);
    const int np = c < V ? c : V;
    __syncthreads();

    // 8. one thread per (member, observed step): the sample at the instant, or the interpolation of its bracket; this
    //    push's own sample comes from the input (the ring entry written above is another thread's store)
    for (int e = tid; e < m * T_obs; e += nt) {
        const int j = e / T_obs, k = e % T_obs;
        const int r = det_rank[j];
        if (r < 0) continue;
        const int s = det_slot[j];
        if (((smask[s] >> (T1 - k)) & 1u) == 0) continue;
        const double nx = round_pos(det.x(j), scale), ny = round_pos(det.y(j), scale);
        double x = nx, y = ny;
        if (k < T1) {
            const int cs = scnt[s], n_old = cs < R - 1 ? cs : R - 1, h = shead[s], i = found[j * T_obs + k];
            const int64_t tau = t_now - (int64_t)(T1 - k) * step;
            const int64_t a = (int64_t)s * R + ring_at(h, n_old, i, R);
            const int64_t ta = t_ring[a];
            x = xy_ring[a * 2];
            y = xy_ring[a * 2 + 1];
            if (ta != tau) {
                int64_t tb = t_now;
                double bx = nx, by = ny;
                if (i + 1 < n_old) {
                    const int64_t b = (int64_t)s * R + ring_at(h, n_old, i + 1, R);
                    tb = t_ring[b];
                    bx = xy_ring[b * 2];
                    by = xy_ring[b * 2 + 1];
                }
                lerp_bracket(ta, x, y, tb, bx, by, tau, scale, x, y);
            }
        }
        obs_abs[((int64_t)k * V + r) * 2] = x;
        obs_abs[((int64_t)k * V + r) * 2 + 1] = y;
    }
    __syncthreads();

    // 9. a member with missed steps: TrackRule::fill in place (a seen step is read before it is written)
    for (int j = tid; j < m; j += nt) {
        const int r = det_rank[j];
        if (r < 0) continue;
        const uint32_t pm = smask[det_slot[j]];
        if (pm == full) continue;
        TrackRule::fill(
            pm, T_obs, scale,
            [&](int t, double &x, double &y) {
                x = obs_abs[((int64_t)t * V + r) * 2];
                y = obs_abs[((int64_t)t * V + r) * 2 + 1];
            },
            [&](int t, double x, double y) {
                obs_abs[((int64_t)t * V + r) * 2] = x;
                obs_abs[((int64_t)t * V + r) * 2 + 1] = y;
            });
    }
    pad_scene(out, T_obs, V, np);
    __syncthreads();
    if (tid == 0) {
        out.num_peds[0] = np;
        head_flags[1] = flags;
        clock[0] = t_now;
        clock[1] = pushes + 1;
    }
    return flags;
}

__global__ __launch_bounds__(kPushThreads) void track_push_timed_kernel(
    const int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count,
    const int64_t *__restrict__ det_time, TimedState st, TimedDims d, TrackRule rule, SceneOut out) {
    track_push_timed_body<kPushThreads>({det_id, 1, det_xy, 2}, det_count[0], det_time[0], st, d, rule, out);
}

// One workgroup per stream (push_stream): a stream not pushed keeps its state, its clock included
template <int kThreads>
__global__ __launch_bounds__(kThreads) void track_push_streams_timed_kernel(
    Detections det, Tick tick, const int64_t *__restrict__ det_time, TimedState st, TimedDims d, TrackRule rule,
    SceneOut out, int32_t *__restrict__ out_flags) {
    push_stream(det, tick, out, d.T_obs, d.V, out_flags, [&](const Detections &mine, int count, const SceneOut &scene) {
        const int b = blockIdx.x;
        return track_push_timed_body<kThreads>(mine, count, det_time[b], st.of_stream(b, d.S, d.R), d, rule, scene);
    });
}

// dynamic LDS of a timed push: the sort arrays, det_slot and det_rank, four words per slot, one byte per
// (detection, step)
static inline size_t push_timed_lds(const TimedDims &d) {
    return det_sort_lds(d.M2) + (size_t)d.M_max * 2 * sizeof(int32_t) + (size_t)d.S * 4 * sizeof(int32_t) +
           (size_t)d.M_max * d.T_obs;
}

// the checks the two entry points share (`counts`: the push's det_count, or the streams' det_start and pushed); fills d.M2
static int timed_args(const char *what, const TrackRule &rule, const Detections &det, bool counts,
                      const int64_t *det_time, const TimedState &st, TimedDims &d, const SceneOut &out) {
    const int M_max = d.M_max, S = d.S, R = d.R, T_obs = d.T_obs, V = d.V, min_seen = rule.min_seen,
              max_gap = rule.max_gap;
    const int64_t step = d.step, max_dt = d.max_dt;
    STG_REQUIRE(M_max >= 1 && M_max <= STG_TRACK_MAX_DETECTIONS && S >= 1 && S <= STG_TRACK_MAX_SLOTS && V >= 1,
                STG_EINVAL, "%s: bad sizes M_max=%d S=%d V=%d", what, M_max, S, V);
    STG_REQUIRE_RULE(what);
    const int rc = timed_size_args(what, R, step, T_obs, "T_obs");
    if (rc != STG_OK) return rc;
    STG_REQUIRE(max_dt >= 1 && max_dt <= (int64_t)(T_obs - 1) * step, STG_EINVAL,
                "%s: max_dt=%lld not in [1, (T_obs - 1) * step = %lld]", what, (long long)max_dt,
                (long long)((int64_t)(T_obs - 1) * step));
    STG_REQUIRE(det.id && det.xy && counts && det_time && st.slot_id && st.t_ring && st.xy_ring && st.slot_head &&
                    st.clock && st.head_flags && out.obs_abs && out.out_ids && out.num_peds && out.seen,
                STG_EINVAL, "%s: null pointer", what);
    d.M2 = det_sort_n(M_max);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_track_push_timed(const int64_t *det_id, const double *det_xy, const int32_t *det_count,
                         const int64_t *det_time, int M_max, int64_t *slot_id, int64_t *t_ring, double *xy_ring,
                         int32_t *slot_head, int64_t *clock, int32_t *head_flags, int S, int R, int T_obs, double scale,
                         int V, int64_t step, int64_t max_dt, int min_seen, int max_gap, double *obs_abs,
                         int64_t *out_ids, int32_t *num_peds, int32_t *seen, void *stream) {
    const char *what = "stg_track_push_timed";
    const stg::Detections det{det_id, 1, det_xy, 2};
    const stg::TimedState st{slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    const stg::TrackRule rule{min_seen, max_gap};
    const stg::SceneOut out{obs_abs, out_ids, num_peds, seen};
    stg::TimedDims d{{M_max, 0, S, T_obs, V, scale}, R, step, max_dt};
    const int rc = stg::timed_args(what, rule, det, det_count != nullptr, det_time, st, d, out);
    if (rc != STG_OK) return rc;
    return stg::launch({what, dim3(1), dim3(stg::kPushThreads), stg::push_timed_lds(d), stg::as_stream(stream), 64 * 1024},
                       stg::track_push_timed_kernel, det_id, det_xy, det_count, det_time, st, d, rule, out);
}

int stg_track_push_streams_timed(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                 int M_total, const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                 int NS, int M_max, int64_t *slot_id, int64_t *t_ring, double *xy_ring,
                                 int32_t *slot_head, int64_t *clock, int32_t *head_flags, int S, int R, int T_obs,
                                 double scale, int V, int64_t step, int64_t max_dt, int min_seen, int max_gap,
                                 double *obs_abs, int64_t *out_ids, int32_t *num_peds, int32_t *out_flags,
                                 int32_t *seen, int block_threads, void *stream) {
    const char *what = "stg_track_push_streams_timed";
    const stg::Detections det{det_id, id_stride, det_xy, xy_stride};
    const stg::Tick tick{det_start, pushed, M_total};
    const stg::TimedState st{slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    const stg::TrackRule rule{min_seen, max_gap};
    const stg::SceneOut out{obs_abs, out_ids, num_peds, seen};
    stg::TimedDims d{{M_max, 0, S, T_obs, V, scale}, R, step, max_dt};
    int rc = stg::push_streams_args(what, NS, M_total, id_stride, xy_stride, block_threads);
    if (rc == STG_OK) rc = stg::timed_args(what, rule, det, det_start && pushed, det_time, st, d, out);
    if (rc != STG_OK) return rc;
    const stg::Launch l{what, dim3(NS), dim3(block_threads), stg::push_timed_lds(d), stg::as_stream(stream), 64 * 1024};
    return stg::with_stream_threads(block_threads, [&](auto kt) {
        return stg::launch(l, stg::track_push_streams_timed_kernel<kt()>, det, tick, det_time, st, d, rule, out,
                           out_flags);
    });
}

}  // extern "C"
