// frames: per-frame prediction scenes from raw tracks, the reference's windowing (utils.py:123-165) with the future
// dropped -- at frame index f the scene is every pedestrian id with a row in each of the frames f-T_obs+1 .. f, in
// ascending id order, positions rounded as np.around(x, 4) (utils.py:145: rint(x * 1e4) / 1e4 in float64).
//
//   stg_frame_scene_counts  recording: one wave per frame; every row of frame f looks its id up (binary search) in the
//                           id-sorted rows of each of the T_obs - 1 frames before -> count[f].  Memory stays linear in
//                           the rows (no ids x frames table: long recordings hold tens of thousands of ids).
//   stg_frame_scenes        recording: one wave per selected frame; the fully observed rows of the frame are compacted
//                           in id order (ballot + popcount under the lane mask) into obs_abs / ids / num_peds.
//   stg_track_push          live stream: ONE workgroup keeps the track state on the device (slot ids, presence masks,
//                           a position ring) and turns one frame of detections into that frame's scene.  The detection
//                           count is read from device memory, so a captured graph replays with a different count.
//   stg_track_push_streams  NS live streams: one workgroup per stream runs the same push (track_push_body) on the
//                           stream's slice of the state and its range of one packed tick of detections; the counts,
//                           offsets and pushed flags are read from device memory, so one captured graph serves a tick.
// The pushes sort their detections and look ids up with detections.hpp, as the score kernels do; the
// slot assignment, the padding of a scene, the per-stream wrapper and the host's stream checks are those of every push
// (track_rule.hpp), the argument records those of the whole live path (live_args.hpp).
//
// Partially observed tracks: TrackRule (track_rule.hpp) admits a pedestrian with a short history or tracker gaps
// and fills the frames it missed.  stg_fill_tracks applies the fill to a batch in place; the *_rule entry points are
// the two recording kernels and the two pushes with the rule in the place of "seen in each of the T_obs frames", plus
// a `seen` output (the presence bits of every scene slot).  The strict entry points launch the strict code.
//
// Pure data movement and integer work: a few KB per frame.  No host synchronisation in the launch functions (the push
// is captured into the per-frame graph of FramePredictor.capture) and plain C++ stores only.
#include "detections.hpp"
#include "track_rule.hpp"

namespace stg {

// row index of `id` in frame g (frame_start offsets, ids sorted by id inside each frame), or -1
__device__ __forceinline__ int row_of(const int32_t *__restrict__ fs, const int64_t *__restrict__ ids, int g, int64_t id) {
    const int lo = fs[g], at = det_find(ids + lo, fs[g + 1] - lo, id);
    return at < 0 ? -1 : lo + at;
}

// One lane per (scene, pedestrian): the column's missed steps filled in place, its seen steps rounded.  A column past
// the scene's count, not seen now or seen only once is left as it is.
__global__ __launch_bounds__(256) void fill_tracks_kernel(double *__restrict__ obs_abs, const int32_t *__restrict__ seen,
                                                          const int32_t *__restrict__ num_peds, int N, int T_obs, int V,
                                                          double scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * V) return;
    const int n = (int)(i / V), v = (int)(i % V);
    if (num_peds && v >= num_peds[n]) return;
    const uint32_t full = T_obs >= 32 ? 0xffffffffu : (1u << T_obs) - 1u;
    const uint32_t m = (uint32_t)seen[i] & full;
    if (!TrackRule{2, T_obs - 2}.member(m)) return;
    double *col = obs_abs + ((int64_t)n * T_obs * V + v) * 2;           // step stride V * 2
    TrackRule::fill(
        m, T_obs, scale,
        [&](int t, double &x, double &y) {
            x = round_pos(col[(int64_t)t * V * 2], scale);
            y = round_pos(col[(int64_t)t * V * 2 + 1], scale);
        },
        [&](int t, double x, double y) {
            col[(int64_t)t * V * 2] = x;
            col[(int64_t)t * V * 2 + 1] = y;
        });
}

// ---- recording ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void frame_scene_counts_kernel(const int32_t *__restrict__ fs,
                                                                const int64_t *__restrict__ ids, int T_obs,
                                                                int32_t *__restrict__ count) {
    const int f = blockIdx.x;
    int c = 0;
    if (f >= T_obs - 1) {
        for (int r = fs[f] + (int)threadIdx.x; r < fs[f + 1]; r += kWave) {
            const int64_t id = ids[r];
            bool full = true;
            for (int g = f - 1; g > f - T_obs && full; --g) full = row_of(fs, ids, g, id) >= 0;
            c += full ? 1 : 0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    if (threadIdx.x == 0) count[f] = c;
}

__global__ __launch_bounds__(64) void frame_scenes_kernel(const int32_t *__restrict__ fs, const int64_t *__restrict__ ids,
                                                          const double *__restrict__ xy,
                                                          const int32_t *__restrict__ frames, int V, int T_obs,
                                                          double scale, double *__restrict__ obs_abs,
                                                          int64_t *__restrict__ out_ids, int32_t *__restrict__ num_peds) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int f = frames[n];
    double *obs = obs_abs + (int64_t)n * T_obs * V * 2;          // (T_obs, V, 2)
    int64_t *oid = out_ids + (int64_t)n * V;
    int base = 0;
    // rows of frame f in id order, 64 at a time: every lane of the wave runs the loop (uniform trip count)
    for (int r0 = fs[f]; r0 < fs[f + 1]; r0 += kWave) {
        const int r = r0 + lane;
        const bool real = r < fs[f + 1];
        const int64_t id = real ? ids[r] : 0;
        bool full = real && f >= T_obs - 1;
        for (int g = f - 1; g > f - T_obs && full; --g) full = row_of(fs, ids, g, id) >= 0;
        const uint64_t m = __ballot(full);
        const int slot = base + lanes_below(m);
        if (full && slot < V) {
            oid[slot] = id;
            for (int t = 0; t < T_obs; ++t) {
                const int g = f - T_obs + 1 + t;
                const int q = t == T_obs - 1 ? r : row_of(fs, ids, g, id);
                obs[((int64_t)t * V + slot) * 2] = round_pos(xy[(int64_t)q * 2], scale);
                obs[((int64_t)t * V + slot) * 2 + 1] = round_pos(xy[(int64_t)q * 2 + 1], scale);
            }
        }
        base += __popcll(m);
    }
    const int c = base < V ? base : V;
    for (int s = c + lane; s < V; s += kWave) {
        oid[s] = -1;
        for (int t = 0; t < T_obs; ++t) {
            obs[((int64_t)t * V + s) * 2] = 0.0;
            obs[((int64_t)t * V + s) * 2 + 1] = 0.0;
        }
    }
    if (lane == 0) num_peds[n] = c;
}

// The recording kernels under a TrackRule.  presence bits of `id`, a row of frame f: bit k = a row in frame f - k
// (frames before the recording's first count as missed).
__device__ __forceinline__ uint32_t presence_bits(const int32_t *__restrict__ fs, const int64_t *__restrict__ ids, int f,
                                                  int T_obs, int64_t id) {
    uint32_t m = 1u;
    for (int k = 1; k < T_obs && k <= f; ++k) m |= row_of(fs, ids, f - k, id) >= 0 ? 1u << k : 0u;
    return m;
}

__global__ __launch_bounds__(64) void frame_scene_counts_rule_kernel(const int32_t *__restrict__ fs,
                                                                     const int64_t *__restrict__ ids, int T_obs,
                                                                     TrackRule rule, int32_t *__restrict__ count) {
    const int f = blockIdx.x;
    int c = 0;
    if (f >= rule.min_seen - 1)
        for (int r = fs[f] + (int)threadIdx.x; r < fs[f + 1]; r += kWave)
            c += rule.member(presence_bits(fs, ids, f, T_obs, ids[r])) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    if (threadIdx.x == 0) count[f] = c;
}

__global__ __launch_bounds__(64) void frame_scenes_rule_kernel(
    const int32_t *__restrict__ fs, const int64_t *__restrict__ ids, const double *__restrict__ xy,
    const int32_t *__restrict__ frames, int V, int T_obs, double scale, TrackRule rule, double *__restrict__ obs_abs,
    int64_t *__restrict__ out_ids, int32_t *__restrict__ num_peds, int32_t *__restrict__ seen) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int f = frames[n];
    double *obs = obs_abs + (int64_t)n * T_obs * V * 2;          // (T_obs, V, 2)
    int64_t *oid = out_ids + (int64_t)n * V;
    int32_t *osn = seen + (int64_t)n * V;
    int base = 0;
    for (int r0 = fs[f]; r0 < fs[f + 1]; r0 += kWave) {
        const int r = r0 + lane;
        const bool real = r < fs[f + 1];
        const int64_t id = real ? ids[r] : 0;
        const uint32_t pm = real ? presence_bits(fs, ids, f, T_obs, id) : 0u;
        const bool in = real && f >= rule.min_seen - 1 && rule.member(pm);
        const uint64_t m = __ballot(in);
        const int slot = base + lanes_below(m);
        if (in && slot < V) {
            oid[slot] = id;
            osn[slot] = (int32_t)pm;
            TrackRule::fill(
                pm, T_obs, scale,
                [&](int t, double &x, double &y) {
                    const int q = t == T_obs - 1 ? r : row_of(fs, ids, f - T_obs + 1 + t, id);
                    x = round_pos(xy[(int64_t)q * 2], scale);
                    y = round_pos(xy[(int64_t)q * 2 + 1], scale);
                },
                [&](int t, double x, double y) {
                    obs[((int64_t)t * V + slot) * 2] = x;
                    obs[((int64_t)t * V + slot) * 2 + 1] = y;
                });
        }
        base += __popcll(m);
    }
    const int c = base < V ? base : V;
    for (int s = c + lane; s < V; s += kWave) {
        oid[s] = -1;
        osn[s] = 0;
        for (int t = 0; t < T_obs; ++t) {
            obs[((int64_t)t * V + s) * 2] = 0.0;
            obs[((int64_t)t * V + s) * 2 + 1] = 0.0;
        }
    }
    if (lane == 0) num_peds[n] = c;
}

// ---- live streams ------------------------------------------------------------------------------------------------
// The strict scene's column `obs` (step stride V * 2) <- the T_obs - 1 earlier ring rows (stride S * 2) of a slot, oldest
// first.  __restrict__ PARAMETERS: a record's members cannot say that scene and ring do not alias.
__device__ __forceinline__ void gather_ring(double *__restrict__ obs, const double *__restrict__ ring, int head, int S,
                                            int T_obs, int V) {
    for (int t = 0; t < T_obs - 1; ++t) {
        const int row = (head + 1 + t) % T_obs;           // head - (T_obs - 1 - t) mod T_obs
        obs[(int64_t)t * V * 2] = ring[(int64_t)row * S * 2];
        obs[(int64_t)t * V * 2 + 1] = ring[(int64_t)row * S * 2 + 1];
    }
}

// One push of one stream by one workgroup of kThreads threads: `count` detections of `det` (more than M_max: the first
// M_max, flag TRUNCATED), the stream's own state and scene (live_args.hpp).  Returns (in every thread) the flags.
// LDS layout (dynamic): sort keys (M2 x int64), sort indices (M2 x int32), det_slot (M_max x int32),
// slot masks (S x uint32), free slots (S x int32)
// kRule: the scene phase admits and fills by `rule` and writes the presence bits of every scene slot to out.seen (V);
// without it (the strict entry points) neither is looked at.
template <int kThreads, bool kRule>
__device__ __forceinline__ int track_push_body(const Detections &det, int count, const TrackState &st, const PushDims &d,
                                               const TrackRule &rule, const SceneOut &out) {
    const int M_max = d.M_max, M2 = d.M2, S = d.S, T_obs = d.T_obs, V = d.V;
    const double scale = d.scale;
    int64_t *slot_id = st.slot_id, *out_ids = out.out_ids;
    uint32_t *mask = st.mask;
    double *ring = st.ring, *obs_abs = out.obs_abs;
    int32_t *head_flags = st.head_flags, *seen = out.seen;
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + M2);
    int32_t *det_slot = kidx + M2;
    uint32_t *smask = reinterpret_cast<uint32_t *>(det_slot + M_max);
    int32_t *free_list = reinterpret_cast<int32_t *>(smask + S);
    __shared__ int wave_cnt[kThreads / kWave];
    __shared__ int flags;

    const int tid = threadIdx.x, nt = blockDim.x;
    const uint32_t full = T_obs >= 32 ? 0xffffffffu : (1u << T_obs) - 1u;
    int m = count;
    const bool truncated = m > M_max;
    m = m < 0 ? 0 : (m > M_max ? M_max : m);
    const int head = (head_flags[0] + 1) % T_obs;          // ring row of this frame
    if (tid == 0) flags = truncated ? kFlagTruncated : 0;

    // 1. age the presence masks (bit t = seen t frames ago); a slot with no presence in the last T_obs - 1 frames
    //    is free.  Load the detections into the sort buffer (padding keys sort last).
    for (int s = tid; s < S; s += nt) {
        const uint32_t mk = (mask[s] << 1) & full;
        smask[s] = mk;
        if (mk == 0) slot_id[s] = -1;
    }
    const int n2 = det_sort_n(m);                           // (<= M2)
    det_load(key, kidx, det, m, n2, tid, nt);
    for (int j = tid; j < m; j += nt) det_slot[j] = -1;
    __syncthreads();

    // 2-4. every detection gets its slot (assign_slots: the one rule of the pushes); a slot is live by its mask
    assign_slots<kThreads>(key, kidx, det_slot, free_list, wave_cnt, &flags, m, n2, S, slot_id,
                           [&](int s) { return smask[s] != 0; });

    // 5. record this frame: id, presence bit 0, rounded position in the ring row `head`
    for (int j = tid; j < m; j += nt) {
        const int s = det_slot[j];
        if (s < 0) continue;
        slot_id[s] = det.id_at(j);
        smask[s] |= 1u;
        ring[((int64_t)head * S + s) * 2] = round_pos(det.x(j), scale);
        ring[((int64_t)head * S + s) * 2 + 1] = round_pos(det.y(j), scale);
    }
    __syncthreads();

    // 6. the scene: slots seen in each of the last T_obs frames, in ascending id order (the sorted detections), the
    //    first V of them; gather their T_obs positions, oldest first
    int c = 0, tot = 0;
    for (int p0 = 0; p0 < m; p0 += nt) {
        const int p = p0 + tid;
        const int j = p < m ? kidx[p] : 0;
        const int s = p < m ? det_slot[j] : -1;
        bool in;
        if constexpr (kRule) in = s >= 0 && rule.member(smask[s]);
        else in = s >= 0 && (smask[s] & full) == full;
        const int r = block_rank<kThreads>(in, c, &tot, wave_cnt);
        if constexpr (kRule) {
            // the rule's scene: the ring rows of the seen frames only (a missed frame's row is stale), this frame's
            // position from the input as below
            if (in && r < V) {
                const uint32_t pm = smask[s];
                out_ids[r] = key[p];
                seen[r] = (int32_t)pm;
                TrackRule::fill(
                    pm, T_obs, scale,
                    [&](int t, double &x, double &y) {
                        if (t == T_obs - 1) {
                            x = round_pos(det.x(j), scale);
                            y = round_pos(det.y(j), scale);
                        } else {
                            const int row = (head + 1 + t) % T_obs;
                            x = ring[((int64_t)row * S + s) * 2];
                            y = ring[((int64_t)row * S + s) * 2 + 1];
                        }
                    },
                    [&](int t, double x, double y) {
                        obs_abs[((int64_t)t * V + r) * 2] = x;
                        obs_abs[((int64_t)t * V + r) * 2 + 1] = y;
                    });
            }
        } else if (in && r < V) {
            out_ids[r] = key[p];
            gather_ring(obs_abs + r * 2, ring + s * 2, head, S, T_obs, V);
            // this frame's position from the input (the ring row written above is another thread's store)
            obs_abs[((int64_t)(T_obs - 1) * V + r) * 2] = round_pos(det.x(j), scale);
            obs_abs[((int64_t)(T_obs - 1) * V + r) * 2 + 1] = round_pos(det.y(j), scale);
        }
        c += tot;
    }
    if (c > V && tid == 0) atomicOr(&flags, kFlagTooMany);
    const int np = c < V ? c : V;
    pad_scene(out, T_obs, V, np);
    for (int s = tid; s < S; s += nt) mask[s] = smask[s];
    __syncthreads();
    if (tid == 0) {
        out.num_peds[0] = np;
        head_flags[0] = head;
        head_flags[1] = flags;
    }
    return flags;
}

// One kernel per (single | streams) push; kRule picks the strict or the rule's scene phase of the body, and the strict
// instantiation reads neither `rule` nor out.seen.
template <bool kRule>
__global__ __launch_bounds__(kPushThreads) void track_push_kernel(
    const int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count,
    TrackState st, PushDims d, TrackRule rule, SceneOut out) {
    if constexpr (!kRule) out.seen = nullptr;
    track_push_body<kPushThreads, kRule>({det_id, 1, det_xy, 2}, det_count[0], st, d, rule, out);
}

// One workgroup per stream (push_stream): every stream's records are its own slices of the (NS, ...) arrays.
template <int kThreads, bool kRule>
__global__ __launch_bounds__(kThreads) void track_push_streams_kernel(Detections det, Tick tick, TrackState st, PushDims d,
                                                                      TrackRule rule, SceneOut out,
                                                                      int32_t *__restrict__ out_flags) {
    if constexpr (!kRule) out.seen = nullptr;
    push_stream(det, tick, out, d.T_obs, d.V, out_flags,
                [&](const Detections &mine, int count, const SceneOut &scene) {
                    return track_push_body<kThreads, kRule>(mine, count, st.of_stream(blockIdx.x, d), d, rule, scene);
                });
}

// ---- the pushes' entry points ---------------------------------------------------------------------------------------
// Each pair (strict, *_rule) shares one function for its checks and its launch, under its own name `what`.  Without
// `ruled` (the strict entry point) T_obs starts at 1, the rule and `seen` are not looked at and the strict kernel runs.
// dynamic LDS of a push: the sort arrays of M2 entries, det_slot, slot masks, free slots.  At most 48 KB (M_max = S =
// 2048: 24 + 8 + 16), below the 64 KB a kernel may use without asking: the launches name that limit and never raise it
static inline size_t push_lds(const PushDims &d) {
    return det_sort_lds(d.M2) + (size_t)d.M_max * sizeof(int32_t) + (size_t)d.S * (sizeof(uint32_t) + sizeof(int32_t));
}

// the checks the two pushes share (`counts`: the push's det_count, or the streams' det_start and pushed); fills d.M2.
// A strict push has no `seen` (its entry points pass null, and its kernels null the member: pad_scene looks at it).
static int push_args(const char *what, bool ruled, const TrackRule &rule, const Detections &det, bool counts,
                     const TrackState &st, PushDims &d, const SceneOut &out) {
    const int T_obs = d.T_obs, min_seen = rule.min_seen, max_gap = rule.max_gap;
    STG_REQUIRE(d.M_max >= 1 && d.M_max <= STG_TRACK_MAX_DETECTIONS && d.S >= 1 && d.S <= STG_TRACK_MAX_SLOTS &&
                    d.V >= 1 && (ruled || (T_obs >= 1 && T_obs <= 32)),
                STG_EINVAL, "%s: bad sizes M_max=%d S=%d V=%d T_obs=%d", what, d.M_max, d.S, d.V, T_obs);
    if (ruled) STG_REQUIRE_RULE(what);
    STG_REQUIRE(det.id && det.xy && counts && st.slot_id && st.mask && st.ring && st.head_flags && out.obs_abs &&
                    out.out_ids && out.num_peds && (out.seen != nullptr) == ruled,
                STG_EINVAL, "%s: null pointer", what);
    d.M2 = det_sort_n(d.M_max);
    return STG_OK;
}

static int track_push(const char *what, bool ruled, TrackRule rule, Detections det, const int32_t *det_count,
                      TrackState st, PushDims d, SceneOut out, void *stream) {
    const int rc = push_args(what, ruled, rule, det, det_count != nullptr, st, d, out);
    if (rc != STG_OK) return rc;
    return launch({what, dim3(1), dim3(kPushThreads), push_lds(d), as_stream(stream), 64 * 1024},
                  ruled ? track_push_kernel<true> : track_push_kernel<false>, det.id, det.xy, det_count, st, d, rule, out);
}

static int track_push_streams(const char *what, bool ruled, TrackRule rule, Detections det, Tick tick, int NS,
                              TrackState st, PushDims d, SceneOut out, int32_t *out_flags, int block_threads,
                              void *stream) {
    int rc = push_streams_args(what, NS, tick.M_total, det.id_stride, det.xy_stride, block_threads);
    if (rc == STG_OK) rc = push_args(what, ruled, rule, det, tick.det_start && tick.pushed, st, d, out);
    if (rc != STG_OK) return rc;
    const Launch l{what, dim3(NS), dim3(block_threads), push_lds(d), as_stream(stream), 64 * 1024};
    // the workgroup size picks the instantiation, `ruled` the kernel of the pair
    return with_stream_threads(block_threads, [&](auto kt) {
        return launch(l, ruled ? track_push_streams_kernel<kt(), true> : track_push_streams_kernel<kt(), false>, det,
                      tick, st, d, rule, out, out_flags);
    });
}

}  // namespace stg

extern "C" {

int stg_frame_scene_counts(const int32_t *frame_start, const int64_t *ids, int F, int T_obs, int32_t *count,
                           void *stream) {
    STG_REQUIRE(F >= 0 && T_obs >= 1, STG_EINVAL, "stg_frame_scene_counts: bad sizes F=%d T_obs=%d", F, T_obs);
    if (F == 0) return STG_OK;
    STG_REQUIRE(frame_start && ids && count, STG_EINVAL, "stg_frame_scene_counts: null pointer");
    return stg::launch({"stg_frame_scene_counts", dim3(F), dim3(stg::kWave), 0, stg::as_stream(stream)},
                       stg::frame_scene_counts_kernel, frame_start, ids, T_obs, count);
}

int stg_frame_scenes(const int32_t *frame_start, const int64_t *ids, const double *xy, const int32_t *frames, int N,
                     int V, int T_obs, double scale, double *obs_abs, int64_t *out_ids, int32_t *num_peds,
                     void *stream) {
    STG_REQUIRE(N >= 0 && V > 0 && T_obs >= 1, STG_EINVAL, "stg_frame_scenes: bad sizes N=%d V=%d T_obs=%d", N, V,
                T_obs);
    if (N == 0) return STG_OK;
    STG_REQUIRE(frame_start && ids && xy && frames && obs_abs && out_ids && num_peds, STG_EINVAL,
                "stg_frame_scenes: null pointer");
    return stg::launch({"stg_frame_scenes", dim3(N), dim3(stg::kWave), 0, stg::as_stream(stream)},
                       stg::frame_scenes_kernel, frame_start, ids, xy, frames, V, T_obs, scale, obs_abs, out_ids,
                       num_peds);
}

int stg_track_push(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, int64_t *slot_id,
                   uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs, double scale, int V,
                   double *obs_abs, int64_t *out_ids, int32_t *num_peds, void *stream) {
    return stg::track_push("stg_track_push", false, {}, {det_id, 1, det_xy, 2}, det_count,
                           {slot_id, mask, ring, head_flags}, {M_max, 0, S, T_obs, V, scale},
                           {obs_abs, out_ids, num_peds, nullptr}, stream);
}

int stg_track_push_streams(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                           int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                           int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                           double scale, int V, double *obs_abs, int64_t *out_ids, int32_t *num_peds,
                           int32_t *out_flags, int block_threads, void *stream) {
    return stg::track_push_streams("stg_track_push_streams", false, {}, {det_id, id_stride, det_xy, xy_stride},
                                   {det_start, pushed, M_total}, NS, {slot_id, mask, ring, head_flags},
                                   {M_max, 0, S, T_obs, V, scale}, {obs_abs, out_ids, num_peds, nullptr}, out_flags,
                                   block_threads, stream);
}

// ---- partially observed tracks: the rule's entry points -------------------------------------------------------------
int stg_fill_tracks(double *obs_abs, const int32_t *seen, const int32_t *num_peds, int N, int T_obs, int V,
                    double scale, void *stream) {
    STG_REQUIRE(N >= 0 && V >= 1 && T_obs >= 2 && T_obs <= 32 && (int64_t)N * V < ((int64_t)1 << 31) * 256, STG_EINVAL,
                "stg_fill_tracks: bad sizes N=%d T_obs=%d V=%d", N, T_obs, V);
    if (N == 0) return STG_OK;
    STG_REQUIRE(obs_abs && seen, STG_EINVAL, "stg_fill_tracks: null pointer");
    const int64_t blocks = ((int64_t)N * V + 255) / 256;
    return stg::launch({"stg_fill_tracks", dim3((unsigned)blocks), dim3(256), 0, stg::as_stream(stream)},
                       stg::fill_tracks_kernel, obs_abs, seen, num_peds, N, T_obs, V, scale);
}

int stg_frame_scene_counts_rule(const int32_t *frame_start, const int64_t *ids, int F, int T_obs, int min_seen,
                                int max_gap, int32_t *count, void *stream) {
    STG_REQUIRE(F >= 0, STG_EINVAL, "stg_frame_scene_counts_rule: bad size F=%d", F);
    STG_REQUIRE_RULE("stg_frame_scene_counts_rule");
    if (F == 0) return STG_OK;
    STG_REQUIRE(frame_start && ids && count, STG_EINVAL, "stg_frame_scene_counts_rule: null pointer");
    return stg::launch({"stg_frame_scene_counts_rule", dim3(F), dim3(stg::kWave), 0, stg::as_stream(stream)},
                       stg::frame_scene_counts_rule_kernel, frame_start, ids, T_obs, stg::TrackRule{min_seen, max_gap},
                       count);
}

int stg_frame_scenes_rule(const int32_t *frame_start, const int64_t *ids, const double *xy, const int32_t *frames,
                          int N, int V, int T_obs, double scale, int min_seen, int max_gap, double *obs_abs,
                          int64_t *out_ids, int32_t *num_peds, int32_t *seen, void *stream) {
    STG_REQUIRE(N >= 0 && V > 0, STG_EINVAL, "stg_frame_scenes_rule: bad sizes N=%d V=%d", N, V);
    STG_REQUIRE_RULE("stg_frame_scenes_rule");
    if (N == 0) return STG_OK;
    STG_REQUIRE(frame_start && ids && xy && frames && obs_abs && out_ids && num_peds && seen, STG_EINVAL,
                "stg_frame_scenes_rule: null pointer");
    return stg::launch({"stg_frame_scenes_rule", dim3(N), dim3(stg::kWave), 0, stg::as_stream(stream)},
                       stg::frame_scenes_rule_kernel, frame_start, ids, xy, frames, V, T_obs, scale,
                       stg::TrackRule{min_seen, max_gap}, obs_abs, out_ids, num_peds, seen);
}

int stg_track_push_rule(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max,
                        int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                        double scale, int V, int min_seen, int max_gap, double *obs_abs, int64_t *out_ids,
                        int32_t *num_peds, int32_t *seen, void *stream) {
    return stg::track_push("stg_track_push_rule", true, {min_seen, max_gap}, {det_id, 1, det_xy, 2}, det_count,
                           {slot_id, mask, ring, head_flags}, {M_max, 0, S, T_obs, V, scale},
                           {obs_abs, out_ids, num_peds, seen}, stream);
}

int stg_track_push_streams_rule(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                                int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                                double scale, int V, int min_seen, int max_gap, double *obs_abs, int64_t *out_ids,
                                int32_t *num_peds, int32_t *out_flags, int32_t *seen, int block_threads,
                                void *stream) {
    return stg::track_push_streams("stg_track_push_streams_rule", true, {min_seen, max_gap},
                                   {det_id, id_stride, det_xy, xy_stride}, {det_start, pushed, M_total}, NS,
                                   {slot_id, mask, ring, head_flags}, {M_max, 0, S, T_obs, V, scale},
                                   {obs_abs, out_ids, num_peds, seen}, out_flags, block_threads, stream);
}

}  // extern "C"
