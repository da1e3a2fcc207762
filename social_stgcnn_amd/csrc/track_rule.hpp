// track_rule: what the live pushes share (frames.hip: one push = one model step; frames_time.hip: timestamped pushes,
// DESIGN.md 5.20) beyond the detection sort of detections.hpp -- the workgroup sizes and flags of a push, the block-wide
// rank, TrackRule, the rule for partially observed tracks, which the recording kernels use too, and the
// parts of a push that do not depend on its state: the slot assignment, the padding of a scene, the
// per-stream wrapper and, on the host, the stream checks and the workgroup-size dispatch of the _streams entry points.
// Device helpers without state, as in detections.hpp: the caller owns the LDS arrays and its thread geometry.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "detections.hpp"

namespace stg {

constexpr int kPushThreads = 1024;
constexpr int kPushWaves = kPushThreads / kWave;
// workgroup of stg_track_push_streams when the caller passes block_threads = 0 (measured)
constexpr int kStreamThreads = 256;
constexpr int kFlagDuplicate = STG_TRACK_DUPLICATE, kFlagOverflow = STG_TRACK_OVERFLOW,
              kFlagTruncated = STG_TRACK_TRUNCATED, kFlagTooMany = STG_TRACK_TOO_MANY;

// lanes below this one whose bit is set in a wave ballot
__device__ __forceinline__ int lanes_below(uint64_t m) {
    const int lane = threadIdx.x & (kWave - 1);
    return __popcll(m & ((1ull << lane) - 1ull));
}

// ---- the rule for partially observed tracks ------------------------------------------------------------------------
// Presence bits m of one pedestrian over the T_obs-frame window: bit t = seen t frames ago (bit 0 = this frame), the
// orientation of the state's masks; window step t (oldest first) is bit T_obs - 1 - t.
//   member  seen now, in at least min_seen frames of the window, and no run of missed frames between two seen ones
//           longer than max_gap (missed frames ahead of the first seen one are no gap)
//   fill    the window with every missed step filled, in float64 with IEEE operations as written (no fused
//           multiply-add): an interior step t between the nearest seen steps a < t < b is
//           round_pos(p[a] + (p[b] - p[a]) * ((double)(t - a) / (double)(b - a))); a leading step t < a0 (the first seen
//           step) is round_pos(q[a0] - (double)(a0 - t) * (q[a0+1] - q[a0])) with q the window after the interior fill
// min_seen = T_obs, max_gap = 0 is the strict rule.
struct TrackRule {
    int min_seen, max_gap;

    __device__ __forceinline__ bool member(uint32_t m) const {
        if ((m & 1u) == 0 || __popc(m) < min_seen) return false;
        // the missed frames below the oldest seen one; a run of max_gap + 1 of them survives max_gap shifted ANDs
        const uint32_t z = ~m & ((1u << (31 - __clz(m))) - 1u);
        uint32_t run = z;
        for (int k = 1; k <= max_gap; ++k) run &= z >> k;
        return run == 0;
    }

    // m: a member's bits (bit 0 and at least one more set, nothing at or above bit T_obs).  read(t, x, y) yields the
    // rounded position of a SEEN step t -- a missed step is never read --, write(t, x, y) takes every step's once.
    // A seen step is read before it is written and a filled one is only written, so the two may be the same memory.
    template <class Read, class Write>
    static __device__ __forceinline__ void fill(uint32_t m, int T_obs, double scale, Read read, Write write) {
#pragma clang fp contract(off)
        const int a0 = T_obs - 1 - (31 - __clz(m));          // the first seen step
        double ax, ay;
        read(a0, ax, ay);
        write(a0, ax, ay);
        const double q0x = ax, q0y = ay;
        double q1x = 0.0, q1y = 0.0;                          // q[a0 + 1]
        int a = a0;
        for (int b = a0 + 1; b < T_obs; ++b) {
            if (((m >> (T_obs - 1 - b)) & 1u) == 0) continue;
            double bx, by;
            read(b, bx, by);
            for (int t = a + 1; t < b; ++t) {
                const double w = (double)(t - a) / (double)(b - a);
                const double x = round_pos(ax + (bx - ax) * w, scale), y = round_pos(ay + (by - ay) * w, scale);
                write(t, x, y);
                if (t == a0 + 1) {
                    q1x = x;
                    q1y = y;
                }
            }
            write(b, bx, by);
            if (b == a0 + 1) {
                q1x = bx;
                q1y = by;
            }
            a = b;
            ax = bx;
            ay = by;
        }
        const double dx = q1x - q0x, dy = q1y - q0y;
        for (int t = 0; t < a0; ++t) {
            const double k = (double)(a0 - t);
            write(t, round_pos(q0x - k * dx, scale), round_pos(q0y - k * dy, scale));
        }
    }
};

// Block-wide exclusive rank of `flag` over the threads (thread order), added to `base`; every thread gets the block
// total in *total.  Called by all kThreads threads of the block (it holds two barriers).
template <int kThreads>
__device__ __forceinline__ int block_rank(bool flag, int base, int *total, int *wave_cnt) {
    constexpr int kWaves = kThreads / kWave;
    const int wave = threadIdx.x / kWave;
    const uint64_t m = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
        const int c = wave_cnt[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();                    // wave_cnt is reused by the next call
    *total = all;
    return base + before + lanes_below(m);
}

// ---- the parts of a push that do not depend on its state ------------------------------------------------------------
// The slot assignment: sort the m detections by (id, detection index), then give every detection j its det_slot[j]
// (-1 on entry).  A live slot keeps its id's detection; THE i-TH NEW DETECTION IN DETECTION ORDER TAKES THE i-TH FREE
// SLOT IN SLOT ORDER.  A repeated id: the first detection wins, the others get -2 and *flags DUPLICATE.  No free slot:
// -3 and *flags OVERFLOW.  live(s): slot s holds a track (the caller's notion: a presence mask, a sample count); its
// id is slot_id[s].  key / kidx (n2 entries, loaded: det_load), det_slot (m), free_list (S), wave_cnt and flags are
// the caller's LDS.  Every thread of the kThreads calls it behind a barrier after det_load; it ends on a barrier.
template <int kThreads, class Live>
__device__ __forceinline__ void assign_slots(int64_t *key, int32_t *kidx, int32_t *det_slot, int32_t *free_list,
                                             int *wave_cnt, int *flags, int m, int n2, int S, const int64_t *slot_id,
                                             Live live) {
    const int tid = threadIdx.x, nt = blockDim.x;
    det_sort(key, kidx, n2, tid, nt);
    for (int p = tid; p < m; p += nt)
        if (p > 0 && key[p] == key[p - 1]) {
            det_slot[kidx[p]] = -2;
            atomicOr(flags, kFlagDuplicate);
        }
    for (int s = tid; s < S; s += nt) {
        if (!live(s)) continue;
        const int at = det_find(key, m, slot_id[s]);         // (the winner)
        if (at >= 0) det_slot[kidx[at]] = s;
    }
    __syncthreads();
    int n_free = 0, tot = 0;
    for (int s0 = 0; s0 < S; s0 += nt) {
        const int s = s0 + tid;
        const bool fr = s < S && !live(s);
        const int r = block_rank<kThreads>(fr, n_free, &tot, wave_cnt);
        if (fr) free_list[r] = s;
        n_free += tot;
    }
    __syncthreads();
    int n_new = 0;
    for (int j0 = 0; j0 < m; j0 += nt) {
        const int j = j0 + tid;
        const bool nw = j < m && det_slot[j] == -1;
        const int r = block_rank<kThreads>(nw, n_new, &tot, wave_cnt);
        if (nw) {
            if (r < n_free) det_slot[j] = free_list[r];
            else {
                det_slot[j] = -3;
                atomicOr(flags, kFlagOverflow);
            }
        }
        n_new += tot;
    }
    __syncthreads();
}

// The padding of one scene (o.seen may be null): slots [from, V) get id -1, seen 0 and zero positions; from = 0 is the
// whole empty scene.  num_peds and the flags are the caller's.  No barrier.
__device__ __forceinline__ void pad_scene(const SceneOut &o, int T_obs, int V, int from) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = from + tid; e < V; e += nt) {
        o.out_ids[e] = -1;
        if (o.seen) o.seen[e] = 0;
    }
    for (int e = tid; e < T_obs * (V - from); e += nt) {
        const int t = e / (V - from), r = from + e % (V - from);
        o.obs_abs[((int64_t)t * V + r) * 2] = 0.0;
        o.obs_abs[((int64_t)t * V + r) * 2 + 1] = 0.0;
    }
}

// One workgroup per stream: stream b = blockIdx.x pushes its range of the tick when pushed[b] != 0: flags =
// body(its detections, count, its scene), the scene being its slices of the (NS, ...) outputs; the body slices its
// state by b (of_stream).  Otherwise no state is touched and the scene is the empty one.
template <class Body>
__device__ __forceinline__ void push_stream(const Detections &det, const Tick &tick, const SceneOut &out, int T_obs, int V,
                                            int32_t *__restrict__ out_flags, Body body) {
    const int b = blockIdx.x;
    const SceneOut mine = out.of_stream(b, T_obs, V);
    int flags = 0;
    if (tick.pushed_at(b) == 0) {                           // uniform over the block: no barrier is skipped halfway
        pad_scene(mine, T_obs, V, 0);
        if (threadIdx.x == 0) mine.num_peds[0] = 0;
    } else {
        int lo;
        const int count = tick.range(b, lo);
        flags = body(det.from(lo), count, mine);
    }
    if (out_flags && threadIdx.x == 0) out_flags[b] = flags;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// the range check of a rule and its window, in an entry point that names them T_obs, min_seen and max_gap
#define STG_REQUIRE_RULE(what)                                                                                        \
    STG_REQUIRE(T_obs >= 2 && T_obs <= 32 && min_seen >= 2 && min_seen <= T_obs && max_gap >= 0 &&                    \
                    max_gap <= T_obs - 2,                                                                             \
                STG_EINVAL, "%s: min_seen=%d not in [2, T_obs=%d] or max_gap=%d not in [0, T_obs - 2]", what, min_seen, \
                T_obs, max_gap)

// What the _streams pushes check of their streams (stream_args, live_args.hpp), under the entry point's name `what`, and
// their workgroup size: block_threads = 0 becomes kStreamThreads
static inline int push_streams_args(const char *what, int NS, int M_total, int64_t id_stride, int64_t xy_stride,
                                    int &block_threads) {
    const int rc = stream_args(what, NS, M_total, id_stride, xy_stride);
    if (rc != STG_OK) return rc;
    if (block_threads == 0) block_threads = kStreamThreads;
    STG_REQUIRE(block_threads == 64 || block_threads == 256 || block_threads == 1024, STG_EINVAL,
                "%s: block_threads=%d (0, 64, 256 or 1024)", what, block_threads);
    return STG_OK;
}

// ... and the instantiation that size picks: go(std::integral_constant<int, kThreads>) for the checked block_threads
template <class Go>
static inline int with_stream_threads(int block_threads, Go go) {
    if (block_threads == 64) return go(std::integral_constant<int, 64>{});
    if (block_threads == 256) return go(std::integral_constant<int, 256>{});
    return go(std::integral_constant<int, 1024>{});
}

}  // namespace stg
