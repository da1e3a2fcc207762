// track_rule: what the live pushes share (frames.hip: one push = one model step; frames_time.hip: timestamped pushes,
// DESIGN.md 5.20) beyond the detection sort of detections.hpp -- the workgroup sizes and flags of a push, the block-wide
// rank, and TrackRule, the rule for partially observed tracks, which the recording kernels use too.
#pragma once
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

// the range check of a rule and its window, in an entry point that names them T_obs, min_seen and max_gap
#define STG_REQUIRE_RULE(what)                                                                                        \
    STG_REQUIRE(T_obs >= 2 && T_obs <= 32 && min_seen >= 2 && min_seen <= T_obs && max_gap >= 0 &&                    \
                    max_gap <= T_obs - 2,                                                                             \
                STG_EINVAL, "%s: min_seen=%d not in [2, T_obs=%d] or max_gap=%d not in [0, T_obs - 2]", what, min_seen, \
                T_obs, max_gap)

}  // namespace stg
