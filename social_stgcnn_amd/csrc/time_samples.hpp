// time_samples: a track's samples in its time ring (TimedState / TimedView of live_args.hpp), the one reader that the
// kernels on the timed track state share -- the push that keeps the rings (frames_time.hip), the score
// (score_time.hip, 5.25) and the harvest (harvest_time.hip, 5.27) behind it; DESIGN.md 5.35.  The refused push, a
// slot's head and count, the ring index of its newest samples and of a logical sample, the search of an instant and
// the interpolation of a bracket.  Device helpers without state; slots, ring indices and counts are int, the callers
// make the int64_t offsets into t_ring / xy_ring.
#pragma once
#include "detections.hpp"

namespace stg {

// did the timed push of this tick refuse its time (frames_time.hip step 0)?  Then it left the state as it was
__device__ __forceinline__ bool push_refused(const int32_t *head_flags) {
    return (head_flags[1] & STG_TRACK_TIME_ORDER) != 0;
}

// Slot s behind a push: returns its sample count clamped to [0, R]; *head is its next write index taken into [0, R)
__device__ __forceinline__ int slot_samples(const int32_t *slot_head, int s, int R, int *head) {
    const int c = slot_head[2 * s + 1];
    *head = (int)((uint32_t)slot_head[2 * s] % (uint32_t)R);
    return c < 0 ? 0 : (c > R ? R : c);
}

// The ring index before i: a slot's newest sample is at ring_before(head), the one before it at ring_before of that
__device__ __forceinline__ int ring_before(int i, int R) { return i == 0 ? R - 1 : i - 1; }

// The n samples of a slot that end just before ring index `head`, oldest first: ring index of logical sample i < n.
// Behind a push n is the slot's count; inside the push, whose own sample is logically the last one and comes from the
// input, n = min(count, R - 1) recorded ones (the one this push overwrites is not among them).
__device__ __forceinline__ int ring_at(int head, int n, int i, int R) {
    const int x = head + R - n + i;                         // < 2 R
    return x >= R ? x - R : x;
}

// Logical index of the last of those n samples at or before tau, or -1; ts = the slot's row of t_ring.  Ring order is
// time order: a binary search, at most log2(n) + 1 dependent loads
__device__ __forceinline__ int last_at_or_before(const int64_t *__restrict__ ts, int head, int n, int R, int64_t tau) {
    int lo = 0, hi = n;                                     // the first sample later than tau
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ts[ring_at(head, n, mid, R)] <= tau) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// round(pa + (pb - pa) * w): the statement's interpolation, one IEEE operation at a time
__device__ __forceinline__ double lerp_pos(double pa, double pb, double w, double scale) {
#pragma clang fp contract(off)
    const double d = pb - pa;
    const double p = d * w;
    return round_pos(pa + p, scale);
}

// The position at tau, ta < tau < tb, in the bracket of the samples (ta, ax, ay) and (tb, bx, by): lerp_pos per
// coordinate with the weight (double)(tau - ta) / (double)(tb - ta)
__device__ __forceinline__ void lerp_bracket(int64_t ta, double ax, double ay, int64_t tb, double bx, double by,
                                             int64_t tau, double scale, double &x, double &y) {
#pragma clang fp contract(off)
    const double w = (double)(tau - ta) / (double)(tb - ta);
    x = lerp_pos(ax, bx, w, scale);
    y = lerp_pos(ay, by, w, scale);
}

}  // namespace stg
