// time_samples: a track's samples in its time ring, what the kernels that resample timed tracks share (frames_time.hip,
// DESIGN.md 5.20; harvest_time.hip): the ring index of a logical sample and the interpolation of a
// bracket.  Device helpers without state.
#pragma once
#include "detections.hpp"

namespace stg {

// round(pa + (pb - pa) * w): the statement's interpolation, one IEEE operation at a time
__device__ __forceinline__ double lerp_pos(double pa, double pb, double w, double scale) {
#pragma clang fp contract(off)
    const double d = pb - pa;
    const double p = d * w;
    return round_pos(pa + p, scale);
}

// The slot's samples as a push sees them, oldest first: the newest n_old = min(count, R - 1) recorded ones (the one
// this push overwrites is not among them) and then this push's own.  ring_at: ring index of logical sample i < n_old.
__device__ __forceinline__ int ring_at(int head, int n_old, int i, int R) {
    const int x = head + R - n_old + i;                     // < 2 R
    return x >= R ? x - R : x;
}

}  // namespace stg
