// associate: what the association kernels (associate.hip) share with anything that sizes or reads
// their launch -- the workgroup sizes, the flag, the LDS image and the two IEEE expressions of the rule.
#pragma once
#include "detections.hpp"

namespace stg {

constexpr int kAssocThreads = 1024;          // stg_associate: one workgroup
constexpr int kAssocStreamThreads = 256;     // stg_associate_streams: one workgroup per stream
constexpr int kFlagAssocFull = STG_ASSOC_FULL;

// LDS image (dynamic): per track slot its predicted position q (2 x float64), its gate (int32: which of the two, -1
// for a free slot), its state word and one entry of the live list / free list (int32 each): 28 bytes; per detection its
// rounded position p (2 x float64) and its state word: 20 bytes.  At both limits (2048, 2048) that is 98,304 bytes of
// the 163,840 a CU holds; at the predictors' defaults (1024, 1024) 49,152, so three workgroups share a CU.
constexpr size_t kAssocTrackBytes = 2 * sizeof(double) + 3 * sizeof(int32_t);
constexpr size_t kAssocDetBytes = 2 * sizeof(double) + sizeof(int32_t);
static inline size_t assoc_lds(int C, int M_max) { return (size_t)C * kAssocTrackBytes + (size_t)M_max * kAssocDetBytes; }

// A state word of a track (of a detection): kUnknown before its first scan, kNone when no free partner is in reach, the
// index >= 0 of its best free partner, or, once matched, assoc_take(partner) <= -3.
constexpr int kNone = -1, kUnknown = -2;
__device__ __forceinline__ int assoc_take(int partner) { return -3 - partner; }
__device__ __forceinline__ bool assoc_taken(int word) { return word <= -3; }
__device__ __forceinline__ int assoc_partner(int word) { return -3 - word; }

// The lanes that share one row or column of a scan, and their reduction: (best, at) <- the minimum of (cost, index)
// over the group's lanes, at < 0 = nothing found.  Every lane of the wave calls it; a group is kAssocGroup aligned lanes.
constexpr int kAssocGroup = 8;
__device__ __forceinline__ void assoc_group_min(double &best, int &at) {
#pragma unroll
    for (int o = kAssocGroup / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, kWave);
        const int oa = __shfl_xor(at, o, kWave);
        if (oa >= 0 && (at < 0 || ob < best || (ob == best && oa < at))) {
            best = ob;
            at = oa;
        }
    }
}

// q = pos + vel * k and the squared distance, one IEEE operation at a time
__device__ __forceinline__ double assoc_predict(double pos, double vel, double k) {
#pragma clang fp contract(off)
    const double t = vel * k;
    return pos + t;
}
__device__ __forceinline__ double assoc_cost(double qx, double qy, double px, double py) {
#pragma clang fp contract(off)
    const double dx = qx - px, dy = qy - py;
    const double a = dx * dx, b = dy * dy;
    return a + b;
}
// vel = (p - pos) / k
__device__ __forceinline__ double assoc_velocity(double p, double pos, double k) {
#pragma clang fp contract(off)
    const double d = p - pos;
    return d / k;
}

}  // namespace stg
