// detections: one push of detections sorted by id in LDS, what the push kernels (frames.hip) and the score kernels
// (score.hip) share.  Device helpers without state: the caller owns the LDS arrays key (n2 x int64)
// and kidx (n2 x int32), its thread geometry (tid of nt threads: blockDim.x in the push, kScoreThreads in the score)
// and every barrier but the sort's.  The order is ascending (id, detection index), so all pairs are distinct and
// FIRST DETECTION WINS: the detections of a repeated id are neighbours in ascending index, and the lower bound of the
// id (det_find) is its first detection.  The scene of a push and the truth of a score are both taken there.
#pragma once
#include "live_args.hpp"

namespace stg {

// the only rounding of a position, np.around(x, d): x * 10^d, round half to even, / 10^d (scale <= 0: no rounding)
__device__ __forceinline__ double round_pos(double x, double scale) { return scale > 0.0 ? rint(x * scale) / scale : x; }

// sort size: the next power of two >= m.  On the host det_sort_n(M_max) sizes the LDS arrays (M2), det_sort_lds their
// bytes at the head of the dynamic LDS
__host__ __device__ __forceinline__ int det_sort_n(int m) {
    int n2 = 1;
    while (n2 < m) n2 <<= 1;
    return n2;
}
static inline size_t det_sort_lds(int m2) { return (size_t)m2 * (sizeof(int64_t) + sizeof(int32_t)); }

// (key, kidx) <- the first m ids.  No barrier: the caller puts its own work ahead of the one det_sort needs
template <class Id>
__device__ __forceinline__ void det_load(int64_t *key, int32_t *kidx, const DetectionsOf<Id> &det, int m, int n2,
                                         int tid, int nt) {
    for (int p = tid; p < n2; p += nt) {
        key[p] = p < m ? det.id_at(p) : INT64_MAX;
        kidx[p] = p;
    }
}

// bitonic network over the n2 entries: every thread calls it, behind a barrier after det_load; it ends on a barrier
__device__ __forceinline__ void det_sort(int64_t *key, int32_t *kidx, int n2, int tid, int nt) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const int64_t a = key[i], b = key[l];
                    const int ia = kidx[i], ib = kidx[l];
                    const bool gt = a > b || (a == b && ia > ib);
                    if (gt == ((i & k) == 0)) {
                        key[i] = b;
                        key[l] = a;
                        kidx[i] = ib;
                        kidx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// position of the first of the n ascending keys that equals id (its lower bound), or -1
__device__ __forceinline__ int det_find(const int64_t *key, int n, int64_t id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && key[lo] == id ? lo : -1;
}

}  // namespace stg
