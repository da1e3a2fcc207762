// harvest_parts: what the window harvests share (harvest.hip: one push = one frame; harvest_time.hip:
// timestamped pushes resampled on the step grid) -- the workgroup size, the block-wide scan, the rows of
// a window, the capacity test and, on the host, the place and write launches of a tick of streams, whose kernels live in
// harvest.hip.  Device helpers without state, as in detections.hpp: the caller owns the LDS arrays.
#pragma once
#include "detections.hpp"
#include "track_rule.hpp"

namespace stg {

constexpr int kHarvestThreads = 256;
constexpr int kHarvestWaves = kHarvestThreads / kWave;

// a ring row as the state holds it -> [0, n): every ring row is taken modulo its depth
__device__ __forceinline__ int ring_row(int row, int n) { return (row % n + n) % n; }

// Block-wide exclusive scan of v over the threads (thread order); every thread gets the block total in *total.  Called
// by all kHarvestThreads threads (two barriers).
__device__ __forceinline__ int block_scan(int v, int *total, int *wave_tot) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int x = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const int y = __shfl_up(x, o, kWave);
        if (lane >= o) x += y;
    }
    if (lane == kWave - 1) wave_tot[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kHarvestWaves; ++w) {
        const int c = wave_tot[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();                    // wave_tot is reused by the next call
    *total = all;
    return before + x - v;
}

// The c rows of one window into the log from row `row0` on: row p is the slot slot_at(p), (2, T_all) float32 with column
// 0 zero and column t = (float)(pos[t] - pos[t-1]), the subtraction in float64 on the rounded positions, oldest first.
// Every store is checked against the log's capacity, every slot against S.
template <class SlotAt>
__device__ __forceinline__ void harvest_rows(const double *__restrict__ ring, const HarvestDims &d, const HarvestLog &log,
                                             int64_t row0, int c, int row, SlotAt slot_at) {
    const int S = d.S, T_all = d.T_all;
    float *__restrict__ rel = log.rel_all;
    for (int e = threadIdx.x; e < c * T_all; e += kHarvestThreads) {
        const int p = e / T_all, t = e % T_all;
        const int s = slot_at(p);
        const int64_t r = row0 + p;
        if (r < 0 || r >= log.cap_rows || s < 0 || s >= S) continue;
        float dx = 0.0f, dy = 0.0f;
        if (t > 0) {
            const int now = (row + 1 + t) % T_all, before = (row + t) % T_all;   // step t is row - (T_all - 1 - t)
            const double *a = ring + ((int64_t)now * S + s) * 2, *b = ring + ((int64_t)before * S + s) * 2;
            dx = (float)(a[0] - b[0]);
            dy = (float)(a[1] - b[1]);
        }
        rel[(r * 2) * T_all + t] = dx;
        rel[(r * 2 + 1) * T_all + t] = dy;
    }
}

// does a window of c rows fit behind (nw windows, nr rows)?  Never once a window has been dropped.
__device__ __forceinline__ bool harvest_fits(const HarvestLog &log, int dropped, int64_t nw, int64_t nr, int c) {
    return dropped == 0 && nw >= 0 && nr >= 0 && nw < log.cap_windows && nr + c <= log.cap_rows;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// dynamic LDS of an update launch: the candidates' sort arrays
static inline size_t harvest_lds(const HarvestDims &d) { return det_sort_lds(det_sort_n(d.S)); }

// The place and the write launch of a tick of NS streams (harvest.hip), behind an update-and-count launch that left the
// candidates and counts in `wk` and every pushed stream's h_head[1] one past its window's tag.
int harvest_place_write(const char *what, const HarvestState &hs, const HarvestDims &d, const HarvestWork &wk,
                        const HarvestLog &log, int NS, hipStream_t st);

}  // namespace stg
