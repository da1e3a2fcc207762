// harvest_parts: what the window harvests share (harvest.hip: one push = one frame; harvest_time.hip:
// timestamped pushes resampled on the step grid; what is shared: DESIGN.md 5.35) -- the workgroup size,
// the block-wide scan, ONE FRAME OF A STREAM'S HISTORY (harvest_frame: the two families differ only in how a live slot
// learns "seen in this frame, at (x, y)", which they pass in), the rows of a window, the capacity test, the tail of a
// lone kernel, the body of an update-and-count launch and, on the host, the checks of the sizes and of the pointers and
// the place and write launches of a tick of streams, whose kernels live in harvest.hip.  Device helpers without state,
// as in detections.hpp: the caller owns the LDS arrays (harvest_count_stream, a kernel's whole body, declares them).
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

// the candidates' sort arrays in the dynamic LDS of an update launch (harvest_lds): det_sort_n(S) ids, then their slots
struct HarvestSort {
    int64_t *key;
    int32_t *kidx;
    __device__ __forceinline__ HarvestSort(unsigned char *lds, int S)
        : key(reinterpret_cast<int64_t *>(lds)), kidx(reinterpret_cast<int32_t *>(key + det_sort_n(S))) {}
};

// One frame of one stream's history by one workgroup, behind the push: age the words (`clear`: empty them first, a run
// of frames has ended), ask seen_at(s, x, y) of every live slot s whether its track is seen in this frame and where,
// keep that position in the ring row of the frame, and leave the candidates -- the slots with all T_all low bits set --
// sorted by id in (so.key, so.kidx = slot).  Behind the barrier that ends the pass over the slots, when every thread
// has read what the caller read of the head (and of its clock), thread 0 stores the head {row, head1} and calls also()
// for the caller's own stores.  Returns (in every thread) the number of candidates, 0 when below min_peds; `row` is the
// history's ring row of the frame.  Ends on a barrier.
template <class SeenAt, class Also>
__device__ __forceinline__ int harvest_frame(const int64_t *__restrict__ slot_id, const HarvestState &hs,
                                             const HarvestDims &d, bool clear, int head1, const HarvestSort &so,
                                             int *wave_cnt, int &row, SeenAt seen_at, Also also) {
    const int tid = threadIdx.x, nt = kHarvestThreads, S = d.S, T_all = d.T_all;
    const uint32_t full = T_all >= 32 ? 0xffffffffu : (1u << T_all) - 1u;
    row = (ring_row(hs.head[0], T_all) + 1) % T_all;
    double *__restrict__ dst = hs.ring + (int64_t)row * S * 2;
    int c = 0, tot = 0;
    for (int s0 = 0; s0 < S; s0 += nt) {
        const int s = s0 + tid;
        int64_t id = -1;
        bool cand = false;
        if (s < S) {
            id = slot_id[s];
            uint32_t w = 0;                                  // a free slot has an empty word
            if (id >= 0) {
                w = clear ? 0u : (hs.word[s] << 1) & full;
                double x, y;
                if (seen_at(s, x, y)) {
                    w |= 1u;
                    dst[s * 2] = x;
                    dst[s * 2 + 1] = y;
                }
            }
            hs.word[s] = w;
            cand = w == full;
        }
        const int r = block_rank<kHarvestThreads>(cand, c, &tot, wave_cnt);
        if (cand) {                                          // (r < S: at most one candidate per slot)
            so.key[r] = id;
            so.kidx[r] = s;
        }
        c += tot;
    }
    __syncthreads();                                         // every thread has read head; key / kidx / ring are written
    if (tid == 0) {
        hs.head[0] = row;
        hs.head[1] = head1;
        also();
    }
    if (c < d.min_peds) return 0;
    const int n2 = det_sort_n(c);                            // (<= det_sort_n(S))
    for (int p = c + tid; p < n2; p += nt) {
        so.key[p] = INT64_MAX;
        so.kidx[p] = -1;
    }
    __syncthreads();
    det_sort(so.key, so.kidx, n2, tid, nt);
    return c;
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

// The header as a lone launch found it: read by every thread ahead of the barriers, written by thread 0 behind them
struct HarvestHeader {
    int nw, nr, dropped;
    __device__ __forceinline__ explicit HarvestHeader(const HarvestLog &log)
        : nw(log.header[0]), nr(log.header[1]), dropped(log.header[2]) {}
};

// The tail of a lone kernel, behind harvest_frame: the window of the c candidates so.kidx[0 .. c) (none: nothing) goes
// behind what the header `at` counts, tagged (stream_index, tag), when it fits, and is counted as dropped when not.
__device__ __forceinline__ void harvest_append(const HarvestState &hs, const HarvestDims &d, const HarvestLog &log,
                                               const HarvestHeader &at, int c, int row, const HarvestSort &so,
                                               int stream_index, int tag) {
    if (c == 0) return;
    const int nw = at.nw, nr = at.nr;
    const bool fits = harvest_fits(log, at.dropped, nw, nr, c);
    if (fits) harvest_rows(hs.ring, d, log, nr, c, row, [&](int p) { return so.kidx[p]; });
    if (threadIdx.x == 0) {
        if (fits) {
            log.win_start[nw + 1] = nr + c;
            log.win_tag[nw * 2] = stream_index;
            log.win_tag[nw * 2 + 1] = tag;
            log.header[0] = nw + 1;
            log.header[1] = nr + c;
        } else {
            log.header[2] = at.dropped + 1;
        }
    }
}

// The body of an update-and-count launch, one workgroup per stream b = blockIdx.x: a pushed stream's frame through
// update(b, so, wave_cnt) -> its candidates' number, their slots to the stream's cand, the number to its count (0 for
// a stream not pushed).  Declares the launch's LDS.
template <class Update>
__device__ __forceinline__ void harvest_count_stream(const int32_t *__restrict__ pushed, const HarvestDims &d,
                                                     const HarvestWork &work, Update update) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int wave_cnt[kHarvestWaves];
    const HarvestSort so(lds, d.S);
    const int b = blockIdx.x;
    const HarvestWork mine = work.of_stream(b, d);
    int c = 0;
    if (pushed[b] != 0) {                                    // uniform over the block: no barrier is skipped halfway
        c = update(b, so, wave_cnt);
        for (int p = threadIdx.x; p < c; p += kHarvestThreads) mine.cand[p] = so.kidx[p];
    }
    if (threadIdx.x == 0) mine.count[0] = c;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// dynamic LDS of an update launch: the candidates' sort arrays
static inline size_t harvest_lds(const HarvestDims &d) { return det_sort_lds(det_sort_n(d.S)); }

// What every harvest entry point checks first, under its own name `what`: the sizes, then the log's capacities
static inline int harvest_size_args(const char *what, const HarvestDims &d, const HarvestLog &log) {
    STG_REQUIRE(d.S >= 1 && d.S <= STG_TRACK_MAX_SLOTS && d.T_obs >= 1 && d.T_all >= 2 && d.T_all <= STG_HARVEST_MAX_STEPS &&
                    d.T_all - d.T_obs >= 1 && d.min_peds >= 1,
                STG_EINVAL, "%s: bad sizes S=%d T_obs=%d T_all=%d min_peds=%d", what, d.S, d.T_obs, d.T_all, d.min_peds);
    STG_REQUIRE(log.cap_windows >= 1 && log.cap_windows < INT32_MAX && log.cap_rows >= 1, STG_EINVAL,
                "%s: bad capacities cap_windows=%d cap_rows=%d", what, log.cap_windows, log.cap_rows);
    return STG_OK;
}

// ... and last, in one test with its track state's pointers: are the history and the log all there?
static inline bool harvest_pointers(const HarvestState &hs, const HarvestLog &log) {
    return hs.word && hs.ring && hs.head && log.rel_all && log.win_start && log.win_tag && log.header;
}

// The place and the write launch of a tick of NS streams (harvest.hip), behind an update-and-count launch that left the
// candidates and counts in `wk` and every pushed stream's h_head[1] one past its window's tag.
int harvest_place_write(const char *what, const HarvestState &hs, const HarvestDims &d, const HarvestWork &wk,
                        const HarvestLog &log, int NS, hipStream_t st);

}  // namespace stg
