// harvest_time: training windows from TIMESTAMPED live pushes.  The timed push (frames_time.hip) keeps,
// per track, a ring of its newest R samples at the tracker's own rate; here those tracks are resampled on the model's
// step grid g_i = g0 + i * step, anchored at the stream's first accepted push, and each resolved grid instant is one
// frame of the harvest of harvest.hip: the same words, position ring, candidates, rows and log.
//
//   stg_window_harvest_timed          one stream: ONE workgroup, behind stg_track_push_timed of the same push.  It reads
//                                     the timed track state only.  Refused push or no pending instant: nothing, decided
//                                     by every thread alike ahead of every barrier.  Else one thread per slot searches
//                                     the newest pending instant g in the slot's time ring (ring order is time order:
//                                     at most log2(R) + 1 dependent loads), takes the sample at g or the interpolation of
//                                     its bracket (time_samples.hpp: the push's own arithmetic), updates the word; then
//                                     compaction, the sort of the candidates, the window's place and rows as in
//                                     window_harvest_kernel.
//   stg_window_harvest_streams_timed  NS streams behind stg_track_push_streams_timed: the timed update + count launch
//                                     here, then the place and write launches of harvest.hip, which tag a window
//                                     h_head[1] - 1: the grid index of the frame just resolved.
//
// Integer work, float64 arithmetic with IEEE operations as written, plain C++ stores, LDS atomics on integer words only,
// no spinning, no host synchronisation: everything, the time included, is read when the kernels run.
#include "harvest_parts.hpp"
#include "time_samples.hpp"

namespace stg {

// What one launch does to one stream, computed alike by every thread from what the push and the last launch left:
// K pending instants, the newest of them g, and the history's counters after it
struct TimedFrame {
    int64_t K, g, g0, skipped;
    int32_t j;                                               // grid instants passed once g is resolved
};

__device__ __forceinline__ TimedFrame timed_frame(const TimedView &tr, const HarvestState &hs, const int64_t *hclock,
                                                  const TimedHarvestDims &t) {
    TimedFrame f;
    const int64_t t_now = tr.clock[0];
    const int64_t j = hs.head[1] < 0 ? 0 : hs.head[1];
    f.g0 = hclock[0] != 0 ? hclock[1] : t_now;               // the first accepted push anchors the grid
    f.skipped = hclock[2];
    const int64_t d = t_now - t.settle - f.g0;
    const int64_t n = d < 0 ? 0 : d / t.step + 1;            // the grid instants at or before t_now - settle
    f.K = n - j;
    f.g = f.g0 + (n - 1) * t.step;                           // (n - 1) * step <= d
    f.j = (int32_t)(n < INT32_MAX ? n : INT32_MAX);
    return f;
}

// One launch on one stream's history by one workgroup, behind the timed push; what harvest_update (harvest.hip) is to
// the untimed one.  Leaves the candidates sorted by id in (key, kidx = slot) and returns their number, 0 when below
// min_peds or when the launch does nothing; `row` is the history's ring row of the frame.  Every return is taken by
// all threads alike.
__device__ __forceinline__ int harvest_update_timed(const TimedView &tr, const HarvestState &hs, int64_t *hclock,
                                                    const HarvestDims &d, const TimedHarvestDims &t, int64_t *key,
                                                    int32_t *kidx, int *wave_cnt, int &row) {
    const int tid = threadIdx.x, nt = kHarvestThreads, S = d.S, R = t.R, T_all = d.T_all;
    const uint32_t full = T_all >= 32 ? 0xffffffffu : (1u << T_all) - 1u;
    // a refused push: nothing.  Uniform over the block, ahead of every barrier
    if (tr.head_flags[1] & STG_TRACK_TIME_ORDER) return 0;
    const TimedFrame f = timed_frame(tr, hs, hclock, t);
    const bool anchored = hclock[0] != 0;
    if (f.K <= 0) {                                          // not pending (uniform): at most the anchor is written
        __syncthreads();                                     // every thread has read the clock
        if (tid == 0 && !anchored) {
            hclock[0] = 1;
            hclock[1] = f.g0;
        }
        return 0;
    }
    const bool clear = f.K >= 2;                             // skipped instants: every run of frames ends here
    const int64_t g = f.g, max_dt = t.max_dt;
    row = (ring_row(hs.head[0], T_all) + 1) % T_all;
    double *__restrict__ dst = hs.ring + (int64_t)row * S * 2;
    int c = 0, tot = 0;
    for (int s0 = 0; s0 < S; s0 += nt) {
        const int s = s0 + tid;
        int64_t id = -1;
        bool cand = false;
        if (s < S) {
            id = tr.slot_id[s];
            uint32_t w = 0;                                  // a free slot has an empty word
            if (id >= 0) {
                w = clear ? 0u : (hs.word[s] << 1) & full;
                int cnt = tr.slot_head[2 * s + 1];
                cnt = cnt < 0 ? 0 : (cnt > R ? R : cnt);
                const int h = ring_row(tr.slot_head[2 * s], R);
                const int64_t *__restrict__ ts = tr.t_ring + (int64_t)s * R;
                const double *__restrict__ ps = tr.xy_ring + (int64_t)s * R * 2;
                int lo = 0, hi = cnt;                        // the first sample later than g
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ts[ring_at(h, cnt, mid, R)] <= g) lo = mid + 1;
                    else hi = mid;
                }
                const int i = lo - 1;
                if (i >= 0) {
                    const int a = ring_at(h, cnt, i, R);
                    const int64_t ta = ts[a];
                    bool seen = ta == g;
                    double x = ps[a * 2], y = ps[a * 2 + 1];
                    if (!seen && i + 1 < cnt) {
                        const int b = ring_at(h, cnt, i + 1, R);
                        const int64_t tb = ts[b];
                        if (tb - ta <= max_dt) {
                            const double wgt = (double)(g - ta) / (double)(tb - ta);
                            x = lerp_pos(x, ps[b * 2], wgt, t.scale);
                            y = lerp_pos(y, ps[b * 2 + 1], wgt, t.scale);
                            seen = true;
                        }
                    }
                    if (seen) {
                        w |= 1u;
                        dst[s * 2] = x;
                        dst[s * 2 + 1] = y;
                    }
                }
            }
            hs.word[s] = w;
            cand = w == full;
        }
        const int r = block_rank<kHarvestThreads>(cand, c, &tot, wave_cnt);
        if (cand) {                                          // (r < S: at most one candidate per slot)
            key[r] = id;
            kidx[r] = s;
        }
        c += tot;
    }
    __syncthreads();                                         // every thread has read head and clock; key / kidx / ring are written
    if (tid == 0) {
        hs.head[0] = row;
        hs.head[1] = f.j;
        hclock[0] = 1;
        hclock[1] = f.g0;
        hclock[2] = f.skipped + (f.K - 1);
    }
    if (c < d.min_peds) return 0;
    const int n2 = det_sort_n(c);                            // (<= det_sort_n(S))
    for (int p = c + tid; p < n2; p += nt) {
        key[p] = INT64_MAX;
        kidx[p] = -1;
    }
    __syncthreads();
    det_sort(key, kidx, n2, tid, nt);
    return c;
}

// ---- one stream ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void window_harvest_timed_kernel(TimedView tr, HarvestState hs,
                                                                               int64_t *hclock, HarvestDims d,
                                                                               TimedHarvestDims t, HarvestLog log,
                                                                               int stream_index) {
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + det_sort_n(d.S));
    __shared__ int wave_cnt[kHarvestWaves];
    // the header as the push found it: read by every thread ahead of the barriers, written by thread 0 behind them
    const int nw = log.header[0], nr = log.header[1], dropped = log.header[2];
    const int tag = timed_frame(tr, hs, hclock, t).j - 1;    // the grid index of the frame this launch resolves, if any
    int row = 0;
    const int c = harvest_update_timed(tr, hs, hclock, d, t, key, kidx, wave_cnt, row);
    if (c == 0) return;
    const bool fits = harvest_fits(log, dropped, nw, nr, c);
    if (fits) harvest_rows(hs.ring, d, log, nr, c, row, [&](int p) { return kidx[p]; });
    if (threadIdx.x == 0) {
        if (fits) {
            log.win_start[nw + 1] = nr + c;
            log.win_tag[nw * 2] = stream_index;
            log.win_tag[nw * 2 + 1] = tag;
            log.header[0] = nw + 1;
            log.header[1] = nr + c;
        } else {
            log.header[2] = dropped + 1;
        }
    }
}

// ---- NS streams: the timed update + count; place and write are harvest.hip's ------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void harvest_update_streams_timed_kernel(
    TimedView tr, const int32_t *__restrict__ pushed, HarvestState hs, int64_t *hclock, HarvestDims d,
    TimedHarvestDims t, HarvestWork work) {
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + det_sort_n(d.S));
    __shared__ int wave_cnt[kHarvestWaves];
    const int b = blockIdx.x;
    const HarvestWork mine = work.of_stream(b, d);
    int c = 0;
    if (pushed[b] != 0) {                                    // uniform over the block: no barrier is skipped halfway
        int row = 0;
        c = harvest_update_timed(tr.of_stream(b, d.S, t.R), hs.of_stream(b, d), hclock + 3 * (int64_t)b, d, t, key, kidx,
                                 wave_cnt, row);
        for (int p = threadIdx.x; p < c; p += kHarvestThreads) mine.cand[p] = kidx[p];
    }
    if (threadIdx.x == 0) mine.count[0] = c;
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int harvest_timed_args(const char *what, const TimedView &tr, const HarvestState &hs, const int64_t *hclock,
                              const HarvestDims &d, const TimedHarvestDims &t, const HarvestLog &log) {
    STG_REQUIRE(d.S >= 1 && d.S <= STG_TRACK_MAX_SLOTS && d.T_obs >= 1 && d.T_all >= 2 && d.T_all <= STG_HARVEST_MAX_STEPS &&
                    d.T_all - d.T_obs >= 1 && d.min_peds >= 1,
                STG_EINVAL, "%s: bad sizes S=%d T_obs=%d T_all=%d min_peds=%d", what, d.S, d.T_obs, d.T_all, d.min_peds);
    STG_REQUIRE(log.cap_windows >= 1 && log.cap_windows < INT32_MAX && log.cap_rows >= 1, STG_EINVAL,
                "%s: bad capacities cap_windows=%d cap_rows=%d", what, log.cap_windows, log.cap_rows);
    STG_REQUIRE(t.R >= 2, STG_EINVAL, "%s: R=%d samples per track (at least 2)", what, t.R);
    STG_REQUIRE(t.R <= STG_TRACK_MAX_HISTORY, STG_EUNSUPPORTED, "%s: R=%d above STG_TRACK_MAX_HISTORY=%d", what, t.R,
                STG_TRACK_MAX_HISTORY);
    STG_REQUIRE(t.step >= 1, STG_EINVAL, "%s: step=%lld ticks (at least 1)", what, (long long)t.step);
    STG_REQUIRE(t.step < ((int64_t)1 << 31) && t.step * d.T_obs < ((int64_t)1 << 31), STG_EUNSUPPORTED,
                "%s: step=%lld: step * T_obs must stay below 2^31", what, (long long)t.step);
    STG_REQUIRE(t.max_dt >= 1 && t.max_dt <= (int64_t)(d.T_obs - 1) * t.step, STG_EINVAL,
                "%s: max_dt=%lld not in [1, (T_obs - 1) * step = %lld]", what, (long long)t.max_dt,
                (long long)((int64_t)(d.T_obs - 1) * t.step));
    STG_REQUIRE(t.settle >= 0 && t.settle <= t.max_dt - 1, STG_EINVAL, "%s: settle=%lld not in [0, max_dt - 1 = %lld]",
                what, (long long)t.settle, (long long)(t.max_dt - 1));
    STG_REQUIRE(tr.slot_id && tr.t_ring && tr.xy_ring && tr.slot_head && tr.clock && tr.head_flags && hs.word && hs.ring &&
                    hs.head && hclock && log.rel_all && log.win_start && log.win_tag && log.header,
                STG_EINVAL, "%s: null pointer", what);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_window_harvest_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                             const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags, int S, int R,
                             int T_obs, int T_all, int min_peds, double scale, int64_t step, int64_t max_dt,
                             int64_t settle, int stream_index, uint32_t *h_word, double *h_ring, int32_t *h_head,
                             int64_t *h_clock, float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header,
                             int cap_windows, int cap_rows, void *stream) {
    const char *what = "stg_window_harvest_timed";
    const stg::TimedView tr{slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    const stg::HarvestState hs{h_word, h_ring, h_head};
    const stg::HarvestDims d{S, T_obs, T_all, min_peds};
    const stg::TimedHarvestDims t{R, scale, step, max_dt, settle};
    const stg::HarvestLog log{rel_all, win_start, win_tag, header, cap_windows, cap_rows};
    const int rc = stg::harvest_timed_args(what, tr, hs, h_clock, d, t, log);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(stream_index >= 0, STG_EINVAL, "%s: bad stream_index=%d", what, stream_index);
    return stg::launch({what, dim3(1), dim3(stg::kHarvestThreads), stg::harvest_lds(d), stg::as_stream(stream), 64 * 1024},
                       stg::window_harvest_timed_kernel, tr, hs, h_clock, d, t, log, stream_index);
}

int stg_window_harvest_streams_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                                     const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags,
                                     const int32_t *pushed, int NS, int S, int R, int T_obs, int T_all, int min_peds,
                                     double scale, int64_t step, int64_t max_dt, int64_t settle, uint32_t *h_word,
                                     double *h_ring, int32_t *h_head, int64_t *h_clock, int32_t *work, float *rel_all,
                                     int32_t *win_start, int32_t *win_tag, int32_t *header, int cap_windows,
                                     int cap_rows, void *stream) {
    const char *what = "stg_window_harvest_streams_timed";
    const stg::TimedView tr{slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    const stg::HarvestState hs{h_word, h_ring, h_head};
    const stg::HarvestDims d{S, T_obs, T_all, min_peds};
    const stg::TimedHarvestDims t{R, scale, step, max_dt, settle};
    const stg::HarvestLog log{rel_all, win_start, win_tag, header, cap_windows, cap_rows};
    STG_REQUIRE(NS >= 1 && NS <= STG_TRACK_MAX_STREAMS, STG_EINVAL, "%s: bad size NS=%d", what, NS);
    int rc = stg::harvest_timed_args(what, tr, hs, h_clock, d, t, log);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(pushed && work, STG_EINVAL, "%s: null pointer", what);
    const stg::HarvestWork wk = stg::HarvestWork::carve(work, NS, S);
    hipStream_t st = stg::as_stream(stream);
    rc = stg::launch({what, dim3(NS), dim3(stg::kHarvestThreads), stg::harvest_lds(d), st, 64 * 1024},
                     stg::harvest_update_streams_timed_kernel, tr, pushed, hs, h_clock, d, t, wk);
    if (rc != STG_OK) return rc;
    return stg::harvest_place_write(what, hs, d, wk, log, NS, st);
}

}  // extern "C"
