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
//                                     its bracket (time_samples.hpp: the push's own search and arithmetic), and that
//                                     is all this family adds: the word, the compaction, the sort of the candidates,
//                                     the window's place and rows are harvest_parts.hpp's, the very code of
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
// the untimed one.  Leaves the candidates sorted by id in (so.key, so.kidx = slot) and returns their number, 0 when
// below min_peds or when the launch does nothing; `row` is the history's ring row of the frame.  Every return is taken
// by all threads alike.
__device__ __forceinline__ int harvest_update_timed(const TimedView &tr, const HarvestState &hs, int64_t *hclock,
                                                    const HarvestDims &d, const TimedHarvestDims &t,
                                                    const HarvestSort &so, int *wave_cnt, int &row) {
    // a refused push: nothing.  Uniform over the block, ahead of every barrier
    if (push_refused(tr.head_flags)) return 0;
    const TimedFrame f = timed_frame(tr, hs, hclock, t);
    const bool anchored = hclock[0] != 0;
    if (f.K <= 0) {                                          // not pending (uniform): at most the anchor is written
        __syncthreads();                                     // every thread has read the clock
        if (threadIdx.x == 0 && !anchored) {
            hclock[0] = 1;
            hclock[1] = f.g0;
        }
        return 0;
    }
    // harvest_frame (harvest_parts.hpp) with this family's answer to "seen in this frame?": a sample at the instant g, or
    // the interpolation of the bracket around g when its ends are at most max_dt apart (time_samples.hpp).  K >= 2:
    // instants were skipped, every run of frames ends here.  Thread 0's stores then include the clock
    const int R = t.R;
    const int64_t g = f.g, max_dt = t.max_dt;
    return harvest_frame(
        tr.slot_id, hs, d, f.K >= 2, f.j, so, wave_cnt, row,
        [&](int s, double &x, double &y) {
            int h;
            const int cnt = slot_samples(tr.slot_head, s, R, &h);
            const int64_t *__restrict__ ts = tr.t_ring + (int64_t)s * R;
            const double *__restrict__ ps = tr.xy_ring + (int64_t)s * R * 2;
            const int i = last_at_or_before(ts, h, cnt, R, g);
            if (i < 0) return false;
            const int a = ring_at(h, cnt, i, R);
            const int64_t ta = ts[a];
            x = ps[a * 2];
            y = ps[a * 2 + 1];
            if (ta == g) return true;
            if (i + 1 >= cnt) return false;
            const int b = ring_at(h, cnt, i + 1, R);
            const int64_t tb = ts[b];
            if (tb - ta > max_dt) return false;
            lerp_bracket(ta, x, y, tb, ps[b * 2], ps[b * 2 + 1], g, t.scale, x, y);
            return true;
        },
        [&] {
            hclock[0] = 1;
            hclock[1] = f.g0;
            hclock[2] = f.skipped + (f.K - 1);
        });
}

// ---- one stream ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void window_harvest_timed_kernel(TimedView tr, HarvestState hs,
                                                                               int64_t *hclock, HarvestDims d,
                                                                               TimedHarvestDims t, HarvestLog log,
                                                                               int stream_index) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int wave_cnt[kHarvestWaves];
    const HarvestSort so(lds, d.S);
    const HarvestHeader at(log);
    const int tag = timed_frame(tr, hs, hclock, t).j - 1;    // the grid index of the frame this launch resolves, if any
    int row = 0;
    const int c = harvest_update_timed(tr, hs, hclock, d, t, so, wave_cnt, row);
    harvest_append(hs, d, log, at, c, row, so, stream_index, tag);
}

// ---- NS streams: the timed update + count; place and write are harvest.hip's ------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void harvest_update_streams_timed_kernel(
    TimedView tr, const int32_t *__restrict__ pushed, HarvestState hs, int64_t *hclock, HarvestDims d,
    TimedHarvestDims t, HarvestWork work) {
    harvest_count_stream(pushed, d, work, [&](int b, const HarvestSort &so, int *wave_cnt) {
        int row = 0;
        return harvest_update_timed(tr.of_stream(b, d.S, t.R), hs.of_stream(b, d), hclock + 3 * (int64_t)b, d, t, so,
                                    wave_cnt, row);
    });
}

// ---- host side ------------------------------------------------------------------------------------------------------
// the sizes and capacities of every harvest, the timed limits (those of the push, then settle), the pointers
static int harvest_timed_args(const char *what, const TimedView &tr, const HarvestState &hs, const int64_t *hclock,
                              const HarvestDims &d, const TimedHarvestDims &t, const HarvestLog &log) {
    int rc = harvest_size_args(what, d, log);
    if (rc == STG_OK) rc = timed_size_args(what, t.R, t.step, d.T_obs, "T_obs");
    if (rc != STG_OK) return rc;
    STG_REQUIRE(t.max_dt >= 1 && t.max_dt <= (int64_t)(d.T_obs - 1) * t.step, STG_EINVAL,
                "%s: max_dt=%lld not in [1, (T_obs - 1) * step = %lld]", what, (long long)t.max_dt,
                (long long)((int64_t)(d.T_obs - 1) * t.step));
    STG_REQUIRE(t.settle >= 0 && t.settle <= t.max_dt - 1, STG_EINVAL, "%s: settle=%lld not in [0, max_dt - 1 = %lld]",
                what, (long long)t.settle, (long long)(t.max_dt - 1));
    STG_REQUIRE(tr.slot_id && tr.t_ring && tr.xy_ring && tr.slot_head && tr.clock && tr.head_flags && hclock &&
                    harvest_pointers(hs, log),
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
