// harvest: training windows taken from the live tracks as they mature.  A track detected in each of
// the last T_all = obs_len + pred_len pushes of its stream is one row of a reference TrajectoryDataset window (utils.py:
// 130-165, with the window's future now known); the rows of one push, at least min_peds of them in ascending id order,
// are one window, appended to a log in the layout DeviceWindows / stg_gather_windows read.
//
//   stg_window_harvest          one stream: ONE workgroup, behind stg_track_push of the same push.  It reads the track
//                               state only (slot ids, presence bit 0, the ring row the push has just written), keeps its
//                               own T_all-deep history, sorts the candidates by id (detections.hpp), places the window
//                               and writes its rows.  The frame, the tail and the streams' body are harvest_parts.hpp's,
//                               shared with harvest_time.hip: this file says where "seen" comes from.
//   stg_window_harvest_streams  NS streams behind stg_track_push_streams, three launches that never wait for each other:
//                               update + count (one workgroup per stream, honours pushed[b]); place (ONE workgroup: the
//                               exclusive scan of the tick's row counts, the capacity test and the header's only
//                               writer); write (one workgroup per stream).  The log is tick-major, stream-minor.
//
// THE LOG IS CLOSED BY ITS FIRST DROP: a window that does not fit (by windows or by rows) is counted in dropped_full and
// from then on every window is, until the caller clears the header.  What the log holds is therefore always a prefix of
// what the feed produced, and the capacity test of a tick is monotone in the stream index.
// Integer work, float64 loads and one float32 conversion per element.  Plain C++ stores; LDS atomics on integer words
// only.  No host synchronisation: everything is read when the kernels run, so the launches are captured with the push.
#include "harvest_parts.hpp"

namespace stg {

// One push of one stream's history by one workgroup, behind the track push; `push` = the pushes before it, as
// hs.head[1] counts them.  harvest_frame (harvest_parts.hpp) with this family's answer to "seen in this frame?": bit 0
// of the slot's presence mask, and the position the push has just written to the track ring.
__device__ __forceinline__ int harvest_update(const TrackView &tr, const HarvestState &hs, const HarvestDims &d, int push,
                                              const HarvestSort &so, int *wave_cnt, int &row) {
    const int trow = ring_row(tr.head_flags[0], d.T_obs);  // the track ring's row of this push
    const double *__restrict__ src = tr.ring + (int64_t)trow * d.S * 2;
    return harvest_frame(
        tr.slot_id, hs, d, false, push + 1, so, wave_cnt, row,
        [&](int s, double &x, double &y) {
            if ((tr.mask[s] & 1u) == 0) return false;        // not really detected in this push
            x = src[s * 2];
            y = src[s * 2 + 1];
            return true;
        },
        [] {});
}

// ---- one stream ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void window_harvest_kernel(TrackView tr, HarvestState hs, HarvestDims d,
                                                                         HarvestLog log, int stream_index) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int wave_cnt[kHarvestWaves];
    const HarvestSort so(lds, d.S);
    const HarvestHeader at(log);
    const int push = hs.head[1];                             // the window's tag
    int row;
    const int c = harvest_update(tr, hs, d, push, so, wave_cnt, row);
    harvest_append(hs, d, log, at, c, row, so, stream_index, push);
}

// ---- NS streams: update + count, place, write --------------------------------------------------------------------------
__global__ __launch_bounds__(kHarvestThreads) void harvest_update_streams_kernel(TrackView tr,
                                                                                 const int32_t *__restrict__ pushed,
                                                                                 HarvestState hs, HarvestDims d,
                                                                                 HarvestWork work) {
    harvest_count_stream(pushed, d, work, [&](int b, const HarvestSort &so, int *wave_cnt) {
        const HarvestState mine = hs.of_stream(b, d);
        int row;
        return harvest_update(tr.of_stream(b, d), mine, d, mine.head[1], so, wave_cnt, row);
    });
}

// ONE workgroup: stream b's window (count[b] rows, 0 = none) goes behind the windows of the streams before it.  The
// exclusive scan counts every window of the tick, placed or not, so the test is monotone: behind the first window that
// does not fit none does.  The only writer of the header, of win_start and of win_tag.
__global__ __launch_bounds__(kHarvestThreads) void harvest_place_kernel(const int32_t *__restrict__ head, HarvestDims d,
                                                                        HarvestWork work, HarvestLog log, int NS) {
    __shared__ int wave_tot[kHarvestWaves];
    __shared__ int sums[3];                                  // windows placed, rows placed, windows dropped
    const int tid = threadIdx.x;
    const int nw0 = log.header[0], nr0 = log.header[1], dropped0 = log.header[2];
    if (tid < 3) sums[tid] = 0;
    __syncthreads();
    int64_t base_r = 0, base_w = 0;
    int placed = 0, rows = 0, drops = 0;
    for (int b0 = 0; b0 < NS; b0 += kHarvestThreads) {
        const int b = b0 + tid;
        int c = b < NS ? work.count[b] : 0;
        c = c < 0 ? 0 : (c > d.S ? d.S : c);
        const int w = c > 0 ? 1 : 0;
        int tot_r, tot_w;
        const int before_r = block_scan(c, &tot_r, wave_tot);
        const int before_w = block_scan(w, &tot_w, wave_tot);
        const int64_t r0 = nr0 + base_r + before_r, wi = nw0 + base_w + before_w;
        const bool fits = w && harvest_fits(log, dropped0, wi, r0, c);
        if (b < NS) {
            work.place[2 * b] = fits ? (int32_t)r0 : -1;
            work.place[2 * b + 1] = fits ? (int32_t)wi : -1;
        }
        if (fits) {
            log.win_start[wi + 1] = (int32_t)(r0 + c);
            log.win_tag[wi * 2] = b;
            log.win_tag[wi * 2 + 1] = head[2 * b + 1] - 1;   // (update has counted this push already)
            placed += 1;
            rows += c;
        } else {
            drops += w;
        }
        base_r += tot_r;
        base_w += tot_w;
    }
    if (placed) {
        atomicAdd(&sums[0], placed);
        atomicAdd(&sums[1], rows);
    }
    if (drops) atomicAdd(&sums[2], drops);
    __syncthreads();
    if (tid == 0) {
        log.header[0] = nw0 + sums[0];
        log.header[1] = nr0 + sums[1];
        log.header[2] = dropped0 + sums[2];
    }
}

__global__ __launch_bounds__(kHarvestThreads) void harvest_write_streams_kernel(HarvestState hs, HarvestDims d,
                                                                                HarvestWork work, HarvestLog log) {
    const int b = blockIdx.x;
    const HarvestWork mine = work.of_stream(b, d);
    const int row0 = mine.place[0];
    if (row0 < 0) return;
    int c = mine.count[0];
    c = c < 0 ? 0 : (c > d.S ? d.S : c);
    const HarvestState st = hs.of_stream(b, d);
    harvest_rows(st.ring, d, log, row0, c, ring_row(st.head[0], d.T_all), [&](int p) { return mine.cand[p]; });
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int harvest_args(const char *what, const TrackView &tr, const HarvestState &hs, const HarvestDims &d,
                        const HarvestLog &log) {
    const int rc = harvest_size_args(what, d, log);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(tr.slot_id && tr.mask && tr.ring && tr.head_flags && harvest_pointers(hs, log), STG_EINVAL,
                "%s: null pointer", what);
    return STG_OK;
}

int harvest_place_write(const char *what, const HarvestState &hs, const HarvestDims &d, const HarvestWork &wk,
                        const HarvestLog &log, int NS, hipStream_t st) {
    const int rc = launch({what, dim3(1), dim3(kHarvestThreads), 0, st}, harvest_place_kernel, (const int32_t *)hs.head, d,
                          wk, log, NS);
    if (rc != STG_OK) return rc;
    return launch({what, dim3(NS), dim3(kHarvestThreads), 0, st}, harvest_write_streams_kernel, hs, d, wk, log);
}

}  // namespace stg

extern "C" {

int stg_window_harvest(const int64_t *slot_id, const uint32_t *mask, const double *ring, const int32_t *head_flags, int S,
                       int T_obs, int T_all, int min_peds, int stream_index, uint32_t *h_word, double *h_ring,
                       int32_t *h_head, float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header,
                       int cap_windows, int cap_rows, void *stream) {
    const char *what = "stg_window_harvest";
    const stg::TrackView tr{slot_id, mask, ring, head_flags};
    const stg::HarvestState hs{h_word, h_ring, h_head};
    const stg::HarvestDims d{S, T_obs, T_all, min_peds};
    const stg::HarvestLog log{rel_all, win_start, win_tag, header, cap_windows, cap_rows};
    const int rc = stg::harvest_args(what, tr, hs, d, log);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(stream_index >= 0, STG_EINVAL, "%s: bad stream_index=%d", what, stream_index);
    return stg::launch({what, dim3(1), dim3(stg::kHarvestThreads), stg::harvest_lds(d), stg::as_stream(stream), 64 * 1024},
                       stg::window_harvest_kernel, tr, hs, d, log, stream_index);
}

int stg_window_harvest_streams(const int64_t *slot_id, const uint32_t *mask, const double *ring,
                               const int32_t *head_flags, const int32_t *pushed, int NS, int S, int T_obs, int T_all,
                               int min_peds, uint32_t *h_word, double *h_ring, int32_t *h_head, int32_t *work,
                               float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header, int cap_windows,
                               int cap_rows, void *stream) {
    const char *what = "stg_window_harvest_streams";
    const stg::TrackView tr{slot_id, mask, ring, head_flags};
    const stg::HarvestState hs{h_word, h_ring, h_head};
    const stg::HarvestDims d{S, T_obs, T_all, min_peds};
    const stg::HarvestLog log{rel_all, win_start, win_tag, header, cap_windows, cap_rows};
    STG_REQUIRE(NS >= 1 && NS <= STG_TRACK_MAX_STREAMS, STG_EINVAL, "%s: bad size NS=%d", what, NS);
    int rc = stg::harvest_args(what, tr, hs, d, log);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(pushed && work, STG_EINVAL, "%s: null pointer", what);
    const stg::HarvestWork wk = stg::HarvestWork::carve(work, NS, S);
    hipStream_t st = stg::as_stream(stream);
    rc = stg::launch({what, dim3(NS), dim3(stg::kHarvestThreads), stg::harvest_lds(d), st, 64 * 1024},
                     stg::harvest_update_streams_kernel, tr, pushed, hs, d, wk);
    if (rc != STG_OK) return rc;
    return stg::harvest_place_write(what, hs, d, wk, log, NS, st);
}

}  // extern "C"
