/* stgcnn_hip_harvest.h -- training windows harvested from the live tracks: part of the C ABI of libstgcnn_hip.so, included
 * by stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and status codes) and not meant
 * to be included on its own.  The binding of these entry points is social_stgcnn_amd/_lib.py's _SIGNATURES_HARVEST;
 * tests/test_harvest_cpu.py holds the two copies against each other.                                                  */
#ifndef STGCNN_HIP_HARVEST_H
#define STGCNN_HIP_HARVEST_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N10  windows for training, taken from the live tracks as they mature (added entry points, the ABI
 *      version stays).  The launch runs behind the push of the same stream(s) (stg_track_push / _rule, stg_track_push_streams
 *      / _rule) and reads that push's state -- slot_id, mask, ring, head_flags, all const here, with the same S and T_obs
 *      -- and nothing else: not the detections.  T_all = T_obs + pred_len, 2 <= T_all <= STG_HARVEST_MAX_STEPS.
 *   History (per stream, all DEVICE memory; zeros start a stream): h_word uint32[S], bit t = the slot was really detected
 *     t pushes ago; h_ring float64 (T_all,S,2); h_head int32[2] = {ring row of the last push, pushes since the zeros}.
 *   One push: every word is aged by one; a slot whose mask has bit 0 set gets bit 0 and its rounded position, copied from
 *     the track ring's row head_flags[0], in the history's next ring row; a free slot (slot_id < 0) gets an empty word.
 *     Frames a rule would fill are gaps here.  Every ring row is taken modulo its depth.
 *   Window: the candidates are the slots with all T_all low bits set, in ascending id order.  min_peds or more of them
 *     are one window ending at this push; row p of it is (2,T_all) float32: column 0 zero, column t = (float)(pos[t] -
 *     pos[t-1]), the subtraction in float64 on the rounded positions, oldest first.  These are the reference's seq_rel
 *     (utils.py:153-155) of the same tracks after the float32 cast, bit for bit.
 *   Log (one for all streams): rel_all float32 (cap_rows,2,T_all), win_start int32[cap_windows+1] with win_start[0] = 0
 *     (the caller's), win_tag int32 (cap_windows,2) = (stream, the stream's push index since its zeros), header int32[3] =
 *     {n_windows, n_rows, dropped_full}; a zero header is the empty log.  Window w holds rows win_start[w] ..
 *     win_start[w+1]-1: the layout stg_gather_windows reads.  A window that does not fit, by windows or by rows, is not
 *     written and counted in dropped_full, and so is every window after it until the header is zeroed: what the log holds
 *     is always a prefix of what the feed produced.  It never wraps.  Every store is checked against the capacities.
 *   stg_window_harvest: one stream, ONE workgroup; stream_index is the window's tag.
 *   stg_window_harvest_streams: NS streams on the (NS, ...) slices of the track state and the history; pushed int32[NS] as
 *     the push read it: a stream not pushed keeps its history bit for bit and gives no window.  The tick's windows land in
 *     stream order.  Three launches, none of which waits for another workgroup: update and count per stream; one
 *     workgroup that scans the counts, decides what fits and is the header's only writer; the rows per stream.  work:
 *     int32[NS * (S + 3)], scratch that carries the candidates from launch to launch.  Equal, bit for bit, to
 *     stg_window_harvest called stream by stream in stream order with stream_index = b.
 *   24 bytes of dynamic LDS per slot of the next power of two >= S (48 KB at the limit).  No host synchronisation; every
 *   count is read when the kernels run, so the launches are captured with the push.  Bad sizes (S above
 *   STG_TRACK_MAX_SLOTS, NS above STG_TRACK_MAX_STREAMS, T_obs < 1, T_all - T_obs < 1, min_peds < 1, capacities < 1), a
 *   negative stream_index or NULL pointers: STG_EINVAL, decided before any launch.                                      */
#define STG_HARVEST_MAX_STEPS 32
int stg_window_harvest(const int64_t *slot_id, const uint32_t *mask, const double *ring, const int32_t *head_flags, int S,
                       int T_obs, int T_all, int min_peds, int stream_index, uint32_t *h_word, double *h_ring,
                       int32_t *h_head, float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header,
                       int cap_windows, int cap_rows, void *stream);
int stg_window_harvest_streams(const int64_t *slot_id, const uint32_t *mask, const double *ring,
                               const int32_t *head_flags, const int32_t *pushed, int NS, int S, int T_obs, int T_all,
                               int min_peds, uint32_t *h_word, double *h_ring, int32_t *h_head, int32_t *work,
                               float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header, int cap_windows,
                               int cap_rows, void *stream);

#endif /* STGCNN_HIP_HARVEST_H */
