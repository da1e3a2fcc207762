/* stgcnn_hip_harvest_time.h -- training windows harvested from TIMESTAMPED live pushes: part of the C ABI of
 * libstgcnn_hip.so, included by stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and
 * status codes and on stgcnn_hip_harvest.h) and not meant to be included on its own.  The binding of these entry points is
 * social_stgcnn_amd/_lib.py's _SIGNATURES_HARVEST_TIME; tests/test_harvest_time_cpu.py holds the two copies against each
 * other.                                                                                                              */
#ifndef STGCNN_HIP_HARVEST_TIME_H
#define STGCNN_HIP_HARVEST_TIME_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N11  windows for training from timed pushes (added entry points, the ABI version stays).  The launch
 *      runs behind the timed push of the same stream(s) (stg_track_push_timed, stg_track_push_streams_timed) and reads the
 *      state that push has left -- slot_id (S), t_ring (S,R), xy_ring (S,R,2), slot_head (S,2), clock (2), head_flags (2),
 *      all const here, with the same S, R, T_obs, scale, step and max_dt -- and nothing else: not the detections.  It
 *      resamples the tracks on the model's step grid; each resolved grid instant is one frame of the harvest of
 *      stgcnn_hip_harvest.h, whose log, rows and capacity rule these are.
 *   History (per stream, all DEVICE memory; zeros start a stream): h_word uint32[S] and h_ring float64 (T_all,S,2) as in
 *     the untimed harvest, bit t = the slot was observed t frames ago; h_head int32[2] = {ring row of the last frame, j =
 *     grid instants passed since the zeros (it saturates at 2^31 - 1)}; h_clock int64[3] = {anchored 0/1, g0, instants
 *     skipped}.
 *   One launch.  Nothing at all -- the history bit for bit, no window -- when the push was refused (STG_TRACK_TIME_ORDER
 *     in head_flags[1], read on the device) or, in the streams form, the stream was not pushed.  The first accepted push
 *     anchors the grid, g0 = clock[0], g_i = g0 + i * step.  With t_now = clock[0] the pending instants are g_j ..
 *     g_{j+K-1}, those with g_i <= t_now - settle (K in int64).  K = 0: nothing changes, no word ages.  K >= 2: the K - 1
 *     older instants are skipped -- every word of the stream is zeroed first and h_clock[2] += K - 1.  The newest pending
 *     instant g is resolved as a frame, and j += K.
 *   Frame at g: a slot with slot_id >= 0 is observed under the timed push's own test on what its ring holds now: a sample
 *     at exactly g (the position as it is), or samples ta < g < tb next to each other with tb - ta <= max_dt (per
 *     coordinate round(pa + (pb - pa) * ((double)(g - ta) / (double)(tb - ta))), one IEEE operation at a time, rounded
 *     by `scale`).  Every word is aged by one; an observed slot gets bit 0 and its position in the history's next ring
 *     row; a free slot gets an empty word.  A slot need not be detected in this push to be observed.
 *   Window: as in the untimed harvest -- the slots with all T_all low bits set, ascending ids, min_peds or more, the same
 *     rows, log, header and closed-by-first-drop rule.  win_tag = (stream, grid index of the window's last frame): that
 *     instant is g0 + tag * step.
 *   settle, 0 <= settle <= max_dt - 1, is how long an instant waits for the sample behind it: with max_dt - 1 every
 *     bracket the rule allows around g has arrived when g is resolved.  The ring must still hold the sample at or before
 *     g by then: R at least the samples of settle + max_dt ticks plus one push interval; a shallower ring makes the frame
 *     a gap, never a wrong position.
 *   stg_window_harvest_timed: one stream, ONE workgroup; stream_index is the window's tag.
 *   stg_window_harvest_streams_timed: NS streams on the (NS, ...) slices of the state and the history (h_clock (NS,3));
 *     pushed int32[NS] as the push read it; work int32[NS * (S + 3)].  Three launches as stg_window_harvest_streams, the
 *     first one timed.  Equal, bit for bit, to the lone entry point called stream by stream in stream order.
 *   Dynamic LDS as the untimed harvest.  No host synchronisation: everything, the time included, is read when the kernels
 *   run, so the launches are captured with the push.  STG_EINVAL, decided before any launch: the untimed harvest's bad
 *   sizes, R < 2, step < 1, max_dt outside [1, (T_obs - 1) * step], settle outside [0, max_dt - 1], a negative
 *   stream_index, NULL pointers.  STG_EUNSUPPORTED: R > STG_TRACK_MAX_HISTORY, step * T_obs >= 2^31.                    */
int stg_window_harvest_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                             const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags, int S, int R,
                             int T_obs, int T_all, int min_peds, double scale, int64_t step, int64_t max_dt,
                             int64_t settle, int stream_index, uint32_t *h_word, double *h_ring, int32_t *h_head,
                             int64_t *h_clock, float *rel_all, int32_t *win_start, int32_t *win_tag, int32_t *header,
                             int cap_windows, int cap_rows, void *stream);
int stg_window_harvest_streams_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                                     const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags,
                                     const int32_t *pushed, int NS, int S, int R, int T_obs, int T_all, int min_peds,
                                     double scale, int64_t step, int64_t max_dt, int64_t settle, uint32_t *h_word,
                                     double *h_ring, int32_t *h_head, int64_t *h_clock, int32_t *work, float *rel_all,
                                     int32_t *win_start, int32_t *win_tag, int32_t *header, int cap_windows,
                                     int cap_rows, void *stream);

#endif /* STGCNN_HIP_HARVEST_TIME_H */
