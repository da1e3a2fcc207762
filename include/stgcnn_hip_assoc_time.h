/* stgcnn_hip_assoc_time.h -- unlabelled detections -> track ids on TIMESTAMPED live pushes: part of the C ABI of
 * libstgcnn_hip.so, included by stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and
 * status codes and on its section N9) and not meant to be included on its own.  The binding of these entry points is
 * social_stgcnn_amd/_lib.py's _SIGNATURES_ASSOC_TIME; tests/test_assoc_time_cpu.py holds the two copies against each
 * other.                                                                                                              */
#ifndef STGCNN_HIP_ASSOC_TIME_H
#define STGCNN_HIP_ASSOC_TIME_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N12  the association of N9 at the tracker's own rate (added entry points, the ABI version stays).  The
 *      launch runs AHEAD of the timed push of the same stream(s) (stg_track_push_timed, stg_track_push_streams_timed):
 *      it reads the time that push will read, det_time, and the clock that push keeps, clock int64[2] = {time of the last
 *      accepted push, accepted pushes}, which it never writes.  Time is integer ticks, `step` the model's step in ticks.
 *   State (all DEVICE memory; zeros and trk_id = -1 start a stream): that of N9 with trk_t int64[C], the time of the
 *     slot's last match, in the place of trk_miss -- trk_id int64[C], trk_pos float64 (C,2), trk_vel float64 (C,2) NOW
 *     THE DISPLACEMENT PER MODEL STEP, trk_t, trk_hits int32[C], next_id int64[1], assoc_flags int32[1].
 *   Order check, the timed push's own test on t_now = det_time[0]: the push is refused iff clock[1] > 0 && t_now <=
 *     clock[0].  A refused push leaves the state bit for bit, writes -1 to the ids of the m = min(max(count, 0), M_max)
 *     detections, sets assoc_flags = STG_ASSOC_TIME_ORDER, and does nothing else.  (The timed push behind it refuses the
 *     same push by the same test and records nothing.)
 *   An accepted push runs steps 1-6 of N9 with three changes:
 *     1., 4. the number of steps is k_s = (double)(t_now - trk_t_s) / (double)step, ONE IEEE division (no fused
 *        multiply-add anywhere, as in N9), in the place of (double)(miss_s + 1): q_s = pos_s + vel_s * k_s, and for a
 *        matched pair vel_s = (p_j - pos_s) / k_s, pos_s = p_j, trk_t_s = t_now, hits_s += 1.  On a feed of one push per
 *        step, t_now - trk_t_s = (miss_s + 1) * step and the quotient is exactly miss_s + 1: ids, positions,
 *        velocities and hits are then those of N9 bit for bit.
 *     5. a live slot not matched is freed (trk_id -1, the rest zero, trk_t too) iff t_now - trk_t_s > max_age; else it is
 *        left as it is.  max_age is in ticks, 0 <= max_age < 2^31; max_age = max_miss * step is N9's lifetime.
 *     6. a new track starts with trk_t = t_now (pos = p_j, vel = 0, hits = 1).
 *     The gates are the caller's distances whatever the gap, as in N9, whose gates do not grow with miss either.
 *   Precondition: k_s > 0 for every live slot of an accepted push.  It holds when the association state is the kernel's
 *     own and is cleared together with the clock: a live slot's trk_t is the time of an accepted push, so trk_t_s <=
 *     clock[0] < t_now.  A state written by anything else, or a clock cleared without it, is the caller's error: the
 *     result is then unspecified, though nothing is read or written out of bounds.  |times| < 2^62, as for the push.
 *   stg_associate_timed: one workgroup of 1,024 threads; det_xy float64 (M_max,2), det_count int32[1], det_time
 *     int64[1], det_id int64[M_max].
 *   stg_associate_streams_timed: one workgroup of 256 threads per stream on the (NS, ...) slices of the state, det_id /
 *     det_xy with strides, M_total, det_start and pushed as stg_track_push_streams_timed reads them, det_time int64[NS],
 *     clock int64 (NS,2): every stream on its own clock.  A stream not pushed keeps its state bit for bit -- its flags
 *     too -- and its ids are not written.  Equal, bit for bit, to the lone entry point called stream by stream.
 *   The matching rounds, the LDS (28 bytes per track slot and 20 per detection) and the limits are N9's.  Sizes above
 *   STG_ASSOC_MAX_*, step >= 2^31: STG_EUNSUPPORTED; bad sizes, gates, step < 1, max_age outside [0, 2^31) or NULL
 *   pointers: STG_EINVAL; both decided before any launch, with a stg_last_error message.  Every count, range, time and
 *   state word is read when the kernel runs, so one captured graph serves every push.  No host synchronisation.        */
#define STG_ASSOC_TIME_ORDER 2 /* the push's time is not after the stream's last accepted push: ids -1, nothing changed */
int stg_associate_timed(int64_t *det_id, const double *det_xy, const int32_t *det_count, const int64_t *det_time,
                        const int64_t *clock, int M_max, int64_t *trk_id, double *trk_pos, double *trk_vel,
                        int64_t *trk_t, int32_t *trk_hits, int64_t *next_id, int32_t *assoc_flags, int C, double scale,
                        double gate2, double gate_new2, int64_t step, int64_t max_age, void *stream);
int stg_associate_streams_timed(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride, int M_total,
                                const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                const int64_t *clock, int NS, int M_max, int64_t *trk_id, double *trk_pos,
                                double *trk_vel, int64_t *trk_t, int32_t *trk_hits, int64_t *next_id,
                                int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int64_t step,
                                int64_t max_age, void *stream);

#endif /* STGCNN_HIP_ASSOC_TIME_H */
