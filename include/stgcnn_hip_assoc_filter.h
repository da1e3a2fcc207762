/* stgcnn_hip_assoc_filter.h -- unlabelled, NOISY detections -> track ids on timestamped live pushes, with a filtered
 * track state: part of the C ABI of libstgcnn_hip.so, included by stgcnn_hip.h (inside its extern "C" block; it relies on
 * that header's types, limits and status codes and on its sections N9 and N12) and not meant to be included on its own.
 * The binding of these entry points is social_stgcnn_amd/_lib.py's _SIGNATURES_ASSOC_FILTER;
 * tests/test_assoc_filter_cpu.py holds the two copies against each other.                                            */
#ifndef STGCNN_HIP_ASSOC_FILTER_H
#define STGCNN_HIP_ASSOC_FILTER_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N13  the association of N12 with a constant-velocity Kalman filter per track and a gate that follows the predicted
 *      uncertainty (added entry points, the ABI version stays).  The launch runs AHEAD of the timed push
 *      as N12's does, and everything N12 says of det_time, clock, the order check and the refused push (ids -1,
 *      assoc_flags = STG_ASSOC_TIME_ORDER, the state bit for bit), of k_s = (double)(t_now - trk_t_s) / (double)step (ONE
 *      IEEE division), of max_age, of births in detection order, of STG_ASSOC_FULL and of the precondition k_s > 0 holds
 *      here word for word.  What changes:
 *   State: N12's arrays and trk_cov float64 (C,3) = {p00, p01, p11}, the covariance of (position, velocity per model
 *     step) of ONE axis; both axes share it, the model being isotropic.  trk_pos is the FILTERED position, trk_vel the
 *     FILTERED velocity per model step.  trk_hits is kept and counted and chooses no gate.
 *   Parameters, squared by the caller in float64: r = sigma_det^2 (m^2), qa = sigma_acc^2 (m^2 per step^3), v0 =
 *     sigma_vel0^2, n2 = gate_sigmas^2, gmax2 = gate_max^2.  r, v0, n2, gmax2 finite and > 0, qa finite and >= 0.
 *   Every expression below is float64, one IEEE operation at a time in the order written, parentheses included, with no
 *   fused multiply-add and IEEE division; x/2 and x/3 are divisions by 2.0 and 3.0.
 *   1. prediction of a live slot over k = k_s:
 *        q   = pos + vel * k                                  (per axis, as in N12)
 *        w   = qa * k
 *        a11 = p11 + w
 *        u   = k * p11
 *        a01 = (p01 + u) + (w * k) / 2
 *        a00 = (p00 + k * (2 * p01 + u)) + ((w * k) * k) / 3
 *        S   = a00 + r                                        (> 0 because r > 0 and a00 >= 0)
 *        g2  = min(n2 * S, gmax2)                             the slot's squared gate: it grows with the gap and with a
 *                                                             young track's unknown velocity; gate_max bounds it
 *   2. a pair (s, j) is a candidate iff |q_s - p_j|^2 <= g2_s, the squared distance as in N9.  The order of the
 *      matching stays N9's: globally greedy by (squared EUCLIDEAN distance, slot, detection).  The Mahalanobis distance
 *      |q - p|^2 / S is deliberately not the order: the rounds then stay the code N9 and N12 run, and ties stay
 *      decidable on an integer grid, where |q - p|^2 is exact and a quotient by S is not.
 *   3. a matched pair, with a00, a01, a11, S of 1. recomputed from the state:
 *        K0 = a00 / S,  K1 = a01 / S
 *        per axis  e = p - q,  pos = q + K0 * e,  vel = vel + K1 * e
 *        p00 = a00 - K0 * a00,  p01 = a01 - K0 * a01,  p11 = a11 - K1 * a01
 *        trk_t = t_now,  hits += 1
 *   4. a live slot not matched is freed (every word zero, trk_cov too, trk_id -1) iff t_now - trk_t > max_age; else it is
 *      untouched: its uncertainty grows through k at the next push.
 *   5. a birth: pos = p, vel = 0, trk_cov = {r, 0, v0}, trk_t = t_now, hits = 1.
 *   stg_associate_filtered: one workgroup of 1,024 threads; the arrays of stg_associate_timed and trk_cov.
 *   stg_associate_streams_filtered: one workgroup of 256 threads per stream on the (NS, ...) slices, trk_cov (NS,C,3);
 *     every stream on its own clock.  A stream not pushed keeps its state bit for bit and its ids are not written.
 *     Equal, bit for bit, to the lone entry point called stream by stream.
 *   The matching rounds and the limits are N9's; the LDS is 36 bytes per track slot (N9's 28 and the slot's gate) and 20
 *   per detection, 114,688 bytes at both limits.  Covariance and gain are recomputed in the update from the state;
 *   nothing of them is kept in LDS.  Sizes above STG_ASSOC_MAX_*, step >= 2^31: STG_EUNSUPPORTED; bad sizes, parameters,
 *   step < 1, max_age outside [0, 2^31) or NULL pointers: STG_EINVAL; both decided before any launch, with a
 *   stg_last_error message.  Every count, range, time and state word is read when the kernel runs, so one captured graph
 *   serves every push.  No host synchronisation.                                                                       */
int stg_associate_filtered(int64_t *det_id, const double *det_xy, const int32_t *det_count, const int64_t *det_time,
                           const int64_t *clock, int M_max, int64_t *trk_id, double *trk_pos, double *trk_vel,
                           int64_t *trk_t, double *trk_cov, int32_t *trk_hits, int64_t *next_id, int32_t *assoc_flags,
                           int C, double scale, double r, double qa, double v0, double n2, double gmax2, int64_t step,
                           int64_t max_age, void *stream);
int stg_associate_streams_filtered(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                   int M_total, const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                   const int64_t *clock, int NS, int M_max, int64_t *trk_id, double *trk_pos,
                                   double *trk_vel, int64_t *trk_t, double *trk_cov, int32_t *trk_hits, int64_t *next_id,
                                   int32_t *assoc_flags, int C, double scale, double r, double qa, double v0, double n2,
                                   double gmax2, int64_t step, int64_t max_age, void *stream);

#endif /* STGCNN_HIP_ASSOC_FILTER_H */
