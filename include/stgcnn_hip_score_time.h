/* stgcnn_hip_score_time.h -- the time-indexed score of the live path: part of the C ABI of libstgcnn_hip.so, included by
 * stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and status codes) and not meant
 * to be included on its own.  The binding of these entry points is social_stgcnn_amd/_lib.py's _SIGNATURES_SCORE_TIME;
 * tests/test_score_time_cpu.py holds the two copies against each other.                                              */
#ifndef STGCNN_HIP_SCORE_TIME_H
#define STGCNN_HIP_SCORE_TIME_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* Timed predictions scored by TIME (added entry points, the ABI version stays).  The launch runs behind
 * the timed push of the same tick (stg_track_push_timed / _streams_timed) and reads that push's state: slot_id, t_ring,
 * xy_ring, slot_head, clock and head_flags, all const here, with the same S, R, scale, step and max_dt.  Per stream:
 *   Nothing happens -- the state keeps every bit, push_totals / push_traj are zero, no record is made -- for a stream
 *     not pushed and for a push the track kernel refused (STG_TRACK_TIME_ORDER in head_flags[1], read on the device).
 *   Records: accepted push number n (0, 1, ... since the state was cleared; an empty push counts) leaves a record in
 *     row n mod Rp: rec_t = t_now = clock[0], the scene's ids and num_peds (clamped to [0, V]), mean, the cumulative
 *     covariance and the K samples as N8 keeps them.  rec_status: 0 empty, 1 pending, 2 retired.  The record is written
 *     last, after scoring and retirement; a row whose occupant is still pending is overwritten and counters[1]
 *     (evictions) advances.  A pending occupant cannot have steps == P, so no full trajectory is ever lost.
 *   Truth: only a track whose newest sample (tb, pb) has tb == t_now takes part; (ta, pa) is the sample before it in
 *     its ring, if the ring holds one.  For a pending record with the track's id at column v < num_peds and h = 1..P in
 *     ascending order, tau = rec_t + h * step:
 *       tau == tb                           the truth is pb, no arithmetic is done;
 *       ta < tau < tb, tb - ta <= max_dt    per coordinate round(pa + (pb - pa) * ((double)(tau - ta) / (double)(tb -
 *                                           ta))), float64 with IEEE operations as written: the timed push's window rule;
 *       ta < tau < tb, tb - ta >  max_dt    that (record, h, v) stays unmatched for good;
 *       anything else                       not this push.
 *     The truth is converted to float32.  It depends on the track state: a detection dropped for lack of a slot
 *     (STG_TRACK_OVERFLOW) is not truth.  The brackets of a track are disjoint, so every (record, h, v) is scored at most
 *     once.
 *   Values: err, d2, nll, best, acc[k], acc_mean and steps exactly as N8, written into the record's own tables matched
 *     int32, err, d2, nll, best float32 (NS,Rp,P,V) (several records can have a horizon in one bracket, so a per-push
 *     (P,V) output cannot hold them).
 *   Retirement: after scoring, a pending record with t_now >= rec_t + P * step is retired: traj_steps int32, traj_ade,
 *     traj_fde, traj_ade_mean, traj_fde_mean float32 (NS,Rp,V) as N8 defines them go into its row, and a pedestrian with
 *     steps == P enters traj_totals.  Several records may retire in one push.  A track not detected in the retiring push
 *     loses its horizon P even where a later bracket would have covered it.
 *   Totals: totals float64 (NS,P,5+Q) and traj_totals (NS,5) with the columns of N8, summed without atomics in an order
 *     fixed by the launch shape; push_totals (NS,P,5+Q) and push_traj (NS,5) are what this push added.
 *   State (stg_score_timed_state, NS leading, all DEVICE memory; zeros start a stream): rec_t int64 (NS,Rp), rec_status,
 *     rec_peds int32 (NS,Rp), rec_ids int64 (NS,Rp,V), rec_mean (NS,Rp,P,V,2), rec_cov (NS,Rp,P,V,3), rec_samples
 *     (NS,Rp,K,P,V,2), acc (NS,Rp,K,V), acc_mean (NS,Rp,V) float32, steps int32 (NS,Rp,V), the tables and the traj_* rows
 *     above, counters int64 (NS,2) = {accepted pushes, evictions}, totals, traj_totals.  Columns v >= num_peds of a row
 *     are not part of the contract.  Rp*V*(28 + 36P) bytes per stream beside the totals, and Rp*V*(8KP + 4K + 4P + 8)
 *     more with samples.
 *   Fed pushes at t = f * step with max_dt = step, no OVERFLOW and Rp >= P, the entries (record of push m, horizon h)
 *   are bit for bit what stg_score_push reports at push m+h in row h-1, and the retired rows its traj_* of push m+P.
 *   NULL samples or K == 0 skips every sample-based value: rec_samples, acc, best, traj_ade, traj_fde may then be NULL.
 *   stg_score_push_timed: one stream (always pushed).  stg_score_push_streams_timed: one workgroup per stream on the
 *   (NS, ...) slices, `pushed` int32[NS] as the push reads it; NS == 0 is a no-op.  One workgroup of 256 threads per
 *   stream, 12 bytes of dynamic LDS per track slot (24 KB at the limit), plain stores, no host synchronisation.  Sizes
 *   above STG_SCORE_MAX_PENDING, the STG_SCORE_MAX_* or the STG_TRACK_MAX_* limits (and step * P >= 2^31):
 *   STG_EUNSUPPORTED; bad sizes, NULL required pointers, mean / samples not 8-byte aligned, step < 1 or max_dt outside
 *   [1, 2^31): STG_EINVAL; both decided before any launch.                                                          */
#define STG_SCORE_MAX_PENDING 1024
typedef struct stg_score_timed_state {
    int64_t *rec_t;
    int32_t *rec_status, *rec_peds;
    int64_t *rec_ids;
    float *rec_mean, *rec_cov, *rec_samples, *acc, *acc_mean;
    int32_t *steps, *matched;
    float *err, *d2, *nll, *best;
    int32_t *traj_steps;
    float *traj_ade, *traj_fde, *traj_ade_mean, *traj_fde_mean;
    int64_t *counters;
    double *totals, *traj_totals;
} stg_score_timed_state;
typedef struct stg_score_timed_out {
    double *push_totals, *push_traj;
} stg_score_timed_out;
int stg_score_push_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring, const int32_t *slot_head,
                         const int64_t *clock, const int32_t *head_flags, int S, int R, double scale, int64_t step,
                         int64_t max_dt, const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf,
                         int64_t p_sp, int64_t p_sv, const float *samples, const int64_t *ids, const int32_t *num_peds,
                         int P, int V, int K, int Rp, const stg_score_timed_state *state, const float *thr, int Q,
                         const stg_score_timed_out *out, void *stream);
int stg_score_push_streams_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                                 const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags,
                                 const int32_t *pushed, int NS, int S, int R, double scale, int64_t step, int64_t max_dt,
                                 const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp,
                                 int64_t p_sv, const float *samples, const int64_t *ids, const int32_t *num_peds, int P,
                                 int V, int K, int Rp, const stg_score_timed_state *state, const float *thr, int Q,
                                 const stg_score_timed_out *out, void *stream);

#endif /* STGCNN_HIP_SCORE_TIME_H */
