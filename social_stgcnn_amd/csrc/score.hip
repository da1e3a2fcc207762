// score: live predictions scored against the tracks that follow, on the device.
//
// The rule, per stream.  Pushes are numbered 0, 1, ... since the state was cleared; a push with no detections is a
// push, a stream that is not pushed does not advance.  Push m leaves a RECORD in row m mod P of the state's ring: its
// scene's ids (V) and num_peds, the mean trajectory (P,V,2), the K sampled trajectories (K,P,V,2) and the cumulative
// covariance (P,V,3): C_h = sum_{t<=h} [sx^2, rho sx sy, sy^2]_t with sx = expf(v_pred[2]), sy = expf(v_pred[3]),
// rho = tanhf(v_pred[4]) -- the terms of sample_draw.hpp -- summed in float32 in ascending t.  The per-step draws are
// independent, so the absolute position at horizon h is N(mean_h, C_h).
//
//   truth    of id i at push m: its first detection among the first min(count, M_max) detections of the push, rounded
//            as the push kernel rounds (rint(x * scale) / scale in float64) and then converted to float32.  Taken from
//            the detections, not from the track state: it depends neither on the slots nor on a TrackRule.
//   values   at push m the pending record of push m-h (h = 1..P, as far as pushes exist) is scored at its step h.  For
//            each of its pedestrians v < num_peds: matched = found among the detections.  Where matched, with
//            dx, dy = mean_h - truth in float32 and (cxx, cxy, cyy) = C_h, every operation in float32 as written (no
//            fused multiply-add):
//              err  = sqrtf(dx*dx + dy*dy)
//              det  = fmaxf(cxx*cyy - cxy*cxy, (cxx*cyy) * 2^-15)   (floored where the difference is rounding noise)
//              d2   = (cyy*(dx*dx) - 2*cxy*dx*dy + cxx*(dy*dy)) / det
//              nll  = 0.5*d2 + 0.5*log(det) + log(2 pi), log(det) the correctly rounded float32 logarithm (taken in
//                     float64 and rounded), log(2 pi) the float32 constant
//              best = min_k |samples[k,h] - truth|
//            and the record's accumulators advance: acc[k] += |samples[k,h] - truth|, acc_mean += err, steps += 1.
//            Unmatched, padded and not yet existing entries are 0, and -1 in rec_ids.
//   outputs  per horizon rec_ids (P,V) (row h-1: the scene of push m-h), matched, err, d2, nll, best (P,V); from the
//            record that turns P pushes old: traj_steps (V), traj_ade = min_k acc[k] / steps, traj_fde = best at h = P
//            (0 if unmatched there), traj_ade_mean = acc_mean / steps, traj_fde_mean = err at h = P.  With steps == P
//            traj_ade / traj_fde are the reference's per-pedestrian best-of-K ADE / FDE.
//   totals   float64 (P, 5+Q) per stream: matched count, sum err, sum d2, sum nll, sum best, and for each of the Q
//            thresholds the number with d2 <= thr_q; traj_totals (5): the number of full trajectories (steps == P)
//            and the sums of their four errors.
//   order    score the pending records; retire the oldest; only then, behind a barrier, write this push's record into
//            the retired row (m mod P) and zero its accumulators.
//   A stream not pushed keeps its state bit for bit and gets all-zero outputs (ids -1).
//
// One workgroup per stream:
//   sort     the detections by (id, index), a bitonic network in LDS: the push kernel's load, sort and lookup
//            (detections.hpp), so the truth of a repeated id is the detection the scene took
//   score    a wave per horizon h (wave w takes h = w+1, w+1+waves, ...), a lane per pedestrian: lower bound of the
//            record's id in the sorted keys, then the loop over k -- the reads of samples[k,h,:] are contiguous in v.
//            The row of a horizon belongs to one wave, so its accumulators are plain read-modify-writes
//   totals   a lane sums its pedestrians in ascending v in float64, the wave adds the 64 partials by a fixed butterfly
//            and lane 0 adds the sum to the stream's totals: the workgroup owns them, no atomics, the same order
//            every run
//   retire   the wave of h = P writes the trajectory outputs from the accumulators it has just advanced
//   enqueue  behind a barrier: ids, the running covariance sum, and the pedestrians' columns of mean and samples into
//            row m mod P
// No host synchronisation (the launch is captured into the live predictors' graph), plain C++ stores only, 24 KB of
// dynamic LDS at the 2,048-detection limit (under the 64 KB the launches name: the kernel's limit is never raised).
//
// The arithmetic of `values`, the trajectory values and totals columns, the covariance sum and the column copies of the
// enqueue and the host's checks of the prediction are score_fn.hpp's, shared with score_time.hip.  This
// file keeps what is its own: the truth from the sorted detections, a wave per horizon, the launch's outputs.
#include "detections.hpp"
#include "score_fn.hpp"

namespace stg {

struct ScoreArgs {
    ScorePred pred;
    stg_score_state st;
    const float *thr;
    stg_score_out out;
    int NS, P, V, K, Q, M_max, M2;
    double scale;
};

// the outputs of a stream that has nothing to report
__device__ __forceinline__ void score_empty(const ScoreArgs &a, int b) {
    const int P = a.P, V = a.V, tid = threadIdx.x;
    const int64_t o = (int64_t)b * P * V;
    for (int e = tid; e < P * V; e += kScoreThreads) {
        a.out.rec_ids[o + e] = -1;
        a.out.matched[o + e] = 0;
        a.out.err[o + e] = 0.f;
        a.out.d2[o + e] = 0.f;
        a.out.nll[o + e] = 0.f;
        if (a.out.best) a.out.best[o + e] = 0.f;
    }
    for (int v = tid; v < V; v += kScoreThreads) {
        const int64_t x = (int64_t)b * V + v;
        a.out.traj_steps[x] = 0;
        if (a.out.traj_ade) a.out.traj_ade[x] = 0.f;
        if (a.out.traj_fde) a.out.traj_fde[x] = 0.f;
        a.out.traj_ade_mean[x] = 0.f;
        a.out.traj_fde_mean[x] = 0.f;
    }
}

// One push of stream b by one workgroup of kScoreThreads threads: `count` detections of `det` (live_args.hpp).
// LDS (dynamic): sort keys (M2 x int64), sort indices (M2 x int32)
__device__ __forceinline__ void score_push_body(const ScoreArgs &a, int b, const Detections &det, int count) {
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + a.M2);

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int P = a.P, V = a.V, K = a.K, Q = a.Q, W = kScoreCols + Q;
    const int m = count < 0 ? 0 : (count > a.M_max ? a.M_max : count);

    // the stream's slices of the state
    int32_t *hd = a.st.head + 2 * b;
    // the ring row of this push and the number of records that exist (clamped: a state that was never cleared must
    // not index outside its arrays)
    const int head = (int)((uint32_t)hd[0] % (uint32_t)P), filled = hd[1] < 0 ? 0 : (hd[1] > P ? P : hd[1]);
    int64_t *rec_ids = a.st.rec_ids + (int64_t)b * P * V;
    int32_t *rec_peds = a.st.rec_peds + (int64_t)b * P;
    const ScoreRows tab = {a.st.rec_mean + (int64_t)b * P * P * V * 2,
                            a.st.rec_cov + (int64_t)b * P * P * V * 3,
                            K > 0 ? a.st.rec_samples + (int64_t)b * P * K * P * V * 2 : nullptr,
                            K > 0 ? a.st.acc + (int64_t)b * P * K * V : nullptr,
                            a.st.acc_mean + (int64_t)b * P * V,
                            a.st.steps + (int64_t)b * P * V,
                            P, V, K};
    double *totals = a.st.totals + (int64_t)b * P * W;
    double *traj_totals = a.st.traj_totals + (int64_t)b * 5;
    const int64_t ob = (int64_t)b * P * V;

    // 1. the detections into the sort buffer (padding keys sort last), sorted by (id, detection index)
    const int n2 = det_sort_n(m);
    det_load(key, kidx, det, m, n2, tid, kScoreThreads);
    __syncthreads();
    det_sort(key, kidx, n2, tid, kScoreThreads);

    // 2. score: wave -> horizon, lane -> pedestrian
    for (int h = 1 + wave; h <= P; h += kScoreWaves) {
        const bool pending = h <= filled;
        const int r = pending ? (head - h + P) % P : 0;             // the row of push m - h
        int np = pending ? rec_peds[r] : 0;
        np = np < 0 ? 0 : (np > V ? V : np);
        const bool retire = pending && h == P;
        double part[kScoreRow], tpart[5];
#pragma unroll
        for (int i = 0; i < kScoreRow; ++i) part[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) tpart[i] = 0.0;
        for (int v0 = 0; v0 < V; v0 += kWave) {
            const int v = v0 + lane;
            if (v >= V) continue;                                   // (the wave sums below are outside this loop)
            int64_t oid = -1;
            int mt = 0, st = 0;
            float err = 0.f, d2 = 0.f, nll = 0.f, best = 0.f;
            float t_ade = 0.f, t_fde = 0.f, t_adem = 0.f, t_fdem = 0.f;
            if (v < np) {
                const int64_t id = rec_ids[r * V + v];
                const int at = det_find(key, m, id);                // the first detection of the id
                if (at >= 0) {
                    const int j = kidx[at];
                    const float tx = (float)round_pos(det.x(j), a.scale);
                    const float ty = (float)round_pos(det.y(j), a.scale);
                    mt = 1;
                    oid = id;
                    score_entry(tab, r, h, v, tx, ty, err, d2, nll, best);
                }
                if (retire) {                                       // from the accumulators just advanced
                    t_fde = best;
                    t_fdem = err;
                    st = score_retire(tab, r, v, t_fde, t_fdem, t_ade, t_adem, tpart);
                }
            }
            const int64_t o = ob + (int64_t)(h - 1) * V + v;
            a.out.rec_ids[o] = oid;
            a.out.matched[o] = mt;
            a.out.err[o] = err;
            a.out.d2[o] = d2;
            a.out.nll[o] = nll;
            if (a.out.best) a.out.best[o] = best;
            if (h == P) {
                const int64_t x = (int64_t)b * V + v;
                a.out.traj_steps[x] = st;
                if (a.out.traj_ade) a.out.traj_ade[x] = t_ade;
                if (a.out.traj_fde) a.out.traj_fde[x] = t_fde;
                a.out.traj_ade_mean[x] = t_adem;
                a.out.traj_fde_mean[x] = t_fdem;
            }
            if (mt) score_cols<true>(part, err, d2, nll, best, a.thr, Q);
        }
        // 3. the horizon's sums: the whole wave is here (h, pending and retire are uniform over it)
        if (pending) {
#pragma unroll
            for (int i = 0; i < kScoreRow; ++i) {
                if (i < W) {                                        // (W is uniform)
                    const double s = wave_sum(part[i]);
                    if (lane == 0) totals[(h - 1) * W + i] += s;
                }
            }
        }
        if (retire) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double s = wave_sum(tpart[i]);
                if (lane == 0) traj_totals[i] += s;
            }
        }
    }
    __syncthreads();

    // 4. enqueue: this push's record into the retired row, its accumulators zeroed.  Every column v < V: those at or
    //    past num_peds carry id -1 and a zero covariance
    int npn = a.pred.num_peds[b];
    npn = npn < 0 ? 0 : (npn > V ? V : npn);
    for (int v = tid; v < V; v += kScoreThreads) {
        rec_ids[head * V + v] = v < npn ? a.pred.ids[(int64_t)b * V + v] : -1;
        tab.acc_mean[head * V + v] = 0.f;
        tab.steps[head * V + v] = 0;
        score_cov_column(a.pred, b, tab, head, v, v < npn);
    }
    score_copy_mean(a.pred, b, tab, head, npn, [](int64_t) {});
    if (K > 0) {
        score_copy_samples(a.pred, a.NS, b, tab, head, npn);
        for (int e = tid; e < K * V; e += kScoreThreads) tab.acc[(int64_t)head * K * V + e] = 0.f;
    }
    if (tid == 0) {                                          // (every read of the head and of rec_peds is behind the barrier)
        rec_peds[head] = npn;
        hd[0] = (head + 1) % P;
        hd[1] = filled < P ? filled + 1 : P;
    }
}

__global__ __launch_bounds__(kScoreThreads) void score_push_kernel(
    const ScoreArgs a, const int64_t *__restrict__ det_id, const double *__restrict__ det_xy,
    const int32_t *__restrict__ det_count) {
    score_push_body(a, 0, {det_id, 1, det_xy, 2}, det_count[0]);
}

// One workgroup per stream: stream b scores against its range of the tick when pushed[b] != 0, as
// stg_track_push_streams reads them.
__global__ __launch_bounds__(kScoreThreads) void score_push_streams_kernel(const ScoreArgs a, Detections det, Tick tick) {
    const int b = blockIdx.x;
    if (tick.pushed_at(b) == 0) {                           // uniform over the block
        score_empty(a, b);
        return;
    }
    int lo;
    const int count = tick.range(b, lo);
    score_push_body(a, b, det.from(lo), count);
}

// the checks both entry points share, on `a` as the entry point filled it from its arguments; completes it (st, out, M2)
static int score_args(const char *what, const stg_score_state *st, const stg_score_out *out, ScoreArgs *a) {
    const int M_max = a->M_max, P = a->P, V = a->V, Q = a->Q;
    STG_REQUIRE(M_max >= 1 && P >= 1 && V >= 1 && a->K >= 0 && Q >= 0, STG_EINVAL,
                "%s: bad sizes M_max=%d P=%d V=%d K=%d Q=%d", what, M_max, P, V, a->K, Q);
    STG_REQUIRE(st && out, STG_EINVAL, "%s: null pointer (state / out)", what);
    STG_REQUIRE(st->rec_ids && st->rec_peds && st->rec_mean && st->rec_cov && st->acc_mean && st->steps && st->head &&
                    st->totals && st->traj_totals,
                STG_EINVAL, "%s: null pointer in the state", what);
    STG_REQUIRE(out->rec_ids && out->matched && out->err && out->d2 && out->nll && out->traj_steps &&
                    out->traj_ade_mean && out->traj_fde_mean,
                STG_EINVAL, "%s: null pointer among the outputs", what);
    const int rc = score_pred_args(what, &a->pred, a->thr, st->rec_mean, st->rec_samples, st->rec_samples && st->acc,
                                   "rec_samples / acc", a->NS, P, V, &a->K, Q);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(a->K == 0 || (out->best && out->traj_ade && out->traj_fde), STG_EINVAL,
                "%s: null pointer among the outputs (best / traj_ade / traj_fde with K=%d)", what, a->K);
    STG_REQUIRE(M_max <= STG_TRACK_MAX_DETECTIONS, STG_EUNSUPPORTED, "%s: M_max=%d above STG_TRACK_MAX_DETECTIONS=%d",
                what, M_max, STG_TRACK_MAX_DETECTIONS);
    a->st = *st;
    a->out = *out;
    a->M2 = det_sort_n(M_max);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_score_push(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, double scale,
                   const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                   const float *samples, const int64_t *ids, const int32_t *num_peds, int P, int V, int K,
                   const stg_score_state *state, const float *thr, int Q, const stg_score_out *out, void *stream) {
    stg::ScoreArgs a{};
    a.pred = {mean, v_pred, p_sn, p_sf, p_sp, p_sv, samples, ids, num_peds};
    a.thr = thr, a.scale = scale;
    a.NS = 1, a.P = P, a.V = V, a.K = K, a.Q = Q, a.M_max = M_max;
    const int rc = stg::score_args("stg_score_push", state, out, &a);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_id && det_xy && det_count, STG_EINVAL, "stg_score_push: null pointer (detections)");
    return stg::launch({"stg_score_push", dim3(1), dim3(stg::kScoreThreads), stg::det_sort_lds(a.M2),
                        stg::as_stream(stream), 64 * 1024},
                       stg::score_push_kernel, a, det_id, det_xy, det_count);
}

int stg_score_push_streams(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                           int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                           double scale, const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf,
                           int64_t p_sp, int64_t p_sv, const float *samples, const int64_t *ids,
                           const int32_t *num_peds, int P, int V, int K, const stg_score_state *state,
                           const float *thr, int Q, const stg_score_out *out, void *stream) {
    int rc = stg::stream_args("stg_score_push_streams", NS, M_total, id_stride, xy_stride, 0, false);    // (see there)
    if (rc != STG_OK || NS == 0) return rc;
    stg::ScoreArgs a{};
    a.pred = {mean, v_pred, p_sn, p_sf, p_sp, p_sv, samples, ids, num_peds};
    a.thr = thr, a.scale = scale;
    a.NS = NS, a.P = P, a.V = V, a.K = K, a.Q = Q, a.M_max = M_max;
    rc = stg::score_args("stg_score_push_streams", state, out, &a);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_id && det_xy && det_start && pushed, STG_EINVAL,
                "stg_score_push_streams: null pointer (detections)");
    STG_REQUIRE(M_total <= STG_TRACK_MAX_TOTAL_DETECTIONS, STG_EUNSUPPORTED,
                "stg_score_push_streams: M_total=%d above STG_TRACK_MAX_TOTAL_DETECTIONS=%d", M_total,
                STG_TRACK_MAX_TOTAL_DETECTIONS);
    return stg::launch({"stg_score_push_streams", dim3((unsigned)NS), dim3(stg::kScoreThreads), stg::det_sort_lds(a.M2),
                        stg::as_stream(stream), 64 * 1024},
                       stg::score_push_streams_kernel, a, stg::Detections{det_id, id_stride, det_xy, xy_stride},
                       stg::Tick{det_start, pushed, M_total});
}

}  // extern "C"
