// score_time: timed live predictions scored against the tracks that follow, indexed by TIME.  The
// push-indexed score (score.hip, 5.17) grades the prediction of h pushes ago at its step h; behind a timed push
// (frames_time.hip, 5.20) a prediction made at time t_r is graded at the instants t_r + h * step, which usually fall
// between two pushes, so the truth is interpolated the way the timed push interpolates its window.
//
// The rule, per stream, behind the timed push of the same tick at t_now = clock[0].
//   nothing    a stream not pushed, or whose push was refused (STG_TRACK_TIME_ORDER in head_flags[1], read here on the
//              device), keeps its state bit for bit; its per-push outputs are zero and it leaves no record.
//   records    accepted push number n (0, 1, ... since the state was cleared; a push with no detections counts) leaves
//              a record in row n mod Rp: its time t_r = t_now, the scene's ids (V) and num_peds, mean (P,V,2), the
//              cumulative covariance (P,V,3) of 5.17 and the K samples.  A row is empty (0), pending (1) or retired (2);
//              a pending occupant that is overwritten advances the stream's eviction counter.
//   truth      from the track rings the timed push keeps.  Only a track whose newest sample (tb, pb) has tb == t_now
//              takes part; (ta, pa) is the sample before it in its ring, if any.  For a pending record that holds the
//              track's id at column v and h = 1..P ascending, tau = t_r + h * step:
//                tau == tb                          the truth is pb, no arithmetic is done
//                ta < tau < tb, tb - ta <= max_dt   per coordinate round(pa + (pb - pa) * ((double)(tau - ta) /
//                                                   (double)(tb - ta))) in float64, one IEEE operation at a time
//                                                   (lerp_bracket of time_samples.hpp, the push's own)
//                ta < tau < tb, a wider bracket     that (record, h, v) stays unmatched for good
//                anything else                      not this push
//              and the truth is converted to float32.  The brackets of a track are disjoint, so every (record, h, v)
//              is scored at most once.
//   values     err, det, d2, nll, best, acc[k], acc_mean, steps exactly as 5.17 (score_fn.hpp), written into the
//              record's own tables matched, err, d2, nll, best (Rp,P,V).
//   retire     after scoring, a pending record with t_now >= t_r + P * step is retired: traj_steps, traj_ade, traj_fde,
//              traj_ade_mean, traj_fde_mean (V) into its row; a pedestrian with steps == P enters traj_totals.
//   totals     float64 totals (P,5+Q) and traj_totals (5) with the columns of 5.17; push_totals / push_traj are what
//              this push added.
//   order      score; retire; only then, behind a barrier, write this push's record.
//
// One workgroup of 256 threads per stream:
//   lookup   the slots whose newest sample is at t_now, sorted by id in LDS (det_sort; a padding key elsewhere)
//   headers  a wave owns the rows w, w+4, ...; a lane per row decides whether the record has an instant in this push's
//            brackets or is due to retire, and the wave visits only those rows
//   score    a wave per record, a lane per pedestrian (v, v+64, ...): the id's slot,
//            its one or two newest samples, the h range of the bracket in integers, then ascending h with the loop
//            over k inside.  A row belongs to one wave: its accumulators are plain read-modify-writes
//   totals   per (record, 64 pedestrians, h) the wave adds its lanes by a fixed butterfly and lane 0 adds the sum to
//            the wave's own partials in LDS; behind a barrier one thread per entry adds the four partials in wave
//            order.  No atomics, the same order every run
//   retire   by the wave that owns the row
//   enqueue  behind the barrier: the columns v < num_peds only, the tables zeroed for those columns only
// No host synchronisation, plain C++ stores only, no scratch.
//
// The arithmetic of `values`, the trajectory values and totals columns, the covariance sum and the column copies of the
// enqueue and the host's checks of the prediction are score_fn.hpp's, shared with score.hip.  The track
// state is live_args.hpp's TimedView; the refused push, a slot's head and count, its two newest samples and the
// interpolation are time_samples.hpp's, shared with the push and the harvest.  This file keeps what is
// its own: which instants fall into a track's newest bracket, a wave per record row behind the header pass, the record's
// own tables.
#include "detections.hpp"
#include "score_fn.hpp"
#include "time_samples.hpp"

namespace stg {

enum { kRecEmpty = 0, kRecPending = 1, kRecRetired = 2 };

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return a - q * b < 0 ? q - 1 : q;
}

// The sizes of a timed score: S track slots with R samples each (S2 = det_sort_n(S), filled in on the host), Rp record
// rows of P horizons, V pedestrians, K samples; Q thresholds
struct TimedScoreDims { int NS, P, V, K, Q, Rp, S, R, S2; int64_t step, max_dt; double scale; };

// stg_score_timed_state with its slicing rule
struct TimedScoreState : stg_score_timed_state {
    __device__ __forceinline__ TimedScoreState of_stream(int64_t b, const TimedScoreDims &d) const {
        const int64_t rp = d.Rp, rv = rp * d.V, rpv = rv * d.P;
        TimedScoreState s = *this;
        s.rec_t += b * rp, s.rec_status += b * rp, s.rec_peds += b * rp, s.rec_ids += b * rv;
        s.rec_mean += b * rpv * 2, s.rec_cov += b * rpv * 3, s.acc_mean += b * rv, s.steps += b * rv;
        if (d.K > 0) s.rec_samples += b * rpv * d.K * 2, s.acc += b * rv * d.K, s.best += b * rpv;
        s.matched += b * rpv, s.err += b * rpv, s.d2 += b * rpv, s.nll += b * rpv;
        s.traj_steps += b * rv, s.traj_ade_mean += b * rv, s.traj_fde_mean += b * rv;
        if (d.K > 0) s.traj_ade += b * rv, s.traj_fde += b * rv;
        s.counters += b * 2, s.totals += b * d.P * (kScoreCols + d.Q), s.traj_totals += b * 5;
        return s;
    }
    __device__ __forceinline__ ScoreRows tables(const TimedScoreDims &d) const {
        return {rec_mean, rec_cov, rec_samples, acc, acc_mean, steps, d.P, d.V, d.K};
    }
};

struct TimedScoreArgs {
    ScorePred pred;
    TimedView trk;                                          // the timed track state (live_args.hpp): read only
    TimedScoreState st;
    const float *thr;
    stg_score_timed_out out;
    TimedScoreDims d;
};

// One timed push of stream b scored by one workgroup of kScoreThreads threads; trk and st are the stream's own.
// LDS (dynamic): sort keys (S2 x int64), sort indices (S2 x int32)
__device__ __forceinline__ void score_timed_body(const TimedScoreArgs &a, int b, const TimedView &trk,
                                                 const TimedScoreState &st, bool pushed) {
    extern __shared__ __align__(16) unsigned char lds[];
    int64_t *key = reinterpret_cast<int64_t *>(lds);
    int32_t *kidx = reinterpret_cast<int32_t *>(key + a.d.S2);
    __shared__ double part[kScoreWaves][STG_SCORE_MAX_P * kScoreRow];
    __shared__ double tpart[kScoreWaves][5];
    __shared__ int top;                                     // one past the highest slot that takes part
    __shared__ unsigned long long ta_low;                   // the oldest `ta` among them, biased to unsigned order

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int P = a.d.P, V = a.d.V, K = a.d.K, Q = a.d.Q, W = kScoreCols + Q, Rp = a.d.Rp, S = a.d.S, R = a.d.R;
    const int64_t step = a.d.step, max_dt = a.d.max_dt;
    const ScoreRows tab = st.tables(a.d);
    double *push_totals = a.out.push_totals + (int64_t)b * P * W, *push_traj = a.out.push_traj + (int64_t)b * 5;

    // 0. a stream not pushed, or a push the track kernel refused: nothing moves (uniform over the block)
    if (!pushed || push_refused(trk.head_flags)) {
        for (int e = tid; e < P * W; e += kScoreThreads) push_totals[e] = 0.0;
        if (tid < 5) push_traj[tid] = 0.0;
        return;
    }
    const int64_t t_now = trk.clock[0];
    const int64_t n_acc = st.counters[0];                   // (read by every thread ahead of the barriers; written last)
    const int head = (int)((uint64_t)n_acc % (uint64_t)Rp);

    // 1. the id -> slot lookup: the slots whose newest sample is this push's, sorted by id (padding keys sort last).
    //    Slots are handed out lowest first, so the sort covers the slots up to the highest one that takes part, not all
    //    S; and the oldest `ta` among them bounds every bracket of this push from below (LDS atomics on integer words).
    constexpr unsigned long long kBias = 1ull << 63;        // int64 order as unsigned order
    if (tid == 0) {
        top = 0;
        ta_low = (unsigned long long)(t_now - 1) ^ kBias;
    }
    __syncthreads();
    for (int p = tid; p < a.d.S2; p += kScoreThreads) {
        int64_t k = INT64_MAX;
        if (p < S) {
            int h;
            const int c = slot_samples(trk.slot_head, p, R, &h), ib = ring_before(h, R);
            if (c > 0 && trk.t_ring[(int64_t)p * R + ib] == t_now) {
                k = trk.slot_id[p];
                atomicMax(&top, p + 1);
                if (c >= 2)
                    atomicMin(&ta_low, (unsigned long long)trk.t_ring[(int64_t)p * R + ring_before(ib, R)] ^ kBias);
            }
        }
        key[p] = k;
        kidx[p] = p;
    }
    for (int e = tid; e < kScoreWaves * STG_SCORE_MAX_P * kScoreRow; e += kScoreThreads) (&part[0][0])[e] = 0.0;
    if (tid < kScoreWaves * 5) (&tpart[0][0])[tid] = 0.0;
    __syncthreads();
    const int n2 = det_sort_n(top < 1 ? 1 : top);           // (<= S2; the keys from `top` on are padding)
    const int64_t ta_min = (int64_t)(ta_low ^ kBias);
    det_sort(key, kidx, n2, tid, kScoreThreads);

    // 2. score and retire: wave -> record, lane -> pedestrian
    //    The headers first, a lane per row of the wave (64 rows at a time): no bracket of this push reaches below
    //    ta_min, so a pending record with no instant in (ta_min, t_now] has no work -- at a steady feed all but the ~P
    //    records whose time is congruent to t_now mod step -- and the wave visits only the rows with work or to retire
    for (int base = 0; base < Rp; base += kWave * kScoreWaves) {
      const int mine = base + lane * kScoreWaves + wave;
      bool visit = false;
      if (mine < Rp && st.rec_status[mine] == kRecPending) {
          const int64_t t_m = st.rec_t[mine];
          const int64_t m_lo = floor_div(ta_min - t_m, step) + 1, m_hi = floor_div(t_now - t_m, step);
          visit = (m_lo < 1 ? 1 : m_lo) <= (m_hi > P ? P : m_hi) || t_now - t_m >= (int64_t)P * step;
      }
      for (unsigned long long rows = __ballot(visit); rows != 0; rows &= rows - 1) {     // uniform over the wave
        const int r = base + (__ffsll(rows) - 1) * kScoreWaves + wave;
        const int64_t t_r = st.rec_t[r];
        int np = st.rec_peds[r];
        np = np < 0 ? 0 : (np > V ? V : np);
        const bool retire = t_now - t_r >= (int64_t)P * step;
        const int64_t r_lo = floor_div(ta_min - t_r, step) + 1, r_hi = floor_div(t_now - t_r, step);
        const bool work = (r_lo < 1 ? 1 : r_lo) <= (r_hi > P ? P : r_hi);
        double tp[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) tp[i] = 0.0;
        for (int v0 = 0; v0 < np; v0 += kWave) {
            const int v = v0 + lane;
            // the bracket (ta, tb] of the pedestrian's track and the horizons whose instant lies in it
            int h_lo = 1, h_hi = 0;
            bool wide = true;
            int64_t ta = 0;
            double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
            if (work && v < np) {
                const int64_t id = st.rec_ids[(int64_t)r * V + v];
                const int at = id == INT64_MAX ? -1 : det_find(key, n2, id);
                if (at >= 0) {
                    const int s = kidx[at];
                    int hd;
                    const int c = slot_samples(trk.slot_head, s, R, &hd), ib = ring_before(hd, R);
                    const int64_t sb = (int64_t)s * R + ib;
                    bx = trk.xy_ring[sb * 2];
                    by = trk.xy_ring[sb * 2 + 1];
                    ta = t_now - 1;                         // no older sample: the bracket holds t_now alone
                    if (c >= 2) {
                        const int64_t sa = (int64_t)s * R + ring_before(ib, R);
                        ta = trk.t_ring[sa];
                        ax = trk.xy_ring[sa * 2];
                        ay = trk.xy_ring[sa * 2 + 1];
                        wide = t_now - ta > max_dt;
                    }
                    const int64_t lo = floor_div(ta - t_r, step) + 1, hi = floor_div(t_now - t_r, step);
                    h_lo = lo < 1 ? 1 : (lo > P ? P + 1 : (int)lo);
                    h_hi = hi > P ? P : (hi < 0 ? 0 : (int)hi);
                }
            }
            for (int h = 1; h <= P; ++h) {
                const int64_t tau = t_r + (int64_t)h * step;
                const bool hit = h >= h_lo && h <= h_hi && (tau == t_now || !wide);
                if (__ballot(hit) == 0) continue;           // uniform over the wave
                double pt[kScoreRow];
#pragma unroll
                for (int i = 0; i < kScoreRow; ++i) pt[i] = 0.0;
                if (hit) {
                    double x = bx, y = by;
                    if (tau != t_now) lerp_bracket(ta, ax, ay, t_now, bx, by, tau, a.d.scale, x, y);
                    const int64_t e = ((int64_t)r * P + (h - 1)) * V + v;
                    float err, d2, nll, best;
                    score_entry(tab, r, h, v, (float)x, (float)y, err, d2, nll, best);
                    if (K > 0) st.best[e] = best;
                    st.matched[e] = 1;
                    st.err[e] = err;
                    st.d2[e] = d2;
                    st.nll[e] = nll;
                    score_cols<false>(pt, err, d2, nll, best, a.thr, Q);
                }
#pragma unroll
                for (int i = 0; i < kScoreRow; ++i) {
                    if (i < W) {                            // (W is uniform)
                        const double s = wave_sum(pt[i]);
                        if (lane == 0) part[wave][(h - 1) * W + i] += s;
                    }
                }
            }
            // 3. retire: the trajectory values from the accumulators this lane has just advanced
            if (retire && v < np) {
                const int64_t x = (int64_t)r * V + v, eP = ((int64_t)r * P + (P - 1)) * V + v;
                const float t_fde = K > 0 ? st.best[eP] : 0.f, t_fdem = st.err[eP];     // h = P: from the record's tables
                float t_ade, t_adem;
                st.traj_steps[x] = score_retire(tab, r, v, t_fde, t_fdem, t_ade, t_adem, tp);
                if (K > 0) {
                    st.traj_ade[x] = t_ade;
                    st.traj_fde[x] = t_fde;
                }
                st.traj_ade_mean[x] = t_adem;
                st.traj_fde_mean[x] = t_fdem;
            }
        }
        if (retire) {                                       // the whole wave is here
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double s = wave_sum(tp[i]);
                if (lane == 0) tpart[wave][i] += s;
            }
            if (lane == 0) st.rec_status[r] = kRecRetired;
        }
      }
    }
    __syncthreads();

    // 4. the totals: the four waves' partials in wave order
    for (int e = tid; e < P * W; e += kScoreThreads) {
        const double s = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
        st.totals[e] += s;
        push_totals[e] = s;
    }
    if (tid < 5) {
        const double s = ((tpart[0][tid] + tpart[1][tid]) + tpart[2][tid]) + tpart[3][tid];
        st.traj_totals[tid] += s;
        push_traj[tid] = s;
    }

    // 5. enqueue: this push's record into row `head`, the columns of its pedestrians only
    const ScorePred &pr = a.pred;
    int npn = pr.num_peds[b];
    npn = npn < 0 ? 0 : (npn > V ? V : npn);
    for (int v = tid; v < V; v += kScoreThreads) {
        const int64_t x = (int64_t)head * V + v;
        st.rec_ids[x] = v < npn ? pr.ids[(int64_t)b * V + v] : -1;
        if (v >= npn) continue;
        st.acc_mean[x] = 0.f;
        st.steps[x] = 0;
        st.traj_steps[x] = 0;
        st.traj_ade_mean[x] = 0.f;
        st.traj_fde_mean[x] = 0.f;
        if (K > 0) {
            st.traj_ade[x] = 0.f;
            st.traj_fde[x] = 0.f;
            for (int k = 0; k < K; ++k) st.acc[((int64_t)head * K + k) * V + v] = 0.f;
        }
        score_cov_column(pr, b, tab, head, v, true);
    }
    score_copy_mean(pr, b, tab, head, npn, [&](int64_t y) {     // and the record's own tables, the same entries
        st.matched[y] = 0;
        st.err[y] = 0.f;
        st.d2[y] = 0.f;
        st.nll[y] = 0.f;
        if (K > 0) st.best[y] = 0.f;
    });
    if (K > 0) score_copy_samples(pr, a.d.NS, b, tab, head, npn);
    if (tid == 0) {                                         // (behind the barrier: retirement has been written)
        const bool evicts = st.rec_status[head] == kRecPending;
        st.rec_t[head] = t_now;
        st.rec_peds[head] = npn;
        st.rec_status[head] = kRecPending;
        st.counters[0] = n_acc + 1;
        if (evicts) st.counters[1] += 1;
    }
}

__global__ __launch_bounds__(kScoreThreads) void score_push_timed_kernel(const TimedScoreArgs a) {
    score_timed_body(a, 0, a.trk, a.st, true);
}

// One workgroup per stream: stream b scores when pushed[b] != 0, as stg_track_push_streams_timed reads it
__global__ __launch_bounds__(kScoreThreads) void score_push_streams_timed_kernel(const TimedScoreArgs a,
                                                                                  const int32_t *__restrict__ pushed) {
    const int b = blockIdx.x;
    score_timed_body(a, b, a.trk.of_stream(b, a.d.S, a.d.R), a.st.of_stream(b, a.d), pushed[b] != 0);
}

// the checks both entry points share, on `a` as the entry point filled it from its arguments; completes it (st, out, S2)
static int score_timed_args(const char *what, const stg_score_timed_state *st, const stg_score_timed_out *out,
                            TimedScoreArgs *a) {
    TimedScoreDims &d = a->d;
    const TimedView &t = a->trk;
    STG_REQUIRE(d.S >= 1 && d.R >= 2 && d.P >= 1 && d.V >= 1 && d.K >= 0 && d.Q >= 0 && d.Rp >= 1, STG_EINVAL,
                "%s: bad sizes S=%d R=%d P=%d V=%d K=%d Q=%d Rp=%d", what, d.S, d.R, d.P, d.V, d.K, d.Q, d.Rp);
    int rc = timed_size_args(what, d.R, d.step, d.P, "P");
    if (rc != STG_OK) return rc;
    STG_REQUIRE(d.max_dt >= 1 && d.max_dt < ((int64_t)1 << 31), STG_EINVAL, "%s: max_dt=%lld not in [1, 2^31)", what,
                (long long)d.max_dt);
    STG_REQUIRE(st && out, STG_EINVAL, "%s: null pointer (state / out)", what);
    STG_REQUIRE(t.slot_id && t.t_ring && t.xy_ring && t.slot_head && t.clock && t.head_flags, STG_EINVAL,
                "%s: null pointer in the track state", what);
    STG_REQUIRE(st->rec_t && st->rec_status && st->rec_peds && st->rec_ids && st->rec_mean && st->rec_cov &&
                    st->acc_mean && st->steps && st->matched && st->err && st->d2 && st->nll && st->traj_steps &&
                    st->traj_ade_mean && st->traj_fde_mean && st->counters && st->totals && st->traj_totals,
                STG_EINVAL, "%s: null pointer in the state", what);
    STG_REQUIRE(out->push_totals && out->push_traj, STG_EINVAL, "%s: null pointer among the outputs", what);
    rc = score_pred_args(what, &a->pred, a->thr, st->rec_mean, st->rec_samples,
                                   st->rec_samples && st->acc && st->best && st->traj_ade && st->traj_fde,
                                   "rec_samples / acc / best / traj_ade / traj_fde", d.NS, d.P, d.V, &d.K, d.Q);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(d.S <= STG_TRACK_MAX_SLOTS, STG_EUNSUPPORTED, "%s: S=%d above STG_TRACK_MAX_SLOTS=%d", what, d.S,
                STG_TRACK_MAX_SLOTS);
    STG_REQUIRE(d.Rp <= STG_SCORE_MAX_PENDING, STG_EUNSUPPORTED, "%s: Rp=%d above STG_SCORE_MAX_PENDING=%d", what, d.Rp,
                STG_SCORE_MAX_PENDING);
    static_cast<stg_score_timed_state &>(a->st) = *st;
    a->out = *out;
    d.S2 = det_sort_n(d.S);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_score_push_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring, const int32_t *slot_head,
                         const int64_t *clock, const int32_t *head_flags, int S, int R, double scale, int64_t step,
                         int64_t max_dt, const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf,
                         int64_t p_sp, int64_t p_sv, const float *samples, const int64_t *ids, const int32_t *num_peds,
                         int P, int V, int K, int Rp, const stg_score_timed_state *state, const float *thr, int Q,
                         const stg_score_timed_out *out, void *stream) {
    const char *what = "stg_score_push_timed";
    stg::TimedScoreArgs a{};
    a.pred = {mean, v_pred, p_sn, p_sf, p_sp, p_sv, samples, ids, num_peds};
    a.trk = {slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    a.thr = thr;
    a.d = {1, P, V, K, Q, Rp, S, R, 0, step, max_dt, scale};
    const int rc = stg::score_timed_args(what, state, out, &a);
    if (rc != STG_OK) return rc;
    return stg::launch({what, dim3(1), dim3(stg::kScoreThreads), stg::det_sort_lds(a.d.S2), stg::as_stream(stream),
                        64 * 1024},
                       stg::score_push_timed_kernel, a);
}

int stg_score_push_streams_timed(const int64_t *slot_id, const int64_t *t_ring, const double *xy_ring,
                                 const int32_t *slot_head, const int64_t *clock, const int32_t *head_flags,
                                 const int32_t *pushed, int NS, int S, int R, double scale, int64_t step, int64_t max_dt,
                                 const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp,
                                 int64_t p_sv, const float *samples, const int64_t *ids, const int32_t *num_peds, int P,
                                 int V, int K, int Rp, const stg_score_timed_state *state, const float *thr, int Q,
                                 const stg_score_timed_out *out, void *stream) {
    const char *what = "stg_score_push_streams_timed";
    STG_REQUIRE(NS >= 0, STG_EINVAL, "%s: bad sizes NS=%d", what, NS);
    if (NS == 0) return STG_OK;
    stg::TimedScoreArgs a{};
    a.pred = {mean, v_pred, p_sn, p_sf, p_sp, p_sv, samples, ids, num_peds};
    a.trk = {slot_id, t_ring, xy_ring, slot_head, clock, head_flags};
    a.thr = thr;
    a.d = {NS, P, V, K, Q, Rp, S, R, 0, step, max_dt, scale};
    const int rc = stg::score_timed_args(what, state, out, &a);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(pushed, STG_EINVAL, "%s: null pointer (pushed)", what);
    return stg::launch({what, dim3((unsigned)NS), dim3(stg::kScoreThreads), stg::det_sort_lds(a.d.S2),
                        stg::as_stream(stream), 64 * 1024},
                       stg::score_push_streams_timed_kernel, a, pushed);
}

}  // extern "C"
