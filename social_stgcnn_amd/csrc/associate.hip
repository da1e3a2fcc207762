// associate: unlabelled detections -> track ids on the device, the front end of the live pushes.
//
//   stg_associate          ONE workgroup on a single stream's arrays
//   stg_associate_streams  one workgroup per stream on its slices of the (NS, ...) state and its range of one packed
//                          tick; a stream not pushed returns before the first barrier, its state untouched
//
// The rule: a per-stream tracker with constant-velocity prediction and gated, globally greedy nearest-neighbour
// matching -- the candidates (cost <= the track's squared gate) taken in ascending (cost, track slot, detection) order,
// each accepted when its track and its detection are both still free.  The kernel reaches that matching in rounds:
// every free track remembers its best free detection, min (cost, j), every free detection its best free track,
// min (cost, s); a pair that is each other's best is accepted.  The smallest remaining candidate is always such a
// pair, so every round with a candidate left accepts at least one, and after min(live tracks, m) rounds nothing is
// left: that is the loop's bound.  A row or column is rescanned only when its remembered partner was taken, by a group
// of 8 lanes that split its partners and reduce (cost, index) by shuffles.
//
// Everything is read from device memory when the kernel runs (count, ranges, state), the ids are written into the
// caller's det_id array, which the push and score launches behind it read.  Plain C++ stores, LDS atomics on integer
// words only, no scratch, no host synchronisation.
#include "associate.hpp"
#include "track_rule.hpp"

namespace stg {

struct AssocState {
    int64_t *trk_id;         // (C)    -1 = free
    double *trk_pos;         // (C,2)  the last matched rounded position
    double *trk_vel;         // (C,2)  displacement per push
    int32_t *trk_miss;       // (C)    pushes since the last match
    int32_t *trk_hits;       // (C)    matches so far
    int64_t *next_id;        // (1)
    int32_t *assoc_flags;    // (1)    STG_ASSOC_* of the last push
};

struct AssocRule {
    double scale, gate2, gate_new2;
    int max_miss;
};

// One push of one stream by one workgroup of kThreads threads: the positions of the detections j < min(count, M_max)
// are read, their ids written.
template <int kThreads>
__device__ __forceinline__ void associate_body(const DetectionsOut &det, int count, int M_max, const AssocState st, int C,
                                               const AssocRule rule) {
    extern __shared__ __align__(16) unsigned char lds[];
    double *tq = reinterpret_cast<double *>(lds);               // (C,2) predicted positions
    double *dp = tq + 2 * (size_t)C;                             // (M_max,2) rounded detections
    int32_t *tgate = reinterpret_cast<int32_t *>(dp + 2 * (size_t)M_max);     // (C) -1 free slot, 0 gate_new2, 1 gate2
    int32_t *tstate = tgate + C;                                 // (C) kUnknown, kNone, best detection >= 0, or taken
    int32_t *list = tstate + C;                                  // (C) live slots in slot order; later the free slots
    int32_t *dstate = list + C;                                  // (M_max) the same for a detection: best track slot
    __shared__ int wave_cnt[kThreads / kWave];
    __shared__ int flags, accepted;

    const int tid = threadIdx.x;
    const int m = count < 0 ? 0 : (count > M_max ? M_max : count);
    const int64_t next0 = st.next_id[0];
    if (tid == 0) {
        flags = 0;
        accepted = 0;
    }

    // 1. predictions and gates of the slots (every load unconditional and no barrier in the loop: the loads of
    //    successive passes are in flight together), the rounded detections; then the live list from LDS
#pragma unroll 4
    for (int s = tid; s < C; s += kThreads) {
        const int64_t id = st.trk_id[s];
        const int hits = st.trk_hits[s];
        const double k = (double)(st.trk_miss[s] + 1);
        tq[2 * s] = assoc_predict(st.trk_pos[2 * s], st.trk_vel[2 * s], k);
        tq[2 * s + 1] = assoc_predict(st.trk_pos[2 * s + 1], st.trk_vel[2 * s + 1], k);
        tgate[s] = id < 0 ? -1 : (hits >= 2 ? 1 : 0);
        tstate[s] = kUnknown;
    }
    for (int j = tid; j < m; j += kThreads) {
        dp[2 * j] = round_pos(det.x(j), rule.scale);
        dp[2 * j + 1] = round_pos(det.y(j), rule.scale);
        dstate[j] = kUnknown;
    }
    __syncthreads();
    int n_live = 0, tot = 0;
    for (int s0 = 0; s0 < C; s0 += kThreads) {
        const int s = s0 + tid;
        const bool live = s < C && tgate[s] >= 0;
        const int r = block_rank<kThreads>(live, n_live, &tot, wave_cnt);
        if (live) list[r] = s;
        n_live += tot;
    }
    __syncthreads();

    // 2. the rounds.  `accepted` only grows; a round that leaves it as it was ends the matching
    const int bound = n_live < m ? n_live : m;
    const int sub = tid & (kAssocGroup - 1), grp = tid / kAssocGroup;
    int done = 0;
    for (int round = 0; round < bound; ++round) {
        // a row (a column) is walked by a group of kAssocGroup lanes, partner sub, sub + kAssocGroup, ...; every lane
        // of the block runs the same passes, so the shuffles of assoc_group_min meet converged
        for (int i0 = 0; i0 < n_live; i0 += kThreads / kAssocGroup) {
            const int i = i0 + grp;
            int s = 0;
            bool scan = false;
            if (i < n_live) {
                s = list[i];
                const int was = tstate[s];
                // not: taken / nothing in reach / the remembered detection is still free, so still the best
                scan = !(assoc_taken(was) || was == kNone || (was >= 0 && !assoc_taken(dstate[was])));
            }
            double best = 0.0;
            int at = kNone;
            if (scan) {
                const double qx = tq[2 * s], qy = tq[2 * s + 1], g2 = tgate[s] ? rule.gate2 : rule.gate_new2;
                for (int j = sub; j < m; j += kAssocGroup) {
                    if (assoc_taken(dstate[j])) continue;
                    const double c = assoc_cost(qx, qy, dp[2 * j], dp[2 * j + 1]);
                    if (c <= g2 && (at < 0 || c < best)) {
                        best = c;
                        at = j;
                    }
                }
            }
            assoc_group_min(best, at);
            if (scan && sub == 0) tstate[s] = at;
        }
        for (int j0 = 0; j0 < m; j0 += kThreads / kAssocGroup) {
            const int j = j0 + grp;
            bool scan = false;
            if (j < m) {
                const int was = dstate[j];
                scan = !(assoc_taken(was) || was == kNone || (was >= 0 && !assoc_taken(tstate[was])));
            }
            double best = 0.0;
            int at = kNone;
            if (scan) {
                const double px = dp[2 * j], py = dp[2 * j + 1];
                for (int i = sub; i < n_live; i += kAssocGroup) {         // slot order within a lane
                    const int s = list[i];
                    if (assoc_taken(tstate[s])) continue;
                    const double c = assoc_cost(tq[2 * s], tq[2 * s + 1], px, py);
                    if (c <= (tgate[s] ? rule.gate2 : rule.gate_new2) && (at < 0 || c < best)) {
                        best = c;
                        at = s;
                    }
                }
            }
            assoc_group_min(best, at);
            if (scan && sub == 0) dstate[j] = at;
        }
        __syncthreads();
        // a free track whose best detection names it back.  (A taken detection holds a negative word, a free one the
        // slot of its own best track: neither is s unless the pair is mutual; each word is written by one thread.)
        for (int i = tid; i < n_live; i += kThreads) {
            const int s = list[i];
            const int j = tstate[s];
            if (j >= 0 && dstate[j] == s) {
                tstate[s] = assoc_take(j);
                dstate[j] = assoc_take(s);
                atomicAdd(&accepted, 1);
            }
        }
        __syncthreads();
        const int now = accepted;
        if (now == done) break;
        done = now;
    }

    // 3. the tracks: a matched one moves, one not matched ages and is freed past max_miss.  Again every load is
    //    unconditional and the loop holds no barrier; tgate becomes the mark of a free slot (-1) for the list below
#pragma unroll 4
    for (int s = tid; s < C; s += kThreads) {
        const int64_t id = st.trk_id[s];
        const int miss = st.trk_miss[s], hits = st.trk_hits[s];
        const double ox = st.trk_pos[2 * s], oy = st.trk_pos[2 * s + 1];
        if (tgate[s] < 0) continue;
        const int was = tstate[s];
        if (assoc_taken(was)) {
            const int j = assoc_partner(was);
            const double k = (double)(miss + 1);
            const double px = dp[2 * j], py = dp[2 * j + 1];
            st.trk_vel[2 * s] = assoc_velocity(px, ox, k);
            st.trk_vel[2 * s + 1] = assoc_velocity(py, oy, k);
            st.trk_pos[2 * s] = px;
            st.trk_pos[2 * s + 1] = py;
            st.trk_miss[s] = 0;
            st.trk_hits[s] = hits + 1;
            det.id_at(j) = id;
            tgate[s] = 0;
        } else if (miss + 1 > rule.max_miss) {
            st.trk_id[s] = -1;
            st.trk_pos[2 * s] = st.trk_pos[2 * s + 1] = 0.0;
            st.trk_vel[2 * s] = st.trk_vel[2 * s + 1] = 0.0;
            st.trk_miss[s] = 0;
            st.trk_hits[s] = 0;
            tgate[s] = -1;
        } else {
            st.trk_miss[s] = miss + 1;
            tgate[s] = 0;
        }
    }
    __syncthreads();
    int n_free = 0;                                           // the free slots in slot order, in the place of the live list
    for (int s0 = 0; s0 < C; s0 += kThreads) {
        const int s = s0 + tid;
        const bool fr = s < C && tgate[s] < 0;
        const int r = block_rank<kThreads>(fr, n_free, &tot, wave_cnt);
        if (fr) list[r] = s;
        n_free += tot;
    }
    __syncthreads();

    // 4. the detections not matched, in detection order: fresh ids, and the free slots while they last
    int n_new = 0;
    for (int j0 = 0; j0 < m; j0 += kThreads) {
        const int j = j0 + tid;
        const bool nw = j < m && !assoc_taken(dstate[j]);
        const int r = block_rank<kThreads>(nw, n_new, &tot, wave_cnt);
        if (nw) {
            det.id_at(j) = next0 + r;
            if (r < n_free) {
                const int s = list[r];
                st.trk_id[s] = next0 + r;
                st.trk_pos[2 * s] = dp[2 * j];
                st.trk_pos[2 * s + 1] = dp[2 * j + 1];
                st.trk_vel[2 * s] = st.trk_vel[2 * s + 1] = 0.0;
                st.trk_miss[s] = 0;
                st.trk_hits[s] = 1;
            } else {
                atomicOr(&flags, kFlagAssocFull);
            }
        }
        n_new += tot;
    }
    __syncthreads();
    if (tid == 0) {
        st.next_id[0] = next0 + n_new;
        st.assoc_flags[0] = flags;
    }
}

__global__ __launch_bounds__(kAssocThreads) void associate_kernel(
    int64_t *__restrict__ det_id, const double *__restrict__ det_xy, const int32_t *__restrict__ det_count, int M_max,
    AssocState st, int C, AssocRule rule) {
    associate_body<kAssocThreads>({det_id, 1, det_xy, 2}, det_count[0], M_max, st, C, rule);
}

__global__ __launch_bounds__(kAssocStreamThreads) void associate_streams_kernel(DetectionsOut det, Tick tick, int M_max,
                                                                                AssocState st, int C, AssocRule rule) {
    const int b = blockIdx.x;
    if (tick.pushed_at(b) == 0) return;                     // uniform over the block, ahead of the first barrier
    int lo;
    const int count = tick.range(b, lo);
    const AssocState mine = {st.trk_id + (int64_t)b * C,   st.trk_pos + (int64_t)b * C * 2, st.trk_vel + (int64_t)b * C * 2,
                             st.trk_miss + (int64_t)b * C, st.trk_hits + (int64_t)b * C,    st.next_id + b,
                             st.assoc_flags + b};
    associate_body<kAssocStreamThreads>(det.from(lo), count, M_max, mine, C, rule);
}

// the checks the two entry points share: sizes (above the limits: STG_EUNSUPPORTED), the rule, the pointers
static int assoc_args(const char *what, int M_max, int C, double gate2, double gate_new2, int max_miss,
                      const void *det_id, const void *det_xy, const AssocState &st) {
    STG_REQUIRE(M_max >= 1 && C >= 1, STG_EINVAL, "%s: bad sizes M_max=%d C=%d", what, M_max, C);
    STG_REQUIRE(M_max <= STG_ASSOC_MAX_DETECTIONS && C <= STG_ASSOC_MAX_SLOTS, STG_EUNSUPPORTED,
                "%s: M_max=%d C=%d above the limits (%d, %d)", what, M_max, C, STG_ASSOC_MAX_DETECTIONS,
                STG_ASSOC_MAX_SLOTS);
    STG_REQUIRE(gate2 > 0.0 && gate2 <= 1.7976931348623157e308 && gate_new2 >= gate2 &&
                    gate_new2 <= 1.7976931348623157e308,
                STG_EINVAL, "%s: squared gates %g, %g: finite, gate2 > 0 and gate_new2 >= gate2 expected", what, gate2,
                gate_new2);
    STG_REQUIRE(max_miss >= 0, STG_EINVAL, "%s: max_miss=%d (at least 0)", what, max_miss);
    STG_REQUIRE(det_id && det_xy && st.trk_id && st.trk_pos && st.trk_vel && st.trk_miss && st.trk_hits &&
                    st.next_id && st.assoc_flags,
                STG_EINVAL, "%s: null pointer", what);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int stg_associate(int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, int64_t *trk_id,
                  double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                  int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                  void *stream) {
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_miss, trk_hits, next_id, assoc_flags};
    const int rc = stg::assoc_args("stg_associate", M_max, C, gate2, gate_new2, max_miss, det_id, det_xy, st);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_count, STG_EINVAL, "stg_associate: null pointer");
    return stg::launch({"stg_associate", dim3(1), dim3(stg::kAssocThreads), stg::assoc_lds(C, M_max),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_kernel, det_id, det_xy, det_count, M_max, st, C,
                       stg::AssocRule{scale, gate2, gate_new2, max_miss});
}

int stg_associate_streams(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride, int M_total,
                          const int32_t *det_start, const int32_t *pushed, int NS, int M_max, int64_t *trk_id,
                          double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                          int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                          void *stream) {
    int rc = stg::stream_args("stg_associate_streams", NS, M_total, id_stride, xy_stride);
    if (rc != STG_OK) return rc;
    const stg::AssocState st = {trk_id, trk_pos, trk_vel, trk_miss, trk_hits, next_id, assoc_flags};
    rc = stg::assoc_args("stg_associate_streams", M_max, C, gate2, gate_new2, max_miss, det_id, det_xy, st);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(det_start && pushed, STG_EINVAL, "stg_associate_streams: null pointer");
    return stg::launch({"stg_associate_streams", dim3(NS), dim3(stg::kAssocStreamThreads), stg::assoc_lds(C, M_max),
                        stg::as_stream(stream), 63 * 1024},
                       stg::associate_streams_kernel, stg::DetectionsOut{det_id, id_stride, det_xy, xy_stride},
                       stg::Tick{det_start, pushed, M_total}, M_max, st, C,
                       stg::AssocRule{scale, gate2, gate_new2, max_miss});
}

}  // extern "C"
