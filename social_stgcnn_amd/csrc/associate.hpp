// associate: what the association kernels (associate.hip; associate_time.hip, DESIGN.md 5.28;
// associate_filter.hip) share with each other and with anything that sizes or reads their launch -- the
// workgroup sizes, the flags, the LDS image, the IEEE expressions of the rule, the state record and the body itself, a
// template over a MOTION POLICY: how many model steps lie between a slot's last match and this push, what a match, a
// miss and a birth do to the word that says so (trk_miss of the untimed rule, trk_t of the timed ones), what a match
// does to the slot's position and velocity, and whether the slot's gate is one of the rule's two (chosen by trk_hits)
// or the policy's own, a float64 per slot in LDS (kSlotGate: the filtered rule).  The matching rounds are the same for
// all three.
#pragma once
#include "detections.hpp"
#include "track_rule.hpp"

namespace stg {

constexpr int kAssocThreads = 1024;          // stg_associate: one workgroup
constexpr int kAssocStreamThreads = 256;     // stg_associate_streams: one workgroup per stream
constexpr int kFlagAssocFull = STG_ASSOC_FULL;

// LDS image (dynamic): per track slot its predicted position q (2 x float64), its gate (int32: which of the two, -1
// for a free slot), its state word and one entry of the live list / free list (int32 each): 28 bytes; per detection its
// rounded position p (2 x float64) and its state word: 20 bytes.  At both limits (2048, 2048) that is 98,304 bytes of
// the 163,840 a CU holds; at the predictors' defaults (1024, 1024) 49,152, so three workgroups share a CU.  A policy
// with kSlotGate adds its squared gate per slot (float64): 36 bytes per slot, 114,688 bytes at both limits.
constexpr size_t kAssocTrackBytes = 2 * sizeof(double) + 3 * sizeof(int32_t);
constexpr size_t kAssocDetBytes = 2 * sizeof(double) + sizeof(int32_t);
static inline size_t assoc_lds(int C, int M_max, bool slot_gate = false) {
    return (size_t)C * (kAssocTrackBytes + (slot_gate ? sizeof(double) : 0)) + (size_t)M_max * kAssocDetBytes;
}

// A state word of a track (of a detection): kUnknown before its first scan, kNone when no free partner is in reach, the
// index >= 0 of its best free partner, or, once matched, assoc_take(partner) <= -3.
constexpr int kNone = -1, kUnknown = -2;
__device__ __forceinline__ int assoc_take(int partner) { return -3 - partner; }
__device__ __forceinline__ bool assoc_taken(int word) { return word <= -3; }
__device__ __forceinline__ int assoc_partner(int word) { return -3 - word; }

// The lanes that share one row or column of a scan, and their reduction: (best, at) <- the minimum of (cost, index)
// over the group's lanes, at < 0 = nothing found.  Every lane of the wave calls it; a group is kAssocGroup aligned lanes.
constexpr int kAssocGroup = 8;
__device__ __forceinline__ void assoc_group_min(double &best, int &at) {
#pragma unroll
    for (int o = kAssocGroup / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, kWave);
        const int oa = __shfl_xor(at, o, kWave);
        if (oa >= 0 && (at < 0 || ob < best || (ob == best && oa < at))) {
            best = ob;
            at = oa;
        }
    }
}

// q = pos + vel * k and the squared distance, one IEEE operation at a time
__device__ __forceinline__ double assoc_predict(double pos, double vel, double k) {
#pragma clang fp contract(off)
    const double t = vel * k;
    return pos + t;
}
__device__ __forceinline__ double assoc_cost(double qx, double qy, double px, double py) {
#pragma clang fp contract(off)
    const double dx = qx - px, dy = qy - py;
    const double a = dx * dx, b = dy * dy;
    return a + b;
}
// vel = (p - pos) / k
__device__ __forceinline__ double assoc_velocity(double p, double pos, double k) {
#pragma clang fp contract(off)
    const double d = p - pos;
    return d / k;
}

// The state both rules keep per slot, and per stream; the slot's word of the motion policy is the policy's own
struct AssocState {
    int64_t *trk_id;         // (C)    -1 = free
    double *trk_pos;         // (C,2)  the last matched rounded position
    double *trk_vel;         // (C,2)  displacement per push (timed: per model step)
    int32_t *trk_hits;       // (C)    matches so far
    int64_t *next_id;        // (1)
    int32_t *assoc_flags;    // (1)    STG_ASSOC_* of the last push
    __device__ __forceinline__ AssocState of_stream(int64_t b, int C) const {
        return {trk_id + b * C, trk_pos + b * C * 2, trk_vel + b * C * 2, trk_hits + b * C, next_id + b, assoc_flags + b};
    }
};

struct AssocGates {
    double scale, gate2, gate_new2;
};

// What a match does under the two-sample rules: vel = (p - pos) / k, pos = p
__device__ __forceinline__ void assoc_two_sample(const AssocState &st, int s, double k, double px, double py, double ox,
                                                 double oy) {
    st.trk_vel[2 * s] = assoc_velocity(px, ox, k);
    st.trk_vel[2 * s + 1] = assoc_velocity(py, oy, k);
    st.trk_pos[2 * s] = px;
    st.trk_pos[2 * s + 1] = py;
}
struct AssocNoMore {};       // what a policy loads per slot ahead of the update, beside the shared words: nothing

// The untimed motion: every push is one step.  The word is trk_miss, the pushes since the last match.
struct PushMotion {
    int32_t *trk_miss;       // (C)
    int max_miss;
    using Word = int;
    using More = AssocNoMore;
    static constexpr bool kSlotGate = false;
    __device__ __forceinline__ More more(const AssocState &, int) const { return {}; }
    // a matched slot: its prediction (qx, qy), detection (px, py) and old position (ox, oy)
    __device__ __forceinline__ void update(const AssocState &st, int s, Word miss, const More &, double, double, double px,
                                           double py, double ox, double oy) const {
        assoc_two_sample(st, s, steps(miss), px, py, ox, oy);
        matched(s);
    }
    __device__ __forceinline__ PushMotion of_stream(int64_t b, int C) const { return {trk_miss + b * C, max_miss}; }
    __device__ __forceinline__ Word word(int s) const { return trk_miss[s]; }
    __device__ __forceinline__ double steps(Word miss) const { return (double)(miss + 1); }
    __device__ __forceinline__ void matched(int s) const { trk_miss[s] = 0; }
    // a live slot not matched: true = it is freed (the word zeroed with the rest), else it ages
    __device__ __forceinline__ bool missed(int s, Word miss) const {
        const bool gone = miss + 1 > max_miss;
        trk_miss[s] = gone ? 0 : miss + 1;
        return gone;
    }
    __device__ __forceinline__ void born(int s) const { trk_miss[s] = 0; }
};

// The order test of the timed push (frames_time.hip, step 0) on the same words, for the rules on timestamped pushes.  A
// refused push: -1 to the ids of its detections, the flag, nothing else.  Returns true when the push was refused;
// uniform over the block, no barrier.
constexpr int kFlagAssocTimeOrder = STG_ASSOC_TIME_ORDER;
template <int kThreads>
__device__ __forceinline__ bool assoc_refused(const DetectionsOut &det, int count, int M_max, int64_t t_now,
                                              const int64_t *clock, int32_t *assoc_flags) {
    if (!(clock[1] > 0 && t_now <= clock[0])) return false;
    const int m = count < 0 ? 0 : (count > M_max ? M_max : count);
    for (int j = threadIdx.x; j < m; j += kThreads) det.id_at(j) = -1;
    if (threadIdx.x == 0) assoc_flags[0] = kFlagAssocTimeOrder;
    return true;
}

// One push of one stream by one workgroup of kThreads threads: the positions of the detections j < min(count, M_max)
// are read, their ids written.
template <int kThreads, class Motion>
__device__ __forceinline__ void associate_body(const DetectionsOut &det, int count, int M_max, const AssocState st,
                                               const Motion mo, int C, const AssocGates rule) {
    extern __shared__ __align__(16) unsigned char lds[];
    double *tq = reinterpret_cast<double *>(lds);               // (C,2) predicted positions
    double *dp = tq + 2 * (size_t)C;                             // (M_max,2) rounded detections
    double *tg2 = dp + 2 * (size_t)M_max;                        // (C) the slot's squared gate, under kSlotGate only
    int32_t *tgate = reinterpret_cast<int32_t *>(tg2 + (Motion::kSlotGate ? (size_t)C : 0));
                                                                 // (C) -1 free slot, 0 gate_new2, 1 gate2
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
        const double k = mo.steps(mo.word(s));
        tq[2 * s] = assoc_predict(st.trk_pos[2 * s], st.trk_vel[2 * s], k);
        tq[2 * s + 1] = assoc_predict(st.trk_pos[2 * s + 1], st.trk_vel[2 * s + 1], k);
        if constexpr (Motion::kSlotGate) tg2[s] = mo.gate(s, k);
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
    const auto gate_of = [&](int s) -> double {
        if constexpr (Motion::kSlotGate) return tg2[s];
        else return tgate[s] ? rule.gate2 : rule.gate_new2;
    };
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
                const double qx = tq[2 * s], qy = tq[2 * s + 1], g2 = gate_of(s);
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
                    if (c <= gate_of(s) && (at < 0 || c < best)) {
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

    // 3. the tracks: a matched one moves, one not matched ages and is freed past the policy's limit.  Again every load is
    //    unconditional and the loop holds no barrier; tgate becomes the mark of a free slot (-1) for the list below
#pragma unroll 4
    for (int s = tid; s < C; s += kThreads) {
        const int64_t id = st.trk_id[s];
        const typename Motion::Word w = mo.word(s);
        const int hits = st.trk_hits[s];
        const double ox = st.trk_pos[2 * s], oy = st.trk_pos[2 * s + 1];
        const typename Motion::More more = mo.more(st, s);
        if (tgate[s] < 0) continue;
        const int was = tstate[s];
        if (assoc_taken(was)) {
            const int j = assoc_partner(was);
            mo.update(st, s, w, more, tq[2 * s], tq[2 * s + 1], dp[2 * j], dp[2 * j + 1], ox, oy);
            st.trk_hits[s] = hits + 1;
            det.id_at(j) = id;
            tgate[s] = 0;
        } else if (mo.missed(s, w)) {
            st.trk_id[s] = -1;
            st.trk_pos[2 * s] = st.trk_pos[2 * s + 1] = 0.0;
            st.trk_vel[2 * s] = st.trk_vel[2 * s + 1] = 0.0;
            st.trk_hits[s] = 0;
            tgate[s] = -1;
        } else {
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
                mo.born(s);
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

}  // namespace stg
