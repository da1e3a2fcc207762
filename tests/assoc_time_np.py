"""The timed association rule of DESIGN.md 5.28 restated in numpy: the sequential greedy in plain loops, float64, the
same operation order as the kernel's statement (include/stgcnn_hip_assoc_time.h, N12).  No part of it looks at the
kernel's rounds.  The clock is the timed push's: {time of the last accepted push, accepted pushes}; the restatement keeps
its own copy and moves it as that push would, so it can be fed alone."""
import numpy as np

from assoc_np import FULL, round_pos

TIME_ORDER = 2                                             # STG_ASSOC_TIME_ORDER


class TimedTracker:
    """One stream: C slots, gates given as plain distances (squared here in float64, as the host does), step and
    max_age in ticks."""

    def __init__(self, capacity, gate, gate_new=None, max_age=0, step=10, m_max=None, decimals=4):
        self.c = int(capacity)
        self.gate2 = np.float64(gate) * np.float64(gate)
        gn = np.float64(2.0 * gate if gate_new is None else gate_new)
        self.gate_new2 = gn * gn
        self.max_age, self.step = int(max_age), int(step)
        assert self.step >= 1 and self.max_age >= 0
        self.m_max = m_max
        self.scale = 0.0 if decimals is None else float(10 ** decimals)
        self.trk_id = np.full(self.c, -1, np.int64)
        self.trk_pos = np.zeros((self.c, 2), np.float64)
        self.trk_vel = np.zeros((self.c, 2), np.float64)
        self.trk_t = np.zeros(self.c, np.int64)
        self.trk_hits = np.zeros(self.c, np.int32)
        self.next_id = np.int64(0)
        self.flags = 0
        self.clock = [0, 0]

    def state(self):
        return (self.trk_id, self.trk_pos, self.trk_vel, self.trk_t, self.trk_hits,
                np.array([self.next_id], np.int64), np.array([self.flags], np.int32))

    def push(self, xy, t_now):
        """xy (count,2) at the time t_now -> the ids of the first m = min(count, m_max) detections."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        t_now = int(t_now)
        m = len(xy) if self.m_max is None else min(len(xy), self.m_max)
        if self.clock[1] > 0 and t_now <= self.clock[0]:
            self.flags = TIME_ORDER
            return np.full(m, -1, np.int64)
        self.clock = [t_now, self.clock[1] + 1]
        p = round_pos(xy[:m], self.scale).reshape(m, 2)
        step = np.float64(self.step)
        live = [s for s in range(self.c) if self.trk_id[s] >= 0]
        k_of = {s: np.float64(t_now - int(self.trk_t[s])) / step for s in live}     # one division
        cand = []
        for s in live:
            assert k_of[s] > 0
            q = self.trk_pos[s] + self.trk_vel[s] * k_of[s]            # one product, one sum per coordinate
            g2 = self.gate2 if self.trk_hits[s] >= 2 else self.gate_new2
            for j in range(m):
                dx = q[0] - p[j, 0]
                dy = q[1] - p[j, 1]
                cost = dx * dx + dy * dy
                if cost <= g2:
                    cand.append((cost, s, j))
        cand.sort()
        t_of, d_of = {}, {}
        for cost, s, j in cand:
            if s not in t_of and j not in d_of:
                t_of[s] = j
                d_of[j] = s
        ids = np.full(m, -1, np.int64)
        for s in live:
            if s in t_of:
                j = t_of[s]
                ids[j] = self.trk_id[s]
                self.trk_vel[s] = (p[j] - self.trk_pos[s]) / k_of[s]
                self.trk_pos[s] = p[j]
                self.trk_t[s] = t_now
                self.trk_hits[s] += 1
            elif t_now - int(self.trk_t[s]) > self.max_age:
                self.trk_id[s] = -1
                self.trk_pos[s] = 0.0
                self.trk_vel[s] = 0.0
                self.trk_t[s] = 0
                self.trk_hits[s] = 0
        free = [s for s in range(self.c) if self.trk_id[s] < 0]
        self.flags = 0
        i = 0
        for j in range(m):
            if j in d_of:
                continue
            ids[j] = self.next_id + i
            if i < len(free):
                s = free[i]
                self.trk_id[s] = ids[j]
                self.trk_pos[s] = p[j]
                self.trk_vel[s] = 0.0
                self.trk_t[s] = t_now
                self.trk_hits[s] = 1
            else:
                self.flags |= FULL
            i += 1
        self.next_id = np.int64(self.next_id + i)
        return ids


def wrong_links(pushes, times, step, gate=1.0, gate_new=2.0, max_age=0, capacity=1024, decimals=4, within=None):
    """pushes: [(recorded ids, xy)] at `times`.  Among the detections whose recorded id was also in the previous push,
    (those whose assigned id differs from the one that pedestrian had then, their number): assoc_np.wrong_links' count.
    within (ticks): the detections whose recorded id was last detected at most `within` ticks ago count too, against the
    id it had at that detection -- the links a track has to survive missed detections and missed pushes for."""
    trk = TimedTracker(capacity, gate, gate_new, max_age, step, decimals=decimals)
    last = {}                                               # recorded id -> (assigned id, the time of that detection)
    t_prev = None
    wrong = total = 0
    for (rec, xy), t in zip(pushes, times):
        got = trk.push(xy, t)
        rec = np.asarray(rec).tolist()
        for r, g in zip(rec, got.tolist()):
            if r in last and (last[r][1] == t_prev or (within is not None and t - last[r][1] <= within)):
                total += 1
                wrong += int(last[r][0] != g)
        for r, g in zip(rec, got.tolist()):
            last[r] = (g, t)
        t_prev = t
    return wrong, total


def damaged(pushes, times, seed=0, drop=0.05):
    """The damaged feed: every push with i % 7 == 3 left out, and of the detections left each dropped with probability
    `drop`, drawn from default_rng(seed) push by push."""
    gen = np.random.default_rng(seed)
    out, at = [], []
    for i, ((ids, xy), t) in enumerate(zip(pushes, times)):
        if i % 7 == 3:
            continue
        keep = gen.random(len(ids)) >= drop
        out.append((np.asarray(ids)[keep], np.asarray(xy).reshape(-1, 2)[keep]))
        at.append(t)
    return out, at
