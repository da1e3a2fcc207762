"""The filtered association rule of DESIGN.md 5.29 restated in numpy: the sequential greedy in plain loops, float64, one
operation at a time in the order of the kernel's statement (include/stgcnn_hip_assoc_filter.h, N13).  No part of it
looks at the kernel's rounds.  The clock is the timed push's: {time of the last accepted push, accepted pushes}; the
restatement keeps its own copy and moves it as that push would, so it can be fed alone."""
import numpy as np

from assoc_np import FULL, round_pos
from assoc_time_np import TIME_ORDER

F = np.float64


def ahead(p00, p01, p11, k, qa, r):
    """N13, 1.: the covariance of one axis predicted over k steps, and the innovation variance -> a00, a01, a11, S."""
    w = qa * k
    a11 = p11 + w
    u = k * p11
    wk = w * k
    a01 = (p01 + u) + wk / F(2.0)
    a00 = (p00 + k * (F(2.0) * p01 + u)) + (wk * k) / F(3.0)
    return a00, a01, a11, a00 + r


class FilteredTracker:
    """One stream: C slots, the parameters given as plain sigmas and distances (squared here in float64, as the host
    does), step and max_age in ticks."""

    def __init__(self, capacity, sigma_det, sigma_acc, sigma_vel0=1.5, gate_sigmas=5.0, gate_max=2.0, max_age=0, step=10,
                 m_max=None, decimals=4):
        self.c = int(capacity)
        self.r = F(sigma_det) * F(sigma_det)
        self.qa = F(sigma_acc) * F(sigma_acc)
        self.v0 = F(sigma_vel0) * F(sigma_vel0)
        self.n2 = F(gate_sigmas) * F(gate_sigmas)
        self.gmax2 = F(gate_max) * F(gate_max)
        assert self.r > 0 and self.qa >= 0 and self.v0 > 0 and self.n2 > 0 and self.gmax2 > 0
        self.max_age, self.step = int(max_age), int(step)
        assert self.step >= 1 and self.max_age >= 0
        self.m_max = m_max
        self.scale = 0.0 if decimals is None else float(10 ** decimals)
        self.trk_id = np.full(self.c, -1, np.int64)
        self.trk_pos = np.zeros((self.c, 2), np.float64)
        self.trk_vel = np.zeros((self.c, 2), np.float64)
        self.trk_t = np.zeros(self.c, np.int64)
        self.trk_cov = np.zeros((self.c, 3), np.float64)
        self.trk_hits = np.zeros(self.c, np.int32)
        self.next_id = np.int64(0)
        self.flags = 0
        self.clock = [0, 0]
        self.last_s = {}                                    # slot -> S of the last accepted push (for the tests)

    def state(self):
        return (self.trk_id, self.trk_pos, self.trk_vel, self.trk_t, self.trk_cov, self.trk_hits,
                np.array([self.next_id], np.int64), np.array([self.flags], np.int32))

    def live(self):
        """(ids, pos, vel) of the live slots in slot order."""
        at = np.flatnonzero(self.trk_id >= 0)
        return self.trk_id[at], self.trk_pos[at], self.trk_vel[at]

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
        step = F(self.step)
        live = [s for s in range(self.c) if self.trk_id[s] >= 0]
        k_of, q_of, a_of = {}, {}, {}
        cand = []
        self.last_s = {}
        for s in live:
            k = F(t_now - int(self.trk_t[s])) / step                   # one division
            assert k > 0
            k_of[s] = k
            q = self.trk_pos[s] + self.trk_vel[s] * k                  # one product, one sum per coordinate
            q_of[s] = q
            a_of[s] = ahead(*self.trk_cov[s], k, self.qa, self.r)
            big_s = a_of[s][3]
            self.last_s[s] = big_s
            g2 = min(self.n2 * big_s, self.gmax2)
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
                a00, a01, a11, big_s = a_of[s]
                k0 = a00 / big_s
                k1 = a01 / big_s
                e = p[j] - q_of[s]
                self.trk_pos[s] = q_of[s] + k0 * e
                self.trk_vel[s] = self.trk_vel[s] + k1 * e
                self.trk_cov[s] = (a00 - k0 * a00, a01 - k0 * a01, a11 - k1 * a01)
                self.trk_t[s] = t_now
                self.trk_hits[s] += 1
            elif t_now - int(self.trk_t[s]) > self.max_age:
                self.trk_id[s] = -1
                self.trk_pos[s] = 0.0
                self.trk_vel[s] = 0.0
                self.trk_t[s] = 0
                self.trk_cov[s] = 0.0
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
                self.trk_cov[s] = (self.r, 0.0, self.v0)
                self.trk_hits[s] = 1
            else:
                self.flags |= FULL
            i += 1
        self.next_id = np.int64(self.next_id + i)
        return ids


def wrong_links(pushes, times, step, sigma_det, sigma_acc, sigma_vel0=1.5, gate_sigmas=5.0, gate_max=2.0, max_age=0,
                capacity=1024, decimals=4, within=None):
    """assoc_time_np.wrong_links' count under the filtered rule: pushes [(recorded ids, xy)] at `times` -> (wrong links,
    links), a link being a detection whose recorded id was in the previous push or, with `within`, was last detected at
    most `within` ticks ago."""
    trk = FilteredTracker(capacity, sigma_det, sigma_acc, sigma_vel0, gate_sigmas, gate_max, max_age, step,
                          decimals=decimals)
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


def noisy(pushes, sigma, seed):
    """Seeded Gaussian detector noise on every detection: gen = default_rng(seed); per push, in order,
    around(xy + gen.normal(0, sigma, xy.shape), 4).  Applied before assoc_time_np.damaged."""
    gen = np.random.default_rng(seed)
    out = []
    for ids, xy in pushes:
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        out.append((ids, np.around(xy + gen.normal(0, sigma, xy.shape), 4)))
    return out
