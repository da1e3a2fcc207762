"""The association rule of DESIGN.md 5.21 restated in numpy: the sequential greedy in plain loops, float64, the same
operation order as the kernel's statement (include/stgcnn_hip.h, N9).  No part of it looks at the kernel's rounds."""
import numpy as np

FULL = 1                                                   # STG_ASSOC_FULL


def round_pos(x, scale):
    """The push kernels' rounding: rint(x * scale) / scale in float64 (scale <= 0: none)."""
    x = np.asarray(x, np.float64)
    return np.rint(x * scale) / scale if scale > 0 else x.copy()


class Tracker:
    """One stream: C slots, gates given as plain distances (squared here in float64, as the host does)."""

    def __init__(self, capacity, gate, gate_new=None, max_miss=0, m_max=None, decimals=4):
        self.c = int(capacity)
        self.gate2 = np.float64(gate) * np.float64(gate)
        gn = np.float64(2.0 * gate if gate_new is None else gate_new)
        self.gate_new2 = gn * gn
        self.max_miss = int(max_miss)
        self.m_max = m_max
        self.scale = 0.0 if decimals is None else float(10 ** decimals)
        self.trk_id = np.full(self.c, -1, np.int64)
        self.trk_pos = np.zeros((self.c, 2), np.float64)
        self.trk_vel = np.zeros((self.c, 2), np.float64)
        self.trk_miss = np.zeros(self.c, np.int32)
        self.trk_hits = np.zeros(self.c, np.int32)
        self.next_id = np.int64(0)
        self.flags = 0

    def state(self):
        return (self.trk_id, self.trk_pos, self.trk_vel, self.trk_miss, self.trk_hits,
                np.array([self.next_id], np.int64), np.array([self.flags], np.int32))

    def push(self, xy):
        """xy (count,2) -> the ids of the first m = min(count, m_max) detections."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        m = len(xy) if self.m_max is None else min(len(xy), self.m_max)
        p = round_pos(xy[:m], self.scale).reshape(m, 2)
        live = [s for s in range(self.c) if self.trk_id[s] >= 0]
        cand = []
        for s in live:
            k = np.float64(int(self.trk_miss[s]) + 1)
            q = self.trk_pos[s] + self.trk_vel[s] * k                  # one product, one sum per coordinate
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
                k = np.float64(int(self.trk_miss[s]) + 1)
                ids[j] = self.trk_id[s]
                self.trk_vel[s] = (p[j] - self.trk_pos[s]) / k
                self.trk_pos[s] = p[j]
                self.trk_miss[s] = 0
                self.trk_hits[s] += 1
            elif int(self.trk_miss[s]) + 1 > self.max_miss:
                self.trk_id[s] = -1
                self.trk_pos[s] = 0.0
                self.trk_vel[s] = 0.0
                self.trk_miss[s] = 0
                self.trk_hits[s] = 0
            else:
                self.trk_miss[s] += 1
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
                self.trk_miss[s] = 0
                self.trk_hits[s] = 1
            else:
                self.flags |= FULL
            i += 1
        self.next_id = np.int64(self.next_id + i)
        return ids


def wrong_links(pushes, gate=1.0, gate_new=2.0, max_miss=0, capacity=1024, decimals=4):
    """pushes: [(recorded ids, xy)] in order.  Among the detections whose recorded id was also in the previous push,
    (those whose assigned id differs from the one that pedestrian had then, their number)."""
    trk = Tracker(capacity, gate, gate_new, max_miss, decimals=decimals)
    prev = {}
    wrong = total = 0
    for rec, xy in pushes:
        got = trk.push(xy)
        now = {}
        for r, g in zip(rec.tolist(), got.tolist()):
            if r in prev:
                total += 1
                wrong += int(prev[r] != g)
            now[r] = g
        prev = now
    return wrong, total
