"""numpy statement of the timed live rule (social_stgcnn_amd.frames.TimeRule), beside
tests/frames_fill_np.py, whose membership and fill it reuses.

Time is integer ticks.  A push carries t_now, strictly greater than the stream's previous push (else nothing changes and
the push returns the empty scene with TIME_ORDER).  A detection is recorded as the sample (t_now, around(x), around(y))
of its id; an id keeps its newest `history` samples.  An id is live while t_now - t_newest <= (obs_len - 1) * step; it
is forgotten, samples and all, at the start of the first push for which that fails.  At most `capacity` ids are live:
a new id (detection order) without a free place is dropped for the push (OVERFLOW).

The window of a push has obs_len steps, oldest first; step k is the instant tau = t_now - (obs_len - 1 - k) * step.  It
is observed iff the id has a sample at exactly tau -- that position is taken as it is -- or two samples ta < tau < tb
next to each other in its history with tb - ta <= max_dt -- the position is then, per coordinate and one float64
operation at a time,

    around(pa + (pb - pa) * (float(tau - ta) / float(tb - ta)))

The observed steps are the presence bits (bit j = step obs_len - 1 - j, the orientation of `seen`); membership and the
fill of the missed steps are frames_fill_np.is_member / fill_window.  Plain lists and Python loops: a test helper."""
import numpy as np

import frames_fill_np
from frames_fill_np import round_pos

DUPLICATE, OVERFLOW, TRUNCATED, TOO_MANY, TIME_ORDER = 1, 2, 4, 8, 16


def position_at(samples, tau, max_dt, decimals):
    """samples [(t, x, y)] in ascending t -> the (2,) position at the instant tau, or None where it is not observed."""
    for t, x, y in samples:
        if t == tau:
            return np.array([x, y], dtype=np.float64)
    for (ta, xa, ya), (tb, xb, yb) in zip(samples[:-1], samples[1:]):
        if ta < tau < tb and tb - ta <= max_dt:
            pa, pb = np.array([xa, ya], dtype=np.float64), np.array([xb, yb], dtype=np.float64)
            return round_pos(pa + (pb - pa) * (float(tau - ta) / float(tb - ta)), decimals)
    return None


class StreamModelTimed:
    """The timed rule push by push.  push(ids, xy, t_now) -> (ids (V_f,) int64, obs_abs (obs_len,V_f,2), seen (V_f,)
    int32, flags)."""

    def __init__(self, obs_len=8, step=10, max_dt=None, history=96, min_seen=None, max_gap=0, max_peds=128, decimals=4,
                 capacity=1024, max_detections=1024):
        self.t, self.step, self.max_dt = obs_len, int(step), int(step if max_dt is None else max_dt)
        self.r, self.min_seen, self.max_gap = int(history), obs_len if min_seen is None else min_seen, max_gap
        self.v, self.decimals, self.s, self.m_max = max_peds, decimals, capacity, max_detections
        assert self.step >= 1 and 1 <= self.max_dt <= (obs_len - 1) * self.step and 2 <= self.r <= 256
        self.reset()

    def reset(self):
        self.tracks = {}                # id -> [(t, x, y)] in ascending t, the newest `history` of them
        self.last = None                # the time of the last accepted push
        self.pushes = 0

    def state(self):
        return ({k: list(v) for k, v in self.tracks.items()}, self.last, self.pushes)

    def push(self, ids, xy, t_now):
        t_now = int(t_now)
        if self.last is not None and t_now <= self.last:
            return np.zeros(0, np.int64), np.zeros((self.t, 0, 2)), np.zeros(0, np.int32), TIME_ORDER
        self.last = t_now
        self.pushes += 1
        flags = 0
        ids = np.asarray(ids, np.int64).reshape(-1).tolist()
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        if len(ids) > self.m_max:
            ids, xy, flags = ids[:self.m_max], xy[:self.m_max], flags | TRUNCATED
        span = (self.t - 1) * self.step
        for k in [k for k, smp in self.tracks.items() if t_now - smp[-1][0] > span]:
            del self.tracks[k]
        free = self.s - len(self.tracks)
        now = {}
        for i, p in zip(ids, xy):
            if i in now:
                flags |= DUPLICATE
                continue
            now[i] = None                                       # (a dropped id still shadows its repeats)
            if i not in self.tracks:
                if free == 0:
                    flags |= OVERFLOW
                    continue
                free -= 1
                self.tracks[i] = []
            q = round_pos(p, self.decimals)
            self.tracks[i] = (self.tracks[i] + [(t_now, float(q[0]), float(q[1]))])[-self.r:]
            now[i] = True
        keys = sorted(k for k, ok in now.items() if ok)
        present = np.zeros((len(keys), self.t), dtype=bool)
        pos = np.zeros((len(keys), self.t, 2))
        for n, key in enumerate(keys):
            for k in range(self.t):
                p = position_at(self.tracks[key], t_now - (self.t - 1 - k) * self.step, self.max_dt, self.decimals)
                if p is not None:
                    present[n, k], pos[n, k] = True, p
            assert present[n, -1]
        ids_o, obs, seen = frames_fill_np._scene(present, pos, keys, self.min_seen, self.max_gap, self.decimals)
        if len(ids_o) > self.v:
            flags |= TOO_MANY
        return ids_o[:self.v], obs[:, :self.v], seen[:self.v], flags
