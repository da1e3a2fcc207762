"""numpy restatement of the rule for partially observed tracks (social_stgcnn_amd.frames.TrackRule),
beside tests/frames_np.py, which states the strict rule.

The window of a frame has obs_len steps, oldest first, the last one the frame itself; frames before the first one count
as missed.  An id is in the scene iff it is seen at the last step, seen in at least min_seen steps, and every run of
missed steps between two seen steps is at most max_gap long (missed steps ahead of the first seen one are no gap).
Missed steps are filled in float64, one operation at a time:

    interior  a < t < b the nearest seen steps:  p[t] = around(p[a] + (p[b] - p[a]) * (float(t - a) / float(b - a)))
    leading   t < a0, the first seen step, q the window after the interior fill:
                                                 p[t] = around(q[a0] - float(a0 - t) * (q[a0 + 1] - q[a0]))

`seen` has bit t set when the pedestrian was observed t frames ago (bit 0: this frame).  Dense (ids x frames) tables
and Python loops: a test helper, not the product path."""
import numpy as np

import frames_np


def round_pos(x, decimals):
    return x if decimals is None else np.around(x, decimals=decimals)


def is_member(present, min_seen, max_gap):
    """present (T,) bool, oldest step first."""
    if not present[-1] or int(present.sum()) < min_seen:
        return False
    at = np.nonzero(present)[0]
    return bool(np.all(np.diff(at) - 1 <= max_gap))


def seen_bits(present):
    t_obs = len(present)
    return sum(1 << (t_obs - 1 - t) for t in range(t_obs) if present[t])


def present_of(bits, t_obs):
    """The inverse of seen_bits: (t_obs,) bool, oldest step first."""
    return np.array([(int(bits) >> (t_obs - 1 - t)) & 1 for t in range(t_obs)], dtype=bool)


def fill_window(pos, present, decimals):
    """pos (T,2) float64 with the rounded positions of the seen steps, present (T,) bool with the last step and at
    least one more seen -> the window (T,2) with every missed step filled."""
    q = np.array(pos, dtype=np.float64)
    at = np.nonzero(present)[0]
    for a, b in zip(at[:-1], at[1:]):
        for t in range(a + 1, b):
            q[t] = round_pos(q[a] + (q[b] - q[a]) * (float(t - a) / float(b - a)), decimals)
    a0 = at[0]
    d = q[a0 + 1] - q[a0]
    for t in range(a0):
        q[t] = round_pos(q[a0] - float(a0 - t) * d, decimals)
    return q


def fill_tracks(obs_abs, seen, num_peds=None, decimals=4):
    """What frames.fill_tracks computes: obs_abs (N,T,V,2) float64, seen (N,V) -> a filled copy.  A column's seen steps
    are rounded and its missed steps filled; a column at or past num_peds, not seen now or seen only once stays."""
    out = np.array(obs_abs, dtype=np.float64)
    n, t_obs, v, _ = out.shape
    for i in range(n):
        for j in range(v if num_peds is None else int(num_peds[i])):
            present = present_of(int(seen[i, j]) & ((1 << t_obs) - 1), t_obs)
            if not present[-1] or present.sum() < 2:
                continue
            col = out[i, :, j].copy()
            col[present] = round_pos(col[present], decimals)
            out[i, :, j] = fill_window(col, present, decimals)
    return out


def _scene(window_present, window_pos, keys, min_seen, max_gap, decimals):
    """window_present (n_p,T) bool, window_pos (n_p,T,2) rounded, keys (n_p,) ascending ids -> (ids, obs (T,V,2),
    seen (V,) int32) of the members."""
    sel = [i for i in range(len(keys)) if is_member(window_present[i], min_seen, max_gap)]
    t_obs = window_present.shape[1]
    obs = np.zeros((t_obs, len(sel), 2))
    for j, i in enumerate(sel):
        obs[:, j] = fill_window(window_pos[i], window_present[i], decimals)
    seen = np.array([seen_bits(window_present[i]) for i in sel], dtype=np.int32)
    return np.asarray(keys, np.int64)[sel], obs, seen


def frame_scenes_rule(rows, obs_len=8, min_seen=8, max_gap=0, min_peds=1, decimals=4):
    """[(frame index f, frame number, ids int64 (V_f,), obs_abs float64 (obs_len,V_f,2), seen int32 (V_f,))] for every
    frame index f >= min_seen - 1 whose scene holds at least min_peds pedestrians."""
    frames, ped_ids, present, pos = frames_np.recording_tables(rows, decimals)
    n_p = len(ped_ids)
    # obs_len - 1 missed frames ahead of the recording's first
    present = np.concatenate([np.zeros((n_p, obs_len - 1), bool), present], axis=1)
    pos = np.concatenate([np.zeros((n_p, obs_len - 1, 2)), pos], axis=1)
    out = []
    for f in range(min_seen - 1, len(frames)):
        now = np.nonzero(present[:, f + obs_len - 1])[0]
        ids, obs, seen = _scene(present[now, f:f + obs_len], pos[now, f:f + obs_len], ped_ids[now], min_seen, max_gap,
                                decimals)
        if len(ids) >= min_peds:
            out.append((f, frames[f], ids, obs, seen))
    return out


class StreamModelRule:
    """The live rule push by push: the window is the last obs_len pushes (fewer at the start: the rest count as
    missed); ids in ascending order, at most max_peds of them (the smallest); positions rounded at push time; a
    repeated id within a push keeps its first detection.  Slots and their overflow are not modelled."""

    def __init__(self, obs_len=8, min_seen=8, max_gap=0, max_peds=128, decimals=4):
        self.t, self.min_seen, self.max_gap, self.v, self.decimals = obs_len, min_seen, max_gap, max_peds, decimals
        self.hist = []                  # one {id: (x, y)} per push

    def reset(self):
        self.hist = []

    def push(self, ids, xy):
        """-> (ids (V_f,) int64, obs_abs (obs_len,V_f,2), seen (V_f,) int32, more than max_peds qualified)"""
        now = {}
        for i, p in zip(np.asarray(ids, np.int64).tolist(), np.asarray(xy, np.float64).reshape(-1, 2)):
            if i not in now:
                now[i] = round_pos(p, self.decimals)
        self.hist.append(now)
        self.hist = self.hist[-self.t:]
        last = [{}] * (self.t - len(self.hist)) + self.hist
        keys = sorted(now)
        present = np.array([[k in h for h in last] for k in keys], dtype=bool).reshape(len(keys), self.t)
        pos = np.array([[h.get(k, (0.0, 0.0)) for h in last] for k in keys], dtype=np.float64).reshape(len(keys), self.t, 2)
        ids_o, obs, seen = _scene(present, pos, keys, self.min_seen, self.max_gap, self.decimals)
        return ids_o[:self.v], obs[:, :self.v], seen[:self.v], len(ids_o) > self.v
