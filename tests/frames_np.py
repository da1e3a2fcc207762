"""numpy restatement of the frame-scene rule (social_stgcnn_amd.frames): the reference's windowing (utils.py:123-165)
with the future dropped.  Frames are the recording's distinct frame numbers in ascending order (np.unique, utils.py:123);
the scene at frame index f >= obs_len - 1 is every pedestrian id with a row in each of the frames f-obs_len+1 .. f, in
ascending id order, positions rounded as np.around(x, decimals) (utils.py:145).  Dense (ids x frames) tables: a test
helper, not the product path."""
import numpy as np


def recording_tables(rows, decimals=4):
    """rows (M,4) -> (frames (F,), ped_ids (n_p,), present (n_p,F) bool, pos (n_p,F,2) float64 rounded)."""
    rows = np.asarray(rows, dtype=np.float64)
    frames = np.unique(rows[:, 0])
    ped_ids = np.unique(rows[:, 1])
    f_idx = np.searchsorted(frames, rows[:, 0])
    p_idx = np.searchsorted(ped_ids, rows[:, 1])
    present = np.zeros((len(ped_ids), len(frames)), dtype=bool)
    present[p_idx, f_idx] = True
    pos = np.zeros((len(ped_ids), len(frames), 2))
    xy = rows[:, 2:4] if decimals is None else np.around(rows[:, 2:4], decimals=decimals)
    pos[p_idx, f_idx] = xy
    return frames, ped_ids, present, pos


def frame_scenes(rows, obs_len=8, min_peds=1, decimals=4):
    """[(frame index f, frame number, ids int64 (V_f,), obs_abs float64 (obs_len, V_f, 2))] for every frame index
    f >= obs_len - 1 whose scene holds at least min_peds pedestrians."""
    frames, ped_ids, present, pos = recording_tables(rows, decimals)
    out = []
    for f in range(obs_len - 1, len(frames)):
        sel = np.nonzero(present[:, f - obs_len + 1:f + 1].all(axis=1))[0]
        if len(sel) < min_peds:
            continue
        out.append((f, frames[f], ped_ids[sel].astype(np.int64),
                    np.ascontiguousarray(np.transpose(pos[sel, f - obs_len + 1:f + 1], (1, 0, 2)))))
    return out


def dataset_windows(rows, obs_len=8, pred_len=12, min_ped=1):
    """The windows data.load_windows keeps for one recording (skip 1), as [(start frame index, ids int64)]: every
    pedestrian tracked over the whole obs_len + pred_len window, more than min_ped of them (utils.py:130-165)."""
    seq_len = obs_len + pred_len
    frames, ped_ids, present, _ = recording_tables(rows, None)
    out = []
    for idx in range(0, len(frames) - seq_len + 1):
        sel = np.nonzero(present[:, idx:idx + seq_len].all(axis=1))[0]
        if len(sel) > min_ped:
            out.append((idx, ped_ids[sel].astype(np.int64)))
    return out


class StreamModel:
    """The live-stream rule restated push by push: a pedestrian is in the scene of a push when it was detected in each
    of the last obs_len pushes (this one included); ids in ascending order, at most max_peds of them (the smallest);
    positions rounded at push time.  Slots and their overflow are not modelled (the default capacity never runs out
    in the tests that use this)."""

    def __init__(self, obs_len=8, max_peds=128, decimals=4):
        self.t, self.v, self.decimals = obs_len, max_peds, decimals
        self.hist = []                  # one {id: (x, y)} per push

    def push(self, ids, xy):
        seen = {}
        for i, p in zip(np.asarray(ids, np.int64).tolist(), np.asarray(xy, np.float64).reshape(-1, 2)):
            if i not in seen:           # a duplicate id within a push: the first detection wins
                seen[i] = p if self.decimals is None else np.around(p, self.decimals)
        self.hist.append(seen)
        last = self.hist[-self.t:]
        if len(last) < self.t:
            return np.zeros(0, np.int64), np.zeros((self.t, 0, 2))
        keep = sorted(i for i in last[-1] if all(i in h for h in last))[:self.v]
        obs = np.array([[h[i] for i in keep] for h in last]).reshape(self.t, len(keep), 2)
        return np.asarray(keep, np.int64), obs
