"""Inputs and scene assertions for the tests of the live path (test_gpu_frames.py, test_gpu_frames_streams.py,
test_gpu_frames_fill.py, test_gpu_score.py, test_gpu_detections.py): the committed recordings as rows and as pushes,
the golden models, a schedule of pushes over many streams, and the bit-for-bit comparison of one padded scene."""
import os

import numpy as np
import torch

from conftest import GOLDEN, load_golden

CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
DATA = os.path.join(GOLDEN, "data")


def _recordings():
    return sorted((d, f) for d in os.listdir(DATA) for f in os.listdir(os.path.join(DATA, d)))


def _rows(d, f):
    from social_stgcnn_amd import data
    return data.read_file(os.path.join(DATA, d, f))


def _model(name, dev):
    from social_stgcnn_amd.model import social_stgcnn
    w = load_golden("weights_%s.npz" % name)
    m = social_stgcnn(**CFG)
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    return m.to(dev).eval()


def _pushes(rows):
    """One (ids, xy) per frame of the recording, rows in file order (the detection order)."""
    frames = np.unique(rows[:, 0])
    f_idx = np.searchsorted(frames, rows[:, 0])
    order = np.argsort(f_idx, kind="stable")
    bounds = np.searchsorted(f_idx[order], np.arange(len(frames) + 1))
    return [(rows[order[a:b], 1].astype(np.int64), np.ascontiguousarray(rows[order[a:b], 2:4]))
            for a, b in zip(bounds[:-1], bounds[1:])]


def _xy(gen, m):
    return gen.uniform(-20, 20, size=(m, 2))            # more decimals than the rounding keeps


class Schedule:
    """Stream s pushes the frames of its recording in order from tick start[s] on; with skip an odd stream skips the
    ticks divisible by s + 3 (its next frame waits for the next tick); a finished recording is not pushed."""

    def __init__(self, pushes, starts, skip=True):
        self.pushes, self.starts, self.skip = pushes, starts, skip
        self.cursor = [0] * len(pushes)

    def tick(self, t):
        out = []
        for s, p in enumerate(self.pushes):
            go = t >= self.starts[s] and self.cursor[s] < len(p) and not (self.skip and s % 2 and t % (s + 3) == 0)
            out.append(p[self.cursor[s]] if go else None)
            self.cursor[s] += int(go)
        return out


def _assert_scene(ids, peds, obs, ref_ids, ref_obs, what, seen=None, ref_seen=None):
    """One padded scene (ids (V,), num_peds, obs (T,V,2), under a TrackRule seen (V,)) equals a restated one bit for
    bit; padded slots are -1 / zeros."""
    c = len(ref_ids)
    assert int(peds) == c, what
    assert np.array_equal(ids[:c], ref_ids) and np.all(ids[c:] == -1), what
    if ref_seen is not None:
        assert np.array_equal(seen[:c], ref_seen) and not np.any(seen[c:]), what
    assert np.array_equal(obs[:, :c], ref_obs), (what, np.argwhere(obs[:, :c] != ref_obs)[:4])
    assert not np.any(obs[:, c:]), what
