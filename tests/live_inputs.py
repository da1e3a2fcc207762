"""Inputs and scene assertions for the tests of the live path (test_gpu_frames.py, test_gpu_frames_streams.py,
test_gpu_frames_fill.py, test_gpu_frames_time.py, test_gpu_score.py, test_gpu_detections.py, test_gpu_push_slots.py):
the committed recordings as rows and as pushes, the golden models, a schedule of pushes over many streams, a sparse
recording, the feed of the slot-table tests, the C push driven directly, and the bit-for-bit comparison of one padded
scene."""
import ctypes
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


def _sparse_rows():
    """40 frames, 30 ids, each present in a frame with probability 0.7."""
    gen = np.random.default_rng(12)
    rows = np.array([(10.0 * t, float(k)) for t in range(40) for k in range(100, 130) if gen.random() < 0.7])
    return np.concatenate([rows, gen.uniform(-20, 20, size=(len(rows), 2))], axis=1)


def _slot_feed():
    """60 pushes (ids, xy) over 120 ids, half of them above 2^33, for a state of 70 slots and 80 detections a push: the
    first n of a permutation, n in [84, 90] when f % 7 == 3 (TRUNCATED, OVERFLOW), in [0, 3] when f % 7 is 1 or 2 (the
    slots run free), else in [4, 35]; when f % 4 == 0 the first id once more (DUPLICATE).  tests/test_push_slots_cpu.py
    holds what the feed has to reach."""
    gen = np.random.default_rng(7)
    ids = np.array([(3 * i + 11) | ((i % 2) << 33) for i in range(120)], np.int64)
    feed = []
    for f in range(60):
        lo, hi = (84, 90) if f % 7 == 3 else (0, 3) if f % 7 in (1, 2) else (4, 35)
        n = int(gen.integers(lo, hi + 1))
        p = gen.permutation(ids)[:n]
        feed.append(np.concatenate([p, p[:1]]) if f % 4 == 0 else p)
    return [(p, _xy(gen, len(p))) for p in feed]


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


class _CPush:
    """stg_track_push_timed (time=(step, max_dt, R)) or stg_track_push_rule driven directly: the caller's state and
    staging tensors.  The outputs are pre-filled with 7s: the kernel writes every element."""

    def __init__(self, dev, rule, v, s, m_max, t_obs=8, decimals=4, time=None):
        from social_stgcnn_amd import frames
        self.dev, self.rule, self.v, self.s, self.m_max, self.t, self.time = dev, rule, v, s, m_max, t_obs, time
        self.scale = frames._scale(decimals)
        z = lambda shape, dt: torch.zeros(shape, device=dev, dtype=dt)      # noqa: E731
        self.slot_id = torch.full((s,), -1, device=dev, dtype=torch.int64)
        self.head_flags = z(2, torch.int32)
        if time is None:
            self.state = (self.slot_id, z(s, torch.int32), z((t_obs, s, 2), torch.float64), self.head_flags)
        else:
            r = time[2]
            self.state = (self.slot_id, z((s, r), torch.int64), z((s, r, 2), torch.float64), z((s, 2), torch.int32),
                          z(2, torch.int64), self.head_flags)

    def push(self, ids, xy, t=None, count=None):
        from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
        dev, m = self.dev, len(ids)
        det_id = torch.zeros(max(m, self.m_max), device=dev, dtype=torch.int64)
        det_xy = torch.zeros((max(m, self.m_max), 2), device=dev, dtype=torch.float64)
        det_id[:m] = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
        det_xy[:m] = torch.from_numpy(np.asarray(xy, np.float64).reshape(-1, 2)).to(dev)
        cnt = torch.tensor([m if count is None else count], device=dev, dtype=torch.int32)
        obs = torch.full((self.t, self.v, 2), 7.0, device=dev, dtype=torch.float64)
        out_ids = torch.full((self.v,), 7, device=dev, dtype=torch.int64)
        peds = torch.full((1,), 7, device=dev, dtype=torch.int32)
        seen = torch.full((self.v,), 7, device=dev, dtype=torch.int32)
        outs = (ptr(obs), ptr(out_ids), ptr(peds), ptr(seen), stream_ptr())
        if self.time is None:
            check(lib().stg_track_push_rule(ptr(det_id), ptr(det_xy), ptr(cnt), self.m_max, *map(ptr, self.state),
                                            self.s, self.t, ctypes.c_double(self.scale), self.v, *self.rule, *outs),
                  "stg_track_push_rule")
        else:
            when = torch.tensor([t], device=dev, dtype=torch.int64)
            check(lib().stg_track_push_timed(ptr(det_id), ptr(det_xy), ptr(cnt), ptr(when), self.m_max,
                                             *map(ptr, self.state), self.s, self.time[2], self.t,
                                             ctypes.c_double(self.scale), self.v, self.time[0], self.time[1],
                                             *self.rule, *outs), "stg_track_push_timed")
        return (out_ids.cpu().numpy(), int(peds.item()), obs.cpu().numpy(), seen.cpu().numpy(),
                int(self.head_flags[1].item()))
