"""GPU (-m gpu): the push and the score kernels stand on one detection sort and one lookup (csrc/detections.hpp,
DESIGN.md 5.18).  The same small detection sets go through stg_track_push and stg_score_push -- and once through the
*_streams forms -- at the sort sizes where a bitonic network or a lower bound can go wrong, ids descending and shuffled,
one id repeated: the scenes bit for bit against frames_np.StreamModel, the scores against score_np.ScoreModel, and the
two kernels against each other on the repeated id."""
import ctypes

import numpy as np
import pytest
import torch

import frames_np
from live_inputs import _assert_scene
from test_gpu_score import BIG, Harness, _exact_prediction, _pos

pytestmark = pytest.mark.gpu
T_OBS, P, V, K, S, M_MAX = 2, 2, 8, 2, 512, 300            # M_MAX is no power of two: the sort buffers hold 512
DUPLICATE, TOO_MANY = 1, 8
# empty, single, two, odd (the first with a repeated id), a power of two, odd again, a wave, a wave and one, more keys
# than the score's 256 threads, the full buffer
SORT_SIZES = (0, 1, 2, 3, 4, 5, 64, 65, 257, 300)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Push:
    """stg_track_push (ns None) or stg_track_push_streams (ns streams, one packed tick) driven directly: the caller's
    state, exact inputs, no model.  tick(entries): entries[s] = None (not pushed) or (ids, xy); returns per stream
    (ids (V,), num_peds, obs (T_OBS,V,2), flags)."""

    def __init__(self, dev, ns=None):
        self.dev, self.ns, n = dev, ns, ns or 1
        self.slot_id = torch.full((n, S), -1, device=dev, dtype=torch.int64)
        self.mask = torch.zeros((n, S), device=dev, dtype=torch.int32)
        self.ring = torch.zeros((n, T_OBS, S, 2), device=dev, dtype=torch.float64)
        self.head_flags = torch.zeros((n, 2), device=dev, dtype=torch.int32)

    def tick(self, entries):
        from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
        dev, n = self.dev, self.ns or 1
        t = lambda a: torch.from_numpy(a).to(dev)             # noqa: E731
        pushed = np.array([e is not None for e in entries], np.int32)
        start = np.concatenate([[0], np.cumsum([0 if e is None else len(e[0]) for e in entries])]).astype(np.int32)
        total = max(M_MAX, int(start[-1]))
        det_id, det_xy = np.zeros(total, np.int64), np.zeros((total, 2))
        for s, e in enumerate(entries):
            if e is not None:
                det_id[start[s]:start[s + 1]], det_xy[start[s]:start[s + 1]] = e
        d_id, d_xy, d_start, d_pushed, d_count = t(det_id), t(det_xy), t(start), t(pushed), t(start[1:])
        obs = torch.full((n, T_OBS, V, 2), 7.0, device=dev, dtype=torch.float64)
        ids = torch.full((n, V), 7, device=dev, dtype=torch.int64)
        peds = torch.full((n,), 7, device=dev, dtype=torch.int32)
        state = (ptr(self.slot_id), ptr(self.mask), ptr(self.ring), ptr(self.head_flags), S, T_OBS,
                 ctypes.c_double(1e4), V)
        if self.ns is None:
            check(lib().stg_track_push(ptr(d_id), ptr(d_xy), ptr(d_count), M_MAX, *state, ptr(obs), ptr(ids),
                                       ptr(peds), stream_ptr()), "stg_track_push")
            flags = self.head_flags[:, 1]
        else:
            flags = torch.full((n,), 7, device=dev, dtype=torch.int32)
            check(lib().stg_track_push_streams(ptr(d_id), 1, ptr(d_xy), 2, total, ptr(d_start), ptr(d_pushed), n,
                                               M_MAX, *state, ptr(obs), ptr(ids), ptr(peds), ptr(flags), 0,
                                               stream_ptr()), "stg_track_push_streams")
        out = [x.cpu().numpy() for x in (ids, peds, obs, flags)]
        return [tuple(x[s] for x in out) for s in range(n)]


def _detections(m, seed):
    """Two pushes of m detections over the same ids (half of them above 2^32), the first in descending id order, the
    second shuffled; positions in eighths (exact under the rounding and in float32).  For m >= 3 the smallest id is
    there twice, the second time somewhere else.  Returns [(ids, xy), (ids, xy)] and the repeated id (or None)."""
    distinct = m - 1 if m >= 3 else m
    ids = np.array([7 + 3 * j + (BIG if j >= distinct // 2 and j else 0) for j in range(distinct)], np.int64)
    gen = np.random.default_rng(seed)
    out = []
    for push in range(2):
        d_ids = ids[::-1].copy()
        d_xy = np.array([_pos(i, push) for i in d_ids]).reshape(-1, 2)
        if m >= 3:
            d_ids = np.append(d_ids, ids[0])
            d_xy = np.concatenate([d_xy, d_xy[-1:] + (1.0, -0.5)])
        if push:
            order = gen.permutation(m)
            d_ids, d_xy = d_ids[order], d_xy[order]
        out.append((d_ids, d_xy))
    return out, (int(ids[0]) if m >= 3 else None)


def _first(det, i):
    """The position of id i's first detection."""
    return det[1][np.nonzero(det[0] == i)[0][0]]


def _prediction(pushes, push, rep):
    """What push `push` enqueues: the V smallest ids (the scene the tracks reach one push later) with exact errors; the
    mean of the repeated id at the next step is where its first detection will be, so its error there is 0 exactly
    when the score's truth is that detection."""
    scene = np.unique(pushes[push][0])[:V]
    pr = _exact_prediction(scene, len(scene), push, P, V, K)
    if rep is not None and push + 1 < len(pushes):
        pr.mean[0, 0] = _first(pushes[push + 1], rep)
    return pr


def _check_stream(m, pushes, rep, scenes, scores, what):
    """scenes[push] = (ids, peds, obs, flags) and scores[push] = the score outputs of one stream over its two pushes."""
    ref = frames_np.StreamModel(T_OBS, V, 4)
    distinct = len(np.unique(pushes[0][0]))
    for push, det in enumerate(pushes):
        ids, peds, obs, flags = scenes[push]
        r_ids, r_obs = ref.push(*det)
        _assert_scene(ids, peds, obs, r_ids, r_obs, (what, push))
        assert len(r_ids) == (min(distinct, V) if push else 0), (what, push)
        want = (DUPLICATE if rep is not None else 0) | (TOO_MANY if push and distinct > V else 0)
        assert int(flags) == want, (what, push, int(flags))
    got = scores[1]
    assert got["matched"][0, :min(distinct, V)].all() and int(got["matched"].sum()) == min(distinct, V), what
    if rep is not None:
        # the repeated id is the smallest: slot 0 of the scene and of the record.  The scene's last step holds its first
        # detection, and so does the score's truth (the record's mean was put there: the error is 0 only then)
        ids, _, obs, _ = scenes[1]
        first = _first(pushes[1], rep)
        assert ids[0] == rep and got["rec_ids"][0, 0] == rep and got["matched"][0, 0] == 1, what
        assert np.array_equal(obs[T_OBS - 1, 0], first), (what, obs[T_OBS - 1, 0], first)
        assert got["err"][0, 0] == 0.0 and got["d2"][0, 0] == 0.0, (what, got["err"][0, 0])
        assert np.any(pushes[1][1][pushes[1][0] == rep] != first), what         # the other detection is elsewhere


@pytest.mark.parametrize("m", SORT_SIZES)
def test_push_and_score_agree_at_every_sort_size(dev, m):
    pushes, rep = _detections(m, 40 + m)
    tracks, h = _Push(dev), Harness(dev, 1, P, V, K, (1.0,), M_MAX, single=True)
    scenes, scores = [], []
    for push, det in enumerate(pushes):
        scenes.append(tracks.tick([det])[0])
        got, refs = h.tick([det + (_prediction(pushes, push, rep),)])
        h.assert_bit_equal(got, refs, (m, push))
        scores.append({n: None if x is None else x[0] for n, x in got.items()})
    _check_stream(m, pushes, rep, scenes, scores, m)


def test_push_and_score_agree_through_the_streams_forms(dev):
    """NS = 3 in one packed tick: stream 0 sorts 65 detections, stream 2 sorts 257, stream 1 is not pushed."""
    sizes = {0: 65, 2: 257}
    dets = {s: _detections(m, 90 + s) for s, m in sizes.items()}
    tracks, h = _Push(dev, 3), Harness(dev, 3, P, V, K, (1.0,), M_MAX)
    scenes, scores = {s: [] for s in sizes}, {s: [] for s in sizes}
    for push in range(2):
        out = tracks.tick([dets[s][0][push] if s in dets else None for s in range(3)])
        got, refs = h.tick([dets[s][0][push] + (_prediction(dets[s][0], push, dets[s][1]),) if s in dets else None
                            for s in range(3)])
        h.assert_bit_equal(got, refs, push)
        ids, peds, obs, flags = out[1]
        assert int(peds) == 0 and np.all(ids == -1) and not np.any(obs) and int(flags) == 0, push
        assert not got["matched"][1].any() and np.all(got["rec_ids"][1] == -1), push
        for s in sizes:
            scenes[s].append(out[s])
            scores[s].append({n: None if x is None else x[s] for n, x in got.items()})
    for s, m in sizes.items():
        _check_stream(m, dets[s][0], dets[s][1], scenes[s], scores[s], ("stream", s))
