"""GPU (-m gpu): the slot table of the live pushes is ONE rule (csrc/track_rule.hpp: assign_slots) -- stg_track_push,
stg_track_push_rule and stg_track_push_timed, and their _streams forms at every workgroup size, put every pedestrian of
the feed of live_inputs._slot_feed into the slot that tests/push_slots_np.py names, after every push, bit for bit.  The
scene tests compare tracks by id and would not see two pushes disagree on a slot.  T_obs = 3, S = 70, M_max = 80 (sort
buffers of 128), V = 8; the timed push at one push per step (step = max_dt = 10, R = 4), where a slot is free exactly
when the mask says so."""
import numpy as np
import pytest
import torch

from live_inputs import _slot_feed
from push_slots_np import DUPLICATE, OVERFLOW, TRUNCATED, SlotModel

pytestmark = pytest.mark.gpu
T, S, M, V, R, STEP, RULE = 3, 70, 80, 8, 4, 10, (2, 1)
KINDS = ("strict", "rule", "timed")
BITS = DUPLICATE | OVERFLOW | TRUNCATED                     # (TOO_MANY depends on the rule)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def want():
    """The feed, the numpy (table, flags) after each of its pushes, and those of its even pushes alone."""
    feed = _slot_feed()
    whole, even = SlotModel(T, S, M), SlotModel(T, S, M)
    return feed, [whole.push(p) for p, _ in feed], [even.push(p) for p, _ in feed[::2]]


class _Push:
    """One kind of push driven through its C entry point: the single-stream one (ns=None) or the _streams one.  The
    state starts as reset() leaves it; the outputs are pre-filled with 7s, so an unwritten element shows."""

    def __init__(self, dev, kind, ns=None, block=0):
        self.dev, self.kind, self.ns, self.block = dev, kind, ns, block
        n = ns or 1
        z = lambda shape, dt: torch.zeros((n,) + shape, device=dev, dtype=dt)       # noqa: E731
        self.slot_id = torch.full((n, S), -1, device=dev, dtype=torch.int64)
        self.head_flags = z((2,), torch.int32)
        if kind == "timed":
            self.state = (self.slot_id, z((S, R), torch.int64), z((S, R, 2), torch.float64), z((S, 2), torch.int32),
                          z((2,), torch.int64), self.head_flags)
        else:
            self.state = (self.slot_id, z((S,), torch.int32), z((T, S, 2), torch.float64), self.head_flags)
        self.start = [x.clone() for x in self.state]

    def push(self, tick):
        """tick: per stream (ids, xy, time), or None for a stream that is not pushed.  -> per stream (slot table,
        flags, out_ids, num_peds, obs_abs, seen or None)."""
        from social_stgcnn_amd import frames
        from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
        dev, n, kind = self.dev, len(tick), self.kind
        go = [e for e in tick if e is not None]
        ids = np.concatenate([e[0] for e in go] + [np.zeros(0, np.int64)])
        xy = np.concatenate([e[1] for e in go] + [np.zeros((0, 2))])
        # (more detections than M_max: the buffers hold them all, the count says so, the kernel reads the first M_max)
        det_id = torch.zeros(max(len(ids), M), device=dev, dtype=torch.int64)
        det_xy = torch.zeros((max(len(ids), M), 2), device=dev, dtype=torch.float64)
        det_id[:len(ids)] = torch.from_numpy(ids).to(dev)
        det_xy[:len(ids)] = torch.from_numpy(xy).to(dev)
        start = np.cumsum([0] + [0 if e is None else len(e[0]) for e in tick])
        det_start = torch.tensor(start, device=dev, dtype=torch.int32)
        pushed = torch.tensor([e is not None for e in tick], device=dev, dtype=torch.int32)
        when = torch.tensor([-5 if e is None else e[2] for e in tick], device=dev, dtype=torch.int64)
        obs = torch.full((n, T, V, 2), 7.0, device=dev, dtype=torch.float64)
        out_ids = torch.full((n, V), 7, device=dev, dtype=torch.int64)
        peds = torch.full((n,), 7, device=dev, dtype=torch.int32)
        seen = None if kind == "strict" else torch.full((n, V), 7, device=dev, dtype=torch.int32)
        out_flags = torch.full((n,), 7, device=dev, dtype=torch.int32)
        scale = frames._scale(4)
        sizes = {"strict": (S, T, scale, V), "rule": (S, T, scale, V) + RULE,
                 "timed": (S, R, T, scale, V, STEP, STEP) + RULE}[kind]
        name = {"strict": "stg_track_push%s", "rule": "stg_track_push%s_rule", "timed": "stg_track_push%s_timed"}[kind]
        t_arg = (ptr(when),) if kind == "timed" else ()
        s_arg = () if seen is None else (ptr(seen),)
        outs = (ptr(obs), ptr(out_ids), ptr(peds))
        if self.ns is None:
            count = det_start[1:2].contiguous()
            check(getattr(lib(), name % "")(ptr(det_id), ptr(det_xy), ptr(count), *t_arg, M, *map(ptr, self.state),
                                             *sizes, *outs, *s_arg, stream_ptr()), name % "")
            flags = self.head_flags[:, 1].cpu().numpy()
        else:
            name = name % "_streams"
            check(getattr(lib(), name)(ptr(det_id), 1, ptr(det_xy), 2, len(det_id), ptr(det_start), ptr(pushed), *t_arg,
                                       n, M, *map(ptr, self.state), *sizes, *outs, ptr(out_flags), *s_arg, self.block,
                                       stream_ptr()), name)
            flags = out_flags.cpu().numpy()
        table, out_ids, peds, obs = (x.cpu().numpy() for x in (self.slot_id, out_ids, peds, obs))
        seen = [None] * n if seen is None else seen.cpu().numpy()
        return [(table[b], int(flags[b]), out_ids[b], int(peds[b]), obs[b], seen[b]) for b in range(n)]


def _assert_empty(out, what):
    _, flags, ids, peds, obs, seen = out
    assert flags == 0 and peds == 0 and np.all(ids == -1) and not obs.any(), what
    assert seen is None or not seen.any(), what


def test_the_three_pushes_keep_one_slot_table(dev, want):
    feed, ref, _ = want
    pushes = [_Push(dev, kind) for kind in KINDS]
    placed = 0
    for f, (ids, xy) in enumerate(feed):
        got = [p.push([(ids, xy, STEP * f)])[0] for p in pushes]
        for kind, (table, flags, *_) in zip(KINDS, got):
            assert np.array_equal(table, got[0][0]), (kind, f)
            assert np.array_equal(table, ref[f][0]), (kind, f, np.nonzero(table != ref[f][0])[0][:8])
            assert flags & BITS == ref[f][1], (kind, f, flags, ref[f][1])
        placed += int((ref[f][0] >= 0).sum())
    assert placed > 1500


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_the_streams_pushes_keep_that_table_per_stream(dev, want, block):
    """Stream 0 is pushed every tick, stream 1 the feed's even pushes on the even ticks (its own clock: one step a
    push), stream 2 never."""
    feed, ref, ref_even = want
    for kind in KINDS:
        p = _Push(dev, kind, ns=3, block=block)
        for t, (ids, xy) in enumerate(feed):
            out = p.push([(ids, xy, STEP * t), (ids, xy, STEP * (t // 2)) if t % 2 == 0 else None, None])
            what = (kind, block, t)
            assert np.array_equal(out[0][0], ref[t][0]) and out[0][1] & BITS == ref[t][1], what
            assert np.array_equal(out[1][0], ref_even[t // 2][0]), what
            if t % 2 == 0:
                assert out[1][1] & BITS == ref_even[t // 2][1], what
            else:
                _assert_empty(out[1], what)
            _assert_empty(out[2], what)
        for x, x0 in zip(p.state, p.start):
            assert torch.equal(x[2], x0[2]), (kind, block)
