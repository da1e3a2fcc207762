"""The feed of tests/test_gpu_push_slots.py against the slot rule (tests/push_slots_np.py), without a GPU: what the
feed has to reach for the GPU test to mean something, so that a later edit of the feed cannot hollow it out."""
import numpy as np

from live_inputs import _slot_feed
from push_slots_np import DUPLICATE, OVERFLOW, TRUNCATED, SlotModel


def test_the_slot_feed_reaches_every_case_of_the_rule():
    feed = _slot_feed()
    assert len(feed) == 60 and max(len(p) for p, _ in feed) > 80 and all(xy.shape == (len(p), 2) for p, xy in feed)
    assert any(int(i) >> 32 for p, _ in feed for i in p)
    ref = SlotModel(3, 70, 80)
    n = dict(overflow=0, truncated=0, duplicate=0, plain=0, holes=0, late_detection=0, high_slot=0)
    for p, _ in feed:
        table, flags = ref.push(p)
        assert table.shape == (70,) and len(set(table[table >= 0].tolist())) == int((table >= 0).sum())
        n["overflow"] += bool(flags & OVERFLOW)
        n["truncated"] += bool(flags & TRUNCATED)
        n["duplicate"] += bool(flags & DUPLICATE)
        n["plain"] += flags == 0
        # at least two new ids meet a free list with a hole in it: the order of both lists matters
        n["holes"] += len(ref.given) >= 2 and bool(np.any(np.diff(ref.free) > 1))
        # a new detection of index >= 64 gets a slot: the second round of the block-wide rank at 64 threads
        n["late_detection"] += any(j >= 64 for j, _ in ref.given)
        n["high_slot"] += any(s >= 64 for _, s in ref.given)
    print(n)
    assert n["plain"] >= 10 and all(v >= 5 for v in n.values()), n
