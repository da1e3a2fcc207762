"""The slot table of a live push, restated in numpy: which slot of the track state every pedestrian id occupies.  The
statements of the scenes (frames_np.StreamModel, frames_fill_np.StreamModelRule, frames_time_np.StreamModelTimed) keep
tracks by id and never say; the push kernels share one rule (csrc/track_rule.hpp: assign_slots), stated here on
(slot_id, presence mask).  A timed stream pushed once per step frees a slot exactly when the mask does."""
import numpy as np

DUPLICATE, OVERFLOW, TRUNCATED = 1, 2, 4


class SlotModel:
    def __init__(self, t_obs, capacity, max_detections):
        self.full, self.m_max = (1 << t_obs) - 1, max_detections
        self.slot_id = np.full(capacity, -1, np.int64)
        self.mask = np.zeros(capacity, np.int64)
        self.free, self.given = [], []  # the last push's free list, and (detection index, slot) of its placed new ids

    def push(self, ids):
        """-> (the slot table after the push, its DUPLICATE | OVERFLOW | TRUNCATED flags)."""
        ids = [int(i) for i in ids]
        flags = TRUNCATED if len(ids) > self.m_max else 0
        self.mask = (self.mask << 1) & self.full                # age; a slot whose mask is 0 is free
        self.slot_id[self.mask == 0] = -1
        first = {}
        for j, i in enumerate(ids[:self.m_max]):                # the first detection of an id wins
            flags |= DUPLICATE if i in first else 0
            first.setdefault(i, j)
        live = {int(i): s for s, i in enumerate(self.slot_id) if self.mask[s]}
        self.free = free = np.nonzero(self.mask == 0)[0].tolist()           # slot order
        new = sorted(j for i, j in first.items() if i not in live)          # detection order
        self.given = list(zip(new, free))
        flags |= OVERFLOW if len(new) > len(free) else 0
        for j, s in self.given:
            self.slot_id[s] = ids[j]
        for s in [live[i] for i in first if i in live] + [s for _, s in self.given]:
            self.mask[s] |= 1
        return self.slot_id.copy(), flags
