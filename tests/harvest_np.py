"""The window harvest restated in numpy (csrc/harvest.hip): the rule, the log with its capacities and
dropped_full, the tags, unpushed streams and reset.

    TrackModel   the strict track state of stg_track_push as the harvest reads it -- slot ids, presence masks, the
                 position ring, the head -- with the slot rule of push_slots_np.SlotModel; the GPU tests feed the
                 harvest the kernels' own state instead
    History      one stream's harvest history: a 32-bit word per slot, a T_all-deep float64 ring, {row, pushes}
    Log          the append-only log in DeviceWindows' layout, closed by its first drop
    Harvester    NS streams and one log: tick({stream: track state}) in stream order
    harvest_recording   a recording pushed frame by frame through TrackModel and Harvester
"""
import numpy as np

OVERFLOW = 2


class TrackModel:
    def __init__(self, t_obs, capacity, decimals=4):
        self.t_obs, self.full, self.decimals = t_obs, (1 << t_obs) - 1, decimals
        self.slot_id = np.full(capacity, -1, np.int64)
        self.mask = np.zeros(capacity, np.int64)
        self.ring = np.zeros((t_obs, capacity, 2))
        self.head = 0

    def push(self, ids, xy):
        """One frame of detections (no id twice); returns the push's flags (OVERFLOW: a new id found no slot)."""
        ids = [int(i) for i in ids]
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        xy = xy if self.decimals is None else np.around(xy, self.decimals)
        self.head = (self.head + 1) % self.t_obs
        self.mask = (self.mask << 1) & self.full                # age; a slot whose mask is 0 is free
        self.slot_id[self.mask == 0] = -1
        live = {int(i): s for s, i in enumerate(self.slot_id) if self.mask[s]}
        free = np.nonzero(self.mask == 0)[0].tolist()           # slot order
        flags = 0
        for j, i in enumerate(ids):                             # new ids take the free slots in detection order
            s = live.get(i)
            if s is None:
                if not free:
                    flags |= OVERFLOW
                    continue
                s = free.pop(0)
                self.slot_id[s] = i
            self.mask[s] |= 1
            self.ring[self.head, s] = xy[j]
        return flags

    def state(self):
        return self.slot_id, self.mask, self.ring, self.head


class History:
    def __init__(self, capacity, t_all):
        self.s, self.t_all, self.full = capacity, t_all, (1 << t_all) - 1
        self.word = np.zeros(capacity, np.int64)
        self.ring = np.zeros((t_all, capacity, 2))
        self.row, self.pushes = 0, 0

    def reset(self):
        self.word[:] = 0
        self.row, self.pushes = 0, 0

    def push(self, slot_id, mask, ring, head, min_peds):
        """Behind a push that left (slot_id, mask, ring, head): age, take presence and positions; returns the window's
        rows (c,2,T_all) float32 in ascending id order, or None when fewer than min_peds tracks are complete."""
        slot_id, mask = np.asarray(slot_id, np.int64), np.asarray(mask, np.int64) & 0xffffffff
        self.row = (self.row % self.t_all + 1) % self.t_all
        self.pushes += 1
        self.word = (self.word << 1) & self.full
        seen = (mask & 1) == 1
        self.word[seen] |= 1
        self.ring[self.row, seen] = np.asarray(ring)[head % ring.shape[0]][seen]
        self.word[slot_id < 0] = 0                              # a free slot has an empty word
        cand = np.nonzero(self.word == self.full)[0]
        if len(cand) < min_peds:
            return None
        cand = cand[np.argsort(slot_id[cand], kind="stable")]
        order = [(self.row + 1 + t) % self.t_all for t in range(self.t_all)]       # oldest first
        pos = np.transpose(self.ring[order][:, cand], (1, 2, 0))                   # (c, 2, T_all) float64
        rel = np.zeros_like(pos)
        rel[:, :, 1:] = pos[:, :, 1:] - pos[:, :, :-1]
        return rel.astype(np.float32)


class Log:
    def __init__(self, cap_windows, cap_rows, t_all):
        self.cap_windows, self.cap_rows = cap_windows, cap_rows
        self.rel_all = np.zeros((cap_rows, 2, t_all), np.float32)
        self.win_start = np.zeros(cap_windows + 1, np.int32)
        self.win_tag = np.zeros((cap_windows, 2), np.int32)
        self.header = np.zeros(3, np.int32)                     # n_windows, n_rows, dropped_full

    def clear(self):
        self.header[:] = 0

    def append(self, stream, push, rows):
        n_w, n_r, dropped = (int(x) for x in self.header)
        c = len(rows)
        if dropped or n_w >= self.cap_windows or n_r + c > self.cap_rows:       # the first drop closes the log
            self.header[2] += 1
            return False
        self.rel_all[n_r:n_r + c] = rows
        self.win_start[n_w + 1] = n_r + c
        self.win_tag[n_w] = (stream, push)
        self.header[:2] = (n_w + 1, n_r + c)
        return True

    @property
    def num_peds(self):
        return np.diff(self.win_start[:int(self.header[0]) + 1])

    @property
    def seq_rel(self):
        return self.rel_all[:int(self.header[1])]

    @property
    def tags(self):
        return self.win_tag[:int(self.header[0])]


class Harvester:
    def __init__(self, streams, capacity, t_all, cap_windows, cap_rows, min_peds=2):
        self.min_peds = min_peds
        self.hist = [History(capacity, t_all) for _ in range(streams)]
        self.log = Log(cap_windows, cap_rows, t_all)

    def tick(self, states):
        """states: {stream: (slot_id, mask, ring, head)} of the streams pushed this tick; the others do not age."""
        for b in sorted(states):
            h = self.hist[b]
            rows = h.push(*states[b], self.min_peds)
            if rows is not None:
                self.log.append(b, h.pushes - 1, rows)

    def reset(self, streams=None):
        for b in range(len(self.hist)) if streams is None else streams:
            self.hist[b].reset()


WIDE_S, WIDE_NS = 272, 2                 # more slots than the 256 threads of a harvest workgroup: a second pass over them


def wide_script(ticks=7, seed=7):
    """The feed of the GPU tests' second-pass case at WIDE_S slots: ticks x WIDE_NS entries (ids, xy) or None (not
    pushed).  Stream 0 holds 264 ids in every tick, shuffled, a negative one and one above 2^32 among them: they fill the
    slots 0 .. 263 in the first tick, so candidates sit past slot 255; from tick 2 on one more id per tick, each seen
    twice, takes the lowest free slot from 264 up (live, never complete) and the last slots stay free.  Stream 1 holds
    five ids and sits out tick 3."""
    gen = np.random.default_rng(seed)
    crowd = list(range(1, 263)) + [-5, (1 << 33) + 7]
    out = []
    for t in range(ticks):
        ids = crowd + [9000 + k for k in (t - 1, t) if k >= 2]
        ids = np.array(ids, np.int64)[gen.permutation(len(ids))]
        few = np.array([3, (1 << 33) + 8, 50, 51, 52], np.int64)[gen.permutation(5)]
        out.append([(ids, gen.uniform(-20, 20, size=(len(ids), 2))),
                    None if t == 3 else (few, gen.uniform(-20, 20, size=(5, 2)))])
    return out


def wide_ticks(script, t_obs=3, t_all=5, caps=(16, 1024), min_peds=2):
    """wide_script tick by tick through one TrackModel per stream and a Harvester: yields (the tick's entries, every
    stream's track state (slot_id, mask, ring, head) behind the tick -- the models' own arrays --, the Harvester behind
    the tick, the slots of stream 0's window or None)."""
    tracks = [TrackModel(t_obs, WIDE_S) for _ in range(WIDE_NS)]
    hv = Harvester(WIDE_NS, WIDE_S, t_all, *caps, min_peds)
    for tick in script:
        for b, d in enumerate(tick):
            if d is not None:
                assert tracks[b].push(*d) == 0
        hv.tick({b: tracks[b].state() for b, d in enumerate(tick) if d is not None})
        cand = np.nonzero(hv.hist[0].word == hv.hist[0].full)[0]
        yield tick, [tr.state() for tr in tracks], hv, cand if tick[0] is not None and len(cand) >= min_peds else None


def wide_conditions(slot_ids, words, full, windows):
    """What a second-pass feed has to reach, on the statement's own state: slot_ids / words per tick of one stream, full
    = the word of a complete track, windows = per tick the slots of the window's rows (or None).  At least one window,
    a row in a slot >= 256, and at some tick a live slot that is no candidate and a free slot, both past slot 255."""
    rows = [w for w in windows if w is not None]
    tail = [(np.asarray(i[256:]), np.asarray(w[256:])) for i, w in zip(slot_ids, words)]
    return (len(rows) >= 1 and any((np.asarray(w) >= 256).any() for w in rows) and
            any(((i >= 0) & (w != full)).any() and (i == -1).any() for i, w in tail))


def pushes_of(rows):
    """rows (M,4) <frame> <ped> <x> <y> -> [(ids int64, xy float64)] per distinct frame number, ascending, ids
    ascending within a frame."""
    rows = np.asarray(rows, np.float64)
    out = []
    for f in np.unique(rows[:, 0]):
        r = rows[rows[:, 0] == f]
        r = r[np.argsort(r[:, 1], kind="stable")]
        out.append((r[:, 1].astype(np.int64), r[:, 2:4].copy()))
    return out


def harvest_recording(rows, obs_len=8, pred_len=12, min_peds=2, capacity=256, cap_windows=4096, cap_rows=1 << 16):
    """A recording pushed frame by frame -> the Log."""
    track = TrackModel(obs_len, capacity)
    hv = Harvester(1, capacity, obs_len + pred_len, cap_windows, cap_rows, min_peds)
    for ids, xy in pushes_of(rows):
        assert track.push(ids, xy) == 0
        hv.tick({0: track.state()})
    return hv.log
