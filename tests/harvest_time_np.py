"""The timed window harvest restated in numpy / Python (csrc/harvest_time.hip), keyed by pedestrian id
over "tracks as ascending sample lists": {id: [(t, x, y)]}, which is StreamModelTimed.state()[0] of frames_time_np or a
device state decoded through slot_head (decode_tracks).  It reuses frames_time_np.position_at and harvest_np.Log.

    TimedHistory     one stream: the grid {anchored, g0, j, skipped}, the ring row, and per id its run -- the positions
                     of its latest consecutive observed frames, at most T_all of them
    TimedHarvester   NS streams and one log: tick({stream: (tracks, t_now, accepted)}) in stream order
    decode_tracks    (slot_id, t_ring, xy_ring, slot_head) of one stream -> {id: samples}
    canonical        a device history in the form it is compared in: per live id (run length = trailing set bits of
                     the word, capped at T_all; the positions of those frames).  Bits of a word above its lowest zero are
                     not compared: a slot keeps them across a change of pedestrian, an id does not, and they cannot
                     reach a window.
    feed_recording   a recording pushed at given times through StreamModelTimed and a TimedHarvester
"""
import numpy as np

from frames_time_np import TIME_ORDER, StreamModelTimed, position_at
from harvest_np import Log, pushes_of

J_MAX = (1 << 31) - 1


class TimedHistory:
    def __init__(self, t_all, step, max_dt, settle, decimals=4):
        assert step >= 1 and 0 <= settle <= max_dt - 1
        self.t_all, self.step, self.max_dt, self.settle, self.decimals = t_all, int(step), int(max_dt), int(settle), decimals
        self.reset()
        self.interpolated = 0               # frames of candidates' runs that were interpolated (a test's precondition)

    def reset(self):
        self.runs = {}                      # id -> [(2,) positions], oldest first, the last one at the last frame
        self.lerped = {}                    # id -> [bool] beside runs: the frame was interpolated
        self.row, self.j = 0, 0
        self.anchored, self.g0, self.skipped = 0, 0, 0

    @property
    def head(self):
        return [self.row, self.j]

    @property
    def clock(self):
        return [self.anchored, self.g0, self.skipped]

    def push(self, tracks, t_now, min_peds):
        """Behind an ACCEPTED push at t_now that left `tracks`.  Returns (rows (c,2,T_all) float32 in ascending id order,
        the grid index of the frame) or None when no window is completed."""
        t_now = int(t_now)
        if not self.anchored:
            self.anchored, self.g0 = 1, t_now
        d = t_now - self.settle - self.g0
        n = 0 if d < 0 else d // self.step + 1
        k = n - self.j
        if k <= 0:
            return None
        if k >= 2:
            self.runs, self.lerped = {}, {}
            self.skipped += k - 1
        g = self.g0 + (n - 1) * self.step
        self.j = min(n, J_MAX)
        self.row = (self.row + 1) % self.t_all
        runs, lerped = {}, {}
        for key, samples in tracks.items():
            if key < 0:                                         # a negative id is a free slot to the harvest
                continue
            p = position_at(samples, g, self.max_dt, self.decimals)
            if p is None:
                runs[key], lerped[key] = [], []
            else:
                exact = any(t == g for t, _, _ in samples)
                runs[key] = (self.runs.get(key, []) + [p])[-self.t_all:]
                lerped[key] = (self.lerped.get(key, []) + [not exact])[-self.t_all:]
        self.runs, self.lerped = runs, lerped
        cand = sorted(key for key, r in runs.items() if len(r) == self.t_all)
        if len(cand) < min_peds:
            return None
        self.interpolated += sum(sum(lerped[key]) for key in cand)
        pos = np.transpose(np.array([runs[key] for key in cand], np.float64), (0, 2, 1))     # (c, 2, T_all)
        rel = np.zeros_like(pos)
        rel[:, :, 1:] = pos[:, :, 1:] - pos[:, :, :-1]
        return rel.astype(np.float32), self.j - 1


class TimedHarvester:
    def __init__(self, streams, t_all, step, max_dt, settle, cap_windows, cap_rows, min_peds=2, decimals=4):
        self.min_peds = min_peds
        self.hist = [TimedHistory(t_all, step, max_dt, settle, decimals) for _ in range(streams)]
        self.log = Log(cap_windows, cap_rows, t_all)

    def tick(self, states):
        """states: {stream: (tracks, t_now, accepted)} of the streams pushed this tick; a stream not pushed, or whose
        push was refused, keeps its history."""
        for b in sorted(states):
            tracks, t_now, accepted = states[b]
            if not accepted:
                continue
            got = self.hist[b].push(tracks, t_now, self.min_peds)
            if got is not None:
                self.log.append(b, got[1], got[0])

    def reset(self, streams=None):
        for b in range(len(self.hist)) if streams is None else streams:
            self.hist[b].reset()


def decode_tracks(slot_id, t_ring, xy_ring, slot_head):
    """One stream's timed track state as host arrays -> {id: [(t, x, y)] ascending} of the slots that hold a track."""
    out = {}
    r = t_ring.shape[1]
    for s, key in enumerate(np.asarray(slot_id).tolist()):
        h, c = int(slot_head[s, 0]), int(slot_head[s, 1])
        if c <= 0 or key == -1:
            continue
        idx = [(h - c + i) % r for i in range(c)]
        assert key not in out
        out[key] = [(int(t_ring[s, i]), float(xy_ring[s, i, 0]), float(xy_ring[s, i, 1])) for i in idx]
    return out


def canonical(slot_id, h_word, h_ring, h_head, t_all):
    """A device history -> {id: [(2,) positions] of its run, oldest first} for every slot with an id >= 0."""
    out = {}
    row = int(h_head[0])
    for s, key in enumerate(np.asarray(slot_id).tolist()):
        if key < 0:
            continue
        w, run = int(h_word[s]) & 0xffffffff, 0
        while run < t_all and (w >> run) & 1:
            run += 1
        out[key] = [h_ring[(row - back) % t_all, s].copy() for back in range(run - 1, -1, -1)]
    return out


def same_runs(got, want):
    """canonical(...) of a device history against TimedHistory.runs: the same ids (an id the statement does not hold has
    an empty run), run lengths and positions, bit for bit."""
    for key in set(got) | set(want):
        a, b = got.get(key, []), want.get(key, [])
        if len(a) != len(b) or any(np.asarray(x).tobytes() != np.asarray(y).tobytes() for x, y in zip(a, b)):
            return False
    return True


def feed(pushes, times, obs_len=8, pred_len=12, step=10, max_dt=None, settle=0, history=96, min_peds=2, capacity=256,
         cap_windows=4096, cap_rows=1 << 16):
    """pushes [(ids, xy)] at `times` through the timed track statement and the harvest -> (TimedHarvester, [the log's
    header after every push])."""
    max_dt = step if max_dt is None else max_dt
    track = StreamModelTimed(obs_len, step, max_dt, history, capacity=capacity)
    hv = TimedHarvester(1, obs_len + pred_len, step, max_dt, settle, cap_windows, cap_rows, min_peds)
    headers = []
    for (ids, xy), t in zip(pushes, times):
        flags = track.push(ids, xy, t)[3]
        hv.tick({0: (track.state()[0], t, not flags & TIME_ORDER)})
        headers.append(tuple(int(x) for x in hv.log.header))
    return hv, headers


def feed_recording(rows, **kw):
    """A recording pushed once per frame at t = 10 * (frame index)."""
    pushes = pushes_of(rows)
    return feed(pushes, [10 * f for f in range(len(pushes))], **kw)


def upsample(pushes, factor):
    """Frames [(ids, xy)] one step apart -> factor pushes per step: between two frames, an id present in both is linearly
    interpolated (in float64, then rounded to 4 decimals as a tracker's output would be), an id in the earlier frame only
    is not detected.  Returns the pushes; push i * factor is frame i unchanged."""
    out = []
    for f, (ids, xy) in enumerate(pushes):
        out.append((np.asarray(ids, np.int64), np.asarray(xy, np.float64)))
        if f + 1 == len(pushes):
            break
        nxt = {int(i): p for i, p in zip(*pushes[f + 1])}
        for m in range(1, factor):
            keep = [(int(i), np.around(p + (nxt[int(i)] - p) * (m / factor), 4)) for i, p in zip(ids, xy) if int(i) in nxt]
            out.append((np.array([i for i, _ in keep], np.int64), np.array([p for _, p in keep], np.float64).reshape(-1, 2)))
    return out


def eth_feed(frames60, offset=0, skip_at=120, empty_frame=45):
    """The GPU tests' recording feed: 60 frames [(ids, xy)] upsampled 4x, one push per tick, step = max_dt = 4 ticks.
    offset = 0: every push from the first on; the grid instants are the frames themselves.  offset in 1..3: the feed
    starts `offset` pushes in, between two frames, and to make the harvest interpolate, every later push ON a grid
    instant is left out; further the 9 pushes from `skip_at` on are left out (more than two steps: a skip), and the push that resolves the
    instant of frame `empty_frame` under settle = 0 is emptied (every track missed once: what settle is for).  Returns
    (pushes, times)."""
    up = upsample(frames60, 4)
    times = list(range(len(up)))
    if offset == 0:
        return up, times
    keep = [i for i in range(offset, len(up)) if (i - offset) % 4 != 0 or i == offset]
    keep = [i for i in keep if not skip_at <= i < skip_at + 9]
    pushes = [up[i] for i in keep]
    at = [n for n, i in enumerate(keep) if i == offset + 4 * empty_frame + 1][0]        # the push that resolves a grid instant
    pushes[at] = (np.zeros(0, np.int64), np.zeros((0, 2)))
    return pushes, [times[i] for i in keep]


NS = 3
CLOCK0 = (0, 1000, -500)                 # the streams' own clocks


def scripted_feed(t_obs, t_all, pushes, seed, step=10):
    """The C ABI test's feed: `pushes` ticks x NS entries (ids, xy, t) or None (not pushed).  Every stream on its own
    clock; inter-push times from {1, 2, 3, 4, 7} with one deliberate gap of 13 and one of 25; stream 1 skips every fourth
    tick; stream 2's push 20 goes back in time (refused).  Tracks move on lines with a little noise: long ones with a
    negative and a huge id, one with a gap wider than max_dt, one that vanishes, one that leaves for longer than a track
    lives and comes back (its slot is reused in between), a late one, a crowd that runs the 16 slots out, and single
    missed detections on three of them."""
    gen = np.random.default_rng(seed)
    w = t_all * step
    rel = [0] * NS                        # ticks since the stream's first push
    count = [0] * NS
    out = []
    for n in range(pushes):
        tick = []
        for s in range(NS):
            if s == 1 and n % 4 == 2:
                tick.append(None)
                continue
            count[s] += 1
            if count[s] > 1:
                rel[s] += 25 if count[s] == 9 else 13 if count[s] == 15 else int(gen.choice([1, 2, 3, 4, 7]))
            tt = rel[s]
            ids = [3, -5, (1 << 33) + 7 + s, 1000]
            if not w + 30 <= tt < w + 44:
                ids.append(11 + s)                               # a gap of 14 ticks or more
            if n < pushes * 2 // 3:
                ids.append(40)                                   # vanishes
            if tt < 60 or tt >= 60 + t_obs * step + 20:
                ids.append(77)                                   # leaves, comes back to another slot
            if 70 <= tt < 70 + (t_obs + 1) * step:
                ids.append(500 + (tt // 5) % 2)                  # short tracks that take the freed slot
            if tt >= 100:
                ids.append(2)                                    # late, the smallest id
            if w + 80 <= tt < w + 100:
                ids += list(range(200, 214))                     # the crowd: more ids than slots
            ids = [i for i in ids if i not in (11 + s, 40, 2) or gen.random() > 0.04]
            ids = np.array(ids, np.int64)[gen.permutation(len(ids))]
            base = np.stack([(ids % 17).astype(np.float64) - 8.0, (ids % 5).astype(np.float64)], 1)
            vel = np.stack([0.01 + (ids % 7) * 0.003, -0.02 + (ids % 3) * 0.011], 1)
            xy = base + vel * tt + gen.normal(0.0, 0.002, size=(len(ids), 2))
            t = CLOCK0[s] + tt
            if s == 2 and count[s] == 20:
                t -= 9                                           # back in time: refused, nothing recorded
            tick.append((ids, xy, t))
        out.append(tick)
    return out


WIDE_S, WIDE_NS = 272, 2                 # more slots than the 256 threads of a harvest workgroup: a second pass over them


def wide_feed(seed=7, step=10):
    """The feed of the GPU test's second-pass case at WIDE_S slots, rings of 4, T_obs 3, T_all 5, max_dt = step, settle 0:
    [WIDE_NS entries (ids, xy, t) or None].  A push every 5 ticks, the grid anchored at the first; stream 0 leaves out
    the pushes at 20, 40 and 60, so those instants are resolved 5 ticks late from the bracket around them (interpolated)
    and the instants 10, 30, 50 from a sample (exact).  Stream 0 holds 264 ids in every push, shuffled, a negative one
    and one above 2^32 among them: the slots 0 .. 263; from the third push on, every third push brings one more id, seen
    twice, that takes the lowest free slot from 264 up (live, never complete); the last slots stay free.  Stream 1, on
    its own clock, holds five ids, is pushed every time but once, and only ever sees exact frames."""
    gen = np.random.default_rng(seed)
    crowd = list(range(1, 263)) + [-5, (1 << 33) + 7]
    out = []
    for n, tt in enumerate(range(0, 70, 5)):
        ids = crowd + [9000 + k for k in (n - 1, n) if k >= 2 and k % 3 == 2]
        ids = np.array(ids, np.int64)[gen.permutation(len(ids))]
        few = np.array([3, (1 << 33) + 8, 50, 51, 52], np.int64)[gen.permutation(5)]
        tick = []
        for i, t0, skip in ((ids, 0, tt in (20, 40, 60)), (few, CLOCK0[1], tt == 35)):
            base = np.stack([(i % 17).astype(np.float64) - 8.0, (i % 5).astype(np.float64)], 1)
            vel = np.stack([0.01 + (i % 7) * 0.003, -0.02 + (i % 3) * 0.011], 1)
            tick.append(None if skip else (i, base + vel * tt + gen.normal(0.0, 0.002, size=(len(i), 2)), t0 + tt))
        out.append(tick)
    return out


def wide_facts(h, slot_of, t_all, window):
    """Stream 0 behind a tick of wide_feed: h its TimedHistory, slot_of {id: slot} of the tracks the state holds, window:
    did the tick append a window of it -> (a row of that window past slot 255, such a row with an interpolated frame, a
    live slot past 255 that is no candidate together with a free one)."""
    past = {k: s for k, s in slot_of.items() if s >= 256 and k >= 0}
    cand = [k for k in past if len(h.runs.get(k, [])) == t_all]
    free = WIDE_S - 256 - sum(s >= 256 for s in slot_of.values())
    return (window and bool(cand), window and any(any(h.lerped[k]) for k in cand), len(cand) < len(past) and free > 0)


def wide_reached(hv, facts):
    """What the second-pass feed has to reach: a window, and each of wide_facts at some tick."""
    return int(hv.log.header[0]) >= 1 and int(hv.log.header[2]) == 0 and all(any(f[i] for f in facts) for i in range(3))


def wide_run(feed, t_obs=3, t_all=5, r=4, step=10, max_dt=10, settle=0, caps=(16, 1024)):
    """wide_feed through the timed track statement and the harvest, the slots handed out as the push hands them out
    (a new id, in detection order, takes the lowest free slot; a forgotten track frees its own) -> (TimedHarvester,
    wide_facts per tick)."""
    tracks = [StreamModelTimed(t_obs, step, max_dt, r, max_peds=WIDE_S, capacity=WIDE_S) for _ in range(WIDE_NS)]
    hv = TimedHarvester(WIDE_NS, t_all, step, max_dt, settle, *caps)
    slot_of, facts = {}, []
    for tick in feed:
        states = {}
        for b, d in enumerate(tick):
            if d is not None:
                assert tracks[b].push(*d)[3] == 0
                states[b] = (tracks[b].state()[0], d[2], True)
        if 0 in states:
            slot_of = {k: s for k, s in slot_of.items() if k in states[0][0]}
            for k in tick[0][0].tolist():
                if k not in slot_of:
                    slot_of[k] = min(set(range(WIDE_S)) - set(slot_of.values()))
        before = int((hv.log.tags[:, 0] == 0).sum())
        hv.tick(states)
        facts.append(wide_facts(hv.hist[0], slot_of, t_all, int((hv.log.tags[:, 0] == 0).sum()) > before))
    return hv, facts


def run_scripted(feed, t_obs, t_all, max_dt, settle, history, caps=(4096, 1 << 16), step=10, capacity=16, min_peds=2):
    """The scripted feed through the timed track statement and the harvest -> (TimedHarvester, the OR of the flags)."""
    tracks = [StreamModelTimed(t_obs, step, max_dt, history, capacity=capacity) for _ in range(NS)]
    hv = TimedHarvester(NS, t_all, step, max_dt, settle, *caps, min_peds)
    seen = 0
    for tick in feed:
        states = {}
        for s, d in enumerate(tick):
            if d is not None:
                flags = tracks[s].push(d[0], d[1], d[2])[3]
                seen |= flags
                states[s] = (tracks[s].state()[0], d[2], not flags & TIME_ORDER)
        hv.tick(states)
    return hv, seen
