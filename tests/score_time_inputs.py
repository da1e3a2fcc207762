"""Inputs for the tests of the time-indexed score (test_score_time_cpu.py, test_gpu_score_time.py): the
exact-arithmetic scripts of irregular timed pushes and the pair of restatements that follow one stream -- the timed push
(frames_time_np.StreamModelTimed), whose track samples are the truth, and the score behind it
(score_time_np.TimedScoreModel).

Exact arithmetic, as in test_gpu_score.py: every pedestrian walks a line with coordinates in eighths, linear in the tick,
so a truth interpolated between two samples -- whatever the weight, dyadic or not -- is within 1e-15 of a multiple of
1/8 and the rounding to four decimals puts it there; predictions sit at Pythagorean offsets (in eighths) from where the
pedestrian will be, and v_pred's channels 2-4 are zero (C_h = h I).  Every err and best is then exact in float32, and
d2 and nll a few IEEE operations on exact operands."""
import numpy as np

import score_np
from frames_time_np import StreamModelTimed, TIME_ORDER
from score_time_np import TimedScoreModel

TRIPLES = np.array([(3, 4), (-5, 12), (8, -15), (-6, -8), (0, 5), (7, 24), (12, 0), (-20, 21)], np.float64)
BIG = 1 << 33                                          # ids above 2^32
STEP, MAX_DT, T_OBS, SLOTS, M_MAX = 4, 8, 8, 8, 16     # max_dt = 2 step: a bracket can hold two horizons of a record
FILLER = 1000                                          # ids from here on are never detected
EXTRA = (200, 201, 202, 203, 204, 205)                 # pushes 30-33: more ids than slots (OVERFLOW)
GAP_P = (0.22, 0.22, 0.2, 0.2, 0.12, 0.04)             # a gap of 13 > max_dt now and then: full trajectories exist


def pos(i, t):
    """Where pedestrian i is at tick t: multiples of 1/8, linear in t."""
    i = int(i % BIG)
    return np.array([(i % 7) * 24 + 2 * t - 40, (i % 5) * 16 - 3 * t + (i % 3)], np.float64) / 8.0


def exact_prediction(ids, t_r, p, v, k, step=STEP):
    """A prediction made at tick t_r for the scene `ids` (padded to v with -1; every column is a pedestrian when len(ids)
    == v): the mean and the samples at Pythagorean offsets from pos(i, t_r + h step)."""
    cols = np.full(v, -1, np.int64)
    cols[:len(ids)] = ids
    mean, samples = np.zeros((p, v, 2), np.float32), np.zeros((k, p, v, 2), np.float32)
    for j, i in enumerate(ids):
        for h in range(1, p + 1):
            at = pos(i, t_r + h * step)
            mean[h - 1, j] = at + TRIPLES[(int(i % BIG) + h + t_r) % 8] / 8.0
            for kk in range(k):
                samples[kk, h - 1, j] = at + (kk + 1) * TRIPLES[(int(i % BIG) + h + 2 * t_r + 3 * kk + 1) % 8] / 8.0
    v_pred = np.zeros((5, p, v), np.float32)
    v_pred[:2] = np.arange(2 * p * v, dtype=np.float32).reshape(2, p, v) / 8.0      # (not read by the score)
    return score_np.Prediction(cols, len(ids), mean, v_pred, samples if k else None)


def script(s, p, v, k, n_push=60):
    """Stream s: [(t, ids, xy, prediction, refused)].  Inter-push times from {1, 2, 3, 4, 7, 13} at step 4.  The
    branches: id 3 leaves at pushes 10-12 and returns (inside the horizon of P = 12, and mostly of P = 3); id 4 leaves at
    push 20 for good; push 15 repeats an id with another position (the first detection is the sample); push 25 is empty;
    pushes 30-33 carry six more ids than the 8 slots hold (OVERFLOW: the dropped ones are in the prediction and are not
    truth); before push 40 a push back in time (refused, nothing changes); ids above 2^32.  The scene of a prediction:
    the push's ids, last detection first, cut to v -- with v = 70 behind 64 ids that are never detected, so a lane owns
    two pedestrians and the second one is the one that is scored."""
    gen = np.random.default_rng(100 + s)
    times = (np.cumsum(gen.choice([1, 2, 3, 4, 7, 13], size=n_push, p=GAP_P)) - 50).tolist()
    base = [1, 2, 3, 4, BIG + 5, BIG + 6] if s != 1 else [BIG + 6, 2, 1, 3, 4]
    out = []
    for n, t in enumerate(times):
        ids = [i for i in base if not (i == 3 and 10 <= n <= 12) and not (i == 4 and n >= 20)]
        if 30 <= n <= 33:
            ids = ids + list(EXTRA)
        xy = [pos(i, t) for i in ids]
        if n == 15:
            ids, xy = ids + ids[:1], xy + [xy[0] + 1.0]
        if n == 25:
            ids, xy = [], []
        scene = list(dict.fromkeys(reversed(ids)))
        if v > 64:
            scene = [FILLER + j for j in range(64)] + scene
        scene = scene[:v - (n % 2 if v <= 64 else 0)]
        if n == 40:
            out.append((times[n - 1] - 2, np.array(ids, np.int64), np.array(xy).reshape(-1, 2),
                        exact_prediction(scene, t, p, v, k), True))
        out.append((t, np.array(ids, np.int64), np.array(xy, np.float64).reshape(-1, 2),
                    exact_prediction(scene, t, p, v, k), False))
    return out


def edge_script(s, p, v, k, empty_scenes=False, n_push=12):
    """Stream s, a dozen pushes (13 at the most) for the edge shapes: [(t, ids, xy, prediction)].  Inter-push times 1 to 7
    at step 4 (no bracket wider than max_dt), at most five ids (no OVERFLOW), id 3 away at pushes 4-5, push 8 empty.  The scene: the
    push's ids, last detection first; with v > 64 never-detected ids between them so that it fills all v columns and a
    detected id sits in the last one; with empty_scenes every other prediction holds no pedestrian."""
    times = (np.cumsum([3, 4, 1, 4, 2, 4, 7, 4, 3, 4, 1, 4, 3][:n_push]) - 20 + s).tolist()
    base = [1, 2, 3, 4, BIG + 5] if s != 1 else [BIG + 5, 2, 1, 3]
    out = []
    for n, t in enumerate(times):
        ids = [] if n == 8 else [i for i in base if not (i == 3 and n in (4, 5))]
        scene = list(dict.fromkeys(reversed(ids)))
        if v > 64:
            scene = scene[:-1] + [FILLER + j for j in range(v - len(scene))] + scene[-1:]
        if empty_scenes and n % 2:
            scene = []
        out.append((t, np.array(ids, np.int64), np.array([pos(i, t) for i in ids], np.float64).reshape(-1, 2),
                    exact_prediction(scene, t, p, v, k)))
    return out


def ring2_script(p, v, k, n_push=26):
    """One stream for rings of TWO samples: [(t, ids, xy, prediction)] at step 4.  A push is at (cell, phase), t = -20 +
    4 cell + phase, and moves on by at most one cell: inter-push times 1 to 7, no push passes two grid instants of the
    harvest (anchored at the first push), and every instant off a push lies in the bracket of the two samples a ring
    keeps -- behind a gap of 5 or 7 so does an earlier step of the push's own window.  Five ids, id 3 away at pushes
    4-5.  The scene of a prediction: the push's ids, last detection first."""
    moves = [(1, 0), (0, 3), (1, 2), (1, 3), (1, 0), (1, 3), (1, 1), (0, 2), (1, 0), (1, 1), (1, 3), (1, 2)]
    cell, times = 0, [-20]
    for n in range(n_push - 1):
        cell += moves[n % len(moves)][0]
        times.append(-20 + 4 * cell + moves[n % len(moves)][1])
    assert all(0 < b - a <= MAX_DT for a, b in zip(times, times[1:]))
    out = []
    for n, t in enumerate(times):
        ids = [i for i in (1, 2, 3, 4, BIG + 5) if not (i == 3 and n in (4, 5))]
        out.append((t, np.array(ids, np.int64), np.array([pos(i, t) for i in ids], np.float64).reshape(-1, 2),
                    exact_prediction(list(reversed(ids)), t, p, v, k)))
    return out


def interpolated_in_scene(scene, tracks, t, t_obs=T_OBS, step=STEP):
    """How many observed positions of a push's scene (StreamModelTimed.push's result) are at no sample's instant."""
    ids, _, seen, _ = scene
    return sum(1 for i, m in zip(ids.tolist(), seen.tolist()) for j in range(t_obs)
               if (m >> j) & 1 and not any(tt == t - j * step for tt, _, _ in tracks[i]))


def interpolated_in_records(rows, times, step=STEP):
    """How many matched entries of the records in a TimedScoreModel's ring were scored between two pushes: their instant
    t_r + h step is no push's time."""
    return sum(int(rec["matched"][h - 1].sum()) for rec in rows if rec is not None
               for h in range(1, rec["matched"].shape[0] + 1) if rec["t"] + h * step not in times)


class StreamRef:
    """One stream restated: the timed push and the score behind it."""

    def __init__(self, p, v, k, thr, pending, r, step=STEP, max_dt=MAX_DT, dtype=np.float32, decimals=4, slots=SLOTS,
                 t_obs=T_OBS, m_max=M_MAX, truth32=True):
        self.track = StreamModelTimed(t_obs, step, max_dt, r, 2, 3, v, decimals, slots, m_max)
        self.score = TimedScoreModel(p, v, k, step, max_dt, pending, thr, decimals, dtype, truth32)

    def push(self, t, ids, xy, pred):
        """-> (the push's flags, {push_totals, push_traj}); self.scene: what the push returned."""
        self.scene = self.track.push(ids, xy, t)
        flags = self.scene[3]
        return flags, self.score.push(self.track.tracks, t, pred, refused=bool(flags & TIME_ORDER))

    def idle(self):
        return self.score.push(self.track.tracks, 0, None)
