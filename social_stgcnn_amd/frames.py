"""Prediction frame by frame from raw tracks, offline (a whole recording) and live (one frame of detections per push).

The reference's windowing (utils.py:130-165) keeps a pedestrian only if they are tracked over all obs_len + pred_len
frames of a window, so it needs the future to decide whom to predict.  The rule here drops the future:

    frames    the recording's distinct frame numbers in ascending order (np.unique, utils.py:123); a stream push is one
    scene     at frame index f >= obs_len - 1: every pedestrian id with a row in each of the frames f-obs_len+1 .. f,
              ascending ids (np.unique, utils.py:133); a track with a gap comes back after obs_len consecutive frames
    obs_abs   float64 (obs_len, V_f, 2), oldest frame first, positions rounded as np.around(x, 4) (utils.py:145)

then the existing chain predict.observed_inputs -> model -> stg_sample_trajectories, fed float64 positions as
predict.sample_test feeds them.  The scenes are built by HIP kernels (csrc/frames.hip): stg_frame_scene_counts /
stg_frame_scenes over a recording uploaded once, stg_track_push with the track state kept on the device.

    recording_scenes   (M,4) rows of data.read_file -> FrameScenes on the device
    predict_recording  Predictor over the frame scenes in batches
    FramePredictor     push(ids, xy) per frame, eager or as ONE captured graph (capture())
    StreamsPredictor   NS independent live streams: push(tick) per tick, one host->device copy of the packed
                       detections and ONE launch chain (stg_track_push_streams -> the batched forward -> sampler)
    TrackRule          tracks=TrackRule(min_seen, max_gap) on any of the four: pedestrians with a short history or
                       tracker gaps are predicted too, their missed frames filled by the kernels
    fill_tracks        the fill alone, on a batch of scenes in place (stg_fill_tracks)
    TimedScoreSpec     score=TimedScoreSpec(levels, best_of_k, pending) on the two live predictors together with time=:
                       records indexed by time, truth interpolated as the timed push interpolates (stg_score_push_timed,
                       DESIGN.md 5.25); `.score`, `.score_totals`, `.score_records`, `.score_evictions`
    ScoreSpec          score=ScoreSpec(levels, best_of_k) on the two live predictors: every push also scores the
                       predictions of the last pred_seq_len pushes against its detections (stg_score_push, DESIGN.md
                       5.17); `.score`, `.score_totals`, and score_summary for host numbers
    TimeRule           time=TimeRule(step, max_dt, history) on the two live predictors: pushes carry their time in
                       integer ticks and arrive at the tracker's own rate; every push predicts from the scene "as of
                       now", the tracks resampled at t - k * step on the device (stg_track_push_timed)
    AssociateSpec      associate=AssociateSpec(gate, gate_new, max_miss) on the two live predictors: pushes carry
                       positions only, push(None, xy); a launch ahead of the push kernel gives every detection its track
                       id on the device (stg_associate); `.det_ids`, `.assoc_flags`
    TimedAssociateSpec associate=TimedAssociateSpec(gate, gate_new, max_age) together with time=: the association at the
                       tracker's own rate, push(None, xy, t=TICKS); a track keeps the time of its last match and its
                       velocity per model step (stg_associate_timed ahead of the timed push)
    FilteredAssociateSpec  associate=FilteredAssociateSpec(sigma_det, sigma_acc, ...) together with time=: the timed
                       association for NOISY detections; a track keeps a constant-velocity Kalman state and its gate
                       follows the predicted uncertainty (stg_associate_filtered); `.assoc_tracks()`
    TimedHarvestSpec   harvest=TimedHarvestSpec(windows, rows, min_peds, pred_len, settle) together with time=: the
                       harvest of HarvestSpec on the timed tracks resampled on the step grid (stg_window_harvest_timed,
                       DESIGN.md 5.27)
    HarvestSpec        harvest=HarvestSpec(windows, rows, min_peds, pred_len) on the two live predictors: a launch behind
                       the push kernel keeps every training window the tracks complete -- a track seen in each of the
                       last obs_len + pred_len pushes is one row of a reference TrajectoryDataset window -- in a log on
                       the device (stg_window_harvest); `.harvest` is the LiveWindows, whose snapshot()
                       is a dataset.DeviceWindows for train.fine_tune

The two live predictors are one core, _LivePredictor: the argument checks (which spec goes with time= is one table,
_OPTIONS), the eager push and its capture (the launches ahead of predict.Predictor.capture_chain and the score behind it;
the capture recipe itself is graphs.py).  What launches around the model is a _Stage each -- _Association, _Tracks,
_Harvest, _Score.  Each class keeps what is its own: how a push is staged, what differs between one stream
and many (its _Feed), its result tuple, which streams its reset names, and how the warm-up is kept from moving the tracks.
"""
import collections
import collections.abc
import ctypes
import functools

import numpy as np
import torch

from . import ops
from ._lib import Bound, call, peds_arg, ptr, require_gpu, seed_i64
from .predict import Prediction, Predictor, ScoreSpec, TimedScoreSpec, eval_mode

MAX_OBS_LEN = 32                       # presence masks are 32-bit
MAX_DETECTIONS = 2048                  # STG_TRACK_MAX_DETECTIONS
MAX_SLOTS = 2048                       # STG_TRACK_MAX_SLOTS
MAX_STREAMS = 4096                     # STG_TRACK_MAX_STREAMS
MAX_TOTAL_DETECTIONS = MAX_STREAMS * MAX_DETECTIONS      # STG_TRACK_MAX_TOTAL_DETECTIONS
MAX_HISTORY = 256                      # STG_TRACK_MAX_HISTORY
STREAM_THREADS = 256                   # stg_track_push_streams' default workgroup (kStreamThreads, csrc/frames.hip)
# FramePrediction.flags bits (STG_TRACK_* in include/stgcnn_hip.h)
DUPLICATE, OVERFLOW, TRUNCATED, TOO_MANY, TIME_ORDER = 1, 2, 4, 8, 16

FrameScenes = collections.namedtuple("FrameScenes", "frame obs_abs ids num_peds")
FrameScenes.__doc__ = """frame (N,) float64 numpy: the frame numbers of the scenes; on the device: obs_abs (N,T_obs,V,2)
float64, ids (N,V) int64 (-1 in padded slots), num_peds (N,) int32.  Padded slots are zeros."""

PartialScenes = collections.namedtuple("PartialScenes", "frame obs_abs ids num_peds seen")
PartialScenes.__doc__ = """FrameScenes under a TrackRule, and seen (N,V) int32 on the device: bit t set = the pedestrian
was observed t frames ago (bit 0: this frame), 0 in padded slots.  The steps whose bit is clear are filled."""


class TrackRule(collections.namedtuple("TrackRule", "min_seen max_gap")):
    """Whom a frame scene holds when tracks are partial.  The window of a frame is its last obs_len frames (frames
    before the first count as missed).  A pedestrian is in the scene iff seen in this frame, seen in at least min_seen
    frames of the window (2 <= min_seen <= obs_len), and no run of missed frames between two seen ones is longer than
    max_gap (0 <= max_gap <= obs_len - 2; missed frames ahead of the first seen one are no gap).  Missed frames are
    filled in float64: between two seen frames by linear interpolation, ahead of the first seen one at the constant
    velocity of the first two frames of the interpolated window; every filled position is rounded like an observed one.
    TrackRule(obs_len, 0) is the strict rule.  Scenes start at frame index min_seen - 1."""
    __slots__ = ()

    def __new__(cls, min_seen, max_gap=0):
        if not _is_int(min_seen, 2, MAX_OBS_LEN):
            raise ValueError("TrackRule: min_seen must be an integer in [2, obs_len <= %d], got %r"
                             % (MAX_OBS_LEN, min_seen))
        if not _is_int(max_gap, 0, MAX_OBS_LEN - 2):
            raise ValueError("TrackRule: max_gap must be an integer in [0, obs_len - 2 <= %d], got %r"
                             % (MAX_OBS_LEN - 2, max_gap))
        return super().__new__(cls, int(min_seen), int(max_gap))

    def checked(self, obs_len):
        """The rule, once it fits a window of obs_len frames."""
        if self.min_seen > obs_len:
            raise ValueError("TrackRule: min_seen=%d > obs_len=%d" % (self.min_seen, obs_len))
        if self.max_gap > obs_len - 2:
            raise ValueError("TrackRule: max_gap=%d > obs_len - 2 = %d (a slot is freed after obs_len - 1 missed "
                             "frames)" % (self.max_gap, obs_len - 2))
        return self


def _rule(tracks, obs_len):
    """tracks (None, a TrackRule or a (min_seen, max_gap) pair) -> None or the TrackRule checked against obs_len."""
    if tracks is None:
        return None
    return (tracks if isinstance(tracks, TrackRule) else TrackRule(*tracks)).checked(obs_len)


class TimeRule(collections.namedtuple("TimeRule", "step max_dt history")):
    """Live pushes with time.  Time is integer ticks (the recording's frame number, microseconds, whatever the caller's
    clock counts); `step` is the model's step in ticks (10 for the ETH/UCY recordings: frame numbers 10 apart).  A push
    at time t predicts from the positions at t - k * step, k = 0 .. obs_len - 1: a sample recorded at exactly that
    instant, else the linear interpolation (float64, rounded like an observed position) of the two samples next to it
    when they are at most max_dt ticks apart (default: step; 1 <= max_dt <= (obs_len - 1) * step); an instant with
    neither is a missed step under the predictor's TrackRule (TrackRule(obs_len, 0) without tracks=).  Every track keeps
    its newest `history` samples (2 .. 256) and lives while its newest one is at most (obs_len - 1) * step old.  A push
    whose time is not after the stream's last one changes nothing and returns the empty scene, flag TIME_ORDER."""
    __slots__ = ()

    def __new__(cls, step, max_dt=None, history=96):
        if not _is_int(step, 1, (1 << 31) - 1):
            raise ValueError("TimeRule: step must be an integer number of ticks in [1, 2^31), got %r" % (step,))
        if max_dt is not None and not _is_int(max_dt, 1, (1 << 31) - 1):
            raise ValueError("TimeRule: max_dt must be None or an integer in [1, (obs_len - 1) * step], got %r"
                             % (max_dt,))
        if not _is_int(history, 2, MAX_HISTORY):
            raise ValueError("TimeRule: history must be an integer in [2, %d], got %r" % (MAX_HISTORY, history))
        return super().__new__(cls, int(step), None if max_dt is None else int(max_dt), int(history))

    def checked(self, obs_len):
        """The rule with max_dt resolved, once it fits a window of obs_len steps."""
        if obs_len < 2:
            raise ValueError("TimeRule: obs_len=%d (a timed window has at least 2 steps)" % obs_len)
        if self.step * obs_len >= 1 << 31:
            raise ValueError("TimeRule: step=%d: step * obs_len must stay below 2^31" % self.step)
        max_dt = self.step if self.max_dt is None else self.max_dt
        if max_dt > (obs_len - 1) * self.step:
            raise ValueError("TimeRule: max_dt=%d > (obs_len - 1) * step = %d (a track is forgotten by then)"
                             % (max_dt, (obs_len - 1) * self.step))
        return TimeRule(self.step, max_dt, self.history)


ASSOC_FULL = 1                         # STG_ASSOC_FULL, a bit of `.assoc_flags`
ASSOC_TIME_ORDER = 2                   # STG_ASSOC_TIME_ORDER (only under a TimedAssociateSpec or FilteredAssociateSpec)


class AssociateSpec(collections.namedtuple("AssociateSpec", "gate gate_new max_miss capacity")):
    """Live pushes without identities: a detector gives positions, the device gives them track ids.
    Per stream a tracker with constant-velocity prediction and gated, globally greedy nearest-neighbour matching: a
    track predicts pos + vel * (pushes since its last match + 1); a detection within `gate` of that (within gate_new,
    default 2 * gate, of a track seen once, which has no velocity yet) is a candidate; the candidates are taken nearest
    first, each track and each detection once.  A track not matched for more than max_miss pushes is forgotten; a
    detection not matched starts a track with a fresh id (0, 1, ... per stream).  `capacity` track slots (default: the
    predictor's capacity); past them a new detection still gets its id but is not remembered (flag ASSOC_FULL).  The
    distances are in the units of the positions, per push."""
    __slots__ = ()

    def __new__(cls, gate, gate_new=None, max_miss=0, capacity=None):
        def number(x, what):
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
                raise ValueError("AssociateSpec: %s must be a finite number, got %r" % (what, x))
            return float(x)
        gate = number(gate, "gate")
        gate_new = 2.0 * gate if gate_new is None else number(gate_new, "gate_new")
        if not gate > 0.0:
            raise ValueError("AssociateSpec: gate must be > 0, got %r" % (gate,))
        if not gate_new >= gate:
            raise ValueError("AssociateSpec: gate_new=%r must be >= gate=%r" % (gate_new, gate))
        if not np.isfinite(gate * gate) or not np.isfinite(gate_new * gate_new) or not gate * gate > 0.0:
            raise ValueError("AssociateSpec: the squared gates must be finite and > 0, got %r, %r" % (gate, gate_new))
        if not _is_int(max_miss, 0, (1 << 31) - 2):
            raise ValueError("AssociateSpec: max_miss must be an integer >= 0, got %r" % (max_miss,))
        return super().__new__(cls, gate, gate_new, int(max_miss), _capacity(capacity, "AssociateSpec"))


class TimedAssociateSpec(collections.namedtuple("TimedAssociateSpec", "gate gate_new max_age capacity")):
    """AssociateSpec for live pushes with time (time=TimeRule(...)): positions without ids, timestamped,
    at the detector's own rate.  The rule is AssociateSpec's with time in the place of the push count: a track keeps the
    time of its last match and its velocity per model step, and predicts pos + vel * (t - that time) / step; a matched
    detection gives vel = (p - pos) / the same quotient.  gate and gate_new (default 2 * gate) are the caller's
    distances whatever the gap, as AssociateSpec's are whatever the misses.  A track not matched is forgotten once its
    last match is more than max_age ticks old (default 0: by the first push that does not match it; max_miss * step is
    AssociateSpec's lifetime).  capacity as in AssociateSpec.  A push whose time is not after the stream's last accepted
    one changes nothing: its ids are -1 and `.assoc_flags` is ASSOC_TIME_ORDER (the timed push behind it refuses it too).
    Fed one push per step it gives AssociateSpec's ids, positions, velocities and hits bit for bit."""
    __slots__ = ()

    def __new__(cls, gate, gate_new=None, max_age=None, capacity=None):
        try:
            base = AssociateSpec(gate, gate_new, 0, capacity)
        except ValueError as e:
            raise ValueError("Timed" + str(e)) from None
        return super().__new__(cls, base.gate, base.gate_new, _max_age(max_age, "TimedAssociateSpec"), base.capacity)


class FilteredAssociateSpec(collections.namedtuple(
        "FilteredAssociateSpec", "sigma_det sigma_acc sigma_vel0 gate_sigmas gate_max max_age capacity")):
    """TimedAssociateSpec for NOISY detections (only together with time=TimeRule(...)): a track keeps a
    constant-velocity Kalman state -- the filtered position, the filtered velocity per model step and their covariance
    -- in the place of the last detection and a two-sample velocity, which amplifies the detector's noise by the number
    of pushes per step.  sigma_det: the detector's noise per axis (m); sigma_acc: the walker's random acceleration (m per
    step^1.5; 0: straight walkers); sigma_vel0: how uncertain a new track's velocity is (m per step).  A track reaches the
    detections within gate_sigmas standard deviations of its predicted position -- the gate grows with the gap since
    the last match and with a young track's unknown velocity -- and never further than gate_max (m).  The matching
    itself, max_age, capacity, the refused push (ids -1, ASSOC_TIME_ORDER) and everything behind the ids are
    TimedAssociateSpec's; the scene still holds what the detector reported, `.assoc_tracks()` the smoothed state."""
    __slots__ = ()

    def __new__(cls, sigma_det, sigma_acc, sigma_vel0=1.5, gate_sigmas=5.0, gate_max=2.0, max_age=0, capacity=None):
        vals = {"sigma_det": sigma_det, "sigma_acc": sigma_acc, "sigma_vel0": sigma_vel0, "gate_sigmas": gate_sigmas,
                "gate_max": gate_max}
        for name, x in vals.items():
            low = name == "sigma_acc"
            if not _is_number(x) or not (x >= 0 if low else x > 0):
                raise ValueError("FilteredAssociateSpec: %s must be a finite number %s 0, got %r"
                                 % (name, ">=" if low else ">", x))
            sq = float(x) * float(x)
            if not np.isfinite(sq) or (sq == 0.0 and not low):
                raise ValueError("FilteredAssociateSpec: the squared %s must be finite and > 0 in float64, got %r"
                                 % (name, x))
        return super().__new__(cls, *(float(x) for x in vals.values()), _max_age(max_age, "FilteredAssociateSpec"),
                               _capacity(capacity, "FilteredAssociateSpec"))


_TIMED_ASSOC = (TimedAssociateSpec, FilteredAssociateSpec)     # the association specs that go with time= only


MAX_WINDOW_STEPS = 32                  # STG_HARVEST_MAX_STEPS: a harvest word is 32 bits


class HarvestSpec(collections.namedtuple("HarvestSpec", "windows rows min_peds pred_len")):
    """Live pushes that also keep the training windows they complete: a track really detected in each
    of the last obs_len + pred_len pushes is one row of a reference TrajectoryDataset window, and min_peds or more of
    them (default 2: the reference's len > min_ped with min_ped = 1), in ascending id order, are one window, appended to
    a log on the device that holds up to `windows` windows and `rows` rows (default windows * max_peds).  pred_len
    defaults to the model's pred_seq_len.  The first window that does not fit closes the log until clear()."""
    __slots__ = ()

    def __new__(cls, windows, rows=None, min_peds=2, pred_len=None):
        if not _is_int(windows, 1, (1 << 31) - 2):
            raise ValueError("HarvestSpec: windows must be an integer in [1, 2^31 - 2], got %r" % (windows,))
        if rows is not None and not _is_int(rows, 1, (1 << 31) - 1):
            raise ValueError("HarvestSpec: rows must be None or an integer in [1, 2^31), got %r" % (rows,))
        if not _is_int(min_peds, 1, MAX_SLOTS):
            raise ValueError("HarvestSpec: min_peds must be an integer in [1, %d], got %r" % (MAX_SLOTS, min_peds))
        if pred_len is not None and not _is_int(pred_len, 1, MAX_WINDOW_STEPS - 1):
            raise ValueError("HarvestSpec: pred_len must be None or an integer in [1, %d], got %r"
                             % (MAX_WINDOW_STEPS - 1, pred_len))
        return super().__new__(cls, int(windows), None if rows is None else int(rows), int(min_peds),
                               None if pred_len is None else int(pred_len))

    def checked(self, obs_len, max_peds, pred_seq_len):
        """The spec with rows and pred_len resolved, once it fits a predictor of obs_len observed steps."""
        pred_len = int(pred_seq_len) if self.pred_len is None else self.pred_len
        if obs_len < 2:
            raise ValueError("HarvestSpec: obs_len=%d: the track state frees a slot after obs_len - 1 missed pushes, so "
                             "with one observed step a slot changes its pedestrian without a gap" % obs_len)
        if not 1 <= pred_len or obs_len + pred_len > MAX_WINDOW_STEPS:
            raise ValueError("HarvestSpec: obs_len + pred_len = %d + %d must stay within %d steps"
                             % (obs_len, pred_len, MAX_WINDOW_STEPS))
        rows = self.windows * int(max_peds) if self.rows is None else self.rows
        if rows >= 1 << 31:
            raise ValueError("HarvestSpec: rows=%d must stay below 2^31" % rows)
        return HarvestSpec(self.windows, rows, self.min_peds, pred_len)


class TimedHarvestSpec(collections.namedtuple("TimedHarvestSpec", "windows rows min_peds pred_len settle")):
    """HarvestSpec for live pushes with time (time=TimeRule(...)): the tracks are resampled on the
    model's step grid g0 + i * step, g0 the time of the stream's first accepted push, and every resolved grid instant
    is one frame of a HarvestSpec's harvest -- a track observed at it under the TimeRule's own test (a sample at the
    instant, or the interpolation of two samples next to it at most max_dt apart), detected in that very push or not.
    windows, rows, min_peds and pred_len as in HarvestSpec.  settle, 0 <= settle <= max_dt - 1 ticks (default max_dt -
    1), is how long an instant waits before it is resolved: at max_dt - 1 every bracket the rule allows around it has
    arrived, so a missed detection costs the track nothing; at 0 an instant is resolved by the first push at or after
    it.  A push more than a step after the last one skips the instants in between and ends every run of frames.  The
    TimeRule's history must still hold the sample at or before an instant when it is resolved: the samples of settle +
    max_dt ticks plus one push interval; a shallower one makes the frame a gap, never a wrong position."""
    __slots__ = ()

    def __new__(cls, windows, rows=None, min_peds=2, pred_len=None, settle=None):
        try:
            base = HarvestSpec(windows, rows, min_peds, pred_len)
        except ValueError as e:
            raise ValueError("Timed" + str(e)) from None
        if settle is not None and not _is_int(settle, 0, (1 << 31) - 2):
            raise ValueError("TimedHarvestSpec: settle must be None or an integer in [0, max_dt - 1], got %r" % (settle,))
        return super().__new__(cls, *base, None if settle is None else int(settle))

    def checked(self, obs_len, max_peds, pred_seq_len, max_dt):
        """The spec with rows, pred_len and settle resolved, once it fits a predictor of obs_len observed steps under a
        TimeRule with that max_dt."""
        try:
            base = HarvestSpec(*self[:4]).checked(obs_len, max_peds, pred_seq_len)
        except ValueError as e:
            raise ValueError("Timed" + str(e)) from None
        settle = max_dt - 1 if self.settle is None else self.settle
        if settle > max_dt - 1:
            raise ValueError("TimedHarvestSpec: settle=%d > max_dt - 1 = %d (no bracket is wider than max_dt)"
                             % (settle, max_dt - 1))
        return TimedHarvestSpec(*base, settle)


class LiveWindows:
    """The windows a harvesting predictor has kept, on the device in dataset.DeviceWindows' own layout: rel_all float32
    (rows,2,T_all), win_start int32 (windows+1,), win_tag int32 (windows,2) = (stream, that stream's push index since
    its reset; under a TimedHarvestSpec the grid index of the window's last frame) and header int32 (3,) = {n_windows, n_rows, dropped_full}.  Append-only: pushes write behind what is
    there, the first window that does not fit is counted in dropped_full and closes the log, clear() empties it."""

    def __init__(self, spec, t_obs, device):
        self.t_obs, self.t_all = int(t_obs), int(t_obs) + spec.pred_len
        self.cap_windows, self.cap_rows = spec.windows, spec.rows
        self.rel_all = torch.zeros((spec.rows, 2, self.t_all), device=device, dtype=torch.float32)
        self.win_start = torch.zeros(spec.windows + 1, device=device, dtype=torch.int32)
        self.win_tag = torch.zeros((spec.windows, 2), device=device, dtype=torch.int32)
        self.header = torch.zeros(3, device=device, dtype=torch.int32)

    def _args(self):
        """the log as the harvest entry points take it"""
        return dict(rel_all=ptr(self.rel_all), win_start=ptr(self.win_start), win_tag=ptr(self.win_tag),
                    header=ptr(self.header), cap_windows=self.cap_windows, cap_rows=self.cap_rows)

    def counts(self):
        """(n_windows, n_rows, dropped_full) as of the pushes enqueued so far: one synchronisation."""
        return tuple(int(x) for x in self.header.cpu().tolist())

    def snapshot(self):
        """The windows kept so far as a dataset.DeviceWindows that views the log's first n_rows rows and n_windows + 1
        offsets without copying (one synchronisation: the header and the offsets come back in one copy).  It stays
        valid until clear(): later pushes only append behind it.  Raises while the log is empty."""
        from .dataset import DeviceWindows
        host = torch.cat((self.header, self.win_start)).cpu().numpy()
        n_w, n_r = int(host[0]), int(host[1])
        if n_w < 1:
            raise ValueError("LiveWindows.snapshot: no window has been harvested yet")
        start = host[3:3 + n_w + 1]
        return DeviceWindows.from_device(self.rel_all[:n_r], self.win_start[:n_w + 1], np.diff(start), self.t_obs)

    def tags(self):
        """(n_windows, 2) int32 numpy: (stream, the stream's push index since its reset) of every window kept; one
        synchronisation."""
        host = torch.cat((self.header, self.win_tag.reshape(-1))).cpu().numpy()
        return host[3:3 + 2 * int(host[0])].reshape(-1, 2).copy()

    def clear(self):
        """Empty the log (the streams' histories go on: the next window is the first of the new log)."""
        self.header.zero_()


def _tick_time(t, what):
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) or not -(1 << 62) <= int(t) < 1 << 62:
        raise ValueError("%s: the time must be an integer number of ticks (|t| < 2^62), got %r" % (what, t))
    return int(t)


FramePrediction = collections.namedtuple("FramePrediction", "ids num_peds obs_abs samples mean v_pred flags")
FramePrediction.__doc__ = """One push, on the device: ids (V,) int64 (-1 in padded slots), num_peds (1,) int32,
obs_abs (1,T_obs,V,2) float64, samples (K,P,V,2), mean (P,V,2), v_pred (5,P,V) float32, flags (1,) int32 (DUPLICATE |
OVERFLOW | TRUNCATED | TOO_MANY | TIME_ORDER of this push).  From a captured push the tensors are the graph's static
buffers, overwritten by the next push."""


def _is_number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating)) and bool(np.isfinite(x))


def _is_int(x, lo, hi=None):
    """x is an integer (a bool is not) with lo <= x (<= hi)."""
    return not isinstance(x, bool) and int(x) == x and lo <= int(x) and (hi is None or int(x) <= hi)


def _max_age(max_age, what):
    """The max_age of the association specs that age their tracks by time (None: 0)."""
    max_age = 0 if max_age is None else max_age
    if not _is_number(max_age) or not _is_int(max_age, 0, (1 << 31) - 1):
        raise ValueError("%s: max_age must be an integer number of ticks in [0, 2^31), got %r" % (what, max_age))
    return int(max_age)


def _capacity(capacity, what):
    """The capacity of an association spec: None (the predictor's), or a number of track slots."""
    if capacity is not None and (not _is_number(capacity) or not _is_int(capacity, 1, MAX_SLOTS)):
        raise ValueError("%s: capacity must be None or an integer in [1, %d], got %r" % (what, MAX_SLOTS, capacity))
    return None if capacity is None else int(capacity)


def _stream_index(key, streams, what):
    if isinstance(key, (bool, np.bool_)) or not isinstance(key, (int, np.integer)) or not 0 <= key < streams:
        raise ValueError("%s: stream index %r not in [0, %d)" % (what, key, streams))


def _obs_len(obs_len):
    if not _is_int(obs_len, 1, MAX_OBS_LEN):
        raise ValueError("obs_len must be an integer in [1, %d], got %r" % (MAX_OBS_LEN, obs_len))
    return int(obs_len)


def _scale(decimals):
    """np.around's 10^decimals (0.0: no rounding)."""
    if decimals is None:
        return 0.0
    if not _is_int(decimals, 0, 15):
        raise ValueError("decimals must be None or an integer in [0, 15], got %r" % (decimals,))
    return float(10 ** int(decimals))


def _integral_ids(ids, what):
    ids = np.asarray(ids)
    if ids.dtype.kind in "iu":
        out = ids.astype(np.int64)
    else:
        f = ids.astype(np.float64)
        if not np.all(np.isfinite(f)) or np.any(f != np.round(f)):
            raise ValueError("%s: pedestrian ids must be integral" % what)
        out = f.astype(np.int64)
    if np.any(out < 0):
        raise ValueError("%s: pedestrian ids must be >= 0 (-1 marks a padded slot)" % what)
    return out


def sorted_rows(rows):
    """(M,4) rows <frame> <ped> <x> <y> -> (frames (F,) float64, frame_start (F+1,) int32, ids (M,) int64,
    xy (M,2) float64): the rows sorted by (frame index, id).  A duplicated (frame, id) row is refused, as
    data.load_windows refuses it."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] < 4:
        raise ValueError("rows (M,4) <frame> <ped> <x> <y> expected, got shape %s" % (rows.shape,))
    if rows.shape[0] >= 1 << 31:
        raise ValueError("recording too long (%d rows)" % rows.shape[0])
    ids = _integral_ids(rows[:, 1], "recording")
    frames = np.unique(rows[:, 0])
    f_idx = np.searchsorted(frames, rows[:, 0])
    order = np.lexsort((ids, f_idx))
    f_s, id_s = f_idx[order], ids[order]
    dup = np.nonzero((f_s[1:] == f_s[:-1]) & (id_s[1:] == id_s[:-1]))[0]
    if len(dup):
        raise ValueError("duplicate row for pedestrian %d in frame %r" % (id_s[dup[0]], frames[f_s[dup[0]]]))
    frame_start = np.searchsorted(f_s, np.arange(len(frames) + 1)).astype(np.int32)
    return frames, frame_start, id_s, np.ascontiguousarray(rows[order, 2:4])


def recording_scenes(rows, device, obs_len=8, min_peds=1, decimals=4, v_pad=None, tracks=None):
    """The frame scenes of a recording (rows as data.read_file returns them) with at least min_peds pedestrians,
    padded to V = the largest scene (or v_pad, which must hold it).  The rows are uploaded once; two launches
    (stg_frame_scene_counts, then stg_frame_scenes) and one read-back of the per-frame counts.  tracks: a TrackRule --
    the scenes under that rule, from frame index min_seen - 1, as PartialScenes (the *_rule kernels)."""
    obs_len = _obs_len(obs_len)
    scale = _scale(decimals)
    rule = _rule(tracks, obs_len)
    if not _is_int(min_peds, 0):
        raise ValueError("min_peds must be an integer >= 0, got %r" % (min_peds,))
    frames, fs, ids, xy = sorted_rows(rows)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("recording_scenes runs on MI355X only: got device %s (no CPU fallback)" % device)
    nf = len(frames)
    fs_d = torch.from_numpy(fs).to(device)
    ids_d = torch.from_numpy(ids).to(device)
    xy_d = torch.from_numpy(xy).to(device)
    count = torch.zeros(nf, device=device, dtype=torch.int32)
    # the strict kernels, or their *_rule twins, which also take the rule and write `seen`
    form, rule_args = ("", {}) if rule is None else ("_rule", rule._asdict())
    call("stg_frame_scene_counts" + form, frame_start=ptr(fs_d), ids=ptr(ids_d), F=nf, T_obs=obs_len, **rule_args,
         count=ptr(count))
    cnt = count.cpu().numpy()
    first = obs_len - 1 if rule is None else rule.min_seen - 1
    sel = np.nonzero((cnt >= int(min_peds)) & (np.arange(nf) >= first))[0]
    vmax = int(cnt[sel].max()) if len(sel) else 0
    if v_pad is None:
        v = max(1, vmax)
    else:
        v = int(v_pad)
        if v < max(1, vmax):
            raise ValueError("v_pad=%d cannot hold the largest frame scene (%d pedestrians)" % (v, vmax))
    n = len(sel)
    obs = torch.empty((n, obs_len, v, 2), device=device, dtype=torch.float64)
    out_ids = torch.empty((n, v), device=device, dtype=torch.int64)
    peds = torch.empty(n, device=device, dtype=torch.int32)
    seen = () if rule is None else (torch.empty((n, v), device=device, dtype=torch.int32),)
    if n:
        sel_d = torch.from_numpy(sel.astype(np.int32)).to(device)
        call("stg_frame_scenes" + form, frame_start=ptr(fs_d), ids=ptr(ids_d), xy=ptr(xy_d), frames=ptr(sel_d), N=n, V=v,
             T_obs=obs_len, scale=scale, **rule_args, obs_abs=ptr(obs), out_ids=ptr(out_ids), num_peds=ptr(peds),
             **{"seen": ptr(x) for x in seen})
    return (FrameScenes if rule is None else PartialScenes)(frames[sel], obs, out_ids, peds, *seen)


def fill_tracks(obs_abs, seen, num_peds=None, decimals=4):
    """Fill the missed frames of a batch of scenes in place (stg_fill_tracks, one lane per scene and pedestrian) and
    return it: obs_abs (N,T_obs,V,2) float64 contiguous device tensor, seen (N,V) integers with bit t set = observed t
    frames ago (bit 0: the last frame), num_peds (N,) or None (every column).  A column's seen frames are rounded to
    `decimals` and its missed frames filled as under a TrackRule; a column at or past num_peds, not seen in the last
    frame or seen only once is left untouched."""
    require_gpu(obs_abs)
    if obs_abs.dim() != 4 or obs_abs.shape[3] != 2 or obs_abs.dtype != torch.float64 or not obs_abs.is_contiguous():
        raise ValueError("fill_tracks: obs_abs (N,T_obs,V,2) float64, contiguous, expected, got %s %s"
                         % (tuple(obs_abs.shape), obs_abs.dtype))
    n, t, v, _ = obs_abs.shape
    if not 2 <= t <= MAX_OBS_LEN:
        raise ValueError("fill_tracks: T_obs must be in [2, %d], got %d" % (MAX_OBS_LEN, t))
    scale = _scale(decimals)
    seen = torch.as_tensor(seen).to(device=obs_abs.device, dtype=torch.int32).contiguous()
    if tuple(seen.shape) != (n, v):
        raise ValueError("fill_tracks: seen (%d,%d) expected, got %s" % (n, v, tuple(seen.shape)))
    peds = peds_arg(num_peds, n, obs_abs.device)
    if n and v:
        call("stg_fill_tracks", obs_abs=ptr(obs_abs), seen=ptr(seen), num_peds=ptr(peds), N=n, T_obs=t, V=v, scale=scale)
    return obs_abs


@torch.no_grad()
def predict_recording(model, rows, k=20, seed=0, batch_size=64, noise_fn=None, min_peds=1, decimals=4, v_pad=None,
                      risk=None, tracks=None, calibration=None):
    """Predictions at every frame scene of a recording (recording_scenes with obs_len = model.seq_len): the Predictor
    over batch_size scenes per launch chain, the draws from the Philox stream keyed by seed + batch index, or from
    noise_fn(batch_index, (k,N,P,V,2)) -> standard normals (as predict.sample_test).  Returns (FrameScenes,
    Prediction) with the per-frame predictions concatenated: samples (K,N,P,V,2), mean (N,P,V,2), v_pred (N,5,P,V).
    risk: a predict.RiskSpec (zones (Z,4), the same for every frame) -- the result is then (FrameScenes, Prediction,
    ops.Risk), the counts of ops.sample_risk over each frame's K samples, concatenated like the predictions.
    tracks: a TrackRule -- the scenes of recording_scenes(tracks=...), a PartialScenes in the place of FrameScenes.
    calibration: a calibrate.Calibration the Predictor applies ahead of the sampler."""
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    dev = next(model.parameters()).device
    scenes = recording_scenes(rows, dev, model.seq_len, min_peds, decimals, v_pad, tracks)
    pred = Predictor(model, k, risk, calibration=calibration)
    if risk is not None and pred.spec.zones is not None and np.ndim(pred.spec.zones) != 2:
        raise ValueError("predict_recording: risk zones (Z,4) expected")
    n, _, v, _ = scenes.obs_abs.shape
    p = model.pred_seq_len
    parts, risks = [], []
    for b, lo in enumerate(range(0, n, int(batch_size))):
        hi = min(n, lo + int(batch_size))
        noise = noise_fn(b, (pred.k, hi - lo, p, v, 2)) if noise_fn is not None else None
        parts.append(pred.predict(scenes.obs_abs[lo:hi], scenes.num_peds[lo:hi], seed + b, noise))
        risks.append(pred.risk)
    if not parts:
        z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)      # noqa: E731
        res = Prediction(z(pred.k, 0, p, v, 2), z(0, p, v, 2), z(0, 5, p, v))
        if risk is None:
            return scenes, res
        zones = pred._zones(0, dev)
        return scenes, res, ops.risk_buffers(0, p, v, pred.k, pred.spec.radius, 0 if zones is None else zones.shape[0],
                                             pred.spec.pairs, dev)
    res = Prediction(torch.cat([r.samples for r in parts], 1), torch.cat([r.mean for r in parts], 0),
                     torch.cat([r.v_pred for r in parts], 0))
    if risk is None:
        return scenes, res
    return scenes, res, ops.Risk(pred.k, *(None if f[0] is None else torch.cat(f, 0) for f in list(zip(*risks))[1:]))


def host_detections(ids, xy, max_detections):
    """One frame of detections given as host arrays -> (ids (M,) int64, xy (M,2) float64), validated: at most
    max_detections of them, integral ids >= 0, no id twice.  ids None (a predictor with associate=): (None, xy)."""
    xy_np = np.asarray(xy.cpu() if torch.is_tensor(xy) else xy, dtype=np.float64).reshape(-1, 2)
    if ids is None:
        if len(xy_np) > max_detections:
            raise ValueError("push: %d detections > max_detections=%d" % (len(xy_np), max_detections))
        return None, np.ascontiguousarray(xy_np)
    ids_np = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
    m = len(ids_np)
    if m > max_detections:
        raise ValueError("push: %d detections > max_detections=%d" % (m, max_detections))
    if xy_np.shape[0] != m:
        raise ValueError("push: %d ids but %d positions" % (m, xy_np.shape[0]))
    ids_np = _integral_ids(ids_np, "push")
    if len(np.unique(ids_np)) != m:
        raise ValueError("push: duplicate pedestrian id in one frame")
    return ids_np, np.ascontiguousarray(xy_np)


_Option = collections.namedtuple("_Option", "plain timed with_time without_time coerce")


def _bare(spec):
    """A bare tuple or number in the place of the push-indexed `spec` -> that spec."""
    return lambda x: spec(*x) if isinstance(x, (tuple, list)) else spec(x)


# Which spec goes with time=, per option in the order they are checked: the push-indexed spec (what a bare tuple or number
# is coerced to), the spec(s) that go with time= only, and the refusal of each without its match (%s: the spec's class).
_OPTIONS = {
    "harvest": _Option(
        HarvestSpec, (TimedHarvestSpec,),
        "harvest= together with time= is not supported: a timed push is not one frame of a window (DESIGN.md 8)",
        "harvest=%s(...) needs time=TimeRule(...): its frames are instants of the step grid (without time= the "
        "push-indexed HarvestSpec serves)", _bare(HarvestSpec)),
    "associate": _Option(
        AssociateSpec, _TIMED_ASSOC,
        "associate= together with time= is not supported: a velocity per tick and a gate that grows with the gap are a "
        "change of their own (DESIGN.md 8)",
        "associate=%s(...) needs time=TimeRule(...): its tracks are aged by time (without time= the push-indexed "
        "AssociateSpec serves)", _bare(AssociateSpec)),
    "score": _Option(
        ScoreSpec, (TimedScoreSpec,),
        "time= together with score= is not supported: the score records are indexed by push, and re-indexing them by "
        "time is a change of its own (DESIGN.md 8); the records indexed by time are score=TimedScoreSpec(...) (DESIGN.md "
        "5.25)",
        "score=%s(...) needs time=TimeRule(...): its records are indexed by time (without time= the push-indexed "
        "ScoreSpec serves)", lambda x: ScoreSpec(*x)),
}

_Feed = collections.namedtuple("_Feed", "lead det when pushed outs tail rings")
_Feed.__doc__ = """What differs between one stream and many, as a predictor hands it to its stages: lead, the leading axis
of every state tensor (() or (NS,)); det, the staging buffers as pointers by the names the push and association kernels
take them under; when, the pointer to the push time(s) (read under time= only); pushed, the (NS,) int32 `pushed` words
(None: one stream, always pushed); outs, the names of those of _outs() that the push kernel writes (`seen` apart); tail,
what the push kernel takes besides, by name; rings, whether reset() clears the position rings too."""
_I32, _I64, _F64 = torch.int32, torch.int64, torch.float64
_PUSH_OUTS = ("obs_abs", "out_ids", "num_peds", "out_flags")        # (out_flags: many streams only)


def _makers(dev, lead):
    """(zeros, empty): (dtype, *shape) -> a device tensor of lead + shape, one set per stream."""
    return tuple(lambda dtype, *shape, make=make: make(lead + shape, device=dev, dtype=dtype)
                 for make in (torch.zeros, torch.empty))


def _ptrs(named):
    return {n: ptr(x) for n, x in named.items()}


class _Stage:
    """One launch around the model in a live push, built once, behind the predictor's staging buffers.  A stage owns its
    device tensors (`named`: by the names the predictor shows them under, which are the names the entry point takes them
    under; `state`: the same as a tuple), says what a reset fills (`cleared`, (tensor, value) pairs) and what an empty
    push moves (`moved`), resolves its entry point -- the lone or the _streams one, in its push-indexed or its timed form
    -- with every argument that stays the same from push to push, and has ONE launch, which takes what varies."""

    def _own(self, named, fill, kept=(), also=()):
        """`named` is the state: a reset fills it with 0, and with fill[name] where that is given, but for the names in
        `kept`; an empty push moves all of it, and `also`."""
        self.named, self.state = named, tuple(named.values())
        self.moved = self.state + also
        self.cleared = [(x, fill.get(n, 0)) for n, x in named.items() if n not in kept]

    def _bind(self, base, feed, form, varying=(), **fixed):
        """The entry point of the family `base` that serves this feed (many streams: the _streams one, which is told how
        many) in this form ("", or the suffix of a twin), its `fixed` arguments bound; a launch names the `varying`."""
        if feed.lead:
            fixed["NS"] = feed.lead[0]
        self.entry = Bound(base + ("_streams" if feed.lead else "") + form, varying, **fixed)

    def launch(self, outs):
        self.entry()


class _Tracks(_Stage):
    """The push kernel and the track state: slot ids, presence masks, the position ring and {head, flags}; with time=
    the sample rings (times, positions), their {write index, count} and the clock in the place of masks and ring."""

    def __init__(self, p, feed):
        zeros, empty = _makers(p.device, feed.lead)
        rule = {} if p.rule is None else p.rule._asdict()
        named = dict(slot_id=empty(_I64, p.s))
        sizes = dict(M_max=p.m_max, S=p.s, T_obs=p.t_obs, scale=p.scale, V=p.v)
        if p.time is None:
            # the strict kernel, or its *_rule twin, which also takes the rule and writes `seen`
            named.update(mask=empty(_I32, p.s), ring=zeros(_F64, p.t_obs, p.s, 2))
            form, rings = "_rule" if rule else "", ("ring",)         # (a ring row is read only where the mask says so)
        else:
            named.update(t_ring=zeros(_I64, p.s, p.time.history), xy_ring=zeros(_F64, p.s, p.time.history, 2),
                         slot_head=empty(_I32, p.s, 2), clock=empty(_I64, 2))
            form, rings = "_timed", ("t_ring", "xy_ring")            # (a ring holds what its count says)
            sizes.update(det_time=feed.when, R=p.time.history, step=p.time.step, max_dt=p.time.max_dt)
        named["head_flags"] = empty(_I32, 2)
        self._own(named, {"slot_id": -1}, kept=() if feed.rings else rings)
        # of _outs() the kernel writes the first, feed.outs, and, under a rule, `seen`, the last
        self.feed, self.seen = feed, slice(-1, None) if rule else slice(0, 0)
        self.outs = feed.outs + (("seen",) if rule else ())
        self._bind("stg_track_push", feed, form, self.outs, **feed.det, **_ptrs(named), **sizes, **rule, **feed.tail)

    def launch(self, outs):
        """staging buffers + track state -> outs"""
        n, pushed = len(self.feed.outs), self.feed.pushed
        self.entry(**{name: ptr(x) for name, x in zip(self.outs, outs[:n] + outs[self.seen])})
        if pushed is not None:                               # many streams: which of them this tick pushed, as a bool
            torch.ne(pushed, 0, out=outs[n])


class _Association(_Stage):
    """With associate=: the launch ahead of the push kernel that writes the ids it reads, and the association state: slot
    ids, positions, velocities, misses (under a TimedAssociateSpec the times of the last match in their place, under a
    FilteredAssociateSpec also the covariances), hits; per stream next_id and the flags."""

    def __init__(self, p, feed, tracks):
        spec = p.assoc
        zeros, empty = _makers(p.device, feed.lead)
        one = feed.lead or (1,)
        c = p.s if spec.capacity is None else spec.capacity
        named = dict(trk_id=empty(_I64, c), trk_pos=zeros(_F64, c, 2), trk_vel=zeros(_F64, c, 2))
        if isinstance(spec, _TIMED_ASSOC):
            # the timed twin, or the filtered one: it reads the time(s) the timed push reads and that push's clock; the
            # lifetime is (step, max_age) ticks
            named["trk_t"] = zeros(_I64, c)
            if isinstance(spec, FilteredAssociateSpec):
                named["trk_cov"] = zeros(_F64, c, 3)
                form, squared = "_filtered", dict(zip(("r", "qa", "v0", "n2", "gmax2"), spec[:5]))
            else:
                form, squared = "_timed", dict(gate2=spec.gate, gate_new2=spec.gate_new)
            rest = dict(det_time=feed.when, clock=ptr(tracks.named["clock"]), step=p.time.step, max_age=spec.max_age)
        else:
            named["trk_miss"] = zeros(_I32, c)
            form, squared, rest = "", dict(gate2=spec.gate, gate_new2=spec.gate_new), dict(max_miss=spec.max_miss)
        named.update(trk_hits=zeros(_I32, c), next_id=torch.zeros(one, device=p.device, dtype=_I64),
                     assoc_flags=torch.zeros(one, device=p.device, dtype=_I32))
        self._own(named, {"trk_id": -1})                     # (an empty push ages the association's tracks too)
        # (the gates, or the filter's five parameters, travel squared, in float64)
        self._bind("stg_associate", feed, form, **feed.det, M_max=p.m_max, **_ptrs(named), C=c, scale=p.scale,
                   **{n: x * x for n, x in squared.items()}, **rest)


class _Harvest(_Stage):
    """With harvest=: the launch behind the push kernel, which reads the state the push has left, the harvest's own
    history, one per stream -- presence words, a T_all-deep position ring, {ring row, pushes since reset}; under a
    TimedHarvestSpec the grid {anchored, g0, instants skipped} behind them --, the ONE log of the predictor and, for many
    streams, the launches' scratch."""

    def __init__(self, p, feed, tracks):
        spec = p.harvest_spec
        zeros, _ = _makers(p.device, feed.lead)
        log = LiveWindows(spec, p.t_obs, p.device)
        named = dict(h_word=zeros(_I32, p.s), h_ring=zeros(_F64, log.t_all, p.s, 2), h_head=zeros(_I32, 2))
        sizes = dict(S=p.s, T_obs=p.t_obs, T_all=log.t_all, min_peds=spec.min_peds)
        form = ""
        if p.time is not None:
            named["h_clock"] = zeros(_I64, 3)
            form = "_timed"
            sizes.update(R=p.time.history, scale=p.scale, step=p.time.step, max_dt=p.time.max_dt, settle=spec.settle)
        # A reset leaves the log alone, and the ring: a ring row is read only where the word says detected.  An empty push
        # ages the words and moves the ring row; it has no candidates, so of the log only the header is kept (its rows,
        # offsets and tags are written for a window alone).
        self._own(named, {}, kept=("h_ring",), also=(log.header,))
        self.named = dict(named, harvest=log)
        if feed.lead:                                        # a _streams entry point is told of its streams; its scratch
            self.work = torch.zeros(feed.lead[0] * (p.s + 3), device=p.device, dtype=_I32)
            streams = dict(pushed=ptr(feed.pushed), work=ptr(self.work))
        else:                                                # the lone one tags its windows with a stream index
            streams = dict(stream_index=0)
        self._bind("stg_window_harvest", feed, form, **_ptrs(tracks.named), **streams, **sizes, **_ptrs(named),
                   **log._args())


class _Score:
    """With score=: the launch behind the sampler (and the risk counts) -- the pending predictions against this push's
    detections, then this push's prediction into the records (ops.score_push); with a TimedScoreSpec against the track
    samples the timed push has just recorded (ops.score_timed_push) -- and the records and totals, which it shows as a
    _Stage shows its tensors.  Its launch also takes the prediction."""
    named = {}

    def __init__(self, p, feed, tracks):
        spec, dev = p.score_spec, p.device
        ns, n_pred, q = (feed.lead or (1,))[0], p.model.pred_seq_len, len(spec.levels)
        thr = torch.tensor(spec.thresholds, dtype=torch.float32).to(dev) if q else None
        if isinstance(spec, TimedScoreSpec):
            self.state = ops.score_timed_state(ns, n_pred, p.v, p.k, spec.pending, dev, spec.best_of_k, q)
            self.fresh = lambda: ops.score_timed_buffers(ns, n_pred, q, dev)
            self.push = functools.partial(ops.score_timed_push, self.state, thr, tracks=tracks.state, step=p.time.step,
                                          max_dt=p.time.max_dt, scale=p.scale, pushed=feed.pushed)
        else:
            self.state = ops.score_state(ns, n_pred, p.v, p.k, dev, spec.best_of_k, q)
            self.fresh = lambda: ops.score_buffers(ns, n_pred, p.v, dev, spec.best_of_k)
            # (ops.score_push takes the staging buffers by the same names, in lower case)
            self.push = functools.partial(ops.score_push, self.state, thr, m_max=p.m_max, scale=p.scale,
                                          **{n.lower(): x for n, x in feed.det.items()})
        self.cleared = [(x, -1 if n == "rec_ids" else 0) for n, x in zip(self.state._fields, self.state) if x is not None]
        self.moved = tuple(x for x, _ in self.cleared)       # an empty push is a push: it scores and enqueues
        self.ids_shape, self.samples = (ns, p.v), spec.best_of_k

    def launch(self, outs, r, out=None):
        """Score the chain's Prediction r of the push that wrote outs; `out`: an earlier result to fill (capture)."""
        return self.push(r.mean, r.v_pred, r.samples if self.samples else None, outs[1].view(self.ids_shape), outs[2],
                         out=out)


class _LivePredictor:
    """What FramePredictor and StreamsPredictor share: the argument checks, the stages on the device (with the
    subclass's leading axis), the eager push and its capture as ONE graph.  The core holds the stages in launch order
    (_build) and shows their tensors under their names; push, capture, reset and the warm-up loop over them.  A subclass
    builds its staging buffers, hands the stages its _Feed and supplies

        _stage(*det, seed)       copy one push's detections (and the seed, unless None) into its device staging buffers;
                                 with time= it takes the push's time(s) by keyword and stages them with the detections
        _outs()                  fresh per-push outputs (obs_abs, ids, num_peds, ...; under a TrackRule `seen` last)
        _wrap(outs, r, static)   the result tuple of outs and the chain's Prediction r (static: a captured push)
        _still()                 make warm-up pushes harmless; returns the (tensor, saved copy) pairs to put back after

    and `seed_dev`, the (1,) int64 device tensor the sampler reads its seed from."""
    assoc = None                         # the AssociateSpec, TimedAssociateSpec or FilteredAssociateSpec; None: ids come
                                         # with the pushes
    harvest = None                       # the LiveWindows of a predictor made with harvest=; None without
    h_clock = None                       # with harvest=TimedHarvestSpec: {anchored, g0, instants skipped} per stream

    def __init__(self, model, k, obs_len, capacity, max_peds, max_detections, decimals, risk=None, keep_samples=True,
                 tracks=None, score=None, time=None, associate=None, harvest=None, calibration=None):
        self.model = model
        self.k = int(k)
        given = dict(harvest=harvest, associate=associate, score=score)
        for name, opt in _OPTIONS.items():
            spec = given[name]
            if spec is None:
                continue
            if isinstance(spec, opt.timed):
                if time is None:
                    raise ValueError(opt.without_time % type(spec).__name__)
            elif time is not None:
                raise ValueError(opt.with_time)
            elif not isinstance(spec, opt.plain) and name != "harvest":
                # (a bare harvest= is coerced below, where it is checked: what it refuses comes behind every other refusal)
                given[name] = opt.coerce(spec)
        self.assoc, score = given["associate"], given["score"]
        self._n_det = 0
        self._risk_args = (risk, keep_samples, calibration)
        if score is not None:
            if score.best_of_k and not keep_samples:
                raise ValueError("score: ScoreSpec(best_of_k=True) scores the K samples, and keep_samples=False leaves "
                                 "none (pass ScoreSpec(best_of_k=False) or keep the samples)")
            if score.best_of_k and not 1 <= self.k <= ops.SCORE_MAX_K:
                raise ValueError("score: best_of_k needs 1 <= k <= %d, got %d" % (ops.SCORE_MAX_K, self.k))
            if int(max_peds) > ops.SCORE_MAX_V:
                raise ValueError("score: max_peds=%d above the score kernel's limit of %d"
                                 % (int(max_peds), ops.SCORE_MAX_V))
            if model.pred_seq_len > ops.SCORE_MAX_P:
                raise ValueError("score: pred_seq_len=%d above the score kernel's limit of %d"
                                 % (model.pred_seq_len, ops.SCORE_MAX_P))
        self.score_spec = score
        self.score = None
        self.t_obs = _obs_len(obs_len)
        if self.t_obs != model.seq_len:
            raise ValueError("obs_len=%d but the model observes %d frames" % (self.t_obs, model.seq_len))
        self.scale = _scale(decimals)
        self.rule = _rule(tracks, self.t_obs)
        self.time = None
        if time is not None:
            self.time = (time if isinstance(time, TimeRule) else TimeRule(*time)).checked(self.t_obs)
            if self.rule is None:                            # a timed push always goes through the rule, and writes `seen`
                self.rule = TrackRule(self.t_obs, 0)
        self.seen = None
        self.s, self.v, self.m_max = int(capacity), int(max_peds), int(max_detections)
        if not 1 <= self.s <= MAX_SLOTS:
            raise ValueError("capacity must be in [1, %d], got %r" % (MAX_SLOTS, capacity))
        if not 1 <= self.m_max <= MAX_DETECTIONS:
            raise ValueError("max_detections must be in [1, %d], got %r" % (MAX_DETECTIONS, max_detections))
        if self.v < 1:
            raise ValueError("max_peds must be >= 1, got %r" % (max_peds,))
        if harvest is not None:
            if not isinstance(harvest, (HarvestSpec, TimedHarvestSpec)):
                harvest = _OPTIONS["harvest"].coerce(harvest)
            # (the spec that goes with time= also fits its settle to the rule's max_dt)
            harvest = harvest.checked(self.t_obs, self.v, model.pred_seq_len,
                                      *(() if self.time is None else (self.time.max_dt,)))
        self.harvest_spec = harvest

    def _device(self):
        """Look the model's device up: every argument has been checked by now."""
        self.device = next(self.model.parameters()).device
        require_gpu(next(self.model.parameters()))
        return self.device

    def _build(self, feed):
        """Build the chain and the stages on the subclass's staging buffers (`feed`); show the stages' tensors by name."""
        self._pred = Predictor(self.model, self.k, *self._risk_args)
        tracks = _Tracks(self, feed)
        # THE order of the launches of a push: association -> tracks -> harvest, then the chain, then the score
        ahead = () if self.assoc is None else (_Association(self, feed, tracks),)
        behind = () if self.harvest_spec is None else (_Harvest(self, feed, tracks),)
        self._scorer = None if self.score_spec is None else _Score(self, feed, tracks)
        self._front_stages = ahead + (tracks,) + behind
        self._stages = self._front_stages + (() if self._scorer is None else (self._scorer,))
        of = {type(st): st.state for st in self._stages}
        self._state, self._assoc_state, self._score_state = (of.get(kind) for kind in (_Tracks, _Association, _Score))
        for st in self._stages:
            vars(self).update(st.named)

    @property
    def score_totals(self):
        """With score=ScoreSpec(...): the running totals on the device since reset(), (totals (NS,P,5+Q) float64,
        traj_totals (NS,5) float64) as ops.ScoreState describes them (NS = 1 for a FramePredictor); reading them is the
        caller's synchronisation -- frames.score_summary turns them into host numbers.  None without a ScoreSpec."""
        st = self._score_state
        return None if st is None else (st.totals, st.traj_totals)

    @property
    def score_records(self):
        """With score=TimedScoreSpec(...): the record ring on the device, the ops.ScoreTimedState itself (NS = 1 for a
        FramePredictor) -- rec_t, rec_status, rec_peds, rec_ids, the tables matched / err / d2 / nll / best (NS,Rp,P,V)
        and the retired rows traj_* (NS,Rp,V); reading it is the caller's synchronisation.  None otherwise."""
        return self._score_state if isinstance(self._score_state, ops.ScoreTimedState) else None

    @property
    def score_evictions(self):
        """With score=TimedScoreSpec(...): (NS,) int64 on the device, the records overwritten while still pending since
        reset() (size `pending` to the feed: predict.TimedScoreSpec).  None otherwise."""
        return None if self.score_records is None else self._score_state.counters[:, 1]

    def assoc_tracks(self, host=False):
        """With associate=: the association's live tracks, (ids (n,) int64, pos (n,2) float64, vel (n,2) float64) in slot
        order -- under a FilteredAssociateSpec the smoothed positions and the smoothed velocities per model step, under
        the other two specs the last matched detections and the two-sample velocities (per push, or per model step).
        A StreamsPredictor returns one such triple per stream.  Device tensors, or with host=True numpy copies; host
        side only: it waits for the device and is no part of a captured push."""
        if self._assoc_state is None:
            raise ValueError("assoc_tracks() needs associate=: without it the ids come with the pushes")

        def one(ids, pos, vel):
            at = torch.nonzero(ids >= 0).flatten()
            got = (ids[at], pos[at], vel[at])
            return tuple(x.cpu().numpy() for x in got) if host else got
        if self.trk_id.dim() == 1:
            return one(self.trk_id, self.trk_pos, self.trk_vel)
        return [one(self.trk_id[b], self.trk_pos[b], self.trk_vel[b]) for b in range(self.trk_id.shape[0])]

    @property
    def harvest_clock(self):
        """With harvest=TimedHarvestSpec(...): (NS,3) int64 on the device (NS = 1 for a FramePredictor), per stream
        {anchored 0/1, g0, grid instants skipped} since its reset -- a window tagged (stream, i) ends at the instant g0 +
        i * step; reading it is the caller's synchronisation.  None otherwise."""
        return None if self.h_clock is None else self.h_clock.view(-1, 3)

    def _front(self, outs):
        """The launches that turn the staged detections into the scene: with associate= the association, then the push;
        with harvest= the window harvest behind it, which reads the state the push has left."""
        for st in self._front_stages:
            st.launch(outs)

    def _clear(self, at=None):
        """Fill what every stage says a reset fills -- the tracks forgotten, the association's ids from 0 again, the
        score's records and totals and the harvest history emptied: everywhere, or at the stream indices `at`."""
        for st in self._stages:
            for x, fill in st.cleared:
                if at is None:
                    x.fill_(fill)
                else:
                    x.index_fill_(0, at, fill)

    @property
    def risk(self):
        """The ops.Risk of the last push (predict.RiskSpec given as `risk`): counts over the K samples, one scene per
        stream; from a captured push the graph's static tensors.  None without a RiskSpec or before the first push."""
        return self._pred.risk

    def _seen_out(self, *shape):
        """Under a TrackRule, the push's extra output: the presence bits of every scene slot (kept at `.seen`)."""
        return () if self.rule is None else (torch.empty(shape, device=self.device, dtype=torch.int32),)

    @property
    def zones(self):
        """The device tensor of rectangles the reducer reads ((Z,4), or per stream (NS,Z,4)); a caller may overwrite
        it between pushes."""
        return self._pred.zones

    @torch.no_grad()
    def push(self, *det, seed=None, noise=None, **when):
        """One push, run eagerly: `det` as the class describes it.  seed (by keyword): the sampler's Philox seed from
        now on (None keeps the last one); noise (K,N,P,V,2) standard normals instead of the Philox stream, N = 1 or
        the number of streams.  when: the push's time(s) under time=, by the class's keyword.  The outputs are fresh
        tensors: earlier results stay."""
        self._stage(*det, seed, **when)
        outs = self._outs()
        self._front(outs)
        if self.rule is not None:
            self.seen = outs[-1]
        with eval_mode(self.model):
            r = self._pred._forward(outs[0], outs[2], 0, noise, self.seed_dev)
        if self._scorer is not None:
            self.score = self._scorer.launch(outs, r)
        return self._wrap(outs, r, False)

    @torch.no_grad()
    def capture(self, warmup=2):
        """Capture ONE linear graph: the push kernel -> observed_inputs -> forward -> stg_sample_trajectories on static
        buffers, the seed read from `seed_dev` (Predictor.capture_chain).  Returns replay(*det, seed=None) -> the
        result on the static outputs, overwritten by the next replay; the detections are staged outside the graph.
        Warm-up and capture leave the track state as it was, and with it the score records and totals, the harvest
        history and the harvested windows."""
        outs = self._outs()
        saved = self._still()
        scored = None if self._scorer is None else self._scorer.fresh()
        try:
            graph, r, chain = self._pred.capture_chain(
                outs[0], outs[2], self.seed_dev, warmup, pre=lambda: self._front(outs),
                post=None if scored is None else lambda res: self._scorer.launch(outs, res, scored))
        finally:
            for x, x0 in saved:
                x.copy_(x0)
        res = self._wrap(outs, r, True)
        # every buffer the graph reads or writes lives as long as the returned replay
        static = (outs, chain, graph, scored)

        def replay(*det, seed=None, **when):
            self._stage(*det, seed, **when)
            static[2].replay()
            self.score = static[3]
            if self.rule is not None:
                self.seen = static[0][-1]
            return res
        return replay


def _ids_or_associate(ids, assoc, what):
    """Ids come from the caller, or from associate=: never both, never neither."""
    if assoc is None and ids is None:
        raise ValueError("%s: ids=None needs a predictor made with associate=AssociateSpec(...)" % what)
    if assoc is not None and ids is not None:
        raise ValueError("%s: a predictor made with associate= assigns the ids itself: pass ids=None" % what)


class FramePredictor(_LivePredictor):
    """Live prediction: push(ids, xy) with one frame of detections returns that frame's scene (the pedestrians seen
    in each of the last obs_len pushes, ascending ids, at most max_peds: the smallest) and K sampled trajectories per
    pedestrian, as a FramePrediction.  ids (M,) integral, xy (M,2) positions: host arrays (a repeated id is refused)
    or device tensors (a repeated id: the first detection wins, flag DUPLICATE).  The tracks live on the device
    (stg_track_push): `capacity` slots, a slot freed once its pedestrian has been missing for obs_len - 1 frames.  Ids
    come from the caller's tracker, or with associate= from the device (below).  tracks: a TrackRule -- the scene holds the
    pedestrians that rule admits, their missed frames filled (stg_track_push_rule); `.seen` (V,) int32 then holds the
    presence bits of the last push's scene slots (from a captured push the graph's static buffer, like `.risk`).
    score: a predict.ScoreSpec -- every push also scores the predictions of the last pred_seq_len pushes against its
    detections (stg_score_push, behind the sampler): `.score` holds the push's ops.Score (leading axis 1; from a captured
    push the graph's static tensors) and `.score_totals` the running totals on the device.
    time: a TimeRule -- push(ids, xy, t=TICKS) and the captured replay(ids, xy, t=TICKS) at any rate: the scene is the
    tracks resampled at t - k * step (stg_track_push_timed; the time is staged into a device int64 next to the count,
    so one graph serves every push); `.seen` is always set; a time not after the last push's: the empty scene, flag
    TIME_ORDER, nothing recorded.  Not together with score=ScoreSpec(...), whose records are indexed by push; with
    score=predict.TimedScoreSpec(...) (only together with time=) the prediction made at t is graded at t + h * step
    against the track's sample or interpolated position at that instant (stg_score_push_timed, behind the sampler):
    `.score` holds what the push added (ops.ScoreTimed), `.score_totals` the running totals, `.score_records` the
    record ring with its per-record tables and retired rows, `.score_evictions` the records lost to a full ring.
    associate: an AssociateSpec -- pushes carry no ids, push(None, xy) and the captured replay(None, xy): stg_associate,
    one launch ahead of the push kernel (inside the captured graph), gives every detection its track id in the staging
    buffer the push and the score read; the returned ids are those track ids, `.det_ids` (M,) the id of every detection
    of the last push in the caller's order, `.assoc_flags` (1,) int32 the association's flags (ASSOC_FULL).  Ids given
    with associate=, or None without it, are refused.  An AssociateSpec does not go together with time=; with time= the
    spec is a TimedAssociateSpec (only together with time=; stg_associate_timed, one launch ahead of the timed push,
    inside the captured graph): push(None, xy, t=TICKS), the tracks aged by time, `.det_ids` and `.assoc_flags` as above
    (ASSOC_TIME_ORDER, ids -1, for a push the timed push refuses); tracks=, risk=, score=TimedScoreSpec(...) and
    harvest=TimedHarvestSpec(...) work behind it unchanged.
    harvest: a HarvestSpec -- every push also keeps the training window it completes, if any (stg_window_harvest, one
    launch behind the push kernel, inside the captured graph; it reads the track state only, so it goes with tracks=,
    associate=, risk= and score=): `.harvest` is the LiveWindows log, its windows tagged (0, push index since reset()).
    reset() empties the harvest history and leaves the log.  Not together with time=: with time= the spec is a
    TimedHarvestSpec (only together with time=; stg_window_harvest_timed, one launch behind the timed push, inside the
    captured graph): the frames are the instants of the step grid anchored at the first accepted push, the windows are
    tagged (0, grid index of their last frame), `.harvest_clock` (1,3) int64 holds {anchored, g0, instants skipped};
    it goes with tracks=, risk= and score=TimedScoreSpec(...).
    calibration: a calibrate.Calibration, as in predict.Predictor -- stg_calib_apply between the model and the sampler,
    inside the captured graph; the returned v_pred, the samples, the risk counts and the score's records are the
    calibrated ones."""

    def __init__(self, model, k=20, obs_len=8, capacity=1024, max_peds=128, max_detections=1024, decimals=4,
                 risk=None, keep_samples=True, tracks=None, score=None, time=None, associate=None, harvest=None,
                 calibration=None):
        super().__init__(model, k, obs_len, capacity, max_peds, max_detections, decimals, risk, keep_samples, tracks,
                         score, time, associate, harvest, calibration)
        dev, m = self._device(), self.m_max
        self.det_id = torch.zeros(m, device=dev, dtype=torch.int64)
        self.det_xy = torch.zeros((m, 2), device=dev, dtype=torch.float64)
        self.det_count = torch.zeros(1, device=dev, dtype=torch.int32)
        self.det_time = torch.zeros(1, device=dev, dtype=torch.int64)
        self.seed_dev = torch.zeros(1, device=dev, dtype=torch.int64)
        self._build(_Feed(lead=(), det=dict(det_id=ptr(self.det_id), det_xy=ptr(self.det_xy),
                                            det_count=ptr(self.det_count)),
                          when=ptr(self.det_time), pushed=None, outs=_PUSH_OUTS[:3], tail={}, rings=False))
        self.reset()

    def reset(self):
        """Forget every track (the next obs_len - 1 pushes return empty scenes), with associate= the association's
        tracks and ids with them (under time= together with the clock), and with score= the pending records and the
        running totals; with harvest= the harvest history, not the log.  The position rings keep what they hold."""
        self._clear()

    @property
    def det_ids(self):
        """With associate=: the track id given to every detection of the last push, (M,) int64 on the device in the
        caller's detection order (a view of the staging buffer, overwritten by the next push)."""
        return None if self.assoc is None else self.det_id[:self._n_det]

    def _stage(self, ids, xy, seed, t=None):
        """Copy one frame of detections (host arrays or device tensors) into the device buffers the push reads, and
        with time= the push's time t."""
        if self.time is None:
            if t is not None:
                raise ValueError("push: t= needs a predictor made with time=TimeRule(...)")
        elif t is None:
            raise ValueError("push: a predictor made with time= needs the push's time, t=TICKS")
        else:
            t = _tick_time(t, "push")
        if (ids is None) != (self.assoc is not None):
            _ids_or_associate(ids, self.assoc, "push")
        if ids is None and torch.is_tensor(xy) and xy.is_cuda:
            m = xy.shape[0] if xy.dim() == 2 and xy.shape[1] == 2 else -1
            if m < 0:
                raise ValueError("push: xy (M,2) tensor expected, got %s" % (tuple(xy.shape),))
            if m > self.m_max:
                raise ValueError("push: %d detections > max_detections=%d" % (m, self.m_max))
            self.det_xy[:m].copy_(xy)
        elif torch.is_tensor(ids) and ids.is_cuda:
            m = ids.numel()
            if m > self.m_max:
                raise ValueError("push: %d detections > max_detections=%d" % (m, self.m_max))
            if not (torch.is_tensor(xy) and tuple(xy.shape) == (m, 2)):
                raise ValueError("push: xy (%d,2) tensor expected with device ids" % m)
            self.det_id[:m].copy_(ids.reshape(-1))
            self.det_xy[:m].copy_(xy)
        else:
            ids_np, xy_np = host_detections(ids, xy, self.m_max)
            m = len(xy_np)
            if m:
                if ids_np is not None:
                    self.det_id[:m].copy_(torch.from_numpy(ids_np))
                self.det_xy[:m].copy_(torch.from_numpy(xy_np))
        self._n_det = m
        self.det_count.fill_(m)
        if t is not None:
            self.det_time.fill_(t)
        if seed is not None:
            self.seed_dev.fill_(seed_i64(seed))

    def _outs(self):
        dev, t, v = self.device, self.t_obs, self.v
        return (torch.empty((1, t, v, 2), device=dev, dtype=torch.float64),
                torch.empty(v, device=dev, dtype=torch.int64),
                torch.empty(1, device=dev, dtype=torch.int32)) + self._seen_out(v)

    def _wrap(self, outs, r, static):
        obs, ids, peds = outs[:3]
        flags = self.head_flags[1:]          # (a captured push returns the state's own flags word)
        return FramePrediction(ids, peds, obs, r.samples[:, 0], r.mean[0], r.v_pred[0],
                               flags if static else flags.clone())

    def _still(self):
        """The warm-up pushes frames without detections, which age the tracks (with time=: move the clock): what every
        stage says an empty push moves goes back after it."""
        saved = [(x, x.clone()) for x in (self.det_count, *(x for st in self._stages for x in st.moved))]
        self.det_count.zero_()
        return saved


StreamsPrediction = collections.namedtuple("StreamsPrediction", "ids num_peds obs_abs samples mean v_pred flags pushed")
StreamsPrediction.__doc__ = """One tick of NS streams, on the device: ids (NS,V) int64 (-1 in padded slots),
num_peds (NS,) int32, obs_abs (NS,T_obs,V,2) float64, samples (K,NS,P,V,2), mean (NS,P,V,2), v_pred (NS,5,P,V) float32,
flags (NS,) int32 (the STG_TRACK_* flags of each stream's push, 0 where not pushed), pushed (NS,) bool.  A stream not
pushed this tick has the empty scene.  From a captured tick the tensors are the graph's static buffers, overwritten by
the next."""

PackedTick = collections.namedtuple("PackedTick", "det_start pushed ids xy")
PackedTick.__doc__ = """One tick packed for stg_track_push_streams: det_start (NS+1,) int32 (stream s owns detections
det_start[s] .. det_start[s+1]-1), pushed (NS,) int32 (1 = pushed this tick, an empty push included), ids (M,) int64 and
xy (M,2) float64: the pushed streams' detections concatenated in stream order."""

DeviceTick = collections.namedtuple("DeviceTick", "ids xy counts")
DeviceTick.__doc__ = """A tick whose detections are already device tensors, packed: ids (M,) int64 and xy (M,2)
float64, the streams' detections concatenated in stream order; counts (NS,) int32 (a device tensor, or host values):
stream s owns counts[s] detections, -1 = not pushed this tick (0 is an empty push).  Ranges past M are clamped; a count
above max_detections uses the first max_detections (flag TRUNCATED); a repeated id within a stream: the first detection
wins (flag DUPLICATE)."""


def pack_tick(tick, streams, max_detections, max_total_detections, associate=False):
    """One tick of host detections -> PackedTick, validated as host_detections validates one push: in every stream at
    most max_detections of them, integral ids >= 0, no id twice; stream indices in [0, streams); at most
    max_total_detections in all.  tick: a mapping {stream index: (ids, xy)} or a length-`streams` sequence of (ids, xy)
    or None (None: the stream is not pushed this tick; (ids, xy) with no detections is an empty push).
    associate: the entries are (None, xy) -- the device assigns the ids --, the PackedTick's ids are None and no id is
    looked at; without it an entry (None, xy) is refused."""
    if isinstance(tick, collections.abc.Mapping):
        entries = []
        for key, det in tick.items():
            _stream_index(key, streams, "tick")
            if det is not None:
                entries.append((int(key), det))
        entries.sort(key=lambda e: e[0])
    else:
        tick = list(tick)
        if len(tick) != streams:
            raise ValueError("tick: %d entries for %d streams" % (len(tick), streams))
        entries = [(s, det) for s, det in enumerate(tick) if det is not None]
    counts = np.zeros(streams, np.int64)
    pushed = np.zeros(streams, np.int32)
    ids_l, xy_l = [], []
    for s, det in entries:
        if len(det) != 2:
            raise ValueError("tick: stream %d: (ids, xy) expected" % s)
        ids_np, xy_np = det
        if (ids_np is None) != bool(associate):
            _ids_or_associate(ids_np, True if associate else None, "tick: stream %d" % s)
        # numpy arrays already in shape are taken as they are (a tick of many streams is packed on the host clock)
        if not associate and (type(ids_np) is not np.ndarray or ids_np.ndim != 1):
            ids_np = np.asarray(ids_np.cpu() if torch.is_tensor(ids_np) else ids_np).reshape(-1)
        if type(xy_np) is not np.ndarray or xy_np.dtype != np.float64 or xy_np.ndim != 2 or xy_np.shape[1] != 2:
            xy_np = np.asarray(xy_np.cpu() if torch.is_tensor(xy_np) else xy_np, dtype=np.float64).reshape(-1, 2)
        m = len(xy_np) if associate else len(ids_np)
        if m > max_detections:
            raise ValueError("tick: stream %d: %d detections > max_detections=%d" % (s, m, max_detections))
        if xy_np.shape[0] != m:
            raise ValueError("tick: stream %d: %d ids but %d positions" % (s, m, xy_np.shape[0]))
        counts[s] = m
        pushed[s] = 1
        ids_l.append(ids_np)
        xy_l.append(xy_np)
    total = int(counts.sum())
    if total > max_total_detections:
        raise ValueError("tick: %d detections > max_total_detections=%d" % (total, max_total_detections))
    xy = np.concatenate(xy_l) if xy_l else np.zeros((0, 2))
    det_start = np.zeros(streams + 1, np.int32)
    det_start[1:] = np.cumsum(counts)
    if associate:
        return PackedTick(det_start, pushed, None, np.ascontiguousarray(xy))
    ids = _integral_ids(np.concatenate(ids_l) if ids_l else np.zeros(0, np.int64), "tick")
    if total > 1:
        # a repeated (stream, id): one sort of stream << b | id where the ids fit in b bits, else a two-key sort
        owner = np.repeat(np.arange(streams, dtype=np.int64), counts)
        b = 63 - int(streams - 1).bit_length()
        if int(ids.max()) < 1 << b:
            key = np.sort((owner << b) | ids)
            dup = np.nonzero(key[1:] == key[:-1])[0]
            if len(dup):
                raise ValueError("tick: stream %d: duplicate pedestrian id %d in one frame"
                                 % (key[dup[0]] >> b, key[dup[0]] & ((1 << b) - 1)))
        else:
            order = np.lexsort((ids, owner))
            same = (owner[order[1:]] == owner[order[:-1]]) & (ids[order[1:]] == ids[order[:-1]])
            if same.any():
                at = order[1:][same][0]
                raise ValueError("tick: stream %d: duplicate pedestrian id %d in one frame" % (owner[at], ids[at]))
    return PackedTick(det_start, pushed, ids, np.ascontiguousarray(xy))


class StreamsPredictor(_LivePredictor):
    """Live prediction for NS independent streams (cameras, tracker feeds) at once.  Each stream is what a
    FramePredictor with the same capacity, max_detections, max_peds and decimals would be, fed only that stream's
    pushes: its own slots, presence masks and ring on the device, so the same pedestrian id in two streams is two
    tracks and a flag of one stream never shows in another.  One push(tick) -> StreamsPrediction stages the whole tick
    with ONE host->device copy (packed in a pinned buffer) and runs stg_track_push_streams (one workgroup per stream) ->
    observed_inputs -> forward -> sampler on the NS scenes as one batch padded to max_peds; capture() makes that ONE
    graph, warmed up and captured with no stream pushed.  tick: a mapping {stream index: (ids, xy)}, a length-NS
    sequence of (ids, xy) or None (host arrays; see pack_tick), or a DeviceTick.  The sampler's Philox draws are keyed
    by the scene's index in the tick: stream s draws what Predictor.predict draws for scene s of the tick's batch, not
    what a lone FramePredictor with the same seed draws.  The seed lives in the staging block.
    max_total_detections (default streams * max_detections) sizes the staging buffers.  risk (a predict.RiskSpec, its
    zones (Z,4) for every stream or (NS,Z,4) per stream) and keep_samples as in predict.Predictor: the tick's counts are
    at `.risk`, 5.4 MB of int32 counts at 600 streams padded to 128 pedestrians, where the samples are 147 MB.
    tracks: a TrackRule for every stream, as in FramePredictor (stg_track_push_streams_rule); `.seen` is (NS,V), zero
    for a stream not pushed.  score: a predict.ScoreSpec for every stream, as in FramePredictor
    (stg_score_push_streams, one workgroup per stream): `.score` is the tick's ops.Score with the streams leading, all
    zero for a stream not pushed, `.score_totals` the per-stream totals.  With best_of_k the records keep every push's
    samples for pred_seq_len pushes: about 3.5 MB per stream at 12 steps, 128 pedestrians and k = 20, so 600 streams
    hold about 2.1 GB (0.4 MB per stream with ScoreSpec(best_of_k=False)).
    associate: an AssociateSpec for every stream, each with its own tracks and its own ids from 0
    (stg_associate_streams, one workgroup per stream ahead of the push launch): tick entries are (None, xy), a
    DeviceTick is DeviceTick(None, xy, counts); `.det_ids` (M,) holds the ids of the tick's packed detections,
    `.assoc_flags` (NS,) the flags of each stream's last push.  A stream not pushed keeps its association state bit for
    bit.  An AssociateSpec does not go together with time=; with time= a TimedAssociateSpec, as in FramePredictor
    (stg_associate_streams_timed, every stream on its own clock): tick entries (None, xy) with times=, or
    DeviceTick(None, xy, counts) with device times.
    time: a TimeRule for every stream, each with its own clock (stg_track_push_streams_timed): push(tick, times=...)
    with times a length-NS sequence or a {stream: t} mapping that covers every pushed stream -- staged in the same ONE
    copy, the staging header extended by NS int64 --, or with a DeviceTick a device int64 (NS) tensor.  The sample
    rings are capacity * history * 24 bytes per stream (2.4 MB at the defaults): size capacity and history to the feed.
    Not together with score=ScoreSpec(...); score=predict.TimedScoreSpec(...) as in FramePredictor
    (stg_score_push_streams_timed, one workgroup per stream, every stream on its own clock): at pending 128, 128
    pedestrians, k = 20 and 12 steps the records hold about 41 MB per stream, 2.6 GB for 64 streams (7.5 MB per stream
    with best_of_k=False).
    harvest: a HarvestSpec for all streams together, as in FramePredictor (stg_window_harvest_streams: three launches
    behind the push launch): ONE log, `.harvest`, in which a tick's windows land in stream order, each tagged (stream,
    that stream's push index since its reset); a stream not pushed keeps its harvest history bit for bit.  With time= a
    TimedHarvestSpec, as in FramePredictor (stg_window_harvest_streams_timed): every stream on its own grid,
    `.harvest_clock` (NS,3).
    calibration: a calibrate.Calibration for every stream, as in FramePredictor."""

    def __init__(self, model, streams, k=20, obs_len=8, capacity=1024, max_peds=128, max_detections=1024, decimals=4,
                 max_total_detections=None, block_threads=0, risk=None, keep_samples=True, tracks=None, score=None,
                 time=None, associate=None, harvest=None, calibration=None):
        super().__init__(model, k, obs_len, capacity, max_peds, max_detections, decimals, risk, keep_samples, tracks,
                         score, time, associate, harvest, calibration)
        if not _is_int(streams, 1, MAX_STREAMS):
            raise ValueError("streams must be an integer in [1, %d], got %r" % (MAX_STREAMS, streams))
        self.ns = int(streams)
        if max_total_detections is None:
            cap = min(self.ns * self.m_max, MAX_TOTAL_DETECTIONS)
        else:
            cap = max_total_detections
            if not _is_int(cap, 1, MAX_TOTAL_DETECTIONS):
                raise ValueError("max_total_detections must be an integer in [1, %d], got %r"
                                 % (MAX_TOTAL_DETECTIONS, max_total_detections))
        self.cap = int(cap)
        if block_threads not in (0, 64, 256, 1024):
            raise ValueError("block_threads must be 0 (default), 64, 256 or 1024, got %r" % (block_threads,))
        self.block_threads = int(block_threads)
        ns = self.ns
        dev = self._device()
        # staging, the same byte layout on the host (pinned) and on the device: det_start (NS+1) int32 | pushed (NS)
        # int32 | seed int64 | cap records (id int64, x, y float64).  A tick copies the header and its M records.
        # With time= the header also holds the streams' push times, (NS) int64 behind the seed.
        o_pushed = 4 * (ns + 1)
        o_seed = (4 * (2 * ns + 1) + 7) // 8 * 8
        self._hdr = o_seed + 8 + (0 if self.time is None else 8 * ns)
        nbytes = self._hdr + 24 * self.cap
        self._host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        self._dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        hb = self._host.numpy()
        self._h_start = hb[:o_pushed].view(np.int32)
        self._h_pushed = hb[o_pushed:o_pushed + 4 * ns].view(np.int32)
        self._h_seed = hb[o_seed:o_seed + 8].view(np.int64)
        self._h_rec_i = hb[self._hdr:].view(np.int64).reshape(self.cap, 3)
        self._h_rec_f = hb[self._hdr:].view(np.float64).reshape(self.cap, 3)
        self.det_start = self._dev[:o_pushed].view(torch.int32)
        self.pushed_dev = self._dev[o_pushed:o_pushed + 4 * ns].view(torch.int32)
        self.seed_dev = self._dev[o_seed:o_seed + 8].view(torch.int64)
        if self.time is not None:
            self._h_times = hb[o_seed + 8:self._hdr].view(np.int64)
            self.times_dev = self._dev[o_seed + 8:self._hdr].view(torch.int64)
        self._rec_i = self._dev[self._hdr:].view(torch.int64).view(self.cap, 3)
        self._rec_f = self._dev[self._hdr:].view(torch.float64).view(self.cap, 3)
        # a record is (id, x, y): ids at stride 3 from its start, positions at stride 3 from 8 bytes in
        det = dict(det_id=ptr(self._rec_i), id_stride=3, det_xy=ctypes.c_void_p(self._rec_f.data_ptr() + 8),
                   xy_stride=3, M_total=self.cap, det_start=ptr(self.det_start), pushed=ptr(self.pushed_dev))
        self._build(_Feed(lead=(ns,), det=det, when=None if self.time is None else ptr(self.times_dev),
                          pushed=self.pushed_dev, outs=_PUSH_OUTS, tail=dict(block_threads=self.block_threads),
                          rings=True))
        self._copied = torch.cuda.Event()
        self._in_flight = False
        self.reset()

    def reset(self, streams=None):
        """Forget every track of all streams, or of the listed stream indices only (their next obs_len - 1 pushes
        return empty scenes; the other streams go on).  With score= their pending records and running totals are
        cleared with them; with harvest= their harvest history, not the log.  The position rings are cleared too."""
        if streams is None:
            self._clear()
            return
        idx = [int(x) for x in (streams if isinstance(streams, (list, tuple, np.ndarray, range)) else [streams])]
        for x in idx:
            if not 0 <= x < self.ns:
                raise ValueError("reset: stream index %d not in [0, %d)" % (x, self.ns))
        if idx:
            self._clear(torch.tensor(idx, dtype=torch.int64).to(self.device))

    @property
    def det_ids(self):
        """With associate=: the track id given to every detection of the last tick, (M,) int64 on the device, the
        pushed streams' detections in stream order as the tick listed them (a view of the staging records, overwritten
        by the next tick).  Ids count from 0 in every stream."""
        return None if self.assoc is None else self._rec_i[:self._n_det, 0]

    def _wait_host(self):
        """The pinned buffer is rewritten only after the previous tick's copy has left it."""
        if self._in_flight:
            self._copied.synchronize()
            self._in_flight = False

    def _copy(self, nbytes):
        self._dev[:nbytes].copy_(self._host[:nbytes], non_blocking=True)
        self._copied.record()
        self._in_flight = True

    def _host_times(self, times, pushed):
        """times (a length-NS sequence, None where a stream has none, or a {stream: t} mapping) -> (NS,) int64 with a
        time for every stream of `pushed`; refuses before anything is written."""
        if not isinstance(times, collections.abc.Mapping) and not torch.is_tensor(times):
            # a full sequence of plain integers, the case of a tick of many streams: no Python loop over the streams
            arr = times if type(times) is np.ndarray else np.asarray(times)
            if arr.dtype.kind == "i" and arr.shape == (self.ns,) and bool(((arr >= -(1 << 62)) & (arr < 1 << 62)).all()):
                return arr.astype(np.int64, copy=False)
        out = np.zeros(self.ns, np.int64)
        have = np.zeros(self.ns, bool)
        if isinstance(times, collections.abc.Mapping):
            entries = list(times.items())
        else:
            entries = list(enumerate(np.asarray(times.cpu()).tolist() if torch.is_tensor(times) else times))
            if len(entries) != self.ns:
                raise ValueError("times: %d entries for %d streams" % (len(entries), self.ns))
        for key, t in entries:
            _stream_index(key, self.ns, "times")
            if t is not None:
                out[key], have[key] = _tick_time(t, "times: stream %d" % key), True
        missing = np.nonzero((np.asarray(pushed) != 0) & ~have)[0]
        if len(missing):
            raise ValueError("times: stream %d is pushed without a time" % missing[0])
        return out

    def _stage(self, tick, seed, times=None):
        """One tick into the device staging buffer: host detections with ONE copy, device detections by device ops."""
        if self.time is None and times is not None:
            raise ValueError("push: times= needs a predictor made with time=TimeRule(...)")
        if self.time is not None and times is None:
            raise ValueError("push: a predictor made with time= needs the streams' push times, times=...")
        if isinstance(tick, DeviceTick):
            return self._stage_device(tick, seed, times)
        # refuses before anything is written or copied
        pk = pack_tick(tick, self.ns, self.m_max, self.cap, self.assoc is not None)
        m = len(pk.xy)
        self._n_det = m
        if times is not None:
            times = self._host_times(times, pk.pushed)
        self._wait_host()
        if times is not None:
            self._h_times[:] = times
        self._h_start[:] = pk.det_start
        self._h_pushed[:] = pk.pushed
        if seed is not None:
            self._h_seed[0] = seed_i64(seed)
        if m:
            if pk.ids is not None:                           # (with associate= the id field is the kernel's to write)
                self._h_rec_i[:m, 0] = pk.ids
            self._h_rec_f[:m, 1:] = pk.xy
        self._copy(self._hdr + 24 * m)

    def _stage_device(self, tick, seed, times=None):
        ids, xy, counts = tick
        if times is not None and not (torch.is_tensor(times) and times.is_cuda and times.dtype == torch.int64
                                      and times.numel() == self.ns):
            raise ValueError("DeviceTick: times must be a device int64 (%d) tensor" % self.ns)
        _ids_or_associate(ids, self.assoc, "DeviceTick")
        if not ((ids is None or (torch.is_tensor(ids) and ids.is_cuda)) and torch.is_tensor(xy) and xy.is_cuda):
            raise ValueError("DeviceTick: ids and xy must be device tensors")
        m = xy.shape[0] if ids is None else ids.numel()
        if m > self.cap:
            raise ValueError("tick: %d detections > max_total_detections=%d" % (m, self.cap))
        if tuple(xy.shape) != (m, 2):
            raise ValueError("DeviceTick: xy (%d,2) expected" % m)
        dev_counts = torch.is_tensor(counts) and counts.is_cuda
        if not dev_counts:
            counts = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).reshape(-1)
            if counts.dtype.kind not in "iu":
                raise ValueError("DeviceTick: counts must be integers")
        n_counts = counts.numel() if dev_counts else counts.size
        if n_counts != self.ns:
            raise ValueError("DeviceTick: %d counts for %d streams" % (n_counts, self.ns))
        self._n_det = m
        self._wait_host()
        if seed is not None:
            self._h_seed[0] = seed_i64(seed)
        if dev_counts:
            c = counts.reshape(-1).to(torch.int32)
            self.pushed_dev.copy_(c >= 0)
            self.det_start[:1].zero_()
            torch.cumsum(c.clamp(min=0), 0, dtype=torch.int32, out=self.det_start[1:])
            self.det_start.clamp_(max=m)
            if seed is not None:
                self.seed_dev.fill_(seed_i64(seed))
        else:
            self._h_pushed[:] = counts >= 0
            self._h_start[0] = 0
            self._h_start[1:] = np.minimum(np.cumsum(np.maximum(counts.astype(np.int64), 0)), m)
            self._copy(self._hdr)
        if times is not None:                                # behind the header copy, which carries stale host times
            self.times_dev.copy_(times.reshape(-1))
        if m:
            if ids is not None:
                self._rec_i[:m, 0].copy_(ids.reshape(-1))
            self._rec_f[:m, 1:].copy_(xy)

    def _outs(self):
        dev, ns, t, v = self.device, self.ns, self.t_obs, self.v
        return (torch.empty((ns, t, v, 2), device=dev, dtype=torch.float64),
                torch.empty((ns, v), device=dev, dtype=torch.int64), torch.empty(ns, device=dev, dtype=torch.int32),
                torch.empty(ns, device=dev, dtype=torch.int32),
                torch.empty(ns, device=dev, dtype=torch.bool)) + self._seen_out(ns, v)

    def _wrap(self, outs, r, static):
        obs, ids, peds, flags, pushed = outs[:5]
        return StreamsPrediction(ids, peds, obs, r.samples, r.mean, r.v_pred, flags, pushed)

    def _still(self):
        """Warm-up and capture run with no stream pushed, so no stream's state moves -- its score records and totals
        included: a stream not pushed keeps them bit for bit -- and nothing is put back."""
        self.det_start.zero_()
        self.pushed_dev.zero_()
        return ()


ScoreSummary = collections.namedtuple("ScoreSummary", "count err d2 nll best coverage trajectories ade fde ade_mean "
                                                      "fde_mean levels")
ScoreSummary.__doc__ = """Host numbers of the running score totals, numpy float64 with the totals' leading axes: per
horizon h = 1..P (last axis) count (matched pedestrians), err (mean displacement of the zero-noise trajectory), d2 (mean
squared Mahalanobis distance: 2 for a calibrated bivariate Gaussian), nll (mean negative log-likelihood) and best (mean
best-of-K displacement); coverage (...,P,Q): the fraction with d2 inside the ellipse of each level (calibrated: the level
itself); over the full trajectories (every one of the P steps matched): trajectories (their number), ade / fde (best-of-K,
as the reference reports them) and ade_mean / fde_mean (zero-noise).  NaN where nothing was counted."""


def score_summary(totals, traj_totals, levels=()):
    """The totals of `.score_totals` (device tensors or arrays, (...,P,5+Q) and (...,5)) as a ScoreSummary.  Reading
    device totals synchronises with the stream: this is the one place where scoring waits for the device, and only when
    the caller asks."""
    tot = np.asarray(totals.cpu() if torch.is_tensor(totals) else totals, dtype=np.float64)
    trj = np.asarray(traj_totals.cpu() if torch.is_tensor(traj_totals) else traj_totals, dtype=np.float64)
    levels = tuple(float(x) for x in levels)
    if tot.ndim < 2 or tot.shape[-1] != 5 + len(levels):
        raise ValueError("score_summary: totals (...,P,5+%d) expected for %d levels, got %s"
                         % (len(levels), len(levels), tot.shape))
    if trj.shape != tot.shape[:-2] + (5,):
        raise ValueError("score_summary: traj_totals %s expected, got %s" % (tot.shape[:-2] + (5,), trj.shape))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = tot[..., 0]
        per = [np.where(n > 0, tot[..., i] / n, np.nan) for i in range(1, 5)]
        cover = np.where(n[..., None] > 0, tot[..., 5:] / n[..., None], np.nan)
        nt = trj[..., 0]
        full = [np.where(nt > 0, trj[..., i] / nt, np.nan) for i in range(1, 5)]
    return ScoreSummary(n, per[0], per[1], per[2], per[3], cover, nt, full[0], full[1], full[2], full[3], levels)
