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
"""
import collections
import ctypes

import numpy as np
import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr
from .predict import Prediction, Predictor, _seed_i64

MAX_OBS_LEN = 32                       # presence masks are 32-bit
MAX_DETECTIONS = 2048                  # STG_TRACK_MAX_DETECTIONS
MAX_SLOTS = 2048                       # STG_TRACK_MAX_SLOTS
# FramePrediction.flags bits (STG_TRACK_* in include/stgcnn_hip.h)
DUPLICATE, OVERFLOW, TRUNCATED, TOO_MANY = 1, 2, 4, 8

FrameScenes = collections.namedtuple("FrameScenes", "frame obs_abs ids num_peds")
FrameScenes.__doc__ = """frame (N,) float64 numpy: the frame numbers of the scenes; on the device: obs_abs (N,T_obs,V,2)
float64, ids (N,V) int64 (-1 in padded slots), num_peds (N,) int32.  Padded slots are zeros."""

FramePrediction = collections.namedtuple("FramePrediction", "ids num_peds obs_abs samples mean v_pred flags")
FramePrediction.__doc__ = """One push, on the device: ids (V,) int64 (-1 in padded slots), num_peds (1,) int32,
obs_abs (1,T_obs,V,2) float64, samples (K,P,V,2), mean (P,V,2), v_pred (5,P,V) float32, flags (1,) int32 (DUPLICATE |
OVERFLOW | TRUNCATED | TOO_MANY of this push).  From a captured push the tensors are the graph's static buffers,
overwritten by the next push."""


def _obs_len(obs_len):
    if isinstance(obs_len, bool) or int(obs_len) != obs_len or not 1 <= int(obs_len) <= MAX_OBS_LEN:
        raise ValueError("obs_len must be an integer in [1, %d], got %r" % (MAX_OBS_LEN, obs_len))
    return int(obs_len)


def _scale(decimals):
    """np.around's 10^decimals (0.0: no rounding)."""
    if decimals is None:
        return 0.0
    if isinstance(decimals, bool) or int(decimals) != decimals or not 0 <= int(decimals) <= 15:
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


def recording_scenes(rows, device, obs_len=8, min_peds=1, decimals=4, v_pad=None):
    """The frame scenes of a recording (rows as data.read_file returns them) with at least min_peds pedestrians,
    padded to V = the largest scene (or v_pad, which must hold it).  The rows are uploaded once; two launches
    (stg_frame_scene_counts, then stg_frame_scenes) and one read-back of the per-frame counts."""
    obs_len = _obs_len(obs_len)
    scale = _scale(decimals)
    if isinstance(min_peds, bool) or int(min_peds) != min_peds or min_peds < 0:
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
    check(lib().stg_frame_scene_counts(ptr(fs_d), ptr(ids_d), nf, obs_len, ptr(count), stream_ptr()),
          "stg_frame_scene_counts")
    cnt = count.cpu().numpy()
    sel = np.nonzero((cnt >= int(min_peds)) & (np.arange(nf) >= obs_len - 1))[0]
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
    if n:
        sel_d = torch.from_numpy(sel.astype(np.int32)).to(device)
        check(lib().stg_frame_scenes(ptr(fs_d), ptr(ids_d), ptr(xy_d), ptr(sel_d), n, v, obs_len, scale, ptr(obs),
                                     ptr(out_ids), ptr(peds), stream_ptr()), "stg_frame_scenes")
    return FrameScenes(frames[sel], obs, out_ids, peds)


@torch.no_grad()
def predict_recording(model, rows, k=20, seed=0, batch_size=64, noise_fn=None, min_peds=1, decimals=4, v_pad=None):
    """Predictions at every frame scene of a recording (recording_scenes with obs_len = model.seq_len): the Predictor
    over batch_size scenes per launch chain, the draws from the Philox stream keyed by seed + batch index, or from
    noise_fn(batch_index, (k,N,P,V,2)) -> standard normals (as predict.sample_test).  Returns (FrameScenes,
    Prediction) with the per-frame predictions concatenated: samples (K,N,P,V,2), mean (N,P,V,2), v_pred (N,5,P,V)."""
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    dev = next(model.parameters()).device
    scenes = recording_scenes(rows, dev, model.seq_len, min_peds, decimals, v_pad)
    pred = Predictor(model, k)
    n, _, v, _ = scenes.obs_abs.shape
    p = model.pred_seq_len
    parts = []
    for b, lo in enumerate(range(0, n, int(batch_size))):
        hi = min(n, lo + int(batch_size))
        noise = noise_fn(b, (pred.k, hi - lo, p, v, 2)) if noise_fn is not None else None
        parts.append(pred.predict(scenes.obs_abs[lo:hi], scenes.num_peds[lo:hi], seed + b, noise))
    if not parts:
        z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)      # noqa: E731
        return scenes, Prediction(z(pred.k, 0, p, v, 2), z(0, p, v, 2), z(0, 5, p, v))
    return scenes, Prediction(torch.cat([r.samples for r in parts], 1), torch.cat([r.mean for r in parts], 0),
                              torch.cat([r.v_pred for r in parts], 0))


def host_detections(ids, xy, max_detections):
    """One frame of detections given as host arrays -> (ids (M,) int64, xy (M,2) float64), validated: at most
    max_detections of them, integral ids >= 0, no id twice."""
    ids_np = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
    xy_np = np.asarray(xy.cpu() if torch.is_tensor(xy) else xy, dtype=np.float64).reshape(-1, 2)
    m = len(ids_np)
    if m > max_detections:
        raise ValueError("push: %d detections > max_detections=%d" % (m, max_detections))
    if xy_np.shape[0] != m:
        raise ValueError("push: %d ids but %d positions" % (m, xy_np.shape[0]))
    ids_np = _integral_ids(ids_np, "push")
    if len(np.unique(ids_np)) != m:
        raise ValueError("push: duplicate pedestrian id in one frame")
    return ids_np, np.ascontiguousarray(xy_np)


class FramePredictor:
    """Live prediction: push(ids, xy) with one frame of detections returns that frame's scene (the pedestrians seen
    in each of the last obs_len pushes, ascending ids, at most max_peds: the smallest) and K sampled trajectories per
    pedestrian.  The tracks live on the device (stg_track_push): `capacity` slots, a slot freed once its pedestrian has
    been missing for obs_len - 1 frames.  Ids come from the caller's tracker (association is not done here)."""

    def __init__(self, model, k=20, obs_len=8, capacity=1024, max_peds=128, max_detections=1024, decimals=4):
        self.model = model
        self.k = int(k)
        self.t_obs = _obs_len(obs_len)
        if self.t_obs != model.seq_len:
            raise ValueError("obs_len=%d but the model observes %d frames" % (self.t_obs, model.seq_len))
        self.scale = _scale(decimals)
        self.s, self.v, self.m_max = int(capacity), int(max_peds), int(max_detections)
        if not 1 <= self.s <= MAX_SLOTS:
            raise ValueError("capacity must be in [1, %d], got %r" % (MAX_SLOTS, capacity))
        if not 1 <= self.m_max <= MAX_DETECTIONS:
            raise ValueError("max_detections must be in [1, %d], got %r" % (MAX_DETECTIONS, max_detections))
        if self.v < 1:
            raise ValueError("max_peds must be >= 1, got %r" % (max_peds,))
        dev = next(model.parameters()).device
        require_gpu(next(model.parameters()))
        self.device = dev
        t, s, v, m = self.t_obs, self.s, self.v, self.m_max
        self.slot_id = torch.empty(s, device=dev, dtype=torch.int64)
        self.mask = torch.empty(s, device=dev, dtype=torch.int32)
        self.ring = torch.zeros((t, s, 2), device=dev, dtype=torch.float64)
        self.head_flags = torch.empty(2, device=dev, dtype=torch.int32)
        self.det_id = torch.zeros(m, device=dev, dtype=torch.int64)
        self.det_xy = torch.zeros((m, 2), device=dev, dtype=torch.float64)
        self.det_count = torch.zeros(1, device=dev, dtype=torch.int32)
        self.seed_dev = torch.zeros(1, device=dev, dtype=torch.int64)
        self._pred = Predictor(model, self.k)
        self.reset()

    def reset(self):
        """Forget every track (the next obs_len - 1 pushes return empty scenes)."""
        self.slot_id.fill_(-1)
        self.mask.zero_()
        self.head_flags.zero_()

    def _stage(self, ids, xy, seed):
        """Copy one frame of detections (host arrays or device tensors) into the device buffers the push reads."""
        if torch.is_tensor(ids) and ids.is_cuda:
            m = ids.numel()
            if m > self.m_max:
                raise ValueError("push: %d detections > max_detections=%d" % (m, self.m_max))
            if not (torch.is_tensor(xy) and tuple(xy.shape) == (m, 2)):
                raise ValueError("push: xy (%d,2) tensor expected with device ids" % m)
            self.det_id[:m].copy_(ids.reshape(-1))
            self.det_xy[:m].copy_(xy)
        else:
            ids_np, xy_np = host_detections(ids, xy, self.m_max)
            m = len(ids_np)
            if m:
                self.det_id[:m].copy_(torch.from_numpy(ids_np))
                self.det_xy[:m].copy_(torch.from_numpy(xy_np))
        self.det_count.fill_(m)
        if seed is not None:
            self.seed_dev.fill_(_seed_i64(seed))

    def _outs(self):
        dev, t, v = self.device, self.t_obs, self.v
        return (torch.empty((1, t, v, 2), device=dev, dtype=torch.float64),
                torch.empty(v, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int32))

    def _push(self, outs):
        obs, ids, peds = outs
        check(lib().stg_track_push(ptr(self.det_id), ptr(self.det_xy), ptr(self.det_count), self.m_max,
                                   ptr(self.slot_id), ptr(self.mask), ptr(self.ring), ptr(self.head_flags), self.s,
                                   self.t_obs, ctypes.c_double(self.scale), self.v, ptr(obs), ptr(ids), ptr(peds),
                                   stream_ptr()), "stg_track_push")

    @staticmethod
    def _frame(outs, r, flags):
        obs, ids, peds = outs
        return FramePrediction(ids, peds, obs, r.samples[:, 0], r.mean[0], r.v_pred[0], flags)

    @torch.no_grad()
    def push(self, ids, xy, seed=None, noise=None):
        """One frame: ids (M,) integral, xy (M,2) positions, host arrays (a repeated id is refused) or device tensors
        (a repeated id: the first detection wins, flag DUPLICATE).  seed: the sampler's Philox seed from now on (None
        keeps the last one); noise (K,1,P,V,2) standard normals instead of the Philox stream.  Runs eagerly."""
        self._stage(ids, xy, seed)
        outs = self._outs()
        self._push(outs)
        was = self.model.training
        self.model.eval()
        try:
            r = self._pred._forward(outs[0], outs[2], 0, noise, self.seed_dev)
        finally:
            self.model.train(was)
        return self._frame(outs, r, self.head_flags[1:].clone())

    @torch.no_grad()
    def capture(self, warmup=2):
        """Capture ONE graph: stg_track_push -> observed_inputs -> forward -> stg_sample_trajectories, on static
        buffers, the seed read from a device tensor (as Predictor.capture).  Returns push(ids, xy, seed=None) ->
        FramePrediction on the static outputs; the detections are copied into the static buffers outside the graph.
        Warm-up and capture leave the track state as it was."""
        model, dev, t, v, p = self.model, self.device, self.t_obs, self.v, self.model.pred_seq_len
        outs = self._outs()
        bufs = (torch.empty((1, t, v, 2), device=dev, dtype=torch.float32),
                torch.empty((1, t, v, 2), device=dev, dtype=torch.float32),
                torch.empty((1, t, v, v), device=dev, dtype=torch.float32))
        samp = (torch.empty((self.k, 1, p, v, 2), device=dev, dtype=torch.float32),
                torch.empty((1, p, v, 2), device=dev, dtype=torch.float32))
        saved = [x.clone() for x in (self.slot_id, self.mask, self.ring, self.head_flags, self.det_count)]

        def step():
            self._push(outs)
            return self._pred._forward(outs[0], outs[2], 0, None, self.seed_dev, bufs, samp)
        was = model.training
        model.eval()
        try:
            self.det_count.zero_()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                r = step()
        finally:
            model.train(was)
            for x, y in zip((self.slot_id, self.mask, self.ring, self.head_flags, self.det_count), saved):
                x.copy_(y)
        res = self._frame(outs, r, self.head_flags[1:])
        # every buffer the graph reads or writes lives as long as the returned push
        static = (outs, bufs, samp, graph)

        def replay(ids, xy, seed=None):
            self._stage(ids, xy, seed)
            static[3].replay()
            return res
        return replay
