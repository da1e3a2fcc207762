"""Prediction from what a user holds -- observed absolute tracks -- to K sampled future trajectories per pedestrian,
batched on the device: the counterpart of the reference's test() (test.py:18-127) and of the `raw_data_dict` that
test_v.py / visualize.py read.

    observed_inputs   obs_abs (N,T_obs,V,2) -> model input x, adjacency, last observed position
    Predictor         relative coordinates -> adj_build -> fused forward -> stg_sample_trajectories; eager
                      (`predict`) or as ONE captured graph (`capture`; `capture_chain` is the same chain on the
                      caller's static inputs, which frames.py puts behind its push kernels).  With `risk=RiskSpec(...)`
                      the chain ends in stg_sample_risk: conflict and zone-occupancy counts over the K samples
    ScoreSpec         what the live predictors (frames.py) score their predictions for once the truth has arrived
    TimedScoreSpec    the same for predictors driven with time=: records indexed by time, truth interpolated
    sample_test       test() over data.SceneWindows: (ade, fde, raw_data_dict)
"""
import collections
import contextlib

import numpy as np
import torch

from . import data, graphs, ops
from ._lib import peds_arg, require_gpu, seed_i64

Prediction = collections.namedtuple("Prediction", "samples mean v_pred")
Prediction.__doc__ = """samples (K,N,P,V,2) absolute sampled trajectories, mean (N,P,V,2) the zero-noise trajectory,
v_pred (N,5,P,V) the model output (the reference's V_pred before its permute).  Padded slots are zeros."""


RiskSpec = collections.namedtuple("RiskSpec", "radius zones pairs", defaults=(None, None, False))
RiskSpec.__doc__ = """What a Predictor reduces its K samples to (ops.sample_risk): radius (two pedestrians closer than
this conflict; None: no conflict counts), zones ((Z,4) rectangles [x0,y0,x1,y1] for every scene or (N,Z,4) per scene;
None: no zone counts), pairs (also the (N,V,V) pair counts)."""


class ScoreSpec(collections.namedtuple("ScoreSpec", "levels best_of_k")):
    """What a live predictor scores its predictions for, once the tracker has delivered the positions they predicted
    (ops.score_push).  levels: at most four probability levels in (0, 1) -- the running totals count how
    often the truth fell inside the predicted Gaussian's ellipse of that level (d2 <= -2 ln(1 - p)), the calibration
    check; best_of_k: also keep each push's K samples on the device and score best-of-K ADE / FDE as the paper defines
    them (needs the predictor's samples: not with keep_samples=False)."""
    __slots__ = ()

    def __new__(cls, levels=(0.5, 0.9, 0.99), best_of_k=True):
        levels = tuple(float(x) for x in levels)
        ops.score_thresholds(levels)                       # refuses a level outside (0, 1) and more than four of them
        if not isinstance(best_of_k, (bool, np.bool_)):
            raise ValueError("ScoreSpec: best_of_k must be True or False, got %r" % (best_of_k,))
        return super().__new__(cls, levels, bool(best_of_k))

    @property
    def thresholds(self):
        """The d2 thresholds of the levels, -2 ln(1 - p)."""
        return ops.score_thresholds(self.levels)


class TimedScoreSpec(collections.namedtuple("TimedScoreSpec", "levels best_of_k pending")):
    """What a live predictor driven with time= scores its predictions for (ops.score_timed_push): the
    prediction made at time t is graded at t + h * step against the track's position at that instant -- a sample at
    exactly that time, or the interpolation of the two samples that bracket it when they are at most max_dt apart, as
    the timed push builds its window.  levels and best_of_k as ScoreSpec; pending: the number of record rows per stream
    (1 .. 1024).  Every accepted push leaves a record and a record lives for pred_seq_len * step ticks, so `pending`
    should be at least (pushes per step) * pred_seq_len -- 48 for a 25 Hz feed and a 0.4 s step at pred_seq_len 12 --
    or records are evicted before their last instant (counted in `.score_evictions`; a full trajectory is never lost
    that way, an evicted one only never becomes full).  The records hold pending * V * (28 + 36 P) bytes per stream and
    pending * V * (8 K P + 4 K + 4 P + 8) more with best_of_k."""
    __slots__ = ()

    def __new__(cls, levels=(0.5, 0.9, 0.99), best_of_k=True, pending=128):
        levels = tuple(float(x) for x in levels)
        ops.score_thresholds(levels)                       # refuses a level outside (0, 1) and more than four of them
        if not isinstance(best_of_k, (bool, np.bool_)):
            raise ValueError("TimedScoreSpec: best_of_k must be True or False, got %r" % (best_of_k,))
        if isinstance(pending, (bool, np.bool_)) or not isinstance(pending, (int, np.integer)) or \
                not 1 <= int(pending) <= ops.SCORE_MAX_PENDING:
            raise ValueError("TimedScoreSpec: pending must be an integer in [1, %d], got %r"
                             % (ops.SCORE_MAX_PENDING, pending))
        return super().__new__(cls, levels, bool(best_of_k), int(pending))

    @property
    def thresholds(self):
        """The d2 thresholds of the levels, -2 ln(1 - p)."""
        return ops.score_thresholds(self.levels)


def observed_inputs(obs_abs, num_peds=None, out=None):
    """obs_abs (N,T_obs,V,2) absolute positions (the data.pad_batch layout, any strides; float32 or float64) ->
    (x (N,2,T_obs,V), adj (N,T_obs,V,V), obs_last (N,V,2)), float32.  Relative coordinates as the reference dataset
    builds them (utils.py:153-158): rel[:,0] = 0, rel[:,t] = obs[:,t] - obs[:,t-1], taken in the input's precision and
    then rounded to float32; the graphs from the adj_build kernel.

    The graph weights are 1 / |rel_h - rel_k| and 0 where two displacements are equal, so they are not continuous in
    rel: pedestrians walking in step have equal displacements when they are taken from the dataset's float64 positions
    and rounded, while float32 differences of float32 positions differ by an ulp of the position -- a weight of ~1e6
    instead of 0.  Pass float64 positions, as the reference dataset holds them, to get the reference's graphs
    (sample_test does).
    `out` = (rel (N,T,V,2) float32, nodes (N,T,V,2), adj (N,T,V,V)) contiguous buffers to fill (graph capture)."""
    require_gpu(obs_abs)
    if obs_abs.dim() != 4 or obs_abs.shape[3] != 2:
        raise ValueError("observed_inputs: obs_abs (N,T_obs,V,2) expected, got %s" % (tuple(obs_abs.shape),))
    if obs_abs.dtype not in (torch.float32, torch.float64):
        obs_abs = obs_abs.to(torch.float32)
    n, t, v, _ = obs_abs.shape
    if out is None:
        rel = torch.empty((n, t, v, 2), device=obs_abs.device, dtype=torch.float32)
        nodes_adj = None
    else:
        rel, nodes, adj = out
        nodes_adj = (nodes, adj)
    rel[:, 0].zero_()
    if obs_abs.dtype == torch.float32:
        torch.sub(obs_abs[:, 1:], obs_abs[:, :-1], out=rel[:, 1:])
    else:
        rel[:, 1:].copy_(obs_abs[:, 1:] - obs_abs[:, :-1])
    nodes, adj = ops.adj_build(rel.permute(0, 2, 3, 1), num_peds, out=nodes_adj)      # (N,V,2,T) view
    return nodes.permute(0, 3, 1, 2), adj, obs_abs[:, -1].to(torch.float32)


@contextlib.contextmanager
def eval_mode(model):
    """The model in eval mode inside the block, its own mode again after it (after an exception too)."""
    was = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was)


class Predictor:
    """K sampled trajectories per pedestrian from observed absolute tracks, for a whole batch of scenes."""

    def __init__(self, model, k=20, risk=None, keep_samples=True, calibration=None):
        """calibration: a calibrate.Calibration (or None) -- one launch of ops.calib_apply between the model and the
        sampler shifts the two log-sigma channels of the model output by the calibration's per-step shift, so the
        samples, the risk counts and Prediction.v_pred (what a live score or ops.dist_metrics judge) are the calibrated
        ones; the mean is untouched.  `self.shift` is the (P,) float32 device tensor the launch reads, one of the static
        buffers of a captured chain.  With None nothing is launched.
        risk: a RiskSpec -- every prediction also reduces its K samples to conflict / zone counts on the device
        (ops.sample_risk, same draws), left at `self.risk` (an ops.Risk) by predict() and by every replay; `self.zones`
        is the device tensor of rectangles the reducer reads, which a caller may overwrite between replays.
        keep_samples=False (with risk only): the samples themselves are not written, Prediction.samples is
        (0,N,P,V,2)."""
        self.model = model
        self.k = int(k)
        if risk is not None:
            risk = RiskSpec(*risk)
            if risk.radius is None and risk.zones is None:
                raise ValueError("Predictor: risk needs a radius or zones")
        elif not keep_samples:
            raise ValueError("Predictor: keep_samples=False without risk leaves nothing to return")
        self.spec = risk
        self.keep_samples = bool(keep_samples)
        self.risk = None
        self.zones = None
        self.calibration = calibration
        self.shift = None
        if calibration is not None and len(calibration.shift) != model.pred_seq_len:
            raise ValueError("Predictor: the calibration holds %d steps, the model predicts %d"
                             % (len(calibration.shift), model.pred_seq_len))

    def _shift(self, dev):
        """The static device tensor of the calibration's shift (None without a calibration)."""
        if self.shift is None and self.calibration is not None:
            self.shift = torch.from_numpy(np.ascontiguousarray(self.calibration.shift, dtype=np.float32)).to(dev)
        return self.shift

    def _zones(self, n, dev):
        """The static device tensor of the spec's rectangles, (Z,4) or (n,Z,4)."""
        if self.zones is None and self.spec.zones is not None:
            self.zones = ops.risk_zones(self.spec.zones, n, dev)[0]
        return self.zones

    def _forward(self, obs_abs, peds, seed, noise, seed_dev=None, bufs=None, outs=(None, None), risk_out=None):
        x, adj, obs_last = observed_inputs(obs_abs, peds, bufs)
        y, _ = self.model(x, adj, peds)
        if self.calibration is not None:
            y = ops.calib_apply(y, self._shift(y.device))
        keep = self.keep_samples
        samples, mean = ops.sample_trajectories(y, obs_last, peds, self.k if keep else 0, noise if keep else None,
                                                seed, seed_dev, *outs)
        if self.spec is not None:
            self.risk = ops.sample_risk(y, obs_last, peds, self.k, self.spec.radius, self._zones(y.shape[0], y.device),
                                        noise, seed, seed_dev, self.spec.pairs, risk_out)
        return Prediction(samples, mean, y)

    @torch.no_grad()
    def predict(self, obs_abs, num_peds=None, seed=0, noise=None):
        """obs_abs (N,T_obs,V,2) device tensor, num_peds (N,) or None, noise (K,N,P,V,2) standard normals or None
        (the kernel's Philox stream keyed by `seed`).  Runs the model in eval mode and restores its mode."""
        require_gpu(obs_abs)
        peds = peds_arg(num_peds, obs_abs.shape[0], obs_abs.device)
        with eval_mode(self.model):
            return self._forward(obs_abs, peds, seed, noise)

    def _chain_buffers(self, n, v, dev):
        """The chain's static buffers for n scenes padded to v pedestrians: (rel, nodes, adj) that observed_inputs
        fills, (samples, mean) that the sampler fills and, with a RiskSpec, the Risk that the reducer fills."""
        t_obs, p = self.model.seq_len, self.model.pred_seq_len
        f32 = dict(device=dev, dtype=torch.float32)
        risk = None
        if self.spec is not None:
            zones = self._zones(n, dev)
            risk = ops.risk_buffers(n, p, v, self.k, self.spec.radius, 0 if zones is None else zones.shape[-2],
                                    self.spec.pairs, dev)
        return ((torch.empty((n, t_obs, v, 2), **f32), torch.empty((n, t_obs, v, 2), **f32),
                 torch.empty((n, t_obs, v, v), **f32)),
                (torch.empty((self.k if self.keep_samples else 0, n, p, v, 2), **f32),
                 torch.empty((n, p, v, 2), **f32)), risk)

    @torch.no_grad()
    def capture_chain(self, obs, peds, seed_dev, warmup=2, pre=None, post=None):
        """Capture ONE graph on the static obs (N,T_obs,V,2), peds (N,) int32 and seed_dev (1,) int64: [pre() ->]
        observed_inputs -> fused forward -> stg_sample_trajectories, the model in eval mode, the seed read from
        seed_dev (and stg_sample_risk into the static `self.risk` with a RiskSpec).  `pre` (optional callable) runs
        inside the graph ahead of the chain -- the live predictors' push launch, which fills obs and peds; `post`
        (optional callable) is given the chain's Prediction and runs inside the graph behind it -- the live predictors'
        score launch; both run in the warm-up too.  Returns (graph, the static Prediction, the
        chain's own buffers): every buffer the graph reads or writes has to live as long as the graph is replayed -- a
        freed one would go back to the caching allocator while the graph still writes it."""
        n, _, v, _ = obs.shape
        bufs, outs, risk = self._chain_buffers(n, v, obs.device)
        self._shift(obs.device)                             # (copied to the device ahead of the capture)

        def step():
            if pre is not None:
                pre()
            r = self._forward(obs, peds, 0, None, seed_dev, bufs, outs, risk)
            if post is not None:
                post(r)
            return r
        with eval_mode(self.model):
            graph, res = graphs.warm_capture(step, warmup)
        return graph, res, (bufs, outs, risk, self.zones, self.shift)

    def capture(self, n, v, num_peds, dtype=torch.float32, warmup=2):
        """Capture ONE graph on static buffers for batches of n scenes padded to v pedestrians, positions of `dtype`
        (see observed_inputs): relative coordinates -> adj_build -> fused forward -> stg_sample_trajectories, the seed
        read from a device tensor.  num_peds: (n,)
        device tensor (no host->device copy inside a graph); its values are copied into the graph's own buffer.
        Returns replay(obs_abs, num_peds=None, seed=None) -> Prediction on the static outputs (overwritten by the
        next replay); the arguments are copied into the static buffers outside the graph, None keeps the last one."""
        if not (torch.is_tensor(num_peds) and num_peds.is_cuda):
            raise ValueError("capture() needs num_peds as a device tensor (no host->device copies in a graph)")
        dev = num_peds.device
        peds = peds_arg(num_peds, n, dev).clone()
        obs = torch.zeros((n, self.model.seq_len, v, 2), device=dev, dtype=dtype)
        seed_dev = torch.zeros(1, device=dev, dtype=torch.int64)
        graph, res, chain = self.capture_chain(obs, peds, seed_dev, warmup)
        self._graph = graph
        static = (obs, peds, seed_dev, chain)          # (alive as long as replay())

        def replay(obs_abs, num_peds=None, seed=None):
            obs_s, peds_s, seed_s = static[:3]
            obs_s.copy_(obs_abs)
            if num_peds is not None:
                peds_s.copy_(torch.as_tensor(num_peds).reshape(-1))
            if seed is not None:
                seed_s.fill_(seed_i64(seed))
            graph.replay()
            return res
        return replay


def _displacement_errors(pred, trgt):
    """metrics.ade / fde arithmetic (metrics.py:21-53) for every sample and pedestrian: float32 differences and
    squares, float64 square root and sums.  pred (K,P,V,2), trgt (P,V,2) -> (ade (K,V), fde (K,V))."""
    d = pred - trgt[None]
    err = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float64))       # (K,P,V)
    return err.sum(axis=1) / err.shape[1], err[:, -1]


@torch.no_grad()
def sample_test(model, windows, k=20, batch_size=64, seed=0, noise_fn=None, calibration=None):
    """test.test() (test.py:18-127) over data.SceneWindows, batch_size windows per launch chain.  Returns (ade, fde,
    raw): raw[step] (1-based, one per window) = {'obs': (T_obs,V_i,2), 'trgt': (P,V_i,2), 'pred': [K x (P,V_i,2)]}
    float32 numpy arrays as test.py:87-105 builds them; ade / fde the best-of-k means over all pedestrians.  The draws
    come from the kernel's Philox stream keyed by seed + batch index, or from noise_fn(batch_index, (k,N,P,V,2)) ->
    standard normals (as in trainer.evaluate_ade_fde_device).  calibration: a calibrate.Calibration the Predictor
    applies ahead of the sampler (None: nothing is launched)."""
    pred = Predictor(model, k, calibration=calibration)
    dev = next(model.parameters()).device
    t_obs = model.seq_len
    raw, ades, fdes, step = {}, [], [], 0
    for b, lo in enumerate(range(0, len(windows), batch_size)):
        idx = np.arange(lo, min(len(windows), lo + batch_size))
        obs_rel, pred_rel, obs_abs, _, counts = data.pad_batch(windows, idx, obs_len=t_obs)
        n, _, v, _ = obs_abs.shape
        obs64 = np.zeros(obs_abs.shape)                    # the dataset's float64 positions (see observed_inputs)
        for j, i in enumerate(idx):
            s0, e0 = windows.seq_start_end[i]
            obs64[j, :, :e0 - s0] = np.transpose(windows.seq[s0:e0, :, :t_obs], (2, 0, 1))
        noise = noise_fn(b, (k, n, pred_rel.shape[1], v, 2)) if noise_fn is not None else None
        r = pred.predict(torch.from_numpy(obs64).to(dev), torch.from_numpy(counts).to(dev), seed + b, noise)
        samples = r.samples.cpu().numpy()
        # nodes_rel_to_nodes_abs (metrics.py:66-75) of the observed / target displacements from the first / last
        # observed position, as test.py:73-79 calls it
        x0, xl = obs_abs[:, 0].astype(np.float64), obs_abs[:, -1].astype(np.float64)
        obs = (np.cumsum(obs_rel, axis=1, dtype=np.float32) + x0[:, None]).astype(np.float32)
        trgt = (np.cumsum(pred_rel, axis=1, dtype=np.float32) + xl[:, None]).astype(np.float32)
        for j in range(n):
            c = int(counts[j])
            step += 1
            s = np.ascontiguousarray(samples[:, j, :, :c])
            raw[step] = {"obs": np.ascontiguousarray(obs[j, :, :c]), "trgt": np.ascontiguousarray(trgt[j, :, :c]),
                         "pred": [s[kk] for kk in range(k)]}
            a, f = _displacement_errors(s, raw[step]["trgt"])
            ades += a.min(axis=0).tolist()
            fdes += f.min(axis=0).tolist()
    return sum(ades) / len(ades), sum(fdes) / len(fdes), raw


@torch.no_grad()
def distribution_test(model, windows, k=20, batch_size=64, seed=0, noise_fn=None, levels=(0.5, 0.9, 0.99),
                      kde_floor=20.0, calibration=None):
    """What sample_test cannot say about a test set: whether the predicted Gaussians are calibrated
    (Mahalanobis distance, NLL, ellipse coverage, the larger eigenvalue), how likely the truth is under the K samples
    (KDE-NLL) and how well a scene as a whole is predicted (joint ADE / FDE).  The batching and the draws are
    sample_test's (seed + batch index, or noise_fn) and the truth is its `trgt`; one Predictor.predict and one
    ops.dist_metrics launch per batch, the sums kept on the device: nothing comes back to the host but the summary and
    the per-pedestrian errors.  Returns (metrics.DistSummary, ade, fde): the best-of-K errors of every pedestrian,
    float64 numpy arrays in sample_test's order, in the arithmetic sample_test evaluates on the host (the kernel's
    ade_ref / fde_ref: float32 differences and squares, float64 root and sum); the summary's .ade / .fde are their means
    summed as sample_test sums them, so the two functions report the same ADE / FDE at the same seed, to the last bit.
    calibration: a calibrate.Calibration the Predictor applies ahead of the sampler, so the Gaussians judged are the
    calibrated ones (None: nothing is launched)."""
    from . import metrics
    pred = Predictor(model, k, calibration=calibration)
    dev = next(model.parameters()).device
    t_obs = model.seq_len
    per_h, traj, ades, fdes = None, None, [], []
    for b, lo in enumerate(range(0, len(windows), batch_size)):
        idx = np.arange(lo, min(len(windows), lo + batch_size))
        _, pred_rel, obs_abs, _, counts = data.pad_batch(windows, idx, obs_len=t_obs)
        n, _, v, _ = obs_abs.shape
        obs64 = np.zeros(obs_abs.shape)                    # the dataset's float64 positions (see observed_inputs)
        for j, i in enumerate(idx):
            s0, e0 = windows.seq_start_end[i]
            obs64[j, :, :e0 - s0] = np.transpose(windows.seq[s0:e0, :, :t_obs], (2, 0, 1))
        noise = noise_fn(b, (k, n, pred_rel.shape[1], v, 2)) if noise_fn is not None else None
        peds = torch.from_numpy(counts).to(dev)
        r = pred.predict(torch.from_numpy(obs64).to(dev), peds, seed + b, noise)
        xl = obs_abs[:, -1].astype(np.float64)             # sample_test's trgt
        trgt = (np.cumsum(pred_rel, axis=1, dtype=np.float32) + xl[:, None]).astype(np.float32)
        ref = (torch.empty((n, v), device=dev, dtype=torch.float64), torch.empty((n, v), device=dev, dtype=torch.float64))
        m = ops.dist_metrics(r.v_pred, r.mean, r.samples, torch.from_numpy(trgt).to(dev), peds, kde_floor,
                             ref_errors=ref)
        sums = metrics.dist_sums(m, peds, levels)
        per_h, traj = (sums if per_h is None else (per_h + sums[0], traj + sums[1]))
        ok = torch.arange(v, device=dev)[None, :] < peds[:, None]
        ades.append(ref[0][ok])
        fdes.append(ref[1][ok])
    ades, fdes = torch.cat(ades).cpu().numpy(), torch.cat(fdes).cpu().numpy()
    s = metrics.summary_of_sums(per_h, traj, levels)
    return (s._replace(ade=sum(ades.tolist()) / len(ades), fde=sum(fdes.tolist()) / len(fdes)), ades, fdes)
