"""Frame-by-frame prediction over a whole recording (frames.predict_recording): at every frame, K sampled future
trajectories for every pedestrian tracked over the last obs_seq_len frames.

    python -m social_stgcnn_amd.predict_frames --checkpoint DIR --recording FILE [--ksteps 20] [--seed 0]
                                               [--min_peds 1] [--delim tab] [--radius R]
                                               [--zones x0,y0,x1,y1 ...] [--min_seen M] [--max_gap G]
                                               [--step TICKS [--max_dt D] [--history R] [--max_peds V]
                                                [--score [--pending N]]
                                                [--harvest_timed WINDOWS [--settle D] [--harvest_out FILE.npz]]
                                                [--associate_timed GATE[,GATE_NEW[,MAX_AGE]]]
                                                [--associate_filtered SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS
                                                                      [,GATE_MAX[,MAX_AGE]]]]]]
                                               [--associate GATE[,GATE_NEW[,MAX_MISS]] [--max_peds V]]
                                               [--harvest WINDOWS [--harvest_out FILE.npz] [--max_peds V]]
                                               [--calibration FILE.npz] --out preds.npz

DIR is a checkpoint directory in the reference's layout (args.pkl and val_best.pth, as social_stgcnn_amd.test reads
it); FILE a recording in the ETH/UCY text format (<frame> <ped> <x> <y>).  The .npz holds, one entry per frame scene:
frame (N,) frame numbers, ids (N,V) int64 (-1 in padded slots), num_peds (N,), mean (N,P,V,2) the zero-noise
trajectories and samples (K,N,P,V,2), float32, zeros in padded slots.  With --radius and / or --zones it also holds
the counts of ops.sample_risk over each frame's K samples, aligned with the frames: risk_k, and risk_conflict (N,P,V),
risk_conflict_any (N,V), risk_partner (N,V), risk_pair (N,V,V) for a radius, risk_zones (Z,4), risk_zone_any (N,P,Z),
risk_zone_count (N,P,Z), risk_ped_zone (N,V,Z) for zones.

--min_seen M and / or --max_gap G predict partially observed tracks too (frames.TrackRule; the other one defaults to
obs_seq_len / 0): a pedestrian seen now, in at least M of the last obs_seq_len frames and with no run of more than G
missed frames between two seen ones; the missed frames are filled.  The .npz then also holds seen (N,V) int32: bit t set
= observed t frames ago, so a caller can tell a filled history from an observed one.

--step TICKS takes the frame column for the TIME of a detection, in integer ticks, and TICKS for the model's step (10 for
the ETH/UCY recordings; frames.TimeRule, with --max_dt and --history): the recording may then come at the tracker's own
rate, with jitter and dropped frames.  Every distinct frame number is one push of a captured frames.FramePredictor, which
predicts from the tracks resampled at t - k * TICKS; the .npz holds one entry per push with at least --min_peds
pedestrians, padded to the largest scene (at most --max_peds, default 128: the smallest ids), and besides the arrays
above `seen` and `time` (N,) int64, the pushes' times (`frame` holds the same numbers as float64).  The sampler's seed is
--seed + the push's index.  Not together with --radius / --zones.  Where a recording skips a frame number the two rules
differ: the frame-index rule makes neighbours of frames 20 ticks apart, the timed rule sees a gap.
With --score every push also grades the earlier predictions against the tracks that followed (predict.TimedScoreSpec with
--pending record rows, DESIGN.md 5.25: the prediction made at t is graded at t + h * TICKS, the truth interpolated as the
window is) and the .npz also holds the running summary at the end of the recording (frames.score_summary), per horizon
score_count, score_err, score_d2, score_nll, score_best (P,) and score_coverage (P,Q) at score_levels (Q,), and
score_trajectories, score_ade, score_fde, score_ade_mean, score_fde_mean over the fully observed trajectories, with
score_evictions, the records that left the ring before their last instant.

--associate GATE[,GATE_NEW[,MAX_MISS]] ignores the id column: every distinct frame number is one push of positions only,
rows in file order, through a captured frames.FramePredictor(associate=frames.AssociateSpec(...)), which gives every
detection its track id on the device.  The .npz holds one entry per push with at least --min_peds
pedestrians, padded to the largest scene (at most --max_peds), its ids the assigned track ids, and assoc_ids (M,) int64:
the assigned id of every row of the recording, in file order.  Not together with --step or --radius / --zones.

--harvest WINDOWS pushes every distinct frame number through a captured frames.FramePredictor(harvest=
frames.HarvestSpec(WINDOWS)), which also keeps the training windows the tracks complete (the windows of
data.load_windows over the same file, in order).  The .npz holds one entry per push with at least --min_peds pedestrians;
--harvest_out FILE.npz gets the windows: seq_rel (R,2,T) float32, num_peds (W,), tags (W,2) = (0, push index) and
dropped_full.  Not together with --step, --associate or --radius / --zones.

--step TICKS --harvest_timed WINDOWS is the same on a timed feed (frames.TimedHarvestSpec(WINDOWS, settle=D), DESIGN.md
5.27): the tracks are resampled on the step grid anchored at the first push's time, an instant resolved --settle D ticks
after it (default max_dt - 1).  --harvest_out FILE.npz then holds seq_rel, num_peds, tags (W,2) = (0, grid index of the
window's last frame), g0 (that frame's time is g0 + index * TICKS), skipped (grid instants passed over) and
dropped_full.  Not together with --harvest or --associate.

--step TICKS --associate_timed GATE[,GATE_NEW[,MAX_AGE]] ignores the id column on a timed feed: every distinct frame
number is one timed push of positions only, rows in file order, through a captured frames.FramePredictor(time=...,
associate=frames.TimedAssociateSpec(...)) (MAX_AGE in ticks, default 0).  The .npz is --step's, its ids
the assigned track ids, and assoc_ids (M,) int64 as with --associate.  It goes together with --score and
--harvest_timed; not with --associate.

--step TICKS --associate_filtered SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS[,GATE_MAX[,MAX_AGE]]]] is the same for a
noisy detector: associate=frames.FilteredAssociateSpec(...), a constant-velocity Kalman filter per track
and a gate of GATE_SIGMAS standard deviations of the predicted position, at most GATE_MAX.  The same arrays; the scenes
hold the detections as reported.  Not with --associate or --associate_timed.

--calibration FILE.npz (what `python -m social_stgcnn_amd.test --calibrate ... --save_calibration` writes; DESIGN.md
5.32) goes with every mode: the predictor shifts the log sigmas of the model output by the file's per-step factors ahead
of the sampler, so the samples, the risk counts and the score are the calibrated ones; the means do not change.
"""
import argparse
import os
import re

import numpy as np
import torch

from . import data
from .calibrate import Calibration
from .frames import (AssociateSpec, FilteredAssociateSpec, FramePredictor, HarvestSpec, TimedAssociateSpec, TimedHarvestSpec, TimeRule, TrackRule,
                     predict_recording, score_summary, sorted_rows)
from .model import social_stgcnn
from .predict import RiskSpec, TimedScoreSpec
from .trainer import load_checkpoint, load_pickle


def build_parser():
    p = argparse.ArgumentParser(description="Per-frame trajectory prediction over a recording (on the device).")
    p.add_argument("--checkpoint", required=True, help="checkpoint directory (args.pkl, val_best.pth)")
    p.add_argument("--recording", required=True, help="recording: <frame> <ped> <x> <y> rows")
    p.add_argument("--ksteps", type=int, default=20, help="samples per pedestrian")
    p.add_argument("--seed", type=int, default=0, help="seed of the device sampler")
    p.add_argument("--min_peds", type=int, default=1, help="skip frames with fewer pedestrians")
    p.add_argument("--delim", default="tab", help="column delimiter of the recording (tab, space or a character)")
    p.add_argument("--radius", type=float, default=None,
                   help="also count the samples in which two pedestrians come closer than this (risk_* arrays)")
    p.add_argument("--zones", nargs="+", default=None, metavar="x0,y0,x1,y1",
                   help="also count the samples in which each rectangle is occupied (risk_* arrays)")
    p.add_argument("--min_seen", type=int, default=None,
                   help="predict a pedestrian seen in at least this many of the last obs_seq_len frames (seen array)")
    p.add_argument("--max_gap", type=int, default=None,
                   help="... with at most this many missed frames in a row between two seen ones (seen array)")
    p.add_argument("--step", type=int, default=None,
                   help="the model's step in ticks of the frame column: predict at every frame number, from the tracks "
                        "resampled in time (seen and time arrays)")
    p.add_argument("--max_dt", type=int, default=None, help="with --step: interpolate between samples at most this many "
                                                            "ticks apart (default: the step)")
    p.add_argument("--history", type=int, default=96, help="with --step: samples kept per track")
    p.add_argument("--max_peds", type=int, default=128,
                   help="with --step or --associate: the widest scene (the smallest ids are kept)")
    p.add_argument("--score", action="store_true",
                   help="with --step: grade the predictions against the tracks that follow (score_* arrays)")
    p.add_argument("--pending", type=int, default=128,
                   help="with --score: record rows kept (at least pushes per step x pred_seq_len)")
    p.add_argument("--associate", default=None, metavar="GATE[,GATE_NEW[,MAX_MISS]]",
                   help="ignore the id column: associate the detections to tracks on the device (assoc_ids array)")
    p.add_argument("--associate_timed", default=None, metavar="GATE[,GATE_NEW[,MAX_AGE]]",
                   help="with --step: ignore the id column and associate the timed detections to tracks on the device, "
                        "a track forgotten MAX_AGE ticks after its last match (assoc_ids array; not with --associate)")
    p.add_argument("--associate_filtered", default=None,
                   metavar="SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS[,GATE_MAX[,MAX_AGE]]]]",
                   help="with --step: --associate_timed for a noisy detector, a Kalman filter per track and a gate that "
                        "follows the predicted uncertainty (not with --associate or --associate_timed)")
    p.add_argument("--harvest", type=int, default=None, metavar="WINDOWS",
                   help="push the recording frame by frame and keep up to this many of the training windows its tracks "
                        "complete (not with --step, --associate or --radius / --zones)")
    p.add_argument("--harvest_out", default=None, metavar="FILE.npz",
                   help="with --harvest or --harvest_timed: write the harvested windows (seq_rel, num_peds, tags) here")
    p.add_argument("--harvest_timed", type=int, default=None, metavar="WINDOWS",
                   help="with --step: keep up to this many of the training windows the timed tracks complete on the "
                        "step grid (not with --harvest or --associate)")
    p.add_argument("--settle", type=int, default=None, metavar="D",
                   help="with --harvest_timed: resolve a grid instant D ticks after it (0 .. max_dt - 1; default "
                        "max_dt - 1)")
    p.add_argument("--calibration", default=None, metavar="FILE.npz",
                   help="apply the per-step covariance factors of this file (calibrate.Calibration.save) ahead of the "
                        "sampler")
    p.add_argument("--out", required=True, help="output .npz")
    # a rectangle may begin with a negative coordinate: "-1,-1,1,1" is a value, not an option
    p._negative_number_matcher = re.compile(r"^-[0-9.][0-9.,eE+-]*$")
    return p


def parse_zones(specs):
    """['x0,y0,x1,y1', ...] -> (Z,4) float32."""
    out = []
    for s in specs:
        parts = s.split(",")
        if len(parts) != 4:
            raise ValueError("--zones: x0,y0,x1,y1 expected, got %r" % s)
        out.append([float(x) for x in parts])
    return np.asarray(out, dtype=np.float32)


def load_model(exp_path, device):
    args = load_pickle(os.path.join(exp_path, "args.pkl"))
    model = social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                          seq_len=args.obs_seq_len, kernel_size=args.kernel_size, pred_seq_len=args.pred_seq_len)
    load_checkpoint(model, os.path.join(exp_path, "val_best.pth"))
    return model.to(device).eval()


def predict_timed(model, rows, time, k=20, seed=0, min_peds=1, tracks=None, max_peds=128, score=None, harvest=None,
                  associate=None, calibration=None):
    """Every distinct frame number of `rows`, taken as a time in ticks, pushed through ONE captured timed
    FramePredictor -> a dict of host arrays, one entry per push whose scene holds at least min_peds pedestrians.
    associate: a frames.TimedAssociateSpec -- the id column is ignored, the rows of a push go in file order, and the dict
    also holds assoc_ids (M,) int64, the assigned id of every row.
    score: a predict.TimedScoreSpec -- the dict also holds the summary of the running totals as score_* arrays.
    harvest: a frames.TimedHarvestSpec -- the result is (that dict, the dict of what the run harvested: seq_rel
    (R,2,T_all) float32, num_peds (W,) int32, tags (W,2) int32 = (0, grid index), g0, skipped, dropped_full)."""
    if associate is None:
        frames, fs, ids, xy = sorted_rows(rows)
    else:                                                    # no id is looked at: the rows of a frame in file order
        rows = np.asarray(rows, dtype=np.float64)
        frames = np.unique(rows[:, 0])
        f_idx = np.searchsorted(frames, rows[:, 0])
        order = np.argsort(f_idx, kind="stable")
        fs = np.searchsorted(f_idx[order], np.arange(len(frames) + 1))
        xy = np.ascontiguousarray(rows[order, 2:4])
        assoc_ids = np.full(len(rows), -1, np.int64)
    if np.any(frames != np.round(frames)):
        raise ValueError("--step: the frame column must hold integer ticks")
    ticks = frames.astype(np.int64)
    m_max = max(1, int(np.diff(fs).max()) if len(frames) else 1)
    fp = FramePredictor(model, k=k, obs_len=model.seq_len, max_peds=max_peds, max_detections=m_max, tracks=tracks,
                        time=time, score=score, harvest=harvest, associate=associate, calibration=calibration)
    replay = fp.capture()
    keep = {name: [] for name in ("time", "ids", "num_peds", "mean", "samples", "seen")}
    for f, t in enumerate(ticks.tolist()):
        out = replay(None if associate is not None else ids[fs[f]:fs[f + 1]], xy[fs[f]:fs[f + 1]], t=t, seed=seed + f)
        if associate is not None:
            assoc_ids[order[fs[f]:fs[f + 1]]] = fp.det_ids.cpu().numpy()
        n = int(out.num_peds.item())
        if n < min_peds:
            continue
        for name, x in (("time", np.int64(t)), ("ids", out.ids), ("num_peds", np.int32(n)), ("mean", out.mean),
                        ("samples", out.samples), ("seen", fp.seen)):
            keep[name].append(x.cpu().numpy() if torch.is_tensor(x) else x)
    v = max(1, max(keep["num_peds"], default=0))
    p = model.pred_seq_len
    empty = dict(time=np.zeros(0, np.int64), ids=np.zeros((0, v), np.int64), num_peds=np.zeros(0, np.int32),
                 mean=np.zeros((0, p, v, 2), np.float32), samples=np.zeros((0, fp.k, p, v, 2), np.float32),
                 seen=np.zeros((0, v), np.int32))
    res = {name: np.stack(x) if x else empty[name] for name, x in keep.items()}
    res.update(ids=res["ids"][:, :v], seen=res["seen"][:, :v], mean=res["mean"][:, :, :v],
               samples=np.ascontiguousarray(np.moveaxis(res["samples"], 0, 1)[:, :, :, :v]))
    res["frame"] = res["time"].astype(np.float64)
    if associate is not None:
        res["assoc_ids"] = assoc_ids
    if score is not None:
        summary = score_summary(*fp.score_totals, score.levels)
        res.update({"score_" + name: np.asarray(x)[0] for name, x in zip(summary._fields[:-1], summary[:-1])})
        res["score_levels"] = np.asarray(score.levels, np.float64)
        res["score_evictions"] = fp.score_evictions.cpu().numpy()[0]
    if harvest is not None:
        log = fp.harvest
        n_w, n_r, dropped = log.counts()
        start = log.win_start[:n_w + 1].cpu().numpy()
        clock = fp.harvest_clock.cpu().numpy()[0]
        return res, dict(seq_rel=log.rel_all[:n_r].cpu().numpy(), num_peds=np.diff(start).astype(np.int32),
                         tags=log.tags(), g0=np.int64(clock[1]), skipped=np.int64(clock[2]),
                         dropped_full=np.int32(dropped))
    return res


def parse_associate(spec):
    """'GATE[,GATE_NEW[,MAX_MISS]]' -> frames.AssociateSpec."""
    parts = spec.split(",")
    if not 1 <= len(parts) <= 3:
        raise ValueError("--associate: GATE[,GATE_NEW[,MAX_MISS]] expected, got %r" % spec)
    return AssociateSpec(float(parts[0]), float(parts[1]) if len(parts) > 1 else None,
                         int(parts[2]) if len(parts) > 2 else 0)


def parse_associate_timed(spec):
    """'GATE[,GATE_NEW[,MAX_AGE]]' -> frames.TimedAssociateSpec."""
    parts = spec.split(",")
    if not 1 <= len(parts) <= 3:
        raise ValueError("--associate_timed: GATE[,GATE_NEW[,MAX_AGE]] expected, got %r" % spec)
    return TimedAssociateSpec(float(parts[0]), float(parts[1]) if len(parts) > 1 else None,
                              int(parts[2]) if len(parts) > 2 else 0)


def parse_associate_filtered(spec):
    """'SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS[,GATE_MAX[,MAX_AGE]]]]' -> frames.FilteredAssociateSpec."""
    parts = spec.split(",")
    if not 2 <= len(parts) <= 6:
        raise ValueError("--associate_filtered: SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS[,GATE_MAX[,MAX_AGE]]]] "
                         "expected, got %r" % spec)
    return FilteredAssociateSpec(*(float(x) for x in parts[:5]), **({"max_age": int(parts[5])} if len(parts) > 5 else {}))


def check_associate_timed_args(a):
    """The refusals of --associate_timed and --associate_filtered, ahead of anything that needs the device -> None, the
    TimedAssociateSpec or the FilteredAssociateSpec."""
    if a.associate_filtered is not None:
        for other in ("associate", "associate_timed"):
            if getattr(a, other) is not None:
                raise ValueError("--associate_filtered does not go together with --%s: a feed is associated by one rule" % other)
        if a.step is None:
            raise ValueError("--associate_filtered needs --step TICKS: its tracks are aged by time")
        return parse_associate_filtered(a.associate_filtered)
    if a.associate_timed is None:
        return None
    if a.associate is not None:
        raise ValueError("--associate_timed does not go together with --associate: one ages its tracks by time, the "
                         "other by push")
    if a.step is None:
        raise ValueError("--associate_timed needs --step TICKS: its tracks are aged by time (without --step, "
                         "--associate serves)")
    return parse_associate_timed(a.associate_timed)


def predict_associated(model, rows, associate, k=20, seed=0, min_peds=1, tracks=None, max_peds=128, calibration=None):
    """Every distinct frame number of `rows` pushed without ids, rows in file order, through ONE captured
    FramePredictor(associate=...) -> a dict of host arrays: one entry per push whose scene holds at least min_peds
    pedestrians, and assoc_ids, the assigned id of every row."""
    rows = np.asarray(rows, dtype=np.float64)
    frames = np.unique(rows[:, 0])
    f_idx = np.searchsorted(frames, rows[:, 0])
    order = np.argsort(f_idx, kind="stable")
    fs = np.searchsorted(f_idx[order], np.arange(len(frames) + 1))
    m_max = max(1, int(np.diff(fs).max()) if len(frames) else 1)
    fp = FramePredictor(model, k=k, obs_len=model.seq_len, max_peds=max_peds, max_detections=m_max, tracks=tracks,
                        associate=associate, calibration=calibration)
    replay = fp.capture()
    assoc_ids = np.full(len(rows), -1, np.int64)
    names = ("frame", "ids", "num_peds", "mean", "samples") + (() if tracks is None else ("seen",))
    keep = {name: [] for name in names}
    for f in range(len(frames)):
        at = order[fs[f]:fs[f + 1]]
        out = replay(None, rows[at, 2:4], seed=seed + f)
        assoc_ids[at] = fp.det_ids.cpu().numpy()
        n = int(out.num_peds.item())
        if n < min_peds:
            continue
        for name, x in zip(names, (frames[f], out.ids, np.int32(n), out.mean, out.samples, fp.seen)):
            keep[name].append(x.cpu().numpy() if torch.is_tensor(x) else x)
    v = max(1, max(keep["num_peds"], default=0))
    p = model.pred_seq_len
    empty = dict(frame=np.zeros(0), ids=np.zeros((0, v), np.int64), num_peds=np.zeros(0, np.int32),
                 mean=np.zeros((0, p, v, 2), np.float32), samples=np.zeros((0, fp.k, p, v, 2), np.float32),
                 seen=np.zeros((0, v), np.int32))
    res = {name: np.stack(x) if x else empty[name] for name, x in keep.items()}
    res.update(ids=res["ids"][:, :v], mean=res["mean"][:, :, :v],
               samples=np.ascontiguousarray(np.moveaxis(res["samples"], 0, 1)[:, :, :, :v]))
    if tracks is not None:
        res["seen"] = res["seen"][:, :v]
    res["assoc_ids"] = assoc_ids
    return res


def check_harvest_args(a):
    """The refusals of --harvest / --harvest_out, ahead of anything that needs the device."""
    if a.harvest_timed is None:
        if a.settle is not None:
            raise ValueError("--settle needs --harvest_timed WINDOWS")
    else:
        if a.harvest is not None:
            raise ValueError("--harvest_timed does not go together with --harvest: one is indexed by time, the other "
                             "by push")
        if a.step is None:
            raise ValueError("--harvest_timed needs --step TICKS: its frames are instants of the step grid")
        if a.associate is not None:
            raise ValueError("--harvest_timed does not go together with --associate")
        if a.harvest_timed < 1:
            raise ValueError("--harvest_timed: at least one window, got %d" % a.harvest_timed)
        max_dt = a.step if a.max_dt is None else a.max_dt
        if a.settle is not None and not 0 <= a.settle <= max_dt - 1:
            raise ValueError("--settle: %d not in [0, max_dt - 1 = %d]" % (a.settle, max_dt - 1))
        return
    if a.harvest is None:
        if a.harvest_out is not None:
            raise ValueError("--harvest_out needs --harvest WINDOWS (or --harvest_timed WINDOWS)")
        return
    if a.step is not None:
        raise ValueError("--harvest does not go together with --step: a timed push is not one frame of a window")
    if a.associate is not None or a.radius is not None or a.zones is not None:
        raise ValueError("--harvest does not go together with --associate or --radius / --zones")
    if a.harvest < 1:
        raise ValueError("--harvest: at least one window, got %d" % a.harvest)


def predict_harvested(model, rows, harvest, k=20, seed=0, min_peds=1, tracks=None, max_peds=128, calibration=None):
    """Every distinct frame number of `rows` pushed through ONE captured FramePredictor(harvest=...) -> (a dict of host
    arrays, one entry per push whose scene holds at least min_peds pedestrians, and the dict of what the run harvested:
    seq_rel (R,2,T_all) float32, num_peds (W,) int32, tags (W,2) int32 = (0, push index), dropped_full)."""
    frames, fs, ids, xy = sorted_rows(rows)
    m_max = max(1, int(np.diff(fs).max()) if len(frames) else 1)
    fp = FramePredictor(model, k=k, obs_len=model.seq_len, capacity=max(1024, m_max), max_peds=max_peds,
                        max_detections=m_max, tracks=tracks, harvest=harvest, calibration=calibration)
    replay = fp.capture()
    names = ("frame", "ids", "num_peds", "mean", "samples") + (() if tracks is None else ("seen",))
    keep = {name: [] for name in names}
    for f in range(len(frames)):
        out = replay(ids[fs[f]:fs[f + 1]], xy[fs[f]:fs[f + 1]], seed=seed + f)
        n = int(out.num_peds.item())
        if n < min_peds:
            continue
        for name, x in zip(names, (frames[f], out.ids, np.int32(n), out.mean, out.samples, fp.seen)):
            keep[name].append(x.cpu().numpy() if torch.is_tensor(x) else x)
    v = max(1, max(keep["num_peds"], default=0))
    p = model.pred_seq_len
    empty = dict(frame=np.zeros(0), ids=np.zeros((0, v), np.int64), num_peds=np.zeros(0, np.int32),
                 mean=np.zeros((0, p, v, 2), np.float32), samples=np.zeros((0, fp.k, p, v, 2), np.float32),
                 seen=np.zeros((0, v), np.int32))
    res = {name: np.stack(x) if x else empty[name] for name, x in keep.items()}
    res.update(ids=res["ids"][:, :v], mean=res["mean"][:, :, :v],
               samples=np.ascontiguousarray(np.moveaxis(res["samples"], 0, 1)[:, :, :, :v]))
    if tracks is not None:
        res["seen"] = res["seen"][:, :v]
    log = fp.harvest
    n_w, n_r, dropped = log.counts()
    start = log.win_start[:n_w + 1].cpu().numpy()
    kept = dict(seq_rel=log.rel_all[:n_r].cpu().numpy(), num_peds=np.diff(start).astype(np.int32), tags=log.tags(),
                dropped_full=np.int32(dropped))
    return res, kept


def main(argv=None):
    a = build_parser().parse_args(argv)
    check_harvest_args(a)
    assoc_timed = check_associate_timed_args(a)
    if not torch.cuda.is_available():
        raise RuntimeError("social_stgcnn_amd.predict_frames needs a GPU (MI355X)")
    model = load_model(a.checkpoint, torch.device("cuda", torch.cuda.current_device()))
    rows = data.read_file(a.recording, a.delim)
    calibration = None if a.calibration is None else Calibration.load(a.calibration)
    extra = {}
    tracks = None
    if a.min_seen is not None or a.max_gap is not None:
        tracks = TrackRule(model.seq_len if a.min_seen is None else a.min_seen, 0 if a.max_gap is None else a.max_gap)
    if a.score and (a.step is None or a.associate is not None):
        raise ValueError("--score needs --step (and does not go with --associate): the records it keeps are indexed "
                         "by time")
    if a.harvest is not None:
        res, kept = predict_harvested(model, rows, HarvestSpec(a.harvest), a.ksteps, a.seed, a.min_peds, tracks,
                                      a.max_peds, calibration)
        np.savez(a.out, **res)
        if a.harvest_out is not None:
            np.savez(a.harvest_out, **kept)
        print("%d pushes with a scene, up to %d pedestrians -> %s; %d windows (%d rows) harvested, %d dropped%s"
              % (len(res["frame"]), res["ids"].shape[1], a.out, len(kept["num_peds"]), len(kept["seq_rel"]),
                 int(kept["dropped_full"]), "" if a.harvest_out is None else " -> " + a.harvest_out))
        return
    if a.associate is not None:
        if a.step is not None or a.radius is not None or a.zones is not None:
            raise ValueError("--associate does not go together with --step or --radius / --zones")
        res = predict_associated(model, rows, parse_associate(a.associate), a.ksteps, a.seed, a.min_peds, tracks,
                                 a.max_peds, calibration)
        np.savez(a.out, **res)
        print("%d pushes with a scene, up to %d pedestrians, %d track ids -> %s"
              % (len(res["frame"]), res["ids"].shape[1], int(res["assoc_ids"].max(initial=-1)) + 1, a.out))
        return
    if a.step is not None:
        if a.radius is not None or a.zones is not None:
            raise ValueError("--step does not go together with --radius / --zones")
        spec = None if a.harvest_timed is None else TimedHarvestSpec(a.harvest_timed, settle=a.settle)
        res = predict_timed(model, rows, TimeRule(a.step, a.max_dt, a.history), a.ksteps, a.seed, a.min_peds, tracks,
                            a.max_peds, TimedScoreSpec(pending=a.pending) if a.score else None, spec, assoc_timed,
                            calibration)
        if spec is not None:
            res, kept = res
            if a.harvest_out is not None:
                np.savez(a.harvest_out, **kept)
        np.savez(a.out, **res)
        print("%d pushes with a scene, up to %d pedestrians -> %s" % (len(res["time"]), res["ids"].shape[1], a.out))
        if assoc_timed is not None:
            print("%d track ids" % (int(res["assoc_ids"].max(initial=-1)) + 1))
        if spec is not None:
            print("%d windows (%d rows) harvested, %d grid instants skipped, %d dropped%s"
                  % (len(kept["num_peds"]), len(kept["seq_rel"]), int(kept["skipped"]), int(kept["dropped_full"]),
                     "" if a.harvest_out is None else " -> " + a.harvest_out))
        if a.score:
            print("scored: %d entries, %d full trajectories, ADE %.4f FDE %.4f, %d records evicted"
                  % (int(res["score_count"].sum()), int(res["score_trajectories"]), float(res["score_ade"]),
                     float(res["score_fde"]), int(res["score_evictions"])))
        return
    if a.radius is None and a.zones is None:
        scenes, pred = predict_recording(model, rows, k=a.ksteps, seed=a.seed, min_peds=a.min_peds, tracks=tracks,
                                         calibration=calibration)
    else:
        zones = parse_zones(a.zones) if a.zones is not None else None
        scenes, pred, risk = predict_recording(model, rows, k=a.ksteps, seed=a.seed, min_peds=a.min_peds,
                                               risk=RiskSpec(a.radius, zones, a.radius is not None), tracks=tracks,
                                               calibration=calibration)
        extra = {"risk_" + f: x.cpu().numpy() for f, x in zip(risk._fields[1:], risk[1:]) if x is not None}
        extra["risk_k"] = np.int32(risk.k)
        if zones is not None:
            extra["risk_zones"] = zones
    if tracks is not None:
        extra["seen"] = scenes.seen.cpu().numpy()
    np.savez(a.out, frame=scenes.frame, ids=scenes.ids.cpu().numpy(), num_peds=scenes.num_peds.cpu().numpy(),
             mean=pred.mean.cpu().numpy(), samples=pred.samples.cpu().numpy(), **extra)
    print("%d frame scenes, up to %d pedestrians -> %s" % (len(scenes.frame), scenes.ids.shape[1], a.out))


if __name__ == "__main__":
    main()
