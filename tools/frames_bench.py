#!/usr/bin/env python3
"""Per-frame prediction timings (social_stgcnn_amd.frames).  One JSON line per case.

    python tools/frames_bench.py [--pushes 2000] [--cases latency,recording] [--k 20]
    python tools/frames_bench.py --cases streams [--streams 1,8,64,256,600] [--ticks 200] [--block 0] [--no-lone]
                                 [--risk none,samples,lean]
    python tools/frames_bench.py --cases score [--streams 1,64,600] [--ticks 200]
    python tools/frames_bench.py --cases associate [--streams 1,64,600] [--ticks 200] [--associate 1.0,2.0,0]
                                 [--no-lone]
    python tools/frames_bench.py --cases associate_timed [--streams 1,64,600] [--ticks 200] [--time 10,10]
                                 [--associate_timed 1.0,2.0,0] [--no-lone] [--noise SIGMA]
    python tools/frames_bench.py --cases associate_filtered [--streams 1,64,600] [--ticks 200] [--time 10,10]
                                 [--associate_filtered 0.05,1.0] [--no-lone] [--noise SIGMA]
    python tools/frames_bench.py --cases harvest [--streams 1,64,600] [--ticks 200] [--pushes 2000]
    python tools/frames_bench.py --harvest ...          the latency and streams cases with harvest=HarvestSpec(...)
    python tools/frames_bench.py --tracks 2,2 ...       every case under frames.TrackRule(2, 2) (the *_rule kernels)
    python tools/frames_bench.py --eager ...            the latency and streams cases (the yardstick too) through push()
                                                        in the place of the captured replay: every launch enqueued by
                                                        the host, so the host's own work per push is in the figure
    python tools/frames_bench.py --time 10,10 ...       the latency, streams, score and harvest cases on timestamped pushes
                                                        (frames.TimeRule(10, history=--history), stg_track_push_timed):
                                                        a model step is 10 ticks and the feed is upsampled 10x by linear
                                                        interpolation, one push per tick (--time STEP: not upsampled)

  latency    the captured FramePredictor (ONE graph: stg_track_push -> observed_inputs -> forward -> sampler) pushed
             every frame of a recording in a loop, --pushes timed pushes after a warm-up.  Host clock around staging +
             replay + synchronise: what a caller with host detections waits per frame.  p50 / p90 / mean in ms, at
             max_peds 32 and 128 (biwi_eth, up to 20 pedestrians) and 128 (students001, up to 73).
  recording  predict_recording (batches of 64 frame scenes) on each test recording: frames/s, host clock around the
             call and a synchronise, after one warm-up call.
  streams    NS streams in ONE captured StreamsPredictor graph (stg_track_push_streams -> forward -> sampler), the six
             test recordings cycled with staggered starts, every stream pushed every tick, max_peds 128: tick p50 / p90
             (host clock around staging + replay + synchronise) and aggregate frames/s.  Beside it the yardstick: the
             same per-stream sequences through NS lone captured FramePredictors one after another (each push timed as
             the latency case times it; a tick is the sum of its NS pushes).  --block picks the push workgroup size
             (0: the default); --no-lone skips the yardstick.  --risk: the modes to time -- none (the default: no
             reducer), samples (RiskSpec(0.5, three rectangles): stg_sample_risk after the sampler) and lean (the same
             with keep_samples=False); result_mb is what a tick leaves for the caller (samples + mean + counts).

  score      the streams case with and without score=ScoreSpec() (stg_score_push_streams behind the sampler, inside the
             graph) at NS = 1, 64 and 600 (or --streams), no yardstick: tick p50 / p90 of both, the difference, what
             the score records hold on the device (state_mb) and the running summary at the last tick.  With --time
             both sides are the timed predictors and the spec is TimedScoreSpec(pending=--pending)
             (stg_score_push_streams_timed, records indexed by time); `evictions` counts the records lost to the ring.

  associate  the streams case with and without associate=AssociateSpec(...) (stg_associate_streams ahead of the push
             launch, inside the graph; ticks of (None, xy)) at NS = 1, 64 and 600 (or --streams), no yardstick: tick p50 /
             p90 of both and host_p50_ms, the host's share (staging + the replay call, before the synchronise); then, on
             crowds_zara01 and students003, a captured FramePredictor with score=ScoreSpec() fed the recording's own ids
             and one fed none: best-of-K ADE / FDE of both, and the share of wrong links (a detection whose recorded id
             was in the previous push and whose assigned id is not the one that pedestrian had then).

  associate_timed  the associate case on timestamped pushes (--time STEP,UP, default 10,10: ten pushes per
             model step): the timed streams case with and without associate=TimedAssociateSpec(...)
             (stg_associate_streams_timed ahead of the timed push launch, inside the graph) at NS = 1, 64 and 600 (or
             --streams); then, on crowds_zara01 upsampled 4x (step 4), a captured timed FramePredictor with
             score=TimedScoreSpec() fed the recording's own ids and one fed none: best-of-K ADE / FDE of both and the
             share of wrong links.

  associate_filtered  the associate_timed case under associate=FilteredAssociateSpec(...) (DESIGN.md 5.29;
             stg_associate_streams_filtered).  --noise SIGMA adds seeded Gaussian noise of that many metres to every
             detection of the feeds of both timed association cases (rounded to 4 decimals, as a recording is), so that
             both rules can be measured on the same noisy feed.

  harvest    the window harvest: the latency case (students001, max_peds 128) and the streams case at
             NS = 1, 64 and 600 (or --streams), each with and without harvest=HarvestSpec(...) sized so that the log never
             fills (one window per stream and tick, 32 rows each): p50 / p90 of both, the difference, and what the log
             holds at the end.  No yardstick.  With --time STEP[,UP] both sides are the timed predictors and the spec is
             TimedHarvestSpec (stg_window_harvest_timed, frames on the step grid).

Kernel times come from a separate run under the profiler (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d OUT -o frames -- python tools/frames_bench.py --cases latency --pushes 500
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
DATA = os.path.join(ROOT, "tests", "golden", "data")
TEST_RECORDINGS = (("eth", "eth_test/biwi_eth.txt"), ("hotel", "hotel_test/biwi_hotel.txt"),
                   ("univ", "univ_test/students001.txt"), ("univ", "univ_test/students003.txt"),
                   ("zara1", "zara1_test/crowds_zara01.txt"), ("zara2", "zara2_test/crowds_zara02.txt"))


# model_for and pushes_of restate _model and _pushes of tests/live_inputs.py: a tool does not import from tests/
def model_for(split, dev):
    from social_stgcnn_amd.model import social_stgcnn
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_%s.npz" % split))
    m = social_stgcnn(**CFG)
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    return m.to(dev).eval()


def pushes_of(rows):
    frames = np.unique(rows[:, 0])
    f_idx = np.searchsorted(frames, rows[:, 0])
    order = np.argsort(f_idx, kind="stable")
    bounds = np.searchsorted(f_idx[order], np.arange(len(frames) + 1))
    return [(rows[order[a:b], 1].astype(np.int64), np.ascontiguousarray(rows[order[a:b], 2:4]))
            for a, b in zip(bounds[:-1], bounds[1:])]


def tracks_kw(tracks, timed=None):
    """--tracks M,G and --time STEP,UP -> the keywords of the predictors (nothing without the flags: the strict calls)."""
    from social_stgcnn_amd import frames
    kw = {} if tracks is None else {"tracks": frames.TrackRule(*tracks)}
    if timed is not None:
        kw["time"] = frames.TimeRule(timed[0], history=timed[2])
    return kw


def timed_pushes(rows, step, up):
    """The recording as timestamped pushes [(ids, xy, t)]: a frame number f (the recordings count 10 per model step)
    is the time f / 10 * step ticks; between two frames 10 apart every pedestrian of both is interpolated linearly at
    up - 1 instants, step / up ticks apart."""
    if step % up:
        raise SystemExit("--time STEP,UP: STEP must be a multiple of UP")
    fnum = np.unique(rows[:, 0])
    base = pushes_of(rows)
    out = []
    for f, (ids, xy) in enumerate(base):
        t0 = int(round(fnum[f] / 10 * step))
        out.append((ids, xy, t0))
        if up > 1 and f + 1 < len(base) and fnum[f + 1] - fnum[f] == 10:
            nxt = dict(zip(base[f + 1][0].tolist(), base[f + 1][1]))
            both = [j for j, i in enumerate(ids.tolist()) if i in nxt]
            a, b = xy[both], np.array([nxt[int(ids[j])] for j in both]).reshape(-1, 2)
            out += [(ids[both], a + (b - a) * (j / up), t0 + j * (step // up)) for j in range(1, up)]
    return out


def noisy(pushes, sigma, seed):
    """Seeded Gaussian detector noise on every detection of [(ids, xy, ...)], rounded to 4 decimals."""
    gen = np.random.default_rng(seed)
    return [(p[0], np.around(p[1] + gen.normal(0, sigma, np.shape(p[1])), 4)) + tuple(p[2:]) for p in pushes]


def harvest_spec(windows, timed=None):
    """A log that `windows` windows of up to 32 rows never fill; with --time the timed spec (settle at its default)."""
    from social_stgcnn_amd import frames
    return (frames.HarvestSpec if timed is None else frames.TimedHarvestSpec)(windows, rows=32 * windows)


def latency_case(split, rec, max_peds, k, n_push, dev, warmup=50, tracks=None, timed=None, harvest=False, eager=False):
    from social_stgcnn_amd import data, frames
    rows = data.read_file(os.path.join(DATA, rec))
    pushes = pushes_of(rows) if timed is None else timed_pushes(rows, *timed[:2])
    kw = {"harvest": harvest_spec(warmup + n_push, timed)} if harvest else {}
    fp = frames.FramePredictor(model_for(split, dev), k=k, max_peds=max_peds, **tracks_kw(tracks, timed), **kw)
    push = fp.push if eager else fp.capture()
    times, peds = [], []
    for i in range(warmup + n_push):
        ids, xy = pushes[i % len(pushes)][:2]
        when = {} if timed is None else {"t": pushes[i % len(pushes)][2]}
        if i % len(pushes) == 0:
            fp.reset()
        t0 = time.perf_counter()
        out = push(ids, xy, **when)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
            peds.append(out.num_peds.clone())
    ms = np.array(times) * 1e3
    peds = torch.cat(peds).cpu().numpy()
    return {"case": "latency", "recording": os.path.basename(rec), "max_peds": max_peds, "k": k, "pushes": n_push,
            "p50_ms": round(float(np.percentile(ms, 50)), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4),
            "mean_ms": round(float(ms.mean()), 4), "frames_per_s_p50": round(1e3 / float(np.percentile(ms, 50)), 1),
            "mean_peds": round(float(peds.mean()), 2), "max_peds_seen": int(peds.max()),
            **({} if tracks is None else {"tracks": list(tracks)}), **({} if timed is None else {"time": list(timed)}),
            **({"harvest": list(fp.harvest.counts())} if harvest else {}), **({"eager": True} if eager else {})}


def recording_case(split, rec, k, dev, tracks=None):
    from social_stgcnn_amd import data, frames
    rows = data.read_file(os.path.join(DATA, rec))
    model = model_for(split, dev)
    frames.predict_recording(model, rows, k=k, **tracks_kw(tracks))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc, _ = frames.predict_recording(model, rows, k=k, **tracks_kw(tracks))
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    n = len(sc.frame)
    return {"case": "recording", "recording": os.path.basename(rec), "k": k, "frame_scenes": n,
            "v": int(sc.ids.shape[1]), "seconds": round(secs, 4), "frames_per_s": round(n / secs, 1),
            "mean_peds": round(float(sc.num_peds.float().mean()), 2),
            **({} if tracks is None else {"tracks": list(tracks)})}


def _stream_sequences(ns, n, timed=None):
    """Per stream the first n pushes of a test recording (cycled over the streams), from a staggered start; with
    `timed` the timestamped pushes (a stream's times wrap with its recording: its tracks then start over, as its
    clock does with reset)."""
    from social_stgcnn_amd import data
    recs = [data.read_file(os.path.join(DATA, rec)) for _, rec in TEST_RECORDINGS]
    recs = [pushes_of(r) if timed is None else timed_pushes(r, *timed[:2]) for r in recs]
    out = []
    for s in range(ns):
        p = recs[s % len(recs)]
        off = (s // len(recs)) * 7
        out.append([p[(off + t) % len(p)] for t in range(n)])
    return out


def streams_case(ns, k, n_ticks, dev, block=0, lone=True, max_peds=128, warmup=20, risk="none", tracks=None,
                 score=None, timed=None, associate=None, harvest=False, noise=0.0, calibration=None, eager=False):
    from social_stgcnn_amd import frames
    model = model_for("univ", dev)
    seq = _stream_sequences(ns, warmup + n_ticks, timed)
    if noise > 0:
        seq = [noisy(q, noise, b) for b, q in enumerate(seq)]
    # a recording that wraps inside the run would push a time that is not after the last: keep the run inside it
    if timed is not None and any(q[t + 1][2] <= q[t][2] for q in seq for t in range(len(q) - 1)):
        raise SystemExit("--time: %d ticks wrap a recording; use fewer --ticks" % (warmup + n_ticks))
    kw = {} if score is None else {"score": score}
    if risk != "none":
        from social_stgcnn_amd.predict import RiskSpec
        kw = dict(risk=RiskSpec(0.5, np.array([[-1, -1, 1, 1], [0, 0, 4, 3], [-50, -50, 50, 50]], np.float32)),
                  keep_samples=risk == "samples")
    kw.update(tracks_kw(tracks, timed))
    if harvest:
        kw["harvest"] = harvest_spec(ns * (warmup + n_ticks), timed)
    if calibration is not None:                              # (tools/predict_bench.py --cases calib)
        kw["calibration"] = calibration
    if associate is not None:
        kw["associate"] = associate
        seq = [[(None,) + tuple(p[1:]) for p in q] for q in seq]
    sp = frames.StreamsPredictor(model, ns, k=k, max_peds=max_peds, block_threads=block, **kw)
    replay = sp.push if eager else sp.capture()
    times, host, peds = [], [], []
    for t in range(warmup + n_ticks):
        tick = [q[t][:2] for q in seq]
        when = {} if timed is None else {"times": [q[t][2] for q in seq]}
        t0 = time.perf_counter()
        out = replay(tick, **when)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if t >= warmup:
            times.append(time.perf_counter() - t0)
            host.append(t1 - t0)
            peds.append(out.num_peds.clone())
    ms = np.array(times) * 1e3
    peds = torch.stack(peds).cpu().numpy()
    p50 = float(np.percentile(ms, 50))
    res = {"case": "streams", "streams": ns, "k": k, "max_peds": max_peds, "block": block or frames.STREAM_THREADS,
           "ticks": n_ticks, "tick_p50_ms": round(p50, 4), "tick_p90_ms": round(float(np.percentile(ms, 90)), 4),
           "frames_per_s_p50": round(ns * 1e3 / p50, 1), "mean_peds": round(float(peds.mean()), 2),
           "max_peds_seen": int(peds.max()), "host_p50_ms": round(float(np.percentile(host, 50)) * 1e3, 4)}
    if associate is not None:
        res["associate"] = list(associate[:-1])
        res["assoc_full"] = int((sp.assoc_flags != 0).sum())
    if tracks is not None:
        res["tracks"] = list(tracks)
    if eager:
        res["eager"] = True
    if harvest:
        res["harvest"] = list(sp.harvest.counts())               # windows, rows, dropped_full
    if timed is not None:
        res["time"] = list(timed)
        res["state_mb_per_stream"] = round(sum(x[0].numel() * x.element_size() for x in sp._state) / 1e6, 3)
    if risk != "none":
        res["risk"] = risk
        res["conflict_any_mean"] = round(float(sp.risk.conflict_any.float().mean()), 3)
    counts = 0 if risk == "none" else sum(x.numel() for x in sp.risk[1:] if x is not None)
    res["result_mb"] = round((out.samples.numel() + out.mean.numel() + counts) * 4 / 1e6, 3)
    if score is not None:
        st = sp._score_state
        s = frames.score_summary(*sp.score_totals, score.levels)
        n = s.count.sum(axis=0)
        res.update({"state_mb": round(sum(x.numel() * x.element_size() for x in st if x is not None) / 1e6, 1),
                    "scored": int(n.sum()), "trajectories": int(s.trajectories.sum()),
                    **({} if sp.score_evictions is None else {"pending": score.pending,
                                                              "evictions": int(sp.score_evictions.sum())}),
                    "err_h1": round(float(np.nansum(s.err[:, 0] * s.count[:, 0]) / max(1.0, n[0])), 4),
                    "err_hP": round(float(np.nansum(s.err[:, -1] * s.count[:, -1]) / max(1.0, n[-1])), 4)})
    if lone:
        # the yardstick: NS lone captured FramePredictors, one after another; fewer ticks at large NS
        n_seq = max(10, min(n_ticks, 4000 // ns))
        fps = [frames.FramePredictor(model, k=k, max_peds=max_peds, **tracks_kw(tracks, timed)) for _ in range(ns)]
        pushes = [fp.push if eager else fp.capture() for fp in fps]
        times = []
        for t in range(warmup + n_seq):
            tot = 0.0
            for s in range(ns):
                ids, xy = seq[s][t][:2]
                when = {} if timed is None else {"t": seq[s][t][2]}
                t0 = time.perf_counter()
                pushes[s](ids, xy, **when)
                torch.cuda.synchronize()
                tot += time.perf_counter() - t0
            if t >= warmup:
                times.append(tot)
        ms = np.array(times) * 1e3
        seq_p50 = float(np.percentile(ms, 50))
        res.update({"lone_ticks": n_seq, "lone_tick_p50_ms": round(seq_p50, 4),
                    "lone_tick_p90_ms": round(float(np.percentile(ms, 90)), 4),
                    "lone_frames_per_s_p50": round(ns * 1e3 / seq_p50, 1), "speedup_p50": round(seq_p50 / p50, 2)})
        del pushes, fps
    return res


def associate_quality(split, rec, k, dev, spec, max_peds=128):
    """One recording through two captured FramePredictors with score=ScoreSpec(): one fed the recording's ids, one fed
    positions only.  What an identity switch costs in prediction quality."""
    from social_stgcnn_amd import data, frames
    from social_stgcnn_amd.predict import ScoreSpec
    pushes = pushes_of(data.read_file(os.path.join(DATA, rec)))
    model = model_for(split, dev)
    score = ScoreSpec()
    res = {"case": "associate_quality", "recording": os.path.basename(rec), "k": k, "associate": list(spec[:3])}
    for name, assoc in (("ids", None), ("assoc", spec)):
        fp = frames.FramePredictor(model, k=k, max_peds=max_peds, score=score, associate=assoc)
        replay = fp.capture()
        prev, wrong, links = {}, 0, 0
        for t, (ids, xy) in enumerate(pushes):
            replay(None if assoc else ids, xy, seed=t)
            if assoc:
                now = dict(zip(ids.tolist(), fp.det_ids.cpu().tolist()))
                links += sum(1 for r in now if r in prev)
                wrong += sum(1 for r, g in now.items() if r in prev and prev[r] != g)
                prev = now
        s = frames.score_summary(*fp.score_totals, score.levels)
        res.update({name + "_trajectories": int(s.trajectories[0]), name + "_ade": round(float(s.ade[0]), 4),
                    name + "_fde": round(float(s.fde[0]), 4), name + "_scored": int(s.count[0].sum())})
        if assoc:
            res.update({"links": links, "wrong_links": wrong, "assoc_full": int(fp.assoc_flags.item())})
    return res


def associate_timed_quality(split, rec, k, dev, spec, step=4, up=4, max_peds=128, noise=0.0):
    """One recording upsampled `up` x (with `noise` metres of seeded Gaussian noise on every detection) through two
    captured timed FramePredictors with score=TimedScoreSpec(): one fed the recording's ids, one fed positions only."""
    from social_stgcnn_amd import data, frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    pushes = timed_pushes(data.read_file(os.path.join(DATA, rec)), step, up)
    if noise > 0:
        pushes = noisy(pushes, noise, 1)
    model = model_for(split, dev)
    score = TimedScoreSpec(pending=max(128, 2 * up * CFG["pred_seq_len"]))
    res = {"case": "associate_filtered_quality" if isinstance(spec, frames.FilteredAssociateSpec)
           else "associate_timed_quality", "recording": os.path.basename(rec), "k": k, "associate": list(spec[:-1]),
           "time": [step, up], "pushes": len(pushes), "noise": noise}
    for name, assoc in (("ids", None), ("assoc", spec)):
        fp = frames.FramePredictor(model, k=k, max_peds=max_peds, score=score, time=frames.TimeRule(step), associate=assoc)
        replay = fp.capture()
        prev, wrong, links = {}, 0, 0
        for n, (ids, xy, t) in enumerate(pushes):
            replay(None if assoc else ids, xy, t=t, seed=n)
            if assoc:
                now = dict(zip(ids.tolist(), fp.det_ids.cpu().tolist()))
                links += sum(1 for r in now if r in prev)
                wrong += sum(1 for r, g in now.items() if r in prev and prev[r] != g)
                prev = now
        s = frames.score_summary(*fp.score_totals, score.levels)
        res.update({name + "_trajectories": int(s.trajectories[0]), name + "_ade": round(float(s.ade[0]), 4),
                    name + "_fde": round(float(s.fde[0]), 4), name + "_scored": int(s.count[0].sum()),
                    name + "_evictions": int(fp.score_evictions.sum())})
        if assoc:
            res.update({"links": links, "wrong_links": wrong, "assoc_flags": int(fp.assoc_flags.item())})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pushes", type=int, default=2000)
    ap.add_argument("--cases", default="latency,recording")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--streams", default="1,8,64,256,600")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--block", default="0", help="push workgroup size(s) of the streams case, comma separated")
    ap.add_argument("--no-lone", action="store_true",
                    help="streams: skip the yardstick; associate: skip the two single-stream quality runs")
    ap.add_argument("--risk", default="none", help="modes of the streams case, comma separated: none, samples, lean")
    ap.add_argument("--tracks", default=None, metavar="M,G",
                    help="run every case under frames.TrackRule(min_seen=M, max_gap=G); default: the strict rule")
    ap.add_argument("--time", default=None, metavar="STEP[,UP]",
                    help="timestamped pushes (frames.TimeRule(STEP)) on the feed upsampled UP x (default 1) by linear "
                         "interpolation: the latency and streams cases")
    ap.add_argument("--history", type=int, default=96, help="with --time: samples kept per track")
    ap.add_argument("--pending", type=int, default=128,
                    help="with --time and the score case: record rows per stream (predict.TimedScoreSpec)")
    ap.add_argument("--harvest", action="store_true",
                    help="the latency and streams cases with harvest=HarvestSpec(...) (with --time: TimedHarvestSpec), "
                         "sized so that the log never fills")
    ap.add_argument("--associate", default="1.0,2.0,0", metavar="GATE[,GATE_NEW[,MAX_MISS]]",
                    help="the AssociateSpec of the associate case")
    ap.add_argument("--associate_timed", default="1.0,2.0,0", metavar="GATE[,GATE_NEW[,MAX_AGE]]",
                    help="the TimedAssociateSpec of the associate_timed case (MAX_AGE in ticks)")
    ap.add_argument("--associate_filtered", default="0.05,1.0",
                    metavar="SIGMA_DET,SIGMA_ACC[,SIGMA_VEL0[,GATE_SIGMAS[,GATE_MAX[,MAX_AGE]]]]",
                    help="the FilteredAssociateSpec of the associate_filtered case (MAX_AGE in ticks)")
    ap.add_argument("--eager", action="store_true",
                    help="the latency and streams cases through push() in the place of the captured replay")
    ap.add_argument("--noise", type=float, default=0.0, metavar="SIGMA",
                    help="associate_timed and associate_filtered: Gaussian noise of SIGMA metres on every detection")
    a = ap.parse_args()
    tracks = None if a.tracks is None else tuple(int(x) for x in a.tracks.split(","))
    timed = None
    if a.time is not None:
        timed = tuple(int(x) for x in a.time.split(","))
        timed = (timed[0], timed[1] if len(timed) > 1 else 1, a.history)
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench needs a GPU (MI355X)")
    dev = torch.device("cuda", 0)
    cases = a.cases.split(",")
    if "latency" in cases:
        for split, rec, v in (("eth", "eth_test/biwi_eth.txt", 32), ("eth", "eth_test/biwi_eth.txt", 128),
                              ("univ", "univ_test/students001.txt", 128)):
            print(json.dumps(latency_case(split, rec, v, a.k, a.pushes, dev, tracks=tracks, timed=timed,
                                          harvest=a.harvest, eager=a.eager)), flush=True)
    if "recording" in cases:
        for split, rec in TEST_RECORDINGS:
            print(json.dumps(recording_case(split, rec, a.k, dev, tracks)), flush=True)
    if "score" in cases:
        from social_stgcnn_amd.predict import ScoreSpec, TimedScoreSpec
        # with --time the timed predictors and the records indexed by time
        spec = ScoreSpec() if timed is None else TimedScoreSpec(pending=a.pending)
        for ns in (int(n) for n in (a.streams if a.streams != "1,8,64,256,600" else "1,64,600").split(",")):
            off = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, timed=timed)
            on = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, score=spec, timed=timed)
            on.update({"case": "score", "tick_p50_ms_without": off["tick_p50_ms"],
                       "tick_p90_ms_without": off["tick_p90_ms"],
                       "score_cost_p50_ms": round(on["tick_p50_ms"] - off["tick_p50_ms"], 4)})
            print(json.dumps(on), flush=True)
    if "harvest" in cases:
        lat = [latency_case("univ", "univ_test/students001.txt", 128, a.k, a.pushes, dev, tracks=tracks, timed=timed,
                            harvest=h) for h in (False, True)]
        lat[1].update({"case": "harvest_latency", "p50_ms_without": lat[0]["p50_ms"], "p90_ms_without": lat[0]["p90_ms"],
                       "harvest_cost_p50_ms": round(lat[1]["p50_ms"] - lat[0]["p50_ms"], 4)})
        print(json.dumps(lat[1]), flush=True)
        for ns in (int(n) for n in (a.streams if a.streams != "1,8,64,256,600" else "1,64,600").split(",")):
            off = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, timed=timed)
            on = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, timed=timed, harvest=True)
            on.update({"case": "harvest", "tick_p50_ms_without": off["tick_p50_ms"],
                       "tick_p90_ms_without": off["tick_p90_ms"],
                       "harvest_cost_p50_ms": round(on["tick_p50_ms"] - off["tick_p50_ms"], 4)})
            print(json.dumps(on), flush=True)
    if "associate" in cases:
        from social_stgcnn_amd.frames import AssociateSpec
        g = a.associate.split(",")
        spec = AssociateSpec(float(g[0]), float(g[1]) if len(g) > 1 else None, int(g[2]) if len(g) > 2 else 0)
        for ns in (int(n) for n in (a.streams if a.streams != "1,8,64,256,600" else "1,64,600").split(",")):
            off = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks)
            on = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, associate=spec)
            on.update({"case": "associate", "tick_p50_ms_without": off["tick_p50_ms"],
                       "tick_p90_ms_without": off["tick_p90_ms"], "host_p50_ms_without": off["host_p50_ms"],
                       "associate_cost_p50_ms": round(on["tick_p50_ms"] - off["tick_p50_ms"], 4)})
            print(json.dumps(on), flush=True)
        for split, rec in (() if a.no_lone else (("zara1", "zara1_test/crowds_zara01.txt"),
                                                 ("univ", "univ_test/students003.txt"))):
            print(json.dumps(associate_quality(split, rec, a.k, dev, spec)), flush=True)
    for case in ("associate_timed", "associate_filtered"):
        if case not in cases:
            continue
        from social_stgcnn_amd.frames import FilteredAssociateSpec, TimedAssociateSpec
        if case == "associate_timed":
            g = a.associate_timed.split(",")
            spec = TimedAssociateSpec(float(g[0]), float(g[1]) if len(g) > 1 else None, int(g[2]) if len(g) > 2 else 0)
        else:
            g = a.associate_filtered.split(",")
            spec = FilteredAssociateSpec(*(float(x) for x in g[:5]), **({"max_age": int(g[5])} if len(g) > 5 else {}))
        t10 = (10, 10, a.history) if timed is None else timed
        for ns in (int(n) for n in (a.streams if a.streams != "1,8,64,256,600" else "1,64,600").split(",")):
            off = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, timed=t10, noise=a.noise)
            on = streams_case(ns, a.k, a.ticks, dev, 0, False, tracks=tracks, timed=t10, associate=spec, noise=a.noise)
            on.update({"case": case, "noise": a.noise, "tick_p50_ms_without": off["tick_p50_ms"],
                       "tick_p90_ms_without": off["tick_p90_ms"], "host_p50_ms_without": off["host_p50_ms"],
                       "associate_cost_p50_ms": round(on["tick_p50_ms"] - off["tick_p50_ms"], 4)})
            print(json.dumps(on), flush=True)
        if not a.no_lone:
            print(json.dumps(associate_timed_quality("zara1", "zara1_test/crowds_zara01.txt", a.k, dev, spec,
                                                     noise=a.noise)), flush=True)
    if "streams" in cases:
        for block in (int(b) for b in a.block.split(",")):
            for ns in (int(n) for n in a.streams.split(",")):
                for mode in a.risk.split(","):
                    print(json.dumps(streams_case(ns, a.k, a.ticks, dev, block, not a.no_lone, risk=mode,
                                                  tracks=tracks, timed=timed, harvest=a.harvest, eager=a.eager)),
                          flush=True)


if __name__ == "__main__":
    main()
