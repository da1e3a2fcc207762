"""GPU (-m gpu): partially observed tracks (frames.TrackRule, fill_tracks, the *_rule entry points of csrc/frames.hip)
against the numpy statement tests/frames_fill_np.py, bit for bit: every presence pattern of an 8-frame window through
the recording kernels and the fill kernel; the live push (the C entry point, FramePredictor eager and captured) against
the recording kernels and the push-by-push statement, with its edge cases; StreamsPredictor against lone
FramePredictors; the strict rule through the new kernels against the strict kernels; predictions, risk counts and the
command end to end; and the accuracy of a history cut to two frames against the full one on the device."""
import argparse
import os

import numpy as np
import pytest
import torch

import frames_fill_np
import frames_np
from live_inputs import DATA, _assert_scene, _CPush, _model, _pushes, _rows, _sparse_rows

pytestmark = pytest.mark.gpu
ETH = os.path.join(DATA, "eth_test", "biwi_eth.txt")
RULES = ((8, 0), (2, 0), (2, 6), (3, 1), (5, 2))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    return _model("eth", dev)


def _eth_rows():
    return _rows("eth_test", "biwi_eth.txt")


def _pattern_rows():
    """8 frames, ids 1 .. 255: id k has a row in frame t iff bit t of k is set; positions with more decimals than the
    rounding keeps.  At frame index 7 the window holds every presence pattern that is seen now."""
    gen = np.random.default_rng(11)
    rows = [(10.0 * t, float(k)) for t in range(8) for k in range(1, 256) if (k >> t) & 1]
    rows = np.array(rows)
    return np.concatenate([rows, gen.uniform(-20, 20, size=(len(rows), 2))], axis=1)


def _host_scenes(sc):
    return sc.ids.cpu().numpy(), sc.num_peds.cpu().numpy(), sc.obs_abs.cpu().numpy(), sc.seen.cpu().numpy()


# ---- 1. every presence pattern at once -------------------------------------------------------------------------------
@pytest.mark.parametrize("decimals", [4, None])
def test_every_presence_pattern_through_the_recording_kernels(dev, decimals):
    """decimals=None is the run that catches a contracted multiply-add: nothing rounds the last bits away."""
    from social_stgcnn_amd import frames
    rows = _pattern_rows()
    for ms, mg in RULES:
        ref = frames_fill_np.frame_scenes_rule(rows, 8, ms, mg, min_peds=0, decimals=decimals)
        sc = frames.recording_scenes(rows, dev, min_peds=0, decimals=decimals, tracks=frames.TrackRule(ms, mg))
        assert isinstance(sc, frames.PartialScenes) and sc.seen.dtype == torch.int32
        assert np.array_equal(sc.frame, np.array([r[1] for r in ref])) and len(ref) == 8 - (ms - 1), (ms, mg)
        ids, peds, obs, seen = _host_scenes(sc)
        assert ids.shape[1] == max(len(r[2]) for r in ref), (ms, mg)
        for i, (_, _, rid, robs, rseen) in enumerate(ref):
            _assert_scene(ids[i], peds[i], obs[i], rid, robs, (ms, mg, decimals, i), seen[i], rseen)
        if (ms, mg) == (2, 6):
            # the last frame holds every pattern seen now and at least once more
            assert int(peds[-1]) == 127 and sorted(seen[-1].tolist()) == list(range(3, 256, 2))
        if (ms, mg) == (8, 0):
            assert ids.tolist() == [[255]] and seen.tolist() == [[255]]


@pytest.mark.parametrize("decimals", [4, None])
def test_every_presence_pattern_through_fill_tracks(dev, decimals):
    from social_stgcnn_amd import frames
    from social_stgcnn_amd._lib import lib, ptr, stream_ptr
    gen = np.random.default_rng(13)
    obs = gen.uniform(-20, 20, size=(2, 8, 255, 2))
    seen = np.tile(np.arange(1, 256, dtype=np.int32), (2, 1))
    seen[1] = seen[1, ::-1] | 0x7fffff00                      # bits at and above T_obs are not looked at
    peds = np.array([255, 100], np.int32)
    want = frames_fill_np.fill_tracks(obs, seen, peds, decimals)
    got = torch.from_numpy(obs).to(dev)
    back = frames.fill_tracks(got, torch.from_numpy(seen).to(dev), torch.from_numpy(peds).to(dev), decimals)
    assert back is got
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want[1, :, 100:], obs[1, :, 100:]) and not np.array_equal(want[1, :, :100], obs[1, :, :100])
    # without counts every column is filled; a second pass changes nothing (rounding is idempotent, seen steps stay)
    all_cols = frames.fill_tracks(torch.from_numpy(obs).to(dev), seen, None, decimals)
    assert np.array_equal(all_cols.cpu().numpy(), frames_fill_np.fill_tracks(obs, seen, None, decimals))
    again = frames.fill_tracks(all_cols.clone(), seen, None, decimals)
    assert torch.equal(again, all_cols)
    # T_obs = 3 through the C entry point: the seven patterns
    obs3 = gen.uniform(-20, 20, size=(1, 3, 7, 2))
    seen3 = np.arange(1, 8, dtype=np.int32)[None]
    d_obs, d_seen = torch.from_numpy(obs3).to(dev), torch.from_numpy(seen3).to(dev)
    rc = lib().stg_fill_tracks(ptr(d_obs), ptr(d_seen), None, 1, 3, 7, frames._scale(decimals), stream_ptr())
    assert rc == 0
    assert np.array_equal(d_obs.cpu().numpy(), frames_fill_np.fill_tracks(obs3, seen3, None, decimals))
    with pytest.raises(ValueError, match="float64"):
        frames.fill_tracks(got.float(), seen)
    with pytest.raises(ValueError, match="seen"):
        frames.fill_tracks(got, seen[:, :10])


# ---- 2. live equals recording ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,rule,decimals", [("pattern", (2, 6), None), ("pattern", (3, 1), 4),
                                                 ("sparse", (2, 2), 4), ("sparse", (5, 2), None)])
def test_live_pushes_equal_the_recording_scenes(dev, model, which, rule, decimals):
    """The C entry point and the recording kernels at V = 256; the predictors at max_peds = 128, the widest scene the
    model's forward serves from one workgroup's LDS (V = 256 needs 210,240 bytes of the 163,840).  No frame of either
    recording has more than 128 ids, so no scene is cut at either width."""
    from social_stgcnn_amd import frames
    rows = _pattern_rows() if which == "pattern" else _sparse_rows()
    tr = frames.TrackRule(*rule)
    v = 256
    sc = frames.recording_scenes(rows, dev, min_peds=0, decimals=decimals, v_pad=v, tracks=tr)
    at = {fn: i for i, fn in enumerate(sc.frame)}
    r_ids, r_peds, r_obs, r_seen = _host_scenes(sc)
    fnums = np.unique(rows[:, 0])
    ref = frames_fill_np.StreamModelRule(8, rule[0], rule[1], max_peds=v, decimals=decimals)
    c_push = _CPush(dev, rule, v, 512, 256, decimals=decimals)
    vp = 128
    assert max(len(ids) for ids, _ in _pushes(rows)) <= vp
    kw = dict(k=2, capacity=512, max_peds=vp, max_detections=256, decimals=decimals, tracks=tr)
    eager = frames.FramePredictor(model, **kw)
    cap = frames.FramePredictor(model, **kw)
    replay = cap.capture()
    assert eager.seen is None
    some, static, earlier = 0, set(), None
    for f, (ids, xy) in enumerate(_pushes(rows)):
        s_ids, s_obs, s_seen, more = ref.push(ids, xy)
        assert not more
        c_ids, c_peds, c_obs, c_seen, c_flags = c_push.push(ids, xy)
        _assert_scene(c_ids, c_peds, c_obs, s_ids, s_obs, ("c", f), c_seen, s_seen)
        assert c_flags == 0
        e = eager.push(ids, xy, seed=f)
        c = replay(ids, xy, seed=f)
        for out, p, what in ((e, eager, "eager"), (c, cap, "captured")):
            assert p.seen.shape == (vp,) and p.seen.dtype == torch.int32
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), s_ids, s_obs,
                          (what, f), p.seen.cpu().numpy(), s_seen)
            assert int(out.flags.item()) == 0
        assert torch.equal(c.mean, e.mean), f          # (random jumps: the sampled positions need not be finite)
        # an eager push leaves earlier results alone; a captured one writes the graph's static buffer
        static.add(cap.seen.data_ptr())
        if earlier is not None:
            assert earlier[0].data_ptr() != eager.seen.data_ptr() and np.array_equal(earlier[0].cpu().numpy(), earlier[1])
        earlier = (eager.seen, eager.seen.cpu().numpy())
        # ... and the recording kernels' scene at this frame
        if f < rule[0] - 1:
            assert len(s_ids) == 0 and fnums[f] not in at
            continue
        i = at[fnums[f]]
        _assert_scene(r_ids[i], r_peds[i], r_obs[i], s_ids, s_obs, ("recording", f), r_seen[i], s_seen)
        some += len(s_ids)
    assert some > 100 and len(static) == 1


def test_live_edge_cases(dev, model):
    from social_stgcnn_amd import frames
    gen = np.random.default_rng(14)
    xy = lambda m: gen.uniform(-20, 20, size=(m, 2))              # noqa: E731
    tr = frames.TrackRule(2, 2)
    # ten eligible ids, max_peds 4: the smallest four, flag TOO_MANY from the second push on
    for mode in ("eager", "captured"):
        fp = frames.FramePredictor(model, k=2, max_peds=4, tracks=tr)
        push = fp.push if mode == "eager" else fp.capture()
        ref = frames_fill_np.StreamModelRule(8, 2, 2, max_peds=4)
        ids = np.array([31, 7, 19, 3, 23, 11, 5, 29, 13, 17], np.int64)
        for f in range(4):
            p = xy(10)
            out = push(ids, p)
            s_ids, s_obs, s_seen, more = ref.push(ids, p)
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), s_ids, s_obs,
                          (mode, f), fp.seen.cpu().numpy(), s_seen)
            assert int(out.flags.item()) == (frames.TOO_MANY if f >= 1 else 0) and more == (f >= 1), (mode, f)
        assert out.ids.tolist() == [3, 5, 7, 11]
    # gaps.  id 1 is always there.  id 2 misses frames 4-6 (max_gap + 1 frames): out while frame 3 and frame 7 share a
    # window (until frame 10), then back as a short track.  id 3 is seen in frames 0-1 and misses 2-8 (T_obs - 1
    # frames): its slot is freed at frame 9, where the new id 9, ahead of it in the push, takes that slot and id 3
    # another; one frame seen is below min_seen, so id 3 is back at frame 10 with two bits.
    script = []
    for f in range(14):
        ids = [1]
        if not 4 <= f <= 6:
            ids.append(2)
        if f >= 9:
            ids.append(9)
        if f <= 1 or f >= 9:
            ids.append(3)
        script.append((np.array(ids, np.int64), xy(len(ids))))
    for mode in ("eager", "captured"):
        fp = frames.FramePredictor(model, k=2, capacity=8, max_peds=8, max_detections=8, tracks=tr)
        push = fp.push if mode == "eager" else fp.capture()
        ref = frames_fill_np.StreamModelRule(8, 2, 2, max_peds=8)
        got, slot3 = [], []
        for f, (ids, p) in enumerate(script):
            out = push(ids, p)
            s_ids, s_obs, s_seen, _ = ref.push(ids, p)
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), s_ids, s_obs,
                          (mode, f), fp.seen.cpu().numpy(), s_seen)
            assert int(out.flags.item()) == 0
            got.append(dict(zip(s_ids.tolist(), s_seen.tolist())))
            slot3.append((fp.slot_id == 3).nonzero().flatten().tolist())
        assert [2 in g for g in got] == [False] + [True] * 3 + [False] * 7 + [True] * 3, mode
        assert got[3][2] == 0b1111 and got[11][2] == 0b11111 and got[13][2] == 0b1111111
        assert [3 in g for g in got] == [False, True] + [False] * 8 + [True] * 4, mode
        assert got[10][3] == 0b11
        assert slot3[1] == slot3[8] and len(slot3[1]) == 1 and len(slot3[9]) == 1 and slot3[9] != slot3[8], mode
        # reset(): every track is forgotten, the next push has nobody with two frames
        fp.reset()
        ref.reset()
        for f, (ids, p) in enumerate(script[:3]):
            out = push(ids, p)
            s_ids, s_obs, s_seen, _ = ref.push(ids, p)
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), s_ids, s_obs,
                          (mode, "reset", f), fp.seen.cpu().numpy(), s_seen)
            assert (f == 0) == (len(s_ids) == 0)
    # a repeated id within a push given as device tensors: flag, the first detection wins
    for mode in ("eager", "captured"):
        fp = frames.FramePredictor(model, k=2, tracks=tr)
        push = fp.push if mode == "eager" else fp.capture()
        ref = frames_fill_np.StreamModelRule(8, 2, 2)
        for f in range(9):
            ids = np.array([4, 9, 4, 1] if f % 3 == 0 else ([9, 1] if f == 4 else [9, 4, 1]), np.int64)
            p = xy(len(ids))
            out = push(torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev))
            s_ids, s_obs, s_seen, _ = ref.push(ids, p)
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), s_ids, s_obs,
                          (mode, f), fp.seen.cpu().numpy(), s_seen)
            assert int(out.flags.item()) == (frames.DUPLICATE if f % 3 == 0 else 0), (mode, f)


# ---- 3. streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [64, 1024])
def test_streams_equal_lone_frame_predictors_under_a_rule(dev, model, block):
    from social_stgcnn_amd import frames
    ns, k, v = 5, 2, 32
    tr = frames.TrackRule(2, 2)
    rows = _eth_rows()
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[29]]
    seqs = []
    for s in range(ns):
        keep = np.random.default_rng(100 + s).random(len(rows)) >= 0.15
        seqs.append(_pushes(rows[keep]))
    n_ticks = min(len(q) for q in seqs)
    kw = dict(k=k, capacity=64, max_peds=v, max_detections=32, tracks=tr)
    eager = frames.StreamsPredictor(model, ns, block_threads=block, **kw)
    cap = frames.StreamsPredictor(model, ns, block_threads=block, **kw)
    replay = cap.capture()
    lone = [frames.FramePredictor(model, **kw) for _ in range(ns - 1)]
    filled = 0
    for t in range(n_ticks):
        # stream 4 is never pushed; stream s sits out the ticks t % 7 == s
        tick = {s: seqs[s][t] for s in range(ns - 1) if t % 7 != s}
        e = eager.push(tick, seed=t)
        c = replay(tick, seed=t)
        assert eager.seen.shape == (ns, v) and eager.seen.dtype == torch.int32
        for a, b, name in zip(e, c, e._fields):
            assert torch.equal(a, b), (t, name)
        assert torch.equal(eager.seen, cap.seen), t
        for s in range(ns):
            if s not in tick:
                assert int(e.num_peds[s]) == 0 and not e.pushed[s] and not eager.seen[s].any(), (t, s)
                assert bool((e.ids[s] == -1).all()) and not e.obs_abs[s].any() and int(e.flags[s]) == 0, (t, s)
                continue
            r = lone[s].push(*tick[s])
            assert torch.equal(e.ids[s], r.ids) and torch.equal(e.num_peds[s:s + 1], r.num_peds), (t, s)
            assert torch.equal(e.obs_abs[s:s + 1], r.obs_abs) and torch.equal(e.flags[s:s + 1], r.flags), (t, s)
            assert torch.equal(eager.seen[s], lone[s].seen), (t, s)
            assert torch.equal(e.v_pred[s], r.v_pred) and torch.equal(e.mean[s], r.mean), (t, s)
            filled += int((lone[s].seen[:int(r.num_peds)] != 255).sum())
        assert int(e.flags.max()) == 0
    assert filled > 200
    assert not eager.mask[ns - 1].any() and bool((eager.slot_id[ns - 1] == -1).all())


# ---- 4. the strict rule through the new kernels ------------------------------------------------------------------------
def test_strict_rule_through_the_new_path_equals_the_old_path(dev, model):
    from social_stgcnn_amd import frames
    rows = _eth_rows()
    tr = frames.TrackRule(8, 0)
    old = frames.recording_scenes(rows, dev)
    new = frames.recording_scenes(rows, dev, tracks=tr)
    assert isinstance(old, frames.FrameScenes) and not hasattr(old, "seen")
    assert np.array_equal(old.frame, new.frame) and len(old.frame) == 725
    assert torch.equal(old.ids, new.ids) and torch.equal(old.num_peds, new.num_peds)
    assert torch.equal(old.obs_abs, new.obs_abs)
    assert torch.equal(new.seen, torch.where(new.ids >= 0, 255, 0).to(torch.int32))
    for kw in (dict(min_peds=0, v_pad=24), dict(min_peds=3, decimals=None)):
        a, b = frames.recording_scenes(rows, dev, **kw), frames.recording_scenes(rows, dev, tracks=tr, **kw)
        assert np.array_equal(a.frame, b.frame)
        assert torch.equal(a.ids, b.ids) and torch.equal(a.num_peds, b.num_peds) and torch.equal(a.obs_abs, b.obs_abs)
    sc_o, pr_o = frames.predict_recording(model, rows, k=3, seed=5)
    sc_n, pr_n = frames.predict_recording(model, rows, k=3, seed=5, tracks=tr)
    for a, b in zip(pr_o, pr_n):
        assert torch.equal(a, b)
    # live, one captured graph each, the comparisons kept on the device
    p_old = frames.FramePredictor(model, k=3)
    p_new = frames.FramePredictor(model, k=3, tracks=tr)
    r_old, r_new = p_old.capture(), p_new.capture()
    same = torch.ones((), device=dev, dtype=torch.bool)
    seen_ok = torch.ones((), device=dev, dtype=torch.bool)
    for f, (ids, xy) in enumerate(_pushes(rows)):
        o, n = r_old(ids, xy, seed=f), r_new(ids, xy, seed=f)
        for a, b in zip(o, n):
            same &= (a == b).all()
        seen_ok &= (p_new.seen == torch.where(n.ids >= 0, 255, 0)).all()
    assert bool(same) and bool(seen_ok)
    assert p_old.seen is None
    for name in ("slot_id", "mask", "ring", "head_flags"):
        assert torch.equal(getattr(p_old, name), getattr(p_new, name)), name


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def _dropped(rows, seed=21, share=0.10):
    """The recording without a seeded tenth of its rows; the first row of every frame stays, so no frame vanishes."""
    first = np.zeros(len(rows), bool)
    first[np.unique(rows[:, 0], return_index=True)[1]] = True
    return rows[first | (np.random.default_rng(seed).random(len(rows)) >= share)]


def test_predictions_of_filled_scenes_end_to_end(dev, model, tmp_path):
    from social_stgcnn_amd import frames, predict_frames
    from social_stgcnn_amd.predict import Predictor, RiskSpec
    from social_stgcnn_amd.trainer import Checkpoint
    full = _eth_rows()
    rows = _dropped(full)
    assert 0.08 < 1 - len(rows) / len(full) < 0.11
    tr = frames.TrackRule(2, 2)
    k = 4
    ref = frames_fill_np.frame_scenes_rule(rows, 8, 2, 2)
    sc, pr, risk = frames.predict_recording(model, rows, k=k, seed=0, tracks=tr, risk=RiskSpec(0.5))
    n, v = sc.ids.shape
    assert np.array_equal(sc.frame, np.array([r[1] for r in ref])) and v == max(len(r[2]) for r in ref)
    ids, peds, obs, seen = _host_scenes(sc)
    want = np.zeros((n, 8, v, 2))
    counts = np.zeros(n, np.int32)
    for i, (_, _, rid, robs, rseen) in enumerate(ref):
        _assert_scene(ids[i], peds[i], obs[i], rid, robs, i, seen[i], rseen)
        want[i, :, :len(rid)] = robs
        counts[i] = len(rid)
    # Predictor.predict on the statement's filled positions: bit-equal at the same padding and batching (the bars of
    # tests/test_gpu_frames.py for this comparison), 1e-5 at a scene's own width
    pred = Predictor(model, k)
    for b, lo in enumerate(range(0, n, 64)):
        hi = min(n, lo + 64)
        r = pred.predict(torch.from_numpy(want[lo:hi]).to(dev), torch.from_numpy(counts[lo:hi]).to(dev), seed=b)
        assert torch.equal(pr.v_pred[lo:hi], r.v_pred), b
        assert torch.equal(pr.samples[:, lo:hi], r.samples) and torch.equal(pr.mean[lo:hi], r.mean), b
    worst = 0.0
    for j in range(0, n, max(1, n // 12)):
        c = int(counts[j])
        own = pred.predict(torch.from_numpy(np.ascontiguousarray(want[j:j + 1, :, :c])).to(dev), seed=0).v_pred
        worst = max(worst, float((own[0] - pr.v_pred[j, :, :, :c]).abs().max()))
    assert worst < 1e-5, worst
    # whom the rule adds: everybody the strict rule predicts on the whole recording and who is detected now, unless a
    # dropped row opened a gap of more than max_gap frames (the statement's tables decide)
    strict = {s[1]: s[2] for s in frames_np.frame_scenes(full)}
    fnum, ped_ids, present, _ = frames_np.recording_tables(rows)
    got = {r[1]: r[2] for r in ref}
    kept_more, broken = 0, 0
    for f, fn in enumerate(fnum):
        now = ped_ids[present[:, f]].astype(np.int64)
        for i in np.intersect1d(strict.get(fn, np.zeros(0, np.int64)), now):
            if i in got.get(fn, ()):
                continue
            win = present[np.searchsorted(ped_ids, i), f - 7:f + 1]
            at = np.nonzero(win)[0]
            assert win[-1] and len(at) >= 2 and np.max(np.diff(at) - 1) > 2, (fn, i)
            broken += 1
        kept_more += len(got.get(fn, ())) - len(np.intersect1d(strict.get(fn, np.zeros(0, np.int64)), now))
    assert kept_more > 500 and 0 < broken < 200
    # the risk counts see the larger scene
    assert n > 725 and risk.conflict.shape == (n, 12, v) and risk.conflict_any.shape == (n, v)
    assert risk.partner.shape == (n, v) and int(risk.conflict.max()) <= k
    pad = torch.arange(v, device=dev)[None] >= sc.num_peds[:, None]
    assert not risk.conflict_any[pad].any() and bool((risk.partner[pad] == -1).all())
    # the command
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    out = str(tmp_path / "preds.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", ETH, "--ksteps", "3", "--seed", "3", "--min_seen", "2",
                         "--max_gap", "2", "--out", out])
    npz = np.load(out)
    sc2, pr2 = frames.predict_recording(model, full, k=3, seed=3, tracks=tr)
    assert np.array_equal(npz["seen"], sc2.seen.cpu().numpy()) and npz["seen"].dtype == np.int32
    assert np.array_equal(npz["frame"], sc2.frame) and np.array_equal(npz["ids"], sc2.ids.cpu().numpy())
    assert np.array_equal(npz["mean"], pr2.mean.cpu().numpy()) and np.array_equal(npz["samples"], pr2.samples.cpu().numpy())
    assert len(sc2.frame) == 860 and int((sc2.seen != 255).sum()) > 1000
    out8 = str(tmp_path / "preds8.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", ETH, "--ksteps", "3", "--seed", "3", "--max_gap", "0",
                         "--out", out8])
    npz8 = np.load(out8)
    assert len(npz8["frame"]) == 725 and np.all(npz8["seen"][npz8["ids"] >= 0] == 255)
    out0 = str(tmp_path / "preds0.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", ETH, "--ksteps", "3", "--seed", "3", "--out", out0])
    assert "seen" not in np.load(out0).files and sorted(np.load(out0).files) == sorted(set(npz8.files) - {"seen"})


# ---- 6. the quality gate on the device ---------------------------------------------------------------------------------
def test_two_frame_histories_cost_little_on_eth(dev, model):
    """eth/test's 70 windows, every history cut to its last two frames and filled by stg_fill_tracks: the
    mean-trajectory ADE stays within 1.10 x the full history's, both from the project's own strict chain in this run
    (the fp64 oracle gives 1.029: the margin is for kernel rounding, nothing else)."""
    from social_stgcnn_amd import data, frames
    from social_stgcnn_amd.predict import Predictor
    win = data.load_windows(os.path.join(DATA, "eth_test"), 8, 12, 1, with_non_linear=False)
    n = len(win)
    assert n == 70
    counts = np.array([e - s for s, e in win.seq_start_end], np.int32)
    v = int(counts.max())
    obs, trgt = np.zeros((n, 8, v, 2)), np.zeros((n, 12, v, 2))
    for j, (s0, e0) in enumerate(win.seq_start_end):
        obs[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))
        trgt[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, 8:], (2, 0, 1))
    real = np.arange(v)[None] < counts[:, None]
    pred = Predictor(model, 1)
    peds = torch.from_numpy(counts).to(dev)

    def ade_fde(o):
        mean = pred.predict(o, peds, seed=0).mean.cpu().numpy().astype(np.float64)        # (N,12,V,2)
        err = np.sqrt(((mean - trgt) ** 2).sum(axis=3))                                  # (N,12,V)
        return float(err.mean(axis=1)[real].mean()), float(err[:, -1][real].mean())
    full = ade_fde(torch.from_numpy(obs).to(dev))
    cut = obs.copy()
    cut[:, :6] = 1e6                                                                    # a missed step is never read
    filled = frames.fill_tracks(torch.from_numpy(cut).to(dev), np.full((n, v), 0b11, np.int32), peds)
    assert np.array_equal(filled.cpu().numpy(), frames_fill_np.fill_tracks(cut, np.full((n, v), 0b11), counts))
    assert torch.equal(filled[:, 6:], torch.from_numpy(obs[:, 6:]).to(dev))
    short = ade_fde(filled)
    print("eth mean-trajectory ADE / FDE on the device: full %.4f / %.4f, h = 2 %.4f / %.4f, ratio %.4f"
          % (full + short + (short[0] / full[0],)))
    assert short[0] <= 1.10 * full[0], (full, short)
