"""GPU (-m gpu): per-frame scenes and predictions from raw tracks (social_stgcnn_amd.frames, csrc/frames.hip).

The recording builder against the numpy restatement on all committed recordings; predictions at the frames whose
scene is a dataset window's pedestrian set against the window path (the reference's windowing); v_pred against the
fp64 oracle, team-kernel sizes included; the live stream, eager and captured, against the recording builder; the
stream's edge cases against the push-by-push restatement; the predict_frames command."""
import argparse
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import frames_np
from live_inputs import DATA, _assert_scene, _model, _pushes, _recordings, _rows, _xy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def test_recording_scenes_equal_the_restatement_on_every_recording(dev):
    from social_stgcnn_amd import frames
    recs = _recordings()
    assert len(recs) == 14
    for rec in recs:
        rows = _rows(*rec)
        ref = frames_np.frame_scenes(rows)
        sc = frames.recording_scenes(rows, dev)
        ids, peds, obs = sc.ids.cpu().numpy(), sc.num_peds.cpu().numpy(), sc.obs_abs.cpu().numpy()
        assert sc.obs_abs.dtype == torch.float64 and sc.ids.dtype == torch.int64 and sc.num_peds.dtype == torch.int32
        assert np.array_equal(sc.frame, np.array([r[1] for r in ref])), rec
        assert ids.shape[1] == max(len(r[2]) for r in ref), rec
        for i, (_, _, rid, robs) in enumerate(ref):
            _assert_scene(ids[i], peds[i], obs[i], rid, robs, (rec, i))
    # every frame (min_peds 0, empty scenes included), a wider padding and no rounding
    rows = _rows("eth_test", "biwi_eth.txt")
    for kw in (dict(min_peds=0, v_pad=24), dict(min_peds=3, decimals=None)):
        ref = frames_np.frame_scenes(rows, min_peds=kw["min_peds"], decimals=kw.get("decimals", 4))
        sc = frames.recording_scenes(rows, dev, **kw)
        ids, peds, obs = sc.ids.cpu().numpy(), sc.num_peds.cpu().numpy(), sc.obs_abs.cpu().numpy()
        assert len(ref) == len(sc.frame) and ids.shape[1] == kw.get("v_pad", max(len(r[2]) for r in ref))
        for i, (_, _, rid, robs) in enumerate(ref):
            _assert_scene(ids[i], peds[i], obs[i], rid, robs, (kw, i))
    assert len(frames.recording_scenes(rows, dev, min_peds=0).frame) == len(np.unique(rows[:, 0])) - 7
    with pytest.raises(ValueError, match="v_pad"):
        frames.recording_scenes(rows, dev, v_pad=19)


@pytest.mark.parametrize("split,rec,n_equal", [("eth", ("eth_test", "biwi_eth.txt"), 11),
                                               ("zara1", ("zara1_test", "crowds_zara01.txt"), 186)])
def test_predictions_at_window_frames_match_the_window_path(dev, split, rec, n_equal):
    """At every frame whose scene is exactly a dataset window's pedestrian set, predict_recording's v_pred is what the
    window path gives: Predictor.predict on the window's float64 positions (data.load_windows, the reference's
    windowing).  Bit-equal at the same padding, 1e-5 at the window's own width."""
    from social_stgcnn_amd import data, frames
    from social_stgcnn_amd.predict import Predictor
    rows = _rows(*rec)
    model = _model(split, dev)
    win = data.load_windows(os.path.join(DATA, rec[0]), 8, 12, 1, with_non_linear=False, files=[rec[1]])
    starts = frames_np.dataset_windows(rows)
    assert len(starts) == len(win)
    sc, pr = frames.predict_recording(model, rows, k=4, seed=0)
    at = {fn: i for i, fn in enumerate(sc.frame)}
    all_frames = np.unique(rows[:, 0])
    ids, peds = sc.ids.cpu().numpy(), sc.num_peds.cpu().numpy()
    matched = []
    for w, (idx, wid) in enumerate(starts):
        i = at[all_frames[idx + 7]]
        if peds[i] == len(wid) and np.array_equal(ids[i, :peds[i]], wid):
            matched.append((w, i))
    assert len(matched) == n_equal
    v = ids.shape[1]
    obs = np.zeros((len(matched), 8, v, 2))
    counts = np.zeros(len(matched), np.int32)
    for j, (w, _) in enumerate(matched):
        s0, e0 = win.seq_start_end[w]
        obs[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))
        counts[j] = e0 - s0
    rows_i = [i for _, i in matched]
    assert np.array_equal(sc.obs_abs[rows_i].cpu().numpy(), obs)
    pred = Predictor(model, 4)
    ref = pred.predict(torch.from_numpy(obs).to(dev), torch.from_numpy(counts).to(dev), seed=0)
    got = pr.v_pred[rows_i]
    assert torch.equal(got, ref.v_pred)
    worst = 0.0
    for j in range(0, len(matched), max(1, len(matched) // 12)):
        c = int(counts[j])
        own = pred.predict(torch.from_numpy(np.ascontiguousarray(obs[j:j + 1, :, :c])).to(dev), seed=0).v_pred
        worst = max(worst, float((own[0] - got[j, :, :, :c]).abs().max()))
    assert worst < 1e-5, worst


@pytest.mark.parametrize("split,rec", [("univ", ("univ_test", "students001.txt")), ("eth", ("eth_test", "biwi_eth.txt"))])
def test_frame_predictions_match_the_fp64_oracle(dev, split, rec):
    from oracle import stgcnn_oracle as O
    from social_stgcnn_amd import frames
    rows = _rows(*rec)
    model = _model(split, dev)
    w = load_golden("weights_%s.npz" % split)
    state = {k: torch.from_numpy(np.array(w[k])).double() for k in w.files}
    sc, pr = frames.predict_recording(model, rows, k=1, seed=0)
    peds = sc.num_peds.cpu().numpy()
    pick = sorted(set(range(0, len(peds), 40)) | {int(np.argmax(peds))})
    if split == "univ":
        assert peds.max() == 73 and int(np.argmax(peds)) in pick          # the team kernels (V > 32)
    obs, vp = sc.obs_abs.cpu().numpy(), pr.v_pred.cpu().numpy()
    worst = 0.0
    with torch.no_grad():
        for i in pick:
            c = int(peds[i])
            rel = np.zeros((8, c, 2))
            rel[1:] = obs[i, 1:, :c] - obs[i, :-1, :c]
            rel = rel.astype(np.float32).astype(np.float64)                  # the model's float32 displacements
            nodes, lap = O.seq_to_graph_np(np.transpose(rel, (1, 2, 0)))
            x = torch.from_numpy(np.asarray(nodes, np.float64)).unsqueeze(0).permute(0, 3, 1, 2)
            y = O.social_stgcnn_forward(state, x, torch.from_numpy(np.asarray(lap, np.float64)), False)
            worst = max(worst, float(np.abs(y[0].numpy() - vp[i, :, :, :c]).max()))
    assert worst < 1e-4, worst


def _noise(i, k, v):
    g = torch.Generator()
    g.manual_seed(1000 + i)
    return torch.randn((k, 1, 12, v, 2), generator=g)


@pytest.mark.parametrize("split,rec", [("eth", ("eth_test", "biwi_eth.txt")), ("univ", ("univ_test", "students001.txt"))])
def test_stream_equals_the_recording_eager_and_captured(dev, split, rec):
    from social_stgcnn_amd import frames
    rows = _rows(*rec)
    model = _model(split, dev)
    k, v = 3, 128
    pushes = _pushes(rows)
    rec_sc = frames.recording_scenes(rows, dev, min_peds=0, v_pad=v)
    assert len(rec_sc.frame) == len(pushes) - 7
    r_ids, r_peds, r_obs = rec_sc.ids.cpu().numpy(), rec_sc.num_peds.cpu().numpy(), rec_sc.obs_abs.cpu().numpy()
    # the recording path with each frame's noise, at the stream's padding and at its own
    noise_fn = lambda b, shape: torch.cat([_noise(7 + j, k, v) for j in range(64 * b, 64 * b + shape[1])], 1)  # noqa
    _, rec_pr = frames.predict_recording(model, rows, k=k, noise_fn=noise_fn, min_peds=0, v_pad=v)
    _, own_pr = frames.predict_recording(model, rows, k=k, min_peds=0)
    own_v = own_pr.mean.shape[2]
    fp = frames.FramePredictor(model, k=k, max_peds=v)
    cap = frames.FramePredictor(model, k=k, max_peds=v)
    replay = cap.capture()
    worst = 0.0
    for i, (ids, xy) in enumerate(pushes):
        e = fp.push(ids, xy, noise=_noise(i, k, v))
        c = replay(ids, xy, seed=i)
        for out, what in ((e, "eager"), (c, "captured")):
            o_ids, o_peds, o_obs = out.ids.cpu().numpy(), out.num_peds.cpu().numpy(), out.obs_abs.cpu().numpy()
            assert int(out.flags.item()) == 0, (what, i)
            if i < 7:
                assert int(o_peds[0]) == 0 and np.all(o_ids == -1) and not np.any(o_obs), (what, i)
                continue
            j = i - 7
            assert int(o_peds[0]) == r_peds[j], (what, i)
            assert np.array_equal(o_ids, r_ids[j]) and np.array_equal(o_obs[0], r_obs[j]), (what, i)
        if i < 7:
            continue
        j = i - 7
        assert torch.equal(e.mean, rec_pr.mean[j]), i
        assert torch.equal(e.samples, rec_pr.samples[:, j]), i
        assert torch.equal(e.v_pred, rec_pr.v_pred[j]), i
        assert torch.equal(c.mean, e.mean), i
        worst = max(worst, float((e.mean[:, :own_v] - own_pr.mean[j]).abs().max()))
    assert worst < 1e-5, worst


def test_stream_flags_stay_clear_on_every_recording(dev):
    from social_stgcnn_amd import frames
    fp = frames.FramePredictor(_model("eth", dev), k=1)
    replay = fp.capture()
    for rec in _recordings():
        fp.reset()
        acc = torch.zeros(1, device=dev, dtype=torch.int32)
        most = torch.zeros(1, device=dev, dtype=torch.int32)
        for ids, xy in _pushes(_rows(*rec)):
            out = replay(ids, xy)
            acc.bitwise_or_(out.flags)
            torch.maximum(most, out.num_peds, out=most)
        assert int(acc.item()) == 0, rec
        assert int(most.item()) == max(len(s[2]) for s in frames_np.frame_scenes(_rows(*rec))), rec


def _run_script(push, script, model_ref):
    """Push every (ids, xy) of the script; each scene must be the restatement's; returns the flags."""
    flags = []
    for i, (ids, xy) in enumerate(script):
        out = push(ids, xy)
        ref_ids, ref_obs = model_ref.push(ids.cpu().numpy() if torch.is_tensor(ids) else ids,
                                          xy.cpu().numpy() if torch.is_tensor(xy) else xy)
        _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), ref_ids, ref_obs, i)
        flags.append(int(out.flags.item()))
    return flags


def test_stream_edge_cases(dev):
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    gen = np.random.default_rng(0)
    # a gap, an empty push, ids that come back after their slot was freed, a changing detection count
    script = []
    for f in range(40):
        ids = [1, 2]
        if f != 10:
            ids.append(3)                                  # 3 misses frame 10: out until frame 17
        if f < 3 or 12 <= f < 30:
            ids.append(4)                                  # 4 leaves at 3 (slot freed at 10), back at 12, leaves at 30
        if f >= 5:
            ids.append(5 + f % 3)                          # short-lived ids: slots keep turning over
        if f == 20:
            ids = []                                       # an empty push: everyone's run restarts
        ids = np.array(ids[::-1] if f % 2 else ids, np.int64)
        script.append((ids, _xy(gen, len(ids))))
    for cap in (3, 8):                                     # capacity 3: the short-lived ids overflow some frames
        for mode in ("eager", "captured"):
            fp = frames.FramePredictor(model, k=2, capacity=cap, max_detections=8)
            push = fp.push if mode == "eager" else fp.capture()
            if cap == 8:
                flags = _run_script(push, script, frames_np.StreamModel())
                assert flags == [0] * len(script), mode
            else:
                # 1, 2 and 3 arrive first and hold the three slots throughout; every other id finds no free slot
                ref = frames_np.StreamModel()
                flags = []
                for i, (ids, xy) in enumerate(script):
                    out = push(ids, xy)
                    keep = np.isin(ids, [1, 2, 3])
                    r_ids, r_obs = ref.push(ids[keep], xy[keep])
                    _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), r_ids,
                                  r_obs, (mode, i))
                    flags.append(int(out.flags.item()))
                assert all(fl in (0, frames.OVERFLOW) for fl in flags) and flags.count(frames.OVERFLOW) > 20, mode
    # a repeated id within a push given as device tensors: flag, the first detection wins
    for mode in ("eager", "captured"):
        fp = frames.FramePredictor(model, k=2)
        push = fp.push if mode == "eager" else fp.capture()
        ref = frames_np.StreamModel()
        flags = []
        for f in range(12):
            ids = np.array([4, 9, 4, 1] if f % 3 == 0 else [9, 4, 1], np.int64)
            xy = _xy(gen, len(ids))
            out = push(torch.from_numpy(ids).to(dev), torch.from_numpy(xy).to(dev))
            r_ids, r_obs = ref.push(ids, xy)
            _assert_scene(out.ids.cpu().numpy(), out.num_peds.item(), out.obs_abs[0].cpu().numpy(), r_ids, r_obs, f)
            flags.append(int(out.flags.item()))
        assert flags == [frames.DUPLICATE if f % 3 == 0 else 0 for f in range(12)], mode
    # more fully observed pedestrians than max_peds: the smallest ids, flag
    for mode in ("eager", "captured"):
        fp = frames.FramePredictor(model, k=2, max_peds=3)
        push = fp.push if mode == "eager" else fp.capture()
        script = [(np.array([7, 3, 11, 5, 2], np.int64), _xy(gen, 5)) for _ in range(10)]
        flags = _run_script(push, script, frames_np.StreamModel(max_peds=3))
        assert flags == [0] * 7 + [frames.TOO_MANY] * 3, mode
    # host arrays with a repeated id are refused before any copy
    fp = frames.FramePredictor(model, k=2)
    with pytest.raises(ValueError, match="duplicate"):
        fp.push(np.array([1, 1]), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="max_detections"):
        fp.push(np.arange(1025), np.zeros((1025, 2)))


def test_predict_frames_command_writes_the_recording_predictions(dev, tmp_path):
    from social_stgcnn_amd import frames, predict_frames
    from social_stgcnn_amd.trainer import Checkpoint
    model = _model("eth", dev)
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    rec = os.path.join(DATA, "eth_test", "biwi_eth.txt")
    out = str(tmp_path / "preds.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", rec, "--ksteps", "5", "--seed", "3", "--out", out])
    got = np.load(out)
    sc, pr = frames.predict_recording(model, _rows("eth_test", "biwi_eth.txt"), k=5, seed=3)
    assert np.array_equal(got["frame"], sc.frame)
    assert np.array_equal(got["ids"], sc.ids.cpu().numpy()) and np.array_equal(got["num_peds"], sc.num_peds.cpu().numpy())
    assert np.array_equal(got["mean"], pr.mean.cpu().numpy())
    assert np.array_equal(got["samples"], pr.samples.cpu().numpy())
