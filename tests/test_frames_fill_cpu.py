"""CPU: the rule for partially observed tracks (frames.TrackRule) as tests/frames_fill_np.py states it:
with (obs_len, 0) it is the strict rule of tests/frames_np.py on the six test recordings, recording form and push by
push; a hand-worked window; what TrackRule and the entry points refuse; and what a filled history costs in accuracy,
with the fp64 oracle on eth's 70 test windows."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import frames_fill_np
import frames_np

DATA = os.path.join(GOLDEN, "data")
TEST_RECORDINGS = (("eth_test", "biwi_eth.txt"), ("hotel_test", "biwi_hotel.txt"), ("univ_test", "students001.txt"),
                   ("univ_test", "students003.txt"), ("zara1_test", "crowds_zara01.txt"),
                   ("zara2_test", "crowds_zara02.txt"))


def _rows(d, f):
    from social_stgcnn_amd import data
    return data.read_file(os.path.join(DATA, d, f))


def _pushes(rows):
    frames = np.unique(rows[:, 0])
    f_idx = np.searchsorted(frames, rows[:, 0])
    order = np.argsort(f_idx, kind="stable")
    bounds = np.searchsorted(f_idx[order], np.arange(len(frames) + 1))
    return [(rows[order[a:b], 1].astype(np.int64), rows[order[a:b], 2:4]) for a, b in zip(bounds[:-1], bounds[1:])]


@pytest.mark.parametrize("rec", TEST_RECORDINGS)
def test_strict_rule_through_the_statement_is_the_strict_statement(rec):
    rows = _rows(*rec)
    ref = frames_np.frame_scenes(rows, min_peds=0)
    got = frames_fill_np.frame_scenes_rule(rows, 8, 8, 0, min_peds=0)
    assert len(ref) == len(got) == len(np.unique(rows[:, 0])) - 7
    for (f, fn, ids, obs), (f2, fn2, ids2, obs2, seen2) in zip(ref, got):
        assert f == f2 and fn == fn2
        assert np.array_equal(ids, ids2) and np.array_equal(obs, obs2)
        assert seen2.dtype == np.int32 and np.all(seen2 == 255)
    # push by push, on the first 120 frames (the dict-per-push model is slow on the crowded recordings)
    a, b = frames_np.StreamModel(), frames_fill_np.StreamModelRule()
    for i, (ids, xy) in enumerate(_pushes(rows)[:120]):
        r_ids, r_obs = a.push(ids, xy)
        g_ids, g_obs, g_seen, more = b.push(ids, xy)
        assert np.array_equal(r_ids, g_ids) and np.array_equal(r_obs, g_obs) and not more, (rec, i)
        if i >= 7:
            assert np.array_equal(g_ids, ref[i - 7][2]), (rec, i)


def test_recording_and_push_statements_agree_under_a_loose_rule():
    rows = _rows("eth_test", "biwi_eth.txt")
    rows = rows[np.random.default_rng(3).random(len(rows)) >= 0.1]
    frames = np.unique(rows[:, 0])
    rows = rows[rows[:, 0] <= frames[150]]
    ref = {s[0]: s for s in frames_fill_np.frame_scenes_rule(rows, 8, 2, 2, min_peds=0)}
    m = frames_fill_np.StreamModelRule(8, 2, 2)
    filled = 0
    for f, (ids, xy) in enumerate(_pushes(rows)):
        g_ids, g_obs, g_seen, _ = m.push(ids, xy)
        if f == 0:
            assert len(g_ids) == 0 and 0 not in ref
            continue
        _, _, r_ids, r_obs, r_seen = ref[f]
        assert np.array_equal(g_ids, r_ids) and np.array_equal(g_obs, r_obs) and np.array_equal(g_seen, r_seen), f
        filled += int(np.sum(r_seen != 255))
    assert filled > 100


def test_a_hand_worked_window():
    """Steps 2, 3, 6 and 7 seen: an interior gap of two steps and two leading steps."""
    present = np.array([0, 0, 1, 1, 0, 0, 1, 1], dtype=bool)
    pos = np.zeros((8, 2))
    pos[[2, 3, 6, 7]] = [[1.0, 0.0], [1.3, -0.5], [2.2, 1.0], [2.5, 1.0]]
    got = frames_fill_np.fill_window(pos, present, 4)
    #   interior: 1.3 + 0.9 * 1/3, 1.3 + 0.9 * 2/3 and -0.5 + 1.5 * 1/3, -0.5 + 1.5 * 2/3
    #   leading:  d = q[3] - q[2] = (0.3, -0.5): q[2] - d, q[2] - 2 d
    want = np.array([[0.4, 1.0], [0.7, 0.5], [1.0, 0.0], [1.3, -0.5], [1.6, 0.0], [1.9, 0.5], [2.2, 1.0], [2.5, 1.0]])
    assert np.array_equal(got, want)
    assert frames_fill_np.seen_bits(present) == 0b00110011
    assert np.array_equal(frames_fill_np.present_of(0b00110011, 8), present)
    assert frames_fill_np.is_member(present, 4, 2) and frames_fill_np.is_member(present, 2, 6)
    assert not frames_fill_np.is_member(present, 4, 1) and not frames_fill_np.is_member(present, 5, 2)
    assert not frames_fill_np.is_member(np.roll(present, -1), 2, 6)               # not seen now
    # without rounding the interpolation weight is the quotient, not a product of reciprocals
    raw = frames_fill_np.fill_window(pos, present, None)
    assert raw[4, 0] == 1.3 + (2.2 - 1.3) * (1.0 / 3.0) and raw[0, 0] == 1.0 - 2.0 * (1.3 - 1.0)
    # the second step of the window may itself be a filled one: step 0 seen, steps 1..6 missed
    sparse = np.array([1, 0, 0, 0, 0, 0, 0, 1], dtype=bool)
    p2 = np.zeros((8, 2))
    p2[7] = [7.0, -3.5]
    assert np.array_equal(frames_fill_np.fill_window(p2, sparse, 4)[:, 0], np.arange(8.0))
    # a leading fill whose velocity comes from a filled step: steps 3 and 5 seen only
    late = np.array([0, 0, 0, 1, 0, 1, 0, 1], dtype=bool)
    p3 = np.zeros((8, 2))
    p3[[3, 5, 7]] = [[3.0, 0.0], [5.0, 0.0], [9.0, 0.0]]
    assert frames_fill_np.fill_window(p3, late, 4)[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 7.0, 9.0]
    # the batch form: columns not seen now, seen once or past num_peds stay as they are
    obs = np.arange(2 * 8 * 3 * 2, dtype=np.float64).reshape(2, 8, 3, 2) + 0.123456
    seen = np.array([[0b11, 0b10, 0b1], [0b10000001, 0b11, 0b11]])
    out = frames_fill_np.fill_tracks(obs, seen, num_peds=[3, 1])
    assert np.array_equal(out[0, :, 1:], obs[0, :, 1:]) and np.array_equal(out[1, :, 1:], obs[1, :, 1:])
    assert np.array_equal(out[0, 6:, 0], np.around(obs[0, 6:, 0], 4)) and not np.array_equal(out[0, :6, 0], obs[0, :6, 0])


def test_track_rule_refusals():
    from social_stgcnn_amd.frames import FramePredictor, TrackRule, recording_scenes
    assert TrackRule(2, 6) == (2, 6) and TrackRule(8) == (8, 0) and TrackRule(3, 1).max_gap == 1
    for bad in (1, 0, 33, 2.5, True, -3):
        with pytest.raises(ValueError, match=r"min_seen must be an integer in \[2, obs_len"):
            TrackRule(bad, 0)
    for bad in (-1, 31, 0.5, False):
        with pytest.raises(ValueError, match=r"max_gap must be an integer in \[0, obs_len - 2"):
            TrackRule(2, bad)
    with pytest.raises(ValueError, match="min_seen=9 > obs_len=8"):
        TrackRule(9, 0).checked(8)
    with pytest.raises(ValueError, match=r"max_gap=7 > obs_len - 2 = 6"):
        TrackRule(2, 7).checked(8)
    assert TrackRule(8, 6).checked(8) == (8, 6)
    rows = _rows("eth_test", "biwi_eth.txt")
    with pytest.raises(ValueError, match="min_seen=9"):
        recording_scenes(rows, "cpu", tracks=TrackRule(9, 0))
    with pytest.raises(ValueError, match="max_gap=3"):
        recording_scenes(rows, "cpu", obs_len=4, tracks=(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        recording_scenes(rows, "cpu", tracks=TrackRule(2, 2))
    from social_stgcnn_amd.model import social_stgcnn
    model = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
    with pytest.raises(ValueError, match="max_gap=7"):
        FramePredictor(model, tracks=TrackRule(2, 7))


def test_rule_entry_points_reject_bad_arguments_without_a_gpu():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call
    for t, ms, mg in ((8, 1, 0), (8, 9, 0), (8, 2, 7), (8, 2, -1), (1, 2, 0), (33, 2, 0)):
        assert L.stg_frame_scene_counts_rule(f, f, 4, t, ms, mg, f, None) == -1, (t, ms, mg)
        assert b"min_seen" in L.stg_last_error()
        assert L.stg_frame_scenes_rule(f, f, f, f, 2, 4, t, 1e4, ms, mg, f, f, f, f, None) == -1
        assert L.stg_track_push_rule(f, f, f, 8, f, f, f, f, 16, t, 1e4, 4, ms, mg, f, f, f, f, None) == -1
        assert L.stg_track_push_streams_rule(f, 1, f, 2, 8, f, f, 2, 8, f, f, f, f, 16, t, 1e4, 4, ms, mg, f, f, f, f, f,
                                             0, None) == -1
    assert L.stg_frame_scene_counts_rule(None, None, 0, 8, 2, 2, None, None) == 0          # F == 0: nothing to launch
    assert L.stg_frame_scenes_rule(None, None, None, None, 0, 4, 8, 1e4, 2, 2, None, None, None, None, None) == 0
    assert L.stg_frame_scenes_rule(f, f, f, f, 2, 4, 8, 1e4, 2, 2, f, f, f, None, None) == -1    # seen is required
    assert b"null" in L.stg_last_error()
    assert L.stg_track_push_rule(f, f, f, 8, f, f, f, f, 16, 8, 1e4, 4, 2, 2, f, f, f, None, None) == -1
    assert L.stg_track_push_rule(f, f, f, 0, f, f, f, f, 16, 8, 1e4, 4, 2, 2, f, f, f, f, None) == -1
    assert L.stg_track_push_streams_rule(f, 1, f, 2, 8, f, f, 2, 8, f, f, f, f, 16, 8, 1e4, 4, 2, 2, f, f, f, f, f, 128,
                                         None) == -1
    assert b"block_threads" in L.stg_last_error()
    assert L.stg_fill_tracks(None, None, None, 0, 8, 4, 1e4, None) == 0
    for n, t, v in ((-1, 8, 4), (2, 1, 4), (2, 33, 4), (2, 8, 0)):
        assert L.stg_fill_tracks(f, f, None, n, t, v, 1e4, None) == -1, (n, t, v)
    assert L.stg_fill_tracks(f, None, None, 2, 8, 4, 1e4, None) == -1
    assert L.stg_abi_version() == 8


def _oracle_mean_errors(state, obs, trgt):
    """Mean-trajectory (ADE, FDE) sums of one window: obs (8,V,2) float64, trgt (12,V,2) -> per-pedestrian arrays."""
    from oracle import stgcnn_oracle as O
    rel = np.zeros_like(obs)
    rel[1:] = obs[1:] - obs[:-1]
    rel = rel.astype(np.float32).astype(np.float64)
    nodes, lap = O.seq_to_graph_np(np.transpose(rel, (1, 2, 0)))
    x = torch.from_numpy(np.asarray(nodes, np.float64)).unsqueeze(0).permute(0, 3, 1, 2)
    with torch.no_grad():
        y = O.social_stgcnn_forward(state, x, torch.from_numpy(np.asarray(lap, np.float64)), False)[0].numpy()
    mean = np.cumsum(np.transpose(y[:2], (1, 2, 0)), axis=0) + obs[-1][None]             # (12,V,2)
    err = np.sqrt(((mean - trgt) ** 2).sum(axis=2))
    return err.mean(axis=0), err[-1]


def test_what_a_filled_history_costs_on_eth():
    """The issue's table for eth, fp64 oracle, shipped weights, mean-trajectory ADE / FDE over the 70 test windows:
    0.988 / 1.804 at the full history, 1.016 / 1.834 with every pedestrian cut to the last h = 2 frames and filled
    backwards, 1.000 / 1.817 at h = 3.  Back-filling stays within 1.10 x the full history; holding the first seen
    position (out of distribution: a pedestrian who stood still and then jumps) does not."""
    from social_stgcnn_amd import data
    win = data.load_windows(os.path.join(DATA, "eth_test"), 8, 12, 1, with_non_linear=False)
    assert len(win) == 70
    w = load_golden("weights_eth.npz")
    state = {k: torch.from_numpy(np.array(w[k])).double() for k in w.files}
    res = {}
    for name in ("h8", "h3", "h2", "hold2"):
        ades, fdes = [], []
        for s0, e0 in win.seq_start_end:
            full = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))                         # (8,V,2) float64
            trgt = np.transpose(win.seq[s0:e0, :, 8:], (2, 0, 1))
            if name == "h8":
                obs = full
            elif name == "hold2":
                obs = full.copy()
                obs[:6] = full[6]
            else:
                h = int(name[1:])
                junk = full.copy()
                junk[:8 - h] = 1e6                                                      # a missed step is never read
                obs = frames_fill_np.fill_tracks(junk[None], np.full((1, e0 - s0), (1 << h) - 1))[0]
                assert np.array_equal(obs[8 - h:], full[8 - h:])
            a, f = _oracle_mean_errors(state, obs, trgt)
            ades += a.tolist()
            fdes += f.tolist()
        res[name] = (float(np.mean(ades)), float(np.mean(fdes)))
    print("eth mean-trajectory ADE / FDE:", {k: (round(a, 4), round(f, 4)) for k, (a, f) in res.items()})
    assert abs(res["h8"][0] - 0.988) < 1e-3 and abs(res["h8"][1] - 1.804) < 1e-3
    assert abs(res["h2"][0] - 1.016) < 1e-3 and abs(res["h2"][1] - 1.834) < 1e-3
    assert abs(res["h3"][0] - 1.000) < 1e-3 and abs(res["h3"][1] - 1.817) < 1e-3
    assert res["h2"][0] <= 1.10 * res["h8"][0]
    assert res["hold2"][0] > 1.10 * res["h8"][0]
