"""GPU (-m gpu): the window harvest (csrc/harvest.hip).

Both entry points through the C ABI, behind the real push kernel, against the numpy restatement (harvest_np) fed the
kernels' own track state, bit for bit: appearing and vanishing tracks, a gap, slot reuse, slots running out, negative
and non-contiguous ids, both ways of filling the log, an unpushed stream; the streams entry point against lone calls;
the predictors -- snapshot() against data.load_windows on whole recordings, eager and captured, capture() on a half-fed
predictor, reset, TrackRule, three streams against three lone predictors; training on a snapshot against training on the
host-built dataset; fine_tune; the predict_frames command."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import harvest_np as H
from live_inputs import DATA, Schedule, _model, _pushes, _rows

pytestmark = pytest.mark.gpu
S, NS = 16, 3
OVERFLOW = 2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- 1. through the C ABI -----------------------------------------------------------------------------------------------
def _script(t_obs, t_all, ticks, seed):
    """ticks x NS entries (ids, xy) or None (not pushed).  Per stream: long tracks with a negative and a huge id, one
    with a gap, one that vanishes, one that leaves for more than T_obs pushes and comes back (its slot is reused in
    between), a late one, and a crowd of 14 short-lived ids that runs the 16 slots out; stream 1 skips every fourth
    tick."""
    gen = np.random.default_rng(seed)
    out = []
    for t in range(ticks):
        tick = []
        for s in range(NS):
            if s == 1 and t % 4 == 2:
                tick.append(None)
                continue
            ids = [3, -5, (1 << 33) + 7 + s, 1000]
            if t != t_all + 3:
                ids.append(11 + s)                               # a gap
            if t < ticks * 2 // 3:
                ids.append(40)                                   # vanishes
            if t < 6 or t >= 6 + t_obs + 2:
                ids.append(77)                                   # leaves, comes back to another slot
            if 7 <= t < 7 + t_obs + 1:
                ids.append(500 + t % 2)                          # short tracks that take the freed slot
            if t >= 10:
                ids.append(2)                                    # late, the smallest id
            if t_all + 8 <= t < t_all + 10:
                ids += list(range(200, 214))                     # the crowd: more ids than slots
            ids = np.array(ids, np.int64)[gen.permutation(len(ids))]
            tick.append((ids, gen.uniform(-20, 20, size=(len(ids), 2))))
        out.append(tick)
    return out


class _Rig:
    """The track state of NS streams and the harvest's history, log and scratch, all pre-filled: the log with 7s, so a
    store past the fill point shows."""

    def __init__(self, dev, t_obs, t_all, cap_w, cap_r, lead=(NS,), S=S):
        z = lambda shape, dt: torch.zeros(shape, device=dev, dtype=dt)      # noqa: E731
        self.track = (torch.full(lead + (S,), -1, device=dev, dtype=torch.int64), z(lead + (S,), torch.int32),
                      z(lead + (t_obs, S, 2), torch.float64), z(lead + (2,), torch.int32))
        self.hist = (z(lead + (S,), torch.int32), z(lead + (t_all, S, 2), torch.float64), z(lead + (2,), torch.int32))
        self.ns = lead[0]
        self.work = z(self.ns * (S + 3), torch.int32)
        self.log = (torch.full((cap_r, 2, t_all), 7.0, device=dev), torch.full((cap_w + 1,), -7, device=dev, dtype=torch.int32),
                    torch.full((cap_w, 2), -7, device=dev, dtype=torch.int32), z(3, torch.int32))
        self.log[1][0] = 0
        self.dims, self.caps = (S, t_obs, t_all), (cap_w, cap_r)

    def same_log(self, other):
        return all(torch.equal(a, b) for a, b in zip(self.log, other.log))


def _push_streams(rig, tick, dev, t_obs, m_max=32):
    """stg_track_push_streams on one tick -> the per-stream flags"""
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    counts = [0 if d is None else len(d[0]) for d in tick]
    start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    pushed = torch.tensor([int(d is not None) for d in tick], dtype=torch.int32).to(dev)
    ids = np.concatenate([d[0] for d in tick if d is not None] + [np.zeros(1, np.int64)])
    xy = np.concatenate([d[1] for d in tick if d is not None] + [np.zeros((1, 2))])
    det_id, det_xy = torch.from_numpy(ids).to(dev), torch.from_numpy(xy).to(dev)
    v = 8
    obs = torch.empty((NS, t_obs, v, 2), device=dev, dtype=torch.float64)
    out_ids = torch.empty((NS, v), device=dev, dtype=torch.int64)
    peds, flags = (torch.empty(NS, device=dev, dtype=torch.int32) for _ in range(2))
    check(lib().stg_track_push_streams(ptr(det_id), 1, ptr(det_xy), 2, len(ids), ptr(start), ptr(pushed), NS, m_max,
                                       *map(ptr, rig.track), S, t_obs, ctypes.c_double(1e4), v, ptr(obs), ptr(out_ids),
                                       ptr(peds), ptr(flags), 0, stream_ptr()), "stg_track_push_streams")
    return pushed, flags.cpu().numpy()


def _harvest_streams(rig, track, pushed, min_peds=2):
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    check(lib().stg_window_harvest_streams(*map(ptr, track), ptr(pushed), rig.ns, *rig.dims, min_peds, *map(ptr, rig.hist),
                                           ptr(rig.work), *map(ptr, rig.log), *rig.caps, stream_ptr()),
          "stg_window_harvest_streams")


def _harvest_lone(rig, track, b, min_peds=2):
    """the lone entry point on stream b's slices"""
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    check(lib().stg_window_harvest(*(ptr(x[b]) for x in track), *rig.dims, min_peds, b, *(ptr(x[b]) for x in rig.hist),
                                   *map(ptr, rig.log), *rig.caps, stream_ptr()), "stg_window_harvest")


def _np_log(ref):
    return ref.log.rel_all, ref.log.win_start, ref.log.win_tag, ref.log.header


@pytest.mark.parametrize("t_obs,t_all,ticks,caps", [(3, 5, 34, (400, 4000)), (3, 5, 34, (21, 4000)), (3, 5, 34, (400, 50)),
                                                    (8, 20, 60, (400, 4000)), (8, 20, 60, (400, 131))])
def test_both_entry_points_equal_the_restatement(dev, t_obs, t_all, ticks, caps):
    """Scripted ticks of three streams: the streams entry point, and lone calls per pushed stream in stream order on a
    second history and log, against harvest_np fed the kernels' own track state.  Every tensor of the history and of the
    log -- the 7s behind the fill point included -- bit for bit after every tick."""
    streams, lone = _Rig(dev, t_obs, t_all, *caps), _Rig(dev, t_obs, t_all, *caps)
    ref = H.Harvester(NS, S, t_all, *caps)
    ref.log.rel_all[:], ref.log.win_start[1:], ref.log.win_tag[:] = 7.0, -7, -7
    seen_flags = 0
    for t, tick in enumerate(_script(t_obs, t_all, ticks, 5)):
        pushed, flags = _push_streams(streams, tick, dev, t_obs)
        seen_flags |= int(np.bitwise_or.reduce(flags))
        _harvest_streams(streams, streams.track, pushed)
        for b in range(NS):
            if tick[b] is not None:
                _harvest_lone(lone, streams.track, b)
        host = [x.cpu().numpy() for x in streams.track]
        ref.tick({b: (host[0][b], host[1][b], host[2][b], int(host[3][b, 0])) for b in range(NS) if tick[b] is not None})
        for got, want in zip(streams.log, _np_log(ref)):
            assert got.cpu().numpy().tobytes() == want.tobytes(), t
        assert np.array_equal(streams.hist[0].cpu().numpy(), np.stack([h.word for h in ref.hist])), t
        assert np.array_equal(streams.hist[2].cpu().numpy(), np.array([[h.row, h.pushes] for h in ref.hist])), t
        assert streams.same_log(lone) and all(torch.equal(a, b) for a, b in zip(streams.hist, lone.hist)), t
    n_w, n_r, dropped = (int(x) for x in ref.log.header)
    sizes = set(ref.log.num_peds.tolist())
    assert seen_flags & OVERFLOW and n_w >= 5 and set(ref.log.tags[:, 0].tolist()) == {0, 1, 2}
    if caps == (400, 4000):
        assert dropped == 0 and n_w >= 60 and len(sizes) >= 3
    elif caps[0] == 21:
        assert dropped > 0 and n_w == 21 and n_r < caps[1]         # full by windows
    else:
        assert dropped > 0 and n_w < caps[0] and n_r <= caps[1]    # full by rows
    # the positions behind the rows: every ring row a word calls detected equals the restatement's
    ring = streams.hist[1].cpu().numpy()
    for b, h in enumerate(ref.hist):
        for back in range(t_all):
            on = ((h.word >> back) & 1) == 1
            assert np.array_equal(ring[b, (h.row - back) % t_all][on], h.ring[(h.row - back) % t_all][on])


def test_a_second_pass_over_the_slots(dev):
    """272 slots for the 256 threads of the workgroup: the pass over the slots runs twice, the second time ragged, with
    candidates in it whose rank goes on from the first pass's count.  harvest_np.wide_script through both entry points,
    the track state written straight into the state tensors from harvest_np.TrackModel (the harvest reads nothing
    else): words, head, log and header bit for bit after every tick, lone calls against the streams call; the
    conditions (tests/test_harvest_cpu.py holds them without a GPU) on the statement itself."""
    t_obs, t_all, caps = 3, 5, (16, 1024)
    streams, lone = (_Rig(dev, t_obs, t_all, *caps, lead=(H.WIDE_NS,), S=H.WIDE_S) for _ in range(2))
    ids, words, windows = [], [], []
    for t, (tick, states, ref, slots) in enumerate(H.wide_ticks(H.wide_script(), t_obs, t_all, caps)):
        if t == 0:                                                # (the log is empty until tick 4)
            ref.log.rel_all[:], ref.log.win_start[1:], ref.log.win_tag[:] = 7.0, -7, -7
        slot_id, mask, pos = (np.stack([s[i] for s in states]) for i in range(3))
        for x, host in zip(streams.track, (slot_id, mask.astype(np.int32), pos)):
            x.copy_(torch.from_numpy(host).to(dev))
        streams.track[3][:, 0] = torch.tensor([s[3] for s in states], dtype=torch.int32).to(dev)
        pushed = torch.tensor([int(d is not None) for d in tick], dtype=torch.int32).to(dev)
        _harvest_streams(streams, streams.track, pushed)
        for b in range(H.WIDE_NS):
            if tick[b] is not None:
                _harvest_lone(lone, streams.track, b)
        for got, want in zip(streams.log, _np_log(ref)):
            assert got.cpu().numpy().tobytes() == want.tobytes(), t
        assert np.array_equal(streams.hist[0].cpu().numpy(), np.stack([h.word for h in ref.hist])), t
        assert np.array_equal(streams.hist[2].cpu().numpy(), np.array([[h.row, h.pushes] for h in ref.hist])), t
        assert streams.same_log(lone) and all(torch.equal(a, b) for a, b in zip(streams.hist, lone.hist)), t
        ids.append(states[0][0].copy())
        words.append(ref.hist[0].word.copy())
        windows.append(slots)
    assert H.wide_conditions(ids, words, ref.hist[0].full, windows)
    ring = streams.hist[1].cpu().numpy()                          # the positions behind the rows, as above
    for b, h in enumerate(ref.hist):
        for back in range(t_all):
            on = ((h.word >> back) & 1) == 1
            assert np.array_equal(ring[b, (h.row - back) % t_all][on], h.ring[(h.row - back) % t_all][on])


def test_every_refusal_launches_nothing(dev):
    """A refused call leaves the history, the log and the scratch as they were (pointers to real memory this time)."""
    from social_stgcnn_amd._lib import lib, ptr
    rig = _Rig(dev, 3, 5, 8, 64)
    for x in rig.hist + (rig.work,):
        x.fill_(3)
    rig.log[3].copy_(torch.tensor([2, 5, 0]))
    before = [x.clone() for x in rig.hist + rig.log + (rig.work,)]
    pushed = torch.ones(NS, device=dev, dtype=torch.int32)
    L = lib()

    def many(ns=NS, s=S, t_obs=3, t_all=5, min_peds=2, cap_w=8, cap_r=64, pushed=pushed, work=rig.work):
        return L.stg_window_harvest_streams(*map(ptr, rig.track), ptr(pushed), ns, s, t_obs, t_all, min_peds,
                                            *map(ptr, rig.hist), ptr(work), *map(ptr, rig.log), cap_w, cap_r, None)

    def one(s=S, t_obs=3, t_all=5, min_peds=2, tag=0, cap_w=8, cap_r=64):
        return L.stg_window_harvest(*(ptr(x[0]) for x in rig.track), s, t_obs, t_all, min_peds, tag,
                                    *(ptr(x[0]) for x in rig.hist), *map(ptr, rig.log), cap_w, cap_r, None)
    for kw in (dict(ns=0), dict(ns=4097), dict(s=0), dict(s=2049), dict(t_obs=0), dict(t_all=33), dict(t_obs=5),
               dict(min_peds=0), dict(cap_w=0), dict(cap_r=0), dict(pushed=None), dict(work=None)):
        assert many(**kw) == -1, kw
        assert L.stg_last_error().startswith(b"stg_window_harvest_streams:"), kw
    for kw in (dict(s=0), dict(s=2049), dict(t_obs=0), dict(t_all=33), dict(t_all=3), dict(min_peds=0), dict(tag=-1),
               dict(cap_w=0), dict(cap_r=0)):
        assert one(**kw) == -1, kw
        assert L.stg_last_error().startswith(b"stg_window_harvest:"), kw
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(rig.hist + rig.log + (rig.work,), before))


# ---- 2. the predictors ----------------------------------------------------------------------------------------------------
def _windows(d, f, dev=None):
    from social_stgcnn_amd import data
    return data.load_windows(os.path.join(DATA, d), files=[f], with_non_linear=False)


def _assert_snapshot(snap, win, what):
    assert np.array_equal(snap.num_peds_host, win.num_peds), what
    assert snap.rel_all.cpu().numpy().tobytes() == win.seq_rel.astype(np.float32).tobytes(), what
    assert np.array_equal(snap.win_start.cpu().numpy(), np.concatenate([[0], np.cumsum(win.num_peds)])), what
    assert (snap.t_obs, snap.t_pred, snap.v_max, len(snap)) == (8, 12, int(win.num_peds.max()), len(win)), what


@pytest.fixture(scope="module")
def eth(dev):
    """biwi_eth pushed through a captured harvesting predictor and, eagerly, through one without: (the harvesting
    predictor, its snapshot, the reference windows, whether every prediction was equal)."""
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    pushes = _pushes(_rows("eth_test", "biwi_eth.txt"))
    fp = frames.FramePredictor(model, k=2, max_peds=16, max_detections=32, capacity=64, harvest=frames.HarvestSpec(128))
    plain = frames.FramePredictor(model, k=2, max_peds=16, max_detections=32, capacity=64)
    replay = fp.capture()
    same = True
    for f, (ids, xy) in enumerate(pushes):
        a, b = replay(ids, xy, seed=f), plain.push(ids, xy, seed=f)
        same = same and all(torch.equal(x, y) for x, y in zip(a, b))
    return fp, fp.harvest.snapshot(), _windows("eth_test", "biwi_eth.txt"), same


def test_snapshot_of_biwi_eth_captured_equals_load_windows(eth):
    fp, snap, win, same = eth
    assert fp.harvest.counts() == (70, 181, 0)
    _assert_snapshot(snap, win, "captured")
    assert snap.rel_all.data_ptr() == fp.harvest.rel_all.data_ptr() and snap.win_start.data_ptr() == fp.harvest.win_start.data_ptr()
    tags = fp.harvest.tags()
    assert tags.shape == (70, 2) and not tags[:, 0].any() and np.all(np.diff(tags[:, 1]) > 0)
    assert same, "the predictions of a harvesting predictor equal those of one without"


def test_snapshot_eager_and_under_a_track_rule(dev, eth):
    """Eager pushes, strict and under TrackRule(2, 2): filled frames are gaps to the harvest, so both logs are the strict
    one.  clear() empties the log and the snapshot raises."""
    from social_stgcnn_amd import frames
    model, win = _model("eth", dev), eth[2]
    pushes = _pushes(_rows("eth_test", "biwi_eth.txt"))
    for tracks in (None, frames.TrackRule(2, 2)):
        fp = frames.FramePredictor(model, k=1, max_peds=16, max_detections=32, capacity=64, tracks=tracks,
                                   harvest=(128, None, 2, None))
        for ids, xy in pushes:
            fp.push(ids, xy)
        _assert_snapshot(fp.harvest.snapshot(), win, tracks)
    fp.harvest.clear()
    assert fp.harvest.counts() == (0, 0, 0)
    with pytest.raises(ValueError, match="no window"):
        fp.harvest.snapshot()


def test_crowds_of_fifty_and_capture_on_a_half_fed_predictor(dev, tmp_path):
    """The first 60 frames of students001 written to a file of their own (crowds of about 50, the team kernels):
    snapshot() equals load_windows of that file, eager; and captured from push 30 on, with capture() leaving the history
    and the log bitwise as they were."""
    from social_stgcnn_amd import data, frames
    rows = _rows("univ_test", "students001.txt")
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[59]]
    with open(tmp_path / "first60.txt", "w") as fh:
        for r in rows:
            fh.write("%s\t%s\t%s\t%s\n" % (repr(float(r[0])), repr(float(r[1])), repr(float(r[2])), repr(float(r[3]))))
    win = data.load_windows(str(tmp_path), files=["first60.txt"], with_non_linear=False)
    assert len(win) == 41 and win.num_peds.max() >= 45
    model = _model("univ", dev)
    pushes = _pushes(rows)
    kw = dict(k=1, max_peds=128, max_detections=128, capacity=256)
    eager = frames.FramePredictor(model, harvest=frames.HarvestSpec(64), **kw)
    for ids, xy in pushes:
        eager.push(ids, xy)
    _assert_snapshot(eager.harvest.snapshot(), win, "eager")
    half = frames.FramePredictor(model, harvest=frames.HarvestSpec(64), **kw)
    for ids, xy in pushes[:30]:
        half.push(ids, xy)
    log = half.harvest
    kept = (half.h_word, half.h_ring, half.h_head, log.rel_all, log.win_start, log.win_tag, log.header)
    before = [x.clone() for x in kept]
    replay = half.capture()
    assert all(torch.equal(a, b) for a, b in zip(kept, before)) and log.counts()[0] == 11
    for ids, xy in pushes[30:]:
        replay(ids, xy)
    _assert_snapshot(log.snapshot(), win, "captured from push 30")
    assert all(torch.equal(a, b) for a, b in zip(eager.harvest.__dict__.values(), log.__dict__.values())
               if torch.is_tensor(a))


def test_three_streams_against_three_lone_predictors(dev):
    """A schedule with skipped streams and a late start, captured; stream 1 reset at tick 40.  The one log holds, tick
    by tick and stream by stream, the windows of three lone predictors fed the same pushes, its tags their push
    indices."""
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    pushes = [_pushes(_rows("eth_test", "biwi_eth.txt"))[150:240], _pushes(_rows("hotel_test", "biwi_hotel.txt"))[:80],
              _pushes(_rows("zara1_test", "crowds_zara01.txt"))[:70]]
    kw = dict(k=1, max_peds=16, max_detections=32, capacity=64)
    sp = frames.StreamsPredictor(model, 3, harvest=frames.HarvestSpec(256), **kw)
    lone = [frames.FramePredictor(model, harvest=frames.HarvestSpec(128), **kw) for _ in range(3)]
    replay = sp.capture()
    sched = Schedule(pushes, [0, 3, 1])
    order, skipped, n1 = [], 0, 0
    for t in range(100):
        if t == 40:
            sp.reset(streams=[1])
            lone[1].reset()
        tick = sched.tick(t)
        skipped += sum(d is None for d in tick)
        n1 += int(t < 40 and tick[1] is not None)              # stream 1's pushes ahead of its reset
        before = [p.harvest.counts()[0] for p in lone]
        for s, d in enumerate(tick):
            if d is not None:
                lone[s].push(*d)
        order += [s for s in range(3) if lone[s].harvest.counts()[0] > before[s]]
        replay(tick)
    assert skipped > 30 and len(order) > 60 and set(order) == {0, 1, 2}
    n_w, n_r, dropped = sp.harvest.counts()
    assert (n_w, dropped) == (len(order), 0)
    tags, start = sp.harvest.tags(), sp.harvest.win_start.cpu().numpy()
    assert tags[:, 0].tolist() == order
    rel = sp.harvest.rel_all.cpu().numpy()
    cursor = [0, 0, 0]
    lone_logs = [(p.harvest.rel_all.cpu().numpy(), p.harvest.win_start.cpu().numpy(), p.harvest.tags()) for p in lone]
    for w, s in enumerate(order):
        l_rel, l_start, l_tags = lone_logs[s]
        i = cursor[s]
        assert tags[w, 1] == l_tags[i, 1], w
        assert rel[start[w]:start[w + 1]].tobytes() == l_rel[l_start[i]:l_start[i + 1]].tobytes(), w
        cursor[s] += 1
    # the reset: biwi_hotel's windows end at its pushes 19..25 and 64..75; the first group comes ahead of the reset, the
    # second is tagged with the push index counted from the reset on (and starts at least 20 pushes behind it)
    s1 = tags[tags[:, 0] == 1][:, 1].tolist()
    assert 26 <= n1 <= 64 - 19 and len(s1) > 7
    assert s1 == list(range(19, 26)) + list(range(64 - n1, 64 - n1 + len(s1) - 7))


# ---- 3. training on what was harvested --------------------------------------------------------------------------------------
def _epoch(model, ds, dev):
    from social_stgcnn_amd.dataset import EpochRunner
    from social_stgcnn_amd.trainer import Trainer
    runner = EpochRunner(Trainer(model, lr=0.01), ds, 16)
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(dev)
    return float(runner.train_epoch(order))


def test_an_epoch_on_the_snapshot_equals_one_on_the_host_built_dataset(dev, eth):
    from social_stgcnn_amd.dataset import DeviceWindows
    _, snap, win, _ = eth
    start = _model("eth", dev)
    a, b = copy.deepcopy(start), copy.deepcopy(start)
    loss_a, loss_b = _epoch(a, snap, dev), _epoch(b, DeviceWindows(win, dev), dev)
    assert np.isfinite(loss_a) and loss_a == loss_b
    changed = False
    for (k, x), (_, y), (_, z) in zip(a.state_dict().items(), b.state_dict().items(), start.state_dict().items()):
        assert torch.equal(x, y), k
        changed = changed or not torch.equal(x, z)
    assert changed


def test_fine_tune_is_reproducible(dev, eth):
    from social_stgcnn_amd.train import fine_tune
    _, snap, _, _ = eth
    start = _model("eth", dev)
    runs = []
    for _ in range(2):
        m = copy.deepcopy(start)
        runs.append(fine_tune(m, snap, 2, batch_size=16, lr=0.01, generator=torch.Generator(device=dev).manual_seed(1)))
    assert len(runs[0]) == 2 and all(np.isfinite(x) for x in runs[0]) and runs[0] == runs[1]
    assert fine_tune(copy.deepcopy(start), snap, 0) == []


# ---- 4. the command ---------------------------------------------------------------------------------------------------------
def test_predict_frames_harvest_round_trip(dev, tmp_path, eth):
    import pickle
    import argparse
    from social_stgcnn_amd import predict_frames as pf
    from live_inputs import CFG
    ck = tmp_path / "ck"
    ck.mkdir()
    model = _model("eth", dev)
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, ck / "val_best.pth")
    with open(ck / "args.pkl", "wb") as fh:
        pickle.dump(argparse.Namespace(n_stgcnn=CFG["n_stgcnn"], n_txpcnn=CFG["n_txpcnn"], output_size=CFG["output_feat"],
                                       obs_seq_len=CFG["seq_len"], kernel_size=CFG["kernel_size"],
                                       pred_seq_len=CFG["pred_seq_len"]), fh)
    rec = os.path.join(DATA, "eth_test", "biwi_eth.txt")
    out, kept = str(tmp_path / "p.npz"), str(tmp_path / "w.npz")
    pf.main(["--checkpoint", str(ck), "--recording", rec, "--ksteps", "2", "--harvest", "100", "--harvest_out", kept,
             "--out", out])
    win = eth[2]
    w = np.load(kept)
    assert w["seq_rel"].tobytes() == win.seq_rel.astype(np.float32).tobytes()
    assert np.array_equal(w["num_peds"], win.num_peds) and w["tags"].shape == (70, 2) and int(w["dropped_full"]) == 0
    p = np.load(out)
    assert len(p["frame"]) == len(p["num_peds"]) > 0 and p["samples"].shape[0] == 2
