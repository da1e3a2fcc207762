"""GPU (-m gpu): timestamped pushes (frames.TimeRule, stg_track_push_timed / stg_track_push_streams_timed of
csrc/frames_time.hip) against the numpy statement tests/frames_time_np.py, bit for bit: a feed of one push per step
against stg_track_push_rule; an irregular feed through every branch of the kernel (a ring that wraps, brackets wider than
max_dt, TOO_MANY, OVERFLOW, a repeated id, TRUNCATED); a push whose time does not increase; biwi_eth upsampled four
times through FramePredictor, eager and as ONE captured graph; StreamsPredictor against lone FramePredictors; risk
counts, reset(), capture and the command end to end."""
import argparse

import numpy as np
import pytest
import torch

from frames_time_np import DUPLICATE, OVERFLOW, TIME_ORDER, TOO_MANY, TRUNCATED, StreamModelTimed
from live_inputs import _assert_scene, _CPush, _model, _pushes, _rows, _sparse_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    return _model("eth", dev)


# ---- 1. one push per step: the rule kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("decimals", [4, None])
@pytest.mark.parametrize("rule", [(8, 0), (2, 2), (3, 6)])
def test_a_regular_feed_equals_the_rule_kernel(dev, rule, decimals):
    """t = 10 f, max_dt = step, R = T_obs: every instant is a push's time, nothing is interpolated, and the ring holds
    just the window.  V = 16 cuts the scenes of the loose rules (TOO_MANY on both sides)."""
    pushes = _pushes(_sparse_rows())
    assert len(pushes) == 40
    timed = _CPush(dev, rule, 16, 64, 32, decimals=decimals, time=(10, 10, 8))
    ruled = _CPush(dev, rule, 16, 64, 32, decimals=decimals)
    ref = StreamModelTimed(8, 10, 10, 8, rule[0], rule[1], 16, decimals, capacity=64, max_detections=32)
    members, flagged = 0, 0
    for f, (ids, xy) in enumerate(pushes):
        got, want = timed.push(ids, xy, 10 * f), ruled.push(ids, xy)
        for a, b, name in zip(got, want, ("ids", "num_peds", "obs_abs", "seen", "flags")):
            assert np.array_equal(a, b), (f, name)
        s_ids, s_obs, s_seen, s_flags = ref.push(ids, xy, 10 * f)
        _assert_scene(got[0], got[1], got[2], s_ids, s_obs, f, got[3], s_seen)
        assert got[4] == s_flags, f
        members += got[1]
        flagged += got[4] == TOO_MANY
    assert members > (20 if rule == (8, 0) else 400) and (flagged > 10 or rule == (8, 0))


# ---- 2. an irregular feed --------------------------------------------------------------------------------------------
def _irregular_feed(seed, n_push=120, n_ids=12, dup=False):
    """[(t, ids, xy)]: inter-push times drawn from {1, 2, 3, 4, 7, 13} ticks; n_ids ids that come and go, present for
    30-150 ticks and absent for 5-120; positions along a line plus noise, with more decimals than the rounding keeps;
    the detections of a push in a shuffled order.  dup: every fifth push repeats its first id with another position."""
    gen = np.random.default_rng(seed)
    times = np.cumsum(gen.choice([1, 2, 3, 4, 7, 13], size=n_push)) - 40
    spans = []
    for _ in range(n_ids):
        t, mine = int(times[0]) - int(gen.integers(0, 100)), []
        while t < times[-1]:
            on = int(gen.integers(30, 151))
            mine.append((t, t + on))
            t += on + int(gen.integers(5, 121))
        spans.append(mine)
    p0, vel = gen.uniform(-20, 20, size=(n_ids, 2)), gen.uniform(-0.05, 0.05, size=(n_ids, 2))
    feed = []
    for n, t in enumerate(times.tolist()):
        ids = [i for i in range(n_ids) if any(a <= t < b for a, b in spans[i])]
        gen.shuffle(ids)
        xy = np.array([p0[i] + vel[i] * t for i in ids]).reshape(-1, 2) + gen.normal(0, 0.01, size=(len(ids), 2))
        ids = [3 * i + 11 for i in ids]
        if dup and n % 5 == 0 and ids:
            ids, xy = ids + ids[:1], np.concatenate([xy, xy[:1] + 1.0])
        feed.append((t, np.array(ids, np.int64), xy))
    return feed


IRREGULAR = {
    "ring wraps": dict(r=4),
    "long ring": dict(r=64),
    "max_dt 3": dict(r=64, max_dt=3),
    "max_dt 70, unrounded": dict(r=64, max_dt=70, decimals=None),
    "T_obs 3": dict(t_obs=3, r=64, rule=(2, 1)),
    "T_obs 3, ring wraps, max_dt 3": dict(t_obs=3, r=4, max_dt=3, rule=(2, 1), decimals=None),
    "strict": dict(r=64, max_dt=13, rule=(8, 0)),
    "TOO_MANY": dict(r=64, v=5, want=TOO_MANY),
    "OVERFLOW": dict(r=64, s=8, want=OVERFLOW),
    "DUPLICATE": dict(r=16, dup=True, want=DUPLICATE),
    "TRUNCATED": dict(r=16, m_max=8, want=TRUNCATED),
}


@pytest.mark.parametrize("case", sorted(IRREGULAR))
def test_an_irregular_feed_equals_the_statement(dev, case):
    kw = dict(t_obs=8, r=64, max_dt=10, rule=(2, 3), v=16, s=32, m_max=16, decimals=4, dup=False, want=0)
    kw.update(IRREGULAR[case])
    t_obs, rule = kw["t_obs"], kw["rule"]
    feed = _irregular_feed(sum(map(ord, case)), dup=kw["dup"])
    assert len(feed) == 120
    c = _CPush(dev, rule, kw["v"], kw["s"], kw["m_max"], t_obs, kw["decimals"], time=(10, kw["max_dt"], kw["r"]))
    ref = StreamModelTimed(t_obs, 10, kw["max_dt"], kw["r"], rule[0], rule[1], kw["v"], kw["decimals"], kw["s"],
                           kw["m_max"])
    full = (1 << t_obs) - 1
    members = partial = flags = off_grid = 0
    for n, (t, ids, xy) in enumerate(feed):
        # (more detections than M_max: the buffers hold them all, the count says so, the kernel reads the first M_max)
        got = c.push(ids, xy, t)
        s_ids, s_obs, s_seen, s_flags = ref.push(ids, xy, t)
        _assert_scene(got[0], got[1], got[2], s_ids, s_obs, (case, n), got[3], s_seen)
        assert got[4] == s_flags, (case, n, got[4], s_flags)
        members += len(s_ids)
        partial += int((s_seen != full).sum())
        flags |= s_flags
        for i in s_ids.tolist():                            # a member whose window holds an instant between samples
            have = {smp[0] for smp in ref.tracks[i]}
            off_grid += any(t - k * 10 not in have for k in range(t_obs))
    assert members > 150 and off_grid > 100, (case, members, off_grid)
    assert partial > 20 or rule == (8, 0), (case, partial)
    assert (flags & TIME_ORDER) == 0 and (kw["want"] == 0 or flags & kw["want"]), (case, flags)


# ---- 3. a push whose time does not increase --------------------------------------------------------------------------
def test_a_push_back_in_time_changes_nothing(dev, model):
    from social_stgcnn_amd import frames
    feed = _irregular_feed(5, n_push=30)
    c = _CPush(dev, (2, 3), 8, 16, 16, time=(10, 10, 8))
    for t, ids, xy in feed[:20]:
        last = c.push(ids, xy, t)
    assert last[1] > 0 and last[4] == 0
    before = [x.clone() for x in c.state]
    for t in (feed[19][0], feed[19][0] - 1, feed[0][0] - 1000):
        got = c.push(feed[20][1], feed[20][2], t)
        assert got[4] == TIME_ORDER and got[1] == 0 and np.all(got[0] == -1) and not got[2].any() and not got[3].any()
        for x, x0, name in zip(c.state[:-1], before, ("slot_id", "t_ring", "xy_ring", "slot_head", "clock")):
            assert torch.equal(x, x0), (t, name)
        assert int(c.head_flags[0]) == int(before[-1][0])          # (the flags word reports the refusal)
    # ... and the stream goes on as if those pushes had not been made
    twin = _CPush(dev, (2, 3), 8, 16, 16, time=(10, 10, 8))
    for t, ids, xy in feed[:20]:
        twin.push(ids, xy, t)
    for t, ids, xy in feed[20:]:
        for a, b in zip(c.push(ids, xy, t), twin.push(ids, xy, t)):
            assert np.array_equal(a, b), t
    # one stream of a tick: its neighbours are pushed as usual
    kw = dict(k=2, capacity=16, max_peds=8, max_detections=16, tracks=(2, 3), time=frames.TimeRule(10, 10, 8))
    sp = frames.StreamsPredictor(model, 3, **kw)
    lone = [frames.FramePredictor(model, **kw) for _ in range(3)]
    for t, ids, xy in feed[:20]:
        sp.push([(ids, xy)] * 3, times=[t, t + 5, t - 7])
        for s, dt in enumerate((0, 5, -7)):
            lone[s].push(ids, xy, t=t + dt)
    state0 = [x.clone() for x in sp._state]
    t, ids, xy = feed[20]
    out = sp.push([(ids, xy)] * 3, times={0: t, 1: feed[19][0] + 5, 2: t - 7})
    assert out.flags.tolist() == [0, TIME_ORDER, 0] and out.pushed.tolist() == [True] * 3
    assert int(out.num_peds[1]) == 0 and bool((out.ids[1] == -1).all()) and not out.obs_abs[1].any()
    assert not sp.seen[1].any()
    for x, x0, name in zip(sp._state[:-1], state0, ("slot_id", "t_ring", "xy_ring", "slot_head", "clock")):
        assert torch.equal(x[1], x0[1]), name
    assert int(sp.clock[0, 0]) == t and int(sp.clock[2, 0]) == t - 7 and sp.clock[:, 1].tolist() == [21, 20, 21]
    for s, dt in ((0, 0), (2, -7)):
        r = lone[s].push(ids, xy, t=t + dt)
        assert int(r.num_peds) > 0 and torch.equal(out.ids[s], r.ids) and torch.equal(out.obs_abs[s:s + 1], r.obs_abs)
        assert torch.equal(sp.seen[s], lone[s].seen) and torch.equal(out.v_pred[s], r.v_pred)


# ---- 4. a recording upsampled four times -----------------------------------------------------------------------------
def _upsampled_eth(n_frames=60, sub=4):
    """biwi_eth's first n_frames frames with the times doubled (a step is 20 ticks) and every track interpolated
    linearly at `sub` instants per step: rows (time, id, x, y) for the n_frames * sub instants from the first frame
    on, and the original pushes.  An id is at an in-between instant iff it is in both frames around it."""
    rows = _rows("eth_test", "biwi_eth.txt")
    fnum = np.unique(rows[:, 0])[:n_frames + 1]
    assert np.all(np.diff(fnum) == 10)
    rows = rows[rows[:, 0] <= fnum[-1]]
    pushes = _pushes(rows)
    out = []
    for f in range(n_frames):
        here = dict(zip(pushes[f][0].tolist(), pushes[f][1]))
        nxt = dict(zip(pushes[f + 1][0].tolist(), pushes[f + 1][1]))
        t0 = int(fnum[f]) * 2
        out += [(t0, i, p[0], p[1]) for i, p in here.items()]
        for j in range(1, sub):
            out += [(t0 + j * (20 // sub), i, *(p + (nxt[i] - p) * (j / sub))) for i, p in here.items() if i in nxt]
    return np.array(out, dtype=np.float64), pushes[:n_frames]


@pytest.fixture(scope="module")
def upsampled():
    return _upsampled_eth()


def test_an_upsampled_recording_through_the_frame_predictor(dev, model, upsampled):
    """At the original frames the window's instants are original frames, each an exact sample: the scene and the
    prediction are those of the untimed FramePredictor fed the original pushes.  In between, every instant lies between
    two samples 5 ticks apart: the statement.  One captured graph serves all 240 pushes."""
    from social_stgcnn_amd import frames
    rows, originals = upsampled
    fine = _pushes(rows)
    ticks = np.unique(rows[:, 0]).astype(np.int64)
    assert len(fine) == 240 and np.all(np.diff(ticks) == 5)
    rule = frames.TimeRule(20, max_dt=20, history=48)
    kw = dict(k=2, capacity=64, max_peds=16, max_detections=32)
    plain = frames.FramePredictor(model, **kw)
    eager = frames.FramePredictor(model, time=rule, **kw)
    cap = frames.FramePredictor(model, time=rule, **kw)
    replay = cap.capture()
    ref = StreamModelTimed(8, 20, 20, 48, max_peds=16, capacity=64, max_detections=32)
    on_grid = between = 0
    static = set()
    for n, ((ids, xy), t) in enumerate(zip(fine, ticks.tolist())):
        e = eager.push(ids, xy, t=t, seed=n)
        c = replay(ids, xy, t=t, seed=n)
        static.add((c.obs_abs.data_ptr(), cap.seen.data_ptr()))
        for a, b, name in zip(e, c, e._fields):
            assert torch.equal(a, b), (n, name)
        assert torch.equal(eager.seen, cap.seen) and int(e.flags) == 0, n
        s_ids, s_obs, s_seen, s_flags = ref.push(ids, xy, t)
        _assert_scene(e.ids.cpu().numpy(), e.num_peds.item(), e.obs_abs[0].cpu().numpy(), s_ids, s_obs, n,
                      eager.seen.cpu().numpy(), s_seen)
        assert s_flags == 0 and np.all(s_seen == 255)
        if n % 4 == 0:
            o = plain.push(*originals[n // 4], seed=n)
            assert torch.equal(e.ids, o.ids) and torch.equal(e.num_peds, o.num_peds), n
            assert torch.equal(e.obs_abs, o.obs_abs) and torch.equal(e.v_pred, o.v_pred), n
            assert torch.equal(e.mean, o.mean) and torch.equal(e.samples, o.samples), n
            on_grid += int(o.num_peds)
        else:
            between += len(s_ids)
    assert on_grid > 100 and between > 300 and len(static) == 1


# ---- 5. streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [64, 1024])
def test_streams_with_their_own_clocks_equal_lone_frame_predictors(dev, model, block):
    """Five streams, each its own feed, clock and rate; stream s sits out the ticks n % 6 == s, stream 4 also every odd
    tick.  `times` as a mapping with host ticks, as a device tensor with a DeviceTick."""
    from social_stgcnn_amd import frames
    ns, n_ticks = 5, 60
    feeds = [_irregular_feed(200 + s, n_push=n_ticks, n_ids=8) for s in range(ns)]
    feeds[3] = [(1000 * t + 123456789012, i, p) for t, i, p in feeds[3]]            # microseconds, say
    rules = [frames.TimeRule(10, 10, 16)] * 3 + [frames.TimeRule(10000, 10000, 16)]
    kw = dict(k=2, capacity=16, max_peds=8, max_detections=8, tracks=(2, 3))
    for rule, members in ((rules[0], (0, 1, 2, 4)), (rules[3], (3,))):
        host = frames.StreamsPredictor(model, ns, block_threads=block, time=rule, **kw)
        devp = frames.StreamsPredictor(model, ns, block_threads=block, time=rule, **kw)
        replay = devp.capture()
        lone = {s: frames.FramePredictor(model, time=rule, **kw) for s in members}
        cursor = {s: 0 for s in members}
        scenes = 0
        for n in range(n_ticks):
            go = [s for s in members if n % 6 != s and not (s == 4 and n % 2)]
            tick = {s: feeds[s][cursor[s]] for s in go}
            state0 = [x.clone() for x in host._state]
            e = host.push({s: (i, p) for s, (t, i, p) in tick.items()}, times={s: t for s, (t, i, p) in tick.items()},
                          seed=n)
            counts = torch.tensor([len(tick[s][1]) if s in tick else -1 for s in range(ns)], dtype=torch.int32)
            ids = np.concatenate([tick[s][1] for s in go] + [np.zeros(0, np.int64)])
            xy = np.concatenate([tick[s][2] for s in go] + [np.zeros((0, 2))])
            times = torch.tensor([tick[s][0] if s in tick else -5 for s in range(ns)], dtype=torch.int64)
            c = replay(frames.DeviceTick(torch.from_numpy(ids).to(dev), torch.from_numpy(xy).to(dev), counts.to(dev)),
                       times=times.to(dev), seed=n)
            for a, b, name in zip(e, c, e._fields):
                assert torch.equal(a, b), (n, name)
            assert torch.equal(host.seen, devp.seen), n
            for s in range(ns):
                if s not in tick:
                    assert int(e.num_peds[s]) == 0 and not e.pushed[s] and int(e.flags[s]) == 0, (n, s)
                    for x, x0 in zip(host._state, state0):
                        assert torch.equal(x[s], x0[s]), (n, s)
                    continue
                t, i, p = tick[s]
                r = lone[s].push(i, p, t=t)
                cursor[s] += 1
                assert torch.equal(e.ids[s], r.ids) and torch.equal(e.num_peds[s:s + 1], r.num_peds), (n, s)
                assert torch.equal(e.obs_abs[s:s + 1], r.obs_abs) and torch.equal(e.flags[s:s + 1], r.flags), (n, s)
                assert torch.equal(host.seen[s], lone[s].seen) and torch.equal(e.v_pred[s], r.v_pred), (n, s)
                scenes += int(r.num_peds)
        assert scenes > 40 * len(members), scenes
        for x, x1 in zip(host._state, devp._state):
            assert torch.equal(x, x1)


# ---- 6. the other combinations ---------------------------------------------------------------------------------------
def test_risk_reset_and_capture_with_time(dev, model, upsampled):
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import RiskSpec
    rows, _ = upsampled
    fine, ticks = _pushes(rows)[:60], np.unique(rows[:, 0]).astype(np.int64).tolist()
    rule = frames.TimeRule(20, history=48)
    kw = dict(k=3, capacity=64, max_peds=16, max_detections=32, time=rule)
    a = frames.FramePredictor(model, risk=RiskSpec(0.5), keep_samples=False, tracks=(2, 2), **kw)
    b = frames.FramePredictor(model, risk=RiskSpec(0.5), keep_samples=False, tracks=(2, 2), **kw)
    assert a.time == (20, 20, 48) and a.rule == (2, 2) and frames.FramePredictor(model, **kw).rule == (8, 0)
    with pytest.raises(ValueError, match="needs the push's time"):
        a.push(*fine[0])
    with pytest.raises(ValueError, match="made with time="):
        frames.FramePredictor(model, k=2).push(*fine[0], t=5)
    # push, capture, push == push, push: the warm-up leaves the tracks and the clock as they were
    for n in range(30):
        ra, rb = a.push(*fine[n], t=ticks[n], seed=n), b.push(*fine[n], t=ticks[n], seed=n)
    clock = a.clock.clone()
    assert clock.tolist() == [ticks[29], 30]
    replay = a.capture()
    assert torch.equal(a.clock, clock)
    for x, y in zip(a._state, b._state):
        assert torch.equal(x, y)
    for n in range(30, 60):
        ra, rb = replay(*fine[n], t=ticks[n], seed=n), b.push(*fine[n], t=ticks[n], seed=n)
        for x, y, name in zip(ra, rb, ra._fields):
            assert torch.equal(x, y), (n, name)
        assert torch.equal(a.seen, b.seen)
        for x, y in zip(a.risk[1:], b.risk[1:]):
            assert (x is None and y is None) or torch.equal(x, y), n
    v = 16
    assert int(ra.num_peds) > 2 and ra.samples.shape[0] == 0
    assert a.risk.conflict.shape == (1, 12, v) and a.risk.conflict_any.shape == (1, v) and int(a.risk.conflict.max()) <= 3
    # reset(): the tracks and the clock are forgotten; an earlier time is a first push again
    b.reset()
    assert b.clock.tolist() == [0, 0] and bool((b.slot_id == -1).all()) and not b.slot_head.any()
    fresh = frames.FramePredictor(model, risk=RiskSpec(0.5), keep_samples=False, tracks=(2, 2), **kw)
    for n in range(12):
        rb, rf = b.push(*fine[n], t=ticks[n], seed=n), fresh.push(*fine[n], t=ticks[n], seed=n)
        assert int(rb.flags) == 0
        for x, y, name in zip(rb, rf, rb._fields):
            assert torch.equal(x, y), (n, name)
    assert int(rb.num_peds) > 0


def test_the_command_on_an_upsampled_recording(dev, model, upsampled, tmp_path):
    from social_stgcnn_amd import frames, predict_frames
    from social_stgcnn_amd.trainer import Checkpoint
    rows, _ = upsampled
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[79]]
    rec = str(tmp_path / "fine.txt")
    np.savetxt(rec, rows, fmt=["%d", "%d", "%.17g", "%.17g"], delimiter="\t")
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    out = str(tmp_path / "timed.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", rec, "--ksteps", "3", "--seed", "3", "--step", "20",
                         "--history", "48", "--min_seen", "2", "--max_gap", "2", "--max_peds", "16", "--out", out])
    npz = np.load(out)
    fp = frames.FramePredictor(model, k=3, max_peds=16, tracks=(2, 2), time=frames.TimeRule(20, None, 48))
    _, fs, ids, xy = frames.sorted_rows(rows)
    keep = []
    for n, t in enumerate(np.unique(rows[:, 0]).astype(np.int64).tolist()):
        r = fp.push(ids[fs[n]:fs[n + 1]], xy[fs[n]:fs[n + 1]], t=t, seed=3 + n)
        if int(r.num_peds) >= 1:
            keep.append((t, r, fp.seen))
    v = max(int(r.num_peds) for _, r, _ in keep)
    assert len(keep) > 60 and 2 < v <= 16 and sorted(npz.files) == ["frame", "ids", "mean", "num_peds", "samples", "seen",
                                                                   "time"]
    assert npz["time"].dtype == np.int64 and npz["time"].tolist() == [t for t, _, _ in keep]
    assert np.array_equal(npz["frame"], npz["time"].astype(np.float64)) and npz["seen"].dtype == np.int32
    assert np.array_equal(npz["ids"], torch.stack([r.ids[:v] for _, r, _ in keep]).cpu().numpy())
    assert np.array_equal(npz["seen"], torch.stack([s[:v] for _, _, s in keep]).cpu().numpy())
    assert np.array_equal(npz["num_peds"], torch.cat([r.num_peds for _, r, _ in keep]).cpu().numpy())
    assert np.array_equal(npz["mean"], torch.stack([r.mean[:, :v] for _, r, _ in keep]).cpu().numpy())
    assert np.array_equal(npz["samples"], torch.stack([r.samples[:, :, :v] for _, r, _ in keep], 1).cpu().numpy())
    assert int((npz["seen"][npz["ids"] >= 0] != 255).sum()) > 20
    with pytest.raises(ValueError, match="--radius"):
        predict_frames.main(["--checkpoint", ck.dir, "--recording", rec, "--step", "20", "--radius", "0.5", "--out", out])
