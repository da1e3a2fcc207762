"""GPU (-m gpu): the timed window harvest (csrc/harvest_time.hip).

Both entry points through the C ABI, behind the real stg_track_push_streams_timed, against the statement (harvest_time_np)
fed the kernels' own decoded track state, bit for bit after every tick: three streams on their own clocks, a skipped
stream, a push back in time, gaps of 13 and 25 ticks, slots running out, a negative and a huge id, rings of 4 and 64, both
ways of filling the log; the streams entry point against lone calls; the predictors -- snapshot() against
data.load_windows, eager and captured, a feed started between two frames against the statement, capture() on a half-fed
predictor, reset, together with TimedScoreSpec, three streams against three lone predictors; training on a snapshot; the
predict_frames command.  tests/test_harvest_time_cpu.py holds what the feeds have to reach."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import harvest_time_np as HT
from frames_time_np import OVERFLOW, TIME_ORDER
from live_inputs import DATA, _model, _pushes, _rows

pytestmark = pytest.mark.gpu
S, NS, STEP = 16, HT.NS, 10


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- 1. through the C ABI -----------------------------------------------------------------------------------------------
class _Rig:
    """The timed track state of NS streams and the harvest's history, log and scratch; the log pre-filled with 7s, so a
    store past the fill point shows."""

    def __init__(self, dev, r, t_obs, t_all, max_dt, settle, cap_w, cap_r, NS=NS, S=S):
        z = lambda shape, dt: torch.zeros(shape, device=dev, dtype=dt)      # noqa: E731
        self.track = (torch.full((NS, S), -1, device=dev, dtype=torch.int64), z((NS, S, r), torch.int64),
                      z((NS, S, r, 2), torch.float64), z((NS, S, 2), torch.int32), z((NS, 2), torch.int64),
                      z((NS, 2), torch.int32))
        self.hist = (z((NS, S), torch.int32), z((NS, t_all, S, 2), torch.float64), z((NS, 2), torch.int32),
                     z((NS, 3), torch.int64))
        self.ns, self.s = NS, S
        self.work = z(NS * (S + 3), torch.int32)
        self.log = (torch.full((cap_r, 2, t_all), 7.0, device=dev), torch.full((cap_w + 1,), -7, device=dev, dtype=torch.int32),
                    torch.full((cap_w, 2), -7, device=dev, dtype=torch.int32), z(3, torch.int32))
        self.log[1][0] = 0
        self.r, self.t_obs, self.t_all, self.max_dt, self.settle, self.caps = r, t_obs, t_all, max_dt, settle, (cap_w, cap_r)

    def sizes(self):
        return (self.s, self.r, self.t_obs, self.t_all, 2, ctypes.c_double(1e4), STEP, self.max_dt, self.settle)


def _push_streams(rig, tick, dev, m_max=32):
    """stg_track_push_streams_timed on one tick -> (pushed, the per-stream flags)"""
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    NS, S = rig.ns, rig.s
    counts = [0 if d is None else len(d[0]) for d in tick]
    start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    pushed = torch.tensor([int(d is not None) for d in tick], dtype=torch.int32).to(dev)
    times = torch.tensor([0 if d is None else d[2] for d in tick], dtype=torch.int64).to(dev)
    ids = np.concatenate([d[0] for d in tick if d is not None] + [np.zeros(1, np.int64)])
    xy = np.concatenate([d[1] for d in tick if d is not None] + [np.zeros((1, 2))])
    det_id, det_xy = torch.from_numpy(ids).to(dev), torch.from_numpy(xy).to(dev)
    v, t_obs = 8, rig.t_obs
    obs = torch.empty((NS, t_obs, v, 2), device=dev, dtype=torch.float64)
    out_ids = torch.empty((NS, v), device=dev, dtype=torch.int64)
    peds, flags, seen = (torch.empty(n, device=dev, dtype=torch.int32) for n in (NS, NS, NS * v))
    check(lib().stg_track_push_streams_timed(ptr(det_id), 1, ptr(det_xy), 2, len(ids), ptr(start), ptr(pushed), ptr(times),
                                             NS, m_max, *map(ptr, rig.track), S, rig.r, t_obs, ctypes.c_double(1e4), v,
                                             STEP, rig.max_dt, t_obs, 0, ptr(obs), ptr(out_ids), ptr(peds), ptr(flags),
                                             ptr(seen), 0, stream_ptr()), "stg_track_push_streams_timed")
    return pushed, flags.cpu().numpy()


def _harvest_streams(rig, track, pushed):
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    check(lib().stg_window_harvest_streams_timed(*map(ptr, track), ptr(pushed), rig.ns, *rig.sizes(), *map(ptr, rig.hist),
                                                 ptr(rig.work), *map(ptr, rig.log), *rig.caps, stream_ptr()),
          "stg_window_harvest_streams_timed")


def _harvest_lone(rig, track, b):
    """the lone entry point on stream b's slices"""
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    check(lib().stg_window_harvest_timed(*(ptr(x[b]) for x in track), *rig.sizes(), b, *(ptr(x[b]) for x in rig.hist),
                                         *map(ptr, rig.log), *rig.caps, stream_ptr()), "stg_window_harvest_timed")


CASES = [(3, 5, 70, 4, 10, 0, (400, 4000)), (3, 5, 70, 64, 13, 12, (21, 4000)), (3, 5, 70, 64, 10, 9, (400, 50)),
         (3, 5, 70, 4, 13, 12, (400, 4000)), (8, 20, 150, 64, 10, 0, (400, 4000)), (8, 20, 150, 64, 13, 12, (400, 4000)),
         (8, 20, 150, 4, 10, 9, (400, 131)), (8, 20, 150, 64, 13, 0, (30, 4000)), (8, 20, 150, 64, 10, 9, (400, 131))]


@pytest.mark.parametrize("t_obs,t_all,pushes,r,max_dt,settle,caps", CASES)
def test_both_entry_points_equal_the_statement(dev, t_obs, t_all, pushes, r, max_dt, settle, caps):
    """The scripted ticks of three streams: the streams entry point, and lone calls per pushed stream in stream order on a
    second history and log, against the statement fed the kernels' own decoded track state.  After every tick the history
    in its canonical form, h_head, h_clock, and every tensor of the log -- the 7s behind the fill point included."""
    streams, lone = (_Rig(dev, r, t_obs, t_all, max_dt, settle, *caps) for _ in range(2))
    ref = HT.TimedHarvester(NS, t_all, STEP, max_dt, settle, *caps)
    ref.log.rel_all[:], ref.log.win_start[1:], ref.log.win_tag[:] = 7.0, -7, -7
    seen_flags = 0
    for n, tick in enumerate(HT.scripted_feed(t_obs, t_all, pushes, 5)):
        pushed, flags = _push_streams(streams, tick, dev)
        seen_flags |= int(np.bitwise_or.reduce(flags))
        _harvest_streams(streams, streams.track, pushed)
        for b in range(NS):
            if tick[b] is not None:
                _harvest_lone(lone, streams.track, b)
        host = [x.cpu().numpy() for x in streams.track]
        ref.tick({b: (HT.decode_tracks(*(x[b] for x in host[:4])), int(host[4][b, 0]), not flags[b] & TIME_ORDER)
                  for b in range(NS) if tick[b] is not None})
        for got, want in zip(streams.log, (ref.log.rel_all, ref.log.win_start, ref.log.win_tag, ref.log.header)):
            assert got.cpu().numpy().tobytes() == want.tobytes(), n
        word, ring, head, clock = (x.cpu().numpy() for x in streams.hist)
        for b, h in enumerate(ref.hist):
            assert head[b].tolist() == h.head and clock[b].tolist() == h.clock, (n, b)
            assert HT.same_runs(HT.canonical(host[0][b], word[b], ring[b], head[b], t_all), h.runs), (n, b)
        assert all(torch.equal(a, b) for a, b in zip(streams.log + streams.hist, lone.log + lone.hist)), n
    n_w, n_r, dropped = (int(x) for x in ref.log.header)
    assert seen_flags & OVERFLOW and seen_flags & TIME_ORDER and all(h.skipped >= 1 for h in ref.hist)
    if caps == (400, 4000):
        assert dropped == 0 and (n_w >= 8 or (r == 4 and settle > 0))
        assert r == 4 or (set(ref.log.tags[:, 0].tolist()) == {0, 1, 2} and all(h.interpolated > 0 for h in ref.hist))
    elif caps[1] == 4000:
        assert dropped > 0 and n_w == caps[0] and n_r < caps[1]    # full by windows
    elif r == 64:
        assert dropped > 0 and n_w < caps[0] and n_r <= caps[1]    # full by rows


def test_a_second_pass_over_the_slots(dev):
    """272 slots for the 256 threads of the workgroup, rings of 4: the pass over the slots runs twice, the second time
    ragged, with candidates in it whose rank goes on from the first pass's count and whose frames are searched and
    interpolated there.  harvest_time_np.wide_feed through the real push (M_max 272) and both entry points, against the
    statement fed the decoded device state, as above; the conditions (tests/test_harvest_time_cpu.py holds them without
    a GPU) on the statement, with the slots the device handed out."""
    t_obs, t_all, r, max_dt, caps = 3, 5, 4, 10, (16, 1024)
    streams, lone = (_Rig(dev, r, t_obs, t_all, max_dt, 0, *caps, NS=HT.WIDE_NS, S=HT.WIDE_S) for _ in range(2))
    ref = HT.TimedHarvester(HT.WIDE_NS, t_all, STEP, max_dt, 0, *caps)
    ref.log.rel_all[:], ref.log.win_start[1:], ref.log.win_tag[:] = 7.0, -7, -7
    facts = []
    for n, tick in enumerate(HT.wide_feed()):
        pushed, flags = _push_streams(streams, tick, dev, m_max=HT.WIDE_S)
        assert not np.bitwise_or.reduce(flags) & (OVERFLOW | TIME_ORDER), n
        _harvest_streams(streams, streams.track, pushed)
        for b in range(HT.WIDE_NS):
            if tick[b] is not None:
                _harvest_lone(lone, streams.track, b)
        host = [x.cpu().numpy() for x in streams.track]
        before = int((ref.log.tags[:, 0] == 0).sum())
        ref.tick({b: (HT.decode_tracks(*(x[b] for x in host[:4])), int(host[4][b, 0]), True)
                  for b in range(HT.WIDE_NS) if tick[b] is not None})
        for got, want in zip(streams.log, (ref.log.rel_all, ref.log.win_start, ref.log.win_tag, ref.log.header)):
            assert got.cpu().numpy().tobytes() == want.tobytes(), n
        word, ring, head, clock = (x.cpu().numpy() for x in streams.hist)
        for b, h in enumerate(ref.hist):
            assert head[b].tolist() == h.head and clock[b].tolist() == h.clock, (n, b)
            assert HT.same_runs(HT.canonical(host[0][b], word[b], ring[b], head[b], t_all), h.runs), (n, b)
        assert all(torch.equal(a, b) for a, b in zip(streams.log + streams.hist, lone.log + lone.hist)), n
        slot_of = {int(k): s for s, k in enumerate(host[0][0]) if host[3][0, s, 1] > 0}
        facts.append(HT.wide_facts(ref.hist[0], slot_of, t_all, int((ref.log.tags[:, 0] == 0).sum()) > before))
    assert HT.wide_reached(ref, facts) and int(ref.log.header[0]) == 6


def test_every_refusal_launches_nothing(dev):
    """A refused call leaves the history, the log and the scratch as they were (pointers to real memory this time)."""
    from social_stgcnn_amd._lib import lib, ptr
    rig = _Rig(dev, 8, 3, 5, 10, 9, 8, 64)
    for x in rig.hist + (rig.work,):
        x.fill_(3)
    rig.log[3].copy_(torch.tensor([2, 5, 0]))
    kept = rig.hist + rig.log + (rig.work,)
    before = [x.clone() for x in kept]
    pushed = torch.ones(NS, device=dev, dtype=torch.int32)
    L = lib()

    def many(ns=NS, s=S, r=8, t_obs=3, t_all=5, min_peds=2, step=10, max_dt=10, settle=9, cap_w=8, cap_r=64, pushed=pushed,
             work=rig.work):
        return L.stg_window_harvest_streams_timed(*map(ptr, rig.track), ptr(pushed), ns, s, r, t_obs, t_all, min_peds, 1e4,
                                                  step, max_dt, settle, *map(ptr, rig.hist), ptr(work), *map(ptr, rig.log),
                                                  cap_w, cap_r, None)

    def one(s=S, r=8, t_obs=3, t_all=5, min_peds=2, step=10, max_dt=10, settle=9, tag=0, cap_w=8, cap_r=64):
        return L.stg_window_harvest_timed(*(ptr(x[0]) for x in rig.track), s, r, t_obs, t_all, min_peds, 1e4, step, max_dt,
                                          settle, tag, *(ptr(x[0]) for x in rig.hist), *map(ptr, rig.log), cap_w, cap_r,
                                          None)
    shared = (dict(s=0), dict(s=2049), dict(t_obs=0), dict(t_all=33), dict(t_obs=5), dict(min_peds=0), dict(cap_w=0),
              dict(cap_r=0), dict(r=1), dict(step=0), dict(max_dt=0, settle=0), dict(max_dt=21), dict(settle=-1),
              dict(settle=10))
    for kw in shared + (dict(ns=0), dict(ns=4097), dict(pushed=None), dict(work=None)):
        assert many(**kw) == -1, kw
        assert L.stg_last_error().startswith(b"stg_window_harvest_streams_timed:"), kw
    for kw in shared + (dict(tag=-1), dict(t_all=3)):
        assert one(**kw) == -1, kw
        assert L.stg_last_error().startswith(b"stg_window_harvest_timed:"), kw
    for kw in (dict(r=257), dict(step=1 << 30)):
        assert many(**kw) == -2 and one(**kw) == -2, kw
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, before))


# ---- 2. the predictors ----------------------------------------------------------------------------------------------------
KW = dict(k=2, max_peds=16, max_detections=32, capacity=64)


def _first60(d, f, tmp):
    """the recording's first 60 frames, as rows and as a file of their own"""
    rows = _rows(d, f)
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[59]]
    path = os.path.join(str(tmp), "first60.txt")
    with open(path, "w") as fh:
        for r in rows:
            fh.write("%s\t%s\t%s\t%s\n" % tuple(repr(float(x)) for x in r[:4]))
    return rows, path


def _rule(history=96):
    from social_stgcnn_amd import frames
    return frames.TimeRule(4, 4, history)


@pytest.fixture(scope="module")
def eth(dev, tmp_path_factory):
    """biwi_eth's first 60 frames upsampled 4x, one push per tick, step = max_dt = 4, settle = 0: pushed through a captured
    harvesting predictor and, eagerly, through one without, and eagerly through a second harvesting one."""
    from social_stgcnn_amd import data, frames
    tmp = tmp_path_factory.mktemp("eth60")
    rows, path = _first60("eth_test", "biwi_eth.txt", tmp)
    win = data.load_windows(str(tmp), files=["first60.txt"], with_non_linear=False)
    model = _model("eth", dev)
    pushes, times = HT.eth_feed(_pushes(rows), 0)
    fp, eager = (frames.FramePredictor(model, time=_rule(), harvest=frames.TimedHarvestSpec(64, settle=0), **KW)
                 for _ in range(2))
    plain = frames.FramePredictor(model, time=_rule(), **KW)
    replay = fp.capture()
    same = True
    for n, ((ids, xy), t) in enumerate(zip(pushes, times)):
        a, b = replay(ids, xy, t=t, seed=n), plain.push(ids, xy, t=t, seed=n)
        same = same and all(torch.equal(x, y) for x, y in zip(a, b))
        eager.push(ids, xy, t=t, seed=n)
    return fp, eager, win, same


def _assert_snapshot(snap, win, what):
    assert np.array_equal(snap.num_peds_host, win.num_peds), what
    assert snap.rel_all.cpu().numpy().tobytes() == win.seq_rel.astype(np.float32).tobytes(), what
    assert np.array_equal(snap.win_start.cpu().numpy(), np.concatenate([[0], np.cumsum(win.num_peds)])), what


def test_snapshot_on_the_grid_equals_load_windows(eth):
    """Eager and captured (one graph): the windows of data.load_windows over those 60 frames, bit for bit, tagged with the
    frame indices; the predictions are those of a predictor without the spec."""
    fp, eager, win, same = eth
    assert len(win) == 2
    for p in (fp, eager):
        assert p.harvest.counts() == (2, 4, 0)
        _assert_snapshot(p.harvest.snapshot(), win, p is fp)
        assert p.harvest.tags().tolist() == [[0, 24], [0, 46]]
        assert p.harvest_clock.cpu().tolist() == [[1, 0, 0]] and p.h_head.cpu().tolist()[1] == 60
    assert same, "the predictions of a harvesting predictor equal those of one without"


def _assert_log(log, ref, what):
    n_w, n_r, dropped = (int(x) for x in ref.log.header)
    assert log.counts() == (n_w, n_r, dropped), what
    assert log.rel_all[:n_r].cpu().numpy().tobytes() == ref.log.seq_rel.tobytes(), what
    assert np.array_equal(log.win_start[:n_w + 1].cpu().numpy(), ref.log.win_start[:n_w + 1]), what
    assert np.array_equal(log.tags(), ref.log.tags), what


@pytest.mark.parametrize("rec,settle,min_peds", [(("eth_test", "biwi_eth.txt"), None, 1),
                                                 (("zara1_test", "crowds_zara01.txt"), 0, 2),
                                                 (("zara1_test", "crowds_zara01.txt"), None, 2)])
def test_a_feed_started_between_two_frames_equals_the_statement(dev, rec, settle, min_peds):
    """The upsampled feed started two pushes in, the pushes on the grid left out, one skip, one emptied push: every frame
    of every window is interpolated on the device.  Captured, against the statement; with TimedScoreSpec beside it; capture()
    on the half-fed predictor leaves history, clock and log as they were; reset() zeroes the history and leaves the log."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    pushes, times = HT.eth_feed(_pushes(_rows(*rec))[:60], 2)
    ref, _ = HT.feed(pushes, times, step=4, max_dt=4, settle=3 if settle is None else settle, min_peds=min_peds, capacity=64)
    assert ref.hist[0].interpolated > 0 and ref.hist[0].clock[:2] == [1, 2] and ref.hist[0].skipped >= 1 and int(ref.log.header[0]) >= 3
    fp = frames.FramePredictor(_model("eth", dev), time=_rule(), score=TimedScoreSpec(pending=64),
                               harvest=frames.TimedHarvestSpec(64, min_peds=min_peds, settle=settle), **KW)
    half = len(pushes) // 2
    for (ids, xy), t in zip(pushes[:half], times[:half]):
        fp.push(ids, xy, t=t)
    log = fp.harvest
    kept = (fp.h_word, fp.h_ring, fp.h_head, fp.h_clock, log.rel_all, log.win_start, log.win_tag, log.header, fp.clock)
    before = [x.clone() for x in kept]
    replay = fp.capture()
    assert all(torch.equal(a, b) for a, b in zip(kept, before)) and fp.harvest.counts()[0] > 0
    for (ids, xy), t in zip(pushes[half:], times[half:]):
        replay(ids, xy, t=t)
    _assert_log(log, ref, "captured from the middle on")
    assert fp.harvest_clock.cpu().tolist() == [ref.hist[0].clock] and fp.h_head.cpu().tolist() == ref.hist[0].head
    assert float(fp.score_totals[0][..., 0].sum()) > 0
    fp.reset()
    assert not fp.h_word.any() and not fp.h_head.any() and not fp.h_clock.any()
    assert log.counts() == tuple(int(x) for x in ref.log.header)


def test_three_streams_against_three_lone_predictors(dev):
    """Three recordings at four pushes per step, each stream on its own clock and started on its own tick; times given as
    a mapping, then as a device tensor with a DeviceTick; stream 1 reset halfway.  The one log holds, tick by tick and
    stream by stream, the windows of three lone predictors fed the same pushes."""
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    feeds = [HT.eth_feed(_pushes(_rows(d, f))[a:a + 50], 2, 30, 35) for d, f, a in (("eth_test", "biwi_eth.txt", 150),
                                                                           ("hotel_test", "biwi_hotel.txt", 40),
                                                                           ("zara1_test", "crowds_zara01.txt", 0))]
    clock0, starts = (0, 5000, -300), (0, 7, 3)
    spec = frames.TimedHarvestSpec(256)
    sp = frames.StreamsPredictor(model, 3, time=_rule(), harvest=spec, **KW)
    lone = [frames.FramePredictor(model, time=_rule(), harvest=spec, **KW) for _ in range(3)]
    replay = sp.capture()
    order = []
    n_ticks = max(len(p) + s for (p, _), s in zip(feeds, starts))
    for n in range(n_ticks):
        if n == 40:
            sp.reset(streams=[1])
            lone[1].reset()
        tick, when = {}, {}
        for s, ((pushes, times), s0) in enumerate(zip(feeds, starts)):
            if s0 <= n < s0 + len(pushes) and not (s == 2 and n % 5 == 4):
                tick[s], when[s] = pushes[n - s0], clock0[s] + times[n - s0]
        before = [p.harvest.counts()[0] for p in lone]
        for s in tick:
            lone[s].push(*tick[s], t=when[s])
        order += [s for s in range(3) if lone[s].harvest.counts()[0] > before[s]]
        if n % 2:
            replay(tick, times=when)
        else:
            ids = [tick[s][0] for s in sorted(tick)] + [np.zeros(0, np.int64)]
            xy = [tick[s][1] for s in sorted(tick)] + [np.zeros((0, 2))]
            counts = [len(tick[s][0]) if s in tick else -1 for s in range(3)]
            t_dev = torch.tensor([when.get(s, 0) for s in range(3)], dtype=torch.int64).to(dev)
            replay(frames.DeviceTick(torch.from_numpy(np.concatenate(ids)).to(dev),
                                     torch.from_numpy(np.concatenate(xy)).to(dev), counts), times=t_dev)
    assert len(order) >= 8 and set(order) == {0, 1, 2}
    n_w, n_r, dropped = sp.harvest.counts()
    assert (n_w, dropped) == (len(order), 0)
    tags, start, rel = sp.harvest.tags(), sp.harvest.win_start.cpu().numpy(), sp.harvest.rel_all.cpu().numpy()
    assert tags[:, 0].tolist() == order
    cursor = [0, 0, 0]
    lone_logs = [(p.harvest.rel_all.cpu().numpy(), p.harvest.win_start.cpu().numpy(), p.harvest.tags()) for p in lone]
    for w, s in enumerate(order):
        l_rel, l_start, l_tags = lone_logs[s]
        i = cursor[s]
        assert tags[w, 1] == l_tags[i, 1], w
        assert rel[start[w]:start[w + 1]].tobytes() == l_rel[l_start[i]:l_start[i + 1]].tobytes(), w
        cursor[s] += 1
    clocks = sp.harvest_clock.cpu().numpy()
    assert clocks.shape == (3, 3)
    for s in range(3):
        assert clocks[s].tolist() == lone[s].harvest_clock.cpu().numpy()[0].tolist(), s
        assert torch.equal(sp.h_head[s], lone[s].h_head), s
    assert clocks[1, 1] > 5000 + 2 and clocks[0, 1] == 2 and clocks[2, 1] == -298        # stream 1 anchored again


# ---- 3. training on what was harvested --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zara(dev):
    """crowds_zara01's first 60 frames started between two frames, captured: (the predictor, the statement)."""
    from social_stgcnn_amd import frames
    pushes, times = HT.eth_feed(_pushes(_rows("zara1_test", "crowds_zara01.txt"))[:60], 2)
    ref, _ = HT.feed(pushes, times, step=4, max_dt=4, settle=3, capacity=64)
    fp = frames.FramePredictor(_model("zara1", dev), time=_rule(), harvest=frames.TimedHarvestSpec(64), **KW)
    replay = fp.capture()
    for (ids, xy), t in zip(pushes, times):
        replay(ids, xy, t=t)
    return fp, ref


def _epoch(model, ds, dev):
    from social_stgcnn_amd.dataset import EpochRunner
    from social_stgcnn_amd.trainer import Trainer
    runner = EpochRunner(Trainer(model, lr=0.01), ds, 16)
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(dev)
    return float(runner.train_epoch(order))


def test_an_epoch_on_the_timed_snapshot_equals_one_on_the_statements_windows(dev, zara):
    from social_stgcnn_amd.dataset import DeviceWindows
    from social_stgcnn_amd.train import fine_tune
    fp, ref = zara
    _assert_log(fp.harvest, ref, "zara01")
    snap = fp.harvest.snapshot()
    assert len(snap) == int(ref.log.header[0]) >= 16
    n_w, n_r = int(ref.log.header[0]), int(ref.log.header[1])
    built = DeviceWindows.from_device(torch.from_numpy(ref.log.seq_rel.copy()).to(dev),
                                      torch.from_numpy(ref.log.win_start[:n_w + 1].copy()).to(dev), ref.log.num_peds, 8)
    start = _model("zara1", dev)
    a, b = copy.deepcopy(start), copy.deepcopy(start)
    loss_a, loss_b = _epoch(a, snap, dev), _epoch(b, built, dev)
    assert np.isfinite(loss_a) and loss_a == loss_b
    changed = False
    for (k, x), (_, y), (_, z) in zip(a.state_dict().items(), b.state_dict().items(), start.state_dict().items()):
        assert torch.equal(x, y), k
        changed = changed or not torch.equal(x, z)
    assert changed
    losses = fine_tune(copy.deepcopy(start), snap, 1, batch_size=16, lr=0.01,
                       generator=torch.Generator(device=dev).manual_seed(1))
    assert len(losses) == 1 and np.isfinite(losses[0])


# ---- 4. the command ---------------------------------------------------------------------------------------------------------
def test_predict_frames_harvest_timed_round_trip(dev, tmp_path):
    """The upsampled frames written to a file whose frame column is the tick: the command's windows are the statement's."""
    import argparse
    import pickle
    from live_inputs import CFG
    from social_stgcnn_amd import predict_frames as pf
    ck = tmp_path / "ck"
    ck.mkdir()
    model = _model("zara1", dev)
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, ck / "val_best.pth")
    with open(ck / "args.pkl", "wb") as fh:
        pickle.dump(argparse.Namespace(n_stgcnn=CFG["n_stgcnn"], n_txpcnn=CFG["n_txpcnn"], output_size=CFG["output_feat"],
                                       obs_seq_len=CFG["seq_len"], kernel_size=CFG["kernel_size"],
                                       pred_seq_len=CFG["pred_seq_len"]), fh)
    pushes, times = HT.eth_feed(_pushes(_rows("zara1_test", "crowds_zara01.txt"))[:60], 2)
    full = [n for n, (i, _) in enumerate(pushes) if len(i)]     # (a file cannot hold an empty push)
    pushes, times = [pushes[n] for n in full], [times[n] for n in full]
    rec = tmp_path / "up.txt"
    with open(rec, "w") as fh:
        for (ids, xy), t in zip(pushes, times):
            for i, p in zip(ids, xy):
                fh.write("%s\t%s\t%s\t%s\n" % (repr(float(t)), repr(float(i)), repr(float(p[0])), repr(float(p[1]))))
    # the command pushes a frame's rows sorted by id, as the statement's feed here
    ref, _ = HT.feed([(np.sort(i), x[np.argsort(i, kind="stable")]) for i, x in pushes], times, step=4, max_dt=4, settle=1,
                     capacity=1024)
    out, kept = str(tmp_path / "p.npz"), str(tmp_path / "w.npz")
    pf.main(["--checkpoint", str(ck), "--recording", str(rec), "--ksteps", "2", "--step", "4", "--harvest_timed", "100",
             "--settle", "1", "--harvest_out", kept, "--max_peds", "16", "--out", out])
    w = np.load(kept)
    assert w["seq_rel"].tobytes() == ref.log.seq_rel.tobytes() and np.array_equal(w["num_peds"], ref.log.num_peds)
    assert np.array_equal(w["tags"], ref.log.tags) and len(w["tags"]) >= 8
    assert (int(w["g0"]), int(w["skipped"]), int(w["dropped_full"])) == (2, ref.hist[0].skipped, 0)
    p = np.load(out)
    assert len(p["time"]) == len(p["num_peds"]) > 0 and p["samples"].shape[0] == 2
