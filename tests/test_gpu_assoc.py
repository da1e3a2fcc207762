"""GPU (-m gpu): unlabelled detections -> track ids on the device (stg_associate, stg_associate_streams).

Through the C ABI against the numpy restatement (assoc_np.Tracker), ids, flags and the whole state bit for bit after
every push: ties, the chain that needs one round per pair, the counts around the wave and the limits, slots running
out, max_miss, the gate of a one-sample track, two recordings; the streams kernel against lone stg_associate calls; and
end to end, FramePredictor / StreamsPredictor with associate= against the same predictors fed the restatement's ids."""
import ctypes

import numpy as np
import pytest
import torch

import assoc_np
from live_inputs import Schedule, _model, _pushes, _rows

pytestmark = pytest.mark.gpu

ZARA1 = ("zara1_test", "crowds_zara01.txt")
UNIV3 = ("univ_test", "students003.txt")
HOTEL = ("hotel_test", "biwi_hotel.txt")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recs():
    """The pushes of the recordings the tests use, read once: [(recorded ids, xy)] per frame."""
    return {r: _pushes(_rows(*r)) for r in (ZARA1, UNIV3, HOTEL)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, ref, what):
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, i, np.argwhere(_bits(a) != _bits(b))[:4])


class DevState:
    """The association state of `lead` streams on the device, as the C ABI takes it."""

    def __init__(self, dev, c, lead=()):
        one = lead or (1,)
        self.t = (torch.full(lead + (c,), -1, device=dev, dtype=torch.int64),
                  torch.zeros(lead + (c, 2), device=dev, dtype=torch.float64),
                  torch.zeros(lead + (c, 2), device=dev, dtype=torch.float64),
                  torch.zeros(lead + (c,), device=dev, dtype=torch.int32),
                  torch.zeros(lead + (c,), device=dev, dtype=torch.int32),
                  torch.zeros(one, device=dev, dtype=torch.int64), torch.zeros(one, device=dev, dtype=torch.int32))

    def ptrs(self):
        return [ctypes.c_void_p(x.data_ptr()) for x in self.t]


UNTOUCHED = -7


class DevTracker:
    """One stream through stg_associate; the staging arrays hold `slack` detections past m_max."""

    def __init__(self, dev, c, m_max, gate, gate_new=None, max_miss=0, decimals=4, slack=4):
        from social_stgcnn_amd._lib import lib
        self.lib, self.dev, self.c, self.m_max = lib(), dev, c, m_max
        self.st = DevState(dev, c)
        self.det_id = torch.full((m_max + slack,), UNTOUCHED, device=dev, dtype=torch.int64)
        self.det_xy = torch.zeros((m_max + slack, 2), device=dev, dtype=torch.float64)
        self.count = torch.zeros(1, device=dev, dtype=torch.int32)
        gn = 2.0 * gate if gate_new is None else gate_new
        self.rule = (1e4 if decimals == 4 else 0.0, float(gate) * float(gate), float(gn) * float(gn), max_miss)

    def push(self, xy):
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        n = len(xy)
        self.det_id.fill_(UNTOUCHED)
        if n:
            self.det_xy[:n].copy_(torch.from_numpy(xy))
        self.count.fill_(n)
        p = lambda x: ctypes.c_void_p(x.data_ptr())        # noqa: E731
        rc = self.lib.stg_associate(p(self.det_id), p(self.det_xy), p(self.count), self.m_max, *self.st.ptrs(), self.c,
                                    *self.rule, None)
        assert rc == 0, self.lib.stg_last_error()
        ids = self.det_id.cpu().numpy()
        m = min(n, self.m_max)
        assert np.all(ids[m:] == UNTOUCHED)                 # past the count, and past M_max: not touched
        return ids[:m]

    def state(self):
        return [x.cpu().numpy() for x in self.st.t]


def _pair(dev, c, m_max, gate, gate_new=None, max_miss=0):
    return (DevTracker(dev, c, m_max, gate, gate_new, max_miss),
            assoc_np.Tracker(c, gate, gate_new, max_miss, m_max=m_max))


def _push_both(pair, xy, what):
    d, r = pair
    got, ref = d.push(xy), r.push(xy)
    assert np.array_equal(got, ref), (what, got[:12], ref[:12])
    _same(d.state(), r.state(), what)
    return got


def test_ties_are_resolved_by_slot_then_detection(dev):
    """Tracks and detections on an integer grid: many pairs share a cost, and the order (cost, s, j) decides."""
    gen = np.random.default_rng(3)
    pair = _pair(dev, 37, 40, gate=2.0, gate_new=3.0, max_miss=1)
    tied = 0
    for t in range(25):
        m = int(gen.integers(10, 41))
        xy = gen.integers(0, 7, size=(m, 2)).astype(np.float64)          # a 7 x 7 grid: repeated positions too
        ids = _push_both(pair, xy, t)
        assert len(set(ids.tolist())) == m
        tied += m - len(np.unique(xy, axis=0))
    assert tied > 40


def test_chain_needs_one_round_per_pair(dev):
    """t0 d0 t1 d1 ... t7 d7 on a line with strictly decreasing gaps: every detection but the last is nearer to the next
    track, so only (t7, d7) is mutually best at first and a round-based kernel needs 8 rounds.  The result is t_i - d_i."""
    gaps = np.arange(16, 0, -1) / 8.0
    x = np.concatenate([[0.0], np.cumsum(gaps)])[:16]
    line = lambda v: np.stack([v, np.zeros_like(v)], 1)                 # noqa: E731
    pair = _pair(dev, 11, 8, gate=100.0)
    assert _push_both(pair, line(x[0::2]), "births").tolist() == list(range(8))
    assert _push_both(pair, line(x[1::2]), "chain").tolist() == list(range(8))
    # and with the detections listed in reverse
    pair = _pair(dev, 11, 8, gate=100.0)
    _push_both(pair, line(x[0::2]), "births")
    assert _push_both(pair, line(x[1::2][::-1]), "chain reversed").tolist() == list(range(8))[::-1]


def _walk(gen, n):
    """n pedestrians spread over 60 x 60 and their per-push steps: most keep their identity under gate 1."""
    return gen.uniform(-30, 30, size=(n, 2)), gen.uniform(-0.3, 0.3, size=(n, 2))


def test_detection_counts_around_the_wave_and_the_limit(dev):
    """m = 0, 1, 63, 64, 65, M_max and M_max + 3 (the first M_max used, the others not touched) with C = 1100 slots: not
    a multiple of the 1024-thread workgroup, so the slot loops run a partial second pass."""
    gen = np.random.default_rng(5)
    m_max = 140
    pair = _pair(dev, 1100, m_max, gate=1.0, max_miss=1)
    pos, step = _walk(gen, m_max + 3)
    for t, m in enumerate((64, 0, 1, 63, 64, 65, m_max, m_max + 3, 65, m_max + 3, 0, m_max)):
        pos = pos + step
        ids = _push_both(pair, pos[:m], (t, m))
        assert len(ids) == min(m, m_max)
    assert int(pair[1].next_id) > m_max                      # births went on after the first full push


def test_slots_full(dev):
    gen = np.random.default_rng(7)
    pair = _pair(dev, 5, 16, gate=0.5)
    pos, step = _walk(gen, 9)
    ids = _push_both(pair, pos, 0)
    assert ids.tolist() == list(range(9))
    assert pair[0].state()[6].tolist() == [assoc_np.FULL] and pair[0].state()[5].tolist() == [9]
    ids = _push_both(pair, pos + 0.01, 1)                   # five remembered, four born again: distinct, next_id right
    assert ids.tolist() == [0, 1, 2, 3, 4, 9, 10, 11, 12]
    assert pair[0].state()[6].tolist() == [assoc_np.FULL] and pair[0].state()[5].tolist() == [13]
    _push_both(pair, pos[:3], 2)
    assert pair[0].state()[6].tolist() == [0]


def test_max_miss_keeps_an_id_over_gaps(dev):
    """max_miss = 2: missed twice, a track comes back with its id (the prediction runs on, the velocity is per push);
    missed three times it is forgotten and the detection gets a new id."""
    pair = _pair(dev, 6, 4, gate=0.5, gate_new=1.0, max_miss=2)
    here = lambda k: [[0.4 * k, 1.0], [20.0 - 0.3 * k, -5.0]]          # noqa: E731
    assert _push_both(pair, here(0), 0).tolist() == [0, 1]
    assert _push_both(pair, here(1), 1).tolist() == [0, 1]
    assert _push_both(pair, here(2)[1:], 2).tolist() == [1]
    assert _push_both(pair, here(3)[1:], 3).tolist() == [1]
    assert _push_both(pair, here(4), 4).tolist() == [0, 1]              # 0 back after two misses
    for k in (5, 6, 7):
        assert _push_both(pair, here(k)[1:], k).tolist() == [1]
    assert _push_both(pair, here(8), 8).tolist() == [2, 1]              # three misses: forgotten


def test_one_sample_track_uses_gate_new(dev):
    """gate 1, gate_new 2: a detection 1.5 from the prediction matches a track seen once and not a track seen twice."""
    pair = _pair(dev, 4, 4, gate=1.0, gate_new=2.0)
    assert _push_both(pair, [[0.0, 0.0]], 0).tolist() == [0]
    assert _push_both(pair, [[0.0, 0.0], [10.0, 0.0]], 1).tolist() == [0, 1]       # track 0: two samples; track 1: one
    assert pair[0].state()[4].tolist() == [2, 1, 0, 0]
    assert _push_both(pair, [[1.5, 0.0], [11.5, 0.0]], 2).tolist() == [2, 1]


@pytest.mark.parametrize("rec, n", [(ZARA1, 60), (UNIV3, 40)])
def test_recordings_push_by_push(dev, recs, rec, n):
    pushes = recs[rec][:n]
    m_max = max(len(i) for i, _ in pushes)
    assert rec != UNIV3 or m_max >= 30                       # (the recording reaches 52 later on)
    pair = _pair(dev, 300, m_max, gate=1.0, gate_new=2.0)
    for t, (_, xy) in enumerate(pushes):
        _push_both(pair, xy, (rec[1], t))


def test_streams_equal_lone_calls_and_keep_idle_state(dev, recs):
    """NS = 3 on a Schedule (stream 1 skips ticks, stream 2 starts late and has an empty push), packed (id, x, y)
    records at strides 3 / 3: every stream equals a lone stg_associate and the restatement fed its pushes; a stream not
    pushed keeps its state bit for bit and its id fields are not written."""
    from social_stgcnn_amd._lib import lib
    L = lib()
    ns, c, m_max, cap = 3, 333, 60, 200                     # 333 slots: a partial second pass of the 256 threads
    pushes = [[xy for _, xy in recs[r][:30]] for r in (UNIV3, ZARA1, HOTEL)]
    pushes[2] = pushes[2][:5] + [np.zeros((0, 2))] + pushes[2][5:]
    sched = Schedule(pushes, [0, 1, 4])
    st = DevState(dev, c, (ns,))
    lone = [DevTracker(dev, c, m_max, 1.0, 2.0, 1) for _ in range(ns)]
    refs = [assoc_np.Tracker(c, 1.0, 2.0, 1, m_max=m_max) for _ in range(ns)]
    rec = torch.zeros((cap, 3), device=dev, dtype=torch.float64)
    rec_i = rec.view(torch.int64)
    idle = empty = 0
    p = lambda x: ctypes.c_void_p(x.data_ptr())            # noqa: E731
    for t in range(34):
        tick = sched.tick(t)
        counts = [0 if d is None else len(d) for d in tick]
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        assert start[-1] <= cap
        host = np.zeros((cap, 3))
        host.view(np.int64)[:, 0] = UNTOUCHED
        for s, d in enumerate(tick):
            if d is not None and len(d):
                host[start[s]:start[s + 1], 1:] = d
        rec.copy_(torch.from_numpy(host))
        start_d = torch.from_numpy(start).to(dev)
        pushed_d = torch.tensor([int(d is not None) for d in tick], dtype=torch.int32).to(dev)
        before = [[x[s].clone() for x in st.t] for s in range(ns)]
        rc = L.stg_associate_streams(p(rec_i), 3, ctypes.c_void_p(rec.data_ptr() + 8), 3, cap, p(start_d), p(pushed_d),
                                     ns, m_max, *st.ptrs(), c, 1e4, 1.0, 4.0, 1, None)
        assert rc == 0, L.stg_last_error()
        ids = rec_i[:, 0].cpu().numpy()
        assert np.all(ids[start[-1]:] == UNTOUCHED), t
        for s, d in enumerate(tick):
            mine = [x[s].cpu().numpy().reshape(y.shape) for x, y in zip(st.t, refs[s].state())]
            if d is None:
                idle += 1
                _same(mine, [x.cpu().numpy().reshape(y.shape) for x, y in zip(before[s], mine)], (t, s, "idle"))
                continue
            empty += int(len(d) == 0)
            got = ids[start[s]:start[s + 1]]
            assert np.array_equal(got, lone[s].push(d)) and np.array_equal(got, refs[s].push(d)), (t, s)
            _same(mine, lone[s].state(), (t, s, "lone"))
            _same(mine, refs[s].state(), (t, s, "restatement"))
    assert idle > 8 and empty == 1


def _fp_fields(r):
    return (r.ids, r.num_peds, r.obs_abs, r.flags, r.samples, r.mean, r.v_pred)


def _np_ids(pushes, spec, cap=1024):
    trk = assoc_np.Tracker(cap, spec.gate, spec.gate_new, spec.max_miss)
    return [trk.push(xy) for _, xy in pushes]


@pytest.mark.parametrize("tracks, max_miss", [(None, 0), ((2, 2), 2)])
def test_frame_predictor_equals_one_fed_the_restatements_ids(dev, recs, tracks, max_miss):
    """30 pushes of crowds_zara01: FramePredictor(associate=...) fed (None, xy) equals a FramePredictor fed
    (assoc_np ids, xy) -- scene, num_peds, flags, and with explicit noise samples, mean and v_pred --, eager and as the
    captured replay; .det_ids are the restatement's ids.  Also under TrackRule(2, 2) with max_miss = 2."""
    from social_stgcnn_amd import frames
    pushes = recs[ZARA1][:30]
    spec = frames.AssociateSpec(1.0, 2.0, max_miss)
    ref_ids = _np_ids(pushes, spec)
    model = _model("eth", dev)
    k, v, p = 3, 32, 12
    kw = dict(k=k, max_peds=v, max_detections=64, tracks=None if tracks is None else frames.TrackRule(*tracks))
    a = frames.FramePredictor(model, associate=spec, **kw)
    c = frames.FramePredictor(model, associate=spec, **kw)
    b = frames.FramePredictor(model, **kw)
    replay = c.capture()
    _same([x.cpu().numpy() for x in c._assoc_state], assoc_np.Tracker(1024, 1.0).state(), "capture moved the state")
    gen = torch.Generator()
    gen.manual_seed(11)
    most = 0
    for t, (_, xy) in enumerate(pushes):
        noise = torch.randn((k, 1, p, v, 2), generator=gen).to(dev)
        ra = a.push(None, xy, noise=noise)
        rb = b.push(ref_ids[t], xy, noise=noise)
        for x, y, name in zip(_fp_fields(ra), _fp_fields(rb), ("ids", "num_peds", "obs_abs", "flags", "samples", "mean",
                                                               "v_pred")):
            assert torch.equal(x, y), (t, name)
        assert np.array_equal(a.det_ids.cpu().numpy(), ref_ids[t]), t
        assert int(a.assoc_flags.item()) == 0
        if tracks is not None:
            assert torch.equal(a.seen, b.seen), t
        # the captured replay against the eager push, both on the Philox stream of seed t
        rc = replay(None, xy, seed=t)
        assert torch.equal(rc.ids, ra.ids) and torch.equal(rc.obs_abs, ra.obs_abs) and torch.equal(rc.mean, ra.mean), t
        assert torch.equal(rc.num_peds, ra.num_peds) and torch.equal(rc.v_pred, ra.v_pred), t
        assert np.array_equal(c.det_ids.cpu().numpy(), ref_ids[t]), t
        for x, y in zip(c._assoc_state, a._assoc_state):
            assert torch.equal(x, y), t
        most = max(most, int(ra.num_peds.item()))
    assert most >= 2
    a.reset()
    _same([x.cpu().numpy() for x in a._assoc_state], assoc_np.Tracker(1024, 1.0).state(), "reset")


def test_captured_samples_equal_the_eager_ones(dev, recs):
    """The same pushes through an eager and a captured predictor with the same seeds: every output equal."""
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    spec = frames.AssociateSpec(1.0, 2.0, 1)
    e = frames.FramePredictor(model, k=2, max_peds=32, max_detections=64, associate=spec)
    c = frames.FramePredictor(model, k=2, max_peds=32, max_detections=64, associate=spec)
    replay = c.capture()
    for t, (_, xy) in enumerate(recs[ZARA1][:30]):
        re_, rc = e.push(None, xy, seed=t), replay(None, xy, seed=t)
        for x, y, name in zip(re_, rc, re_._fields):
            assert torch.equal(x, y), (t, name)
        assert torch.equal(e.det_ids, c.det_ids), t


def test_score_totals_equal_with_associated_ids(dev, recs):
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import ScoreSpec
    pushes = recs[ZARA1][:30]
    spec = frames.AssociateSpec(1.0, 2.0, 0)
    ref_ids = _np_ids(pushes, spec)
    model = _model("eth", dev)
    kw = dict(k=3, max_peds=32, max_detections=64, score=ScoreSpec())
    a = frames.FramePredictor(model, associate=spec, **kw)
    b = frames.FramePredictor(model, **kw)
    for t, (_, xy) in enumerate(pushes):
        a.push(None, xy, seed=t)
        b.push(ref_ids[t], xy, seed=t)
        for x, y in zip(a.score, b.score):
            assert (x is None and y is None) or torch.equal(x, y), t
    for x, y in zip(a.score_totals, b.score_totals):
        assert torch.equal(x, y)
    assert float(a.score_totals[0][0, :, 0].sum()) > 0                   # pedestrians were matched and scored


def test_streams_predictor_equals_lone_predictors(dev, recs):
    """NS = 3 with associate= on a Schedule, explicit noise: each pushed stream's scene, flags, track state, association
    state and predictions equal a lone FramePredictor(associate=...) fed that stream's pushes with noise[:, s:s+1]; a
    stream not pushed keeps its association state bit for bit; reset([s]) clears that stream's alone.  The captured
    tick equals the eager one."""
    from social_stgcnn_amd import frames
    ns, k, v, p = 3, 2, 64, 12
    spec = frames.AssociateSpec(1.0, 2.0, 1, capacity=200)
    pushes = [[xy for _, xy in recs[r][:30]] for r in (ZARA1, UNIV3, HOTEL)]
    model = _model("eth", dev)
    kw = dict(k=k, max_peds=v, max_detections=64, capacity=256, associate=spec)
    sp = frames.StreamsPredictor(model, ns, **kw)
    cp = frames.StreamsPredictor(model, ns, **kw)
    replay = cp.capture()
    lone = [frames.FramePredictor(model, **kw) for _ in range(ns)]
    sched = Schedule(pushes, [0, 2, 1])
    gen = torch.Generator()
    gen.manual_seed(2)
    idle = 0
    for t in range(30):
        tick = [None if d is None else (None, d) for d in sched.tick(t)]
        noise = torch.randn((k, ns, p, v, 2), generator=gen).to(dev)
        before = [[x[s].clone() for x in sp._assoc_state] for s in range(ns)]
        out = sp.push(tick, noise=noise)
        if t % 3 == 0:
            m = sum(len(d[1]) for d in tick if d is not None)
            xy = np.concatenate([d[1] for d in tick if d is not None] + [np.zeros((0, 2))])
            dt = frames.DeviceTick(None, torch.from_numpy(xy).to(dev), [-1 if d is None else len(d[1]) for d in tick])
            cap_out = replay(dt)
            assert m == len(xy)
        else:
            cap_out = replay(tick)
        for name in ("ids", "num_peds", "obs_abs", "mean", "v_pred", "flags", "pushed"):
            assert torch.equal(getattr(out, name), getattr(cap_out, name)), (t, name)
        assert torch.equal(sp.det_ids, cp.det_ids), t
        at = 0
        for s in range(ns):
            mine = [x[s] for x in sp._assoc_state]
            if tick[s] is None:
                idle += 1
                for x, y in zip(mine, before[s]):
                    assert torch.equal(x, y), (t, s)
                continue
            r = lone[s].push(*tick[s], noise=noise[:, s:s + 1])
            n = len(tick[s][1])
            assert torch.equal(sp.det_ids[at:at + n], lone[s].det_ids), (t, s)
            at += n
            assert torch.equal(out.ids[s], r.ids) and torch.equal(out.num_peds[s:s + 1], r.num_peds), (t, s)
            assert torch.equal(out.obs_abs[s:s + 1], r.obs_abs) and torch.equal(out.flags[s:s + 1], r.flags), (t, s)
            assert torch.equal(out.v_pred[s], r.v_pred) and torch.equal(out.mean[s], r.mean), (t, s)
            assert torch.equal(out.samples[:, s], r.samples), (t, s)
            for x, y in zip(mine, lone[s]._assoc_state):
                assert torch.equal(x.reshape(y.shape), y), (t, s)
            for x, y in zip((sp.slot_id[s], sp.mask[s], sp.ring[s], sp.head_flags[s]),
                            (lone[s].slot_id, lone[s].mask, lone[s].ring, lone[s].head_flags)):
                assert torch.equal(x, y), (t, s)
    assert idle >= 3
    keep = [x[0].clone() for x in sp._assoc_state]
    sp.reset([1])
    _same([x[1].cpu().numpy().reshape(y.shape) for x, y in zip(sp._assoc_state, assoc_np.Tracker(200, 1.0).state())],
          assoc_np.Tracker(200, 1.0).state(), "reset([1])")
    for x, y in zip(keep, (x[0] for x in sp._assoc_state)):
        assert torch.equal(x, y)


def test_entry_points_refuse_bad_arguments(dev):
    from social_stgcnn_amd._lib import lib
    L = lib()
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call

    def one(det=f, xy=f, count=f, m_max=8, trk=f, nxt=f, flags=f, c=16, g2=1.0, gn2=4.0, miss=0):
        return L.stg_associate(det, xy, count, m_max, trk, f, f, f, f, nxt, flags, c, 1e4, g2, gn2, miss, None)

    def many(det=f, start=f, pushed=f, ns=4, m_total=16, m_max=8, trk=f, c=16, g2=1.0, gn2=4.0, miss=0, stride=3):
        return L.stg_associate_streams(det, stride, f, 3, m_total, start, pushed, ns, m_max, trk, f, f, f, f, f, f, c, 1e4,
                                       g2, gn2, miss, None)
    inf, nan = float("inf"), float("nan")
    shared = {"null det_id": (dict(det=None), -1), "null trk_id": (dict(trk=None), -1), "M_max=0": (dict(m_max=0), -1),
              "C=0": (dict(c=0), -1), "M_max above the limit": (dict(m_max=2049), -2), "C above the limit": (dict(c=2049), -2),
              "gate2=0": (dict(g2=0.0), -1), "gate2<0": (dict(g2=-1.0), -1), "gate2 inf": (dict(g2=inf, gn2=inf), -1),
              "gate2 nan": (dict(g2=nan), -1), "gate_new2 nan": (dict(gn2=nan), -1), "gate_new2 inf": (dict(gn2=inf), -1),
              "gate_new2 < gate2": (dict(gn2=0.5), -1), "max_miss<0": (dict(miss=-1), -1)}
    for name, (kw, rc) in shared.items():
        assert one(**kw) == rc, name
        assert b"stg_associate:" in L.stg_last_error(), name
        assert many(**kw) == rc, name
        assert b"stg_associate_streams:" in L.stg_last_error(), name
    for name, kw in {"null det_xy": dict(xy=None), "null det_count": dict(count=None), "null next_id": dict(nxt=None),
                     "null assoc_flags": dict(flags=None)}.items():
        assert one(**kw) == -1, name
    for name, kw in {"NS=0": dict(ns=0), "NS too large": dict(ns=4097), "M_total<0": dict(m_total=-1),
                     "M_total too large": dict(m_total=(1 << 23) + 1), "id_stride=0": dict(stride=0),
                     "null det_start": dict(start=None), "null pushed": dict(pushed=None)}.items():
        assert many(**kw) == -1, name
        assert b"stg_associate_streams" in L.stg_last_error(), name


def test_the_command_ignores_the_id_column(dev, recs, tmp_path):
    """predict_frames --associate on the first 40 frames of crowds_zara01 with its id column scrambled: assoc_ids (one per
    row, file order) are the restatement's, and the scenes those of an eager FramePredictor(associate=...)."""
    import argparse
    from social_stgcnn_amd import frames, predict_frames
    from social_stgcnn_amd.trainer import Checkpoint
    model = _model("eth", dev)
    rows = _rows(*ZARA1)
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[39]].copy()
    rows[:, 1] = 7
    rec = str(tmp_path / "noids.txt")
    np.savetxt(rec, rows, fmt=["%d", "%d", "%.17g", "%.17g"], delimiter="\t")
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    out = str(tmp_path / "assoc.npz")
    predict_frames.main(["--checkpoint", ck.dir, "--recording", rec, "--ksteps", "3", "--seed", "3", "--associate",
                         "1.0,2.0,1", "--max_peds", "16", "--out", out])
    npz = np.load(out)
    assert sorted(npz.files) == ["assoc_ids", "frame", "ids", "mean", "num_peds", "samples"]
    pushes = recs[ZARA1][:40]
    spec = frames.AssociateSpec(1.0, 2.0, 1)
    assert np.array_equal(npz["assoc_ids"], np.concatenate(_np_ids(pushes, spec)))
    fp = frames.FramePredictor(model, k=3, max_peds=16, max_detections=max(len(i) for i, _ in pushes), associate=spec)
    keep = []
    for n, (_, xy) in enumerate(pushes):
        r = fp.push(None, xy, seed=3 + n)
        if int(r.num_peds) >= 1:
            keep.append(r)
    v = max(int(r.num_peds) for r in keep)
    assert len(keep) > 20 and np.array_equal(npz["ids"], torch.stack([r.ids[:v] for r in keep]).cpu().numpy())
    assert np.array_equal(npz["mean"], torch.stack([r.mean[:, :v] for r in keep]).cpu().numpy())
    assert np.array_equal(npz["samples"], torch.stack([r.samples[:, :, :v] for r in keep], 1).cpu().numpy())
    with pytest.raises(ValueError, match="--associate does not go together"):
        predict_frames.main(["--checkpoint", ck.dir, "--recording", rec, "--associate", "1", "--step", "10", "--out", out])
