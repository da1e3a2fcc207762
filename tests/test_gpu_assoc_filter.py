"""GPU (-m gpu): unlabelled noisy detections -> track ids on timestamped pushes with a filtered track state
(stg_associate_filtered, stg_associate_streams_filtered).

Through the C ABI against the numpy restatement (assoc_filter_np.FilteredTracker), ids, flags and the whole state --
trk_cov included -- bit for bit after every push: ties on an integer grid under irregular times with gaps beyond
max_age, pushes back in time and at the same time, empty pushes and slots running out, the chain that needs one round per
pair, the counts around the wave and the limits, a noisy recording at four pushes per step; the streams kernel against
lone calls, every stream on its own clock; and end to end, FramePredictor / StreamsPredictor with FilteredAssociateSpec
against the same timed predictors fed the restatement's ids, alone and with tracks=, score=TimedScoreSpec and
harvest=TimedHarvestSpec behind it; .assoc_tracks(); the command; the refusals, which launch nothing.  The clock is the
timed push's: where the association runs alone the test moves it as that push would."""
import ctypes

import numpy as np
import pytest
import torch

import assoc_filter_np as AF
import assoc_np
import assoc_time_np as AT
from harvest_time_np import upsample
from live_inputs import CFG, _model, _pushes, _rows

pytestmark = pytest.mark.gpu

ZARA1 = ("zara1_test", "crowds_zara01.txt")
ETH = ("eth_test", "biwi_eth.txt")
HOTEL = ("hotel_test", "biwi_hotel.txt")
UNTOUCHED = -7
SIGMA = 0.05
NOISY = (SIGMA, 1.0, 1.5, 5.0, 2.0)                # sigma_det, sigma_acc, sigma_vel0, gate_sigmas, gate_max
GRID = (0.5, 0.5, 1.0, 2.0, 3.0)


def _sq(par):
    return tuple(float(x) * float(x) for x in par)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ups():
    """The first 60 frames of the recordings upsampled 4x, one push per tick, with 0.05 m of detector noise:
    [(recorded ids, xy)]."""
    return {r: AF.noisy(upsample(_pushes(_rows(*r))[:60], 4), SIGMA, 1) for r in (ZARA1, ETH, HOTEL)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, ref, what):
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), \
            (what, i, np.argwhere(_bits(a) != _bits(b))[:4])


def _p(x):
    return ctypes.c_void_p(x.data_ptr())


class DevState:
    """The filtered association state of `lead` streams on the device, as the C ABI takes it, and the clock(s)."""

    def __init__(self, dev, c, lead=()):
        one = lead or (1,)
        self.t = (torch.full(lead + (c,), -1, device=dev, dtype=torch.int64),
                  torch.zeros(lead + (c, 2), device=dev, dtype=torch.float64),
                  torch.zeros(lead + (c, 2), device=dev, dtype=torch.float64),
                  torch.zeros(lead + (c,), device=dev, dtype=torch.int64),
                  torch.zeros(lead + (c, 3), device=dev, dtype=torch.float64),
                  torch.zeros(lead + (c,), device=dev, dtype=torch.int32),
                  torch.zeros(one, device=dev, dtype=torch.int64), torch.zeros(one, device=dev, dtype=torch.int32))
        self.clock = torch.zeros(lead + (2,), device=dev, dtype=torch.int64)

    def ptrs(self):
        return [_p(x) for x in self.t]


class DevTracker:
    """One stream through stg_associate_filtered; the staging arrays hold `slack` detections past m_max.  The clock moves
    on the host's word, not the kernel's: an accepted push sets {t, pushes + 1} behind the launch."""

    def __init__(self, dev, c, m_max, par, max_age=0, step=4, slack=4):
        from social_stgcnn_amd._lib import lib
        self.lib, self.dev, self.c, self.m_max = lib(), dev, c, m_max
        self.st = DevState(dev, c)
        self.det_id = torch.full((m_max + slack,), UNTOUCHED, device=dev, dtype=torch.int64)
        self.det_xy = torch.zeros((m_max + slack, 2), device=dev, dtype=torch.float64)
        self.count = torch.zeros(1, device=dev, dtype=torch.int32)
        self.when = torch.zeros(1, device=dev, dtype=torch.int64)
        self.rule = (1e4,) + _sq(par) + (step, max_age)
        self.host_clock = [0, 0]

    def push(self, xy, t):
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        n = len(xy)
        self.det_id.fill_(UNTOUCHED)
        if n:
            self.det_xy[:n].copy_(torch.from_numpy(xy))
        self.count.fill_(n)
        self.when.fill_(t)
        clock0 = self.st.clock.clone()
        rc = self.lib.stg_associate_filtered(_p(self.det_id), _p(self.det_xy), _p(self.count), _p(self.when),
                                             _p(self.st.clock), self.m_max, *self.st.ptrs(), self.c, *self.rule, None)
        assert rc == 0, self.lib.stg_last_error()
        assert torch.equal(self.st.clock, clock0)            # the clock is the push's: read only here
        if not (self.host_clock[1] > 0 and t <= self.host_clock[0]):
            self.host_clock = [t, self.host_clock[1] + 1]
            self.st.clock.copy_(torch.tensor(self.host_clock, dtype=torch.int64))
        ids = self.det_id.cpu().numpy()
        m = min(n, self.m_max)
        assert np.all(ids[m:] == UNTOUCHED)                 # past the count, and past M_max: not touched
        return ids[:m]

    def state(self):
        return [x.cpu().numpy() for x in self.st.t]


def _pair(dev, c, m_max, par, max_age=0, step=4):
    return (DevTracker(dev, c, m_max, par, max_age, step), AF.FilteredTracker(c, *par, max_age, step, m_max=m_max))


def _push_both(pair, xy, t, what):
    d, r = pair
    got, ref = d.push(xy, t), r.push(xy, t)
    assert np.array_equal(got, ref), (what, got[:12], ref[:12])
    _same(d.state(), r.state(), what)
    assert d.host_clock == r.clock, what
    return got


# ---- 1. through the C ABI -----------------------------------------------------------------------------------------------
def test_grid_ties_irregular_times_refusal_empty_pushes_and_full_slots(dev):
    """C = 16, M_max = 8, step 4, max_age 5, dyadic sigmas: detections on an integer grid (equal costs: the order
    (cost, s, j) decides), inter-push times from {1, 2, 3, 4, 7} -- 7 is beyond max_age, so every track not matched then is freed, the
    others are left as they are --, every ninth push back in time or at the same time (refused: ids -1, the flag, the
    state bit for bit), empty pushes, and more births than free slots."""
    gen = np.random.default_rng(3)
    pair = _pair(dev, 16, 8, GRID, max_age=5)
    t, seen, tied, aged_out, kept_over_gap = 1000, 0, 0, 0, 0
    for n in range(72):
        dt = int(gen.choice([1, 2, 3, 4, 7]))
        m = 0 if n % 13 == 6 else int(gen.integers(1, 12))               # up to M_max + 3 given
        xy = gen.integers(0, 9, size=(m, 2)).astype(np.float64)
        if n % 9 == 8:
            before = pair[0].state()
            ids = _push_both(pair, xy, t - (n % 2) * 5, ("refused", n))
            assert ids.tolist() == [-1] * min(m, 8)
            _same(pair[0].state()[:7], before[:7], ("refused: the state", n))
            seen |= int(pair[0].state()[7][0])
            continue
        t += dt
        live0 = pair[1].trk_id >= 0
        old = (t - pair[1].trk_t > 5) & live0
        ids = _push_both(pair, xy, t, n)
        assert len(set(ids.tolist())) == min(m, 8) and (ids >= 0).all()
        seen |= int(pair[0].state()[7][0])
        tied += min(m, 8) - len(np.unique(xy[:8], axis=0))
        aged_out += int(old.sum())
        kept_over_gap += int((live0 & (pair[1].trk_t < t) & (pair[1].trk_id >= 0) & ~old).sum())
    assert seen == (assoc_np.FULL | AT.TIME_ORDER) and tied > 10 and aged_out > 5 and kept_over_gap > 20


def test_chain_needs_one_round_per_pair(dev):
    """t0 d0 t1 d1 ... t7 d7 on a line with strictly decreasing gaps, three quarters of a step after the births (one-sample
    tracks predict their own position whatever the gap): only (t7, d7) is mutually best at first and a round-based kernel
    needs 8 rounds.  The result is t_i - d_i.  (The gate is wide open: 100 sigmas, gate_max 100.)"""
    gaps = np.arange(16, 0, -1) / 8.0
    x = np.concatenate([[0.0], np.cumsum(gaps)])[:16]
    line = lambda v: np.stack([v, np.zeros_like(v)], 1)                 # noqa: E731
    for rev in (False, True):
        pair = _pair(dev, 16, 8, (0.5, 0.0, 1.0, 100.0, 100.0))
        assert _push_both(pair, line(x[0::2]), 40, "births").tolist() == list(range(8))
        d = x[1::2][::-1] if rev else x[1::2]
        assert _push_both(pair, line(d), 43, "chain").tolist() == list(range(8))[::-1 if rev else 1]
        assert (pair[0].state()[5][:8] == 2).all()


def test_detection_counts_around_the_wave_and_the_limit(dev):
    """m = 0, 1, 63, 64, 65, M_max and M_max + 3 (the first M_max used, the others not touched) with C = 1100 slots: not
    a multiple of the 1024-thread workgroup, so the slot loops run a partial second pass.  Irregular times, step 4,
    max_age 6."""
    gen = np.random.default_rng(5)
    m_max = 140
    pair = _pair(dev, 1100, m_max, (0.02, 1.0, 1.5, 5.0, 1.0), max_age=6)
    pos, vel = gen.uniform(-30, 30, size=(m_max + 3, 2)), gen.uniform(-0.08, 0.08, size=(m_max + 3, 2))
    t = -50
    for n, m in enumerate((64, 0, 1, 63, 64, 65, m_max, m_max + 3, 65, m_max + 3, 0, m_max)):
        dt = (1, 2, 3, 4, 7)[n % 5]
        t += dt
        pos = pos + vel * dt
        ids = _push_both(pair, pos[:m], t, (n, m))
        assert len(ids) == min(m, m_max)
    assert int(pair[1].next_id) > m_max                      # births went on after the first full push


def test_both_limits_at_once(dev):
    """C = 2,048 and M_max = 2,048: 114,688 bytes of LDS, 36 per slot and 20 per detection.  Three pushes of a few
    detections each, the slot loops in two full passes."""
    pair = _pair(dev, 2048, 2048, NOISY, max_age=8)
    xy = np.array([[0.0, 0.0], [3.0, 1.0], [-2.0, 5.0], [7.5, 7.5], [1.0, -4.0]])
    assert _push_both(pair, xy, 10, "births").tolist() == [0, 1, 2, 3, 4]
    assert _push_both(pair, xy[::-1] + 0.03, 12, "matched").tolist() == [4, 3, 2, 1, 0]
    assert _push_both(pair, xy[1:4] - 0.02, 15, "three of five").tolist() == [1, 2, 3]


def test_a_noisy_recording_at_four_pushes_per_step(dev, ups):
    """60 pushes of crowds_zara01 upsampled 4x with 0.05 m of noise, every seventh left out, step 4, max_age 8."""
    pushes = ups[ZARA1][:60]
    pair = _pair(dev, 64, max(len(i) for i, _ in pushes), NOISY, max_age=8)
    for t, (_, xy) in enumerate(pushes):
        if t % 7 != 3:
            _push_both(pair, xy, t, t)
    assert int(pair[1].next_id) >= 5


def test_streams_equal_lone_calls_on_their_own_clocks(dev, ups):
    """NS = 3, packed (id, x, y) records at strides 3 / 3, C = 333 (a partial second pass of the 256 threads): stream 0
    pushes every tick, stream 1 skips every third tick (idle: state and id fields untouched), stream 2 starts late, has an
    empty push and a push back in time (refused: ids -1, its flag, nothing else).  Every stream equals a lone
    stg_associate_filtered and the restatement fed its pushes at its times."""
    from social_stgcnn_amd._lib import lib
    L = lib()
    ns, c, m_max, cap = 3, 333, 24, 96
    feeds = [[xy for _, xy in ups[r][:40]] for r in (ETH, ZARA1, HOTEL)]
    feeds[2][7] = np.zeros((0, 2))
    clock0 = (0, 10 ** 12, -300)
    st = DevState(dev, c, (ns,))
    lone = [DevTracker(dev, c, m_max, NOISY, 5) for _ in range(ns)]
    refs = [AF.FilteredTracker(c, *NOISY, 5, 4, m_max=m_max) for _ in range(ns)]
    rec = torch.zeros((cap, 3), device=dev, dtype=torch.float64)
    rec_i = rec.view(torch.int64)
    cursor = [0, 0, 0]
    idle = empty = refused = 0
    for n in range(44):
        tick, when = [], []
        for s in range(ns):
            go = cursor[s] < len(feeds[s]) and not (s == 1 and n % 3 == 2) and not (s == 2 and n < 4)
            tick.append(feeds[s][cursor[s]] if go else None)
            back = 6 if (s == 2 and cursor[s] == 20) else 0
            when.append(clock0[s] + n - back)
            cursor[s] += int(go)
        counts = [0 if d is None else len(d) for d in tick]
        assert max(counts) <= m_max
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
        when_d = torch.tensor(when, dtype=torch.int64).to(dev)
        before = [[x[s].clone() for x in st.t] for s in range(ns)]
        rc = L.stg_associate_streams_filtered(_p(rec_i), 3, ctypes.c_void_p(rec.data_ptr() + 8), 3, cap, _p(start_d),
                                              _p(pushed_d), _p(when_d), _p(st.clock), ns, m_max, *st.ptrs(), c, 1e4,
                                              *_sq(NOISY), 4, 5, None)
        assert rc == 0, L.stg_last_error()
        ids = rec_i[:, 0].cpu().numpy()
        assert np.all(ids[start[-1]:] == UNTOUCHED), n
        for s, d in enumerate(tick):
            mine = [x[s].cpu().numpy().reshape(y.shape) for x, y in zip(st.t, refs[s].state())]
            if d is None:
                idle += 1
                _same(mine, [x.cpu().numpy().reshape(y.shape) for x, y in zip(before[s], mine)], (n, s, "idle"))
                continue
            empty += int(len(d) == 0)
            got = ids[start[s]:start[s + 1]]
            want = refs[s].push(d, when[s])
            assert np.array_equal(got, lone[s].push(d, when[s])) and np.array_equal(got, want), (n, s)
            if refs[s].flags == AT.TIME_ORDER:
                refused += 1
                assert got.tolist() == [-1] * len(d)
            _same(mine, lone[s].state(), (n, s, "lone"))
            _same(mine, refs[s].state(), (n, s, "restatement"))
            st.clock[s].copy_(torch.tensor(refs[s].clock, dtype=torch.int64))     # as the push behind it would
    assert idle > 12 and empty == 1 and refused == 1


def test_the_refusals_launch_nothing(dev):
    """Bad arguments with real buffers behind them: the status, the message, and nothing written -- ids, state, clock."""
    from social_stgcnn_amd._lib import lib
    L = lib()
    d = DevTracker(dev, 16, 8, NOISY)
    d.push([[0.0, 0.0], [3.0, 0.0]], 5)
    d.det_id.fill_(UNTOUCHED)
    d.count.fill_(2)
    d.when.fill_(9)
    kept = d.st.t + (d.st.clock, d.det_id)
    before = [x.clone() for x in kept]
    start = torch.tensor([0, 2], device=dev, dtype=torch.int32)
    pushed = torch.ones(1, device=dev, dtype=torch.int32)

    def one(m_max=8, c=16, r=0.0025, qa=1.0, v0=2.25, n2=25.0, gmax2=4.0, step=4, max_age=0):
        return L.stg_associate_filtered(_p(d.det_id), _p(d.det_xy), _p(d.count), _p(d.when), _p(d.st.clock), m_max,
                                        *d.st.ptrs(), c, 1e4, r, qa, v0, n2, gmax2, step, max_age, None)

    def many(m_max=8, c=16, r=0.0025, qa=1.0, v0=2.25, n2=25.0, gmax2=4.0, step=4, max_age=0, ns=1):
        return L.stg_associate_streams_filtered(_p(d.det_id), 1, _p(d.det_xy), 2, 8, _p(start), _p(pushed), _p(d.when),
                                                _p(d.st.clock), ns, m_max, *d.st.ptrs(), c, 1e4, r, qa, v0, n2, gmax2,
                                                step, max_age, None)
    for kw, rc in ((dict(m_max=0), -1), (dict(c=0), -1), (dict(r=0.0), -1), (dict(qa=-1.0), -1), (dict(v0=0.0), -1),
                   (dict(n2=float("inf")), -1), (dict(gmax2=float("nan")), -1), (dict(step=0), -1),
                   (dict(max_age=-1), -1), (dict(max_age=1 << 31), -1),
                   (dict(m_max=2049), -2), (dict(c=2049), -2), (dict(step=1 << 31), -2)):
        assert one(**kw) == rc, kw
        assert L.stg_last_error().startswith(b"stg_associate_filtered:"), kw
        assert many(**kw) == rc, kw
        assert L.stg_last_error().startswith(b"stg_associate_streams_filtered:"), kw
    assert many(ns=0) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, before))


# ---- 2. the predictors ----------------------------------------------------------------------------------------------------
KW = dict(k=2, max_peds=16, max_detections=32, capacity=64)
STEP = 4


def _rule():
    from social_stgcnn_amd import frames
    return frames.TimeRule(STEP, STEP, 96)


def _np_ids(pushes, times, spec, cap=64):
    trk = AF.FilteredTracker(cap, *spec[:6], STEP)
    return [trk.push(xy, t) for (_, xy), t in zip(pushes, times)], trk


def _extras(variant):
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    return {"plain": {}, "tracks": dict(tracks=frames.TrackRule(2, 2)), "score": dict(score=TimedScoreSpec(pending=64)),
            "harvest": dict(harvest=frames.TimedHarvestSpec(64, min_peds=1, settle=0))}[variant]


def _assert_behind(a, b, variant, what):
    """what runs behind the push, equal in the two predictors"""
    if variant == "score":
        for x, y in zip(a.score_totals, b.score_totals):
            assert torch.equal(x, y), what
    if variant == "harvest":
        n_w, n_r, dropped = a.harvest.counts()
        assert (n_w, n_r, dropped) == b.harvest.counts(), what
        assert torch.equal(a.harvest.rel_all[:n_r], b.harvest.rel_all[:n_r]), what
        assert torch.equal(a.harvest.win_start[:n_w + 1], b.harvest.win_start[:n_w + 1]), what
        assert np.array_equal(a.harvest.tags(), b.harvest.tags()), what


@pytest.mark.parametrize("variant", ["plain", "tracks", "score", "harvest"])
def test_frame_predictor_equals_one_fed_the_restatements_ids(dev, ups, variant):
    """biwi_eth's first 60 frames upsampled 4x with 0.05 m of noise, one push per tick, every 7th left out (so max_age
    = 2 steps is used): FramePredictor(time=, associate=FilteredAssociateSpec) fed (None, xy, t) equals the same timed predictor fed (the
    restatement's ids, xy, t) -- scene, seen, flags, samples, mean and v_pred --, eager and as the captured replay;
    .det_ids are the restatement's ids, the association state its state and .assoc_tracks() its live slots.  Also with tracks=TrackRule(2, 2), with
    score=TimedScoreSpec (the totals equal) and with harvest=TimedHarvestSpec (the log equal)."""
    from social_stgcnn_amd import frames
    keep = [t for t in range(len(ups[ETH])) if t % 7 != 3]
    pushes, times = [ups[ETH][t] for t in keep], keep
    spec = frames.FilteredAssociateSpec(*NOISY, max_age=2 * STEP)
    ref_ids, trk = _np_ids(pushes, times, spec)
    model = _model("eth", dev)
    kw = dict(KW, time=_rule(), **_extras(variant))
    a = frames.FramePredictor(model, associate=spec, **kw)
    c = frames.FramePredictor(model, associate=spec, **kw)
    b = frames.FramePredictor(model, **kw)
    fresh = AF.FilteredTracker(64, *NOISY, 2 * STEP, STEP).state()
    replay = c.capture()
    _same([x.cpu().numpy() for x in c._assoc_state], fresh, "capture moved the state")
    assert not c.clock.any()
    most = 0
    for n, ((_, xy), t) in enumerate(zip(pushes, times)):
        ra = a.push(None, xy, t=t, seed=n)
        rb = b.push(ref_ids[n], xy, t=t, seed=n)
        rc = replay(None, xy, t=t, seed=n)
        for name in ra._fields:
            assert torch.equal(getattr(ra, name), getattr(rb, name)), (n, name)
            assert torch.equal(getattr(rc, name), getattr(rb, name)), (n, name, "captured")
        assert torch.equal(a.seen, b.seen) and torch.equal(c.seen, b.seen), n
        assert np.array_equal(a.det_ids.cpu().numpy(), ref_ids[n]) and torch.equal(c.det_ids, a.det_ids), n
        assert int(a.assoc_flags.item()) == 0 == int(c.assoc_flags.item())
        most = max(most, int(ra.num_peds.item()))
    assert most >= 2
    _same([x.cpu().numpy() for x in a._assoc_state], trk.state(), "the state at the end")
    _same([x.cpu().numpy() for x in c._assoc_state], trk.state(), "the captured state at the end")
    _assert_behind(a, b, variant, "eager")
    _assert_behind(c, b, variant, "captured")
    if variant == "plain":
        with pytest.raises(ValueError, match="needs associate="):
            b.assoc_tracks()
        dev_view, host_copy = a.assoc_tracks(), c.assoc_tracks(host=True)
        assert all(x.is_cuda for x in dev_view) and len(trk.live()[0]) >= 2
        _same([x.cpu().numpy() for x in dev_view], trk.live(), "assoc_tracks()")
        _same(host_copy, trk.live(), "assoc_tracks(host=True)")
    if variant == "score":
        assert float(a.score_totals[0][..., 0].sum()) > 0
    if variant == "harvest":
        assert a.harvest.counts()[0] >= 1
    # a push back in time: refused by the association and by the push, nothing moved; then reset()
    state = [x.clone() for x in a._assoc_state[:7]] + [a.clock.clone()]
    r = a.push(None, pushes[-1][1], t=times[-1])
    assert int(r.flags.item()) == frames.TIME_ORDER and int(a.assoc_flags.item()) == frames.ASSOC_TIME_ORDER
    assert a.det_ids.cpu().tolist() == [-1] * len(pushes[-1][1])
    assert all(torch.equal(x, y) for x, y in zip(state, list(a._assoc_state[:7]) + [a.clock]))
    a.reset()
    _same([x.cpu().numpy() for x in a._assoc_state], fresh, "reset")
    assert not a.clock.any()


def test_streams_predictor_equals_one_fed_the_restatements_ids(dev, ups):
    """NS = 3 on their own clocks with tracks=TrackRule(2, 2), score= and harvest= behind the association: stream 0 every
    tick, stream 1 idle every third tick, stream 2 late and with an empty push.  StreamsPredictor(associate=
    FilteredAssociateSpec) fed (None, xy) equals the same predictor fed the restatement's ids, eager and captured (host ticks
    and DeviceTicks); a stream not pushed keeps its association state; reset([1]) clears that stream's alone, with its
    clock; .assoc_tracks() gives every stream's live slots."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    ns = 3
    spec = frames.FilteredAssociateSpec(*NOISY, max_age=STEP, capacity=48)
    feeds = [[xy for _, xy in ups[r][:90]] for r in (ETH, ZARA1, HOTEL)]
    feeds[2][9] = np.zeros((0, 2))
    clock0 = (0, 5000, -300)
    model = _model("eth", dev)
    kw = dict(KW, time=_rule(), tracks=frames.TrackRule(2, 2), score=TimedScoreSpec(pending=64),
              harvest=frames.TimedHarvestSpec(64, min_peds=1))
    sp = frames.StreamsPredictor(model, ns, associate=spec, **kw)
    cp = frames.StreamsPredictor(model, ns, associate=spec, **kw)
    bp = frames.StreamsPredictor(model, ns, **kw)
    replay = cp.capture()
    refs = [AF.FilteredTracker(48, *NOISY, STEP, STEP) for _ in range(ns)]
    cursor = [0, 0, 0]
    idle = 0
    for n in range(96):
        tick, fed, when = {}, {}, {}
        for s in range(ns):
            if cursor[s] < len(feeds[s]) and not (s == 1 and n % 3 == 2) and not (s == 2 and n < 5):
                xy = feeds[s][cursor[s]]
                cursor[s] += 1
                when[s] = clock0[s] + n
                tick[s], fed[s] = (None, xy), (refs[s].push(xy, when[s]), xy)
        before = [[x[s].clone() for x in sp._assoc_state] for s in range(ns)]
        out = sp.push(tick, times=when, seed=n)
        ref = bp.push(fed, times=when, seed=n)
        if n % 2:
            cap_out = replay(tick, times=when, seed=n)
        else:
            xy = np.concatenate([tick[s][1] for s in sorted(tick)] + [np.zeros((0, 2))])
            t_dev = torch.tensor([when.get(s, 0) for s in range(ns)], dtype=torch.int64).to(dev)
            cap_out = replay(frames.DeviceTick(None, torch.from_numpy(xy).to(dev),
                                               [len(tick[s][1]) if s in tick else -1 for s in range(ns)]),
                             times=t_dev, seed=n)
        for name in out._fields:
            assert torch.equal(getattr(out, name), getattr(ref, name)), (n, name)
            assert torch.equal(getattr(cap_out, name), getattr(ref, name)), (n, name, "captured")
        assert torch.equal(sp.seen, bp.seen) and torch.equal(cp.seen, bp.seen), n
        want = np.concatenate([fed[s][0] for s in sorted(fed)] + [np.zeros(0, np.int64)])
        assert np.array_equal(sp.det_ids.cpu().numpy(), want) and torch.equal(cp.det_ids, sp.det_ids), n
        for s in range(ns):
            if s not in tick:
                idle += 1
                assert all(torch.equal(x[s], y) for x, y in zip(sp._assoc_state, before[s])), (n, s)
    assert idle > 30 and not sp.assoc_flags.any()
    for s in range(ns):
        for p in (sp, cp):
            _same([x[s].cpu().numpy().reshape(y.shape) for x, y in zip(p._assoc_state, refs[s].state())],
                  refs[s].state(), (s, p is cp))
    for p in (sp, cp):
        for x, y in zip(p.score_totals, bp.score_totals):
            assert torch.equal(x, y)
        _assert_behind(p, bp, "harvest", p is cp)
    assert float(sp.score_totals[0][..., 0].sum()) > 0 and sp.harvest.counts()[0] >= 1
    for s, got in enumerate(sp.assoc_tracks(host=True)):
        _same(got, refs[s].live(), ("assoc_tracks", s))
    keep = [x[0].clone() for x in sp._assoc_state] + [sp.clock[0].clone()]
    sp.reset([1])
    fresh = AF.FilteredTracker(48, *NOISY).state()
    _same([x[1].cpu().numpy().reshape(y.shape) for x, y in zip(sp._assoc_state, fresh)], fresh, "reset([1])")
    assert not sp.clock[1].any()
    assert all(torch.equal(x, y) for x, y in zip(keep, [x[0] for x in sp._assoc_state] + [sp.clock[0]]))


# ---- 3. the command ---------------------------------------------------------------------------------------------------------
def test_the_command_ignores_the_id_column_of_a_timed_recording(dev, ups, tmp_path):
    """predict_frames --step 4 --associate_filtered on crowds_zara01 upsampled 4x with 0.05 m of noise, written with the tick as its frame column
    and a scrambled id column: assoc_ids (one per row, file order) are the restatement's, the scenes those of an eager
    FramePredictor fed the restatement's ids; together with --score and --harvest_timed; --associate with --step is still
    refused.  (A file holds what repr() round-trips: the detections are already rounded to 4 decimals.)"""
    import argparse
    import pickle
    from social_stgcnn_amd import frames
    from social_stgcnn_amd import predict_frames as pf
    ck = tmp_path / "ck"
    ck.mkdir()
    model = _model("zara1", dev)
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, ck / "val_best.pth")
    with open(ck / "args.pkl", "wb") as fh:
        pickle.dump(argparse.Namespace(n_stgcnn=CFG["n_stgcnn"], n_txpcnn=CFG["n_txpcnn"], output_size=CFG["output_feat"],
                                       obs_seq_len=CFG["seq_len"], kernel_size=CFG["kernel_size"],
                                       pred_seq_len=CFG["pred_seq_len"]), fh)
    feed = [(t, xy) for t, (i, xy) in enumerate(ups[ZARA1][:120]) if len(i) and t % 7 != 3]     # (no empty push in a file)
    rec = tmp_path / "noids.txt"
    with open(rec, "w") as fh:
        for t, xy in feed:
            for p in xy:
                fh.write("%s\t7.0\t%s\t%s\n" % (repr(float(t)), repr(float(p[0])), repr(float(p[1]))))
    out, kept = str(tmp_path / "p.npz"), str(tmp_path / "w.npz")
    pf.main(["--checkpoint", str(ck), "--recording", str(rec), "--ksteps", "2", "--seed", "3", "--step", "4",
             "--associate_filtered", "0.05,1.0,1.5,5.0,2.0,8", "--score", "--pending", "64", "--harvest_timed", "50",
             "--harvest_out", kept,
             "--max_peds", "16", "--out", out])
    npz = np.load(out)
    assert {"assoc_ids", "time", "ids", "mean", "samples", "seen", "score_count"} <= set(npz.files)
    spec = frames.FilteredAssociateSpec(*NOISY, max_age=8)
    trk = AF.FilteredTracker(1024, *NOISY, 8, 4)
    ref_ids = [trk.push(xy, t) for t, xy in feed]
    assert np.array_equal(npz["assoc_ids"], np.concatenate(ref_ids))
    fp = frames.FramePredictor(model, k=2, max_peds=16, max_detections=max(len(xy) for _, xy in feed), time=_rule(),
                               associate=spec)
    rows = []
    for n, (t, xy) in enumerate(feed):
        r = fp.push(None, xy, t=t, seed=3 + n)
        if int(r.num_peds) >= 1:
            rows.append((t, r))
    v = max(int(r.num_peds) for _, r in rows)
    assert len(rows) > 40 and npz["time"].tolist() == [t for t, _ in rows]
    assert np.array_equal(npz["ids"], torch.stack([r.ids[:v] for _, r in rows]).cpu().numpy())
    assert np.array_equal(npz["mean"], torch.stack([r.mean[:, :v] for _, r in rows]).cpu().numpy())
    assert np.array_equal(npz["samples"], torch.stack([r.samples[:, :, :v] for _, r in rows], 1).cpu().numpy())
    assert int(npz["score_count"].sum()) > 0 and len(np.load(kept)["tags"]) >= 1
    with pytest.raises(ValueError, match="--associate does not go together with --step or --radius / --zones"):
        pf.main(["--checkpoint", str(ck), "--recording", str(rec), "--associate", "1", "--step", "4", "--out", out])
