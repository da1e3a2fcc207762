"""GPU: every option of the live predictors in ONE predictor -- tracks=, associate=, score=, harvest=, risk= and
calibration=, push-indexed and with time= -- for FramePredictor and for StreamsPredictor.  What every launch around the
model owns on the device is followed through capture(), the pushes and reset(), bit for bit:

  1. capture() moves nothing: every state tensor, and the harvest log's header, is a never-pushed predictor's;
  2. the captured replay equals the eager push on every push, in everything a push returns or leaves on the predictor, and
     at the end in every state tensor and in the harvested windows;
  3. reset() writes what the class's reset writes (a FramePredictor keeps its rings, the harvest keeps its ring and its
     log), and reset([1]) of the streams leaves stream 0 alone;
  4. the feed does something: scenes of two pedestrians, scored entries, a harvested window.

The feed is biwi_eth's first 40 frames (with time=: upsampled 4x, one push per tick, every 7th left out); of the two
streams, stream 1 is not pushed every third tick and runs on a clock of its own."""
import numpy as np
import pytest
import torch

from harvest_time_np import upsample
from live_inputs import _model, _pushes, _rows

pytestmark = pytest.mark.gpu

ETH = ("eth_test", "biwi_eth.txt")
KW = dict(k=2, max_peds=16, max_detections=32, capacity=64)          # the sizes of test_gpu_assoc_time.py
NS = 2
CLOCK1 = 1000                                                        # stream 1's clock runs this far ahead of stream 0's


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def feeds():
    """timed or not -> [(tick, xy)]: one push of positions per entry."""
    frames40 = _pushes(_rows(*ETH))[:40]
    fine = upsample(frames40, 4)
    return {False: [(n, xy) for n, (_, xy) in enumerate(frames40)],
            True: [(t, xy) for t, (_, xy) in enumerate(fine) if t % 7 != 3]}


def _options(timed):
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.calibrate import Calibration
    from social_stgcnn_amd.predict import RiskSpec, ScoreSpec, TimedScoreSpec
    g = np.exp(np.random.default_rng(2).uniform(-1.0, 3.0, 12)).astype(np.float32)
    kw = dict(KW, tracks=frames.TrackRule(2, 2), risk=RiskSpec(0.5, np.array([[0, 0, 8, 6]], np.float32)),
              calibration=Calibration(g, "coverage", 0.9))
    if timed:
        return dict(kw, time=frames.TimeRule(4, 4, 96), associate=frames.FilteredAssociateSpec(0.05, 1.0),
                    score=TimedScoreSpec(pending=64), harvest=frames.TimedHarvestSpec(64, min_peds=1, settle=0))
    return dict(kw, associate=frames.AssociateSpec(1.0, 2.0, 1), score=ScoreSpec(),
                harvest=frames.HarvestSpec(64, min_peds=1))


def _state(p):
    """Every state tensor of the predictor by a name, and the header of its harvest log."""
    out = {"track.%d" % i: x for i, x in enumerate(p._state)}
    out.update(("assoc.%d" % i, x) for i, x in enumerate(p._assoc_state))
    out.update(("score." + n, x) for n, x in zip(p._score_state._fields, p._score_state) if x is not None)
    out.update(h_word=p.h_word, h_ring=p.h_ring, h_head=p.h_head, header=p.harvest.header)
    if p.h_clock is not None:
        out["h_clock"] = p.h_clock
    return out


def _rings(p):
    """The names in _state(p) of the track rings, which a FramePredictor's reset() leaves."""
    return {"track.%d" % i for i, x in enumerate(p._state)
            if any(x is r for r in (getattr(p, n, None) for n in ("ring", "t_ring", "xy_ring")))}


def _assert_states(a, b, what, skip=(), at=None):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for name in sa:
        if name not in skip:
            x, y = (sa[name], sb[name]) if at is None or name == "header" else (sa[name][at], sb[name][at])
            assert torch.equal(x, y), (what, name)


def _assert_pushes(ra, rc, a, c, n):
    """What a push returns and leaves on the predictor: the eager one's against the captured one's."""
    for name in ra._fields:
        assert torch.equal(getattr(ra, name), getattr(rc, name)), (n, name)
    assert torch.equal(a.seen, c.seen) and torch.equal(a.det_ids, c.det_ids), n
    assert torch.equal(a.assoc_flags, c.assoc_flags), n
    assert type(a.score) is type(c.score)
    for name, x, y in zip(a.score._fields, a.score, c.score):
        assert (x is None and y is None) or torch.equal(x, y), (n, "score", name)
    for name, x, y in zip(a.risk._fields, a.risk, c.risk):
        assert (x is None and y is None) or (x == y if name == "k" else torch.equal(x, y)), (n, "risk", name)


def _assert_logs(a, c):
    n_w, n_r, dropped = a.harvest.counts()
    assert (n_w, n_r, dropped) == c.harvest.counts()
    assert torch.equal(a.harvest.rel_all[:n_r], c.harvest.rel_all[:n_r])
    assert torch.equal(a.harvest.win_start[:n_w + 1], c.harvest.win_start[:n_w + 1])
    assert torch.equal(a.harvest.win_tag[:n_w], c.harvest.win_tag[:n_w])


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_frame_predictor_with_every_option(dev, feeds, timed):
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    fresh, a, c = (frames.FramePredictor(model, **_options(timed)) for _ in range(3))
    replay = c.capture()
    _assert_states(c, fresh, "capture moved the state")
    most = 0
    for n, (t, xy) in enumerate(feeds[timed]):
        when = dict(t=t) if timed else {}
        ra = a.push(None, xy, seed=n, **when)
        rc = replay(None, xy, seed=n, **when)
        _assert_pushes(ra, rc, a, c, n)
        most = max(most, int(ra.num_peds.item()))
    _assert_states(a, c, "the states at the end")
    _assert_logs(a, c)
    assert most >= 2 and float(a.score_totals[0][..., 0].sum()) > 0 and a.harvest.counts()[0] >= 1
    counts = a.harvest.counts()
    a.reset()
    _assert_states(a, fresh, "reset", skip=_rings(a) | {"h_ring", "header"})
    assert a.harvest.counts() == counts


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_streams_predictor_with_every_option(dev, feeds, timed):
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    fresh, a, c = (frames.StreamsPredictor(model, NS, **_options(timed)) for _ in range(3))
    replay = c.capture()
    _assert_states(c, fresh, "capture moved the state")
    most = idle = 0
    for n, (t, xy) in enumerate(feeds[timed]):
        tick, times = {0: (None, xy)}, {0: t}
        if n % 3 != 2:
            tick[1], times[1] = (None, xy), CLOCK1 + t
        else:
            idle += 1
        when = dict(times=times) if timed else {}
        ra = a.push(tick, seed=n, **when)
        rc = replay(tick, seed=n, **when)
        _assert_pushes(ra, rc, a, c, n)
        assert ra.pushed.cpu().tolist() == [True, 1 in tick], n
        most = max(most, int(ra.num_peds.max().item()))
    assert idle >= 10
    _assert_states(a, c, "the states at the end")
    _assert_logs(a, c)
    assert most >= 2 and float(a.score_totals[0][..., 0].sum()) > 0 and a.harvest.counts()[0] >= 1
    counts = a.harvest.counts()
    c.reset([1])
    _assert_states(c, a, "reset([1]) moved stream 0", at=0)
    _assert_states(c, fresh, "reset([1])", skip={"h_ring", "header"}, at=1)
    assert c.harvest.counts() == counts
    a.reset()
    _assert_states(a, fresh, "reset", skip={"h_ring", "header"})
    assert a.harvest.counts() == counts
