"""CPU: the timed live rule (frames.TimeRule) as tests/frames_time_np.py states it: on a feed of one
push per step it is the push-by-push rule of tests/frames_fill_np.py on the six test recordings; a hand-worked window;
time going backwards; and what TimeRule, the predictors and the two C entry points refuse, without a device."""
import ctypes
import os

import numpy as np
import pytest

import frames_fill_np
from frames_time_np import DUPLICATE, OVERFLOW, TIME_ORDER, TOO_MANY, TRUNCATED, StreamModelTimed
from live_inputs import _pushes, _rows

TEST_RECORDINGS = (("eth_test", "biwi_eth.txt"), ("hotel_test", "biwi_hotel.txt"), ("univ_test", "students001.txt"),
                   ("univ_test", "students003.txt"), ("zara1_test", "crowds_zara01.txt"),
                   ("zara2_test", "crowds_zara02.txt"))


@pytest.mark.parametrize("rule", [(8, 0), (2, 2)])
@pytest.mark.parametrize("rec", TEST_RECORDINGS)
def test_one_push_per_step_is_the_frame_index_rule(rec, rule):
    """t = 10 * (frame index), max_dt = step = 10: every instant of a window is a push's time, so a step is observed
    iff the id was in that push, and nothing is interpolated.  max_peds 16 cuts the crowded scenes (TOO_MANY)."""
    pushes = _pushes(_rows(*rec))
    a = frames_fill_np.StreamModelRule(8, rule[0], rule[1], max_peds=16)
    b = StreamModelTimed(8, 10, 10, history=8 + len(rec[1]) % 3, min_seen=rule[0], max_gap=rule[1], max_peds=16)
    cut = some = 0
    for f, (ids, xy) in enumerate(pushes):
        r_ids, r_obs, r_seen, more = a.push(ids, xy)
        g_ids, g_obs, g_seen, flags = b.push(ids, xy, 10 * f)
        assert np.array_equal(r_ids, g_ids) and np.array_equal(r_obs, g_obs) and np.array_equal(r_seen, g_seen), (rec, f)
        assert g_seen.dtype == np.int32 and flags == (TOO_MANY if more else 0), (rec, f)
        cut, some = cut + int(more), some + len(g_ids)
    assert some > 500 and (cut > 0 or rec[0] != "univ_test")


def test_a_hand_worked_window():
    """obs_len 4, step 10, max_dt 10, decimals 4, TrackRule(2, 2); the push at t = 100 looks at the instants 70, 80,
    90, 100.

    id 1, exact: samples at 70, 80, 90, 100 = (1,1) (2,1) (3,1) (4,1): the window is the samples, seen 0b1111.

    id 2, off the grid, samples (t: x, y)  66: 1.0, 0.0   73: 2.4, 0.7   78: 3.4, 1.2   85: 4.8, 1.9   93: 6.4, 2.7
    100: 7.5, 3.3:
        70  between 66 and 73 (7 apart), w = 4/7:  x = 1.0 + 1.4 * 4/7 = 1.8,    y = 0.0 + 0.7 * 4/7 = 0.4
        80  between 78 and 85 (7 apart), w = 2/7:  x = 3.4 + 1.4 * 2/7 = 3.8,    y = 1.2 + 0.7 * 2/7 = 1.4
        90  between 85 and 93 (8 apart), w = 5/8:  x = 4.8 + 1.6 * 0.625 = 5.8,  y = 1.9 + 0.8 * 0.625 = 2.4
        100 its own sample: 7.5, 3.3
    every step observed: seen 0b1111 although no earlier sample is on the grid.

    id 3, samples 70: (0,5)  80: (1,5)  95: (2.8,5)  100: (3,5): the instant 90 lies between 80 and 95, 15 apart and
    wider than max_dt, so step 2 is missed (seen 0b1101) and is FILLED from steps 1 and 3, x = 1 + (3 - 1) * 1/2 = 2.0
    -- not 2.2, which the interpolation in time, 1 + 1.8 * 10/15, would give."""
    tracks = {1: [(70, 1, 1), (80, 2, 1), (90, 3, 1), (100, 4, 1)],
              2: [(66, 1.0, 0.0), (73, 2.4, 0.7), (78, 3.4, 1.2), (85, 4.8, 1.9), (93, 6.4, 2.7), (100, 7.5, 3.3)],
              3: [(70, 0, 5), (80, 1, 5), (95, 2.8, 5), (100, 3, 5)]}
    m = StreamModelTimed(4, 10, 10, history=8, min_seen=2, max_gap=2)
    for t in sorted({s[0] for smp in tracks.values() for s in smp}):
        det = [(i, s[1:]) for i, smp in sorted(tracks.items(), reverse=True) for s in smp if s[0] == t]
        ids, obs, seen, flags = m.push([d[0] for d in det], [d[1] for d in det], t)
        assert flags == 0
    assert ids.tolist() == [1, 2, 3] and seen.tolist() == [0b1111, 0b1111, 0b1101]
    assert obs[:, 0].tolist() == [[1, 1], [2, 1], [3, 1], [4, 1]]
    assert obs[:, 1].tolist() == [[1.8, 0.4], [3.8, 1.4], [5.8, 2.4], [7.5, 3.3]]
    assert obs[:, 2].tolist() == [[0, 5], [1, 5], [2.0, 5], [3, 5]]
    # with max_dt = 15 the bracket holds and step 2 is observed at the interpolated 2.2
    m = StreamModelTimed(4, 10, 15, history=8, min_seen=2, max_gap=2)
    for t in (70, 80, 95, 100):
        ids, obs, seen, _ = m.push([3], [[s[1:] for s in tracks[3] if s[0] == t][0]], t)
    assert seen.tolist() == [0b1111] and obs[:, 0].tolist() == [[0, 5], [1, 5], [2.2, 5], [3, 5]]
    # a history of 2 samples keeps (95, 100) only: steps 0-2 are lost, one step seen is below min_seen
    m = StreamModelTimed(4, 10, 10, history=2, min_seen=2, max_gap=2)
    for t in (70, 80, 95, 100):
        ids, obs, seen, _ = m.push([3], [[s[1:] for s in tracks[3] if s[0] == t][0]], t)
    assert len(ids) == 0 and m.tracks[3] == [(95, 2.8, 5.0), (100, 3.0, 5.0)]


def test_time_must_move_forward_and_tracks_expire():
    m = StreamModelTimed(4, 10, 10, history=4, min_seen=2, max_gap=2, capacity=2, max_detections=3)
    assert m.push([5], [[0, 0]], -40)[3] == 0                     # the first push takes any time
    ids, obs, seen, flags = m.push([5, 5], [[1, 1], [9, 9]], -30)
    assert ids.tolist() == [5] and flags == DUPLICATE and obs[:, 0].tolist() == [[-2, -2], [-1, -1], [0, 0], [1, 1]]
    before = m.state()
    for t in (-30, -31, -1000):
        ids, obs, seen, flags = m.push([5, 6], [[2, 2], [3, 3]], t)
        assert flags == TIME_ORDER and len(ids) == 0 and obs.shape == (4, 0, 2) and len(seen) == 0
        assert m.state() == before
    # two places: 5 lives, 6 takes the free one, 7 finds none; the fourth detection is past max_detections
    ids, _, seen, flags = m.push([5, 6, 7, 8], np.zeros((4, 2)), -20)
    assert flags == OVERFLOW | TRUNCATED and ids.tolist() == [5] and seen.tolist() == [0b111]
    assert sorted(m.tracks) == [5, 6]
    # 30 ticks after its newest sample a track still lives, 31 ticks after it is forgotten with its samples
    assert m.push([6], [[0, 0]], 10)[0].tolist() == [6] and sorted(m.tracks) == [5, 6]
    ids, _, _, flags = m.push([5], [[0, 0]], 11)
    assert len(ids) == 0 and flags == 0 and m.tracks[5] == [(11, 0.0, 0.0)]


def test_time_rule_and_push_refusals():
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import FramePredictor, StreamsPredictor, TimeRule
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import ScoreSpec
    assert TimeRule(10) == (10, None, 96) and TimeRule(10).checked(8) == (10, 10, 96)
    assert TimeRule(400000, 1200000, 2).checked(8) == (400000, 1200000, 2) and frames.TIME_ORDER == 16
    for bad in (0, -1, 2.5, True, 1 << 31):
        with pytest.raises(ValueError, match="step must be an integer"):
            TimeRule(bad)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="max_dt must be None or an integer"):
            TimeRule(10, bad)
    for bad in (1, 257, 0, 8.5):
        with pytest.raises(ValueError, match=r"history must be an integer in \[2, 256\]"):
            TimeRule(10, history=bad)
    with pytest.raises(ValueError, match=r"max_dt=71 > \(obs_len - 1\) \* step = 70"):
        TimeRule(10, 71).checked(8)
    with pytest.raises(ValueError, match="below 2\\^31"):
        TimeRule(1 << 28).checked(8)
    model = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
    for make in (lambda **kw: FramePredictor(model, **kw), lambda **kw: StreamsPredictor(model, 3, **kw)):
        with pytest.raises(ValueError, match="max_dt=71"):
            make(time=TimeRule(10, 71))
        with pytest.raises(ValueError, match="history"):
            make(time=(10, None, 1))
        with pytest.raises(ValueError, match="indexed by push"):
            make(time=TimeRule(10), score=ScoreSpec())
    # the push's own checks come ahead of any device work: a predictor that never saw a device
    fp = FramePredictor.__new__(FramePredictor)
    fp.time, fp.m_max = TimeRule(10).checked(8), 4
    with pytest.raises(ValueError, match="needs the push's time"):
        fp._stage([1], [[0.0, 0.0]], None)
    for bad in (1.0, True, "3", 1 << 62):
        with pytest.raises(ValueError, match="integer number of ticks"):
            fp._stage([1], [[0.0, 0.0]], None, t=bad)
    fp.time = None
    with pytest.raises(ValueError, match="made with time="):
        fp._stage([1], [[0.0, 0.0]], None, t=5)
    sp = StreamsPredictor.__new__(StreamsPredictor)
    sp.time, sp.ns, sp.m_max, sp.cap = TimeRule(10).checked(8), 3, 4, 12
    tick = {0: ([1], [[0.0, 0.0]]), 2: ([1], [[0.0, 0.0]])}
    with pytest.raises(ValueError, match="needs the streams' push times"):
        sp._stage(tick, None)
    with pytest.raises(ValueError, match="stream 2 is pushed without a time"):
        sp._stage(tick, None, times={0: 5})
    with pytest.raises(ValueError, match="stream 2 is pushed without a time"):
        sp._stage(tick, None, times=[5, 6, None])
    with pytest.raises(ValueError, match="2 entries for 3 streams"):
        sp._stage(tick, None, times=[5, 6])
    with pytest.raises(ValueError, match="stream index 3"):
        sp._stage(tick, None, times={0: 5, 2: 5, 3: 1})
    with pytest.raises(ValueError, match="integer number of ticks"):
        sp._stage(tick, None, times={0: 5, 2: 0.5})
    assert sp._host_times({0: 5, 2: -7}, [1, 0, 1]).tolist() == [5, 0, -7]
    sp.time = None
    with pytest.raises(ValueError, match="made with time="):
        sp._stage(tick, None, times=[1, 2, 3])


def test_timed_entry_points_refuse_before_any_launch():
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    f = ctypes.c_void_p(64)

    def one(m_max=8, s=16, r=8, t=8, v=4, step=10, max_dt=10, ms=2, mg=2, det_time=f, clock=f, seen=f):
        return L.stg_track_push_timed(f, f, f, det_time, m_max, f, f, f, f, clock, f, s, r, t, 1e4, v, step, max_dt, ms,
                                      mg, f, f, f, seen, None)

    def many(ns=2, m_total=8, id_stride=1, xy_stride=2, block=0, det_time=f, **kw):
        a = dict(m_max=8, s=16, r=8, t=8, v=4, step=10, max_dt=10, ms=2, mg=2)
        a.update(kw)
        return L.stg_track_push_streams_timed(f, id_stride, f, xy_stride, m_total, f, f, det_time, ns, a["m_max"], f, f,
                                              f, f, f, f, a["s"], a["r"], a["t"], 1e4, a["v"], a["step"], a["max_dt"],
                                              a["ms"], a["mg"], f, f, f, f, f, block, None)
    einval = {"R=1": dict(r=1), "R=0": dict(r=0), "step=0": dict(step=0), "step<0": dict(step=-10),
              "max_dt=0": dict(max_dt=0), "max_dt=71": dict(max_dt=71), "M_max=0": dict(m_max=0),
              "M_max": dict(m_max=2049), "S": dict(s=2049), "V=0": dict(v=0), "T_obs=1": dict(t=1, max_dt=1),
              "T_obs=33": dict(t=33), "min_seen": dict(ms=9), "max_gap": dict(mg=7)}
    for call, name in ((one, b"stg_track_push_timed"), (many, b"stg_track_push_streams_timed")):
        for what, kw in einval.items():
            assert call(**kw) == -1, (name, what)
            assert name + b":" in L.stg_last_error(), (name, what)
        assert call(det_time=None) == -1 and b"null" in L.stg_last_error()
        for what, kw in {"R=257": dict(r=257), "step": dict(step=1 << 28, max_dt=1 << 28),
                         "step 2^40": dict(step=1 << 40, max_dt=5)}.items():
            assert call(**kw) == _lib.EUNSUPPORTED, (name, what)
    assert one(clock=None) == -1 and one(seen=None) == -1
    for what, kw in {"NS=0": dict(ns=0), "NS": dict(ns=4097), "M_total<0": dict(m_total=-1),
                     "id_stride=0": dict(id_stride=0), "xy_stride=1": dict(xy_stride=1)}.items():
        assert many(**kw) == -1, what
    assert many(block=128) == -1 and b"block_threads" in L.stg_last_error()
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stgcnn_hip.h")).read()
    assert "#define STG_TRACK_MAX_HISTORY 256" in hdr and "#define STG_TRACK_TIME_ORDER 16" in hdr
    for name in ("stg_track_push_timed", "stg_track_push_streams_timed"):
        assert name in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
