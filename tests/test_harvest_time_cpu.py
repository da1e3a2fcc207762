"""No GPU: the timed window harvest (csrc/harvest_time.hip) -- its numpy statement (harvest_time_np)
against the untimed statement on whole recordings, hand-worked cases with every value written out, the preconditions of
the feeds the GPU tests use, the spec and the refusals, and the new header against its binding.  Everything is compared
bit for bit: the rule is integer work plus float64 operations in a written order."""
import ctypes
import os
import re

import numpy as np
import pytest

import harvest_np as H
import harvest_time_np as HT
from frames_time_np import OVERFLOW, TIME_ORDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
# recording -> (windows, rows) of data.load_windows(min_ped=1): the counts of DESIGN.md 5.26
RECORDINGS = {"eth_test/biwi_eth.txt": (70, 181), "zara1_test/crowds_zara01.txt": (602, 2253),
              "hotel_test/biwi_hotel.txt": (301, 1053)}


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _recording(rec):
    from social_stgcnn_amd import data
    return data.read_file(os.path.join(DATA, rec))


# ---- 1. one push per step is the untimed harvest ------------------------------------------------------------------------
@pytest.mark.parametrize("rec", sorted(RECORDINGS))
def test_one_push_per_step_is_the_untimed_harvest(rec):
    """t = 10 * (frame index), step = max_dt = 10, settle = 0: windows, rows and tags of harvest_np.harvest_recording bit
    for bit, at the same push; nothing skipped.  With settle = 9 the same windows, each one push later, and the last
    frame's window is absent."""
    rows = _recording(rec)
    ref = H.harvest_recording(rows)
    assert tuple(ref.header) == RECORDINGS[rec] + (0,)
    hv, headers = HT.feed_recording(rows)
    assert tuple(hv.log.header) == RECORDINGS[rec] + (0,)
    assert hv.log.seq_rel.tobytes() == ref.seq_rel.tobytes()
    assert np.array_equal(hv.log.win_start, ref.win_start) and np.array_equal(hv.log.tags, ref.tags)
    assert hv.hist[0].clock == [1, 0, 0] and hv.hist[0].j == len(headers) and hv.hist[0].interpolated == 0
    # ... at the same push: the untimed log grows where the window's tag says
    grown = [f for f in range(len(headers)) if headers[f][0] > (headers[f - 1][0] if f else 0)]
    assert grown == ref.tags[:, 1].tolist()
    late, late_headers = HT.feed_recording(rows, settle=9)
    assert late_headers[1:] == headers[:-1] and late_headers[0] == (0, 0, 0)
    n = late_headers[-1][0]
    assert n == headers[-2][0] and np.array_equal(late.log.tags, ref.tags[:n])
    assert late.log.seq_rel.tobytes() == ref.seq_rel[:late_headers[-1][1]].tobytes()
    assert late.hist[0].j == len(headers) - 1


# ---- 2. hand-worked cases -----------------------------------------------------------------------------------------------
def _run(script, settle, max_dt=10, history=8, min_peds=1, caps=(16, 64), reset_before=()):
    """script [(t, {id: x})] (y = 0) with obs_len 3, pred_len 1 (T_all = 4), step 10 -> (the harvester, after every push
    (header, [row, j], [anchored, g0, skipped]), the flags)."""
    track = HT.StreamModelTimed(3, 10, max_dt, history, capacity=4)
    hv = HT.TimedHarvester(1, 4, 10, max_dt, settle, *caps, min_peds)
    trace, flags = [], []
    for n, (t, det) in enumerate(script):
        if n in reset_before:
            track.reset()
            hv.reset()
        fl = track.push(list(det), [(x, 0.0) for x in det.values()], t)[3]
        flags.append(fl)
        hv.tick({0: (track.state()[0], t, not fl & TIME_ORDER)})
        trace.append((tuple(int(x) for x in hv.log.header), list(hv.hist[0].head), list(hv.hist[0].clock)))
    return hv, trace, flags


def _x(hv, w=None):
    """the x rows of the log (or of window w) as a list of lists"""
    rows = hv.log.seq_rel if w is None else hv.log.seq_rel[hv.log.win_start[w]:hv.log.win_start[w + 1]]
    assert not rows[:, 1].any()
    return rows[:, 0].tolist()


def test_exact_samples():
    hv, trace, _ = _run([(100, {1: 0.0}), (110, {1: 1.0}), (120, {1: 2.5}), (130, {1: 3.0}), (140, {1: 5.0})], 0)
    assert [h for h, _, _ in trace] == [(0, 0, 0)] * 3 + [(1, 1, 0), (2, 2, 0)]
    assert [hd for _, hd, _ in trace] == [[1, 1], [2, 2], [3, 3], [0, 4], [1, 5]]
    assert all(c == [1, 100, 0] for _, _, c in trace)
    assert _x(hv) == [[0.0, 1.0, 1.5, 0.5], [0.0, 1.5, 0.5, 2.0]] and hv.log.tags.tolist() == [[0, 3], [0, 4]]
    assert hv.hist[0].interpolated == 0


def test_an_interpolated_frame():
    """g = 10 lies between the samples at 7 and 14 (7 <= max_dt apart): 0.7 + (2.1 - 0.7) * (3 / 7) = 1.3 after the
    rounding to four decimals.  It is resolved by the push at 14, the first at or after it."""
    hv, trace, _ = _run([(0, {1: 0.0}), (7, {1: 0.7}), (14, {1: 2.1}), (20, {1: 2.0}), (30, {1: 3.0})], 0)
    assert [hd for _, hd, _ in trace] == [[1, 1], [1, 1], [2, 2], [3, 3], [0, 4]]
    assert hv.hist[0].runs[1][1].tolist() == [1.3, 0.0]
    assert _x(hv) == [[0.0, float(np.float32(1.3)), float(np.float32(2.0 - 1.3)), 1.0]]
    assert hv.log.tags.tolist() == [[0, 3]] and hv.hist[0].interpolated == 1


def test_a_bracket_wider_than_max_dt_is_a_gap():
    """18 and 29 are 11 apart: the frame at 20 is a gap, and the next window is the one of the frames 30 .. 60."""
    script = [(0, {1: 0.0}), (10, {1: 1.0}), (18, {1: 1.8}), (29, {1: 2.9}), (30, {1: 3.0}), (40, {1: 4.0}), (50, {1: 5.0}),
              (60, {1: 6.0}), (70, {1: 7.5})]
    hv, trace, _ = _run(script, 0)
    assert [h[0] for h, _, _ in trace] == [0, 0, 0, 0, 0, 0, 0, 1, 2]
    assert hv.log.tags.tolist() == [[0, 6], [0, 7]] and _x(hv) == [[0.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.5]]
    hv, _, _ = _run(script, 0, max_dt=11)                     # ... and a frame under max_dt = 11
    assert hv.log.tags[:, 1].tolist() == [3, 4, 5, 6, 7]
    assert _x(hv, 0) == [[0.0, 1.0, 1.0, 1.0]]


def test_settle_waits_for_the_sample_behind_the_instant():
    """Pedestrian 2 is missed in the push at 20, which resolves g = 20 under settle = 0: its run ends there.  Under settle
    = 9 the instant is resolved by the push at 30 (25 - 9 < 20), when 15 and 25 bracket it: (1.5 + 2.5) / 2 = 2.0."""
    script = [(t, {1: t / 10.0, 2: t / 10.0} if t != 20 else {1: 2.0}) for t in range(0, 75, 5)]
    now, trace0, _ = _run(script, 0)
    late, trace9, _ = _run(script, 9)
    # K = 0 at the pushes between two instants: nothing moves
    assert [hd[1] for _, hd, _ in trace0] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8]
    assert [hd[1] for _, hd, _ in trace9] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7]
    assert trace0[3] == trace0[2] and trace9[3] == trace9[2]
    assert now.log.tags[:, 1].tolist() == [3, 4, 5, 6, 7] and now.log.num_peds.tolist() == [1, 1, 1, 2, 2]
    assert late.log.tags[:, 1].tolist() == [3, 4, 5, 6] and late.log.num_peds.tolist() == [2, 2, 2, 2]
    assert _x(late, 0) == [[0.0, 1.0, 1.0, 1.0]] * 2 and late.hist[0].interpolated > 0


def test_a_push_two_instants_late_skips_one_and_clears_the_words():
    """Pushes at 0, 10, 20, 40: the last one finds 30 and 40 pending, skips 30 and resolves 40.  The frames 10, 20, 40,
    50 are no window: the first one is 40 .. 70, tag 7."""
    script = [(0, {1: 0.0}), (10, {1: 1.0}), (20, {1: 2.0}), (40, {1: 4.0}), (50, {1: 5.0}), (60, {1: 6.0}), (70, {1: 7.0}),
              (80, {1: 8.5})]
    hv, trace, _ = _run(script, 0)
    assert [hd for _, hd, _ in trace] == [[1, 1], [2, 2], [3, 3], [0, 5], [1, 6], [2, 7], [3, 8], [0, 9]]
    assert [c[2] for _, _, c in trace] == [0, 0, 0, 1, 1, 1, 1, 1]
    assert len(hv.hist[0].runs[1]) == 4 and [h[0] for h, _, _ in trace] == [0, 0, 0, 0, 0, 0, 1, 2]
    assert hv.log.tags.tolist() == [[0, 7], [0, 8]] and _x(hv) == [[0.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.5]]


def test_a_refused_push_changes_nothing():
    script = [(0, {1: 0.0}), (10, {1: 1.0}), (20, {1: 2.0}), (15, {1: 9.0}), (20, {1: 9.0}), (30, {1: 3.0})]
    hv, trace, flags = _run(script, 0)
    assert [f & TIME_ORDER for f in flags] == [0, 0, 0, TIME_ORDER, TIME_ORDER, 0]
    assert trace[2] == trace[3] == trace[4]
    assert hv.log.tags.tolist() == [[0, 3]] and _x(hv) == [[0.0, 1.0, 1.0, 1.0]]


def test_a_ring_of_two_loses_the_sample_before_the_instant():
    """settle = 9: g = 10 is resolved by the push at 19, when a ring of two holds 16 and 19 only -- the frame is a gap,
    never a wrong position; a ring of eight still holds 8 and 12."""
    script = [(0, {1: 0.0}), (4, {1: 0.4}), (8, {1: 0.8}), (12, {1: 1.2}), (16, {1: 1.6}), (19, {1: 1.9}), (20, {1: 2.0}),
              (29, {1: 2.9}), (30, {1: 3.0}), (39, {1: 3.9})]
    deep, _, _ = _run(script, 9, history=8)
    assert deep.log.tags.tolist() == [[0, 3]] and _x(deep) == [[0.0, 1.0, 1.0, 1.0]]
    shallow, trace, _ = _run(script, 9, history=2)
    assert tuple(shallow.log.header) == (0, 0, 0) and trace[-1][1:] == ([0, 4], [1, 0, 0])
    assert len(shallow.hist[0].runs[1]) == 2                                 # the frames 20 and 30 alone


def test_the_log_full_by_windows_and_by_rows():
    script = [(10 * f, {1: float(f), 2: 2.0 * f}) for f in range(9)]
    hv, trace, _ = _run(script, 0, caps=(2, 64))
    assert [h for h, _, _ in trace][3:] == [(1, 2, 0), (2, 4, 0), (2, 4, 1), (2, 4, 2), (2, 4, 3), (2, 4, 4)]
    assert hv.log.tags.tolist() == [[0, 3], [0, 4]]
    hv, trace, _ = _run(script, 0, caps=(16, 5))
    assert [h for h, _, _ in trace][3:] == [(1, 2, 0), (2, 4, 0), (2, 4, 1), (2, 4, 2), (2, 4, 3), (2, 4, 4)]
    assert _x(hv) == [[0.0, 1.0, 1.0, 1.0], [0.0, 2.0, 2.0, 2.0]] * 2
    hv.log.clear()
    assert tuple(hv.log.header) == (0, 0, 0)


def test_a_reset_starts_the_grid_again():
    script = [(10 * f, {1: float(f)}) for f in range(5)] + [(57 + 10 * f, {1: float(f)}) for f in range(5)]
    hv, trace, _ = _run(script, 0, reset_before=(5,))
    assert [c for _, _, c in trace][4:6] == [[1, 0, 0], [1, 57, 0]]
    assert [hd for _, hd, _ in trace][4:] == [[1, 5], [1, 1], [2, 2], [3, 3], [0, 4], [1, 5]]
    assert hv.log.tags.tolist() == [[0, 3], [0, 4], [0, 3], [0, 4]]          # the log is left alone


# ---- 3. the feeds of the GPU tests: what they have to reach ---------------------------------------------------------------
def _windows(hv):
    return [(tuple(hv.log.win_tag[w]), hv.log.seq_rel[hv.log.win_start[w]:hv.log.win_start[w + 1]].tobytes())
            for w in range(int(hv.log.header[0]))]


@pytest.mark.parametrize("t_obs,t_all,pushes", [(3, 5, 70), (8, 20, 150)])
@pytest.mark.parametrize("max_dt", [10, 13])
def test_the_scripted_feed_reaches_what_the_gpu_test_needs(t_obs, t_all, pushes, max_dt):
    """With a ring of 64: at least 8 windows under both settings, interpolated frames inside windows, skip events, a
    refused push, slots running out, windows from all three streams, and windows that differ between settle = 0 and
    settle = max_dt - 1.  A ring of 4 is too shallow for settle = max_dt - 1: it loses windows, and only there."""
    feed = HT.scripted_feed(t_obs, t_all, pushes, 5)
    runs = {}
    for settle in (0, max_dt - 1):
        hv, flags = HT.run_scripted(feed, t_obs, t_all, max_dt, settle, 64)
        assert flags & OVERFLOW and flags & TIME_ORDER
        assert int(hv.log.header[0]) >= 8 and int(hv.log.header[2]) == 0
        assert set(hv.log.tags[:, 0].tolist()) == {0, 1, 2}
        assert all(h.interpolated > 0 and h.skipped >= 1 for h in hv.hist)
        assert [h.g0 for h in hv.hist] == list(HT.CLOCK0)
        runs[settle] = hv
    assert set(_windows(runs[0])) != set(_windows(runs[max_dt - 1]))
    shallow0, _ = HT.run_scripted(feed, t_obs, t_all, max_dt, 0, 4)
    assert _windows(shallow0) == _windows(runs[0])
    shallow, _ = HT.run_scripted(feed, t_obs, t_all, max_dt, max_dt - 1, 4)
    assert int(shallow.log.header[0]) < int(runs[max_dt - 1].log.header[0])


def test_the_wide_feed_reaches_what_the_gpu_test_needs():
    """272 slots, more than a harvest workgroup has threads: three windows of 263 rows of stream 0, each with rows past
    slot 255 that hold interpolated frames, beside a live slot that is no candidate and a free one past 255; three
    windows of stream 1 without an interpolated frame."""
    hv, facts = HT.wide_run(HT.wide_feed())
    assert HT.wide_reached(hv, facts) and not HT.wide_reached(hv, [(False,) * 3] * len(facts))
    assert hv.log.tags.tolist() == [[1, 4], [0, 4], [0, 5], [1, 5], [1, 6], [0, 6]]
    assert hv.log.num_peds.tolist() == [5, 263, 263, 5, 5, 263]
    assert hv.hist[0].interpolated == 263 * (2 + 2 + 3) and hv.hist[1].interpolated == 0
    assert [h.clock for h in hv.hist] == [[1, 0, 0], [1, HT.CLOCK0[1], 0]]


def _frames60(d, f):
    from live_inputs import _pushes, _rows
    return _pushes(_rows(d, f))[:60]


def test_the_recording_feeds_reach_what_the_gpu_tests_need(tmp_path):
    """crowds_zara01's first 60 frames upsampled 4x and started in between: at least 8 windows under both settings,
    interpolated frames inside them, one skip, and windows that differ between the settings.  biwi_eth's first 60 frames,
    the feed whose windows the GPU test holds against load_windows, are sparse: 2 windows (5 of single pedestrians); its
    in-between feed still interpolates and skips."""
    dense = {}
    for settle in (0, 3):
        hv, _ = HT.feed(*HT.eth_feed(_frames60("zara1_test", "crowds_zara01.txt"), 2), step=4, max_dt=4, settle=settle)
        assert int(hv.log.header[0]) >= 8 and hv.hist[0].interpolated > 0 and hv.hist[0].clock[:2] == [1, 2] and hv.hist[0].skipped >= 1
        dense[settle] = hv
    assert set(_windows(dense[0])) != set(_windows(dense[3]))
    frames = _frames60("eth_test", "biwi_eth.txt")
    on_grid, _ = HT.feed(*HT.eth_feed(frames, 0), step=4, max_dt=4, settle=0)
    assert tuple(on_grid.log.header) == (2, 4, 0) and on_grid.log.tags[:, 1].tolist() == [24, 46]
    between, _ = HT.feed(*HT.eth_feed(frames, 2), step=4, max_dt=4, settle=3, min_peds=1)
    assert int(between.log.header[0]) >= 3 and between.hist[0].interpolated > 0 and between.hist[0].clock[:2] == [1, 2] and between.hist[0].skipped >= 1


def test_upsampled_frames_on_the_grid_are_the_frames():
    """Four pushes per step with the frames on the grid, settle = 0: the windows of the frames pushed one per step."""
    from live_inputs import _pushes, _rows
    frames = _pushes(_rows("zara1_test", "crowds_zara01.txt"))[:60]
    ref, _ = HT.feed(frames, [10 * f for f in range(60)])
    hv, _ = HT.feed(*HT.eth_feed(frames, 0), step=4, max_dt=4, settle=0)
    assert _windows(hv) == _windows(ref) and int(hv.log.header[0]) == 41 and hv.hist[0].interpolated == 0


# ---- 4. the spec and the refusals ---------------------------------------------------------------------------------------
def test_timed_harvest_spec_checks():
    from social_stgcnn_amd.frames import TimedHarvestSpec
    s = TimedHarvestSpec(100)
    assert s == (100, None, 2, None, None) and s.checked(8, 128, 12, 10) == (100, 12800, 2, 12, 9)
    assert TimedHarvestSpec(5, 7, 1, 2, 0).checked(3, 4, 12, 13) == (5, 7, 1, 2, 0)
    assert TimedHarvestSpec(5, settle=12).checked(3, 4, 2, 13).settle == 12
    for bad in (dict(windows=0), dict(windows=1.5), dict(windows=True), dict(windows=4, rows=0),
                dict(windows=4, min_peds=0), dict(windows=4, pred_len=0), dict(windows=4, pred_len=32),
                dict(windows=4, settle=-1), dict(windows=4, settle=1.5), dict(windows=4, settle=True)):
        with pytest.raises(ValueError, match="TimedHarvestSpec"):
            TimedHarvestSpec(**bad)
    with pytest.raises(ValueError, match="TimedHarvestSpec: settle=13 > max_dt - 1 = 12"):
        TimedHarvestSpec(4, settle=13).checked(8, 128, 12, 13)
    with pytest.raises(ValueError, match="TimedHarvestSpec.*within 32 steps"):
        TimedHarvestSpec(4).checked(8, 128, 25, 10)
    with pytest.raises(ValueError, match="TimedHarvestSpec.*obs_len=1"):
        TimedHarvestSpec(4).checked(1, 128, 12, 10)


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_both_refusals_of_the_predictors():
    """Ahead of anything that needs the device: the timed spec without time=, the untimed spec with it (word for word
    what it was), a settle the TimeRule does not allow, and associate= with time=."""
    from social_stgcnn_amd.frames import (AssociateSpec, FramePredictor, HarvestSpec, StreamsPredictor, TimedHarvestSpec,
                                          TimeRule)
    for make in (lambda **kw: FramePredictor(_Model(), **kw), lambda **kw: StreamsPredictor(_Model(), 3, **kw)):
        with pytest.raises(ValueError, match=r"harvest=TimedHarvestSpec\(\.\.\.\) needs time=TimeRule"):
            make(harvest=TimedHarvestSpec(10))
        with pytest.raises(ValueError) as e:
            make(harvest=HarvestSpec(10), time=TimeRule(10))
        assert str(e.value) == ("harvest= together with time= is not supported: a timed push is not one frame of a window "
                                "(DESIGN.md 8)")
        with pytest.raises(ValueError, match="harvest= together with time="):
            make(harvest=(10,), time=TimeRule(10))
        with pytest.raises(ValueError, match="settle=10 > max_dt - 1 = 9"):
            make(harvest=TimedHarvestSpec(10, settle=10), time=TimeRule(10))
        with pytest.raises(ValueError, match="associate= together with time="):
            make(harvest=TimedHarvestSpec(10), time=TimeRule(10), associate=AssociateSpec(0.5))


def test_predict_frames_refusals():
    from social_stgcnn_amd import predict_frames as pf
    base = ["--checkpoint", "c", "--recording", "r", "--out", "o.npz"]
    for extra, msg in ((["--harvest_timed", "10"], "--harvest_timed needs --step"),
                       (["--harvest_timed", "10", "--step", "10", "--harvest", "10"], "--harvest_timed does not go together "
                                                                                       "with --harvest"),
                       (["--harvest", "10", "--step", "10"], "--harvest does not go together with --step"),
                       (["--settle", "3", "--step", "10"], "--settle needs --harvest_timed"),
                       (["--harvest_timed", "10", "--step", "10", "--settle", "10"], "--settle: 10 not in"),
                       (["--harvest_timed", "10", "--step", "10", "--max_dt", "13", "--settle", "13"], "--settle: 13 not in"),
                       (["--harvest_timed", "10", "--step", "10", "--settle", "-1"], "--settle: -1 not in"),
                       (["--harvest_timed", "10", "--step", "10", "--associate", "0.5"], "--associate"),
                       (["--harvest_timed", "0", "--step", "10"], "at least one window"),
                       (["--harvest_out", "w.npz", "--step", "10"], "needs --harvest")):
        with pytest.raises(ValueError, match=msg):
            pf.main(base + extra)


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------
def test_the_timed_harvest_header_its_binding_and_the_exports(L):
    """include/stgcnn_hip_harvest_time.h -- which stgcnn_hip.h includes inside its extern "C" block, behind the untimed
    harvest's -- as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its two
    entry points by name, nothing but void *, int, int64_t and double among their parameters, ABI version 8."""
    from social_stgcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    inc = '#include "stgcnn_hip_harvest_time.h"'
    assert re.search("^" + re.escape(inc) + "$", main, re.M)
    assert main.index('extern "C" {') < main.index('#include "stgcnn_hip_harvest.h"') < main.index(inc) \
        < main.rindex("#ifdef __cplusplus")
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_harvest_time.h")).read()
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_window_harvest_timed", "stg_window_harvest_streams_timed"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}, p.name
        assert fn.restype == ctypes.c_int, p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    # the other two part-headers and the main header keep their prototypes
    for f, n in (("stgcnn_hip_harvest.h", 2), ("stgcnn_hip.h", 51)):
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
        text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
        assert len(re.findall(r"\b(stg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)) == n, f


PTRS = ("slot_id", "t_ring", "xy_ring", "slot_head", "clock", "head_flags", "h_word", "h_ring", "h_head", "h_clock",
        "rel_all", "win_start", "win_tag", "header")


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    f = ctypes.c_void_p(64)

    def one(s=16, r=8, t_obs=8, t_all=20, min_peds=2, step=10, max_dt=10, settle=9, tag=0, cap_w=4, cap_r=16, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_window_harvest_timed(*(p[n] for n in PTRS[:6]), s, r, t_obs, t_all, min_peds, 1e4, step, max_dt,
                                          settle, tag, *(p[n] for n in PTRS[6:]), cap_w, cap_r, None)

    def many(ns=3, s=16, r=8, t_obs=8, t_all=20, min_peds=2, step=10, max_dt=10, settle=9, cap_w=4, cap_r=16, pushed=f,
             work=f, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_window_harvest_streams_timed(*(p[n] for n in PTRS[:6]), pushed, ns, s, r, t_obs, t_all, min_peds, 1e4,
                                                  step, max_dt, settle, *(p[n] for n in PTRS[6:10]), work,
                                                  *(p[n] for n in PTRS[10:]), cap_w, cap_r, None)
    einval = {"S=0": dict(s=0), "S=2049": dict(s=2049), "T_obs=0": dict(t_obs=0), "T_all=1": dict(t_obs=1, t_all=1),
              "T_all=33": dict(t_all=33), "pred_len=0": dict(t_obs=8, t_all=8), "min_peds=0": dict(min_peds=0),
              "cap_windows=0": dict(cap_w=0), "cap_rows=0": dict(cap_r=0), "R=1": dict(r=1), "step=0": dict(step=0),
              "max_dt=0": dict(max_dt=0, settle=0), "max_dt=71": dict(max_dt=71), "T_obs=1": dict(t_obs=1, t_all=3),
              "settle=-1": dict(settle=-1), "settle=max_dt": dict(settle=10),
              **{"null " + n: {n: True} for n in PTRS}}
    unsupported = {"R=257": dict(r=257), "step * T_obs = 2^31": dict(step=1 << 28, max_dt=10)}
    for name, kw in einval.items():
        assert one(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_window_harvest_timed:"), name
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_window_harvest_streams_timed:"), name
    for name, kw in unsupported.items():
        assert one(**kw) == -2 and many(**kw) == -2, name
    assert one(tag=-1) == -1 and L.stg_last_error().startswith(b"stg_window_harvest_timed:")
    for name, kw in {"NS=0": dict(ns=0), "NS=4097": dict(ns=4097), "null pushed": dict(pushed=None),
                     "null work": dict(work=None)}.items():
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_window_harvest_streams_timed:"), name
