"""CPU: the window harvest -- its numpy restatement against data.load_windows on the five test
recordings, hand-worked cases of the rule and the log, HarvestSpec and the refusals of the predictors and of
predict_frames, the C ABI's declarations, binding and refusals before any launch, DeviceWindows.from_device's checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import harvest_np as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
# recording -> (windows, rows, largest crowd) of data.load_windows(min_ped=1)
RECORDINGS = {"eth_test/biwi_eth.txt": (70, 181, 5), "hotel_test/biwi_hotel.txt": (301, 1053, 8),
              "zara1_test/crowds_zara01.txt": (602, 2253, 14), "univ_test/students001.txt": (425, 14295, 57),
              "zara2_test/crowds_zara02.txt": (921, 5833, 14)}


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. the restatement against the reference's windowing -------------------------------------------------------------
@pytest.mark.parametrize("rec", sorted(RECORDINGS))
def test_restatement_equals_load_windows(rec):
    """Pushed frame by frame, the recording's harvested windows are data.load_windows' windows: the same counts in the
    same order and seq_rel after the float32 cast bit for bit."""
    from social_stgcnn_amd import data
    d, f = os.path.split(os.path.join(DATA, rec))
    ref = data.load_windows(d, files=[f], with_non_linear=False)
    log = H.harvest_recording(data.read_file(os.path.join(d, f)))
    n_w, n_r, v = RECORDINGS[rec]
    assert (len(ref), len(ref.seq_rel), int(ref.num_peds.max())) == (n_w, n_r, v)
    assert tuple(log.header) == (n_w, n_r, 0)
    assert np.array_equal(log.num_peds, ref.num_peds)
    assert log.seq_rel.tobytes() == ref.seq_rel.astype(np.float32).tobytes()
    assert np.array_equal(log.tags[:, 0], np.zeros(n_w)) and np.all(np.diff(log.tags[:, 1]) > 0)


# ---- 2. hand-worked cases ---------------------------------------------------------------------------------------------
def _walk(n, x0=0.0, step=0.25):
    """n positions on a line: exactly representable, so every difference is exact"""
    return np.stack([x0 + step * np.arange(n), np.full(n, 1.5)], axis=1)


def _feed(script, t_obs, t_all, min_peds=2, capacity=8, cap_windows=16, cap_rows=64):
    """script: one {id: (x, y)} per push -> the Harvester after the last push"""
    track = H.TrackModel(t_obs, capacity)
    hv = H.Harvester(1, capacity, t_all, cap_windows, cap_rows, min_peds)
    for det in script:
        track.push(list(det), [det[i] for i in det])
        hv.tick({0: track.state()})
    return hv


@pytest.mark.parametrize("pushes, windows", [(19, 0), (20, 1), (21, 2)])
def test_a_track_of_19_20_21_pushes(pushes, windows):
    a, b = _walk(pushes), _walk(pushes, 5.0, -0.5)
    log = _feed([{3: a[n], 9: b[n]} for n in range(pushes)], 8, 20).log
    assert tuple(log.header) == (windows, 2 * windows, 0)
    for w in range(windows):
        rel = log.seq_rel[2 * w:2 * w + 2]
        assert np.array_equal(rel[:, :, 0], np.zeros((2, 2)))
        assert np.array_equal(rel[0, 0, 1:], np.full(19, 0.25, np.float32))
        assert np.array_equal(rel[1, 0, 1:], np.full(19, -0.5, np.float32))
        assert np.array_equal(rel[:, 1, 1:], np.zeros((2, 19), np.float32))
        assert tuple(log.tags[w]) == (0, 19 + w)


def test_one_missed_push_in_the_middle():
    """Pedestrian 9 misses push 12 of 45: its first window ends 20 pushes after the gap, at push 32; 3 and 5 alone make
    the windows in between."""
    n = 45
    a, b, c = _walk(n), _walk(n, 2.0), _walk(n, 7.0, 0.125)
    script = [{3: a[i], 5: b[i], **({} if i == 12 else {9: c[i]})} for i in range(n)]
    log = _feed(script, 8, 20, cap_windows=64, cap_rows=256).log
    by_push = dict(zip(log.tags[:, 1].tolist(), log.num_peds.tolist()))
    assert sorted(by_push) == list(range(19, n))
    assert all(by_push[p] == (3 if p >= 32 else 2) for p in by_push)
    last = log.seq_rel[-3:]
    assert np.array_equal(last[2, 0, 1:], np.full(19, 0.125, np.float32))


def test_a_window_of_one_pedestrian_is_dropped_by_min_peds():
    a = _walk(25)
    assert tuple(_feed([{4: a[i]} for i in range(25)], 8, 20).log.header) == (0, 0, 0)
    one = _feed([{4: a[i]} for i in range(25)], 8, 20, min_peds=1).log
    assert tuple(one.header) == (6, 6, 0) and one.tags[:, 1].tolist() == list(range(19, 25))


def test_the_log_full_by_windows_and_by_rows():
    n = 30
    a, b, c = _walk(n), _walk(n, 2.0), _walk(n, 4.0)
    two = [{1: a[i], 2: b[i]} for i in range(n)]
    by_windows = _feed(two, 8, 20, cap_windows=3, cap_rows=64).log
    assert tuple(by_windows.header) == (3, 6, 8) and by_windows.win_start.tolist() == [0, 2, 4, 6]
    by_rows = _feed(two, 8, 20, cap_windows=16, cap_rows=5).log
    assert tuple(by_rows.header) == (2, 4, 9)
    # the first drop closes the log: pedestrian 3 leaves at push 22, and the smaller windows that follow would fit the
    # rows left, but are dropped like the one before them
    three = [{1: a[i], 2: b[i], **({3: c[i]} if i < 22 else {})} for i in range(n)]
    closed = _feed(three, 8, 20, cap_windows=16, cap_rows=8).log
    assert tuple(closed.header) == (2, 6, 9)
    closed.clear()
    assert tuple(closed.header) == (0, 0, 0)


def test_windows_of_five_steps():
    """T_all = 5 (obs_len 3 + pred_len 2), ids in descending detection order, one stream of two not pushed on odd ticks,
    a reset in the middle."""
    n = 12
    a, b = _walk(n), _walk(n, 9.0, -1.0)
    tracks = [H.TrackModel(3, 4), H.TrackModel(3, 4)]
    hv = H.Harvester(2, 4, 5, 32, 64)
    for i in range(n):
        states = {}
        for s in (0, 1):
            if s == 1 and i % 2:
                continue
            tracks[s].push([7, -2 if s else 2], [b[i], a[i]])
            states[s] = tracks[s].state()
        if i == 8:
            hv.reset([0])
        hv.tick(states)
    log = hv.log
    # stream 0: windows at its pushes 4..7, then (reset ahead of push 8) at 4..; the negative id of stream 1 never counts
    assert [tuple(t) for t in log.tags if t[0] == 0] == [(0, 4), (0, 5), (0, 6), (0, 7)]
    assert not (log.tags[:, 0] == 1).any()
    assert np.array_equal(log.seq_rel[0], np.array([[0, .25, .25, .25, .25], [0, 0, 0, 0, 0]], np.float32))
    assert np.array_equal(log.seq_rel[1, 0], np.array([0, -1, -1, -1, -1], np.float32))


def test_slot_reuse_and_overflow_never_join_two_pedestrians():
    """capacity 2: a third id finds no slot (OVERFLOW) until one is freed after T_obs - 1 missed pushes, and a slot's new
    pedestrian starts with an empty history."""
    n = 40
    a, b, c = _walk(n), _walk(n, 2.0), _walk(n, 4.0, 0.5)
    track, hv = H.TrackModel(3, 2), H.Harvester(1, 2, 5, 64, 128)
    flags = []
    for i in range(n):
        det = {1: a[i], 3: c[i]} if i >= 10 else {1: a[i], 2: b[i], 3: c[i]}
        flags.append(track.push(list(det), list(det.values())))
        hv.tick({0: track.state()})
    assert flags[:10] == [H.OVERFLOW] * 10 and flags[10:12] == [H.OVERFLOW] * 2 and not any(flags[12:])
    log = hv.log
    pushes = log.tags[:, 1].tolist()
    assert pushes == list(range(4, 10)) + list(range(16, n))          # 3 holds slot 1 from push 12: 5 pushes by 16
    second = log.seq_rel[2 * pushes.index(16) + 1]
    assert np.array_equal(second[0], np.array([0, .5, .5, .5, .5], np.float32))


def test_the_wide_feed_reaches_what_the_gpu_test_needs():
    """272 slots, more than a harvest workgroup has threads: windows from tick 4 on with rows past slot 255, a live slot
    that is no candidate and a free slot past 255, windows of both streams, nothing dropped."""
    ids, words, windows = [], [], []
    for _, states, hv, slots in H.wide_ticks(H.wide_script()):
        ids.append(states[0][0].copy())
        words.append(hv.hist[0].word.copy())
        windows.append(slots)
    assert H.wide_conditions(ids, words, hv.hist[0].full, windows)
    assert [w is not None for w in windows] == [False] * 4 + [True] * 3 and all(len(w) == 263 for w in windows[4:])
    assert hv.log.header.tolist() == [5, 3 * 263 + 2 * 5, 0] and hv.log.tags.tolist() == [[0, 4], [0, 5], [1, 4], [0, 6], [1, 5]]
    assert not H.wide_conditions(ids, words, hv.hist[0].full, [None] * 7)


# ---- 3. the spec and the refusals ---------------------------------------------------------------------------------------
def test_harvest_spec_checks():
    from social_stgcnn_amd.frames import HarvestSpec
    s = HarvestSpec(100)
    assert s == (100, None, 2, None) and s.checked(8, 128, 12) == (100, 12800, 2, 12)
    assert HarvestSpec(5, 7, 1, 2).checked(3, 4, 12) == (5, 7, 1, 2)
    for bad in (dict(windows=0), dict(windows=1.5), dict(windows=True), dict(windows=4, rows=0),
                dict(windows=4, min_peds=0), dict(windows=4, pred_len=0), dict(windows=4, pred_len=32)):
        with pytest.raises(ValueError, match="HarvestSpec"):
            HarvestSpec(**bad)
    with pytest.raises(ValueError, match="within 32 steps"):
        HarvestSpec(4).checked(8, 128, 25)
    with pytest.raises(ValueError, match="obs_len=1"):
        HarvestSpec(4).checked(1, 128, 12)
    with pytest.raises(ValueError, match="below 2\\^31"):
        HarvestSpec((1 << 31) - 2).checked(8, 128, 12)


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_harvest_with_time_is_refused():
    """Ahead of anything that needs the device."""
    from social_stgcnn_amd.frames import FramePredictor, HarvestSpec, StreamsPredictor, TimeRule
    with pytest.raises(ValueError, match="harvest= together with time="):
        FramePredictor(_Model(), harvest=HarvestSpec(10), time=TimeRule(10))
    with pytest.raises(ValueError, match="harvest= together with time="):
        StreamsPredictor(_Model(), 3, harvest=HarvestSpec(10), time=TimeRule(10))
    with pytest.raises(ValueError, match="HarvestSpec"):
        FramePredictor(_Model(), harvest=0)


def test_predict_frames_refusals():
    from social_stgcnn_amd import predict_frames as pf
    base = ["--checkpoint", "c", "--recording", "r", "--out", "o.npz"]
    for extra, msg in ((["--harvest", "10", "--step", "10"], "--step"),
                       (["--harvest", "10", "--associate", "0.5"], "--associate"),
                       (["--harvest", "10", "--radius", "0.2"], "--radius"),
                       (["--harvest", "0"], "at least one window"),
                       (["--harvest_out", "w.npz"], "needs --harvest")):
        with pytest.raises(ValueError, match=msg):
            pf.main(base + extra)


def test_from_device_argument_checks():
    from social_stgcnn_amd.dataset import DeviceWindows
    rel, start = torch.zeros((5, 2, 20)), torch.tensor([0, 2, 5], dtype=torch.int32)
    ok = dict(rel_all=rel, win_start=start, num_peds_host=np.array([2, 3]), obs_len=8)
    for name, kw in {"rel dtype": dict(rel_all=rel.double()), "rel shape": dict(rel_all=torch.zeros((5, 3, 20))),
                     "rel strided": dict(rel_all=torch.zeros((5, 2, 40))[:, :, ::2]),
                     "start dtype": dict(win_start=start.long()), "start shape": dict(win_start=start.reshape(1, 3)),
                     "peds length": dict(num_peds_host=np.array([5])), "peds sum": dict(num_peds_host=np.array([2, 2])),
                     "peds zero": dict(num_peds_host=np.array([5, 0])), "peds float": dict(num_peds_host=np.array([2., 3.])),
                     "obs_len 0": dict(obs_len=0), "obs_len T_all": dict(obs_len=20), "obs_len 2.5": dict(obs_len=2.5)}.items():
        with pytest.raises(ValueError, match="from_device"):
            DeviceWindows.from_device(**{**ok, **kw})
        print(name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # host tensors: refused, never read
        DeviceWindows.from_device(**ok)


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------
def test_the_harvest_header_its_binding_and_the_exports(L):
    """include/stgcnn_hip_harvest.h -- which stgcnn_hip.h includes inside its extern "C" block -- against
    as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its two entry points by
    name, nothing but void * and int among their parameters, ABI version 8, the limit."""
    from social_stgcnn_amd import _lib, frames
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r'^#include "stgcnn_hip_harvest.h"$', main, re.M)
    assert main.index('extern "C" {') < main.index('#include "stgcnn_hip_harvest.h"') < main.rindex("#ifdef __cplusplus")
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_harvest.h")).read()
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_window_harvest", "stg_window_harvest_streams"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int}, p.name
        assert fn.restype == ctypes.c_int, p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    assert re.search(r"#define STG_HARVEST_MAX_STEPS 32\b", raw_hdr) and frames.MAX_WINDOW_STEPS == 32


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    f = ctypes.c_void_p(64)

    def one(s=16, t_obs=8, t_all=20, min_peds=2, tag=0, cap_w=4, cap_r=16, **null):
        p = {n: None if n in null else f for n in ("slot_id", "mask", "ring", "head_flags", "h_word", "h_ring", "h_head",
                                                    "rel_all", "win_start", "win_tag", "header")}
        return L.stg_window_harvest(p["slot_id"], p["mask"], p["ring"], p["head_flags"], s, t_obs, t_all, min_peds, tag,
                                    p["h_word"], p["h_ring"], p["h_head"], p["rel_all"], p["win_start"], p["win_tag"],
                                    p["header"], cap_w, cap_r, None)

    def many(ns=3, s=16, t_obs=8, t_all=20, min_peds=2, cap_w=4, cap_r=16, pushed=f, work=f, header=f):
        return L.stg_window_harvest_streams(f, f, f, f, pushed, ns, s, t_obs, t_all, min_peds, f, f, f, work, f, f, f,
                                            header, cap_w, cap_r, None)
    cases = {"S=0": dict(s=0), "S=2049": dict(s=2049), "T_obs=0": dict(t_obs=0), "T_all=1": dict(t_obs=1, t_all=1),
             "T_all=33": dict(t_all=33), "pred_len=0": dict(t_obs=8, t_all=8), "min_peds=0": dict(min_peds=0),
             "cap_windows=0": dict(cap_w=0), "cap_rows=0": dict(cap_r=0), "tag<0": dict(tag=-1),
             **{"null " + n: {n: True} for n in ("slot_id", "mask", "ring", "head_flags", "h_word", "h_ring", "h_head",
                                                 "rel_all", "win_start", "win_tag", "header")}}
    for name, kw in cases.items():
        assert one(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_window_harvest:"), name
    for name, kw in {"NS=0": dict(ns=0), "NS=4097": dict(ns=4097), "S=0": dict(s=0), "T_all=33": dict(t_all=33),
                     "pred_len=0": dict(t_obs=20), "min_peds=0": dict(min_peds=0), "cap_rows=0": dict(cap_r=0),
                     "null pushed": dict(pushed=None), "null work": dict(work=None), "null header": dict(header=None)}.items():
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_window_harvest_streams:"), name
