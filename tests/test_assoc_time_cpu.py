"""CPU: the timed association rule restated (assoc_time_np) on hand-computed cases, its equivalence with the untimed
restatement on a feed of one push per step, the checks of frames.TimedAssociateSpec and both refusals of the live
predictors, the packing of timed ticks without ids, the header against the binding, the command's refusals, and the
identity quality the rule must keep on three committed recordings at four pushes per step."""
import ctypes
import os
import re

import numpy as np
import pytest

import assoc_np
import assoc_time_np as AT
from harvest_time_np import upsample
from live_inputs import _pushes, _rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECS = {"crowds_zara01": ("zara1_test", "crowds_zara01.txt"), "biwi_hotel": ("hotel_test", "biwi_hotel.txt"),
        "biwi_eth": ("eth_test", "biwi_eth.txt")}


@pytest.fixture(scope="module")
def frames_of():
    """The recordings as pushes [(recorded ids, xy)], read once."""
    return {name: _pushes(_rows(*rec)) for name, rec in RECS.items()}


# ---- 1. the restatement on hand-computed cases ---------------------------------------------------------------------------
def test_a_gap_of_two_and_a_half_steps():
    """step 4: a track matched at t = 0 and t = 4 moves 1.0 per step; at t = 14, 2.5 steps on, it predicts 1 + 1 * 2.5 =
    3.5, takes the detection at 3.9 (0.16 <= 1) and its velocity becomes (3.9 - 1) / 2.5 per step.  The gates do not grow
    with the gap: from 3.5 the detection at 4.6 (1.21 > 1) would be out of reach."""
    t = AT.TimedTracker(3, gate=1.0, gate_new=2.0, max_age=0, step=4)
    assert t.push([[0.0, 0.0]], 0).tolist() == [0]
    assert t.push([[1.0, 0.0]], 4).tolist() == [0] and t.trk_vel[0].tolist() == [1.0, 0.0]
    assert t.push([[3.9, 0.0]], 14).tolist() == [0]
    assert t.trk_vel[0].tolist() == [(3.9 - 1.0) / 2.5, 0.0] and t.trk_t.tolist() == [14, 0, 0]
    assert t.trk_hits.tolist() == [3, 0, 0] and t.clock == [14, 3]
    # one tick on, a quarter of a step: 3.9 + 1.16 * 0.25 = 4.19
    q = 3.9 + (3.9 - 1.0) / 2.5 * 0.25
    assert t.push([[q + 1.01, 0.0]], 15).tolist() == [1]                       # out of reach: a birth, track 0 freed
    assert t.trk_id.tolist() == [1, -1, -1] and t.trk_t.tolist() == [15, 0, 0]
    u = AT.TimedTracker(3, gate=1.0, gate_new=2.0, max_age=0, step=4)
    for xy, at in (([[0.0, 0.0]], 0), ([[1.0, 0.0]], 4)):
        u.push(xy, at)
    assert u.push([[4.6, 0.0]], 14).tolist() == [1]


def test_a_first_sample_has_no_velocity_and_takes_gate_new():
    """gate 1, gate_new 2, step 10, three ticks after the birth: the track predicts its own position whatever the gap
    (vel = 0), reaches 1.5 away (2.25 <= 4) and not 2.1 away (4.41 > 4); matched, its velocity is per STEP:
    1.5 / 0.3."""
    t = AT.TimedTracker(4, gate=1.0, gate_new=2.0, max_age=0, step=10)
    assert t.push([[0.00004, 0.0], [10.0, 0.00006]], 100).tolist() == [0, 1]
    assert t.trk_pos.tolist()[:2] == [[0.0, 0.0], [10.0, 0.0001]] and t.trk_t.tolist() == [100, 100, 0, 0]
    assert t.push([[7.9, 0.0001], [1.5, 0.0]], 103).tolist() == [2, 0]
    assert t.trk_vel[0].tolist() == [1.5 / np.float64(0.3), 0.0] and t.trk_hits.tolist() == [2, 1, 0, 0]
    assert t.trk_id.tolist() == [0, 2, -1, -1]                                  # track 1 aged out (max_age 0), slot reused


def test_ageing_at_exactly_max_age_and_one_past_it():
    """max_age 6 ticks: a slot whose last match is exactly 6 ticks old is left as it is (not even a counter moves); 7
    ticks old it is freed, zeros and all."""
    for gap, kept in ((6, True), (7, False)):
        t = AT.TimedTracker(2, gate=0.5, max_age=6, step=4)
        t.push([[0.0, 0.0]], 50)
        before = [x.copy() for x in t.state()[:5]]
        assert t.push(np.zeros((0, 2)), 50 + gap).tolist() == []
        if kept:
            assert all(np.array_equal(a, b) for a, b in zip(before, t.state()[:5]))
            assert t.push([[0.2, 0.0]], 50 + gap + 1).tolist() == [0]           # and comes back with its id
            assert t.trk_vel[0].tolist() == [0.2 / ((gap + 1) / 4.0), 0.0]
        else:
            assert t.trk_id.tolist() == [-1, -1] and t.trk_t.tolist() == [0, 0] and t.trk_hits.tolist() == [0, 0]
            assert t.push([[0.2, 0.0]], 50 + gap + 1).tolist() == [1]


def test_a_push_that_is_not_after_the_last_one_is_refused():
    t = AT.TimedTracker(3, gate=1.0, max_age=10, step=4, m_max=2)
    assert t.push([[0.0, 0.0], [5.0, 0.0]], -7).tolist() == [0, 1]              # the first push takes any time
    before = [x.copy() for x in t.state()[:6]]
    for when in (-7, -8):
        assert t.push([[0.1, 0.0], [5.1, 0.0], [9.0, 9.0]], when).tolist() == [-1, -1]      # m = min(count, m_max)
        assert t.flags == AT.TIME_ORDER and t.clock == [-7, 1]
        assert all(np.array_equal(a, b) for a, b in zip(before, t.state()[:6]))
    assert t.push([[0.1, 0.0], [5.1, 0.0]], -6).tolist() == [0, 1] and t.flags == 0 and t.clock == [-6, 2]


def test_when_the_slots_run_out():
    t = AT.TimedTracker(2, gate=0.5, step=3)
    ids = t.push([[0.0, 0.0], [5.0, 0.0], [10.0, 0.0], [15.0, 0.0]], 0)
    assert ids.tolist() == [0, 1, 2, 3] and t.flags == assoc_np.FULL and int(t.next_id) == 4
    assert t.trk_id.tolist() == [0, 1]
    ids = t.push([[10.0, 0.0], [0.1, 0.0]], 1)                                  # 10.0 was never remembered: a fresh id
    assert ids.tolist() == [4, 0] and t.flags == 0 and t.trk_id.tolist() == [0, 4]


# ---- 2. one push per step is the untimed rule ----------------------------------------------------------------------------
@pytest.mark.parametrize("step", [10, 7])
@pytest.mark.parametrize("max_miss", [0, 2])
@pytest.mark.parametrize("rec", sorted(RECS))
def test_one_push_per_step_is_the_untimed_rule_bit_for_bit(frames_of, rec, step, max_miss):
    """200 pushes one step apart with max_age = max_miss * step: ids, positions, velocities and hits are those of
    assoc_np.Tracker bytewise after every push, and t_now - trk_t == miss * step in every live slot.  (Every 11th push
    is halved so that tracks are missed and come back.)"""
    pushes = [xy if i % 11 != 5 else xy[::2] for i, (_, xy) in enumerate(frames_of[rec][:200])]
    a = assoc_np.Tracker(256, 1.0, 2.0, max_miss)
    b = AT.TimedTracker(256, 1.0, 2.0, max_miss * step, step)
    aged = 0
    for i, xy in enumerate(pushes):
        t_now = -333 + i * step
        assert a.push(xy).tobytes() == b.push(xy, t_now).tobytes(), i
        for x, y in ((a.trk_id, b.trk_id), (a.trk_pos, b.trk_pos), (a.trk_vel, b.trk_vel), (a.trk_hits, b.trk_hits)):
            assert x.tobytes() == y.tobytes(), i
        live = a.trk_id >= 0
        assert np.array_equal((t_now - b.trk_t)[live], a.trk_miss[live].astype(np.int64) * step), i
        assert not b.trk_t[~live].any() and int(a.next_id) == int(b.next_id) and a.flags == b.flags
        aged += int(a.trk_miss[live].sum())
    assert (aged > 50) == (max_miss > 0)


# ---- 3. the spec, both refusals, staging and packing ---------------------------------------------------------------------
def test_timed_associate_spec_checks():
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import TimedAssociateSpec
    assert TimedAssociateSpec(1.0) == (1.0, 2.0, 0, None) and TimedAssociateSpec(0.5, 0.5, 30, 64) == (0.5, 0.5, 30, 64)
    assert TimedAssociateSpec(1.0, max_age=None).max_age == 0 and TimedAssociateSpec(1, 2, np.int64(7)).max_age == 7
    assert frames.ASSOC_FULL == 1 and frames.ASSOC_TIME_ORDER == 2 == AT.TIME_ORDER
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="TimedAssociateSpec: gate"):
            TimedAssociateSpec(bad)
    for bad in (0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="TimedAssociateSpec: gate_new"):
            TimedAssociateSpec(1.0, bad)
    for bad in (1e200, 1e-200):
        with pytest.raises(ValueError, match="TimedAssociateSpec: the squared gates"):
            TimedAssociateSpec(bad)
    for bad in (-1, 0.5, True, 1 << 31, "3", float("nan")):
        with pytest.raises(ValueError, match="TimedAssociateSpec: max_age"):
            TimedAssociateSpec(1.0, max_age=bad)
    for bad in (0, 2049, 1.5):
        with pytest.raises(ValueError, match="TimedAssociateSpec: capacity"):
            TimedAssociateSpec(1.0, capacity=bad)


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_both_refusals_of_the_predictors():
    """Ahead of anything that needs the device: the timed spec without time=, and the untimed spec with it, word for
    word what it was."""
    from social_stgcnn_amd.frames import AssociateSpec, FramePredictor, StreamsPredictor, TimedAssociateSpec, TimeRule
    for make in (lambda **kw: FramePredictor(_Model(), **kw), lambda **kw: StreamsPredictor(_Model(), 3, **kw)):
        with pytest.raises(ValueError, match=r"associate=TimedAssociateSpec\(\.\.\.\) needs time=TimeRule"):
            make(associate=TimedAssociateSpec(1.0))
        for spec in (AssociateSpec(1.0), (1.0,), 1.0):
            with pytest.raises(ValueError) as e:
                make(associate=spec, time=TimeRule(10))
            assert str(e.value) == ("associate= together with time= is not supported: a velocity per tick and a gate that "
                                    "grows with the gap are a change of their own (DESIGN.md 8)")


def test_staging_checks_of_timed_pushes_without_ids():
    """The push's own checks come ahead of any device work: predictors that never saw a device."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import FramePredictor, StreamsPredictor, TimedAssociateSpec, TimeRule
    fp = FramePredictor.__new__(FramePredictor)
    fp.time, fp.m_max, fp.assoc = TimeRule(4).checked(8), 4, TimedAssociateSpec(1.0)
    with pytest.raises(ValueError, match="needs the push's time"):
        fp._stage(None, [[0.0, 0.0]], None)
    with pytest.raises(ValueError, match="integer number of ticks"):
        fp._stage(None, [[0.0, 0.0]], None, t=1.5)
    with pytest.raises(ValueError, match="assigns the ids itself"):
        fp._stage([1], [[0.0, 0.0]], None, t=3)
    with pytest.raises(ValueError, match="5 detections > max_detections=4"):
        fp._stage(None, np.zeros((5, 2)), None, t=3)
    sp = StreamsPredictor.__new__(StreamsPredictor)
    sp.time, sp.ns, sp.m_max, sp.cap, sp.assoc = TimeRule(4).checked(8), 3, 4, 12, TimedAssociateSpec(1.0)
    with pytest.raises(ValueError, match="needs the streams' push times"):
        sp._stage({0: (None, [[0.0, 0.0]])}, None)
    with pytest.raises(ValueError, match="stream 0: .*assigns the ids itself"):
        sp._stage({0: ([1], [[0.0, 0.0]])}, None, times=[0, 0, 0])
    with pytest.raises(ValueError, match="stream 2 is pushed without a time"):
        sp._stage({0: (None, [[0.0, 0.0]]), 2: (None, [[1.0, 0.0]])}, None, times={0: 5})
    with pytest.raises(ValueError, match="DeviceTick: times must be a device int64"):
        sp._stage(frames.DeviceTick(None, None, None), None, times=[0, 0, 0])


def test_packing_of_timed_ticks_without_ids():
    """A timed tick of (None, xy) entries packs as an untimed one, and its times as those of a tick with ids."""
    from social_stgcnn_amd.frames import StreamsPredictor, pack_tick
    a, b = np.arange(6.0).reshape(3, 2), np.zeros((0, 2))
    pk = pack_tick([(None, a), None, (None, b), (None, [[7.0, 8.0]])], 4, 3, 8, associate=True)
    assert pk.ids is None and pk.det_start.tolist() == [0, 3, 3, 3, 4] and pk.pushed.tolist() == [1, 0, 1, 1]
    assert pk.xy.tolist() == a.tolist() + [[7.0, 8.0]] and pk.xy.dtype == np.float64
    sp = StreamsPredictor.__new__(StreamsPredictor)
    sp.ns = 4
    assert sp._host_times([5, None, -9, 1 << 40], pk.pushed).tolist() == [5, 0, -9, 1 << 40]
    assert sp._host_times({0: 5, 2: 6, 3: 7}, pk.pushed).tolist() == [5, 0, 6, 7]
    assert sp._host_times(np.array([1, 2, 3, 4]), pk.pushed).tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="stream 3 is pushed without a time"):
        sp._host_times({0: 5, 2: 6}, pk.pushed)


# ---- 4. the C ABI and the command ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_timed_association_header_its_binding_and_the_exports(L):
    """include/stgcnn_hip_assoc_time.h -- which stgcnn_hip.h includes inside its extern "C" block, behind the other
    part-headers -- as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its two
    entry points by name, nothing but void *, int, int64_t and double among their parameters, the new flag beside the old
    one, ABI version 8."""
    from social_stgcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    inc = '#include "stgcnn_hip_assoc_time.h"'
    assert re.search("^" + re.escape(inc) + "$", main, re.M)
    assert main.index('extern "C" {') < main.index('#include "stgcnn_hip_harvest_time.h"') < main.index(inc) \
        < main.rindex("#ifdef __cplusplus")
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_assoc_time.h")).read()
    assert re.search(r"^#define STG_ASSOC_TIME_ORDER 2\b", raw_hdr, re.M) and re.search(r"^#define STG_ASSOC_FULL 1\b", main, re.M)
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_associate_timed", "stg_associate_streams_timed"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}, p.name
        assert fn.restype == ctypes.c_int, p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


PTRS = ("det_id", "det_xy", "det_time", "clock", "trk_id", "trk_pos", "trk_vel", "trk_t", "trk_hits", "next_id",
        "assoc_flags")


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    f = ctypes.c_void_p(64)

    def one(m_max=8, c=16, g2=1.0, gn2=4.0, step=10, max_age=0, count=f, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_associate_timed(p["det_id"], p["det_xy"], count, p["det_time"], p["clock"], m_max,
                                     *(p[n] for n in PTRS[4:]), c, 1e4, g2, gn2, step, max_age, None)

    def many(m_max=8, c=16, g2=1.0, gn2=4.0, step=10, max_age=0, ns=4, m_total=16, stride=3, start=f, pushed=f, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_associate_streams_timed(p["det_id"], stride, p["det_xy"], 3, m_total, start, pushed, p["det_time"],
                                             p["clock"], ns, m_max, *(p[n] for n in PTRS[4:]), c, 1e4, g2, gn2, step,
                                             max_age, None)
    inf, nan = float("inf"), float("nan")
    einval = {"M_max=0": dict(m_max=0), "C=0": dict(c=0), "gate2=0": dict(g2=0.0), "gate2<0": dict(g2=-1.0),
              "gate2 inf": dict(g2=inf, gn2=inf), "gate2 nan": dict(g2=nan), "gate_new2 nan": dict(gn2=nan),
              "gate_new2 inf": dict(gn2=inf), "gate_new2 < gate2": dict(gn2=0.5), "step=0": dict(step=0),
              "step<0": dict(step=-4), "max_age<0": dict(max_age=-1), "max_age=2^31": dict(max_age=1 << 31),
              **{"null " + n: {n: True} for n in PTRS}}
    unsupported = {"M_max above the limit": dict(m_max=2049), "C above the limit": dict(c=2049),
                   "step=2^31": dict(step=1 << 31)}
    for name, kw in einval.items():
        assert one(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_timed:"), name
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_streams_timed:"), name
    for name, kw in unsupported.items():
        assert one(**kw) == -2 and many(**kw) == -2, name
    assert one(max_age=(1 << 31) - 1, step=(1 << 31) - 1, count=None) == -1          # the limits themselves are taken
    assert L.stg_last_error() == b"stg_associate_timed: null pointer"
    for name, kw in {"NS=0": dict(ns=0), "NS too large": dict(ns=4097), "M_total<0": dict(m_total=-1),
                     "M_total too large": dict(m_total=(1 << 23) + 1), "id_stride=0": dict(stride=0),
                     "null det_start": dict(start=None), "null pushed": dict(pushed=None)}.items():
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_streams_timed:"), name


def test_predict_frames_refusals():
    from social_stgcnn_amd import predict_frames as pf
    base = ["--checkpoint", "c", "--recording", "r", "--out", "o.npz"]
    for extra, msg in ((["--associate_timed", "1"], "--associate_timed needs --step"),
                       (["--associate_timed", "1", "--step", "4", "--associate", "1"],
                        "--associate_timed does not go together with --associate"),
                       (["--associate_timed", "1,2,3,4", "--step", "4"], r"GATE\[,GATE_NEW\[,MAX_AGE\]\] expected"),
                       (["--associate_timed", "1,0.5", "--step", "4"], "TimedAssociateSpec: gate_new"),
                       (["--associate_timed", "1,2,-1", "--step", "4"], "TimedAssociateSpec: max_age"),
                       (["--associate_timed", "1", "--step", "4", "--harvest", "9"],
                        "--harvest does not go together with --step"),
                       # the refusals of --associate, word for word
                       (["--harvest_timed", "10", "--step", "10", "--associate", "0.5"],
                        "^--harvest_timed does not go together with --associate$"),
                       (["--harvest", "10", "--associate", "0.5"],
                        "^--harvest does not go together with --associate or --radius / --zones$")):
        with pytest.raises(ValueError, match=msg):
            pf.main(base + extra)
    assert pf.parse_associate_timed("0.5") == (0.5, 1.0, 0, None) and pf.parse_associate_timed("1,3,40") == (1.0, 3.0, 40, None)


# ---- 5. identity quality -----------------------------------------------------------------------------------------------------
MEASURED = {"crowds_zara01": ((0, 20020), (0, 15454), (4, 16263)), "biwi_hotel": ((0, 24616), (1, 19011), (2, 19984)),
            "biwi_eth": ((1, 20528), (3, 15800), (5, 16636))}


@pytest.mark.parametrize("rec", sorted(RECS))
def test_rule_keeps_identities_at_four_pushes_per_step(frames_of, rec):
    """The recording upsampled 4x (harvest_time_np.upsample), step 4, gates 1 / 2 m, one push per tick.  The condition,
    on each of two feeds: at most 0.1 % of the detections whose recorded id was also in the previous push get another id
    than that pedestrian had then.
      regular   every push, max_age 0
      damaged   every push with i % 7 == 3 left out and 5 % of the detections dropped (default_rng(0)), max_age = step
    Measured (wrong / links): crowds_zara01 0 / 20,020 and 0 / 15,454, biwi_hotel 0 / 24,616 and 1 / 19,011, biwi_eth
    1 / 20,528 and 3 / 15,800; the totals are asserted.  On the damaged feed the links over a missed detection or a missed
    push are held to the same cap: a recorded id last detected at most max_age ticks ago, against the id it had then --
    4 / 16,263, 2 / 19,984 and 5 / 16,636.  (The untimed rule on the original 2.5 Hz feed: 11 / 5,005, 13 / 6,154 and
    379 / 5,132.)"""
    up = upsample(frames_of[rec], 4)
    times = list(range(len(up)))
    dp, dt = AT.damaged(up, times)
    got = (AT.wrong_links(up, times, 4, 1.0, 2.0, 0), AT.wrong_links(dp, dt, 4, 1.0, 2.0, 4),
           AT.wrong_links(dp, dt, 4, 1.0, 2.0, 4, within=4))
    for what, (wrong, total), measured in zip(("regular", "damaged", "damaged, over gaps"), got, MEASURED[rec]):
        print("%s %s: %d wrong links of %d (%.4f %%)" % (rec, what, wrong, total, 100.0 * wrong / total))
        assert total == measured[1], (what, total)
        assert wrong <= 0.001 * total, (what, wrong, total)
    assert len(dp) == len(up) - len(range(3, len(up), 7))
