"""CPU: the filtered association rule restated (assoc_filter_np) on hand-computed cases, the checks of
frames.FilteredAssociateSpec and both refusals of the live predictors, the packing of timed ticks without ids, the header
against the binding, the entry points' and the command's refusals, and the identity quality the rule must keep on three
committed recordings at ten NOISY pushes per step."""
import ctypes
import os
import re

import numpy as np
import pytest

import assoc_filter_np as AF
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


@pytest.fixture(scope="module")
def up10(frames_of):
    """... upsampled 10x, once."""
    return {name: upsample(p, 10) for name, p in frames_of.items()}


# ---- 1. the restatement on hand-computed cases ---------------------------------------------------------------------------
# Dyadic parameters: sigma_det 0.5 (r = 0.25), sigma_vel0 1 (v0 = 1), step 4, so that every predicted covariance and S is
# an exact dyadic number; what is rounded is the two quotients K0, K1 and their products, written out below.
def _dyadic(**kw):
    args = dict(capacity=3, sigma_det=0.5, sigma_acc=0.0, sigma_vel0=1.0, gate_sigmas=2.0, gate_max=4.0, max_age=0, step=4)
    args.update(kw)
    return AF.FilteredTracker(**args)


def test_a_birth_a_first_match_and_a_gap_of_two_and_a_half_steps():
    t = _dyadic()
    # the birth: pos = p, vel = 0, cov = {r, 0, v0}
    assert t.push([[0.0, 0.0]], 0).tolist() == [0]
    assert t.trk_pos[0].tolist() == [0.0, 0.0] and t.trk_vel[0].tolist() == [0.0, 0.0]
    assert t.trk_cov[0].tolist() == [0.25, 0.0, 1.0] and t.trk_t.tolist() == [0, 0, 0] and t.trk_hits.tolist() == [1, 0, 0]
    # one step on (k = 1): a11 = 1, a01 = 0 + 1 * 1 = 1, a00 = 0.25 + 1 * (0 + 1) = 1.25, S = 1.5, g2 = min(4 * 1.5, 16) = 6
    assert t.push([[1.5, -0.5]], 4).tolist() == [0] and t.last_s == {0: 1.5}
    k0, k1 = 1.25 / 1.5, 1.0 / 1.5
    assert t.trk_pos[0].tolist() == [0.0 + k0 * 1.5, 0.0 + k0 * -0.5]
    assert t.trk_vel[0].tolist() == [0.0 + k1 * 1.5, 0.0 + k1 * -0.5]
    p00, p01, p11 = 1.25 - k0 * 1.25, 1.0 - k0 * 1.0, 1.0 - k1 * 1.0
    assert t.trk_cov[0].tolist() == [p00, p01, p11] and t.trk_t.tolist() == [4, 0, 0] and t.trk_hits.tolist() == [2, 0, 0]
    assert abs(p00 - 0.25 * 1.25 / 1.5) < 1e-15 and abs(p11 - 1.0 / 3.0) < 1e-15          # r a00 / S, a11 - a01^2 / S
    # two and a half steps on (t = 14, k = 2.5), sigma_acc = 0: every qa term is +0
    px, py = t.trk_pos[0].tolist()
    vx, vy = t.trk_vel[0].tolist()
    qx, qy = px + vx * 2.5, py + vy * 2.5
    u = 2.5 * p11
    a11, a01, a00 = p11 + 0.0, (p01 + u) + 0.0, (p00 + 2.5 * (2.0 * p01 + u)) + 0.0
    s = a00 + 0.25
    assert t.push([[4.5, -1.75]], 14).tolist() == [0] and t.last_s == {0: s}
    k0, k1 = a00 / s, a01 / s
    assert t.trk_pos[0].tolist() == [qx + k0 * (4.5 - qx), qy + k0 * (-1.75 - qy)]
    assert t.trk_vel[0].tolist() == [vx + k1 * (4.5 - qx), vy + k1 * (-1.75 - qy)]
    assert t.trk_cov[0].tolist() == [a00 - k0 * a00, a01 - k0 * a01, a11 - k1 * a01]
    assert t.trk_t.tolist() == [14, 0, 0] and t.trk_hits.tolist() == [3, 0, 0] and t.clock == [14, 3]


def test_the_acceleration_terms_in_the_statement_order():
    """sigma_acc 1 (qa = 1), one step after a birth: w = 1, a11 = 1 + 1, a01 = (0 + 1) + (1 * 1) / 2, a00 = (0.25 + 1 * (0 +
    1)) + ((1 * 1) * 1) / 3; and at k = 0.75 (step 4, 3 ticks) the products in the order written."""
    t = _dyadic(sigma_acc=1.0)
    t.push([[0.0, 0.0]], 0)
    t.push([[0.25, 0.0]], 4)
    a00, a01, a11 = 1.25 + 1.0 / 3.0, 1.5, 2.0
    s = a00 + 0.25
    k0, k1 = a00 / s, a01 / s
    assert t.last_s == {0: s} and t.trk_cov[0].tolist() == [a00 - k0 * a00, a01 - k0 * a01, a11 - k1 * a01]
    assert t.trk_pos[0].tolist() == [k0 * 0.25, 0.0] and t.trk_vel[0].tolist() == [k1 * 0.25, 0.0]
    p00, p01, p11 = t.trk_cov[0].tolist()
    k = 0.75
    w = 1.0 * k
    u = k * p11
    wk = w * k
    b00, b01, b11 = (p00 + k * (2.0 * p01 + u)) + (wk * k) / 3.0, (p01 + u) + wk / 2.0, p11 + w
    got = AF.ahead(np.float64(p00), np.float64(p01), np.float64(p11), np.float64(k), np.float64(1.0), np.float64(0.25))
    assert [float(x) for x in got] == [b00, b01, b11, b00 + 0.25]
    t.push([[0.5, 0.0]], 7)
    assert t.last_s == {0: b00 + 0.25}


def test_the_gate_grows_with_the_gap_and_gate_max_bounds_it():
    """gate_sigmas 1, gate_max 2.5, a track born at the origin (vel 0, so it predicts the origin whatever the gap).  One
    step on S = 1.5: a detection 2.0 away (4 > 1.5) is out of reach, as it is of N12's fixed gate of 1; two steps on S =
    0.25 + 4 + 0.25 = 4.5 and it is taken (4 <= 4.5).  Two and a half steps on S = 6.75 but gate_max^2 = 6.25: a
    detection 2.55 away (6.5025) is within the sigmas and refused by gate_max; 2.5 away (6.25 <= 6.25) is taken."""
    def born():
        t = _dyadic(gate_sigmas=1.0, gate_max=2.5, max_age=100)
        t.push([[0.0, 0.0]], 0)
        return t
    t = born()
    assert t.push([[2.0, 0.0]], 4).tolist() == [1] and t.last_s == {0: 1.5}
    t = born()
    assert t.push([[2.0, 0.0]], 8).tolist() == [0] and t.last_s == {0: 4.5}
    t = born()
    assert t.push([[0.0, 2.55]], 10).tolist() == [1] and t.last_s == {0: 6.75} and t.trk_hits.tolist() == [1, 1, 0]
    t = born()
    assert t.push([[0.0, -2.5]], 10).tolist() == [0] and t.trk_hits.tolist() == [2, 0, 0]
    u = AT.TimedTracker(3, gate=1.0, gate_new=1.0, max_age=100, step=4)
    u.push([[0.0, 0.0]], 0)
    assert u.push([[2.0, 0.0]], 8).tolist() == [1]                            # the two-sample rule's gate does not grow


def test_the_order_is_euclidean_and_ties_go_to_the_lower_slot():
    """Two tracks, one detection between them at equal distance: slot 0 takes it, whatever the two slots' S."""
    t = _dyadic(max_age=100)
    t.push([[0.0, 0.0]], 0)
    t.push([[0.0, 0.0], [2.0, 0.0]], 4)                                         # slot 1 is younger: a larger S
    assert t.trk_id.tolist() == [0, 1, -1] and t.trk_cov[1, 0] > t.trk_cov[0, 0]
    assert t.push([[1.0, 0.0]], 8).tolist() == [0]
    assert t.trk_hits.tolist() == [3, 1, 0]


def test_ageing_at_exactly_max_age_and_one_past_it():
    for gap, kept in ((6, True), (7, False)):
        t = _dyadic(capacity=2, max_age=6)
        t.push([[0.0, 0.0]], 50)
        before = [x.copy() for x in t.state()[:6]]
        assert t.push(np.zeros((0, 2)), 50 + gap).tolist() == []
        if kept:
            assert all(np.array_equal(a, b) for a, b in zip(before, t.state()[:6]))
            assert t.push([[0.2, 0.0]], 50 + gap + 1).tolist() == [0]           # and comes back with its id
            k = np.float64(gap + 1) / 4.0
            assert t.last_s == {0: (0.25 + k * (0.0 + k * 1.0)) + 0.25}           # the uncertainty grew through k
        else:
            assert t.trk_id.tolist() == [-1, -1] and not t.trk_t.any() and not t.trk_cov.any() and not t.trk_hits.any()
            assert t.push([[0.2, 0.0]], 50 + gap + 1).tolist() == [1]


def test_a_push_that_is_not_after_the_last_one_is_refused():
    t = _dyadic(max_age=10, m_max=2)
    assert t.push([[0.0, 0.0], [5.0, 0.0]], -7).tolist() == [0, 1]
    before = [x.copy() for x in t.state()[:7]]
    for when in (-7, -8):
        assert t.push([[0.1, 0.0], [5.1, 0.0], [9.0, 9.0]], when).tolist() == [-1, -1]      # m = min(count, m_max)
        assert t.flags == AT.TIME_ORDER == 2 and t.clock == [-7, 1]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, t.state()[:7]))
    assert t.push([[0.1, 0.0], [5.1, 0.0]], -6).tolist() == [0, 1] and t.flags == 0 and t.clock == [-6, 2]


def test_when_the_slots_run_out():
    t = _dyadic(capacity=2)
    ids = t.push([[0.0, 0.0], [5.0, 0.0], [10.0, 0.0], [15.0, 0.0]], 0)
    assert ids.tolist() == [0, 1, 2, 3] and t.flags == assoc_np.FULL and int(t.next_id) == 4
    assert t.trk_id.tolist() == [0, 1] and t.trk_cov.tolist() == [[0.25, 0.0, 1.0]] * 2
    ids = t.push([[10.0, 0.0], [0.1, 0.0]], 1)                                  # 10.0 was never remembered: a fresh id
    assert ids.tolist() == [4, 0] and t.flags == 0 and t.trk_id.tolist() == [0, 4]


def _feed(frames_of, rec="crowds_zara01", n=200, sigma=0.05):
    up = upsample(frames_of[rec][:n // 4 + 2], 4)[:n]
    return AT.damaged(AF.noisy(up, sigma, 1), list(range(len(up))))


def test_without_acceleration_p11_never_grows(frames_of):
    """sigma_acc = 0: a prediction leaves p11 as it is and an update takes a01^2 / S >= 0 off it."""
    pushes, times = _feed(frames_of)
    t = AF.FilteredTracker(256, 0.05, 0.0, max_age=8, step=4)
    p11 = {}
    matched = 0
    for (_, xy), at in zip(pushes, times):
        t.push(xy, at)
        for s in np.flatnonzero(t.trk_id >= 0):
            key = (s, int(t.trk_id[s]))
            if key in p11:
                assert t.trk_cov[s, 2] <= p11[key]
                matched += int(t.trk_cov[s, 2] < p11[key])
            p11[key] = t.trk_cov[s, 2]
    assert matched > 500


@pytest.mark.parametrize("sigma_acc", [0.0, 1.0])
def test_the_variances_stay_positive_over_200_pushes(frames_of, sigma_acc):
    pushes, times = _feed(frames_of)
    t = AF.FilteredTracker(256, 0.05, sigma_acc, max_age=8, step=4)
    seen = 0
    for (_, xy), at in zip(pushes, times):
        t.push(xy, at)
        assert all(s > 0 for s in t.last_s.values())
        live = t.trk_id >= 0
        assert (t.trk_cov[live][:, [0, 2]] >= 0).all() and np.isfinite(t.trk_cov).all() and not t.trk_cov[~live].any()
        seen += len(t.last_s)
    assert seen > 1000 and len(pushes) > 160


# ---- 2. the spec, both refusals, staging and packing ---------------------------------------------------------------------
def test_filtered_associate_spec_checks():
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import FilteredAssociateSpec as Spec
    assert Spec(0.05, 1.0) == (0.05, 1.0, 1.5, 5.0, 2.0, 0, None)
    assert Spec(1, 0, 2, 3, 4, np.int64(7), 64) == (1.0, 0.0, 2.0, 3.0, 4.0, 7, 64) and Spec(0.1, 0.0).sigma_acc == 0.0
    assert Spec(0.1, 1.0, max_age=None).max_age == 0 and frames.ASSOC_TIME_ORDER == 2
    assert Spec._fields == ("sigma_det", "sigma_acc", "sigma_vel0", "gate_sigmas", "gate_max", "max_age", "capacity")
    for name in ("sigma_det", "sigma_vel0", "gate_sigmas", "gate_max"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True, None, 1e200, 1e-200):
            with pytest.raises(ValueError, match="FilteredAssociateSpec: .*" + name):
                Spec(**{"sigma_det": 0.1, "sigma_acc": 1.0, name: bad})
    for bad in (-0.5, float("nan"), float("inf"), "1", True, None, 1e200):
        with pytest.raises(ValueError, match="FilteredAssociateSpec: .*sigma_acc"):
            Spec(0.1, bad)
    for bad in (-1, 0.5, True, 1 << 31, "3", float("nan")):
        with pytest.raises(ValueError, match="FilteredAssociateSpec: max_age"):
            Spec(0.1, 1.0, max_age=bad)
    for bad in (0, 2049, 1.5):
        with pytest.raises(ValueError, match="FilteredAssociateSpec: capacity"):
            Spec(0.1, 1.0, capacity=bad)


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_both_refusals_of_the_predictors():
    """Ahead of anything that needs the device: the filtered spec without time=, and the untimed spec with it, word for
    word what it was; the timed spec's refusal too."""
    from social_stgcnn_amd.frames import (AssociateSpec, FilteredAssociateSpec, FramePredictor, StreamsPredictor,
                                          TimedAssociateSpec, TimeRule)
    for make in (lambda **kw: FramePredictor(_Model(), **kw), lambda **kw: StreamsPredictor(_Model(), 3, **kw)):
        with pytest.raises(ValueError, match=r"associate=FilteredAssociateSpec\(\.\.\.\) needs time=TimeRule"):
            make(associate=FilteredAssociateSpec(0.05, 1.0))
        with pytest.raises(ValueError) as e:
            make(associate=TimedAssociateSpec(1.0))
        assert str(e.value) == ("associate=TimedAssociateSpec(...) needs time=TimeRule(...): its tracks are aged by time "
                                "(without time= the push-indexed AssociateSpec serves)")
        with pytest.raises(ValueError) as e:
            make(associate=AssociateSpec(1.0), time=TimeRule(10))
        assert str(e.value) == ("associate= together with time= is not supported: a velocity per tick and a gate that "
                                "grows with the gap are a change of their own (DESIGN.md 8)")


def test_staging_and_packing_of_timed_ticks_without_ids():
    """The push's own checks come ahead of any device work, under the filtered spec as under the timed one; a tick of
    (None, xy) entries packs without ids."""
    from social_stgcnn_amd.frames import FilteredAssociateSpec, FramePredictor, StreamsPredictor, TimeRule, pack_tick
    spec = FilteredAssociateSpec(0.05, 1.0)
    fp = FramePredictor.__new__(FramePredictor)
    fp.time, fp.m_max, fp.assoc = TimeRule(4).checked(8), 4, spec
    with pytest.raises(ValueError, match="needs the push's time"):
        fp._stage(None, [[0.0, 0.0]], None)
    with pytest.raises(ValueError, match="assigns the ids itself"):
        fp._stage([1], [[0.0, 0.0]], None, t=3)
    with pytest.raises(ValueError, match="5 detections > max_detections=4"):
        fp._stage(None, np.zeros((5, 2)), None, t=3)
    sp = StreamsPredictor.__new__(StreamsPredictor)
    sp.time, sp.ns, sp.m_max, sp.cap, sp.assoc = TimeRule(4).checked(8), 3, 4, 12, spec
    with pytest.raises(ValueError, match="needs the streams' push times"):
        sp._stage({0: (None, [[0.0, 0.0]])}, None)
    with pytest.raises(ValueError, match="stream 0: .*assigns the ids itself"):
        sp._stage({0: ([1], [[0.0, 0.0]])}, None, times=[0, 0, 0])
    a = np.arange(6.0).reshape(3, 2)
    pk = pack_tick([(None, a), None, (None, np.zeros((0, 2))), (None, [[7.0, 8.0]])], 4, 3, 8, associate=True)
    assert pk.ids is None and pk.det_start.tolist() == [0, 3, 3, 3, 4] and pk.pushed.tolist() == [1, 0, 1, 1]
    assert pk.xy.tolist() == a.tolist() + [[7.0, 8.0]] and pk.xy.dtype == np.float64
    with pytest.raises(ValueError, match="needs associate="):
        fp._assoc_state = None
        fp.assoc_tracks()


# ---- 3. the C ABI and the command ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_filtered_association_header_its_binding_and_the_exports(L):
    """include/stgcnn_hip_assoc_filter.h -- which stgcnn_hip.h includes inside its extern "C" block, behind the N12
    header -- as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its two entry
    points by name, nothing but void *, int, int64_t and double among their parameters, four more of them than their
    timed twins take, ABI version 8."""
    from social_stgcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    inc = '#include "stgcnn_hip_assoc_filter.h"'
    assert re.search("^" + re.escape(inc) + "$", main, re.M)
    assert main.index('extern "C" {') < main.index('#include "stgcnn_hip_assoc_time.h"') < main.index(inc) \
        < main.rindex("#ifdef __cplusplus")
    protos = _lib.parse_header(open(os.path.join(ROOT, "include", "stgcnn_hip_assoc_filter.h")).read())
    assert [p.name for p in protos] == ["stg_associate_filtered", "stg_associate_streams_filtered"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}, p.name
        assert fn.restype == ctypes.c_int, p.name
    # the filtered entry points are the timed ones with trk_cov behind trk_t and five doubles in the place of two
    for name, twin in (("stg_associate_filtered", "stg_associate_timed"),
                       ("stg_associate_streams_filtered", "stg_associate_streams_timed")):
        mine, theirs = ([n for n, _ in _lib.PROTOTYPES[e].params] for e in (name, twin))
        assert len(getattr(L, name).argtypes) == len(mine) == len(getattr(L, twin).argtypes) + 4 == len(theirs) + 4
        at, k = theirs.index("gate2"), theirs.index("trk_t") + 1
        assert theirs[at:at + 2] == ["gate2", "gate_new2"] and mine[at + 1:at + 6] == ["r", "qa", "v0", "n2", "gmax2"]
        assert mine[:at + 1] == theirs[:k] + ["trk_cov"] + theirs[k:at] and mine[at + 6:] == theirs[at + 2:]
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


PTRS = ("det_id", "det_xy", "det_time", "clock", "trk_id", "trk_pos", "trk_vel", "trk_t", "trk_cov", "trk_hits", "next_id",
        "assoc_flags")


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    f = ctypes.c_void_p(64)

    def one(m_max=8, c=16, r=0.01, qa=1.0, v0=2.25, n2=25.0, gmax2=4.0, step=10, max_age=0, count=f, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_associate_filtered(p["det_id"], p["det_xy"], count, p["det_time"], p["clock"], m_max,
                                        *(p[n] for n in PTRS[4:]), c, 1e4, r, qa, v0, n2, gmax2, step, max_age, None)

    def many(m_max=8, c=16, r=0.01, qa=1.0, v0=2.25, n2=25.0, gmax2=4.0, step=10, max_age=0, ns=4, m_total=16, stride=3,
             start=f, pushed=f, **null):
        p = {n: None if n in null else f for n in PTRS}
        return L.stg_associate_streams_filtered(p["det_id"], stride, p["det_xy"], 3, m_total, start, pushed,
                                                p["det_time"], p["clock"], ns, m_max, *(p[n] for n in PTRS[4:]), c, 1e4,
                                                r, qa, v0, n2, gmax2, step, max_age, None)
    inf, nan = float("inf"), float("nan")
    einval = {"M_max=0": dict(m_max=0), "C=0": dict(c=0), "qa<0": dict(qa=-1.0), "qa nan": dict(qa=nan),
              "qa inf": dict(qa=inf), "step=0": dict(step=0), "step<0": dict(step=-4), "max_age<0": dict(max_age=-1),
              "max_age=2^31": dict(max_age=1 << 31), **{"null " + n: {n: True} for n in PTRS}}
    for name in ("r", "v0", "n2", "gmax2"):
        einval.update({"%s %r" % (name, bad): {name: bad} for bad in (0.0, -1.0, nan, inf)})
    unsupported = {"M_max above the limit": dict(m_max=2049), "C above the limit": dict(c=2049),
                   "step=2^31": dict(step=1 << 31)}
    for name, kw in einval.items():
        assert one(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_filtered:"), name
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_streams_filtered:"), name
    for name, kw in unsupported.items():
        assert one(**kw) == -2 and many(**kw) == -2, name
    # the limits themselves, and qa = 0, are taken: the next check is the one that fails
    assert one(max_age=(1 << 31) - 1, step=(1 << 31) - 1, qa=0.0, m_max=2048, c=2048, count=None) == -1
    assert L.stg_last_error() == b"stg_associate_filtered: null pointer"
    for name, kw in {"NS=0": dict(ns=0), "NS too large": dict(ns=4097), "M_total<0": dict(m_total=-1),
                     "M_total too large": dict(m_total=(1 << 23) + 1), "id_stride=0": dict(stride=0),
                     "null det_start": dict(start=None), "null pushed": dict(pushed=None)}.items():
        assert many(**kw) == -1, name
        assert L.stg_last_error().startswith(b"stg_associate_streams_filtered:"), name


def test_predict_frames_refusals():
    from social_stgcnn_amd import predict_frames as pf
    base = ["--checkpoint", "c", "--recording", "r", "--out", "o.npz"]
    for extra, msg in ((["--associate_filtered", "0.05,1"], "--associate_filtered needs --step"),
                       (["--associate_filtered", "0.05,1", "--step", "4", "--associate", "1"],
                        "--associate_filtered does not go together with --associate:"),
                       (["--associate_filtered", "0.05,1", "--step", "4", "--associate_timed", "1"],
                        "--associate_filtered does not go together with --associate_timed:"),
                       (["--associate_filtered", "0.05", "--step", "4"], r"SIGMA_DET,SIGMA_ACC\[,SIGMA_VEL0.* expected"),
                       (["--associate_filtered", "1,2,3,4,5,6,7", "--step", "4"], r"SIGMA_DET,SIGMA_ACC\[.* expected"),
                       (["--associate_filtered", "0,1", "--step", "4"], "FilteredAssociateSpec: sigma_det"),
                       (["--associate_filtered", "0.05,-1", "--step", "4"], "FilteredAssociateSpec: sigma_acc"),
                       (["--associate_filtered", "0.05,1,1.5,5,2,-1", "--step", "4"], "FilteredAssociateSpec: max_age"),
                       (["--associate_filtered", "0.05,1", "--step", "4", "--harvest", "9"],
                        "--harvest does not go together with --step"),
                       # the refusals of --associate_timed, word for word
                       (["--associate_timed", "1"], "^--associate_timed needs --step TICKS: its tracks are aged by time "
                                                    r"\(without --step, --associate serves\)$"),
                       (["--associate_timed", "1", "--step", "4", "--associate", "1"],
                        "^--associate_timed does not go together with --associate: one ages its tracks by time, the "
                        "other by push$")):
        with pytest.raises(ValueError, match=msg):
            pf.main(base + extra)
    assert pf.parse_associate_filtered("0.05,1") == (0.05, 1.0, 1.5, 5.0, 2.0, 0, None)
    assert pf.parse_associate_filtered("0.1,0,1,4,3,40") == (0.1, 0.0, 1.0, 4.0, 3.0, 40, None)


# ---- 4. identity quality -----------------------------------------------------------------------------------------------------
LINKS = {"crowds_zara01": 40748, "biwi_hotel": 50043, "biwi_eth": 41722}


@pytest.mark.parametrize("sigma", [0.05, 0.10])
@pytest.mark.parametrize("rec", sorted(RECS))
def test_rule_keeps_identities_on_noisy_feeds_at_ten_pushes_per_step(up10, rec, sigma):
    """The recording upsampled 10x (harvest_time_np.upsample), Gaussian noise of sigma metres on every detection
    (noisy(.., sigma, seed 1)), then every push with i % 7 == 3 left out and 5 % of the detections dropped
    (assoc_time_np.damaged, seed 0); step 10, max_age 20, links counted over gaps of up to 20 ticks.  The spec is
    (sigma, 1.0, 1.5, 5.0, 2.0).  The conditions:
      1. sigma 0.05: at most 0.1 % wrong links, the project's cap.
      2. sigma 0.05: at most a third of the wrong links of the two-sample rule (assoc_time_np, gates 1 / 2 m, max_age 20)
         on the identical feed.
      3. sigma 0.10: at most 0.5 % wrong links.
      4. the link totals are asserted: 40,748 / 50,043 / 41,722.
    Measured, wrong links of the filtered rule (of the two-sample rule), crowds_zara01 / biwi_hotel / biwi_eth:
      sigma 0.02    0 (3)       2 (1)       4 (1)          (not asserted)
      sigma 0.05    5 (95)      5 (191)     15 (83)        0.012 / 0.010 / 0.036 %, ratios 0.05 / 0.03 / 0.18
      sigma 0.10    64 (2,179)  153 (2,355) 124 (1,855)    0.16 / 0.31 / 0.30 % against 5.3 / 4.7 / 4.4 %"""
    up = up10[rec]
    times = list(range(len(up)))
    pushes, at = AT.damaged(AF.noisy(up, sigma, 1), times, seed=0)
    wrong, total = AF.wrong_links(pushes, at, 10, sigma, 1.0, 1.5, 5.0, 2.0, max_age=20, within=20)
    print("%s sigma %.2f filtered: %d wrong links of %d (%.4f %%)" % (rec, sigma, wrong, total, 100.0 * wrong / total))
    assert total == LINKS[rec]
    if sigma == 0.05:
        assert wrong <= 0.001 * total, (wrong, total)
        other, total2 = AT.wrong_links(pushes, at, 10, 1.0, 2.0, 20, within=20)
        print("%s sigma %.2f two-sample: %d wrong links of %d" % (rec, sigma, other, total2))
        assert total2 == total and 3 * wrong <= other, (wrong, other)
    else:
        assert wrong <= 0.005 * total, (wrong, total)
