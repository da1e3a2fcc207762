"""CPU: the association rule restated (assoc_np) on hand-computed cases, the checks of frames.AssociateSpec and the
refusals of the live predictors, the packing of (None, xy) ticks, and the identity quality the rule must keep on three
committed recordings."""
import numpy as np
import pytest

import assoc_np
from live_inputs import _pushes, _rows


def test_restatement_on_hand_computed_cases():
    t = assoc_np.Tracker(4, gate=1.0, gate_new=2.0, max_miss=1, decimals=4)
    # two births in detection order, the rounding of the push kernels
    assert t.push([[0.00004, 0.0], [10.0, 0.00006]]).tolist() == [0, 1]
    assert t.trk_id.tolist() == [0, 1, -1, -1] and t.trk_hits.tolist() == [1, 1, 0, 0]
    assert t.trk_pos.tolist() == [[0.0, 0.0], [10.0, 0.0001], [0.0, 0.0], [0.0, 0.0]] and int(t.next_id) == 2
    # a one-sample track reaches gate_new = 2 (cost 2.25 + 0 <= 4), not further (cost 4.41 > 4 from track 1: a birth)
    assert t.push([[7.9, 0.0001], [1.5, 0.0]]).tolist() == [2, 0]
    assert t.trk_id.tolist() == [0, 1, 2, -1] and t.trk_vel[0].tolist() == [1.5, 0.0]
    assert t.trk_miss.tolist() == [0, 1, 0, 0] and t.trk_hits.tolist() == [2, 1, 1, 0]
    # track 0 predicts 1.5 + 1.5 = 3.0 and has gate 1 now: 4.1 is out of reach (1.21 > 1), 3.9 is in (0.81)
    assert t.push([[4.1, 0.0]]).tolist() == [3]
    # track 1 missed twice > max_miss: freed, its slot taken by the birth; track 2 (7.9) missed once
    assert t.trk_id.tolist() == [0, 3, 2, -1] and t.trk_miss.tolist() == [1, 0, 1, 0]
    # missed once: track 0 predicts 1.5 + 1.5 * 2 = 4.5, and the velocity is the displacement per push: (5.1 - 1.5) / 2
    assert t.push([[5.1, 0.0]]).tolist() == [0]
    assert t.trk_vel[0].tolist() == [(5.1 - 1.5) / 2.0, 0.0] and t.trk_miss[0] == 0 and t.trk_hits[0] == 3
    assert t.trk_id.tolist() == [0, 3, -1, -1]                        # track 2 missed twice: freed, zeros
    assert t.trk_hits.tolist() == [3, 1, 0, 0] and t.flags == 0 and int(t.next_id) == 4


def test_restatement_is_globally_greedy_with_ties_by_slot_then_detection():
    t = assoc_np.Tracker(3, gate=5.0, gate_new=5.0)
    t.push([[0.0, 0.0], [2.0, 0.0], [4.0, 0.0]])
    # detection 0 at 1.0 is 1 away from tracks 0 and 1: the tie goes to the lower slot; detection 1 at 3.0 is 1 away from
    # tracks 1 and 2: again the lower slot; track 2 is left without one and 9.5 is out of everyone's reach: a birth
    assert t.push([[1.0, 0.0], [3.0, 0.0], [9.5, 0.0]]).tolist() == [0, 1, 3]
    assert t.trk_id.tolist() == [0, 1, 3]                              # track 2 (max_miss 0) freed, its slot reused
    # one track, two detections at the same distance: the lower detection index
    u = assoc_np.Tracker(2, gate=5.0, gate_new=5.0)
    u.push([[0.0, 0.0]])
    assert u.push([[0.0, 1.0], [1.0, 0.0]]).tolist() == [0, 1]
    # greedy, not optimal: the closest pair (track 1, 0.9) goes first, and track 0 cannot reach 2.2 (4.84 > 2.25)
    w = assoc_np.Tracker(2, gate=1.5, gate_new=1.5)
    w.push([[0.0, 0.0], [1.0, 0.0]])
    assert w.push([[0.9, 0.0], [2.2, 0.0]]).tolist() == [1, 2]
    assert w.trk_id.tolist() == [2, 1] and w.trk_pos.tolist() == [[2.2, 0.0], [0.9, 0.0]]


def test_restatement_when_the_slots_run_out():
    t = assoc_np.Tracker(2, gate=0.5)
    ids = t.push([[0.0, 0.0], [5.0, 0.0], [10.0, 0.0], [15.0, 0.0]])
    assert ids.tolist() == [0, 1, 2, 3] and t.flags == assoc_np.FULL and int(t.next_id) == 4
    assert t.trk_id.tolist() == [0, 1]
    ids = t.push([[10.0, 0.0], [0.1, 0.0]])                            # 10.0 was never remembered: a fresh id again
    assert ids.tolist() == [4, 0] and t.flags == 0 and t.trk_id.tolist() == [0, 4]
    v = assoc_np.Tracker(2, gate=0.5, m_max=2)
    assert v.push([[0.0, 0.0], [5.0, 0.0], [9.0, 0.0]]).tolist() == [0, 1] and v.flags == 0     # past m_max: not touched


def test_associate_spec_checks_and_refusals():
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import AssociateSpec, FramePredictor, StreamsPredictor, TimeRule, pack_tick
    from social_stgcnn_amd.model import social_stgcnn
    assert AssociateSpec(1.0) == (1.0, 2.0, 0, None) and AssociateSpec(0.5, 0.5, 3, 64) == (0.5, 0.5, 3, 64)
    assert frames.ASSOC_FULL == 1
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="gate"):
            AssociateSpec(bad)
    for bad in (0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gate_new"):
            AssociateSpec(1.0, bad)
    with pytest.raises(ValueError, match="squared gates"):
        AssociateSpec(1e200)
    with pytest.raises(ValueError, match="squared gates"):
        AssociateSpec(1e-200)
    for bad in (-1, 0.5, True):
        with pytest.raises(ValueError, match="max_miss"):
            AssociateSpec(1.0, max_miss=bad)
    for bad in (0, 2049, 1.5):
        with pytest.raises(ValueError, match="capacity"):
            AssociateSpec(1.0, capacity=bad)
    model = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
    for make in (lambda **kw: FramePredictor(model, **kw), lambda **kw: StreamsPredictor(model, 3, **kw)):
        with pytest.raises(ValueError, match="associate= together with time="):
            make(associate=AssociateSpec(1.0), time=TimeRule(10))
        with pytest.raises(ValueError, match="gate_new"):
            make(associate=(1.0, 0.5))
    # the push's own checks come ahead of any device work: a predictor that never saw a device
    fp = FramePredictor.__new__(FramePredictor)
    fp.time, fp.m_max = None, 4
    with pytest.raises(ValueError, match="ids=None needs a predictor made with associate="):
        fp._stage(None, [[0.0, 0.0]], None)
    fp.assoc = AssociateSpec(1.0)
    with pytest.raises(ValueError, match="assigns the ids itself"):
        fp._stage([1], [[0.0, 0.0]], None)
    with pytest.raises(ValueError, match="5 detections > max_detections=4"):
        fp._stage(None, np.zeros((5, 2)), None)
    sp = StreamsPredictor.__new__(StreamsPredictor)
    sp.time, sp.ns, sp.m_max, sp.cap = None, 3, 4, 12
    with pytest.raises(ValueError, match="stream 2: ids=None needs a predictor made with associate="):
        sp._stage({0: ([1], [[0.0, 0.0]]), 2: (None, [[0.0, 0.0]])}, None)
    with pytest.raises(ValueError, match="DeviceTick: ids=None needs"):
        sp._stage(frames.DeviceTick(None, None, None), None)
    sp.assoc = AssociateSpec(1.0)
    with pytest.raises(ValueError, match="stream 0: .*assigns the ids itself"):
        sp._stage({0: ([1], [[0.0, 0.0]])}, None)
    with pytest.raises(ValueError, match="DeviceTick: .*assigns the ids itself"):
        sp._stage(frames.DeviceTick([1], None, None), None)
    with pytest.raises(ValueError, match="assigns the ids itself"):
        pack_tick([([1], [[0.0, 0.0]])], 1, 4, 4, associate=True)


def test_packing_of_ticks_without_ids():
    from social_stgcnn_amd.frames import pack_tick
    a, b = np.arange(6.0).reshape(3, 2), np.zeros((0, 2))
    pk = pack_tick([(None, a), None, (None, b), (None, [[7.0, 8.0]])], 4, 3, 8, associate=True)
    assert pk.ids is None
    assert pk.det_start.tolist() == [0, 3, 3, 3, 4] and pk.pushed.tolist() == [1, 0, 1, 1]
    assert pk.xy.tolist() == a.tolist() + [[7.0, 8.0]] and pk.xy.dtype == np.float64
    pk = pack_tick({2: (None, a)}, 4, 3, 8, associate=True)
    assert pk.det_start.tolist() == [0, 0, 0, 3, 3] and pk.pushed.tolist() == [0, 0, 1, 0]
    with pytest.raises(ValueError, match="stream 0: 3 detections > max_detections=2"):
        pack_tick([(None, a)], 1, 2, 8, associate=True)
    with pytest.raises(ValueError, match="6 detections > max_total_detections=5"):
        pack_tick([(None, a), (None, a)], 2, 3, 5, associate=True)
    # a tick with ids packs as before
    pk = pack_tick([([4, 2, 9], a)], 1, 3, 8)
    assert pk.ids.tolist() == [4, 2, 9]


@pytest.mark.parametrize("rec, measured", [(("zara1_test", "crowds_zara01.txt"), (11, 5005)),
                                           (("univ_test", "students003.txt"), (9, 17519)),
                                           (("hotel_test", "biwi_hotel.txt"), (13, 6154))])
def test_rule_keeps_identities_on_the_recordings(rec, measured):
    """AssociateSpec(1.0, 2.0, 0), one push per frame in file order, positions rounded to 4 decimals: among the
    detections whose recorded id was also in the previous push, at most 0.5 % get another id than that pedestrian had
    then.  Measured: 11 / 5,005, 9 / 17,519 and 13 / 6,154 (0.22 %, 0.05 %, 0.21 %)."""
    pushes = _pushes(_rows(*rec))
    wrong, total = assoc_np.wrong_links(pushes, 1.0, 2.0, 0)
    print("%s: %d wrong links of %d (%.3f %%)" % (rec[1], wrong, total, 100.0 * wrong / total))
    assert total == measured[1]
    assert wrong <= 0.005 * total, (wrong, total)
