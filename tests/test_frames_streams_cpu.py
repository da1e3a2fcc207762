"""CPU: the host side of frames.StreamsPredictor -- packing one tick of many streams (frames.pack_tick) and every
refusal, raised before any device work (this machine needs no GPU for them)."""
import numpy as np
import pytest
import torch


def _model():
    from social_stgcnn_amd.model import social_stgcnn
    return social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)


def test_pack_tick_mapping():
    from social_stgcnn_amd.frames import pack_tick
    pk = pack_tick({3: ([9, 2], [[1.5, 2.5], [3.0, 4.0]]), 0: (np.array([7]), np.array([[5.0, 6.0]])),
                    1: ([], np.zeros((0, 2))), 4: None}, 5, 8, 100)
    assert pk.det_start.dtype == np.int32 and pk.det_start.tolist() == [0, 1, 1, 1, 3, 3]
    assert pk.pushed.dtype == np.int32 and pk.pushed.tolist() == [1, 1, 0, 1, 0]       # 1: an empty push; 4: None
    assert pk.ids.dtype == np.int64 and pk.ids.tolist() == [7, 9, 2]                   # stream order, detection order
    assert pk.xy.dtype == np.float64 and pk.xy.tolist() == [[5, 6], [1.5, 2.5], [3, 4]]
    assert pk.xy.flags.c_contiguous


def test_pack_tick_sequence():
    from social_stgcnn_amd.frames import pack_tick
    tick = [None, (np.array([4, 1.0, 3]), np.arange(6.0).reshape(3, 2)),
            (torch.tensor([4]), torch.tensor([[7.0, 8.0]])), (np.zeros(0), np.zeros((0, 2))), None]
    pk = pack_tick(tick, 5, 8, 100)
    assert pk.det_start.tolist() == [0, 0, 3, 4, 4, 4]
    assert pk.pushed.tolist() == [0, 1, 1, 1, 0]
    assert pk.ids.tolist() == [4, 1, 3, 4]                          # the same id in two streams: two tracks
    assert pk.xy.tolist() == [[0, 1], [2, 3], [4, 5], [7, 8]]
    pk = pack_tick([None] * 3, 3, 8, 100)                           # nobody pushed
    assert pk.det_start.tolist() == [0, 0, 0, 0] and pk.pushed.tolist() == [0, 0, 0]
    assert pk.ids.shape == (0,) and pk.xy.shape == (0, 2)
    pk = pack_tick({}, 2, 8, 100)
    assert pk.pushed.tolist() == [0, 0] and pk.det_start.tolist() == [0, 0, 0]


def test_pack_tick_refusals():
    from social_stgcnn_amd.frames import pack_tick
    ok = (np.array([1, 2]), np.zeros((2, 2)))
    cases = [({5: ok}, "stream index"), ({-1: ok}, "stream index"), ({True: ok}, "stream index"),
             ({"a": ok}, "stream index"), ([ok] * 4, "4 entries for 5 streams"),
             ({0: (np.arange(9), np.zeros((9, 2)))}, "stream 0: 9 detections > max_detections=8"),
             ({2: ([1, 2], np.zeros((3, 2)))}, "stream 2: 2 ids but 3 positions"),
             ({1: ([3, 4, 3], np.zeros((3, 2)))}, "stream 1: duplicate pedestrian id 3"),
             ({0: ok, 1: ([1.5], np.zeros((1, 2)))}, "integral"), ({3: ([-1], np.zeros((1, 2)))}, ">= 0"),
             ({0: (np.arange(8), np.zeros((8, 2))), 4: (np.arange(8), np.zeros((8, 2)))}, "16 detections > "
                                                                                          "max_total_detections=12"),
             ({0: (np.arange(3),)}, r"\(ids, xy\) expected")]
    for tick, msg in cases:
        with pytest.raises(ValueError, match=msg):
            pack_tick(tick, 5, 8, 12)
    # the same ids in different streams are no duplicate
    assert pack_tick({0: ok, 1: ok}, 5, 8, 12).ids.tolist() == [1, 2, 1, 2]
    # ids too wide to share one sort key with the stream index take the two-key sort: same answers
    big = np.array([2 ** 62, 5], np.int64)
    both = pack_tick({0: (big, np.zeros((2, 2))), 3: (big, np.zeros((2, 2)))}, 5, 8, 12)
    assert both.ids.tolist() == [2 ** 62, 5] * 2
    with pytest.raises(ValueError, match="stream 3: duplicate pedestrian id %d" % 2 ** 62):
        pack_tick({0: (big, np.zeros((2, 2))), 3: (big[[0, 1, 0]], np.zeros((3, 2)))}, 5, 8, 12)


def test_streams_predictor_refuses_bad_arguments_before_device_work():
    from social_stgcnn_amd.frames import StreamsPredictor
    m = _model()
    for kw, msg in ((dict(streams=0), "streams"), (dict(streams=4097), "streams"), (dict(streams=2.5), "streams"),
                    (dict(streams=True), "streams"), (dict(streams=2, capacity=0), "capacity"),
                    (dict(streams=2, capacity=4096), "capacity"), (dict(streams=2, max_detections=0), "max_detections"),
                    (dict(streams=2, max_detections=4096), "max_detections"), (dict(streams=2, max_peds=0), "max_peds"),
                    (dict(streams=2, obs_len=0), "obs_len"), (dict(streams=2, obs_len=9), "obs_len=9"),
                    (dict(streams=2, decimals=16), "decimals"), (dict(streams=2, max_total_detections=0),
                                                                 "max_total_detections"),
                    (dict(streams=2, max_total_detections=(1 << 23) + 1), "max_total_detections"),
                    (dict(streams=2, block_threads=128), "block_threads")):
        with pytest.raises(ValueError, match=msg):
            StreamsPredictor(m, **kw)
    # valid arguments never fall back to the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StreamsPredictor(m, 2)
