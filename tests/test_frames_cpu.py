"""CPU: the frame-scene rule of social_stgcnn_amd.frames, restated in numpy (tests/frames_np.py), against the reference's
windowing as data.load_windows pins it; the scene counts of the committed recordings; host-side validation of the
recording builder and of a live push; argument checks of the three entry points without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
import frames_np

DATA = os.path.join(GOLDEN, "data")
# recording: (frames, dataset windows, frame scenes with >= 1 pedestrian, largest frame scene,
#             frames whose scene has exactly a dataset window's pedestrian set)
TABLE = {("eth_test", "biwi_eth.txt"): (876, 70, 725, 20, 11),
         ("univ_test", "students001.txt"): (444, 425, 437, 73, 0),
         ("zara1_test", "crowds_zara01.txt"): (872, 602, 838, 18, 186),
         ("zara2_test", "crowds_zara02.txt"): (1052, 921, 1039, 17, 174)}


def _rows(d, f):
    from social_stgcnn_amd import data
    return data.read_file(os.path.join(DATA, d, f))


def all_recordings():
    return sorted((d, f) for d in os.listdir(DATA) for f in os.listdir(os.path.join(DATA, d)))


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("rec", sorted(TABLE))
def test_restatement_agrees_with_the_dataset_windows(rec):
    """Every window data.load_windows keeps comes from the restated window rule, its pedestrians are in the frame
    scene at its last observed frame with the window's float64 positions, and where the two sets are equal the whole
    frame scene is the window's observed part, bit for bit."""
    from social_stgcnn_amd import data
    rows = _rows(*rec)
    win = data.load_windows(os.path.join(DATA, rec[0]), 8, 12, 1, with_non_linear=False, files=[rec[1]])
    starts = frames_np.dataset_windows(rows)
    scenes = {s[0]: s for s in frames_np.frame_scenes(rows)}
    assert len(starts) == len(win)
    equal = 0
    for w, (idx, ids) in enumerate(starts):
        s0, e0 = win.seq_start_end[w]
        obs_w = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))                    # (8, V_w, 2) float64
        _, _, sid, sobs = scenes[idx + 7]
        at = np.searchsorted(sid, ids)
        assert np.array_equal(sid[at], ids)
        assert np.array_equal(sobs[:, at], obs_w)
        if np.array_equal(sid, ids):
            assert np.array_equal(sobs, obs_w)
            equal += 1
    assert equal == TABLE[rec][4]


@pytest.mark.parametrize("rec", sorted(TABLE))
def test_restatement_scene_counts(rec):
    rows = _rows(*rec)
    sc = frames_np.frame_scenes(rows)
    nf, nw, ns, vmax, _ = TABLE[rec]
    assert len(np.unique(rows[:, 0])) == nf
    assert len(frames_np.dataset_windows(rows)) == nw
    assert len(sc) == ns
    assert max(len(s[2]) for s in sc) == vmax
    assert all(len(s[2]) >= 1 and np.all(np.diff(s[2]) > 0) for s in sc)


def test_rounding_is_rint_times_ten_thousand_over_ten_thousand():
    """What the kernels compute, rint(x * 1e4) / 1e4 in float64, is np.around(x, 4) on every committed recording."""
    from social_stgcnn_amd.frames import _scale
    assert _scale(4) == 1e4 and _scale(None) == 0.0
    for rec in all_recordings():
        xy = _rows(*rec)[:, 2:4]
        assert np.array_equal(np.around(xy, 4), np.rint(xy * _scale(4)) / _scale(4)), rec
    assert len(all_recordings()) == 14


def test_sorted_rows_orders_by_frame_then_id():
    from social_stgcnn_amd.frames import sorted_rows
    rows = np.array([[20, 3, 1.0, 2.0], [10, 5, 3.0, 4.0], [10, 2, 5.0, 6.0], [30, 2, 7.0, 8.0], [20, 2, 9.0, 1.0]])
    frames, fs, ids, xy = sorted_rows(rows)
    assert frames.tolist() == [10, 20, 30]
    assert fs.dtype == np.int32 and fs.tolist() == [0, 2, 4, 5]
    assert ids.dtype == np.int64 and ids.tolist() == [2, 5, 2, 3, 2]
    assert xy.tolist() == [[5, 6], [3, 4], [9, 1], [1, 2], [7, 8]]


def test_recording_validation():
    from social_stgcnn_amd.frames import recording_scenes, sorted_rows
    rows = _rows("eth_test", "biwi_eth.txt")
    dup = np.concatenate([rows, rows[5:6]])
    with pytest.raises(ValueError, match="duplicate"):
        sorted_rows(dup)
    with pytest.raises(ValueError, match="duplicate"):
        recording_scenes(dup, "cpu")
    frac = rows.copy()
    frac[3, 1] += 0.5
    with pytest.raises(ValueError, match="integral"):
        recording_scenes(frac, "cpu")
    neg = rows.copy()
    neg[3, 1] = -1
    with pytest.raises(ValueError, match=">= 0"):
        sorted_rows(neg)
    for bad in (0, 33, 2.5, -1, True):
        with pytest.raises(ValueError, match="obs_len"):
            recording_scenes(rows, "cpu", obs_len=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="min_peds"):
            recording_scenes(rows, "cpu", min_peds=bad)
    for bad in (-1, 2.5, 16):
        with pytest.raises(ValueError, match="decimals"):
            recording_scenes(rows, "cpu", decimals=bad)
    with pytest.raises(ValueError, match=r"\(M,4\)"):
        sorted_rows(rows[:, :3])
    # a valid call never falls back to the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        recording_scenes(rows, "cpu")


def test_push_validation():
    from social_stgcnn_amd.frames import host_detections
    ids, xy = host_detections([3, 1.0, 7], [[0, 1], [2, 3], [4, 5]], 3)
    assert ids.dtype == np.int64 and ids.tolist() == [3, 1, 7] and xy.dtype == np.float64 and xy.shape == (3, 2)
    with pytest.raises(ValueError, match="max_detections"):
        host_detections(np.arange(5), np.zeros((5, 2)), 4)
    with pytest.raises(ValueError, match="duplicate"):
        host_detections([1, 2, 1], np.zeros((3, 2)), 8)
    with pytest.raises(ValueError, match="integral"):
        host_detections([1, 2.5], np.zeros((2, 2)), 8)
    with pytest.raises(ValueError, match="positions"):
        host_detections([1, 2], np.zeros((3, 2)), 8)
    ids, xy = host_detections([], np.zeros((0, 2)), 8)
    assert ids.shape == (0,) and xy.shape == (0, 2)


def test_stream_restatement_edge_cases():
    """The push-by-push statement: a gap drops a track until it has obs_len consecutive frames again; a repeated id
    keeps its first detection; the smallest max_peds ids are kept."""
    m = frames_np.StreamModel(obs_len=3, max_peds=2)
    outs = [m.push([5, 1], [[0.5, 0], [1, 0]]), m.push([1, 5], [[1, 1], [0.5, 1]]),
            m.push([5, 1, 5, 9], [[0.5, 2], [1, 2], [9, 9], [9, 0]])]
    assert len(outs[0][0]) == 0 and len(outs[1][0]) == 0
    assert outs[2][0].tolist() == [1, 5]
    assert outs[2][1][:, 1].tolist() == [[0.5, 0], [0.5, 1], [0.5, 2]]
    assert m.push([9, 1], [[0, 0], [0, 0]])[0].tolist() == [1]          # 5 missing; 9 only twice
    assert m.push([9, 1, 5], np.zeros((3, 2)))[0].tolist() == [1, 9]


def test_entry_points_reject_bad_arguments_without_a_gpu(L):
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call

    def push(m_max=8, s=16, t=8, v=4, det=f):
        return L.stg_track_push(det, f, f, m_max, f, f, f, f, s, t, 1e4, v, f, f, f, None)
    cases = {"M_max=0": dict(m_max=0), "M_max too large": dict(m_max=4096), "S=0": dict(s=0),
             "S too large": dict(s=4096), "T_obs=0": dict(t=0), "T_obs=33": dict(t=33), "V=0": dict(v=0),
             "null det_id": dict(det=None)}
    for name, kw in cases.items():
        assert push(**kw) == -1, name
        assert b"stg_track_push" in L.stg_last_error(), name
    assert L.stg_frame_scene_counts(f, f, -1, 8, f, None) == -1
    assert L.stg_frame_scene_counts(f, f, 4, 0, f, None) == -1
    assert L.stg_frame_scene_counts(None, None, 0, 8, None, None) == 0          # F == 0: nothing to launch
    assert L.stg_frame_scenes(f, f, f, f, 2, 0, 8, 1e4, f, f, f, None) == -1
    assert L.stg_frame_scenes(f, None, f, f, 2, 4, 8, 1e4, f, f, f, None) == -1
    assert b"null" in L.stg_last_error()
    assert L.stg_frame_scenes(None, None, None, None, 0, 4, 8, 1e4, None, None, None, None) == 0
