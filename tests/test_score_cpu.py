"""CPU: the scoring rule.  The restatement tests/score_np.py is pinned to the reference's best-of-K
ADE / FDE on a golden eth/test window; the C ABI declares, exports and refuses what it should before any launch; the host
side -- ScoreSpec, the thresholds, score_summary -- does its arithmetic."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
import score_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _window(e, i):
    starts = np.concatenate([[0], np.cumsum(e["num_peds"])])
    s, t = starts[i], starts[i + 1]
    return e["seq"][s:t], e["seq_rel"][s:t]                    # (V,2,20) each


@pytest.mark.parametrize("window", (0, 5))
def test_restatement_is_the_references_best_of_k(window):
    """A golden eth/test window as 20 pushes: its 8 observed frames, then the 12 target frames as the reference holds
    them (float64 running sums of the float32 displacements from the last observed position, metrics.py:66-75).  The
    prediction enqueued at the 8th push -- seeded V_pred, the K samples built from handed-in draws as test.py:59-91
    builds them -- retires at the 20th with traj_ade / traj_fde == oracle.best_of_k_errors_noise to 1e-9, every step
    matched.  The truth is kept in float64 here (truth32=False), as the reference's targets are: the rule's conversion
    of the truth to float32 moves an error by up to half a float32 ulp of the position (5e-7 at 10 m)."""
    from oracle import stgcnn_oracle as O
    e = load_golden("eth_test_windows.npz")
    seq, rel = _window(e, window)
    v, p, k = seq.shape[0], 12, 20
    assert v >= 2
    torch.manual_seed(7 + window)
    vp = torch.randn(p, v, 5) * 0.5
    eps = torch.stack([torch.randn(p, v, 2) for _ in range(k)])
    obs_last = seq[:, :, 7]
    target_rel = np.ascontiguousarray(np.transpose(rel[:, :, 8:], (2, 0, 1)))
    want_ade, want_fde = O.best_of_k_errors_noise(vp, obs_last, target_rel, eps)
    # the samples and the zero-noise trajectory as test.py builds them: float32 running sums from the last position
    sx, sy, rho = torch.exp(vp[..., 2]), torch.exp(vp[..., 3]), torch.tanh(vp[..., 4])
    cov = torch.stack([torch.stack([sx * sx, rho * sx * sy], -1), torch.stack([rho * sx * sy, sy * sy], -1)], -2)
    tril = torch.linalg.cholesky(cov)
    samples = np.stack([O.rel_to_abs((vp[..., :2] + (tril @ eps[j].unsqueeze(-1)).squeeze(-1)).numpy(), obs_last)
                        for j in range(k)])
    mean = O.rel_to_abs(vp[..., :2].numpy(), obs_last)
    tgt_abs = O.rel_to_abs(target_rel.astype(np.float64), obs_last)                       # (12,V,2) float64
    ids = np.arange(v, dtype=np.int64) * 3 + 11
    m = score_np.ScoreModel(p, v, k, decimals=None, truth32=False)
    idle = score_np.Prediction(np.zeros(v, np.int64), 0, np.zeros((p, v, 2)), np.zeros((5, p, v)), np.zeros((k, p, v, 2)))
    pred = score_np.Prediction(ids, v, mean, vp.permute(2, 0, 1).numpy(), samples)
    order = np.arange(v)[::-1]                                                            # detections in another order
    for f in range(20):
        xy = seq[:, :, f].astype(np.float64) if f < 8 else tgt_abs[f - 8]
        out = m.push(ids[order], xy[order], pred if f == 7 else idle)
        if f < 19:
            assert not out["traj_steps"].any()
    assert np.array_equal(out["traj_steps"], np.full(v, 12))
    assert np.abs(out["traj_ade"] - np.array(want_ade)).max() < 1e-9
    assert np.abs(out["traj_fde"] - np.array(want_fde)).max() < 1e-9
    assert m.traj_totals[0] == v and abs(m.traj_totals[1] - sum(want_ade)) < 1e-9 * v
    assert np.array_equal(m.totals[:, 0], np.full(12, v))


def test_restatement_branches():
    """By hand: a pedestrian missed at one step, a repeated id (the first detection wins), the truncation to m_max and
    the stream that is not pushed."""
    p, v = 2, 3
    m = score_np.ScoreModel(p, v, 0, thr=(2.0,), m_max=2, decimals=None, dtype=np.float32)
    mean = np.zeros((p, v, 2), np.float32)
    mean[:, 0] = (3, 4)
    mean[:, 1] = (1, 0)
    pr = score_np.Prediction([5, 9, 0], 2, mean, np.zeros((5, p, v)))
    none = score_np.Prediction([0, 0, 0], 0, mean, np.zeros((5, p, v)))
    assert not m.push([], np.zeros((0, 2)), pr)["matched"].any()
    o = m.push([5, 5, 9], [[0, 0], [3, 4], [1, 0]], none)          # 9 is past m_max = 2; the first 5 wins
    assert o["matched"].tolist() == [[1, 0, 0], [0, 0, 0]] and o["err"][0, 0] == 5 and o["d2"][0, 0] == 25
    assert o["nll"][0, 0] == np.float32(12.5) + np.float32(score_np.LOG_2PI)
    before = (m.totals.copy(), len(m.records))
    assert not m.push([5], [[0, 0]], None)["matched"].any() and len(m.records) == before[1]
    assert np.array_equal(m.totals, before[0])
    o = m.push([9, 5], [[1, 0], [3, 1]], none)                     # step 2: C = 2 I
    assert o["matched"].tolist() == [[0, 0, 0], [1, 1, 0]]
    assert o["err"][1].tolist() == [3, 0, 0] and o["d2"][1, 0] == 4.5
    assert o["traj_steps"].tolist() == [2, 1, 0] and o["traj_ade_mean"].tolist() == [4, 0, 0]
    assert o["traj_fde_mean"].tolist() == [3, 0, 0]
    assert m.totals[:, 0].tolist() == [1, 2] and m.totals[1, 5] == 1 and m.traj_totals.tolist() == [1, 0, 0, 4, 3]


def test_header_symbols_are_exported_and_the_abi_stays(L):
    from social_stgcnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    declared = set(re.findall(r"\b(stg_[a-z0-9_]+)\s*\(", hdr))
    assert {"stg_score_push", "stg_score_push_streams"} <= declared
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("stg_score_push", "stg_score_push_streams"):
        assert hasattr(raw, name), name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    for name, lim in (("V", 256), ("K", 64), ("P", 32), ("Q", 4)):
        assert re.search(r"#define STG_SCORE_MAX_%s %d\b" % (name, lim), hdr), name
    from social_stgcnn_amd import ops
    assert (ops.SCORE_MAX_V, ops.SCORE_MAX_K, ops.SCORE_MAX_P, ops.SCORE_MAX_Q) == (256, 64, 32, 4)


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    from social_stgcnn_amd import _lib
    f = ctypes.c_void_p(64)

    def structs(no_state=(), no_out=()):
        st = _lib.ScoreState(*[None if n in no_state else 64 for n, _ in _lib.ScoreState._fields_])
        so = _lib.ScoreOut(*[None if n in no_out else 64 for n, _ in _lib.ScoreOut._fields_])
        return ctypes.byref(st), ctypes.byref(so)

    def one(m_max=8, p=3, v=5, k=2, q=1, det=f, mean=f, samples=f, thr=f, no_state=(), no_out=(), count=f):
        st, so = structs(no_state, no_out)
        return L.stg_score_push(det, f, count, m_max, 1e4, mean, f, 60, 15, 5, 1, samples, f, f, p, v, k, st, thr, q,
                                so, None)

    def many(ns=3, m_total=16, id_stride=3, xy_stride=3, start=f, pushed=f, m_max=8, v=5):
        st, so = structs()
        return L.stg_score_push_streams(f, id_stride, f, xy_stride, m_total, start, pushed, ns, m_max, 1e4, f, f, 60,
                                        15, 5, 1, f, f, f, 3, v, 2, st, f, 1, so, None)
    einval = {"M_max=0": dict(m_max=0), "P=0": dict(p=0), "V=0": dict(v=0), "K<0": dict(k=-1), "Q<0": dict(q=-1),
              "null det_id": dict(det=None), "null det_count": dict(count=None), "null mean": dict(mean=None),
              "null thr": dict(thr=None), "null rec_cov": dict(no_state=("rec_cov",)),
              "null acc with K": dict(no_state=("acc",)), "null totals": dict(no_state=("totals",)),
              "null err": dict(no_out=("err",)), "null best with K": dict(no_out=("best",)),
              "misaligned mean": dict(mean=ctypes.c_void_p(68))}
    for name, kw in einval.items():
        assert one(**kw) == -1, name
        assert b"stg_score_push" in L.stg_last_error(), name
    unsupported = {"V": dict(v=257), "K": dict(k=65), "P": dict(p=33), "Q": dict(q=5), "M_max": dict(m_max=2049)}
    for name, kw in unsupported.items():
        assert one(**kw) == _lib.EUNSUPPORTED, name
        assert name.encode() in L.stg_last_error(), name
    for name, kw in {"NS<0": dict(ns=-1), "M_total<0": dict(m_total=-1), "id_stride=0": dict(id_stride=0),
                     "xy_stride=1": dict(xy_stride=1), "null det_start": dict(start=None),
                     "null pushed": dict(pushed=None), "V=0": dict(v=0)}.items():
        assert many(**kw) == -1, name
        assert b"stg_score_push_streams" in L.stg_last_error(), name
    for name, kw in {"NS": dict(ns=4097), "M_total": dict(m_total=(1 << 23) + 1), "M_max": dict(m_max=4096),
                     "V": dict(v=300)}.items():
        assert many(**kw) == _lib.EUNSUPPORTED, name
    assert many(ns=0, start=None) == 0                          # no streams: a no-op, nothing is looked at


SHARED_REFUSALS = {           # case -> (arguments, status, the message behind the entry point's name)
    "null mean": (dict(mean=None), -1, ": null pointer (mean / v_pred / ids / num_peds)"),
    "misaligned samples": (dict(samples=ctypes.c_void_p(68)), -1,
                           ": mean / samples and their records must be 8-byte aligned"),
    "null thr with Q": (dict(thr=None), -1, ": null pointer (thr with Q=1)"),
    "V": (dict(v=257), "EUNSUPPORTED", ": V=257 above STG_SCORE_MAX_V=256"),
    "K": (dict(k=65), "EUNSUPPORTED", ": K=65 above STG_SCORE_MAX_K=64"),
    "P": (dict(p=33), "EUNSUPPORTED", ": P=33 above STG_SCORE_MAX_P=32"),
    "Q": (dict(q=5), "EUNSUPPORTED", ": Q=5 above STG_SCORE_MAX_Q=4"),
}


@pytest.mark.parametrize("entry", ("stg_score_push", "stg_score_push_streams", "stg_score_push_timed",
                                   "stg_score_push_streams_timed"))
def test_the_four_entry_points_share_their_refusals(L, entry):
    """What the push-indexed and the time-indexed pair check in one place (score_fn.hpp) comes back from each of the
    four with the same status and the same words behind its own name, before any launch: every pointer is 64 or 68."""
    from social_stgcnn_amd import _lib
    f = ctypes.c_void_p(64)
    timed = entry.endswith("_timed")
    kinds = (_lib.ScoreTimedState, _lib.ScoreTimedOut) if timed else (_lib.ScoreState, _lib.ScoreOut)

    def call(mean=f, samples=f, thr=f, p=3, v=5, k=2, q=1):
        st, so = (cls(*[64] * len(cls._fields_)) for cls in kinds)
        tail = (mean, f, 60, 15, 5, 1, samples, f, f, p, v, k) + ((6,) if timed else ()) + \
            (ctypes.byref(st), thr, q, ctypes.byref(so), None)
        head = {"stg_score_push": (f, f, f, 8, 1e4), "stg_score_push_streams": (f, 3, f, 3, 16, f, f, 3, 8, 1e4),
                "stg_score_push_timed": (f, f, f, f, f, f, 8, 4, 1e4, 10, 10),
                "stg_score_push_streams_timed": (f, f, f, f, f, f, f, 3, 8, 4, 1e4, 10, 10)}[entry]
        return getattr(L, entry)(*head, *tail)
    for name, (kw, status, words) in SHARED_REFUSALS.items():
        assert call(**kw) == (_lib.EUNSUPPORTED if status == "EUNSUPPORTED" else status), name
        assert L.stg_last_error().decode().endswith(entry + words), (name, L.stg_last_error())


def test_score_spec_and_thresholds():
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.predict import ScoreSpec
    s = ScoreSpec()
    assert s.levels == (0.5, 0.9, 0.99) and s.best_of_k is True
    assert s.thresholds == pytest.approx([2 * math.log(2), 2 * math.log(10), 2 * math.log(100)], rel=1e-15)
    # the chi-square law with two degrees of freedom: P(d2 <= thr) = 1 - exp(-thr / 2)
    for level, thr in zip(s.levels, s.thresholds):
        assert 1 - math.exp(-thr / 2) == pytest.approx(level, rel=1e-14)
    draws = np.random.default_rng(0).normal(size=(200000, 2))
    assert np.mean((draws ** 2).sum(1) <= s.thresholds[1]) == pytest.approx(0.9, abs=3e-3)
    assert ScoreSpec((), False) == ((), False) and ScoreSpec((), False).thresholds == []
    assert ScoreSpec([0.25]).levels == (0.25,)
    for bad in ((0.0,), (1.0,), (-0.1,), (0.1, 0.2, 0.3, 0.4, 0.5), (float("nan"),)):
        with pytest.raises(ValueError, match="level"):
            ScoreSpec(bad)
    with pytest.raises(ValueError, match="best_of_k"):
        ScoreSpec((0.5,), 1)
    with pytest.raises(ValueError, match="limit"):
        ops.score_state(1, 12, 257, 20, "cpu")
    st = ops.score_state(2, 12, 128, 20, "meta")
    per_stream = sum(x.numel() * x.element_size() for n, x in zip(st._fields, st)
                     if n not in ("totals", "traj_totals", "head", "rec_peds")) // 2
    assert per_stream == 12 * 128 * (8 + 20 * 12 + 8 * 20 * 12 + 4 * 20 + 8) and 3.4e6 < per_stream < 3.6e6
    lean = ops.score_state(1, 12, 128, 20, "meta", samples=False)
    assert lean.rec_samples is None and lean.acc is None and lean.totals.shape == (1, 12, 8)
    assert sum(x.numel() * x.element_size() for x in lean if x is not None) < 0.41e6


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_live_predictors_refuse_best_of_k_without_samples():
    """Decided from the arguments, ahead of any device work."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import RiskSpec, ScoreSpec
    for make in (lambda **kw: frames.FramePredictor(_Model(), **kw),
                 lambda **kw: frames.StreamsPredictor(_Model(), 3, **kw)):
        with pytest.raises(ValueError, match="keep_samples=False"):
            make(risk=RiskSpec(0.5), keep_samples=False, score=ScoreSpec())
        with pytest.raises(ValueError, match="k <= 64"):
            make(k=65, score=ScoreSpec())
        with pytest.raises(ValueError, match="max_peds=300"):
            make(max_peds=300, score=ScoreSpec((0.5,), False))


def test_score_summary_arithmetic():
    from social_stgcnn_amd import frames
    levels = (0.5, 0.9)
    tot = np.zeros((2, 3, 7))
    tot[0, 0] = (4, 2.0, 8.0, 6.0, 1.0, 2, 4)
    tot[0, 2] = (1, 0.5, 3.0, 2.5, 0.25, 0, 1)
    trj = np.array([[2, 1.0, 3.0, 1.5, 4.0], [0, 0, 0, 0, 0]], np.float64)
    s = frames.score_summary(torch.from_numpy(tot), torch.from_numpy(trj), levels)
    assert s.count.tolist() == [[4, 0, 1], [0, 0, 0]] and s.levels == levels
    assert s.err[0, 0] == 0.5 and s.d2[0, 0] == 2.0 and s.nll[0, 0] == 1.5 and s.best[0, 0] == 0.25
    assert s.coverage[0, 0].tolist() == [0.5, 1.0] and s.coverage[0, 2].tolist() == [0.0, 1.0]
    assert np.isnan(s.err[0, 1]) and np.isnan(s.coverage[1]).all() and np.isnan(s.ade[1])
    assert (s.trajectories.tolist(), s.ade[0], s.fde[0], s.ade_mean[0], s.fde_mean[0]) == ([2, 0], 0.5, 1.5, 0.75, 2.0)
    with pytest.raises(ValueError, match="totals"):
        frames.score_summary(tot, trj, (0.5,))
    with pytest.raises(ValueError, match="traj_totals"):
        frames.score_summary(tot, trj[:1], levels)
