"""CPU: the time-indexed scoring rule.  The restatement tests/score_time_np.py on a hand-worked case
with every value written out; its anchor -- fed on the grid it IS the push-indexed rule of tests/score_np.py -- on a golden
eth/test window, down to the reference's best-of-K ADE / FDE; eviction, a refused push, the exact scripts the GPU tests
run reaching their branches; the C ABI declares, exports and refuses what it should before any launch; TimedScoreSpec and
the live predictors check their arguments."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
import score_np
import score_time_inputs as sti
from frames_time_np import OVERFLOW, TIME_ORDER, StreamModelTimed
from score_time_np import TABLES, TRAJ, TimedScoreModel, truth_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _same(a, b):
    """Deep bit-for-bit equality of nested dicts / lists / arrays / scalars."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def _snapshot(m):
    return copy.deepcopy((m.rows, m.accepted, m.evictions, m.totals, m.traj_totals))


def test_truth_at_by_hand():
    smp = [(0, 1.0, 2.0), (5, 2.0, 4.0), (15, 4.0, 0.0)]
    assert truth_at(smp, 15, 10, None)[1].tolist() == [4.0, 0.0]                 # a sample at the instant: as it is
    assert truth_at(smp, 10, 10, None)[1].tolist() == [3.0, 2.0]                 # half way between the two newest
    assert truth_at(smp, 7, 10, None)[1].tolist() == [2.0 + 2.0 * 0.2, 4.0 + -4.0 * 0.2]
    assert truth_at(smp, 10, 9, None) == ("wide", None)                          # the bracket is wider than max_dt
    assert truth_at(smp, 5, 10, None) == (None, None) and truth_at(smp, 3, 10, None) == (None, None)    # older brackets
    assert truth_at(smp, 16, 10, None) == (None, None) and truth_at(smp[:1], 0, 10, None)[0] == "hit"
    assert truth_at(smp[:1], -1, 10, None) == (None, None)
    assert truth_at([(0, 0.0, 0.0), (3, 1.0, 1.0)], 1, 4, 4)[1].tolist() == [0.3333, 0.3333]            # rounded


def test_restatement_by_hand():
    """step 10, max_dt 20 = 2 step, P 3, K 1, one threshold (2.0), float32, no rounding.  The prediction made at t = 0
    holds four pedestrians; every later push enqueues an empty scene.  C_h = h I.
      id 1  on the grid: a sample at t = 10 (h = 1); the bracket (10, 30) of width 20 holds tau = 20 (h = 2,
            interpolated half way) and ends on tau = 30 (h = 3): all three at the push of t = 30 but the first
      id 2  between two samples: (5, 15) holds tau = 10
      id 3  samples at 0 and 25: the bracket is wider than max_dt, tau = 10 and 20 stay unmatched for good
      id 4  samples at 5 and 25: ONE bracket of width 20 holds tau = 10 and tau = 20, two horizons of the record"""
    p, v, k = 3, 4, 1
    track = StreamModelTimed(8, 10, 20, 4, 2, 3, v, None, 8, 8)
    m = TimedScoreModel(p, v, k, 10, 20, 8, thr=(2.0,), decimals=None, dtype=F)
    mean = np.zeros((p, v, 2), F)
    mean[:, 0] = [(4, 4), (2, 5), (3, 0)]           # truths (1,0), (2,0), (3,0): offsets (3,4), (0,5), (0,0)
    mean[0, 1] = (0, 4)                             # truth (0,4): offset 0
    mean[:, 2] = 9
    mean[:2, 3] = [(11, 6), (8, 6)]                 # truths (8,2), (8,6): offsets (3,4), (0,0)
    truth = np.zeros((p, v, 2), F)
    truth[:, 0], truth[0, 1], truth[:2, 3] = [(1, 0), (2, 0), (3, 0)], (0, 4), [(8, 2), (8, 6)]
    samples = (truth + 2 * (mean - truth))[None]    # twice the mean's offset: best = 2 err
    first = score_np.Prediction([1, 2, 3, 4], 4, mean, np.zeros((5, p, v)), samples)
    idle = score_np.Prediction([0] * v, 0, np.zeros((p, v, 2)), np.zeros((5, p, v)), np.zeros((k, p, v, 2)))
    feed = [(0, [1, 2, 3, 4], [(0, 0), (0, 0), (0, 0), (0, 0)]), (5, [2, 4], [(0, 2), (8, 0)]), (10, [1], [(1, 0)]),
            (15, [2], [(0, 6)]), (25, [3, 4], [(5, 5), (8, 8)]), (30, [1], [(3, 0)])]
    outs = []
    for n, (t, ids, xy) in enumerate(feed):
        assert track.push(ids, xy, t)[3] == 0
        outs.append(m.push(track.tracks, t, first if n == 0 else idle))
    rec = m.rows[0]
    log2pi = F(score_np.LOG_2PI)
    assert rec["t"] == 0 and rec["status"] == "retired" and [r["status"] for r in m.rows[1:6]] == ["pending"] * 5
    assert rec["matched"].tolist() == [[1, 1, 0, 1], [1, 0, 0, 1], [1, 0, 0, 0]]
    assert rec["err"].tolist() == [[5, 0, 0, 5], [5, 0, 0, 0], [0, 0, 0, 0]]
    assert rec["best"].tolist() == [[10, 0, 0, 10], [10, 0, 0, 0], [0, 0, 0, 0]]
    assert rec["d2"].tolist() == [[25, 0, 0, 25], [12.5, 0, 0, 0], [0, 0, 0, 0]]
    half_log = lambda x: F(F(0.5) * F(np.log(np.float64(x))))                    # noqa: E731
    assert rec["nll"][0].tolist() == [F(12.5) + log2pi, log2pi, 0, F(12.5) + log2pi]
    assert rec["nll"][1].tolist() == [F(F(6.25) + half_log(4)) + log2pi, 0, 0, F(half_log(4)) + log2pi]
    assert rec["nll"][2].tolist() == [F(half_log(9)) + log2pi, 0, 0, 0]
    assert rec["steps"].tolist() == [3, 1, 0, 2] and rec["traj_steps"].tolist() == [3, 1, 0, 2]
    assert rec["traj_ade_mean"].tolist() == [F(10) / F(3), 0, 0, 2.5] and rec["traj_fde_mean"].tolist() == [0, 0, 0, 0]
    assert rec["traj_ade"].tolist() == [F(20) / F(3), 0, 0, 5] and rec["traj_fde"].tolist() == [0, 0, 0, 0]
    # what each push added: nothing at t = 0 and 5; id 1 at 10; id 2 at 15; id 4 twice at 25; id 1 twice at 30
    assert not outs[0]["push_totals"].any() and not outs[1]["push_totals"].any()
    assert outs[2]["push_totals"][:, :3].tolist() == [[1, 5, 25], [0, 0, 0], [0, 0, 0]]
    assert outs[3]["push_totals"][0].tolist() == [1, 0, 0, float(log2pi), 0, 1]
    assert outs[4]["push_totals"][:, [0, 1, 2, 4, 5]].tolist() == [[1, 5, 25, 10, 0], [1, 0, 0, 0, 1], [0, 0, 0, 0, 0]]
    assert outs[5]["push_totals"][:, [0, 1, 2, 4, 5]].tolist() == [[0, 0, 0, 0, 0], [1, 5, 12.5, 10, 0], [1, 0, 0, 0, 1]]
    assert all(not o["push_traj"].any() for o in outs[:5])
    assert outs[5]["push_traj"].tolist() == [1, float(F(20) / F(3)), 0, float(F(10) / F(3)), 0]
    assert m.totals[:, 0].tolist() == [3, 2, 1] and m.totals[:, 1].tolist() == [10, 5, 0]
    assert m.totals[:, 5].tolist() == [1, 1, 1] and np.array_equal(m.traj_totals, outs[5]["push_traj"])
    assert np.array_equal(m.totals, sum(o["push_totals"] for o in outs))
    assert m.accepted == 6 and m.evictions == 0
    # a stream that is not pushed: nothing moves
    before = _snapshot(m)
    assert not m.push(track.tracks, 40, None)["push_totals"].any() and _same(before, _snapshot(m))


def _window(e, i):
    starts = np.concatenate([[0], np.cumsum(e["num_peds"])])
    s, t = starts[i], starts[i + 1]
    return e["seq"][s:t], e["seq_rel"][s:t]                    # (V,2,20) each


@pytest.mark.parametrize("window", (0, 5))
def test_fed_on_the_grid_it_is_the_push_indexed_rule(window):
    """The anchor.  A golden eth/test window as 20 pushes at t = 10 f with step 10 and max_dt = step, as
    test_score_cpu.py feeds score_np: every push enqueues a prediction here (seeded, the one of the 8th push the window's
    own).  The entries (record of push m, horizon h) equal what score_np reports at push m + h in row h - 1, the retired
    rows its traj_* of push m + P, bit for bit in float64, and the totals agree; the window's own record retires with
    traj_ade / traj_fde == oracle.best_of_k_errors_noise to 1e-9 (the truth kept in float64, as there)."""
    from oracle import stgcnn_oracle as O
    e = load_golden("eth_test_windows.npz")
    seq, rel = _window(e, window)
    v, p, k = seq.shape[0], 12, 20
    torch.manual_seed(7 + window)
    vp = torch.randn(p, v, 5) * 0.5
    eps = torch.stack([torch.randn(p, v, 2) for _ in range(k)])
    obs_last = seq[:, :, 7]
    target_rel = np.ascontiguousarray(np.transpose(rel[:, :, 8:], (2, 0, 1)))
    want_ade, want_fde = O.best_of_k_errors_noise(vp, obs_last, target_rel, eps)
    sx, sy, rho = torch.exp(vp[..., 2]), torch.exp(vp[..., 3]), torch.tanh(vp[..., 4])
    cov = torch.stack([torch.stack([sx * sx, rho * sx * sy], -1), torch.stack([rho * sx * sy, sy * sy], -1)], -2)
    tril = torch.linalg.cholesky(cov)
    samples = np.stack([O.rel_to_abs((vp[..., :2] + (tril @ eps[j].unsqueeze(-1)).squeeze(-1)).numpy(), obs_last)
                        for j in range(k)])
    mean = O.rel_to_abs(vp[..., :2].numpy(), obs_last)
    tgt_abs = O.rel_to_abs(target_rel.astype(np.float64), obs_last)
    ids = np.arange(v, dtype=np.int64) * 3 + 11
    gen = np.random.default_rng(window)
    preds = [score_np.Prediction(ids, v, mean + F(0.01 * f), gen.normal(0, 0.5, (5, p, v)),
                                 samples + gen.normal(0, 0.3, samples.shape)) for f in range(20)]
    preds[7] = score_np.Prediction(ids, v, mean, vp.permute(2, 0, 1).numpy(), samples)
    timed = TimedScoreModel(p, v, k, 10, 10, 20, thr=(1.0, 4.0), decimals=None, truth32=False)
    track = StreamModelTimed(8, 10, 10, 4, 2, 3, v, None, 64, 64)
    untimed = score_np.ScoreModel(p, v, k, (1.0, 4.0), 64, None, truth32=False)
    order = np.arange(v)[::-1]
    for f in range(20):
        xy = seq[:, :, f].astype(np.float64) if f < 8 else tgt_abs[f - 8]
        assert track.push(ids[order], xy[order], 10 * f)[3] == 0
        added = timed.push(track.tracks, 10 * f, preds[f])
        out = untimed.push(ids[order], xy[order], preds[f])
        for h in range(1, min(f, p) + 1):
            rec = timed.rows[f - h]
            for name in TABLES:
                assert _same(rec[name][h - 1], out[name][h - 1].astype(rec[name].dtype)), (f, h, name)
        assert np.array_equal(added["push_totals"][:, 0], out["matched"].sum(axis=1))
        if f >= p:
            rec = timed.rows[f - p]
            assert rec["status"] == "retired"
            for name in TRAJ:
                assert _same(rec[name], out[name].astype(rec[name].dtype)), (f, name)
    assert np.allclose(timed.totals, untimed.totals, rtol=1e-12, atol=0) and timed.totals[:, 0].sum() > 100
    assert np.allclose(timed.traj_totals, untimed.traj_totals, rtol=1e-12, atol=0) and timed.traj_totals[0] == 8 * v
    rec = timed.rows[7]
    assert np.array_equal(rec["traj_steps"], np.full(v, 12))
    assert np.abs(rec["traj_ade"] - np.array(want_ade)).max() < 1e-9
    assert np.abs(rec["traj_fde"] - np.array(want_fde)).max() < 1e-9


def _run_script(s, p, v, k, pending, r, thr=(0.75, 3.0, 8.0)):
    ref = sti.StreamRef(p, v, k, thr, pending, r)
    flags, refused = 0, 0
    for t, ids, xy, pred, back in sti.script(s, p, v, k):
        before = (_snapshot(ref.score), ref.track.state()) if back else None
        f, _ = ref.push(t, ids, xy, pred)
        assert bool(f & TIME_ORDER) == back
        if back:                                                # a refused push leaves everything as it was
            assert _same(before[0], _snapshot(ref.score)) and before[1] == ref.track.state()
            refused += 1
        flags |= f
    assert refused == 1
    return ref, flags


def test_the_ring_of_two_script_reaches_what_the_gpu_test_needs():
    """Rings of two samples through the three statements: scene positions, scored entries and harvested frames that are
    interpolated from the only bracket such a ring holds, and windows of nine frames in the log."""
    import harvest_time_np as HT
    p, v, k = 3, 8, 2
    ref = sti.StreamRef(p, v, k, (0.75, 3.0), 4, 2, slots=16)
    hv = HT.TimedHarvester(1, 9, sti.STEP, sti.MAX_DT, 0, 32, 256)
    script = sti.ring2_script(p, v, k)
    in_scene = 0
    for t, ids, xy, pred in script:
        assert ref.push(t, ids, xy, pred)[0] == 0
        assert all(len(smp) <= 2 for smp in ref.track.tracks.values())
        in_scene += sti.interpolated_in_scene(ref.scene, ref.track.tracks, t)
        hv.tick({0: (ref.track.state()[0], t, True)})
    assert in_scene == 38 and sti.interpolated_in_records(ref.score.rows, [e[0] for e in script]) == 15
    assert hv.log.header.tolist() == [14, 64, 0] and hv.hist[0].interpolated > 0 and hv.hist[0].clock == [1, -20, 0]


def test_scripts_reach_their_branches():
    """What test_gpu_score_time.py relies on, checked where it is cheap: the exact scripts reach every branch of the
    rule, and their distances are exact in float32 (the float64 restatement gives the same numbers)."""
    p, v, k = 12, 5, 2
    ref, flags = _run_script(0, p, v, k, 60, 8)
    m = ref.score
    assert flags & OVERFLOW and m.evictions == 0 and m.accepted == 60
    retired = [r for r in m.rows if r is not None and r["status"] == "retired"]
    steps = np.concatenate([r["traj_steps"][:r["num_peds"]] for r in retired])
    assert (steps == p).sum() > 50 and ((steps > 0) & (steps < p)).sum() > 50 and (steps == 0).sum() > 5
    assert m.traj_totals[0] > 20 and m.totals[:, 0].min() > 50 and 0 < m.totals[:, 5].sum() < m.totals[:, 7].sum()
    # brackets: interpolated instants, brackets wider than max_dt, a bracket with two horizons of one record
    times = [t for t, _, _, _, back in sti.script(0, p, v, k) if not back]
    wide = sum(b - a > sti.MAX_DT for a, b in zip(times[:-1], times[1:]))
    inside = [sum(a < t_r + h * sti.STEP < b for h in range(1, p + 1))
              for a, b in zip(times[:-1], times[1:]) if b - a <= sti.MAX_DT for t_r in times if t_r < a]
    assert wide >= 3 and sum(n == 1 for n in inside) > 100 and sum(n == 2 for n in inside) > 5
    f64 = sti.StreamRef(p, v, k, (0.75, 3.0, 8.0), 60, 8, dtype=np.float64)
    for t, ids, xy, pred, _ in sti.script(0, p, v, k):
        f64.push(t, ids, xy, pred)
    assert np.array_equal(f64.score.totals[:, [0, 1, 4, 5, 6, 7]], m.totals[:, [0, 1, 4, 5, 6, 7]])   # (d2 = |d|^2 / h rounds)
    # an id that returns inside the horizon is matched again; an OVERFLOW id in the scene is never truth
    for row in m.rows:
        if row is None:
            continue
        for c, i in enumerate(row["ids"][:row["num_peds"]].tolist()):
            if i in sti.EXTRA[3:]:
                assert not row["matched"][:, c].any()
    # v = 70: the scored pedestrians sit in columns 64 and up
    wide, _ = _run_script(1, 3, 70, 0, 40, 2)
    cols = np.zeros(70, np.int64)
    for row in wide.score.rows:
        if row is not None:
            cols += row["matched"].sum(axis=0)
    assert not cols[:64].any() and cols[64:].sum() > 50


def test_eviction_with_four_rows():
    """pending = 4 at P = 12, step 4: a record lives 48 ticks and about ten pushes arrive in that time, so most records
    are overwritten while pending.  The restatement asserts that no evicted pedestrian had all P steps."""
    ref, _ = _run_script(0, 12, 5, 2, 4, 8)
    m = ref.score
    assert m.accepted == 60 and m.evictions > 40 and m.traj_totals[0] == 0
    assert m.totals[:3, 0].min() > 10                               # the near horizons are still scored
    roomy, _ = _run_script(0, 12, 5, 2, 60, 8)
    assert roomy.score.evictions == 0 and roomy.score.traj_totals[0] > 20
    assert (roomy.score.totals[:, 0] >= m.totals[:, 0]).all()


def test_the_score_time_header_its_binding_and_the_exports(L):
    """include/stgcnn_hip_score_time.h -- which stgcnn_hip.h includes, so one include still declares the whole C ABI --
    as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its two entry points by
    name, nothing but void * and four scalar types among their parameters (a struct pointer travels as void*: the
    binding passes ctypes.byref), the ABI version 8, the limit and the structs field for field."""
    from social_stgcnn_amd import _lib, ops
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r'^#include "stgcnn_hip_score_time.h"$', main, re.M)
    assert main.index('#include "stgcnn_hip_score_time.h"') > main.index('extern "C" {')
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_score_time.h")).read()
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_score_push_timed", "stg_score_push_streams_timed"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_float}, p.name
        assert fn.restype == ctypes.c_int, p.name
    hdr = re.sub(r"/\*.*?\*/", " ", raw_hdr, flags=re.S)
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    assert re.search(r"#define STG_SCORE_MAX_PENDING 1024\b", raw_hdr) and ops.SCORE_MAX_PENDING == 1024
    for struct, cls in (("stg_score_timed_state", _lib.ScoreTimedState), ("stg_score_timed_out", _lib.ScoreTimedOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        assert re.findall(r"\*(\w+)", body) == [n for n, _ in cls._fields_], struct
    assert list(ops.ScoreTimedState._fields) == [n for n, _ in _lib.ScoreTimedState._fields_]


def test_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    from social_stgcnn_amd import _lib
    f = ctypes.c_void_p(64)

    def structs(no_state=(), no_out=()):
        st = _lib.ScoreTimedState(*[None if n in no_state else 64 for n, _ in _lib.ScoreTimedState._fields_])
        so = _lib.ScoreTimedOut(*[None if n in no_out else 64 for n, _ in _lib.ScoreTimedOut._fields_])
        return ctypes.byref(st), ctypes.byref(so)

    def one(s=8, r=4, step=10, max_dt=10, p=3, v=5, k=2, q=1, rp=6, clock=f, flags=f, mean=f, samples=f, thr=f,
            no_state=(), no_out=()):
        st, so = structs(no_state, no_out)
        return L.stg_score_push_timed(f, f, f, f, clock, flags, s, r, 1e4, step, max_dt, mean, f, 60, 15, 5, 1, samples,
                                      f, f, p, v, k, rp, st, thr, q, so, None)

    def many(ns=3, pushed=f, rp=6, v=5, step=10):
        st, so = structs()
        return L.stg_score_push_streams_timed(f, f, f, f, f, f, pushed, ns, 8, 4, 1e4, step, 10, f, f, 60, 15, 5, 1, f,
                                              f, f, 3, v, 2, rp, st, f, 1, so, None)
    einval = {"S=0": dict(s=0), "R=1": dict(r=1), "P=0": dict(p=0), "V=0": dict(v=0), "K<0": dict(k=-1),
              "Q<0": dict(q=-1), "Rp=0": dict(rp=0), "step=0": dict(step=0), "max_dt=0": dict(max_dt=0),
              "max_dt=2^31": dict(max_dt=1 << 31), "null clock": dict(clock=None), "null head_flags": dict(flags=None),
              "null mean": dict(mean=None), "null thr": dict(thr=None), "null rec_t": dict(no_state=("rec_t",)),
              "null matched": dict(no_state=("matched",)), "null counters": dict(no_state=("counters",)),
              "null acc with K": dict(no_state=("acc",)), "null best with K": dict(no_state=("best",)),
              "null push_totals": dict(no_out=("push_totals",)), "null push_traj": dict(no_out=("push_traj",)),
              "misaligned mean": dict(mean=ctypes.c_void_p(68)), "misaligned samples": dict(samples=ctypes.c_void_p(68))}
    for name, kw in einval.items():
        assert one(**kw) == -1, name
        assert b"stg_score_push_timed" in L.stg_last_error(), name
    unsupported = {"V": dict(v=257), "K": dict(k=65), "P": dict(p=33), "Q": dict(q=5), "Rp": dict(rp=1025),
                   "S": dict(s=2049), "R": dict(r=257), "step": dict(step=1 << 30)}
    for name, kw in unsupported.items():
        assert one(**kw) == _lib.EUNSUPPORTED, name
        assert name.encode() in L.stg_last_error(), name
    for name, kw in {"NS<0": dict(ns=-1), "null pushed": dict(pushed=None), "V=0": dict(v=0), "Rp=0": dict(rp=0),
                     "step=-1": dict(step=-1)}.items():
        assert many(**kw) == -1, name
        assert b"stg_score_push_streams_timed" in L.stg_last_error(), name
    for name, kw in {"NS": dict(ns=4097), "Rp": dict(rp=2000), "V": dict(v=300)}.items():
        assert many(**kw) == _lib.EUNSUPPORTED, name
    assert many(ns=0, pushed=None) == 0                         # no streams: a no-op, nothing is looked at


def test_timed_score_spec_and_state_sizes():
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.predict import ScoreSpec, TimedScoreSpec
    s = TimedScoreSpec()
    assert s == ((0.5, 0.9, 0.99), True, 128) and s.thresholds == ScoreSpec().thresholds
    assert TimedScoreSpec((), False, 1) == ((), False, 1) and TimedScoreSpec([0.25], pending=1024).pending == 1024
    for bad in ((0.0,), (1.0,), (0.1, 0.2, 0.3, 0.4, 0.5), (float("nan"),)):
        with pytest.raises(ValueError, match="level"):
            TimedScoreSpec(bad)
    with pytest.raises(ValueError, match="best_of_k"):
        TimedScoreSpec((0.5,), 1)
    for bad in (0, 1025, -1, 2.0, True, None):
        with pytest.raises(ValueError, match=r"pending must be an integer in \[1, 1024\]"):
            TimedScoreSpec(pending=bad)
    for kw in (dict(v=257), dict(pending=1025), dict(k=65), dict(p=33), dict(q=5)):
        a = dict(ns=1, p=12, v=128, k=20, pending=128, device="meta")
        a.update(kw)
        with pytest.raises(ValueError, match="limit"):
            ops.score_timed_state(**a)
    with pytest.raises(ValueError, match="bad sizes"):
        ops.score_timed_state(1, 12, 128, 20, 0, "meta")
    st = ops.score_timed_state(2, 12, 128, 20, 128, "meta")
    small = ("totals", "traj_totals", "counters", "rec_t", "rec_status", "rec_peds")
    per_stream = sum(x.numel() * x.element_size() for n, x in zip(st._fields, st) if n not in small) // 2
    rv = 128 * 128
    assert per_stream == rv * (28 + 36 * 12) + rv * (8 * 20 * 12 + 4 * 20 + 4 * 12 + 8) and 41e6 < per_stream < 42e6
    assert st.rec_samples.numel() * 4 // 2 == 31457280                          # the samples: 31.5 MB of it
    assert st.rec_ids.dtype == torch.int64 and st.counters.shape == (2, 2) and st.totals.shape == (2, 12, 8)
    lean = ops.score_timed_state(1, 12, 128, 20, 128, "meta", samples=False)
    assert all(getattr(lean, n) is None for n in ("rec_samples", "acc", "best", "traj_ade", "traj_fde"))
    assert 7.5e6 < sum(x.numel() * x.element_size() for x in lean if x is not None) < 7.6e6


class _Model:
    seq_len, pred_seq_len = 8, 12


def test_live_predictors_check_the_timed_spec():
    """Decided from the arguments, ahead of any device work."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.frames import AssociateSpec, TimeRule
    from social_stgcnn_amd.predict import RiskSpec, ScoreSpec, TimedScoreSpec
    for make in (lambda **kw: frames.FramePredictor(_Model(), **kw),
                 lambda **kw: frames.StreamsPredictor(_Model(), 3, **kw)):
        with pytest.raises(ValueError, match="needs time=TimeRule"):
            make(score=TimedScoreSpec())
        with pytest.raises(ValueError, match="indexed by push.*TimedScoreSpec"):
            make(time=TimeRule(10), score=ScoreSpec())
        with pytest.raises(ValueError, match="associate= together with time="):
            make(time=TimeRule(10), score=TimedScoreSpec(), associate=AssociateSpec(1.0))
        with pytest.raises(ValueError, match="needs time=TimeRule"):
            make(score=TimedScoreSpec(), associate=AssociateSpec(1.0))
        with pytest.raises(ValueError, match="keep_samples=False"):
            make(time=TimeRule(10), risk=RiskSpec(0.5), keep_samples=False, score=TimedScoreSpec())
        with pytest.raises(ValueError, match="k <= 64"):
            make(time=TimeRule(10), k=65, score=TimedScoreSpec())
        with pytest.raises(ValueError, match="max_peds=300"):
            make(time=TimeRule(10), max_peds=300, score=TimedScoreSpec((0.5,), False))
