"""GPU (-m gpu): live predictions scored against the tracks that follow (stg_score_push / stg_score_push_streams,
DESIGN.md 5.17), against the push-by-push restatement tests/score_np.py.

Bit-exact scripts through the C ABI (every branch of the rule, two ring wraps), seeded real-valued inputs against the
float64 restatement inside derived bounds, the size limits, the live predictors (eager against captured, streams
against lone predictors, a TrackRule, capture leaving the records alone) and the cross-check against the project's
best-of-K metric at a frame whose scene is a dataset window."""
import os

import numpy as np
import pytest
import torch

import frames_np
from live_inputs import DATA, Schedule, _model, _pushes, _recordings, _rows
import score_np

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                                       # float32 unit roundoff
FLOAT_FIELDS = ("err", "d2", "nll", "best", "traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- through the C ABI -------------------------------------------------------------------------------------------
class Harness:
    """ns streams through ops.score_push (the packed-tick entry point, or the single-stream one with ns = 1 and
    single=True) beside one score_np.ScoreModel per stream.  tick(entries): entries[s] = None (not pushed) or
    (det_ids, det_xy, score_np.Prediction); returns (device outputs as numpy, one restatement output per stream)."""

    def __init__(self, dev, ns, p, v, k, thr, m_max, decimals=4, dtype=np.float32, single=False):
        from social_stgcnn_amd import ops
        self.ops, self.dev, self.ns, self.p, self.v, self.k, self.m_max = ops, dev, ns, p, v, k, m_max
        self.single = single
        self.scale = 0.0 if decimals is None else float(10 ** decimals)
        self.state = ops.score_state(ns, p, v, k, dev, samples=k > 0, q=len(thr))
        self.thr = torch.tensor(list(thr), dtype=torch.float32).to(dev) if len(thr) else None
        self.models = [score_np.ScoreModel(p, v, k, thr, m_max, decimals, dtype) for _ in range(ns)]

    def tick(self, entries):
        ns, p, v, k = self.ns, self.p, self.v, self.k
        mean = np.zeros((ns, p, v, 2), np.float32)
        v_pred = np.zeros((ns, 5, p, v), np.float32)
        samples = np.zeros((k, ns, p, v, 2), np.float32)
        ids = np.full((ns, v), -1, np.int64)
        peds = np.zeros(ns, np.int32)
        det_ids, det_xy, start, pushed = [], [], [0], []
        refs = []
        for s, e in enumerate(entries):
            if e is None:
                pushed.append(0)
                start.append(start[-1])
                refs.append(self.models[s].push(None, None, None))
                continue
            d_ids, d_xy, pr = e
            d_ids, d_xy = np.asarray(d_ids, np.int64).reshape(-1), np.asarray(d_xy, np.float64).reshape(-1, 2)
            det_ids.append(d_ids)
            det_xy.append(d_xy)
            start.append(start[-1] + len(d_ids))
            pushed.append(1)
            mean[s], v_pred[s], ids[s], peds[s] = pr.mean, pr.v_pred, pr.ids, pr.num_peds
            if k:
                samples[:, s] = pr.samples
            refs.append(self.models[s].push(d_ids, d_xy, pr))
        total = max(1, start[-1], self.m_max if self.single else 0)
        all_ids, all_xy = np.zeros(total, np.int64), np.zeros((total, 2))
        if start[-1]:
            all_ids[:start[-1]], all_xy[:start[-1]] = np.concatenate(det_ids), np.concatenate(det_xy)
        t = lambda a: torch.from_numpy(a).to(self.dev)         # noqa: E731
        kw = dict(det_count=t(np.array([start[-1]], np.int32))) if self.single else \
            dict(det_start=t(np.array(start, np.int32)), pushed=t(np.array(pushed, np.int32)), m_total=total)
        out = self.ops.score_push(self.state, self.thr, t(mean), t(v_pred), t(samples) if k else None, t(ids), t(peds),
                                  t(all_ids), t(all_xy), self.m_max, self.scale, **kw)
        return {n: None if x is None else x.cpu().numpy() for n, x in zip(out._fields, out)}, refs

    def totals(self):
        return self.state.totals.cpu().numpy(), self.state.traj_totals.cpu().numpy()

    def assert_bit_equal(self, got, refs, what):
        for s, ref in enumerate(refs):
            for name in score_np.FIELDS:
                if got[name] is None:
                    assert self.k == 0 and name in ("best", "traj_ade", "traj_fde"), (what, name)
                    continue
                a, b = got[name][s], ref[name]
                if name in FLOAT_FIELDS:
                    a, b = a.view(np.int32), b.astype(np.float32).view(np.int32)
                assert np.array_equal(a, b), (what, s, name, got[name][s], ref[name])
        tot, trj = self.totals()
        for s, m in enumerate(self.models):
            assert np.array_equal(tot[s], m.totals), (what, s, tot[s], m.totals)
            assert np.array_equal(trj[s], m.traj_totals), (what, s, trj[s], m.traj_totals)


TRIPLES = np.array([(3, 4), (-5, 12), (8, -15), (-6, -8), (0, 5), (7, 24), (12, 0), (-20, 21)], np.float64)
BIG = 1 << 33                                          # ids above 2^32


def _pos(i, m):
    """Where pedestrian i is at push m: multiples of 1/8 (exact under the rounding to four decimals and in float32)."""
    i = int(i % BIG)
    return np.array([(i % 7) * 24 + 2 * m - 40, (i % 5) * 16 - 3 * m + (i % 3)], np.float64) / 8.0


def _exact_prediction(ids, num_peds, m, p, v, k):
    """A prediction made at push m whose every error is exact in float32: v_pred channels 2-4 zero (C_h = h I), the
    mean and the samples at Pythagorean offsets (in eighths) from where the pedestrian will be."""
    slot_ids = np.full(v, -1, np.int64)
    slot_ids[:len(ids)] = ids
    mean, samples = np.zeros((p, v, 2), np.float32), np.zeros((k, p, v, 2), np.float32)
    for j, i in enumerate(ids):
        for h in range(1, p + 1):
            at = _pos(i, m + h)
            mean[h - 1, j] = at + TRIPLES[(int(i % BIG) + h + m) % 8] / 8.0
            for kk in range(k):
                samples[kk, h - 1, j] = at + (kk + 1) * TRIPLES[(int(i % BIG) + h + 2 * m + 3 * kk + 1) % 8] / 8.0
    v_pred = np.zeros((5, p, v), np.float32)
    v_pred[:2] = np.arange(2 * p * v, dtype=np.float32).reshape(2, p, v) / 8.0      # (not read by the score)
    return score_np.Prediction(slot_ids, num_peds, mean, v_pred, samples)


def _script_entry(s, m, p, v, k):
    """Stream s at its push m: (detection ids, positions, prediction).  The branches: id 3 leaves at pushes 3-4 and is
    back at 5 (inside the horizon); id 4 leaves at push 2 for good; push 6 repeats ids with another position (the first
    detection wins); push 7 is empty; push 8 holds nine detections for M_max = 7, the last two tracked ids; ids above
    2^32; the prediction of push 5 has num_peds 0; scenes of fewer than V pedestrians leave padded slots."""
    base = [1, 2, 3, 4, BIG + 5, BIG + 6][: 4 + (s + m) % 3] if s != 1 else [BIG + 6, 2, 1, 3, 4]
    ids = [i for i in base if not (i == 3 and m in (3, 4)) and not (i == 4 and m >= 2)]
    xy = [_pos(i, m) for i in ids]
    if m == 6:
        ids = ids + [ids[0], ids[1]]
        xy = xy + [xy[0] + 1.0, xy[1] - 0.5]
    if m == 7:
        ids, xy = [], []
    if m == 8 and s == 0:
        extra = [100, 101, 102, 103, 104, 105]
        ids = extra + [ids[2]] + ids[:2]                 # 9 detections: the 8th and 9th are tracked and cut off
        xy = [_pos(i, m) for i in ids]
    scene = sorted(set(ids))[: v - (m % 2)]
    num_peds = 0 if m == 5 else len(scene)
    return (np.array(ids, np.int64), np.array(xy, np.float64).reshape(-1, 2),
            _exact_prediction(scene, num_peds, m, p, v, k))


@pytest.mark.parametrize("k,thr", [(2, (0.75, 3.0)), (0, (0.75, 3.0)), (2, ())], ids=["k2_q2", "k0_null_samples", "q0"])
def test_scripts_are_bit_exact(dev, k, thr):
    """NS 3, P 3, V 5, M_max 7 (no power of two), 3P + 2 = 11 ticks (two ring wraps): every output and the totals equal
    the restatement evaluated in float32, bit for bit.  Stream 1 is not pushed at ticks 2 and 6 (its state stays bit for
    bit, its outputs are empty), stream 2 is reset before tick 5."""
    from social_stgcnn_amd import ops
    ns, p, v, m_max = 3, 3, 5, 7
    h = Harness(dev, ns, p, v, k, thr, m_max)
    count = [0] * ns
    seen = dict(matched=0, retired_full=0, retired_part=0)
    since_reset = np.zeros((2, ns))                      # matched, full trajectories: what the totals hold
    for t in range(3 * p + 2):
        if t == 5:
            ops.score_reset(h.state, torch.tensor([2]).to(dev))
            h.models[2].reset()
            count[2] = 0
            since_reset[:, 2] = 0
        entries = []
        for s in range(ns):
            if s == 1 and t in (2, 6):
                entries.append(None)
                continue
            entries.append(_script_entry(s, count[s], p, v, k))
            count[s] += 1
        before = [x[1].clone() for x in h.state if x is not None]
        got, refs = h.tick(entries)
        h.assert_bit_equal(got, refs, t)
        if entries[1] is None:
            for a, b in zip((x[1] for x in h.state if x is not None), before):
                assert torch.equal(a, b), t
            assert not got["matched"][1].any() and (got["rec_ids"][1] == -1).all() and not got["traj_steps"][1].any()
        seen["matched"] += int(got["matched"].sum())
        since_reset[0] += got["matched"].sum(axis=(1, 2))
        since_reset[1] += (got["traj_steps"] == p).sum(axis=1)
        seen["retired_full"] += int((got["traj_steps"] == p).sum())
        seen["retired_part"] += int(((got["traj_steps"] > 0) & (got["traj_steps"] < p)).sum())
    tot, trj = h.totals()
    assert seen["matched"] > 60 and seen["retired_full"] > 10 and seen["retired_part"] > 3
    assert np.array_equal(tot[:, :, 0].sum(axis=1), since_reset[0]) and np.array_equal(trj[:, 0], since_reset[1])
    assert since_reset[0, 2] < seen["matched"] / 3 and since_reset[0].sum() < seen["matched"]    # the reset took hold
    assert count == [11, 9, 6]
    if thr:
        assert 0 < tot[:, :, 5].sum() < tot[:, :, 6].sum() < tot[:, :, 0].sum()      # the thresholds cut the d2 values


EDGES = {                      # p, v, k, thr: the shapes at which the helpers of score_fn.hpp take another path
    "k0": (3, 5, 0, (0.75, 3.0)),                        # no samples: best, traj_ade and traj_fde are absent
    "q0": (3, 5, 2, ()),
    "p1": (1, 5, 2, (0.75, 3.0)),                        # one ring row: retired and enqueued on every push
    "v65": (3, 65, 2, (0.75, 3.0)),                      # a scene of 65: two lane passes, the second with one live lane
    "peds0": (3, 5, 2, (0.75, 3.0)),                     # every other prediction holds no pedestrian
}
FILLER = 1000                                          # ids from here on are never detected


def _edge_entry(case, s, m, p, v, k):
    """The detections of _script_entry; the scene is the detected ids, for v65 with never-detected ids between them so
    that it fills all 65 columns and a detected id sits in column 64."""
    ids, xy, _ = _script_entry(s, m, p, 5, 0)
    scene = sorted(set(ids.tolist()))[:5 - m % 2]
    if case == "v65":
        scene = scene[:-1] + [FILLER + j for j in range(v - len(scene))] + scene[-1:]
    if case == "peds0" and m % 2:
        scene = []
    return ids, xy, _exact_prediction(scene, len(scene), m, p, v, k)


def _real_covariance(pr, seed):
    """Seeded log sigma in [-2.5, -0.5] and |v_pred[4]| <= 1.2 (the family of test_real_inputs_...) into a prediction."""
    g = np.random.default_rng(seed)
    pr.v_pred[2:4] = g.uniform(-2.5, -0.5, pr.v_pred[2:4].shape)
    pr.v_pred[4] = g.uniform(-1.2, 1.2, pr.v_pred[4].shape)
    return pr


def _assert_cov(got, pr, what):
    """A record's rec_cov (P,V,3) against the float64 running sum of the prediction's v_pred, the columns of its
    pedestrians: cxx and cyy within (5 + P-1) u relative, cxy within (10 + P-1) u of sqrt(cxx cyy) -- the bounds of
    _d2_bounds (expf within 1 ulp, tanhf within 2, P-1 float32 additions).  A wrong stride or column is off by O(1)."""
    p, c = pr.v_pred.shape[1], pr.num_peds
    ref, got = score_np.cumulative_cov(pr.v_pred)[:, :c], got[:, :c].astype(np.float64)
    assert c > 0 and (np.abs(got[..., [0, 2]] - ref[..., [0, 2]]) <= (5 + p - 1) * U * ref[..., [0, 2]]).all(), what
    assert (np.abs(got[..., 1] - ref[..., 1]) <= (10 + p - 1) * U * np.sqrt(ref[..., 0] * ref[..., 2])).all(), what


@pytest.mark.parametrize("single", (False, True), ids=("streams", "lone"))
@pytest.mark.parametrize("case", sorted(EDGES))
def test_edge_shapes_are_bit_exact(dev, case, single):
    """M_max 7, 12 ticks, through stg_score_push_streams (two streams, stream 1 not pushed at ticks 2 and 6) and through
    stg_score_push (one stream): every output and the totals equal the restatement evaluated in float32, bit for bit."""
    p, v, k, thr = EDGES[case]
    ns = 1 if single else 2
    h = Harness(dev, ns, p, v, k, thr, 7, single=single)
    count = [0] * ns
    matched = np.zeros((p, v), np.int64)
    full = 0
    for t in range(12):
        entries = []
        for s in range(ns):
            if s == 1 and t in (2, 6):
                entries.append(None)
                continue
            entries.append(_edge_entry(case, s, count[s], p, v, k))
            count[s] += 1
        got, refs = h.tick(entries)
        h.assert_bit_equal(got, refs, (case, t))
        assert (got["best"] is None) == (got["traj_ade"] is None) == (got["traj_fde"] is None) == (k == 0)
        matched += got["matched"].sum(axis=0)
        full += int((got["traj_steps"] == p).sum())
    tot, trj = h.totals()
    assert matched.sum() == tot[:, :, 0].sum() and matched.sum() > 20 * ns
    assert full == trj[:, 0].sum() and full > 5 * ns
    assert tot.shape[2] == 5 + len(thr)
    if case == "v65":
        assert matched[:, 64].all() and matched[:, :64].any() and not matched[:, 5:64].any()
    # the covariance sum at this shape on real sigma and rho channels (the scripts hold C_h = h I): one more push of
    # stream 0, its record against the float64 sum; the columns past num_peds carry zeros
    ids, xy, pr = _edge_entry(case, 0, count[0], p, v, k)
    h.tick([(ids, xy, _real_covariance(pr, 5))] + [None] * (ns - 1))
    cov = h.state.rec_cov[0, (int(h.state.head[0, 0]) - 1) % p].cpu().numpy()
    _assert_cov(cov, pr, case)
    assert not cov[:, pr.num_peds:].any()


@pytest.mark.parametrize("what", ("m_max_2048", "v_256"))
def test_limits(dev, what):
    """The largest sort (2,048 detections, ids descending) and the widest scene (256 pedestrians), bit-exact scripts
    over P + 2 pushes through the single-stream entry point."""
    p, k = 3, 2
    v, m_max, n_ids = (5, 2048, 2048) if what == "m_max_2048" else (256, 512, 300)
    h = Harness(dev, 1, p, v, k, (1.0,), m_max, single=True)
    ids = np.arange(n_ids, dtype=np.int64)[::-1] * 3 + BIG
    matched = 0
    for m in range(p + 2):
        xy = np.array([_pos(i, m) for i in ids])
        scene = np.sort(ids)[7::max(1, n_ids // v)][:v]
        got, refs = h.tick([(ids, xy, _exact_prediction(scene, len(scene), m, p, v, k))])
        h.assert_bit_equal(got, refs, (what, m))
        matched += int(got["matched"].sum())
    assert matched == v * (1 + 2 + 3 + 3)


def _d2_bounds(cov, p):
    """Relative bound on the float32 d2 and absolute bound on log(det), per element, from the rule's arithmetic
    (DESIGN.md 5.17).  With u = 2^-24: expf within 1 ulp and tanhf within 2 ulp (the HIP device library's stated
    accuracy) put every term of cxx, cyy within 5u and of cxy within 10u; h <= p float32 additions add (p-1)u, so
    |dcxx| <= a cxx, |dcyy| <= a cyy, |dcxy| <= b sqrt(cxx cyy) with a = (5 + p-1)u, b = (10 + p-1)u.  With
    r2 = cxy^2 / (cxx cyy) and kappa = 1 / (1 - r2): |ddet| / det <= kappa (2a + 2b + 3u); the numerator's terms are
    bounded by 2 (cyy dx^2 + cxx dy^2) (b + 5u) (dx, dy carry one rounding each, the products three more) against a
    value of at least (1 - |r|)(cyy dx^2 + cxx dy^2); one more rounding for the division."""
    a, b = (5 + p - 1) * U, (10 + p - 1) * U
    r2 = cov[..., 1] ** 2 / (cov[..., 0] * cov[..., 2])
    kappa = 1.0 / (1.0 - r2)
    det_rel = kappa * (2 * a + 2 * b + 3 * U)
    num_rel = 2 * (b + 5 * U) / (1.0 - np.sqrt(r2))
    return num_rel + det_rel + U, det_rel


def _assert_close(got, ref, cov_of, p, k, worst, what):
    """One stream's outputs of one push against the float64 restatement: exact integers; err / best 1e-6 and the
    trajectory errors 2e-6 relative; d2 and nll inside the derived bounds.  cov_of(h) -> (P,V,3) float64 covariances of
    the record scored at horizon h."""
    # (cov_of(h) is the record's (P,V,3): its step h - 1 is the one scored)
    for name in ("rec_ids", "matched", "traj_steps"):
        assert np.array_equal(got[name], ref[name]), (what, name)
    on = ref["matched"] == 1
    for name, tol in (("err", 1e-6), ("best", 1e-6)):
        if got[name] is None:
            continue
        assert not got[name][~on].any(), (what, name)
        rel = np.abs(got[name][on] - ref[name][on]) / ref[name][on]
        worst[name] = max(worst[name], float(rel.max(initial=0.0)))
        assert (rel <= tol).all(), (what, name, rel.max())
    for name in ("traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean"):
        if got[name] is None:
            continue
        nz = ref[name] != 0
        assert not got[name][~nz].any(), (what, name)
        rel = np.abs(got[name][nz] - ref[name][nz]) / ref[name][nz]
        worst["traj"] = max(worst["traj"], float(rel.max(initial=0.0)))
        assert (rel <= 2e-6).all(), (what, name, rel.max())
    for h in range(1, p + 1):
        row = on[h - 1]
        if not row.any():
            continue
        d2_rel, det_rel = _d2_bounds(cov_of(h)[h - 1][row], p)
        d2r, d2g = ref["d2"][h - 1][row], got["d2"][h - 1][row].astype(np.float64)
        rel = np.abs(d2g - d2r) / d2r
        worst["d2"] = max(worst["d2"], float(rel.max()))
        worst["d2_bound"] = max(worst["d2_bound"], float(d2_rel.max()))
        assert (rel <= d2_rel).all(), (what, h, rel.max(), d2_rel.max())
        nr, ng = ref["nll"][h - 1][row], got["nll"][h - 1][row].astype(np.float64)
        # half the error of d2, half the error of log(det) (|d log det| <= ddet / det) and three float32 roundings of
        # sums bounded by 0.5 d2 + 0.5 |log det| + log(2 pi)
        mag = 0.5 * d2r + np.abs(nr - 0.5 * d2r - score_np.LOG_2PI) + score_np.LOG_2PI
        bound = 0.5 * d2_rel * d2r + 0.5 * det_rel * 1.01 + 4 * U * mag
        worst["nll"] = max(worst["nll"], float(np.abs(ng - nr).max()))
        worst["nll_bound"] = max(worst["nll_bound"], float(bound.max()))
        assert (np.abs(ng - nr) <= bound).all(), (what, h, np.abs(ng - nr).max())
    assert not got["d2"][~on].any() and not got["nll"][~on].any(), what


def _worst():
    return dict(err=0.0, best=0.0, traj=0.0, d2=0.0, d2_bound=0.0, nll=0.0, nll_bound=0.0)


def test_real_inputs_inside_the_derived_bounds(dev):
    """P 12, V 37, K 20, 40 pushes of one stream (the single-stream entry point): seeded log sigma in [-2.5, -0.5] and
    |v_pred[4]| <= 1.2, pedestrians that come and go, positions to four decimals.  Against the float64 restatement:
    matched / rec_ids / traj_steps exact, err / best 1e-6, traj_* 2e-6, d2 / nll inside the derived bounds (at most 3.5e-5
    relative on d2 for this family: 1 / (1 - rho^2) <= 3.3); the coverage counts exact outside 1e-3 of a threshold, the
    totals 1e-9 against float64 sums of the outputs.  Measured on the MI355X: err 1.3e-7, best 1.3e-7, traj 1.7e-7,
    d2 6.5e-7 relative (largest bound 3.37e-5), nll 7.6e-6 absolute; 18 of 38,724 coverage comparisons left out."""
    from social_stgcnn_amd.predict import ScoreSpec
    p, v, k, m_max, n_push, n_ids = 12, 37, 20, 64, 40, 45
    levels = (0.5, 0.9, 0.99)
    thr = ScoreSpec(levels).thresholds
    g = np.random.default_rng(17)
    h = Harness(dev, 1, p, v, k, thr, m_max, dtype=np.float64, single=True)
    ids_all = np.sort(g.choice(10 ** 6, n_ids, replace=False)).astype(np.int64)
    walk = np.cumsum(g.normal(scale=0.4, size=(n_ids, n_push + p + 1, 2)), axis=1) + g.uniform(-10, 10, (n_ids, 1, 2))
    covs = []
    worst = _worst()
    thr32 = np.asarray(thr, np.float32)
    sums = np.zeros((p, 5 + len(thr)))
    left_out = counted = 0
    for m in range(n_push):
        here = np.nonzero(g.random(n_ids) < 0.9)[0]
        g.shuffle(here)
        scene = np.sort(g.choice(here, min(len(here), v - m % 3), replace=False)) if len(here) else here
        v_pred = np.zeros((5, p, v), np.float32)
        v_pred[:2] = g.normal(scale=0.3, size=(2, p, v))
        v_pred[2:4] = g.uniform(-2.5, -0.5, size=(2, p, v))
        v_pred[4] = g.uniform(-1.2, 1.2, size=(p, v))
        cov = score_np.cumulative_cov(v_pred)
        covs.append(cov)
        mean, samples = np.zeros((p, v, 2), np.float32), np.zeros((k, p, v, 2), np.float32)
        sd = np.sqrt(cov[..., [0, 2]])
        for j, i in enumerate(scene):
            mean[:, j] = walk[i, m + 1:m + p + 1] + 1.2 * sd[:, j] * g.normal(size=(p, 2))
            samples[:, :, j] = mean[:, j] + sd[:, j] * g.normal(size=(k, p, 2))
        slot_ids = np.full(v, -1, np.int64)
        slot_ids[:len(scene)] = ids_all[scene]
        pr = score_np.Prediction(slot_ids, len(scene), mean, v_pred, samples)
        got, refs = h.tick([(ids_all[here], walk[here, m], pr)])
        got = {n: x[0] for n, x in got.items()}
        _assert_close(got, refs[0], lambda hh: covs[m - hh], p, k, worst, m)
        on = got["matched"] == 1
        for hh in range(p):
            row = on[hh]
            sums[hh, 0] += row.sum()
            for c, name in enumerate(("err", "d2", "nll", "best")):
                sums[hh, 1 + c] += got[name][hh][row].astype(np.float64).sum()
            inside_dev = got["d2"][hh][row][:, None] <= thr32[None]
            sums[hh, 5:] += inside_dev.sum(axis=0)
            d64 = refs[0]["d2"][hh][row][:, None]
            near = np.abs(d64 - thr32[None].astype(np.float64)) <= 1e-3 * thr32[None]
            left_out += int(near.sum())
            counted += near.size
            assert np.array_equal(inside_dev[~near], (d64 <= thr32[None])[~near]), (m, hh)
    tot, trj = h.totals()
    assert counted > 10000 and left_out <= 0.01 * counted, (left_out, counted)
    assert np.array_equal(tot[0][:, 0], sums[:, 0]) and np.array_equal(tot[0][:, 5:], sums[:, 5:])
    assert np.allclose(tot[0], sums, rtol=1e-9, atol=0)
    assert np.allclose(tot[0], h.models[0].totals, rtol=1e-5) and np.allclose(trj[0], h.models[0].traj_totals, rtol=1e-5)
    frac = tot[0][:, 5:].sum(axis=0) / tot[0][:, 0].sum()
    print("score real inputs: worst %s; left out %d of %d; coverage %s" % (worst, left_out, counted, frac))
    assert worst["d2_bound"] <= 3.5e-5 and trj[0][0] > 100
    assert frac[0] < frac[1] < frac[2] < 1.0


# ---- through the live predictors ---------------------------------------------------------------------------------
def _score_np_of(score, s=0):
    return {n: None if x is None else x[s].cpu().numpy() for n, x in zip(score._fields, score)}


def _restate_push(model_np, det, out, k):
    """Feed the restatement one push with the device's own prediction (a FramePrediction)."""
    pr = score_np.Prediction(out.ids.cpu().numpy(), int(out.num_peds[0]), out.mean.cpu().numpy(),
                             out.v_pred.cpu().numpy(), out.samples.cpu().numpy() if k else None)
    return model_np.push(det[0], det[1], pr), score_np.cumulative_cov(pr.v_pred)


def test_frame_predictor_eager_captured_and_restatement(dev):
    """biwi_eth with the eth weights, 45 pushes, max_peds 12, k 5: FramePredictor(score=...) eager and captured give
    bit-equal Scores and totals; the eager one against the float64 restatement fed the device's own mean, v_pred and
    samples, the totals against float64 sums of the outputs; capture() leaves records and totals as they were."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import ScoreSpec
    pushes = _pushes(_rows("eth_test", "biwi_eth.txt"))[:45]
    model = _model("eth", dev)
    k, v, p = 5, 12, 12
    spec = ScoreSpec((0.5, 0.9))
    eager = frames.FramePredictor(model, k=k, max_peds=v, score=spec)
    cap = frames.FramePredictor(model, k=k, max_peds=v, score=spec)
    ref = score_np.ScoreModel(p, v, k, spec.thresholds, 1024)
    assert eager.score is None and eager.score_totals[0].shape == (1, p, 7)
    covs, worst, scored = [], _worst(), 0
    replay = None
    for t, det in enumerate(pushes):
        if t == 20:                                      # capture in mid-stream: the records and totals stay
            before = [x.clone() for x in cap._score_state if x is not None]
            replay = cap.capture()
            for a, b in zip((x for x in cap._score_state if x is not None), before):
                assert torch.equal(a, b)
        e = eager.push(*det, seed=t)
        c = replay(*det, seed=t) if replay else cap.push(*det, seed=t)
        assert torch.equal(e.samples, c.samples)
        for a, b, name in zip(eager.score, cap.score, eager.score._fields):
            assert torch.equal(a, b), (t, name)
        for a, b in zip(eager.score_totals, cap.score_totals):
            assert torch.equal(a, b), t
        r, cov = _restate_push(ref, det, e, k)
        covs.append(cov)
        got = _score_np_of(eager.score)
        _assert_close(got, r, lambda hh: covs[t - hh], p, k, worst, t)
        scored += int(got["matched"].sum())
    tot, trj = (x.cpu().numpy()[0] for x in eager.score_totals)
    assert scored > 200 and tot[:, 0].sum() == scored and trj[0] >= 3
    assert np.array_equal(tot[:, 0], ref.totals[:, 0]) and np.allclose(tot[:, [1, 4]], ref.totals[:, [1, 4]], rtol=1e-5)
    assert np.allclose(trj, ref.traj_totals, rtol=1e-5)
    s = frames.score_summary(*eager.score_totals, spec.levels)
    assert s.count.shape == (1, p) and s.err[0, -1] > s.err[0, 0]               # the error grows with the horizon
    print("frame predictor score: worst %s; ade %.4f fde %.4f over %d trajectories; coverage at h=12 %s"
          % (worst, s.ade[0], s.fde[0], s.trajectories[0], s.coverage[0, -1]))
    eager.reset()
    assert not eager.score_totals[0].any() and not eager._score_state.head.any()
    assert (eager._score_state.rec_ids == -1).all()


def test_streams_equal_lone_frame_predictors(dev):
    """14 recordings, staggered starts, explicit noise: the Score and the totals of stream s are those of a lone
    FramePredictor fed that stream's pushes with noise[:, s:s+1], bit for bit, eager for 24 ticks and captured after;
    a stream not pushed has the empty Score and unchanged totals; reset([s]) clears that stream's totals alone."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import ScoreSpec
    recs = _recordings()
    assert len(recs) == 14
    pushes = [_pushes(_rows(*r))[:40] for r in recs]
    ns, k, v, p = 14, 3, 128, 12
    model = _model("eth", dev)
    spec = ScoreSpec((0.9,))
    sp = frames.StreamsPredictor(model, ns, k=k, max_peds=v, score=spec)
    lone = [frames.FramePredictor(model, k=k, max_peds=v, score=spec) for _ in range(ns)]
    sched = Schedule(pushes, [s % 5 for s in range(ns)])
    gen = torch.Generator()
    gen.manual_seed(3)
    matched = 0
    for t in range(24):
        tick = sched.tick(t)
        noise = torch.randn((k, ns, p, v, 2), generator=gen).to(dev)
        tot_before = sp.score_totals[0].clone()
        sp.push(tick, noise=noise)
        for s in range(ns):
            if tick[s] is None:
                assert not sp.score.matched[s].any() and (sp.score.rec_ids[s] == -1).all(), (t, s)
                assert not sp.score.err[s].any() and not sp.score.traj_steps[s].any(), (t, s)
                assert torch.equal(sp.score_totals[0][s], tot_before[s]), (t, s)
                continue
            lone[s].push(*tick[s], noise=noise[:, s:s + 1])
            for a, b, name in zip(sp.score, lone[s].score, sp.score._fields):
                assert torch.equal(a[s], b[0]), (t, s, name)
        matched += int(sp.score.matched.sum())
    assert matched > 2000
    for s in range(ns):
        for a, b in zip(sp.score_totals, lone[s].score_totals):
            assert torch.equal(a[s], b[0]), s
    # captured ticks go on from the same records (in-kernel draws: the matching, the mean errors and d2 do not depend
    # on them)
    before = [x.clone() for x in sp._score_state if x is not None]
    replay = sp.capture()
    for a, b in zip((x for x in sp._score_state if x is not None), before):
        assert torch.equal(a, b)
    for t in range(24, 30):
        tick = sched.tick(t)
        replay(tick, seed=t)
        for s in range(ns):
            if tick[s] is None:
                continue
            lone[s].push(*tick[s], seed=t)
            for name in ("rec_ids", "matched", "err", "d2", "nll", "traj_steps", "traj_ade_mean", "traj_fde_mean"):
                assert torch.equal(getattr(sp.score, name)[s], getattr(lone[s].score, name)[0]), (t, s, name)
    keep = sp.score_totals[0].clone()
    sp.reset([4])
    assert not sp.score_totals[0][4].any() and not sp.score_totals[1][4].any()
    assert not sp._score_state.head[4].any() and keep[4].any()
    others = [s for s in range(ns) if s != 4]
    assert torch.equal(sp.score_totals[0][others], keep[others])


def test_scores_follow_the_filled_scenes_of_a_track_rule(dev):
    """Under TrackRule(2, 2) a pedestrian with a short or gapped history is in the scene and is scored: row h-1 of
    rec_ids is the scene of h pushes ago wherever its pedestrian is among this push's detections."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import ScoreSpec
    pushes = _pushes(_rows("eth_test", "biwi_eth.txt"))[:40]
    # a tracker with gaps: every third frame loses its first detection
    pushes = [(i[1:], x[1:]) if t % 3 == 2 and len(i) > 1 else (i, x) for t, (i, x) in enumerate(pushes)]
    model = _model("eth", dev)
    fp = frames.FramePredictor(model, k=2, max_peds=16, tracks=frames.TrackRule(2, 2), score=ScoreSpec((), False))
    strict = frames.FramePredictor(model, k=2, max_peds=16, score=ScoreSpec((), False))
    assert fp.score_totals[0].shape == (1, 12, 5)
    scenes, partial = [], 0
    for t, det in enumerate(pushes):
        out = fp.push(*det, seed=t)
        strict.push(*det, seed=t)
        assert fp.score.best is None and fp.score.traj_ade is None
        rec = fp.score.rec_ids[0].cpu().numpy()
        now = set(det[0].tolist())
        for h in range(1, 13):
            want = np.full(16, -1, np.int64)
            if t - h >= 0:
                ids, c, seen = scenes[t - h]
                for j in range(c):
                    if int(ids[j]) in now:
                        want[j] = ids[j]
                        partial += int(seen[j] != 0xff)
            assert np.array_equal(rec[h - 1], want), (t, h)
        scenes.append((out.ids.cpu().numpy(), int(out.num_peds[0]), fp.seen.cpu().numpy()))
    assert partial > 50
    assert float(fp.score_totals[0][0, :, 0].sum()) > float(strict.score_totals[0][0, :, 0].sum()) > 0


def test_trajectory_errors_are_the_projects_best_of_k(dev):
    """At a frame whose scene is exactly a dataset window's pedestrian set (eth: 11 such frames), with explicit noise,
    traj_ade / traj_fde twelve pushes later are ops.best_of_k on that window with the same draws, within the project's
    1e-5 bar; every step of every pedestrian is matched.  Measured on the MI355X: 5.4e-7 at the most
    (the two differ in how the truth is built: float32 sums of the window's displacements there, the rounded positions
    here)."""
    from social_stgcnn_amd import data, frames, ops
    from social_stgcnn_amd.predict import ScoreSpec
    rec = ("eth_test", "biwi_eth.txt")
    rows = _rows(*rec)
    win = data.load_windows(os.path.join(DATA, rec[0]), 8, 12, 1, with_non_linear=False, files=[rec[1]])
    starts = frames_np.dataset_windows(rows)
    assert len(starts) == len(win)
    scenes = {f: ids for f, _, ids, _ in frames_np.frame_scenes(rows)}
    equal = [(w, idx) for w, (idx, wid) in enumerate(starts) if np.array_equal(scenes.get(idx + 7, ()), wid)]
    assert len(equal) == 11
    pushes = _pushes(rows)
    model = _model("eth", dev)
    k, v, p = 20, 16, 12
    gen = torch.Generator()
    gen.manual_seed(11)
    noise = torch.randn((k, 1, p, v, 2), generator=gen).to(dev)
    worst = 0.0
    for w, idx in equal[:3]:
        fp = frames.FramePredictor(model, k=k, max_peds=v, score=ScoreSpec((0.9,)))
        first = max(0, idx - 4)                          # the tracks need the 8 frames of the window's observation
        for f in range(first, idx + 20):
            out = fp.push(*pushes[f], noise=noise)
            if f == idx + 7:
                c = int(out.num_peds[0])
                assert c == win.num_peds[w]
                y, obs_last = out.v_pred.clone()[None], out.obs_abs[0, -1].to(torch.float32).clone()[None]
        _, pred_rel, _, _, counts = data.pad_batch(win, np.array([w]), v_pad=v)
        ade, fde = ops.best_of_k(y, torch.from_numpy(pred_rel).to(dev), obs_last, torch.from_numpy(counts).to(dev), k,
                                 noise)
        assert torch.equal(fp.score.traj_steps[0, :c], torch.full((c,), p, dtype=torch.int32, device=dev))
        d_ade = float((fp.score.traj_ade[0, :c] - ade[0, :c]).abs().max())
        d_fde = float((fp.score.traj_fde[0, :c] - fde[0, :c]).abs().max())
        worst = max(worst, d_ade, d_fde)
        assert not fp.score.traj_ade[0, c:].any()
    print("score traj_ade / traj_fde against ops.best_of_k: worst difference %.3g" % worst)
    assert worst < 1e-5, worst
