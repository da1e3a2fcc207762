"""GPU (-m gpu): the kernels that read V_pred at evaluation time -- stg_sample_trajectories, stg_bestofk_eval,
stg_sample_risk, stg_score_push_streams, stg_score_push_streams_timed -- on the saturated-correlation grid of
tests/dist_edges.py (raw correlations to +-88, log sigmas to +-10) against the float64 reference, inside the bounds
derived from the written arithmetic (validated on the CPU by test_dist_edges_cpu.py).  No flat
tolerance, and no element left out but the num_peds padding.

Measured on the MI355X, worst error / bound: see DESIGN.md 2.4."""
import numpy as np
import pytest
import torch

import dist_edges as de
import score_np
import score_time_inputs as sti
from dist_edges import SHAPES
from frames_time_np import OVERFLOW, TIME_ORDER
from test_gpu_risk import FIELDS as RISK_FIELDS
from test_gpu_score import Harness as PushHarness
from test_gpu_score_time import Harness as TimedHarness, _assert_rows

pytestmark = pytest.mark.gpu
K, SEED = de.SAMPLES_K, de.SAMPLES_SEED


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _vp(a):
    return np.moveaxis(np.asarray(a), -3, -2)


_case = de.sampler_case


def _device_inputs(i, philox, dev):
    base, obs, tgt, noise, ok, ref, bound = _case(i, philox)
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)                      # (N,5,P,V) view of (N,P,V,5)
    nz = None if philox else torch.from_numpy(noise.astype(np.float32)).to(dev)
    pd = torch.tensor(SHAPES[i][3], dtype=torch.int32, device=dev)
    return y, torch.from_numpy(obs).to(dev), torch.from_numpy(tgt).to(dev), nz, pd


def _samples(i, philox, dev):
    from social_stgcnn_amd import ops
    y, ol, _, nz, pd = _device_inputs(i, philox, dev)
    if SHAPES[i][2] == 8:        # an output view that is 8- but not 16-byte aligned: the one-pedestrian kernel
        n, p, v, _ = SHAPES[i]
        buf = torch.full((K * n * p * v * 2 + 2,), 5.0, device=dev)
        out = buf[2:].view(K, n, p, v, 2)
        s, mean = ops.sample_trajectories(y, ol, pd, K, nz, SEED, samples=out)
        assert s.data_ptr() == out.data_ptr() and float(buf[:2].min()) == 5.0
        return s, mean
    return ops.sample_trajectories(y, ol, pd, K, nz, SEED)


@pytest.mark.parametrize("philox", [False, True], ids=["caller_noise", "philox"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["v40", "v7", "v8_unaligned"])
def test_samples_are_finite_and_inside_the_bound(dev, i, philox):
    """Every valid element finite and within sample_bound of the float64 reference; padded slots exactly 0; the mean
    trajectory is the float64 running sum of the means (P + 1 roundings) and does not depend on channels 2-4."""
    from social_stgcnn_amd import ops
    base, obs, _, _, ok, ref, bound = _case(i, philox)
    s, mean = _samples(i, philox, dev)
    got = s.cpu().numpy().astype(np.float64)
    assert np.isfinite(_vp(got)[:, ok]).all()
    ratio = (_vp(np.abs(got - ref)) / _vp(bound))[:, ok]
    print("samples %s philox=%s: worst error / bound %.3f" % (SHAPES[i][:3], philox, ratio.max()))
    assert (ratio <= 1.0).all(), float(ratio.max())
    assert np.all(_vp(got)[:, ~ok] == 0)
    m = mean.cpu().numpy()
    part = np.cumsum(base[..., 0:2].astype(np.float64), axis=1)
    want = part + obs[:, None]
    m_b = de.U * ((base.shape[1] + 1) * np.maximum.accumulate(np.abs(part), axis=1) + np.abs(want)) * de.SLOP
    assert (_vp(np.abs(m - want))[ok] <= _vp(m_b)[ok]).all() and np.all(_vp(m)[~ok] == 0)
    y, ol, _, _, pd = _device_inputs(i, philox, dev)
    flat = base.copy()
    flat[..., 2:5] = 0
    _, mean0 = ops.sample_trajectories(torch.from_numpy(flat).to(dev).permute(0, 3, 1, 2), ol, pd, k=0)
    assert torch.equal(mean0, mean)


@pytest.mark.parametrize("philox", [False, True], ids=["caller_noise", "philox"])
@pytest.mark.parametrize("i", [0, 1], ids=["v40", "v7"])
def test_best_of_k_is_the_best_of_all_k(dev, i, philox):
    """ADE / FDE equal the minimum over ALL K reference samples within the bound carried through the distance (a NaN
    sample dropped by fminf would leave the best of fewer), and so does the minimum over sample_trajectories' own
    samples, taken in float64 (the two kernels may contract differently; each is inside the bound on its own)."""
    from social_stgcnn_amd import ops
    base, obs, tgt, _, ok, ref, bound = _case(i, philox)
    y, ol, tg, nz, pd = _device_inputs(i, philox, dev)
    ade, fde, ade_b, fde_b = de.best_of_k_reference(ref, tgt, obs, bound)
    a, f = (x.cpu().numpy().astype(np.float64) for x in ops.best_of_k(y, tg, ol, pd, K, nz, SEED))
    assert np.isfinite(a).all() and np.isfinite(f).all() and not a[~ok].any() and not f[~ok].any()
    ra, rf = np.abs(a - ade)[ok] / ade_b[ok], np.abs(f - fde)[ok] / fde_b[ok]
    print("best_of_k %s philox=%s: worst error / bound ADE %.3f FDE %.3f" % (SHAPES[i][:3], philox, ra.max(), rf.max()))
    assert (ra <= 1.0).all() and (rf <= 1.0).all(), (float(ra.max()), float(rf.max()))
    s = _samples(i, philox, dev)[0].cpu().numpy().astype(np.float64)
    gt = np.cumsum(tgt.astype(np.float64), axis=1) + obs[:, None]
    d = np.sqrt(((s - gt[None]) ** 2).sum(-1))
    sa, sf = d.mean(axis=2).min(axis=0), d[:, :, -1].min(axis=0)
    assert (np.abs(sa - ade)[ok] <= ade_b[ok]).all() and (np.abs(sf - fde)[ok] <= fde_b[ok]).all()


@pytest.mark.parametrize("philox", [False, True], ids=["caller_noise", "philox"])
@pytest.mark.parametrize("i", [0, 1], ids=["v40", "v7"])
def test_risk_counts_equal_the_reference(dev, i, philox):
    """Radii, rectangles and last positions chosen on the CPU (dist_edges.risk_case) so that the float64 samples leave
    no count undecided when every pedestrian's positions move by its own derived bound (risk_np.bounds with the (N,V)
    allowance): the device's integer counts then equal the reference's -- at a radius with counts strictly between 0
    and K and at one where every conflict count is K.  A NaN sample compares false and would leave a count low."""
    from social_stgcnn_amd import ops
    obs, radii, zones, wants = de.risk_case(i, philox)
    y, _, _, nz, pd = _device_inputs(i, philox, dev)
    ol, zn = torch.from_numpy(obs).to(dev), torch.from_numpy(zones).to(dev)
    for radius, want in zip(radii, wants):
        r = ops.sample_risk(y, ol, pd, K, radius, zn, noise=nz, seed=SEED, pairs=True)
        for name in RISK_FIELDS:
            got = getattr(r, name).cpu().numpy()
            assert np.array_equal(got, want[name]), (radius, name, int((got != want[name]).sum()))
    mixed = int(((wants[0]["conflict"] > 0) & (wants[0]["conflict"] < K)).sum())
    print("risk %s philox=%s: radii %g and %g, %d rectangles, %d conflict counts strictly between 0 and K"
          % (SHAPES[i][:3], philox, radii[0], radii[1], len(zones), mixed))
    assert mixed > 0 and wants[1]["conflict"].max() == K


# ---- the score kernels ---------------------------------------------------------------------------------------------
LEVELS = (0.5, 0.9, 0.99)


def _check_cov(dev_cov, v_pred, c, p, padding=True):
    """The device's float32 C_h (P,V,3) of a record against the float64 one inside cov_eps; zeros in the padding."""
    want = score_np.cumulative_cov(v_pred)[:, :c]
    a, b = de.cov_eps(p)
    got = dev_cov[:, :c].astype(np.float64)
    root = np.sqrt(want[..., 0] * want[..., 2])
    assert (np.abs(got[..., 0] - want[..., 0]) <= a * de.SLOP * want[..., 0]).all()
    assert (np.abs(got[..., 2] - want[..., 2]) <= a * de.SLOP * want[..., 2]).all()
    assert (np.abs(got[..., 1] - want[..., 1]) <= b * de.SLOP * root).all()
    assert not padding or not dev_cov[:, c:].any()
    return want


def _check_values(case, s, m_rec, h, d2, nll, ref_d2, ref_nll, cov64, worst, decimals):
    """d2 / nll (c,) of the record of push m_rec at horizon h against the float64 restatement inside score_bound."""
    c = case.num_peds[s]
    dx, dy = case.offsets(s, m_rec, h, decimals)
    d2_b, nll_b, r_d = de.score_bound(cov64[h - 1, :c], dx, dy, ref_d2, case.p)
    e2, en = np.abs(d2.astype(np.float64) - ref_d2), np.abs(nll.astype(np.float64) - ref_nll)
    assert np.isfinite(d2).all() and np.isfinite(nll).all() and (r_d < 0.5).all()
    assert (e2 <= d2_b).all(), (s, m_rec, h, e2 / d2_b)
    assert (en <= nll_b).all(), (s, m_rec, h, en / nll_b)
    worst["d2"], worst["nll"] = max(worst["d2"], float((e2 / d2_b).max())), max(worst["nll"], float((en / nll_b).max()))
    worst["n"] += c


def _check_summary(tot, trj):
    from social_stgcnn_amd import frames
    assert np.isfinite(tot).all() and np.isfinite(trj).all()
    s = frames.score_summary(tot, trj, LEVELS)
    assert (s.count > 0).all() and (s.trajectories > 0).all()
    for name, x in zip(s._fields, s):
        if name != "levels":
            assert np.isfinite(np.asarray(x, np.float64)).all(), name


def test_score_push_on_the_four_arrangements(dev):
    """14 pushes of two streams (V 8, K 4, P 12; stream 1 with five pedestrians and junk in its padding), every step
    saturated / step 1 saturated / alternating signs / moderate, truths on and off the degenerate line.  The device's
    C_h inside cov_eps of the float64 one; fed that C_h, the float32 restatement gives every output field bit for bit,
    and both totals are its values summed in the kernel's order (coverage counts are checked this way only); d2 and
    nll inside score_bound of the float64 restatement; everything finite, the summary without a NaN."""
    from social_stgcnn_amd.predict import ScoreSpec
    case = de.score_case()
    ns, p, v, k = case.ns, case.p, case.v, case.k
    thr = ScoreSpec(LEVELS).thresholds
    h = PushHarness(dev, ns, p, v, k, thr, 16, decimals=None)
    f64 = [score_np.ScoreModel(p, v, k, thr, 16, None) for _ in range(ns)]
    cov64, worst = {}, dict(d2=0.0, nll=0.0, n=0)
    tot, trj = np.zeros((ns, p, 5 + len(thr))), np.zeros((ns, 5))
    for m in range(case.n_push):
        entries = [case.detections(s, m) + (case.preds[s, m],) for s in range(ns)]
        got, refs = h.tick(entries)
        dev_cov = h.state.rec_cov.cpu().numpy()
        for s in range(ns):
            c = case.num_peds[s]
            for name in score_np.FIELDS:
                a, b = got[name][s], refs[s][name]
                if a.dtype == np.float32:
                    assert np.isfinite(a).all(), (m, s, name)
                    a, b = a.view(np.int32), b.astype(np.float32).view(np.int32)
                assert np.array_equal(a, b), (m, s, name)
            want = f64[s].push(*entries[s])
            for hh in range(1, min(m, p) + 1):
                _check_values(case, s, m - hh, hh, got["d2"][s][hh - 1, :c], got["nll"][s][hh - 1, :c],
                              want["d2"][hh - 1, :c], want["nll"][hh - 1, :c], cov64[s, m - hh], worst, None)
            tot[s] += de.push_sums(refs[s], np.asarray(thr, np.float32))
            trj[s] += de.traj_sums(refs[s], p)
            # the record of this push: the restatement goes on from the device's own C_h
            cov64[s, m] = _check_cov(dev_cov[s, m % p], case.preds[s, m].v_pred, c, p)
            h.models[s].records[-1]["cov"] = dev_cov[s, m % p].copy()
    dt, dj = h.totals()
    assert np.array_equal(dt, tot) and np.array_equal(dj, trj)
    _check_summary(dt, dj)
    print("score_push: worst error / bound over %d elements: d2 %.3f nll %.3f" % (worst["n"], worst["d2"], worst["nll"]))
    assert worst["n"] == 13 * 90 and dj[:, 0].tolist() == [16.0, 10.0]


def test_score_timed_push_on_the_four_arrangements(dev):
    """The same 14 pushes fed on the time grid (t = 4 m, step 4, 16 pending rows) through stg_track_push_timed and
    stg_score_push_streams_timed: the truth is the track's rounded sample.  The ring's tables bit for bit against the
    float32 restatement fed the device's C_h, what each push added and the running totals as its values summed in the
    kernel's order, d2 / nll inside score_bound of the float64 restatement, everything finite."""
    from social_stgcnn_amd.predict import ScoreSpec
    case = de.score_case()
    ns, p, v, k, rp = case.ns, case.p, case.v, case.k, 16
    thr = ScoreSpec(LEVELS).thresholds
    thr32 = np.asarray(thr, np.float32)
    h = TimedHarness(dev, ns, p, v, k, thr, rp, 8)
    f64 = [sti.StreamRef(p, v, k, thr, rp, 8, dtype=np.float64) for _ in range(ns)]
    t_ = lambda a: torch.from_numpy(a).to(dev)               # noqa: E731
    cov64, worst = {}, dict(d2=0.0, nll=0.0, n=0)
    tot, trj = np.zeros((ns, p, 5 + len(thr))), np.zeros((ns, 5))
    for m in range(case.n_push):
        t = sti.STEP * m
        mean = np.stack([case.preds[s, m].mean for s in range(ns)])
        v_pred = np.stack([case.preds[s, m].v_pred for s in range(ns)])
        samples = np.stack([case.preds[s, m].samples for s in range(ns)], axis=1)
        ids = np.stack([case.preds[s, m].ids for s in range(ns)])
        peds = np.array(case.num_peds, np.int32)
        for s in range(ns):
            d_ids, d_xy = case.detections(s, m)
            flags = h.push[s].push(d_ids, d_xy, t)[4]
            f_ref, _ = h.refs[s].push(t, d_ids, d_xy, case.preds[s, m])
            f64[s].push(t, d_ids, d_xy, case.preds[s, m])
            assert flags == f_ref and not flags & (OVERFLOW | TIME_ORDER), (m, s, flags, f_ref)
        out = h.ops.score_timed_push(h.state, h.thr, t_(mean), t_(v_pred), t_(samples), t_(ids), t_(peds), h.tracks,
                                     sti.STEP, sti.MAX_DT, 1e4, pushed=t_(np.ones(ns, np.int32)))
        added, added_traj = (x.cpu().numpy() for x in out)
        st = h.snapshot()
        for s in range(ns):
            c = case.num_peds[s]
            model, ref64 = h.refs[s].score, f64[s].score
            _assert_rows(st, s, model, k, (m, s))
            want_add, want_traj = np.zeros((p, 5 + len(thr))), np.zeros(5)
            for hh in range(1, min(m, p) + 1):                 # the record of push m - hh is scored at horizon hh
                rec, rec64 = model.rows[(m - hh) % rp], ref64.rows[(m - hh) % rp]
                assert rec["t"] == sti.STEP * (m - hh) and rec["matched"][hh - 1, :c].all()
                row = {n: rec[n][hh - 1:hh] for n in ("matched", "err", "d2", "nll", "best")}
                want_add[hh - 1] = de.push_sums(row, thr32)[0]
                _check_values(case, s, m - hh, hh, st["d2"][s, (m - hh) % rp, hh - 1, :c],
                              st["nll"][s, (m - hh) % rp, hh - 1, :c], rec64["d2"][hh - 1, :c], rec64["nll"][hh - 1, :c],
                              cov64[s, m - hh], worst, 4)
            if m >= p:
                rec = model.rows[(m - p) % rp]
                assert rec["status"] == "retired"
                want_traj = de.traj_sums(rec, p)
            assert np.array_equal(added[s], want_add) and np.array_equal(added_traj[s], want_traj), (m, s)
            tot[s] += want_add
            trj[s] += want_traj
            cov64[s, m] = _check_cov(st["rec_cov"][s, m % rp], case.preds[s, m].v_pred, c, p, padding=False)
            model.rows[m % rp]["cov"] = st["rec_cov"][s, m % rp].copy()
    for name in ("err", "d2", "nll", "best", "traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean"):
        assert np.isfinite(st[name]).all(), name
    assert np.array_equal(st["totals"], tot) and np.array_equal(st["traj_totals"], trj)
    assert st["counters"].tolist() == [[case.n_push, 0]] * ns
    _check_summary(st["totals"], st["traj_totals"])
    print("score_timed_push: worst error / bound over %d elements: d2 %.3f nll %.3f" % (worst["n"], worst["d2"], worst["nll"]))
    assert worst["n"] == 13 * 90 and trj[:, 0].tolist() == [16.0, 10.0]
