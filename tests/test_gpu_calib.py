"""GPU (-m gpu): stg_calib_fit / stg_calib_apply, ops.calib_fit / calib_apply, calibrate.fit_calibration and the
calibration= keyword of the predictors against tests/calib_np.py.

The restatement is fed the device's own sig -- numpy's float32 exp / tanh are not the device's, as in the score tests,
which start from the device's C_h -- and from there every bit is asked for."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import calib_np as cn
import dist_edges as de
from live_inputs import _model, _pushes, _rows

pytestmark = pytest.mark.gpu
F = np.float32
MODES = {"moment": cn.MOMENT, "coverage": cn.COVERAGE}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _fit_np(fit):
    return {n: x.cpu().numpy() for n, x in zip(fit._fields, fit)}


def _assert_fit(got, want, what):
    """Bit for bit: g, bracket, flags, and the three stats (the count and the number inside are integers; the sum of d2
    is the float64 sum in the kernel's order)."""
    assert np.array_equal(got["flags"], want["flags"]), (what, got["flags"], want["flags"])
    assert np.array_equal(got["g"].view(np.int32), np.asarray(want["g"], F).view(np.int32)), (what, got["g"], want["g"])
    assert np.array_equal(got["bracket"].view(np.int32), np.asarray(want["bracket"], F).view(np.int32)), what
    assert np.array_equal(got["stats"][:, [0, 2]], want["stats"][:, [0, 2]]), (what, got["stats"], want["stats"])
    assert np.array_equal(got["stats"][:, 1].view(np.int64), want["stats"][:, 1].view(np.int64)), \
        (what, got["stats"][:, 1], want["stats"][:, 1])


@pytest.mark.parametrize("level", (0.5, 0.9))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", range(len(cn.CASES)))
def test_fit_is_the_restatement_fed_the_devices_sig(dev, case, mode, level):
    """Every case of calib_np.CASES on a permuted V_pred: sig inside the bound of its three operations and zero in the
    padded slots; g, bracket, flags and stats bit-equal to the restatement fed that sig; a second run gives the same
    bits.  moment: under the test's own precondition that at every candidate the search visited the restatement's
    |sum d2 - 2 count| exceeds what a float64 sum in another order could differ by (calib_np.order_bound); test_calib_cpu
    holds the same margins for numpy's sig."""
    from social_stgcnn_amd import ops
    base, mean, truth, peds = cn.case_inputs(case)
    n, p, v, _ = base.shape
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    mean_d, truth_d = _dev(dev, mean, truth)
    fit = ops.calib_fit(y, mean_d, truth_d, peds, mode, level)
    got = _fit_np(fit)
    ok = cn.dm.clamp_peds(peds, n, v)[:, None] > np.arange(v)[None, :]
    okp = np.broadcast_to(ok[:, None, :], (n, p, v))
    sig = got["sig"]
    assert not sig[~okp].any()
    ref = cn.sig_terms(base.transpose(0, 3, 1, 2), np.float64)[okp]                       # (elements x P, 3)
    rel = (de.A_T + 2 * de.A_E + 2 * de.U) * de.SLOP          # tanhf, two expf, two products (dist_edges.cov_eps)
    assert (np.abs(sig[okp] - ref) <= rel * np.sqrt(ref[:, 0] * ref[:, 2])[:, None].clip(np.abs(ref))).all()
    want = cn.fit(sig, mean, truth, peds, MODES[mode], level)
    if mode == "moment":
        margin = cn.moment_margin(want)
        print("case %d level %s: moment margin %.3g" % (case, level, margin))
        assert margin > 0
    print("case %d %s %s: g %s flags %s" % (case, mode, level, got["g"], got["flags"]))
    _assert_fit(got, want, (case, mode, level))
    assert got["stats"][:, 0].tolist() == [float(ok.sum())] * p
    again = ops.calib_fit(y, mean_d, truth_d, peds, mode, level)
    for a, b, name in zip(fit, again, fit._fields):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("mode", sorted(MODES))
def test_clamps_and_edges(dev, mode):
    """truth == mean -> LOW, g = 2^-10; the truth 1e4 sigma away -> HIGH, g = 2^21; every num_peds 0 -> EMPTY, g = 1; no
    scene at all -> the same without a launch; dist_edges.edge_pred (raw correlations to +-88, log sigmas to +-10) ->
    every output finite and the restatement's."""
    from social_stgcnn_amd import ops
    base, mean, truth, peds = cn.case_inputs(3)
    n, p, v, _ = base.shape
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    mean_d, truth_d = _dev(dev, mean, truth)
    r = _fit_np(ops.calib_fit(y, mean_d, mean_d, peds, mode, 0.9))
    assert (r["flags"] == cn.LOW).all() and (r["g"] == F(2.0 ** -10)).all() and (r["bracket"] == F(2.0 ** -10)).all()
    assert r["stats"].tolist() == [[169.0, 0.0, 169.0]] * p
    sig = r["sig"]
    far = (mean + F(1e4 * np.sqrt(12 * max(sig[..., 0].max(), sig[..., 2].max())))).astype(F)
    r = _fit_np(ops.calib_fit(y, mean_d, _dev(dev, far)[0], peds, mode, 0.9))
    assert (r["flags"] == cn.HIGH).all() and (r["g"] == F(2.0 ** 21)).all() and (r["bracket"] == F(2.0 ** 21)).all()
    assert (r["stats"][:, 0] == 169).all() and not r["stats"][:, 2].any()
    _assert_fit(r, cn.fit(sig, mean, far, peds, MODES[mode], 0.9), "far")
    r = _fit_np(ops.calib_fit(y, mean_d, truth_d, (0,) * n, mode, 0.9))
    assert (r["flags"] == cn.EMPTY).all() and (r["g"] == 1).all() and (r["bracket"] == 1).all()
    assert not r["stats"].any() and not r["sig"].any()
    r = _fit_np(ops.calib_fit(y[:0], mean_d[:0], truth_d[:0], None, mode, 0.9))
    assert (r["flags"] == cn.EMPTY).all() and (r["g"] == 1).all() and not r["stats"].any() and r["sig"].shape[0] == 0
    # saturated correlations and extreme sigmas
    peds_e = (40, 17, 0)
    base = de.edge_pred(3, 12, 40, peds_e, 3)
    assert len(de.cross_of(base, peds_e)) == len(de.RAW) * len(de.PAIRS)
    rng = np.random.default_rng(4)
    mean = np.cumsum(base[..., 0:2], axis=1).astype(F)
    spread = np.sqrt(np.cumsum(np.exp(2.0 * base[..., 2:4].astype(np.float64)), axis=1))
    truth = (mean + 1.5 * spread * rng.normal(size=mean.shape)).astype(F)
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    r = _fit_np(ops.calib_fit(y, *_dev(dev, mean, truth), peds_e, mode, 0.9))
    assert all(np.isfinite(r[name]).all() for name in ("g", "bracket", "stats", "sig")), r
    assert (r["g"] >= F(2.0 ** -10)).all() and (r["g"] <= F(2.0 ** 21)).all() and (r["stats"][:, 0] == 57).all()
    want = cn.fit(r["sig"], mean, truth, peds_e, MODES[mode], 0.9)
    if mode == "moment":
        assert cn.moment_margin(want) > 0
    _assert_fit(r, want, "edge_pred")


def test_ops_refuse(dev):
    """What the Python layer and, behind it, the entry points refuse -- with device memory this time."""
    from social_stgcnn_amd import ops
    base, mean, truth, peds = cn.case_inputs(0)
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    mean_d, truth_d = _dev(dev, mean, truth)
    out, ws = ops.calib_buffers(3, 12, 5, dev)
    assert ws.numel() * 8 == ops.lib().stg_calib_fit_ws_bytes(3, 12, 5)
    for kw, msg in ((dict(mode="median"), "mode must be"), (dict(level=1.0), "level must lie"),
                    (dict(level=0.0), "level must lie"), (dict(out=out), "go together"),
                    (dict(out=out._replace(g=out.flags), ws=ws), "out.g does not fit"),
                    (dict(out=out._replace(sig=out.sig[:2]), ws=ws), "out.sig does not fit")):
        with pytest.raises(ValueError, match=msg):
            ops.calib_fit(y, mean_d, truth_d, peds, **kw)
    with pytest.raises(RuntimeError, match="ws_bytes"):
        ops.calib_fit(y, mean_d, truth_d, peds, out=out, ws=ws[:-1])
    with pytest.raises(ValueError, match="mean must be"):
        ops.calib_fit(y, mean_d[:, :, :4], truth_d, peds)
    with pytest.raises(ValueError, match="truth must be"):
        ops.calib_fit(y, mean_d, truth_d.double(), peds)
    with pytest.raises(ValueError, match=r"v_pred \(N,5,P,V\)"):
        ops.calib_fit(y[:, :4], mean_d, truth_d, peds)
    with pytest.raises(ValueError, match="above the kernel's limit"):
        ops.calib_fit(torch.zeros((1, 5, 33, 2), device=dev), torch.zeros((1, 33, 2, 2), device=dev),
                      torch.zeros((1, 33, 2, 2), device=dev))
    shift = torch.zeros(12, device=dev)
    with pytest.raises(ValueError, match="shift must be"):
        ops.calib_apply(y, shift[:11])
    with pytest.raises(ValueError, match="out must be"):
        ops.calib_apply(y, shift, out=torch.zeros((3, 5, 12, 4), device=dev))
    with pytest.raises(RuntimeError, match="other strides"):           # the same memory read as another layout
        ops.calib_apply(y, shift, out=torch.as_strided(y, (3, 5, 12, 5), (300, 5, 25, 1)))
    with pytest.raises(RuntimeError, match="V=257"):
        ops.calib_apply(torch.zeros((1, 5, 2, 257), device=dev), torch.zeros(2, device=dev))


@pytest.mark.parametrize("permuted_out", (False, True))
@pytest.mark.parametrize("permuted_in", (False, True))
def test_apply_is_the_float32_add(dev, permuted_in, permuted_out):
    """Contiguous and permuted V_pred, in place and into a contiguous or permuted out, more than one workgroup and a
    last partial one (3 x 5 x 12 x 37): fields 2 and 3 bit-equal to the float32 add, fields 0, 1 and 4 untouched, the
    input untouched when out is given."""
    from social_stgcnn_amd import ops
    n, p, v = 3, 12, 37
    rng = np.random.default_rng(9)
    base = rng.normal(0, 2.0, (n, p, v, 5)).astype(F)
    shift = cn.shift_of(np.exp(rng.uniform(-7, 14, p)).astype(F))
    want = cn.apply(base.transpose(0, 3, 1, 2), shift)
    shift_d = torch.from_numpy(shift).to(dev)

    def fresh(perm):
        if perm:
            return torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
        return torch.from_numpy(np.ascontiguousarray(base.transpose(0, 3, 1, 2))).to(dev)
    y = fresh(permuted_in)
    out = torch.full((n, p, v, 5), 7.0, device=dev).permute(0, 3, 1, 2) if permuted_out else \
        torch.full((n, 5, p, v), 7.0, device=dev)
    r = ops.calib_apply(y, shift_d, out=out)
    assert r is out and out.is_contiguous() != permuted_out
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(y.cpu().numpy(), base.transpose(0, 3, 1, 2))
    if not permuted_out:                                     # in place, once per input layout
        r = ops.calib_apply(y, shift_d)
        assert r is y and np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(y.cpu().numpy()[:, [0, 1, 4]], base.transpose(0, 3, 1, 2)[:, [0, 1, 4]])


def test_capture_fit_and_replay_on_new_inputs(dev):
    """ops.calib_fit captured on static buffers (case 3: three waves, ragged scenes), replayed on other inputs and other
    num_peds: the replay equals the eager fit of those inputs bit for bit -- every size the launches depend on is read
    from device memory."""
    from social_stgcnn_amd import ops
    base, mean, truth, peds = cn.case_inputs(3)
    n, p, v, _ = base.shape
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    mean_d, truth_d = _dev(dev, mean, truth)
    peds_d = torch.tensor(peds, dtype=torch.int32, device=dev)
    out, ws = ops.calib_buffers(n, p, v, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.calib_fit(y, mean_d, truth_d, peds_d, "moment", 0.9, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.calib_fit(y, mean_d, truth_d, peds_d, "moment", 0.9, out=out, ws=ws)
    rng = np.random.default_rng(77)
    y.copy_(torch.from_numpy(base + rng.normal(0, 0.2, base.shape).astype(F)).to(dev).permute(0, 3, 1, 2))
    truth_d.copy_(torch.from_numpy(truth + rng.normal(0, 0.5, truth.shape).astype(F)).to(dev))
    peds_d.copy_(torch.tensor((3, 70, 64, 0, 12), dtype=torch.int32))
    for x in out:
        x.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.calib_fit(y, mean_d, truth_d, peds_d, "moment", 0.9)
    for a, b, name in zip(out, eager, out._fields):
        assert torch.equal(a, b), name
    assert (out.stats[:, 0] == 149).all() and not (out.flags & 4).any()


# ---- through the predictors --------------------------------------------------------------------------------------------
def _calibration(p=12, seed=2):
    from social_stgcnn_amd.calibrate import Calibration
    g = np.exp(np.random.default_rng(seed).uniform(-1.0, 3.0, p)).astype(F)
    return Calibration(g, "coverage", 0.9)


def _shifted(v_pred, shift):
    """The float32 add on the device tensor's copy: (N,5,P,V) numpy."""
    return cn.apply(v_pred.cpu().numpy(), shift)


def test_predictor_with_a_calibration(dev):
    """Predictor(calibration=c) against the plain one on the same scenes and noise: v_pred is the plain v_pred plus the
    shift bit for bit, the mean is bit-equal, the samples are ops.sample_trajectories fed the shifted v_pred; eager and
    captured.  calibration=None is the predictor built without the keyword."""
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.predict import Predictor
    n, v, k = 4, 6, 5
    model = _model("eth", dev)
    rng = np.random.default_rng(5)
    obs = torch.from_numpy(np.cumsum(rng.normal(0, 0.3, (n, 8, v, 2)), axis=1)).to(dev)
    peds = torch.tensor([6, 3, 0, 1], dtype=torch.int32, device=dev)
    noise = torch.from_numpy(rng.standard_normal((k, n, 12, v, 2)).astype(F)).to(dev)
    c = _calibration()
    plain = Predictor(model, k).predict(obs, peds, noise=noise)
    none = Predictor(model, k, calibration=None).predict(obs, peds, noise=noise)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    plain_v = plain.v_pred.cpu().numpy().copy()
    pc = Predictor(model, k, calibration=c)
    r = pc.predict(obs, peds, noise=noise)
    want = cn.apply(plain_v, c.shift)
    assert np.array_equal(r.v_pred.cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(r.mean, plain.mean) and not torch.equal(r.samples, plain.samples)
    samples, mean = ops.sample_trajectories(torch.from_numpy(want).to(dev), obs[:, -1].float(), peds, k, noise=noise)
    assert torch.equal(r.samples, samples) and torch.equal(r.mean, mean)
    replay = Predictor(model, k, calibration=c).capture(n, v, peds, dtype=torch.float64)
    g = replay(obs, peds, seed=9)
    assert np.array_equal(g.v_pred.cpu().numpy().view(np.int32), want.view(np.int32))
    samples, _ = ops.sample_trajectories(torch.from_numpy(want).to(dev), obs[:, -1].float(), peds, k, seed=9)
    assert torch.equal(g.samples, samples) and torch.equal(g.mean, plain.mean)
    with pytest.raises(ValueError, match="holds 5 steps"):
        Predictor(model, k, calibration=_calibration(5))


def test_dist_metrics_behind_the_apply_counts_what_the_fit_counted(dev):
    """Case 4 (630 elements): fit, apply the fitted shift, ops.dist_metrics on the shifted V_pred.  Per horizon the number
    of d2 <= thr differs from the fit's stats by at most the number of elements whose float64 d2 lies within
    calib_np.coverage_slack's distance of thr (the rounding of shift, of ls + shift and of the second expf)."""
    from social_stgcnn_amd import ops
    base, mean, truth, peds = cn.case_inputs(4)
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)
    mean_d, truth_d = _dev(dev, mean, truth)
    for mode, level in (("coverage", 0.9), ("moment", 0.5)):
        fit = ops.calib_fit(y, mean_d, truth_d, peds, mode, level)
        g = fit.g.cpu().numpy()
        shifted = ops.calib_apply(y, torch.from_numpy(cn.shift_of(g)).to(dev), out=torch.empty((9, 5, 12, 70), device=dev))
        m = ops.dist_metrics(shifted, mean_d, None, truth_d, peds)
        thr = cn.threshold(level)
        inside = (m.d2.cpu().numpy() <= thr).sum(axis=(0, 2))
        slack = cn.coverage_slack(fit.sig.cpu().numpy(), base.transpose(0, 3, 1, 2), mean, truth, peds, g, thr)
        diff = np.abs(inside - fit.stats[:, 2].cpu().numpy())
        print(mode, "inside", inside, "fit", fit.stats[:, 2].cpu().numpy(), "slack", slack)
        assert (diff <= slack).all(), (diff, slack)
        if mode == "coverage":                               # the fit's own guarantee, and it is tight: one step of the
            assert (fit.stats[:, 2].cpu().numpy() >= float(F(level)) * 630).all()        # search lower fails it


def _live_relations(pred, plain, shift, k, dev, seed, what):
    """The three relations of one push / tick: pred (calibrated) against plain on the same detections and seed."""
    from social_stgcnn_amd import ops
    lead = pred.v_pred.dim() == 3
    v_cal, v_plain = (x.v_pred[None] if lead else x.v_pred for x in (pred, plain))
    want = _shifted(v_plain, shift)
    assert np.array_equal(v_cal.cpu().numpy().view(np.int32), want.view(np.int32)), what
    assert torch.equal(pred.mean, plain.mean) and torch.equal(pred.ids, plain.ids), what
    obs = pred.obs_abs if pred.obs_abs.dim() == 4 else pred.obs_abs[None]
    samples, _ = ops.sample_trajectories(torch.from_numpy(want).to(dev), obs[:, -1].float(), pred.num_peds.reshape(-1), k,
                                         seed=seed)
    assert torch.equal(pred.samples.reshape(samples.shape), samples), what


def test_frame_predictor_with_a_calibration(dev):
    """biwi_eth, 30 pushes, captured from push 12 on: on every push the calibrated predictor's v_pred is the plain one's
    plus the shift, the mean and the scene are the plain one's, the samples are the sampler's on the shifted v_pred;
    calibration=None is the predictor built without the keyword."""
    from social_stgcnn_amd import frames
    pushes = _pushes(_rows("eth_test", "biwi_eth.txt"))[:30]
    model, k, v = _model("eth", dev), 3, 12
    c = _calibration()
    cal = frames.FramePredictor(model, k=k, max_peds=v, calibration=c)
    plain = frames.FramePredictor(model, k=k, max_peds=v)
    none = frames.FramePredictor(model, k=k, max_peds=v, calibration=None)
    replay, busy = None, 0
    for t, det in enumerate(pushes):
        if t == 12:
            replay = cal.capture()
        a = replay(*det, seed=t) if replay else cal.push(*det, seed=t)
        b, n = plain.push(*det, seed=t), none.push(*det, seed=t)
        for x, y in zip(b, n):
            assert torch.equal(x, y), t
        _live_relations(a, b, c.shift, k, dev, t, t)
        busy += int(a.num_peds.sum())
    assert busy > 50


def test_streams_predictor_with_a_calibration(dev):
    """Two streams (biwi_eth and biwi_hotel), 30 ticks, captured from tick 12 on: the same relations on every tick, the
    shift the same for both streams."""
    from social_stgcnn_amd import frames
    feeds = [_pushes(_rows("eth_test", "biwi_eth.txt"))[:30], _pushes(_rows("hotel_test", "biwi_hotel.txt"))[:30]]
    model, k, v = _model("eth", dev), 3, 16
    c = _calibration()
    cal = frames.StreamsPredictor(model, 2, k=k, max_peds=v, calibration=c)
    plain = frames.StreamsPredictor(model, 2, k=k, max_peds=v)
    replay, busy = None, 0
    for t in range(30):
        tick = [feeds[0][t], feeds[1][t] if t % 3 else None]
        if t == 12:
            replay = cal.capture()
        a = replay(tick, seed=t) if replay else cal.push(tick, seed=t)
        b = plain.push(tick, seed=t)
        _live_relations(a, b, c.shift, k, dev, t, t)
        busy += int(a.num_peds.sum())
    assert busy > 100


# ---- real data -----------------------------------------------------------------------------------------------------------
def _windows(name, files=None):
    from social_stgcnn_amd import data
    return data.load_windows(os.path.join(GOLDEN, "data", name), 8, 12, 1, with_non_linear=False, files=files)


@functools.lru_cache(maxsize=None)
def _zara1():
    """The fit set (the first 300 windows of crowds_zara02_train), the test set and the model, loaded once."""
    from social_stgcnn_amd import data
    w = _windows("eth_train", ["crowds_zara02_train.txt"])
    end = w.seq_start_end[299][1]
    first = data.SceneWindows(w.seq[:end], w.seq_rel[:end], w.loss_mask[:end], w.non_linear[:end], w.num_peds[:300],
                              w.max_peds_in_frame)
    return first, _windows("zara1_test"), _model("zara1", torch.device("cuda", 0))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_calibration_carries_over_to_the_test_set(dev, mode):
    """weights_zara1, fit_calibration on the first 300 windows of crowds_zara02_train.txt (1,200 pedestrians), then
    distribution_test(calibration=c) on zara1_test (2,253): the 90 % ellipses hold 0.759 of the truths uncalibrated and
    must hold 0.90 +- 0.03 calibrated (the float64 reference gives 0.914 for coverage, 0.921 for moment:
    test_calib_cpu.py); every factor lies strictly inside the clamps with flag 0.  The means are untouched, so the
    summary's count is the same."""
    from social_stgcnn_amd.calibrate import fit_calibration
    from social_stgcnn_amd.predict import distribution_test
    fit_on, test_on, model = _zara1()
    assert int(fit_on.num_peds.sum()) == 1200 and len(fit_on) == 300 and int(test_on.num_peds.sum()) == 2253
    c, fit = fit_calibration(model, fit_on, mode=mode, level=0.9)
    g, flags = fit.g.cpu().numpy(), fit.flags.cpu().numpy()
    print(mode, "g", g, "flags", flags, "stats", fit.stats.cpu().numpy()[:, 1:].tolist())
    assert not flags.any() and (g > F(2.0 ** -10)).all() and (g < F(2.0 ** 21)).all()
    assert np.array_equal(c.g, g) and (c.mode, c.level) == (mode, float(F(0.9)))
    assert (fit.stats[:, 0].cpu().numpy() == 1200).all()
    s = distribution_test(model, test_on, k=20, seed=0, levels=(0.5, 0.9, 0.99), calibration=c)[0]
    print(mode, "calibrated coverage", s.coverage, "ADE %.4f FDE %.4f" % (s.ade, s.fde))
    assert s.pedestrians == 2253
    assert abs(s.coverage[1] - 0.90) <= 0.03, s.coverage


# ---- the commands --------------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, model, name="eth"):
    import argparse
    from social_stgcnn_amd.trainer import Checkpoint
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset=name)
    ck = Checkpoint(str(tmp_path / "checkpoint" / ("social-stgcnn-" + name)) + "/", args)
    ck.record(0, model, 1.0, 0.5)
    return ck.dir


def test_the_test_command_calibrates(dev, tmp_path, capsys):
    """test.main --calibrate val on a checkpoint of the eth weights whose val/ holds biwi_eth_train.txt: every line of
    the plain run is there, in order; behind the checkpoint's ADE / FDE line the factors and the calibrated lines are
    fit_calibration's and sample_test's / distribution_test's with that calibration; --save_calibration writes the file
    predict_frames --calibration reads, and that command's means stay while its samples become the calibrated ones."""
    from social_stgcnn_amd import frames, predict_frames, test as test_cmd
    from social_stgcnn_amd.calibrate import Calibration, fit_calibration
    from social_stgcnn_amd.predict import distribution_test, sample_test
    model = _model("eth", dev)
    ck = _checkpoint(tmp_path, model)
    root = tmp_path / "datasets"
    os.makedirs(root / "eth")
    os.symlink(os.path.join(GOLDEN, "data", "eth_test"), root / "eth" / "test")
    os.symlink(os.path.join(GOLDEN, "data", "train_extra"), root / "eth" / "val")
    argv = ["--checkpoints", str(tmp_path / "checkpoint" / "*social-stgcnn*"), "--datasets", str(root)]
    capsys.readouterr()
    test_cmd.main(argv)
    plain = capsys.readouterr().out.split("\n")
    test_cmd.main(argv + ["--calibrate", "val", "--calib_mode", "moment", "--metrics", "--levels", "0.9",
                          "--save_calibration"])
    full = capsys.readouterr().out.split("\n")
    it = iter(full)
    assert all(line in it for line in plain)                  # the plain lines, in order
    held_out, test_on = _windows("train_extra"), _windows("eth_test")
    c, fit = fit_calibration(model, held_out, "moment", 0.9)
    ade, fde, _ = sample_test(model, test_on, k=20, seed=0, calibration=c)
    s = distribution_test(model, test_on, k=20, seed=0, levels=(0.9,), calibration=c)[0]
    assert "Calibration: moment at %g on %d windows, %d pedestrians of val" % (
        c.level, len(held_out), int(held_out.num_peds.sum())) in full
    assert "g: " + " ".join("%.4g" % x for x in c.g) in full
    assert "Calibrated ADE: %s  FDE: %s" % (ade, fde) in full
    assert "Calibrated Coverage: 0.9: %s" % s.coverage[0] in full and "Avg Calibrated ADE: %s" % ade in full
    path = os.path.join(ck, "calibration.npz")
    saved = Calibration.load(path)
    assert np.array_equal(saved.g, c.g) and (saved.mode, saved.level) == ("moment", c.level)
    assert np.array_equal(saved.g, fit.g.cpu().numpy())
    with pytest.raises(SystemExit, match="--save_calibration needs"):
        test_cmd.main(argv + ["--save_calibration"])
    capsys.readouterr()
    rec = os.path.join(GOLDEN, "data", "eth_test", "biwi_eth.txt")
    outs = [str(tmp_path / "plain.npz"), str(tmp_path / "cal.npz")]
    base = ["--checkpoint", ck, "--recording", rec, "--ksteps", "4", "--seed", "3"]
    predict_frames.main(base + ["--out", outs[0]])
    predict_frames.main(base + ["--out", outs[1], "--calibration", path])
    a, b = np.load(outs[0]), np.load(outs[1])
    assert sorted(a.files) == sorted(b.files) and np.array_equal(a["mean"], b["mean"])
    assert np.array_equal(a["ids"], b["ids"]) and not np.array_equal(a["samples"], b["samples"])
    _, pr = frames.predict_recording(model, _rows("eth_test", "biwi_eth.txt"), k=4, seed=3, calibration=saved)
    assert np.array_equal(b["samples"], pr.samples.cpu().numpy())


def test_evaluate_dist_device_with_a_calibration(dev):
    """trainer.evaluate_dist_device(calibration=c) over two batch tuples of eth/test: the summary of the same chain with
    ops.calib_apply between the forward and the sampler, field for field; the coverage moves, the count does not."""
    from social_stgcnn_amd import data, metrics, ops
    from social_stgcnn_amd.predict import observed_inputs
    from social_stgcnn_amd.trainer import evaluate_dist_device
    win, model, c = _windows("eth_test"), _model("eth", dev), _calibration()
    batches = []
    for lo in (0, 40):
        idx = np.arange(lo, min(len(win), lo + 40))
        _, pred_rel, obs_abs, _, counts = data.pad_batch(win, idx, obs_len=8)
        peds = torch.from_numpy(counts).to(dev)
        x, adj, obs_last = observed_inputs(torch.from_numpy(obs_abs.astype(np.float64)).to(dev), peds)
        batches.append((x, adj, peds, obs_last, torch.from_numpy(pred_rel).to(dev)))
    s = evaluate_dist_device(model, batches, k_steps=20, seed=3, levels=(0.9,), calibration=c)
    plain = evaluate_dist_device(model, batches, k_steps=20, seed=3, levels=(0.9,))
    shift = torch.from_numpy(c.shift).to(dev)
    sums = None
    with torch.no_grad():
        for b, (x, adj, peds, obs_last, tgt) in enumerate(batches):
            y = ops.calib_apply(model(x, adj, peds)[0], shift)
            samples, mean = ops.sample_trajectories(y, obs_last, peds, 20, seed=3 + b)
            truth = (torch.cumsum(tgt, dim=1) + obs_last[:, None]).contiguous()
            part = metrics.dist_sums(ops.dist_metrics(y, mean, samples, truth, peds), peds, (0.9,))
            sums = part if sums is None else (sums[0] + part[0], sums[1] + part[1])
    want = metrics.summary_of_sums(*sums, (0.9,))
    for a, b in zip(s, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert s.pedestrians == plain.pedestrians and np.array_equal(s.count, plain.count)
    assert s.coverage[0] > plain.coverage[0] and s.amv > plain.amv
