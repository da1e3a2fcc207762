"""GPU (-m gpu): stg_sample_risk / ops.sample_risk -- conflict and zone-occupancy counts over the K samples, reduced on
the device -- and its surface in Predictor, the live predictors and the predict_frames command.

Exact tier: inputs on a 1/4 grid with unit Cholesky factors, so every sample is exact in float32 and every count must
equal the numpy statement (tests/risk_np.py) of the host's own samples.  Real tier and Philox tier: every count must lie
between the statement evaluated at radius - delta and radius + delta (rectangles shrunk / grown by delta) on the float32
samples stg_sample_trajectories writes for the same arguments.

delta = 1e-4: the project's 1e-5 bar for the same sample out of another kernel (measured 2e-6), times
2 sqrt 2 for a difference of two positions, plus the float32 rounding of the squared distance, rounded up.  At most 1 %
of the entries of any output may have different lower and upper counts (a condition on the case, not a measurement)."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import risk_np
from sampling_inputs import random_pred as _random_pred

pytestmark = pytest.mark.gpu
CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
DATA = os.path.join(GOLDEN, "data")
P = 12
DELTA = 1e-4
ZONES = np.array([[-1, -1, 1, 1], [0, 0, 4, 3], [-50, -50, 50, 50]], np.float32)
FIELDS = ("conflict", "conflict_any", "partner", "pair", "zone_any", "zone_count", "ped_zone")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _model(name, dev):
    from social_stgcnn_amd.model import social_stgcnn
    w = load_golden("weights_%s.npz" % name)
    m = social_stgcnn(**CFG)
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    return m.to(dev).eval()


def _host(r):
    return {f: getattr(r, f).cpu().numpy() for f in FIELDS if getattr(r, f) is not None}


def _assert_equal(got, want, what):
    for name in want:
        assert np.array_equal(got[name], want[name]), (what, name, int((got[name] != want[name]).sum()))


def _assert_padding(got, vi, what):
    """Slots at or above the scene's count: 0, and -1 in partner."""
    n, v = got["conflict_any"].shape if "conflict_any" in got else got["ped_zone"].shape[:2]
    pad = np.arange(v)[None, :] >= vi[:, None]                                         # (N,V)
    if "conflict" in got:
        assert not got["conflict"].transpose(0, 2, 1)[pad].any(), what
        assert not got["conflict_any"][pad].any() and np.all(got["partner"][pad] == -1), what
        if "pair" in got:
            assert not got["pair"][pad].any() and not got["pair"].transpose(0, 2, 1)[pad].any(), what
    if "ped_zone" in got:
        assert not got["ped_zone"][pad].any(), what


# ---- exact tier ---------------------------------------------------------------------------------------------------

EXACT_SHAPES = {1: [1, 1], 2: [2, 2, 1], 33: [33, 20, 0], 65: [65, 41], 130: [130]}
EXACT_ZONES = np.array([[-1, -1, 1, 1], [0.25, -2, 2.5, 0.75], [1, 1, -1, -1]], np.float32)      # the last: inverted


@functools.lru_cache(maxsize=None)
def _exact_case(v, k):
    """Means, last positions and normals in multiples of 1/4, log-sigmas and raw correlation 0 (expf(0) = 1,
    tanhf(0) = 0: a sample is mean + eps exactly).  Returns the (N,P,V,5) base of pred, obs_last, noise and the
    host's samples (exact in float32 and float64 alike)."""
    peds = EXACT_SHAPES[v]
    n = len(peds)
    rng = np.random.default_rng(1000 * v + k)
    base = np.zeros((n, P, v, 5), np.float32)
    base[..., 0:2] = rng.integers(-1, 2, size=(n, P, v, 2)) / 4.0
    half = 4 * max(1, int(round(np.sqrt(v))))                                  # +-sqrt(V) metres on the 1/4 grid
    obs_last = (rng.integers(-half, half + 1, size=(n, v, 2)) / 4.0).astype(np.float32)
    noise = (rng.integers(-4, 5, size=(k, n, P, v, 2)) / 4.0).astype(np.float32)
    step = base[None, ..., 0:2].astype(np.float64) + noise
    samples = np.cumsum(step, axis=2) + obs_last[None, :, None].astype(np.float64)
    assert np.array_equal(samples, samples.astype(np.float32))
    return base, obs_last, noise, samples


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("v", sorted(EXACT_SHAPES))
def test_exact_counts_equal_the_numpy_statement(dev, v, k):
    from social_stgcnn_amd import ops
    base, obs_last, noise, samples = _exact_case(v, k)
    peds = np.array(EXACT_SHAPES[v], np.int32)
    n = len(peds)
    y = torch.from_numpy(base).to(dev).permute(0, 3, 1, 2)                     # (N,5,P,V) view of (N,P,V,5)
    assert not y.is_contiguous()
    ol, nz = torch.from_numpy(obs_last).to(dev), torch.from_numpy(noise).to(dev)
    zones = torch.from_numpy(EXACT_ZONES).to(dev)
    # the device sampler writes the host's samples, so the tier's premise holds
    s_dev, _ = ops.sample_trajectories(y, ol, None, k, nz)
    assert np.array_equal(s_dev.cpu().numpy(), samples.astype(np.float32))
    # the case holds what it is there for: a pair at exactly the radius, samples exactly on x0 and on x1
    if v >= 33:
        d = samples[:, 0, :, :, None] - samples[:, 0, :, None]
        assert np.any((d ** 2).sum(-1) == 0.75 ** 2)
        assert np.any(samples[..., 0] == -1.0) and np.any(samples[..., 0] == 1.0)
    out_of_range = np.where(np.arange(n) % 2 == 0, v + 7, -3).astype(np.int32)
    ties, wants = 0, {}
    for what, pd in (("given", peds), ("none", None), ("out of range", out_of_range)):
        key = tuple(risk_np.clamp_peds(pd, n, v))
        if key not in wants:
            wants[key] = risk_np.risk(samples, pd, 0.75, EXACT_ZONES)
        want = wants[key]
        r = ops.sample_risk(y, ol, pd, k, 0.75, zones, noise=nz, pairs=True)
        assert r.k == k and all(getattr(r, f).dtype == torch.int32 for f in FIELDS)
        got = _host(r)
        _assert_equal(got, want, (v, k, what))
        _assert_padding(got, risk_np.clamp_peds(pd, n, v), (v, k, what))
        assert not got["zone_any"][:, :, 2].any() and not got["ped_zone"][:, :, 2].any()         # the inverted zone
        assert np.array_equal(got["pair"], got["pair"].transpose(0, 2, 1))
        top = got["pair"].max(axis=2, keepdims=True)
        ties += int((((got["pair"] == top) & (top > 0)).sum(axis=2) > 1).sum())
        # pair = NULL: the same partner and everything else
        r2 = ops.sample_risk(y, ol, pd, k, 0.75, zones, noise=nz)
        assert r2.pair is None
        _assert_equal(_host(r2), {f: x for f, x in got.items() if f != "pair"}, (v, k, what, "no pair"))
        # the shared set (z_sn = 0) and the same set per scene agree; so do conflicts alone and zones alone
        r3 = ops.sample_risk(y, ol, pd, k, 0.75, zones[None].repeat(n, 1, 1), noise=nz, pairs=True)
        _assert_equal(_host(r3), got, (v, k, what, "per scene"))
        r4, r5 = ops.sample_risk(y, ol, pd, k, 0.75, None, noise=nz), ops.sample_risk(y, ol, pd, k, None, zones, noise=nz)
        assert r4.zone_any is None and r5.conflict is None and r5.partner is None
        _assert_equal({**_host(r4), **_host(r5)}, {f: x for f, x in got.items() if f != "pair"}, (v, k, what, "halves"))
    if v >= 33:
        assert ties > 0                                                        # partner ties occurred (smallest j won)
    # per-scene rectangles that differ between the scenes
    per = np.stack([np.roll(EXACT_ZONES, b, axis=0) + np.float32(0.25 * b) for b in range(n)])
    want = risk_np.risk(samples, peds, None, per)
    _assert_equal(_host(ops.sample_risk(y, ol, peds, k, None, torch.from_numpy(per).to(dev), noise=nz)), want,
                  (v, k, "per-scene zones"))


# ---- real tier ----------------------------------------------------------------------------------------------------

REAL_SHAPES = {8: ([8, 5, 8, 1, 3], 3.0), 33: ([33, 20, 0, 27], 6.0), 130: ([130], 12.0)}


def _real_inputs(v, dev, seed):
    peds, half = REAL_SHAPES[v]
    n = len(peds)
    gen = torch.Generator().manual_seed(seed)
    y = _random_pred(gen, n, P, v, dev)
    ol = ((torch.rand((n, v, 2), generator=gen) * 2 - 1) * half).to(dev)
    return y, ol, torch.tensor(peds, dtype=torch.int32, device=dev), gen


def _assert_sandwiched(r, samples, peds, radius, zones, what, with_pair=True):
    """Every device count between the statement at -delta and +delta; at most 1 % of any output ambiguous; partner
    is the first maximum of the device's own pair row."""
    got = _host(r)
    lo, hi = risk_np.bounds(samples, peds, radius, zones, DELTA)
    shares = {}
    for name in lo:
        if name == "partner" or name not in got:
            continue
        shares[name] = float((lo[name] != hi[name]).mean())
        assert np.all(lo[name] <= got[name]) and np.all(got[name] <= hi[name]), (what, name)
        assert shares[name] <= 0.01, (what, name, shares[name])
    if with_pair:
        assert np.array_equal(got["partner"], risk_np.partner_of(got["pair"])), what
    _assert_padding(got, risk_np.clamp_peds(peds, samples.shape[1], samples.shape[3]), what)
    return got, shares


@pytest.mark.parametrize("v", sorted(REAL_SHAPES))
def test_real_counts_lie_between_the_statement_at_both_deltas(dev, v):
    from social_stgcnn_amd import ops
    k = 20
    y, ol, peds, gen = _real_inputs(v, dev, 40 + v)
    n = y.shape[0]
    noise = torch.randn((k, n, P, v, 2), generator=gen).to(dev)
    samples = ops.sample_trajectories(y, ol, peds, k, noise)[0].cpu().numpy()
    zones = torch.from_numpy(ZONES).to(dev)
    pd = peds.cpu().numpy()
    vi = risk_np.clamp_peds(pd, n, v)
    for radius in (0.5, 1.0):
        r = ops.sample_risk(y, ol, peds, k, radius, zones, noise=noise, pairs=True)
        got, shares = _assert_sandwiched(r, samples, pd, radius, ZONES, (v, radius))
        valid = (np.arange(v)[None, :] < vi[:, None])[:, None, :].repeat(P, axis=1)
        c = got["conflict"][valid]
        mixed = float(((c > 0) & (c < k)).mean())
        print("V=%d radius %.1f: ambiguous shares %s; conflict entries strictly between 0 and K: %.1f %%"
              % (v, radius, {a: "%.3f %%" % (100 * b) for a, b in shares.items()}, 100 * mixed))
        assert mixed > 0.05, (v, radius, mixed)                                # the case is not trivial
    # the wide rectangle holds every valid pedestrian at every step of every sample
    assert np.array_equal(got["zone_count"][:, :, 2], np.repeat(k * vi[:, None], P, axis=1))
    assert np.array_equal(got["zone_any"][:, :, 2], np.repeat(k * (vi[:, None] > 0), P, axis=1))


# ---- Philox tier --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", [8, 33])
def test_philox_draws_are_the_samplers(dev, v):
    from social_stgcnn_amd import ops
    k, seed = 20, 0x1234567890ABCDEF
    y, ol, peds, _ = _real_inputs(v, dev, 70 + v)
    samples = ops.sample_trajectories(y, ol, peds, k, None, seed)[0].cpu().numpy()
    zones = torch.from_numpy(ZONES).to(dev)
    pd = peds.cpu().numpy()
    r1 = ops.sample_risk(y, ol, peds, k, 1.0, zones, seed=seed, pairs=True)
    got1, _ = _assert_sandwiched(r1, samples, pd, 1.0, ZONES, (v, "host seed"))
    seed_dev = torch.tensor([seed], dtype=torch.int64, device=dev)
    r2 = ops.sample_risk(y, ol, peds, k, 1.0, zones, seed=99, seed_dev=seed_dev, pairs=True)    # seed_dev wins
    got2, _ = _assert_sandwiched(r2, samples, pd, 1.0, ZONES, (v, "device seed"))
    _assert_equal(got2, got1, (v, "device seed == host seed"))
    r3 = ops.sample_risk(y, ol, peds, k, 1.0, zones, seed=seed, pairs=True, out=r2)             # fills `out`
    assert r3 is r2
    _assert_equal(_host(r3), got1, (v, "second launch"))
    other = _host(ops.sample_risk(y, ol, peds, k, 1.0, zones, seed=seed + 1, pairs=True))
    assert not np.array_equal(other["conflict"], got1["conflict"])


# ---- surface ------------------------------------------------------------------------------------------------------

def _synthetic_tracks(gen, n, v, t=8, spread=6.0):
    start = torch.rand((n, 1, v, 2), generator=gen) * 2 * spread - spread
    steps = torch.randn((n, t - 1, v, 2), generator=gen) * 0.3 + 0.2
    tracks = torch.cat([start, start + torch.cumsum(steps, dim=1)], dim=1)
    peds = torch.randint(2, v + 1, (n,), generator=gen, dtype=torch.int32)
    ok = (torch.arange(v)[None, :] < peds[:, None]).float()
    return tracks * ok[:, None, :, None], peds


def _risk_equal(a, b):
    assert a.k == b.k
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        assert x is None or torch.equal(x, y), f


def test_predictor_risk_eager_captured_and_without_samples(dev):
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.predict import Predictor, RiskSpec
    m = _model("eth", dev)
    n, v, k = 5, 24, 20
    gen = torch.Generator().manual_seed(11)
    tracks, peds = _synthetic_tracks(gen, n, v)
    obs, pd = tracks.to(dev), peds.to(dev)
    spec = RiskSpec(0.8, ZONES, True)
    pr = Predictor(m, k, risk=spec)
    e = pr.predict(obs, pd, seed=5)
    want = ops.sample_risk(e.v_pred, obs[:, -1], pd, k, 0.8, torch.from_numpy(ZONES).to(dev), seed=5, pairs=True)
    _risk_equal(pr.risk, want)
    assert 0 < int(want.conflict_any.max()) and int(want.zone_count[:, :, 2].min()) > 0
    plain = Predictor(m, k).predict(obs, pd, seed=5)                           # risk=None: the prediction is the same
    assert torch.equal(plain.samples, e.samples) and torch.equal(plain.mean, e.mean)
    # captured == eager, and the static rectangles may be overwritten between replays
    cap = Predictor(m, k, risk=spec)
    replay = cap.capture(n, v, pd)
    r = replay(obs, seed=5)
    assert torch.equal(r.samples, e.samples) and torch.equal(r.v_pred, e.v_pred)
    _risk_equal(cap.risk, want)
    cap.zones.copy_(torch.from_numpy(ZONES + np.float32(0.5)).to(dev))
    replay(obs)
    moved = ops.sample_risk(e.v_pred, obs[:, -1], pd, k, 0.8, torch.from_numpy(ZONES + np.float32(0.5)).to(dev), seed=5,
                            pairs=True)
    _risk_equal(cap.risk, moved)
    assert not torch.equal(moved.zone_count, want.zone_count)
    # keep_samples=False: the same risk and mean, no samples -- eager and captured
    lean = Predictor(m, k, risk=spec, keep_samples=False)
    le = lean.predict(obs, pd, seed=5)
    assert tuple(le.samples.shape) == (0, n, P, v, 2)
    assert torch.equal(le.mean, e.mean) and torch.equal(le.v_pred, e.v_pred)
    _risk_equal(lean.risk, want)
    lr = lean.capture(n, v, pd)(obs, seed=5)
    assert tuple(lr.samples.shape) == (0, n, P, v, 2) and torch.equal(lr.mean, e.mean)
    _risk_equal(lean.risk, want)
    # explicit noise goes to both kernels
    noise = torch.randn((k, n, P, v, 2), generator=gen).to(dev)
    en = pr.predict(obs, pd, noise=noise)
    _risk_equal(pr.risk, ops.sample_risk(en.v_pred, obs[:, -1], pd, k, 0.8, torch.from_numpy(ZONES).to(dev), noise=noise,
                                         pairs=True))


def test_captured_streams_predictor_with_per_stream_zones(dev):
    """3 streams, per-stream rectangles, stream 1 never pushed: every stream's counts are ops.sample_risk's on the
    tick's batch; the stream that was not pushed is all zeros / -1."""
    from social_stgcnn_amd import frames, ops
    from social_stgcnn_amd.predict import RiskSpec
    m = _model("eth", dev)
    ns, v, k = 3, 16, 6
    zones = np.stack([ZONES, ZONES + np.float32(1.0), ZONES[::-1].copy()])
    spec = RiskSpec(1.0, zones, True)
    sp = frames.StreamsPredictor(m, ns, k=k, max_peds=v, risk=spec)
    assert sp.risk is None
    replay = sp.capture()
    fp = frames.FramePredictor(m, k=k, max_peds=v, risk=RiskSpec(1.0, ZONES), keep_samples=False)
    rng = np.random.default_rng(2)
    ids = [np.arange(10), None, np.arange(100, 107)]
    pos = [rng.uniform(-2, 2, (10, 2)), None, rng.uniform(-1, 3, (7, 2))]
    for t in range(9):
        tick = [None if i is None else (i, x + 0.3 * t + 0.05 * rng.standard_normal(x.shape)) for i, x in zip(ids, pos)]
        out = replay(tick, seed=t)
        one = fp.push(*tick[0], seed=t)
    assert out.num_peds.cpu().tolist() == [10, 0, 7] and tuple(out.samples.shape) == (k, ns, P, v, 2)
    want = ops.sample_risk(out.v_pred, out.obs_abs[:, -1].to(torch.float32), out.num_peds, k, 1.0,
                           torch.from_numpy(zones).to(dev), seed_dev=sp.seed_dev, pairs=True)
    _risk_equal(sp.risk, want)
    got = _host(sp.risk)
    assert got["conflict_any"][0].max() > 0 and got["zone_count"][0].max() > 0
    for f in FIELDS:
        assert np.all(got[f][1] == (-1 if f == "partner" else 0)), f
    assert torch.equal(sp.zones, torch.from_numpy(zones).to(dev))
    # the single-stream predictor: its own scene, counts present, no samples
    assert tuple(one.samples.shape) == (0, P, v, 2) and int(one.num_peds) == 10
    assert fp.risk.pair is None and tuple(fp.risk.conflict.shape) == (1, P, v) and fp.risk.zone_count.max() > 0


def test_predict_frames_command_writes_the_risk_arrays(dev, tmp_path):
    from social_stgcnn_amd import data, frames, ops, predict_frames
    from social_stgcnn_amd.trainer import Checkpoint
    model = _model("eth", dev)
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    src = open(os.path.join(DATA, "eth_test", "biwi_eth.txt")).read().splitlines(True)
    rec = str(tmp_path / "short.txt")
    with open(rec, "w") as fh:
        fh.writelines(src[:260])
    rows = data.read_file(rec)
    base = ["--checkpoint", ck.dir, "--recording", rec, "--ksteps", "5", "--seed", "3"]
    plain, risky = str(tmp_path / "plain.npz"), str(tmp_path / "risk.npz")
    predict_frames.main(base + ["--out", plain])
    predict_frames.main(base + ["--radius", "1.5", "--zones", "-1,-1,1,1", "0,0,14,9", "--out", risky])
    a, b = np.load(plain), np.load(risky)
    # without the flags: the arrays the command wrote before, equal to predict_recording's
    assert sorted(a.files) == ["frame", "ids", "mean", "num_peds", "samples"]
    sc, pr = frames.predict_recording(model, rows, k=5, seed=3)
    assert len(sc.frame) > 3
    assert np.array_equal(a["frame"], sc.frame) and np.array_equal(a["ids"], sc.ids.cpu().numpy())
    assert np.array_equal(a["num_peds"], sc.num_peds.cpu().numpy())
    assert np.array_equal(a["mean"], pr.mean.cpu().numpy()) and np.array_equal(a["samples"], pr.samples.cpu().numpy())
    for name in a.files:
        assert np.array_equal(a[name], b[name]), name
    zones = np.array([[-1, -1, 1, 1], [0, 0, 14, 9]], np.float32)
    assert int(b["risk_k"]) == 5 and np.array_equal(b["risk_zones"], zones)
    obs_last = sc.obs_abs[:, -1].to(torch.float32)
    parts = [_host(ops.sample_risk(pr.v_pred[lo:lo + 64], obs_last[lo:lo + 64], sc.num_peds[lo:lo + 64], 5, 1.5,
                                   torch.from_numpy(zones).to(dev), seed=3 + b, pairs=True))
             for b, lo in enumerate(range(0, len(sc.frame), 64))]           # predict_recording's batches and seeds
    want = {f: np.concatenate([q[f] for q in parts]) for f in FIELDS}
    assert sorted(b.files) == sorted(a.files + ["risk_k", "risk_zones"] + ["risk_" + f for f in FIELDS])
    for f in FIELDS:
        assert np.array_equal(b["risk_" + f], want[f]), f
    assert len(b["risk_conflict"]) == len(b["frame"]) and b["risk_zone_count"].max() > 0
