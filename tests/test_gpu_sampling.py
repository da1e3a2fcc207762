"""GPU (-m gpu): stg_sample_trajectories / ops.sample_trajectories, the Predictor and sample_test.

The reference's own sampled trajectories on eth/test come back (samples_eth.npz, tests/golden/make_golden_samples.py);
the in-kernel normal stream is the documented Philox stream (tests/philox_np.py); best-of-K over the samples is what
stg_bestofk_eval reports; the mean trajectory, padding, sample statistics; the Predictor from absolute tracks, eager
and captured."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import philox_np
from sampling_inputs import random_pred as _random_pred

pytestmark = pytest.mark.gpu
CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _eth_windows():
    from social_stgcnn_amd import data
    g = load_golden("eval_splits.npz")
    win = data.load_windows(os.path.join(GOLDEN, "data", "eth_test"), 8, 12, 1, with_non_linear=False)
    assert np.array_equal(win.num_peds, g["eth/num_peds"])
    return win


def _eth_model(dev):
    from social_stgcnn_amd.model import social_stgcnn
    w = load_golden("weights_eth.npz")
    m = social_stgcnn(**CFG)
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    return m.to(dev).eval()


def _reference_noise_fn(win):
    """The reference sampler's standard-normal stream: after torch.manual_seed(0), per scene and sample one
    randn(P, V_i, 2) (test.py:87-89)."""
    at = [0]

    def noise_fn(b, shape):
        k, n, p, v, _ = shape
        out = torch.zeros(shape)
        for i in range(n):
            c = int(win.num_peds[at[0] + i])
            for kk in range(k):
                out[kk, i, :, :c] = torch.randn(p, c, 2)
        at[0] += n
        return out
    return noise_fn


def _host_samples(y, obs_last, noise):
    """float64 statement of the kernel: obs_last + cumsum_t(mu_t + chol(cov_t) eps).  y (N,5,P,V), obs_last (N,V,2),
    noise (K,N,P,V,2) -> (K,N,P,V,2)."""
    y = np.asarray(y, np.float64)
    mx, my = y[:, 0], y[:, 1]
    sx, sy, rho = np.exp(y[:, 2]), np.exp(y[:, 3]), np.tanh(y[:, 4])
    ex, ey = noise[..., 0], noise[..., 1]
    dx = mx + sx * ex
    dy = my + rho * sy * ex + np.sqrt(1.0 - rho * rho) * sy * ey
    return np.stack([np.cumsum(dx, axis=2), np.cumsum(dy, axis=2)], axis=-1) + obs_last[None, :, None]


def _valid(num_peds, v):
    return np.arange(v)[None, :] < np.asarray(num_peds)[:, None]                  # (N,V)


def _vp(a):
    """(..., N, P, V, 2) -> (..., N, V, P, 2): an (N,V) pedestrian mask then indexes the scene / pedestrian axes."""
    return np.moveaxis(np.asarray(a), -3, -2)


def test_sample_test_returns_the_reference_trajectories(dev):
    """sample_test on eth/test, fed the reference sampler's own normals, gives back the reference test()'s
    raw_data_dict (obs / trgt / K = 20 sampled trajectories per window) and its ADE / FDE."""
    from social_stgcnn_amd.predict import sample_test
    win, m = _eth_windows(), _eth_model(dev)
    s, g = load_golden("samples_eth.npz"), load_golden("eval_splits.npz")
    torch.manual_seed(0)
    ade, fde, raw = sample_test(m, win, k=20, batch_size=64, noise_fn=_reference_noise_fn(win))
    assert sorted(raw) == list(range(1, len(win) + 1))
    for st in raw:
        c = int(win.num_peds[st - 1])
        assert raw[st]["obs"].shape == (8, c, 2) and raw[st]["trgt"].shape == (12, c, 2)
        assert len(raw[st]["pred"]) == 20 and all(p.shape == (12, c, 2) and p.dtype == np.float32
                                                  for p in raw[st]["pred"])
    steps = range(1, len(win) + 1)
    obs = np.concatenate([raw[st]["obs"] for st in steps], axis=1)
    trgt = np.concatenate([raw[st]["trgt"] for st in steps], axis=1)
    pred = np.stack([np.concatenate([raw[st]["pred"][k] for st in steps], axis=1) for k in range(20)])
    e_o, e_t, e_p = (float(np.abs(a - s[n]).max()) for a, n in ((obs, "obs"), (trgt, "trgt"), (pred, "pred")))
    print("eth/test vs reference raw_data_dict: obs %.2e trgt %.2e pred %.2e; ADE %.6f (%.6f) FDE %.6f (%.6f)"
          % (e_o, e_t, e_p, ade, float(g["eth/ade"]), fde, float(g["eth/fde"])))
    assert e_o < 1e-5 and e_t < 1e-5 and e_p < 1e-4
    assert abs(ade - float(g["eth/ade"])) < 5e-5 and abs(fde - float(g["eth/fde"])) < 5e-5


def test_in_kernel_stream_is_the_documented_philox_stream(dev):
    """mu = 0, sigma = 1, rho = 0: the first differences of the samples are the kernel's normals, which must be the
    numpy replay's.  V = 40 (20 pedestrian pairs per scene) so waves cut scenes; ragged; K = 7."""
    from social_stgcnn_amd import ops
    n, p, v, k = 9, 12, 40, 7
    peds = np.array([40, 3, 17, 40, 0, 39, 2, 40, 21], dtype=np.int32)
    gen = torch.Generator().manual_seed(11)
    y = torch.zeros((n, 5, p, v), device=dev)
    obs_last = (torch.rand((n, v, 2), generator=gen) * 10 - 5).to(dev)
    pd = torch.from_numpy(peds).to(dev)
    samples, mean = ops.sample_trajectories(y, obs_last, pd, k=k, seed=1234)
    s = samples.cpu().numpy().astype(np.float64)
    start = np.broadcast_to(obs_last.cpu().numpy()[None, :, None], (k, n, 1, v, 2))
    eps = np.diff(np.concatenate([start, s], axis=2), axis=2)
    want = philox_np.noise_tensor(1234, k, n, p, v)
    ok = _valid(peds, v)
    err = float(_vp(np.abs(eps - want))[:, ok].max())
    print("in-kernel normals vs numpy replay: max diff %.2e" % err)
    assert err < 1e-5
    assert np.all(_vp(s)[:, ~ok] == 0) and np.all(_vp(mean.cpu().numpy())[~ok] == 0)
    seed_dev = torch.tensor([1234], dtype=torch.int64, device=dev)
    s2, _ = ops.sample_trajectories(y, obs_last, pd, k=k, seed=99, seed_dev=seed_dev)
    assert torch.equal(s2, samples)                       # the device seed wins over the argument
    big = (1 << 64) - 3                                    # a seed above 2^63 travels as the same 64 bits
    s3, _ = ops.sample_trajectories(y, obs_last, pd, k=k, seed=big)
    s4, _ = ops.sample_trajectories(y, obs_last, pd, k=k, seed_dev=torch.tensor([big - (1 << 64)], device=dev))
    assert torch.equal(s3, s4)
    s5, _ = ops.sample_trajectories(y, obs_last, pd, k=k, seed=1235)
    diff = _vp((s5 - samples).abs().cpu().numpy())[:, ok]
    assert (diff > 1e-3).mean() > 0.99


@pytest.mark.parametrize("noise", [False, True])
def test_best_of_k_over_samples_equals_stg_bestofk_eval(dev, noise):
    """Random V_pred (rho != 0, unequal sigmas) as a permuted view, ragged, obs_last, K = 20: min ADE / FDE over the
    samples is ops.best_of_k's for the same seed, and for the same caller-provided noise."""
    from social_stgcnn_amd import ops
    n, p, v, k = 37, 12, 24, 20
    gen = torch.Generator().manual_seed(5)
    y = _random_pred(gen, n, p, v, dev)
    assert not y.is_contiguous()
    peds = torch.randint(2, v + 1, (n,), generator=gen, dtype=torch.int32)
    peds[3] = v
    pd = peds.to(dev)
    tgt = (torch.randn((n, p, v, 2), generator=gen) * 0.4).to(dev)
    obs_last = (torch.rand((n, v, 2), generator=gen) * 20 - 10).to(dev)
    nz = torch.randn((k, n, p, v, 2), generator=gen).to(dev) if noise else None
    samples, _ = ops.sample_trajectories(y, obs_last, pd, k=k, noise=nz, seed=77)
    a_ref, f_ref = ops.best_of_k(y, tgt, obs_last, pd, k, nz, 77)
    gt = obs_last[None, :, None] + torch.cumsum(tgt, dim=1)[None]                     # (1,N,P,V,2)
    err = torch.sqrt(((samples - gt) ** 2).sum(-1))                                   # (K,N,P,V)
    ade = err.mean(dim=2).min(dim=0).values
    fde = err[:, :, -1].min(dim=0).values
    ok = torch.from_numpy(_valid(peds.numpy(), v)).to(dev)
    ea = float((ade - a_ref)[ok].abs().max())
    ef = float((fde - f_ref)[ok].abs().max())
    print("best-of-%d from samples vs stg_bestofk_eval (noise=%s): ADE %.2e FDE %.2e" % (k, noise, ea, ef))
    assert ea < 1e-5 and ef < 1e-5
    if nz is not None:                                    # caller noise: the float64 statement of the kernel
        want = _host_samples(y.cpu().numpy(), obs_last.cpu().numpy(), nz.cpu().numpy().astype(np.float64))
        assert float(_vp(np.abs(samples.cpu().numpy() - want))[:, _valid(peds.numpy(), v)].max()) < 1e-4


def test_mean_trajectory_padding_k0_and_empty_batch(dev):
    from social_stgcnn_amd import ops
    n, p, v, k = 6, 12, 7, 3                              # odd V: one pedestrian per lane
    gen = torch.Generator().manual_seed(8)
    y = _random_pred(gen, n, p, v, dev)
    peds = np.array([7, 2, 5, 1, 0, 6], dtype=np.int32)
    y.permute(0, 3, 1, 2)[torch.from_numpy(~_valid(peds, v)).to(dev)] = 7.0       # junk in the padded slots
    pd = torch.from_numpy(peds).to(dev)
    obs_last = (torch.rand((n, v, 2), generator=gen) * 4).to(dev)
    samples, mean = ops.sample_trajectories(y, obs_last, pd, k=k, seed=3)
    ok = _valid(peds, v)
    want = obs_last.cpu().numpy()[:, None] + np.cumsum(y.cpu().numpy()[:, 0:2].transpose(0, 2, 3, 1), axis=1)
    m = mean.cpu().numpy()
    assert float(_vp(np.abs(m - want))[ok].max()) < 1e-6
    assert np.all(_vp(m)[~ok] == 0)
    assert np.all(_vp(samples.cpu().numpy())[:, ~ok] == 0)
    # K = 0 with the mean only
    s0, m0 = ops.sample_trajectories(y, obs_last, pd, k=0)
    assert s0.shape == (0, n, p, v, 2) and torch.equal(m0, mean)
    # obs_last None: from the origin; even V with an output view that is 8- but not 16-byte aligned takes the
    # one-pedestrian kernel
    buf = torch.full((k * n * p * 8 * 2 + 2,), 5.0, device=dev)
    y8 = _random_pred(gen, n, p, 8, dev)
    out = buf[2:].view(k, n, p, 8, 2)
    s_al, _ = ops.sample_trajectories(y8, None, pd, k=k, seed=3)
    s_un, _ = ops.sample_trajectories(y8, None, pd, k=k, seed=3, samples=out)
    assert s_un.data_ptr() == out.data_ptr() and torch.equal(s_al, s_un) and float(buf[:2].min()) == 5.0
    # N = 0 is a no-op
    e_s, e_m = ops.sample_trajectories(torch.zeros((0, 5, p, v), device=dev), None, None, k=k)
    assert e_s.shape == (k, 0, p, v, 2) and e_m.shape == (0, p, v, 2)
    torch.cuda.synchronize()


def test_sample_statistics(dev):
    """One scene, V = 64, K = 8192 in-kernel draws, sigma_x != sigma_y, rho = +-0.8: the first-step displacement's
    mean and covariance lie within 5 standard errors; increments are uncorrelated across time (|r| < 5 / sqrt(K))."""
    from social_stgcnn_amd import ops
    p, v, k = 12, 64, 8192
    y = torch.zeros((1, 5, p, v))
    y[0, 0], y[0, 1] = 0.3, -0.2
    y[0, 2], y[0, 3] = math.log(0.5), math.log(1.5)
    rho = np.where(np.arange(v) % 2 == 0, 0.8, -0.8)
    y[0, 4] = torch.from_numpy(np.arctanh(rho)).float()[None, :]
    samples, _ = ops.sample_trajectories(y.to(dev), None, None, k=k, seed=2024)
    s = samples[:, 0].double().cpu().numpy()                                  # (K,P,V,2)
    d = s[:, 0]                                                               # first step, (K,V,2)
    sx, sy = 0.5, 1.5
    se = 5.0 / math.sqrt(k)
    assert np.all(np.abs(d[..., 0].mean(0) - 0.3) < se * sx) and np.all(np.abs(d[..., 1].mean(0) + 0.2) < se * sy)
    c = d - d.mean(0)
    var_x, var_y, cov = (c[..., 0] ** 2).mean(0), (c[..., 1] ** 2).mean(0), (c[..., 0] * c[..., 1]).mean(0)
    assert np.all(np.abs(var_x - sx * sx) < se * math.sqrt(2) * sx * sx)
    assert np.all(np.abs(var_y - sy * sy) < se * math.sqrt(2) * sy * sy)
    assert np.all(np.abs(cov - rho * sx * sy) < se * sx * sy * np.sqrt(1 + rho * rho))
    inc = np.diff(s, axis=1)                                                  # (K,P-1,V,2)
    for comp in range(2):
        a, b = inc[:, :-1, :, comp], inc[:, 1:, :, comp]
        a, b = a - a.mean(0), b - b.mean(0)
        r = (a * b).mean(0) / np.sqrt((a * a).mean(0) * (b * b).mean(0))     # (P-2,V)
        assert float(np.abs(r).max()) < 5.0 / math.sqrt(k)


def test_predictor_from_absolute_tracks_matches_the_dataset_path(dev):
    """Predictor.predict on eth/test's observed absolute tracks (float64, as the dataset holds them): V_pred equals
    the dataset path (relative coordinates from the loader, graphs by adj_build) to 1e-5.  The first differences are
    taken on the device here, on the host in the loader."""
    from social_stgcnn_amd import data, ops
    from social_stgcnn_amd.predict import Predictor
    win, m = _eth_windows(), _eth_model(dev)
    m.train()
    pr = Predictor(m, k=20)
    worst = 0.0
    for lo in range(0, len(win), 64):
        idx = np.arange(lo, min(len(win), lo + 64))
        obs_rel, _, obs_abs, _, counts = data.pad_batch(win, idx)
        obs64 = np.zeros(obs_abs.shape)
        for j, i in enumerate(idx):
            s0, e0 = win.seq_start_end[i]
            obs64[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))
        assert np.array_equal(obs64.astype(np.float32), obs_abs)
        peds = torch.from_numpy(counts).to(dev)
        res = pr.predict(torch.from_numpy(obs64).to(dev), peds, seed=lo)
        assert m.training                                   # the model's mode is restored
        nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev).permute(0, 2, 3, 1), peds)
        m.eval()
        with torch.no_grad():
            y, _ = m(nodes.permute(0, 3, 1, 2), adj, peds)
        m.train()
        ok = torch.from_numpy(_valid(counts, y.shape[3])).to(dev)
        worst = max(worst, float((res.v_pred - y).abs().permute(0, 3, 1, 2)[ok].max()))
        assert res.samples.shape == (20, len(idx), 12, y.shape[3], 2)
        ol = torch.from_numpy(obs_abs[:, -1]).to(dev)
        _, mean = ops.sample_trajectories(res.v_pred, ol, peds, k=0)
        assert torch.equal(mean, res.mean)
    print("Predictor V_pred vs dataset path: %.2e" % worst)
    assert worst < 1e-5


def _synthetic_tracks(gen, n, v, t=8):
    start = torch.rand((n, 1, v, 2), generator=gen) * 20 - 10
    steps = torch.randn((n, t - 1, v, 2), generator=gen) * 0.3 + 0.2
    tracks = torch.cat([start, start + torch.cumsum(steps, dim=1)], dim=1)
    peds = torch.randint(2, v + 1, (n,), generator=gen, dtype=torch.int32)
    tracks = tracks * torch.from_numpy(_valid(peds.numpy(), v)).float()[:, None, :, None]
    return tracks, peds


def test_captured_predictor_replays_eager(dev):
    """One graph for rel -> adj_build -> forward -> sampling: replay equals eager bitwise; a new seed changes the
    samples and the old one reproduces them; refreshed tracks give the eager result for the new tracks."""
    from social_stgcnn_amd import data
    from social_stgcnn_amd.predict import Predictor
    win, m = _eth_windows(), _eth_model(dev)
    pr = Predictor(m, k=20)
    idx = np.arange(0, 64)
    _, _, obs_abs, _, counts = data.pad_batch(win, idx)
    obs = torch.from_numpy(obs_abs).to(dev)
    peds = torch.from_numpy(counts).to(dev)
    replay = pr.capture(len(idx), obs.shape[2], peds)
    r1 = replay(obs, seed=5)
    first = r1.samples.clone()
    e1 = pr.predict(obs, peds, seed=5)
    assert torch.equal(r1.samples, e1.samples) and torch.equal(r1.mean, e1.mean) and torch.equal(r1.v_pred, e1.v_pred)
    r2 = replay(obs, seed=6)
    assert not torch.equal(r2.samples, first)
    r3 = replay(obs, seed=5)
    assert torch.equal(r3.samples, first)
    gen = torch.Generator().manual_seed(3)
    ok = torch.from_numpy(_valid(counts, obs.shape[2])).float()[:, None, :, None].to(dev)
    obs2 = obs + (torch.randn(obs.shape, generator=gen) * 0.05).to(dev) * ok
    r4 = replay(obs2)                                   # the seed stays 5
    e4 = pr.predict(obs2, peds, seed=5)
    assert torch.equal(r4.samples, e4.samples) and torch.equal(r4.v_pred, e4.v_pred)
    assert not torch.equal(r4.samples, first)


def test_captured_predictor_at_bench_size(dev):
    """N = 2048, V = 32, K = 20 (1.3 M sampled pedestrian trajectories): replay equals eager bitwise, and a seeded
    sub-sample of scenes equals the float64 statement of the sampling on the replay's own V_pred with the numpy
    replay of the Philox stream."""
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import Predictor
    n, v, k = 2048, 32, 20
    torch.manual_seed(0)
    m = social_stgcnn(**CFG).to(dev).eval()
    gen = torch.Generator().manual_seed(21)
    tracks, peds = _synthetic_tracks(gen, n, v)
    obs, pd = tracks.to(dev), peds.to(dev)
    pr = Predictor(m, k=k)
    replay = pr.capture(n, v, pd)
    r = replay(obs, seed=0xC0FFEE)
    e = pr.predict(obs, pd, seed=0xC0FFEE)
    assert torch.equal(r.samples, e.samples) and torch.equal(r.mean, e.mean)
    rng = np.random.default_rng(4)
    sub = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), 14, replace=False)]))
    sub_t = torch.from_numpy(sub).to(dev)
    y = r.v_pred.index_select(0, sub_t).cpu().numpy()
    got = r.samples.index_select(1, sub_t).cpu().numpy()
    noise = philox_np.noise_tensor(0xC0FFEE, k, n, 12, v, scenes=sub)
    want = _host_samples(y, tracks[sub, -1].numpy().astype(np.float64), noise)
    ok = _valid(peds.numpy()[sub], v)
    err = float(_vp(np.abs(got - want))[:, ok].max())
    print("bench-size replay, %d scenes vs float64 host sampling: %.2e" % (len(sub), err))
    assert err < 1e-4
    assert np.all(_vp(got)[:, ~ok] == 0)
