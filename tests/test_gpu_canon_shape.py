"""The canonical model's folded scene kernels (txp_x6.hip): a uniform batch of 32 pedestrians per scene runs
Shape::Canon32 without num_peds and Shape::Canon with num_peds = 32 for every scene.  Only integer and address
arithmetic differs between the two, so V_pred and the per-scene losses must be bitwise equal; the parameter
gradients (a different scene order inside the reductions is allowed) meet the bars of the parity tests."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 1536 uniform scenes of 32: the solo wave-per-scene kernels (smaller batches of 32 are cut into teams of waves)
N, V = 1536, 32


def _run(dev, x, adj, tgt, w, peds):
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.model import social_stgcnn
    torch.manual_seed(21)
    m = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12).to(dev).train()
    y, _ = m(x, adj, peds)
    losses = ops.backward_from_target(m, y.detach(), tgt, w)
    assert losses is not None
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().double()) for k, p in m.named_parameters()}
    return y.detach().cpu(), losses.detach().cpu(), grads


def test_canon32_equals_canon_on_a_uniform_batch():
    import bench
    from social_stgcnn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    dev = torch.device("cuda", 0)
    obs_rel, target = bench.synth_scenes(N, V, 77)
    nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev))
    x, tgt = nodes.permute(0, 3, 1, 2), torch.from_numpy(target).to(dev)
    w = torch.rand(N, generator=torch.Generator().manual_seed(8)).to(dev)
    y32, l32, g32 = _run(dev, x, adj, tgt, w, None)
    peds = torch.full((N,), V, dtype=torch.int32, device=dev)
    yc, lc, gc = _run(dev, x, adj, tgt, w, peds)
    assert torch.isfinite(y32).all() and torch.isfinite(l32).all()
    assert torch.equal(y32, yc), float((y32 - yc).abs().max())
    assert torch.equal(l32, lc), float((l32 - lc).abs().max())
    gmax = max(float(g.abs().max()) for g in gc.values() if g is not None)
    for k, g in gc.items():
        assert (g is None) == (g32[k] is None), k
        if g is None:
            continue
        err = float((g32[k] - g).abs().max())
        assert err <= 2e-5 * max(1.0, gmax), (k, err, gmax)
        assert np.isfinite(g32[k].numpy()).all(), k
