"""The table-free Shape::Canon32 scene kernels (txp_x6.hip) against the Shape::Canon build, which keeps the position
table: a uniform batch of 32 pedestrians per scene runs Canon32 without num_peds and Canon with num_peds = 32 for every
scene.  Canon32 takes every tile's row and column from compile-time constants and the lane id instead of the table, so
only address arithmetic differs: V_pred and the per-scene losses must be bitwise equal, the parameter gradients (the
reduction order over scenes may differ, nothing else) within 2e-5 * max(1, max|g|), everything finite.

The solo kernels only run for uniform V = 32 batches of at least 1536 scenes (smaller ones are cut into teams of waves):
N = 1536 in both storage modes (the saved row strides differ with bf16 storage; its forward with num_peds is the Generic
build, a table kernel as well), and N = 2050, where two waves walk a second scene and rebuild their per-scene lane
bases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 32


def _run(dev, x, adj, tgt, w, peds, bf16_store):
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.model import social_stgcnn
    torch.manual_seed(21)
    m = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12).to(dev).train()
    m.options = ops.KernelOptions(bf16_store=bf16_store)
    y, _ = m(x, adj, peds)
    losses = ops.backward_from_target(m, y.detach(), tgt, w)
    assert losses is not None
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().double()) for k, p in m.named_parameters()}
    return y.detach().cpu(), losses.detach().cpu(), grads


@pytest.mark.parametrize("n,bf16_store", [(1536, False), (2050, False), (1536, True)])
def test_table_free_canon32_equals_the_table_build(n, bf16_store):
    import bench
    from social_stgcnn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    dev = torch.device("cuda", 0)
    obs_rel, target = bench.synth_scenes(n, V, 77)
    nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev))
    x, tgt = nodes.permute(0, 3, 1, 2), torch.from_numpy(target).to(dev)
    w = torch.rand(n, generator=torch.Generator().manual_seed(8)).to(dev)
    y32, l32, g32 = _run(dev, x, adj, tgt, w, None, bf16_store)                  # Canon32: no table
    peds = torch.full((n,), V, dtype=torch.int32, device=dev)
    yc, lc, gc = _run(dev, x, adj, tgt, w, peds, bf16_store)                     # Canon: the runtime table
    assert torch.isfinite(y32).all() and torch.isfinite(l32).all()
    assert torch.isfinite(yc).all() and torch.isfinite(lc).all()
    assert float(y32.abs().max()) > 0 and float(l32.abs().max()) > 0
    assert torch.equal(y32, yc), float((y32 - yc).abs().max())
    assert torch.equal(l32, lc), float((l32 - lc).abs().max())
    gmax = max(float(g.abs().max()) for g in gc.values() if g is not None)
    for k, g in gc.items():
        assert (g is None) == (g32[k] is None), k
        if g is None:
            continue
        assert np.isfinite(g32[k].numpy()).all() and np.isfinite(g.numpy()).all(), k
        err = float((g32[k] - g).abs().max())
        print("N=%d bf16_store=%s %s: max|dg| %.3e (bar %.3e)" % (n, bf16_store, k, err, 2e-5 * max(1.0, gmax)))
        assert err <= 2e-5 * max(1.0, gmax), (k, err, gmax)
