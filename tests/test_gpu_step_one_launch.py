"""The training step in one library call (stg_model_step) with the forward and the backward scene kernels as ONE launch
(txp_x6.hip, txp_step_x6_kernel) against the same call forced to two launches (KernelOptions(separate_fb=True)) and
against the two calls it replaces (stg_model_fwd + stg_model_bwd_step).

The one launch runs the solo kernels' own scene functions one behind the other in the same wave, every arithmetic
operation and its order unchanged, so everything is compared BITWISE: the reported loss, the per-scene losses, V_pred and
every state_dict entry after two consecutive steps from the seeded initial weights, eager and captured.

Canonical model, V = 32, uniform: N = 1, 3 and 5 (fewer scenes than a workgroup has waves, one workgroup crossed -- batches
this small are cut into teams of waves by both passes, so they check that the new entry point keeps that path; one launch
serves both passes above 1024 scenes only).  N = 1027 and N = 2050 run the one launch with a partly filled last workgroup
(three and two of its four waves have a scene: the others must leave behind the workgroup's barrier without writing past
scene N into the workspace, V_pred, the gradient rows or the dz hand-off -- arrays that lie one behind the other, so a
stray scene lands in what is compared).  N = 2052 (more scenes than the chip's 2048 wave slots: the one-launch kernel has
no scene loop, its 513th workgroup starts in the slot and the LDS region that a finished one leaves behind after a backward
pass, where the separate kernels' waves walk a second scene).  bf16 storage at N = 5, 1027 and 2052.  Two batches that
must fall back to two launches whatever the switch says: V = 32 with a num_peds vector, and V = 28."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(dev, options):
    from social_stgcnn_amd.model import social_stgcnn
    torch.manual_seed(5)
    m = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12).to(dev).train()
    m.options = options
    return m


def _batch(dev, n, v, peds):
    import bench
    from social_stgcnn_amd import ops
    obs_rel, target = bench.synth_scenes(n, v, 31)
    peds_d = None if peds is None else torch.full((n,), peds, dtype=torch.int32, device=dev)
    nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev), peds_d)
    w = torch.rand(n, generator=torch.Generator().manual_seed(3)).to(dev) / n
    return nodes.permute(0, 3, 1, 2), adj, torch.from_numpy(target).to(dev), peds_d, w


def _two_steps(dev, batch, mode, **opts):
    """[(total, losses, V_pred) of step 1 and 2, state_dict after them]"""
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.trainer import Trainer
    x, adj, tgt, peds, w = batch
    m = _model(dev, ops.KernelOptions(**opts))
    tr = Trainer(m, lr=0.01)
    if mode == "two_calls":                            # what Trainer.step ran before stg_model_step
        def step():
            for p in m.parameters():
                p.grad = None
            y, _ = m._forward(x, adj, peds, True)
            losses, total = ops.backward_from_target(m, y.detach(), tgt, w, (tr.lr, tr._lr_tensor(dev)))
            return total, losses, y.detach()
    elif mode == "captured":
        step = tr.capture(x, adj, tgt, peds, w, warmup=1)
    else:
        def step():
            return tr.step(x, adj, tgt, peds, w)
    out = []
    for _ in range(2):
        total, losses, y = step()
        out.append((total.detach().clone().cpu().reshape(()), losses.detach().clone().cpu(), y.detach().clone().cpu()))
    torch.cuda.synchronize()
    return out, {k: t.detach().clone().cpu() for k, t in m.state_dict().items()}


def _assert_same(a, b, what):
    (steps_a, state_a), (steps_b, state_b) = a, b
    for k, (sa, sb) in enumerate(zip(steps_a, steps_b)):
        for name, ta, tb in zip(("loss", "losses", "V_pred"), sa, sb):
            assert torch.isfinite(ta).all(), (what, k, name)
            assert torch.equal(ta, tb), (what, "step %d" % k, name, float((ta - tb).abs().max()))
    assert state_a.keys() == state_b.keys()
    for k in state_a:
        assert torch.equal(state_a[k], state_b[k]), (what, k, float((state_a[k].float() - state_b[k].float()).abs().max()))


CASES = [(1, 32, None, False), (3, 32, None, False), (5, 32, None, False), (1027, 32, None, False),
         (2050, 32, None, False), (2052, 32, None, False),
         (5, 32, None, True), (1027, 32, None, True), (2052, 32, None, True),
         (1540, 32, 32, False), (1540, 28, None, False)]                # (the last two: no one-launch form)


@pytest.mark.parametrize("n,v,peds,bf16", CASES)
def test_one_launch_step_is_bitwise_the_two_launches(n, v, peds, bf16):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    dev = torch.device("cuda", 0)
    batch = _batch(dev, n, v, peds)
    ref = _two_steps(dev, batch, "two_calls", bf16_store=bf16)
    assert float(ref[0][0][2].abs().max()) > 0 and float(ref[0][0][1].abs().max()) > 0
    assert not torch.equal(ref[0][0][2], ref[0][1][2]), "the second step must run on updated weights"
    for mode in ("eager", "captured"):
        one = _two_steps(dev, batch, mode, bf16_store=bf16)
        two = _two_steps(dev, batch, mode, bf16_store=bf16, separate_fb=True)
        _assert_same(one, two, "%s: one launch vs separate launches" % mode)
        _assert_same(one, ref, "%s: stg_model_step vs stg_model_fwd + stg_model_bwd_step" % mode)


def _kernel_ms(dev, batch, **opts):
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.trainer import Trainer
    x, adj, tgt, peds, w = batch
    m = _model(dev, ops.KernelOptions(**opts))
    tr = Trainer(m, lr=0.01)
    tr.step(x, adj, tgt, peds, w)
    m.timer = ops.KernelTimer()
    for _ in range(3):
        tr.step(x, adj, tgt, peds, w)
    torch.cuda.synchronize()
    return m.timer.kernel_ms("model_fwd"), m.timer.kernel_ms("model_bwd")


@pytest.mark.parametrize("n", [1027, 2052])
def test_one_launch_reports_one_interval_in_the_backward_slot(n):
    """the kernel timer's five slots (aggregation, F | B, K2, reduction) keep their places: with one launch the forward
    scene kernel's slot is an empty interval (two events back to back) and the backward's holds both stages -- which
    also shows that these batches do run the one launch, N = 1027 with a partly filled last workgroup"""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    dev = torch.device("cuda", 0)
    batch = _batch(dev, n, 32, None)
    f1, b1 = _kernel_ms(dev, batch)
    f2, b2 = _kernel_ms(dev, batch, separate_fb=True)
    print("one launch: fwd %s bwd %s ms   separate: fwd %s bwd %s ms" % (f1[:2], b1[:3], f2[:2], b2[:3]))
    assert len(f1) >= 2 and len(b1) >= 3 and len(f2) >= 2 and len(b2) >= 3
    # separate: F is a scene kernel of tens of microseconds; one launch: nothing runs between the two events
    assert f1[1] < 0.25 * f2[1], (f1, f2)
    # the one launch holds both stages: longer than the backward alone
    assert b1[0] > b2[0], (b1, b2)
