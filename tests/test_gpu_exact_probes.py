"""GPU (-m gpu): EXACT-CLASS PROBES of the convolutions inside the scene kernels -- bit-exact, no tolerance anywhere.

Each case is one probe of tests/exact_probes.py (a full model and a batch built so that the float64 oracle's result is
a float32 value reached exactly by any float32 evaluation order; validity is checked on the CPU,
tests/test_exact_probes_cpu.py) run in eval mode (`bn_mode` 0, a runtime field of every compiled shape, so the
convolution code is the training step's) on one compiled variant of the scene kernels, reached by batch geometry and
options as tests/test_gpu_canon_shape.py and tests/test_gpu_step_one_launch.py reach them (exact_probes.variants).
Forward probes run stg_model_fwd: V_pred on the valid block of EVERY scene of the batch is asserted torch.equal to
float32(oracle64), the padding exactly zero.  Backward probes run stg_model_fwd with a workspace and stg_model_bwd from
the probe's sparse dy: every parameter gradient is asserted torch.equal, and dx on the workgroup path.  A failing case
names the variant, the focus (the convolution whose operands carry the wide values) and the operand class, which with
the completeness table points at a piece product, a K slot or an image offset.

Outside the exact class by design, and without probes: `split_bf16` (two-piece operands: the l products are dropped on
purpose) and `bf16_store` (saved planes rounded to bf16)."""
import numpy as np
import pytest
import torch

import exact_probes as EP
import layout_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", EP.probe_cases(), ids=repr)
def test_forward_probe_is_bit_exact(dev, case):
    from social_stgcnn_amd import ops
    v = case.variant
    pr = case.build()
    m = LC.make_model(*v.layout)
    m.load_state_dict(pr.state, strict=True)
    m = m.to(dev).eval()
    m.options = ops.KernelOptions(**v.options)
    xu, au, counts, idx = EP.batch_tensors(pr, v)
    sel = torch.from_numpy(idx).to(dev)
    x, adj = xu.to(dev)[sel], au.to(dev)[sel]
    peds = torch.from_numpy(counts).to(dev) if v.ragged else None
    with torch.no_grad():
        y, _ = m(x, adj, peds)
    assert m.last_ws_floats == 0
    want = torch.zeros((len(pr.scenes), EP.C_OUT, EP.T_PRED, v.vpad), dtype=torch.float32)
    for i, e in pr.expected.items():
        want[i, :, :, :e.shape[2]] = torch.from_numpy(e)
    want = want.to(dev)[sel]
    if not torch.equal(y, want):
        bad = (y != want).nonzero()
        n, c, p, w = (int(k) for k in bad[0])
        raise AssertionError("%s: %d of %d elements differ in %d scenes; first at scene %d (unique %d, %d pedestrians) "
                             "[c %d, t %d, v %d]: got %r, expected %r"
                             % (case.id, len(bad), y.numel(), len(torch.unique(bad[:, 0])), n, int(idx[n]),
                                int(counts[n]), c, p, w, float(y[n, c, p, w]), float(want[n, c, p, w])))


@pytest.mark.parametrize("case", EP.bwd_probe_cases(), ids=repr)
def test_backward_probe_is_bit_exact(dev, case):
    """stg_model_fwd with a workspace in eval mode, then stg_model_bwd from the probe's sparse dy: every parameter
    gradient torch.equal to float32 of the float64 oracle's autograd gradient (the parameters the reference's forward
    never reads have none on either side); on the workgroup path also dx, on every scene of the batch."""
    from social_stgcnn_amd import ops
    v = case.variant
    pr = case.build()
    m = LC.make_model(*v.layout)
    m.load_state_dict(pr.state, strict=True)
    m = m.to(dev).eval()
    m.options = ops.KernelOptions(**v.options)
    xu, au, counts, idx = EP.batch_tensors(pr, v)
    sel = torch.from_numpy(idx).to(dev)
    x, adj = xu.to(dev)[sel], au.to(dev)[sel]
    peds = torch.from_numpy(counts).to(dev) if v.ragged else None
    want_dx = v.name == "wg"
    x.requires_grad_(want_dx)
    dy = torch.zeros((len(idx), EP.C_OUT, EP.T_PRED, v.vpad), dtype=torch.float32)
    for n, (where, vals) in pr.dy.items():
        dy[n, where[:, 0], where[:, 1], where[:, 2]] = torch.from_numpy(vals)
    y, _ = m(x, adj, peds)
    assert m.last_ws_floats > 0
    y.backward(dy.to(dev))
    got = dict(m.named_parameters())
    assert set(got) == set(pr.grads)
    bad = []
    for k, p in got.items():
        if pr.grads[k] is None:
            assert p.grad is None, k
            continue
        g, e = p.grad.detach().cpu(), torch.from_numpy(pr.grads[k]).reshape(p.shape)
        if not torch.equal(g, e):
            at = tuple(int(i) for i in (g != e).nonzero()[0])
            bad.append("%s: %d of %d differ, first at %s: got %r, expected %r"
                       % (k, int((g != e).sum()), g.numel(), at, float(g[at]), float(e[at])))
    assert not bad, "%s\n  %s" % (case.id, "\n  ".join(bad))
    if want_dx:
        want = torch.zeros_like(x)
        for n, d in pr.dx.items():
            want[n, :, :, :d.shape[2]] = torch.from_numpy(d).to(dev)
        assert torch.equal(x.grad, want), (case.id, "dx")
