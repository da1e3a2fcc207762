"""The weight-gradient kernel compiled for the canonical model with uniform scenes of 32 pedestrians (txp_wgrad_bf16.hip,
Shape::Canon32) against the generic kernel it replaces for such batches (KernelOptions(generic_wgrad=True)).

The Canon32 form folds addresses, strides and predicates into constants; the item walk, the workgroup count, the slab
rows and the order of every floating-point operation are the generic kernel's, so everything is compared BITWISE.

Whole step: the reported loss, the per-scene losses, V_pred and every state_dict entry after two consecutive steps from
the seeded initial weights, eager and captured (the helpers of test_gpu_step_one_launch.py).  N = 1 (one item, one round),
3 (fewer scenes than a workgroup has waves), 90 (more items than a layer's ~87 workgroups: some workgroups run two rounds,
others one, and the second LDS image is used), 200 (three rounds, the last partly filled), 1027 (the one-launch step in
front, a partly filled last workgroup); bf16 storage (the 5-wave, one-image shape) at N = 3 and 200.  Two batches the
generic kernel serves whatever the option says: V = 32 with a num_peds vector, and V = 28.

Kernel alone: tools/micro/k2_bench on synthetic saved arrays with garbage in the channels no layer reads, the library's
kernel within 1e-6 of max |dW| of an fp64 host sum per layer (the bar of test_gpu_k2.py), and the slab of the Canon32
kernel against the generic kernel's: a difference of exactly 0."""
import os
import re
import subprocess

import pytest
import torch

import test_gpu_step_one_launch as one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "micro", "k2_bench")

pytestmark = pytest.mark.gpu


CASES = [(1, 32, None, False), (3, 32, None, False), (90, 32, None, False), (200, 32, None, False),
         (1027, 32, None, False), (3, 32, None, True), (200, 32, None, True),
         (90, 32, 32, False), (90, 28, None, False)]                   # (the last two: the generic kernel either way)


@pytest.mark.parametrize("n,v,peds,bf16", CASES)
def test_canon32_weight_gradient_step_is_bitwise_the_generic_kernels(n, v, peds, bf16):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    dev = torch.device("cuda", 0)
    batch = one._batch(dev, n, v, peds)
    for mode in ("eager", "captured"):
        canon = one._two_steps(dev, batch, mode, bf16_store=bf16)
        generic = one._two_steps(dev, batch, mode, bf16_store=bf16, generic_wgrad=True)
        (s1, s2), _ = canon
        assert float(s1[2].abs().max()) > 0 and float(s1[1].abs().max()) > 0
        assert not torch.equal(s1[2], s2[2]), "the second step must run on updated weights"
        one._assert_same(canon, generic, "%s: Canon32 vs generic weight-gradient kernel" % mode)


K2_CASES = [(n, bf16) for bf16 in (0, 1) for n in (1, 3, 90, 200)]


@pytest.mark.parametrize("n,bf16", K2_CASES, ids=["%d-32-%s" % (n, "bf16" if b else "fp32") for n, b in K2_CASES])
def test_canon32_kernel_alone_against_fp64_and_the_generic_kernel(n, bf16):
    if not os.path.exists(BIN):
        pytest.fail("tools/micro/k2_bench is not built (__graft_entry__.build() builds it)")
    env = dict(os.environ, K2_GARBAGE="1", K2_FP64="1")
    out = subprocess.run([BIN, str(n), "32", "0", str(bf16), "0"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"layer (\d+): shipped vs fp64 host: max \|diff\| (\S+) of (\S+)", out.stdout)
    same = re.findall(r"canon32 against generic: max \|diff\| (\S+) \((\d+) of \d+ slab floats differ\)", out.stdout)
    print("k2 N=%d V=32 bf16=%d: %s; canon32 against generic: %s" % (n, bf16, "; ".join(
        "layer %s %.2e of %s" % (layer, float(diff), ref) for layer, diff, ref in rows), same))
    assert len(rows) == 5, out.stdout
    for layer, diff, ref in rows:
        assert float(ref) > 0 and float(diff) <= 1e-6 * float(ref), (layer, diff, ref)
    # the Canon32 kernel served the batch, and its slab is the generic kernel's bit for bit
    assert len(same) == 1, out.stdout
    assert float(same[0][0]) == 0.0 and int(same[0][1]) == 0, out.stdout
