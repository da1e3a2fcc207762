"""The weight-gradient kernel (K2, csrc/txp_wgrad_bf16.hip) on its own: tools/micro/k2_bench (built by
__graft_entry__.build()) runs the library's kernel on synthetic saved arrays and prints its distance to an fp64 host sum per
layer.  Small batches matter here: with one round per workgroup the item loop's first iteration is all there is, and that is
where an instruction-hazard bug of the kernel's inline-assembly MFMAs once lived -- invisible at bench sizes
against a tolerance, obvious against fp64 at N = 1..40.  The bench sizes run too (K2_FP64=1: the host sum at any N): V = 64 x
2048, V = 128 x 4096 (four 32-column chunks per scene, 16 k work items) and the ragged V = 128 x 4096 batch on the SORTED
schedule -- order / key_start from the library's scene sort, compact chunk lists [chunk 0 of every scene | chunk 1 of those
with more than 32 | chunk 2 above 64 | chunk 3 above 96] -- as the model hands it to the kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "micro", "k2_bench")

pytestmark = pytest.mark.gpu


CASES = [(1, 32, 0, 0, 0), (3, 32, 1, 0, 0), (8, 32, 1, 0, 0), (8, 32, 1, 1, 0), (16, 32, 0, 1, 0), (40, 32, 1, 0, 0),
         (24, 64, 1, 0, 0), (24, 64, 1, 1, 0), (12, 128, 1, 0, 0), (64, 20, 1, 0, 0),
         # bench sizes (the fp64 host sum: ~10 s of host work at 4096 x 128) and the sorted schedule
         (40, 128, 1, 0, 1), (2048, 64, 0, 0, 0), (4096, 128, 0, 0, 0), (4096, 128, 1, 0, 1)]


@pytest.mark.parametrize("n,v,ragged,bf16,srt", CASES,
                         ids=["%d-%d-%d-%d" % c[:4] + ("-sorted" if c[4] else "") for c in CASES])
def test_weight_gradient_kernel_against_fp64_host_sum(n, v, ragged, bf16, srt):
    if not os.path.exists(BIN):
        pytest.fail("tools/micro/k2_bench is not built (__graft_entry__.build() builds it)")
    # K2_GARBAGE: nonzero values in the channels of a_0 that no layer reads; K2_FP64: the fp64 host sum at every N.
    # K2_GRID (bench sizes): data on a dyadic grid, every partial sum exact in fp32 -- with full-mantissa data the fp32
    # accumulators of a workgroup's ~10^4 MFMA steps drift by 1e-6 .. 3e-6 of max |dW| (measured at 2048 x 64 and
    # 4096 x 128), which is rounding; on the grid the bar stays 1e-6 and a lost or repeated work item shows at full size.
    env = dict(os.environ, K2_GARBAGE="1", K2_FP64="1", K2_GRID="1" if n > 64 else "0")
    out = subprocess.run([BIN, str(n), str(v), str(ragged), str(bf16), str(srt)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"layer (\d+): shipped vs fp64 host: max \|diff\| (\S+) of (\S+)", out.stdout)
    print("k2 N=%d V=%d ragged=%d bf16=%d sorted=%d: %s" % (n, v, ragged, bf16, srt, "; ".join(
        "layer %s %.2e of %s" % (layer, float(diff), ref) for layer, diff, ref in rows)))
    assert len(rows) == 5, out.stdout
    if srt:
        # the sorted schedule ran, with every chunk list of the padded V non-empty
        items = re.findall(r"sorted: items per chunk ((?:\d+ ?)+)", out.stdout)
        assert items, out.stdout
        items = [int(c) for c in items[0].split()]
        print("    sorted chunk lists:", items)
        assert len(items) == (v + 31) // 32 and min(items) > 0, items
    for layer, diff, ref in rows:
        assert float(diff) <= 1e-6 * max(float(ref), 1e-3), (layer, diff, ref)
    # the tree's kernel source compiled into the harness (both workgroup shapes) against the library's
    for rel in re.findall(r"vs shipped: max \|diff\| \S+ of max \|ref\| \S+  \(rel (\S+),", out.stdout):
        assert float(rel) <= 2e-6, out.stdout
