"""Diagnostic (STG_STAMPS=1, diagnostic library): when every wave of the exact-bf16 scene kernels takes up its scene and
when it is done with it -- the start skew and the end skew of a launch, for the forward and the backward scene kernels as
two launches and as one (stg_model_step).

For a launch with scenes s:  span = max(end) - min(start) = mean(start - min start) + mean(end - start) + mean(max end - end)
                                                             start skew              wave lifetime       end skew
The stamps are s_memrealtime ticks (one counter for the whole chip; s_memtime differs from XCD to XCD); the tick length is calibrated against the HIP-event interval of the same launch."""
import ctypes
import os
import sys

os.environ["STG_STAMPS"] = "1"
os.environ["STG_USE_DIAG_LIB"] = "1"        # stamps exist only in the diagnostic build (make -C csrc DIAG=1)
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from social_stgcnn_amd import ops
from social_stgcnn_amd.model import social_stgcnn
from social_stgcnn_amd.trainer import Trainer

dev = torch.device("cuda", 0)
n, v = int(os.environ.get("STAMPS_N", "2048")), int(os.environ.get("STAMPS_V", "32"))
reps = int(os.environ.get("STAMPS_REPS", "5"))
obs_rel, target = bench.synth_scenes(n, v, 1)
nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev))
x, tgt = nodes.permute(0, 3, 1, 2), torch.from_numpy(target).to(dev)
w = torch.full((n,), 1.0 / n, device=dev)


def stamps_of(buf, off):
    return buf[off: off + n * 32].cpu().numpy().view(np.uint64).reshape(n, 16).astype(np.int64)


def report(name, st, ms):
    start, end = st[:, 0], st[:, 8]
    t0, t1 = start.min(), end.max()
    span = float(t1 - t0)
    us = ms * 1e3 / span                      # microseconds per tick, from the event interval of the same launch
    print("%-22s event %.1f us, stamp span %d ticks (%.4f us/tick)" % (name, ms * 1e3, span, us))
    print("    start skew  mean %.1f  p50 %.1f  p90 %.1f  max %.1f us" % tuple(
        us * f for f in ((start - t0).mean(), np.percentile(start - t0, 50), np.percentile(start - t0, 90), (start - t0).max())))
    print("    lifetime    mean %.1f  p10 %.1f  p90 %.1f us" % tuple(
        us * f for f in ((end - start).mean(), np.percentile(end - start, 10), np.percentile(end - start, 90))))
    print("    end skew    mean %.1f  p50 %.1f  p90 %.1f  max %.1f us" % tuple(
        us * f for f in ((t1 - end).mean(), np.percentile(t1 - end, 50), np.percentile(t1 - end, 90), (t1 - end).max())))
    return us


for separate in (True, False):
    torch.manual_seed(0)
    m = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12).to(dev).train()
    m.options = ops.KernelOptions(separate_fb=separate)
    tr = Trainer(m, lr=0.01)
    # where the library carves the stamps out of its two scratch buffers (negative: this build writes none)
    desc = ctypes.byref(m._launch_args(adj)[0])
    off_f, off_b = ops.lib().stg_model_fwd_stamps_offset(desc, n, v), ops.lib().stg_model_bwd_stamps_offset(desc, n, v)
    assert off_f >= 0 and off_b >= 0, "no stamps: build the diagnostic library (make -C social_stgcnn_amd/csrc DIAG=1)"
    for _ in range(3):
        tr.step(x, adj, tgt, None, w)
    print("==== %s ====" % ("F and B as two launches" if separate else "F and B as one launch"))
    for rep in range(reps):
        m.timer = ops.KernelTimer()
        tr.step(x, adj, tgt, None, w)
        torch.cuda.synchronize()
        f_ms, b_ms = m.timer.kernel_ms("model_fwd"), m.timer.kernel_ms("model_bwd")
        m.timer = None
        sf = stamps_of(m._last_fwd_scratch, off_f)
        sb = stamps_of(m._last_bwd_scratch, off_b)
        print("-- repetition %d" % rep)
        if separate:
            report("F", sf, f_ms[1])
            report("B", sb, b_ms[0])
        else:
            both = sf.copy()
            both[:, 8] = sb[:, 8]
            us = report("F+B (one launch)", both, b_ms[0])
            print("    F part mean %.1f us, B part mean %.1f us; B's end skew is the launch's" % (
                us * (sf[:, 8] - sf[:, 0]).mean(), us * (sb[:, 8] - sb[:, 0]).mean()))
