#!/usr/bin/env python3
"""train.sh on the device for several seeds: every ETH/UCY split trained with fit() (250 epochs, batch 128, lr 0.01,
StepLR(150, 0.2), no clipping), its best-validation model evaluated with sample_test (K = 20, device sampler seed 0)
beside the shipped model of the split.  The split directories are rebuilt from the recordings under tests/golden (as
tests/test_oracle_splits.py does).  Prints one row per (seed, split) -- the DESIGN.md table -- and with --repeat trains
the first seed a second time and reports whether the two runs' losses and weights are bitwise equal.

    python tools/fit_splits.py --seeds 0 1 2 3 4 [--repeat] [--epochs 250]
"""
import argparse
import os
import pathlib
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from test_oracle_splits import _split_directory          # noqa: E402  (tests/ helper: split directories)

SPLITS = ("eth", "hotel", "univ", "zara1", "zara2")
CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)


def train_split(sets, seed, epochs, ckdir, dev):
    from social_stgcnn_amd.dataset import DeviceWindows
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.train import fit
    from social_stgcnn_amd.trainer import Checkpoint
    torch.manual_seed(seed)
    m = social_stgcnn(**CFG).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    ck = Checkpoint(ckdir + "/")
    train_ds, val_ds = DeviceWindows(sets[0], dev), DeviceWindows(sets[1], dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics, cm = fit(m, train_ds, val_ds, ck, batch_size=128, num_epochs=epochs, lr=0.01, clip_grad=None,
                      lr_sh_rate=150, generator=gen)
    torch.cuda.synchronize()
    return metrics, cm, time.perf_counter() - t0, ck.dir + "val_best.pth"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0])
    ap.add_argument("--epochs", type=int, default=250)
    ap.add_argument("--splits", nargs="+", default=list(SPLITS))
    ap.add_argument("--repeat", action="store_true")
    a = ap.parse_args()
    from social_stgcnn_amd import data
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import sample_test
    from social_stgcnn_amd.trainer import load_checkpoint
    dev = torch.device("cuda", 0)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="fit_splits_"))
    sets, shipped = {}, {}
    for name in a.splits:
        sets[name] = [data.load_windows(_split_directory(tmp, name, part), 8, 12, 1, with_non_linear=False)
                      for part in ("train", "val", "test")]
        w = np.load(os.path.join(ROOT, "tests", "golden", "weights_%s.npz" % name))
        m = social_stgcnn(**CFG)
        m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
        shipped[name] = sample_test(m.to(dev), sets[name][2], k=20, seed=0)[:2]
    print("seed  split   min_val_loss  epoch   ADE     FDE    shipped ADE  FDE    train s", flush=True)
    total = {}
    for seed in a.seeds:
        means = []
        for name in a.splits:
            _, cm, secs, path = train_split(sets[name], seed, a.epochs, str(tmp / ("s%d_%s" % (seed, name))), dev)
            ade, fde, _ = sample_test(load_checkpoint(social_stgcnn(**CFG), path).to(dev), sets[name][2], k=20, seed=0)
            means.append((ade, fde) + shipped[name])
            total[seed] = total.get(seed, 0.0) + secs
            print("%4d  %-6s  %11.6f  %5d  %6.4f  %6.4f   %6.4f  %6.4f  %6.2f" % (
                seed, name, cm["min_val_loss"], cm["min_val_epoch"], ade, fde, shipped[name][0], shipped[name][1],
                secs), flush=True)
        mm = np.mean(means, axis=0)
        print("%4d  mean                 %6.4f  %6.4f   %6.4f  %6.4f  %6.2f  (ADE %.3fx, FDE %.3fx shipped)" % (
            seed, mm[0], mm[1], mm[2], mm[3], total[seed], mm[0] / mm[2], mm[1] / mm[3]), flush=True)
    if a.repeat:
        seed, name = a.seeds[0], a.splits[0]
        runs = [train_split(sets[name], seed, a.epochs, str(tmp / ("rep%d_%s" % (i, name))), dev) for i in range(2)]
        same_loss = runs[0][0] == runs[1][0]
        sd = [torch.load(r[3], weights_only=True) for r in runs]
        same_w = all(torch.equal(sd[0][k], sd[1][k]) for k in sd[0])
        print("repeat seed %d %s: losses bitwise equal %s, val_best weights bitwise equal %s" % (
            seed, name, same_loss, same_w), flush=True)


if __name__ == "__main__":
    main()
