#!/usr/bin/env python3
"""Golden fixture `fit_eth.npz`: the REFERENCE's own train() / vald() (train.py:28-122) driven through three shuffled
epochs the way train.py:213-246 drives them, on the real eth split: datasets/eth/train (2,785 windows) and
datasets/eth/val (660), batch 128, SGD lr 0.01, StepLR(2, 0.2), no clipping, model from torch.manual_seed(0).
Epoch e trains on the windows in the order torch.randperm(n, generator=torch.Generator().manual_seed(1000 + e)) -- the
permutations are stored, so the device loop replays the same epochs; validation runs in dataset order.

Also stored, as plain values (JSON text): the 15 args.pkl fields and constant_metrics of the five shipped checkpoints.

Run in the build container only (the one place /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fit.py
Nothing of the reference is copied: the outputs are numbers.  The reference's seconds per epoch on one CPU thread are
printed (not stored: the fixture regenerates bit-identically)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as G                     # sets up sys.path for /root/reference, shared helpers
import train as ref_train                   # /root/reference/train.py
import utils as ref_utils                   # /root/reference/utils.py

from social_stgcnn_amd.trainer import load_pickle

SPLITS = ("eth", "hotel", "univ", "zara1", "zara2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    out_dir = ap.parse_args().out
    out = {}
    dirs = {part: os.path.join(G.REF, "datasets", "eth", part) for part in ("train", "val")}
    sets = {}
    for part, d in dirs.items():
        t0 = time.time()
        out["listdir_" + part] = np.asarray(os.listdir(d))            # the order the reference walks (utils.py:116-117)
        sets[part] = ref_utils.TrajectoryDataset(d + "/", obs_len=8, pred_len=12, skip=1, norm_lap_matr=True)
        out["num_peds_" + part] = np.asarray([e - s for s, e in sets[part].seq_start_end], dtype=np.int32)
        print("eth/%s: %d windows (%.0f s)" % (part, len(sets[part]), time.time() - t0), flush=True)
    train_b = [[t.unsqueeze(0) for t in sets["train"][i]] for i in range(len(sets["train"]))]
    val_b = [[t.unsqueeze(0) for t in sets["val"][i]] for i in range(len(sets["val"]))]
    n, bs, lr, epochs, sh_rate = len(train_b), 128, 0.01, 3, 2
    m = G.new_ref_model(seed=0)
    before = G.sd_to_np(m.state_dict())
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=sh_rate, gamma=0.2)
    targs = argparse.Namespace(batch_size=bs, clip_grad=None)
    tl, vl, perms, secs = [], [], [], []
    best, min_val, min_epoch = None, 9999999999999999, -1
    for ep in range(epochs):
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1000 + ep))
        perms.append(perm.numpy().astype(np.int16))
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            tl.append(ref_train.train(ep, m, [train_b[i] for i in perm.tolist()], opt, targs, torch.device("cpu")))
            secs.append(time.time() - t0)
            vl.append(ref_train.vald(ep, m, val_b, targs, torch.device("cpu")))
        sched.step()
        if vl[-1] < min_val:                                          # train.py:228-231
            min_val, min_epoch, best = vl[-1], ep, G.sd_to_np(m.state_dict())
    out.update({"train_loss": np.asarray(tl, np.float64), "val_loss": np.asarray(vl, np.float64),
                "perms": np.stack(perms), "batch_size": np.int64(bs), "lr": np.float64(lr), "epochs": np.int64(epochs),
                "lr_sh_rate": np.int64(sh_rate), "min_val_epoch": np.int64(min_epoch),
                "min_val_loss": np.float64(min_val)})
    for k, v in before.items():
        out["before/" + k] = v
    for k, v in G.sd_to_np(m.state_dict()).items():
        out["after/" + k] = v
    for k, v in best.items():
        out["best/" + k] = v
    for name in SPLITS:
        d = os.path.join(G.REF, "checkpoint", "social-stgcnn-" + name)
        out["shipped/%s/args" % name] = np.asarray(json.dumps(vars(load_pickle(os.path.join(d, "args.pkl")))))
        out["shipped/%s/constant_metrics" % name] = np.asarray(
            json.dumps(load_pickle(os.path.join(d, "constant_metrics.pkl"))))
    np.savez(os.path.join(out_dir, "fit_eth.npz"), **out)
    print("train", tl)
    print("val  ", vl)
    print("min_val_epoch", min_epoch)
    print("reference train() seconds per epoch (one CPU thread, %d windows): %s" % (n, ["%.1f" % s for s in secs]))


if __name__ == "__main__":
    main()
