"""The reference's test.py (test.py:129-204) on the device: every checkpoint directory matching a glob, in sorted order,
evaluated with best-of-K ADE / FDE on its split's test set (predict.sample_test).

    python -m social_stgcnn_amd.test [--checkpoints './checkpoint/*social-stgcnn*'] [--datasets ./datasets/]
                                     [--ksteps 20] [--seed 0]

The draws come from the device sampler (Philox, keyed by seed + batch index): statistically equal to the reference's
CPU draws, not bitwise.  args.pkl and constant_metrics.pkl are read with trainer.load_pickle (argparse.Namespace and
plain values only).
"""
import argparse
import glob
import os

import torch

from . import data
from .model import social_stgcnn
from .predict import sample_test
from .trainer import load_checkpoint, load_pickle


def build_parser():
    p = argparse.ArgumentParser(description="Best-of-K ADE / FDE of trained checkpoints (test.py on the device).")
    p.add_argument("--checkpoints", default="./checkpoint/*social-stgcnn*", help="glob of checkpoint directories")
    p.add_argument("--datasets", default="./datasets/", help="directory holding <dataset>/test/")
    p.add_argument("--ksteps", type=int, default=20, help="samples per pedestrian")
    p.add_argument("--seed", type=int, default=0, help="seed of the device sampler")
    return p


def evaluate(exp_path, datasets, ksteps=20, seed=0, device=None):
    """one checkpoint directory -> (ade, fde, constant_metrics) as test.py:147-197 computes them"""
    args = load_pickle(os.path.join(exp_path, "args.pkl"))
    cm = load_pickle(os.path.join(exp_path, "constant_metrics.pkl"))
    model = social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                          seq_len=args.obs_seq_len, kernel_size=args.kernel_size, pred_seq_len=args.pred_seq_len)
    load_checkpoint(model, os.path.join(exp_path, "val_best.pth"))
    model.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    windows = data.load_windows(os.path.join(datasets, args.dataset, "test"), args.obs_seq_len, args.pred_seq_len, 1,
                                with_non_linear=False)
    ade_, fde_, _ = sample_test(model, windows, k=ksteps, seed=seed)
    return ade_, fde_, cm


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("social_stgcnn_amd.test needs a GPU (MI355X)")
    exps = sorted(glob.glob(a.checkpoints))
    print("*" * 50)
    print("Number of samples:", a.ksteps)
    print("*" * 50)
    print("Model being tested are:", exps)
    if not exps:
        raise SystemExit("no checkpoint directory matches %s" % a.checkpoints)
    ade_ls, fde_ls = [], []
    for exp_path in exps:
        print("*" * 50)
        print("Evaluating model:", exp_path)
        ade_, fde_, cm = evaluate(exp_path, a.datasets, a.ksteps, a.seed)
        print("Stats:", cm)
        ade_ls.append(ade_)
        fde_ls.append(fde_)
        print("ADE:", ade_, " FDE:", fde_)
    print("*" * 50)
    print("Avg ADE:", sum(ade_ls) / len(ade_ls))
    print("Avg FDE:", sum(fde_ls) / len(fde_ls))


if __name__ == "__main__":
    main()
