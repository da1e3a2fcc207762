"""The reference's test.py (test.py:129-204) on the device: every checkpoint directory matching a glob, in sorted order,
evaluated with best-of-K ADE / FDE on its split's test set (predict.sample_test).

    python -m social_stgcnn_amd.test [--checkpoints './checkpoint/*social-stgcnn*'] [--datasets ./datasets/]
                                     [--ksteps 20] [--seed 0] [--metrics [--levels 0.5,0.9,0.99] [--kde_floor 20]]

The draws come from the device sampler (Philox, keyed by seed + batch index): statistically equal to the reference's
CPU draws, not bitwise.  args.pkl and constant_metrics.pkl are read with trainer.load_pickle (argparse.Namespace and
plain values only).

--metrics: after the ADE / FDE line of each checkpoint, the distribution metrics of its test set
(predict.distribution_test; the same draws): AMD, AMV, NLL, KDE-NLL, joint ADE / FDE and the coverage of
the ellipses at --levels; their averages at the end.  Without the flag the output is what it always was.
"""
import argparse
import glob
import os

import torch

from . import data
from .model import social_stgcnn
from .predict import distribution_test, sample_test
from .trainer import load_checkpoint, load_pickle


def build_parser():
    p = argparse.ArgumentParser(description="Best-of-K ADE / FDE of trained checkpoints (test.py on the device).")
    p.add_argument("--checkpoints", default="./checkpoint/*social-stgcnn*", help="glob of checkpoint directories")
    p.add_argument("--datasets", default="./datasets/", help="directory holding <dataset>/test/")
    p.add_argument("--ksteps", type=int, default=20, help="samples per pedestrian")
    p.add_argument("--seed", type=int, default=0, help="seed of the device sampler")
    p.add_argument("--metrics", action="store_true", help="also print the distribution metrics of each test set")
    p.add_argument("--levels", default="0.5,0.9,0.99", help="probability levels of the coverage figures (--metrics)")
    p.add_argument("--kde_floor", type=float, default=20.0, help="KDE-NLL is clipped from above here (--metrics)")
    return p


METRIC_NAMES = ("AMD", "AMV", "NLL", "KDE-NLL", "JADE", "JFDE")


def evaluate(exp_path, datasets, ksteps=20, seed=0, device=None, levels=None, kde_floor=20.0):
    """one checkpoint directory -> (ade, fde, constant_metrics) as test.py:147-197 computes them; with `levels` also
    the metrics.DistSummary of its test set as a fourth value"""
    args = load_pickle(os.path.join(exp_path, "args.pkl"))
    cm = load_pickle(os.path.join(exp_path, "constant_metrics.pkl"))
    model = social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                          seq_len=args.obs_seq_len, kernel_size=args.kernel_size, pred_seq_len=args.pred_seq_len)
    load_checkpoint(model, os.path.join(exp_path, "val_best.pth"))
    model.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    windows = data.load_windows(os.path.join(datasets, args.dataset, "test"), args.obs_seq_len, args.pred_seq_len, 1,
                                with_non_linear=False)
    ade_, fde_, _ = sample_test(model, windows, k=ksteps, seed=seed)
    if levels is None:
        return ade_, fde_, cm
    return ade_, fde_, cm, distribution_test(model, windows, k=ksteps, seed=seed, levels=levels, kde_floor=kde_floor)[0]


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
    levels = tuple(float(x) for x in a.levels.split(",")) if a.metrics else None
    ade_ls, fde_ls, dist_ls = [], [], []
    for exp_path in exps:
        print("*" * 50)
        print("Evaluating model:", exp_path)
        ade_, fde_, cm, *dist = evaluate(exp_path, a.datasets, a.ksteps, a.seed, levels=levels, kde_floor=a.kde_floor)
        print("Stats:", cm)
        ade_ls.append(ade_)
        fde_ls.append(fde_)
        print("ADE:", ade_, " FDE:", fde_)
        if dist:
            s = dist[0]
            row = (s.amd, s.amv, s.nll, s.kde_nll, s.jade, s.jfde)
            dist_ls.append(row + tuple(s.coverage))
            print(" ".join("%s: %s " % (n, x) for n, x in zip(METRIC_NAMES, row)).rstrip())
            print("Coverage:", " ".join("%g: %s " % (p, c) for p, c in zip(s.levels, s.coverage)).rstrip())
    print("*" * 50)
    print("Avg ADE:", sum(ade_ls) / len(ade_ls))
    print("Avg FDE:", sum(fde_ls) / len(fde_ls))
    if dist_ls:
        avg = [sum(col) / len(col) for col in zip(*dist_ls)]
        for n, x in zip(METRIC_NAMES, avg):
            print("Avg %s:" % n, x)
        print("Avg Coverage:", " ".join("%g: %s " % (p, c) for p, c in zip(levels, avg[len(METRIC_NAMES):])).rstrip())


if __name__ == "__main__":
    main()
