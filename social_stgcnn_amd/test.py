"""The reference's test.py (test.py:129-204) on the device: every checkpoint directory matching a glob, in sorted order,
evaluated with best-of-K ADE / FDE on its split's test set (predict.sample_test).

    python -m social_stgcnn_amd.test [--checkpoints './checkpoint/*social-stgcnn*'] [--datasets ./datasets/]
                                     [--ksteps 20] [--seed 0] [--metrics [--levels 0.5,0.9,0.99] [--kde_floor 20]]
                                     [--calibrate {val,train,DIR} [--calib_mode moment|coverage] [--calib_level P]
                                      [--save_calibration]]

The draws come from the device sampler (Philox, keyed by seed + batch index): statistically equal to the reference's
CPU draws, not bitwise.  args.pkl and constant_metrics.pkl are read with trainer.load_pickle (argparse.Namespace and
plain values only).

--metrics: after the ADE / FDE line of each checkpoint, the distribution metrics of its test set
(predict.distribution_test; the same draws): AMD, AMV, NLL, KDE-NLL, joint ADE / FDE and the coverage of
the ellipses at --levels; their averages at the end.  Without the flag the output is what it always was.

--calibrate PART: fit one factor per predicted step on the covariances of each checkpoint (calibrate.fit_calibration,
DESIGN.md 5.32) on <datasets>/<dataset>/val or /train, or on the recordings of the directory DIR -- never on the test
set it is then judged on --, print the factors, and behind the lines above the same lines for the calibrated model,
prefixed "Calibrated".  --calib_mode and --calib_level choose the rule (default coverage at 0.9); --save_calibration
writes <checkpoint>/calibration.npz, which `python -m social_stgcnn_amd.predict_frames --calibration` reads.
"""
import argparse
import glob
import os

import torch

from . import data
from .calibrate import fit_calibration
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
    p.add_argument("--calibrate", default=None, metavar="{val,train,DIR}",
                   help="fit per-step covariance factors on this part of each checkpoint's dataset (or on the recordings "
                        "in DIR) and evaluate the calibrated model as well")
    p.add_argument("--calib_mode", default="coverage", choices=("moment", "coverage"), help="the rule of the fit")
    p.add_argument("--calib_level", type=float, default=0.9, help="the probability level of the fit")
    p.add_argument("--save_calibration", action="store_true", help="write <checkpoint>/calibration.npz (--calibrate)")
    return p


METRIC_NAMES = ("AMD", "AMV", "NLL", "KDE-NLL", "JADE", "JFDE")


def evaluate(exp_path, datasets, ksteps=20, seed=0, device=None, levels=None, kde_floor=20.0, calibrate=None,
             calib_mode="coverage", calib_level=0.9):
    """one checkpoint directory -> (ade, fde, constant_metrics) as test.py:147-197 computes them; with `levels` also
    the metrics.DistSummary of its test set as a fourth value.  calibrate ("val", "train" or a directory of recordings):
    a last value (Calibration, CalibFit, windows fitted on, (ade, fde) and, with `levels`, the DistSummary of the
    calibrated model)"""
    args = load_pickle(os.path.join(exp_path, "args.pkl"))
    cm = load_pickle(os.path.join(exp_path, "constant_metrics.pkl"))
    model = social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                          seq_len=args.obs_seq_len, kernel_size=args.kernel_size, pred_seq_len=args.pred_seq_len)
    load_checkpoint(model, os.path.join(exp_path, "val_best.pth"))
    model.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    windows = data.load_windows(os.path.join(datasets, args.dataset, "test"), args.obs_seq_len, args.pred_seq_len, 1,
                                with_non_linear=False)
    ade_, fde_, _ = sample_test(model, windows, k=ksteps, seed=seed)
    res = (ade_, fde_, cm)
    if levels is not None:
        res += (distribution_test(model, windows, k=ksteps, seed=seed, levels=levels, kde_floor=kde_floor)[0],)
    if calibrate is None:
        return res
    part = os.path.join(datasets, args.dataset, calibrate) if calibrate in ("val", "train") else calibrate
    held_out = data.load_windows(part, args.obs_seq_len, args.pred_seq_len, 1, with_non_linear=False)
    cal, fit = fit_calibration(model, held_out, calib_mode, calib_level)
    c_ade, c_fde, _ = sample_test(model, windows, k=ksteps, seed=seed, calibration=cal)
    c_res = (c_ade, c_fde)
    if levels is not None:
        c_res += (distribution_test(model, windows, k=ksteps, seed=seed, levels=levels, kde_floor=kde_floor,
                                    calibration=cal)[0],)
    return res + ((cal, fit, held_out, c_res),)


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
    if a.calibrate is None and a.save_calibration:
        raise SystemExit("--save_calibration needs --calibrate {val,train,DIR}")
    ade_ls, fde_ls, dist_ls, cal_ls = [], [], [], []
    for exp_path in exps:
        print("*" * 50)
        print("Evaluating model:", exp_path)
        ade_, fde_, cm, *dist = evaluate(exp_path, a.datasets, a.ksteps, a.seed, levels=levels, kde_floor=a.kde_floor,
                                         calibrate=a.calibrate, calib_mode=a.calib_mode, calib_level=a.calib_level)
        calibrated = dist.pop() if a.calibrate is not None else None
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
        if calibrated is not None:
            cal, fit, held_out, (c_ade, c_fde, *c_dist) = calibrated
            flags = fit.flags.cpu().numpy()
            print("Calibration: %s at %g on %d windows, %d pedestrians of %s"
                  % (cal.mode, cal.level, len(held_out), int(held_out.num_peds.sum()), a.calibrate))
            print("g:", " ".join("%.4g" % x for x in cal.g))
            if flags.any():
                print("flags (1 low clamp, 2 high clamp, 4 no element):", " ".join(str(x) for x in flags))
            print("Calibrated ADE:", c_ade, " FDE:", c_fde)
            row = (c_ade, c_fde)
            if c_dist:
                s = c_dist[0]
                row += (s.amd, s.amv, s.nll, s.kde_nll, s.jade, s.jfde) + tuple(s.coverage)
                print("Calibrated", " ".join("%s: %s " % (n, x) for n, x in zip(METRIC_NAMES, row[2:])).rstrip())
                print("Calibrated Coverage:", " ".join("%g: %s " % (p, c) for p, c in zip(s.levels, s.coverage)).rstrip())
            cal_ls.append(row)
            if a.save_calibration:
                cal.save(os.path.join(exp_path, "calibration.npz"))
                print("Calibration written to", os.path.join(exp_path, "calibration.npz"))
    print("*" * 50)
    print("Avg ADE:", sum(ade_ls) / len(ade_ls))
    print("Avg FDE:", sum(fde_ls) / len(fde_ls))
    if dist_ls:
        avg = [sum(col) / len(col) for col in zip(*dist_ls)]
        for n, x in zip(METRIC_NAMES, avg):
            print("Avg %s:" % n, x)
        print("Avg Coverage:", " ".join("%g: %s " % (p, c) for p, c in zip(levels, avg[len(METRIC_NAMES):])).rstrip())
    if cal_ls:
        avg = [sum(col) / len(col) for col in zip(*cal_ls)]
        for n, x in zip(("ADE", "FDE") + METRIC_NAMES, avg):
            print("Avg Calibrated %s:" % n, x)
        if levels is not None:
            print("Avg Calibrated Coverage:",
                  " ".join("%g: %s " % (p, c) for p, c in zip(levels, avg[2 + len(METRIC_NAMES):])).rstrip())


if __name__ == "__main__":
    main()
