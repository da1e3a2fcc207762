"""The reference's training workflow on the device: `fit` is the epoch loop of train.py:213-246 over device-resident
datasets (dataset.EpochRunner), `main` the command line of train.py:124-246 (what train.sh runs once per split).

    python -m social_stgcnn_amd.train --lr 0.01 --n_stgcnn 1 --n_txpcnn 5 --dataset eth --tag social-stgcnn-eth \\
        --use_lrschd --num_epochs 250 [--datasets ./datasets/] [--checkpoints ./checkpoint/] [--seed 0]

reads <datasets>/<dataset>/{train,val}/ and writes <checkpoints>/<tag>/{args.pkl, val_best.pth, metrics.pkl,
constant_metrics.pkl} in the reference's layout, so its test.py (or `python -m social_stgcnn_amd.test`) reads them.
"""
import argparse
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import data
from .dataset import DeviceWindows, EpochRunner
from .model import social_stgcnn
from .trainer import Checkpoint, Trainer

# the fields of the reference's args.pkl, in train.py:128-154's order
REFERENCE_FIELDS = ("input_size", "output_size", "n_stgcnn", "n_txpcnn", "kernel_size", "obs_seq_len", "pred_seq_len",
                    "dataset", "batch_size", "num_epochs", "clip_grad", "lr", "lr_sh_rate", "use_lrschd", "tag")


def _device_order(order, ds):
    """an epoch order as the contiguous int32 device tensor EpochRunner reads (a host array costs one copy)"""
    if torch.is_tensor(order) and order.device == ds.device and order.dtype == torch.int32 and order.is_contiguous():
        return order
    return torch.as_tensor(np.asarray(order.cpu() if torch.is_tensor(order) else order),
                           dtype=torch.int32).contiguous().to(ds.device)


def fit(model, train_ds, val_ds, checkpoint, batch_size=128, num_epochs=250, lr=0.01, clip_grad=None,
        lr_sh_rate=None, orders=None, generator=None, log=None):
    """train.py:213-246 on one GPU.  Every epoch e, in this order:
        order = orders(e), or train_ds.shuffled_order(generator) (DataLoader(shuffle=True))
        train loss = train_runner.train_epoch(order)      captured group steps (train.py:28-79)
        val loss   = val_runner.val_epoch()              captured eval groups in dataset order (train.py:81-122)
        trainer.scheduler_step()                         when lr_sh_rate is set: StepLR(lr_sh_rate, 0.2)
        checkpoint.record(e, model, train loss, val loss)  val_best.pth / metrics.pkl / constant_metrics.pkl
    model: social_stgcnn on the GPU; train_ds / val_ds: dataset.DeviceWindows (each gets its own EpochRunner, so the
    validation set is padded to its own largest crowd); checkpoint: trainer.Checkpoint.  The two losses are read back
    once per epoch (the only host synchronisations; after the first epoch, which captures the graphs, and besides the
    state copy of an improved model).  `log(line)` receives one line per epoch.
    Returns (checkpoint.metrics, checkpoint.constant_metrics)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("fit() trains on one GPU; drive Trainer / EpochRunner per rank for data parallelism")
    trainer = Trainer(model, lr=lr, clip_grad=clip_grad, lr_sh_rate=lr_sh_rate)
    train_runner = EpochRunner(trainer, train_ds, batch_size)
    val_runner = EpochRunner(trainer, val_ds, batch_size)
    for epoch in range(int(num_epochs)):
        order = _device_order(orders(epoch), train_ds) if orders is not None else train_ds.shuffled_order(generator)
        train_loss = float(train_runner.train_epoch(order))
        val_loss = float(val_runner.val_epoch())
        if lr_sh_rate:
            trainer.scheduler_step()
        checkpoint.record(epoch, model, train_loss, val_loss)
        if log is not None:
            cm = checkpoint.constant_metrics
            log("epoch %d  train_loss %.9g  val_loss %.9g  min_val_loss %.9g (epoch %d)"
                % (epoch, train_loss, val_loss, cm["min_val_loss"], cm["min_val_epoch"]))
    return checkpoint.metrics, checkpoint.constant_metrics


def fine_tune(model, ds, epochs, batch_size=128, lr=0.01, clip_grad=None, generator=None, orders=None):
    """fit's training half alone, for windows that are on the device already (frames.LiveWindows.snapshot(), or any
    dataset.DeviceWindows): a Trainer and an EpochRunner over `ds`, `epochs` times
        order = orders(e), or ds.shuffled_order(generator)
        loss  = runner.train_epoch(order)                 captured group steps (train.py:28-79)
    with no validation set, no scheduler and no checkpoint files.  Returns the per-epoch train losses, each read back
    once (the only host synchronisations besides the first epoch's captures).  The model is left in training mode, as
    fit leaves it; a live predictor switches to eval mode for its own pushes."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("fine_tune() trains on one GPU; drive Trainer / EpochRunner per rank for data "
                                  "parallelism")
    if isinstance(epochs, bool) or int(epochs) != epochs or int(epochs) < 0:
        raise ValueError("fine_tune: epochs must be an integer >= 0, got %r" % (epochs,))
    trainer = Trainer(model, lr=lr, clip_grad=clip_grad)
    runner = EpochRunner(trainer, ds, batch_size)
    losses = []
    for epoch in range(int(epochs)):
        order = _device_order(orders(epoch), ds) if orders is not None else ds.shuffled_order(generator)
        losses.append(float(runner.train_epoch(order)))
    return losses


def build_parser():
    """train.py:125-154's 15 flags (same names, types, defaults) + --datasets, --checkpoints, --seed"""
    p = argparse.ArgumentParser(description="Train Social-STGCNN on one ETH/UCY split (train.py on the device).")
    p.add_argument("--input_size", type=int, default=2)
    p.add_argument("--output_size", type=int, default=5)
    p.add_argument("--n_stgcnn", type=int, default=1, help="st_gcn blocks")
    p.add_argument("--n_txpcnn", type=int, default=5, help="TXP-CNN layers")
    p.add_argument("--kernel_size", type=int, default=3)
    p.add_argument("--obs_seq_len", type=int, default=8)
    p.add_argument("--pred_seq_len", type=int, default=12)
    p.add_argument("--dataset", default="eth", help="eth, hotel, univ, zara1 or zara2")
    p.add_argument("--batch_size", type=int, default=128, help="scenes per optimizer step")
    p.add_argument("--num_epochs", type=int, default=250)
    p.add_argument("--clip_grad", type=float, default=None, help="gradient-norm clipping (off by default)")
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--lr_sh_rate", type=int, default=150, help="StepLR step size in epochs")
    p.add_argument("--use_lrschd", action="store_true", default=False, help="use the StepLR schedule")
    p.add_argument("--tag", default="tag", help="checkpoint directory name")
    p.add_argument("--datasets", default="./datasets/", help="directory holding <dataset>/{train,val,test}/")
    p.add_argument("--checkpoints", default="./checkpoint/", help="directory receiving <tag>/")
    p.add_argument("--seed", type=int, default=0, help="initialisation and shuffling seed")
    return p


def reference_args(args):
    """the Namespace the reference's train.py would pickle: its 15 fields only"""
    return argparse.Namespace(**{k: getattr(args, k) for k in REFERENCE_FIELDS})


def main(argv=None):
    args = build_parser().parse_args(argv)
    ref_args = reference_args(args)
    print(ref_args)
    if not torch.cuda.is_available():
        raise RuntimeError("social_stgcnn_amd.train needs a GPU (MI355X)")
    dev = torch.device("cuda", torch.cuda.current_device())
    root = os.path.join(args.datasets, args.dataset)
    windows = [data.load_windows(os.path.join(root, part), args.obs_seq_len, args.pred_seq_len, 1,
                                 with_non_linear=False) for part in ("train", "val")]
    train_ds, val_ds = (DeviceWindows(w, dev, obs_len=args.obs_seq_len) for w in windows)
    torch.manual_seed(args.seed)
    model = social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                          seq_len=args.obs_seq_len, kernel_size=args.kernel_size, pred_seq_len=args.pred_seq_len)
    model = model.to(dev)                    # initialised on the CPU, as the reference initialises it
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    ck = Checkpoint(os.path.join(args.checkpoints, args.tag) + "/", ref_args)
    print("train: %d windows, val: %d windows; checkpoint dir: %s" % (len(train_ds), len(val_ds), ck.dir))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, cm = fit(model, train_ds, val_ds, ck, batch_size=args.batch_size, num_epochs=args.num_epochs, lr=args.lr,
                clip_grad=args.clip_grad, lr_sh_rate=args.lr_sh_rate if args.use_lrschd else None, generator=gen,
                log=lambda line: print(line, flush=True))
    torch.cuda.synchronize()
    print("best: %s" % cm)
    print("Training time: %.3f s (%d epochs)" % (time.perf_counter() - t0, args.num_epochs))


if __name__ == "__main__":
    main()
