"""GPU (-m gpu): the reference's training workflow (train.py, train.sh, test.py) end to end on the device --
EpochRunner.val_epoch against the host-batched Trainer.val_epoch, fit() against the reference's own shuffled epochs on
eth (fixture fit_eth.npz, tests/golden/make_golden_fit.py), train.sh's five splits trained for 250 epochs against the
shipped models, and the train / test commands as fresh processes."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_oracle_splits import _split_directory

pytestmark = pytest.mark.gpu
CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
SPLITS = ("eth", "hotel", "univ", "zara1", "zara2")


def _state(npz, prefix=""):
    return {k[len(prefix):]: torch.from_numpy(np.array(npz[k])) for k in npz.files if k.startswith(prefix)}


def _model(state, dev):
    from social_stgcnn_amd.model import social_stgcnn
    m = social_stgcnn(**CFG)
    m.load_state_dict(state)
    return m.to(dev)


def _eth_windows(tmp_path, part, g):
    """eth/<part> rebuilt from the committed recordings, files in the order the reference listed them"""
    from social_stgcnn_amd import data
    (tmp_path / "eth").mkdir(exist_ok=True)
    w = data.load_windows(_split_directory(tmp_path, "eth", part), 8, 12, 1, with_non_linear=False,
                          files=[str(f) for f in g["listdir_" + part]])
    assert np.array_equal(w.num_peds, g["num_peds_" + part]), part
    return w


def _update_error(state, g, prefix):
    """|update - reference update| / |reference update| over all parameters and running statistics (updates from
    before/, 2-norms in float64); num_batches_tracked must be exact"""
    before, num, den = _state(g, "before/"), 0.0, 0.0
    for k, val in state.items():
        ref = g[prefix + k]
        if "num_batches" in k:
            assert int(val) == int(ref), k
            continue
        upd_ref = ref.astype(np.float64) - before[k].double().numpy()
        upd = val.cpu().double().numpy() - before[k].double().numpy()
        num += float(((upd - upd_ref) ** 2).sum())
        den += float((upd_ref ** 2).sum())
    err = (num / den) ** 0.5
    print("%s relative update error %.2e" % (prefix, err))
    return err


@pytest.mark.parametrize("bs", [128, 97])
def test_device_validation_epoch_equals_the_host_batched_one(tmp_path, bs):
    """vald() over eth/val (660 windows, up to 42 pedestrians; 128 and 97 leave short closing groups of 20 and 78):
    EpochRunner.val_epoch (captured groups, padded to the set's own crowd) == Trainer.val_epoch over host-collated
    batches of the same windows (pinned to the reference by test_six_epochs_follow_the_reference_training_curve)."""
    from social_stgcnn_amd import data, ops
    from social_stgcnn_amd.dataset import DeviceWindows, EpochRunner
    from social_stgcnn_amd.trainer import Trainer
    g = load_golden("fit_eth.npz")
    win = _eth_windows(tmp_path, "val", g)
    assert len(win) == 660 and int(win.num_peds.max()) == 42
    dev = torch.device("cuda", 0)
    m = _model(_state(g, "before/"), dev)
    tr = Trainer(m)
    runner = EpochRunner(tr, DeviceWindows(win, dev), bs)
    idx = np.arange(len(win)) if bs == 128 else np.random.default_rng(bs).permutation(len(win))
    order = None if bs == 128 else torch.from_numpy(idx.astype(np.int32)).to(dev)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    got = runner.val_epoch(order)
    assert got.dim() == 0 and got.is_cuda and not m.training

    def batcher(lo, hi):
        obs_rel, pred_rel, _, _, counts = data.pad_batch(win, idx[lo:hi])
        peds = torch.from_numpy(counts).to(dev)
        nodes, adj = ops.adj_build(torch.from_numpy(obs_rel).to(dev).permute(0, 2, 3, 1), peds)
        return nodes.permute(0, 3, 1, 2), adj, torch.from_numpy(pred_rel).to(dev), peds
    want = tr.val_epoch(batcher, len(win), bs)
    got = float(got)
    print("val epoch bs %d: device %.9g host %.9g" % (bs, got, want))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert float(runner.val_epoch(order)) == got                 # replays of the same graphs
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                     # eval mode: nothing moves


def test_fit_follows_the_reference_shuffled_epochs(tmp_path):
    """fit() on eth (2,785 train / 660 val windows) with the reference's own epoch permutations: 3 epochs x 22 optimizer
    steps at batch 128, lr 0.01, StepLR(2, 0.2), against the reference's train() / vald() (fit_eth.npz)."""
    from social_stgcnn_amd.dataset import DeviceWindows
    from social_stgcnn_amd.train import fit
    from social_stgcnn_amd.trainer import Checkpoint, load_pickle
    g = load_golden("fit_eth.npz")
    tw, vw = _eth_windows(tmp_path, "train", g), _eth_windows(tmp_path, "val", g)
    dev = torch.device("cuda", 0)
    m = _model(_state(g, "before/"), dev)
    perms = torch.from_numpy(g["perms"].astype(np.int32)).to(dev)
    epochs = int(g["epochs"])
    ck = Checkpoint(str(tmp_path / "checkpoint" / "social-stgcnn-eth") + "/")
    metrics, cm = fit(m, DeviceWindows(tw, dev), DeviceWindows(vw, dev), ck, batch_size=int(g["batch_size"]),
                      num_epochs=epochs, lr=float(g["lr"]), clip_grad=None, lr_sh_rate=int(g["lr_sh_rate"]),
                      orders=lambda e: perms[e].contiguous())
    for ep in range(epochs):
        for key in ("train_loss", "val_loss"):
            ref = float(g[key][ep])
            print("epoch %d %s: %.9g reference %.9g (%.2e)" % (ep, key, metrics[key][ep], ref, metrics[key][ep] - ref))
    # epoch 0 (22 steps from the same weights): the loss bar of test_six_epochs_follow_the_reference_training_curve
    assert abs(metrics["train_loss"][0] - float(g["train_loss"][0])) < 5e-6
    assert abs(metrics["val_loss"][0] - float(g["val_loss"][0])) < 5e-6
    # epochs 1 and 2: without clipping this trajectory amplifies rounding (one float32 ulp on the initial
    # weights, or the fp32-MFMA kernels, moves these losses by up to 6.9e-5 and the final weights by 5.6-6.4e-4 of the
    # update's norm, as far as they are from the reference); the bars are ~3x the device's own measured gap to it
    for ep in range(1, epochs):
        assert abs(metrics["train_loss"][ep] - float(g["train_loss"][ep])) < 2.5e-4, ep
        assert abs(metrics["val_loss"][ep] - float(g["val_loss"][ep])) < 2.5e-4, ep
    final = m.state_dict()
    assert _update_error(final, g, "after/") < 3e-3
    for k, val in final.items():
        if "num_batches" in k:
            assert int(val) == int(g["after/" + k]) == epochs * len(tw), k
    assert load_pickle(ck.dir + "metrics.pkl") == metrics == {"train_loss": metrics["train_loss"],
                                                              "val_loss": metrics["val_loss"]}
    assert all(len(v) == epochs for v in metrics.values())
    assert cm == load_pickle(ck.dir + "constant_metrics.pkl")
    assert cm["min_val_epoch"] == int(g["min_val_epoch"]) and cm["min_val_loss"] == min(metrics["val_loss"])
    best = torch.load(ck.dir + "val_best.pth", weights_only=True)
    assert _update_error(best, g, "best/") < 3e-3


def test_train_sh_quality_on_the_five_splits(tmp_path):
    """train.sh: each split trained for 250 epochs at batch 128, lr 0.01, StepLR(150, 0.2), no clipping, seed 0, its best-
    validation checkpoint against the shipped model of that split under the same device sampler (K = 20, seed 0)."""
    from social_stgcnn_amd import data
    from social_stgcnn_amd.dataset import DeviceWindows
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import sample_test
    from social_stgcnn_amd.train import fit
    from social_stgcnn_amd.trainer import Checkpoint, load_checkpoint
    dev = torch.device("cuda", 0)
    rows = {}
    t_all = time.perf_counter()
    for name in SPLITS:
        tw, vw, sw = (data.load_windows(_split_directory(tmp_path, name, part), 8, 12, 1, with_non_linear=False)
                      for part in ("train", "val", "test"))
        torch.manual_seed(0)
        m = social_stgcnn(**CFG).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        ck = Checkpoint(str(tmp_path / "checkpoint" / ("social-stgcnn-" + name)) + "/")
        train_ds, val_ds = DeviceWindows(tw, dev), DeviceWindows(vw, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, cm = fit(m, train_ds, val_ds, ck, batch_size=128, num_epochs=250, lr=0.01, clip_grad=None, lr_sh_rate=150,
                    generator=gen)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        trained = load_checkpoint(social_stgcnn(**CFG), ck.dir + "val_best.pth").to(dev)
        ade, fde, _ = sample_test(trained, sw, k=20, seed=0)
        s_ade, s_fde, _ = sample_test(_model(_state(load_golden("weights_%s.npz" % name)), dev), sw, k=20, seed=0)
        rows[name] = (cm["min_val_loss"], cm["min_val_epoch"], ade, fde, s_ade, s_fde, secs)
    print("\nsplit   min_val_loss  epoch   ADE     FDE    shipped ADE  FDE    train s")
    for name, r in rows.items():
        print("%-6s  %11.6f  %5d  %6.4f  %6.4f   %6.4f  %6.4f  %6.2f" % ((name,) + r))
    mean = np.mean([r[2:6] for r in rows.values()], axis=0)
    print("mean                        %6.4f  %6.4f   %6.4f  %6.4f  (whole test %.1f s)"
          % (tuple(mean) + (time.perf_counter() - t_all,)))
    for name, (vl, _, ade, fde, s_ade, s_fde, _) in rows.items():
        assert vl < 0, (name, vl)
        assert ade <= 1.30 * s_ade and fde <= 1.30 * s_fde, (name, ade, s_ade, fde, s_fde)
    assert mean[0] <= 1.10 * mean[2] and mean[1] <= 1.10 * mean[3], mean


@pytest.mark.auto_path
def test_train_and_test_commands_end_to_end(tmp_path):
    """`python -m social_stgcnn_amd.train` for 2 epochs on eth, then `python -m social_stgcnn_amd.test` on what it
    wrote, each a fresh process with its own time limit.  (auto_path: this process runs the library's default kernel
    choice, as the commands do.)"""
    from social_stgcnn_amd import data
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import sample_test
    from social_stgcnn_amd.train import REFERENCE_FIELDS
    from social_stgcnn_amd.trainer import load_checkpoint, load_pickle
    root = tmp_path / "datasets"
    for part in ("train", "val"):
        _split_directory(root, "eth", part)
    os.symlink(_split_directory(root, "eth", "test"), root / "eth" / "test")
    ckroot = tmp_path / "checkpoint"
    run = dict(cwd=ROOT, capture_output=True, text=True, timeout=600)
    r = subprocess.run([sys.executable, "-m", "social_stgcnn_amd.train", "--lr", "0.01", "--n_stgcnn", "1", "--n_txpcnn",
                        "5", "--dataset", "eth", "--tag", "social-stgcnn-eth", "--use_lrschd", "--num_epochs", "2",
                        "--datasets", str(root), "--checkpoints", str(ckroot)], **run)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    assert len(re.findall(r"^epoch \d+ ", r.stdout, re.M)) == 2 and "Training time:" in r.stdout
    d = ckroot / "social-stgcnn-eth"
    assert sorted(os.listdir(d)) == ["args.pkl", "constant_metrics.pkl", "metrics.pkl", "val_best.pth"]
    state = torch.load(str(d / "val_best.pth"), map_location="cpu", weights_only=True)
    assert len(state) == 40
    args = load_pickle(str(d / "args.pkl"))
    assert list(vars(args)) == list(REFERENCE_FIELDS)
    assert (args.dataset, args.num_epochs, args.use_lrschd, args.tag) == ("eth", 2, True, "social-stgcnn-eth")
    metrics = load_pickle(str(d / "metrics.pkl"))
    assert sorted(metrics) == ["train_loss", "val_loss"] and all(len(v) == 2 for v in metrics.values())
    assert load_pickle(str(d / "constant_metrics.pkl"))["min_val_epoch"] in (0, 1)

    r = subprocess.run([sys.executable, "-m", "social_stgcnn_amd.test", "--checkpoints", str(ckroot / "*social-stgcnn*"),
                        "--datasets", str(root)], **run)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    found = re.findall(r"^ADE: (\S+)  FDE: (\S+)$", r.stdout, re.M)
    assert len(found) == 1
    dev = torch.device("cuda", 0)
    m = load_checkpoint(social_stgcnn(n_stgcnn=args.n_stgcnn, n_txpcnn=args.n_txpcnn, output_feat=args.output_size,
                                      seq_len=args.obs_seq_len, kernel_size=args.kernel_size,
                                      pred_seq_len=args.pred_seq_len), str(d / "val_best.pth")).to(dev)
    ade, fde, _ = sample_test(m, data.load_windows(str(root / "eth" / "test"), 8, 12, 1, with_non_linear=False), k=20,
                              seed=0)
    assert (float(found[0][0]), float(found[0][1])) == (ade, fde)
    assert re.search(r"^Avg ADE: (\S+)$", r.stdout, re.M).group(1) == found[0][0]
