"""CPU: the train / test commands' host side -- the train command's flags against the shipped checkpoints' args.pkl
(fixture fit_eth.npz, tests/golden/make_golden_fit.py), the restricted reader of a checkpoint's pickles, fit()'s
single-GPU guard."""
import argparse
import json
import pickle

import pytest
import torch

from conftest import load_golden

SPLITS = ("eth", "hotel", "univ", "zara1", "zara2")
# train.sh, one line per split (the reference's own command lines)
TRAIN_SH = "--lr 0.01 --n_stgcnn 1 --n_txpcnn 5  --dataset {0} --tag social-stgcnn-{0} --use_lrschd --num_epochs 250"


@pytest.mark.parametrize("name", SPLITS)
def test_train_command_parses_train_sh_into_the_shipped_args(name):
    from social_stgcnn_amd.train import REFERENCE_FIELDS, build_parser, reference_args
    shipped = json.loads(str(load_golden("fit_eth.npz")["shipped/%s/args" % name]))
    args = build_parser().parse_args(TRAIN_SH.format(name).split())
    ns = reference_args(args)
    assert list(vars(ns)) == list(shipped) == list(REFERENCE_FIELDS)
    assert {k: (type(v), v) for k, v in vars(ns).items()} == {k: (type(v), v) for k, v in shipped.items()}
    # the three flags of this command have their defaults and stay out of args.pkl
    assert (args.datasets, args.checkpoints, args.seed) == ("./datasets/", "./checkpoint/", 0)
    defaults = vars(reference_args(build_parser().parse_args([])))
    assert defaults["clip_grad"] is None and defaults["use_lrschd"] is False and defaults["lr_sh_rate"] == 150


def test_test_command_flags():
    from social_stgcnn_amd.test import build_parser
    a = build_parser().parse_args([])
    assert (a.checkpoints, a.datasets, a.ksteps, a.seed) == ("./checkpoint/*social-stgcnn*", "./datasets/", 20, 0)


def test_restricted_unpickler_reads_checkpoint_pickles(tmp_path):
    from social_stgcnn_amd.trainer import Checkpoint, load_pickle
    g = load_golden("fit_eth.npz")
    for name in SPLITS:
        ns = argparse.Namespace(**json.loads(str(g["shipped/%s/args" % name])))
        cm = json.loads(str(g["shipped/%s/constant_metrics" % name]))
        d = tmp_path / name
        d.mkdir()
        with open(d / "args.pkl", "wb") as fp:
            pickle.dump(ns, fp, protocol=3)                     # the shipped files' protocol
        with open(d / "constant_metrics.pkl", "wb") as fp:
            pickle.dump(cm, fp, protocol=3)
        assert load_pickle(str(d / "args.pkl")) == ns
        assert load_pickle(str(d / "constant_metrics.pkl")) == cm
        assert cm["min_val_loss"] < 0 and 0 <= cm["min_val_epoch"] < 250
    # what Checkpoint writes reads back the same way
    ck = Checkpoint(str(tmp_path / "ck") + "/", argparse.Namespace(dataset="eth", clip_grad=None, use_lrschd=True))
    ck.metrics = {"train_loss": [0.5, 0.25], "val_loss": [0.125, -0.5]}
    with open(ck.dir + "metrics.pkl", "wb") as fp:
        pickle.dump(ck.metrics, fp)
    assert load_pickle(ck.dir + "args.pkl") == argparse.Namespace(dataset="eth", clip_grad=None, use_lrschd=True)
    assert load_pickle(ck.dir + "metrics.pkl") == ck.metrics


def test_restricted_unpickler_refuses_other_globals_without_running_them(tmp_path):
    from social_stgcnn_amd.trainer import load_pickle
    marker = tmp_path / "ran"
    # protocol-0 text of "os.system('touch <marker>')": GLOBAL os system, MARK, STRING, TUPLE, REDUCE, STOP
    evil = tmp_path / "args.pkl"
    evil.write_bytes(b"cos\nsystem\n(S'touch " + str(marker).encode() + b"'\ntR.")
    with pytest.raises(pickle.UnpicklingError, match="os.system"):
        load_pickle(str(evil))
    assert not marker.exists()
    # the same through the protocol-2+ opcode (STACK_GLOBAL) and a global hidden inside a dict
    for obj in ({"min_val_loss": torch.Size([1])}, torch.Size):
        p = tmp_path / "x.pkl"
        p.write_bytes(pickle.dumps(obj, protocol=4))
        with pytest.raises(pickle.UnpicklingError):
            load_pickle(str(p))


def test_fit_refuses_a_multi_rank_world(monkeypatch):
    import torch.distributed as dist
    from social_stgcnn_amd.train import fit
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        fit(None, None, None, None)
