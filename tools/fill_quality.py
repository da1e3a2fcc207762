#!/usr/bin/env python3
"""What a filled history costs in accuracy (frames.fill_tracks).  One JSON line per (split, pattern).

    python tools/fill_quality.py [--splits eth,hotel,univ,zara1,zara2] [--k 20] [--seed 0] [--batch 64]

Every window of a test split (tests/golden/data/<split>_test, the committed weights of that split) is predicted from
its full 8-frame history and from histories with frames taken away and filled by stg_fill_tracks, every pedestrian of
the window cut alike:

    h8 h6 h4 h3 h2   only the last h frames seen (h8: the full history), the others filled backwards
    gap34            frames 3 and 4 of the window missed (an interior gap of two)
    gap1-5           frames 1 .. 5 missed: five of the six interior frames, seen only at 0, 6 and 7

ade / fde: best of k sampled trajectories per pedestrian (the device sampler, seed + batch index), as test.py
reports them; mean_ade / mean_fde: of the zero-noise trajectory.  Means over all pedestrians of all windows.  Reads the
committed data and weights only.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

CFG = dict(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# pattern -> presence bits of every pedestrian: bit t = seen t frames ago (window step s is bit 7 - s)
PATTERNS = (("h8", 0xff), ("h6", 0x3f), ("h4", 0x0f), ("h3", 0x07), ("h2", 0x03), ("gap34", 0xff & ~0x18),
            ("gap1-5", 0x83))


def split_case(split, k, seed, batch, dev):
    from social_stgcnn_amd import data, frames
    from social_stgcnn_amd.model import social_stgcnn
    from social_stgcnn_amd.predict import Predictor
    w = np.load(os.path.join(GOLDEN, "weights_%s.npz" % split))
    model = social_stgcnn(**CFG)
    model.load_state_dict({key: torch.from_numpy(np.array(w[key])) for key in w.files})
    model = model.to(dev).eval()
    win = data.load_windows(os.path.join(GOLDEN, "data", "%s_test" % split), 8, 12, 1, with_non_linear=False)
    pred = Predictor(model, k)
    out = []
    for name, bits in PATTERNS:
        sums = np.zeros(4)
        n_ped = 0
        for b, lo in enumerate(range(0, len(win), batch)):
            se = win.seq_start_end[lo:lo + batch]
            counts = np.array([e - s for s, e in se], np.int32)
            n, v = len(se), int(counts.max())
            obs, trgt = np.zeros((n, 8, v, 2)), np.zeros((n, 12, v, 2))
            for j, (s0, e0) in enumerate(se):
                obs[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, :8], (2, 0, 1))
                trgt[j, :, :e0 - s0] = np.transpose(win.seq[s0:e0, :, 8:], (2, 0, 1))
            missed = [s for s in range(8) if not (bits >> (7 - s)) & 1]
            obs[:, missed] = 1e6                                   # a missed frame is never read
            peds = torch.from_numpy(counts).to(dev)
            filled = frames.fill_tracks(torch.from_numpy(obs).to(dev), np.full((n, v), bits, np.int32), peds)
            r = pred.predict(filled, peds, seed + b)
            real = np.arange(v)[None] < counts[:, None]
            t = torch.from_numpy(trgt).to(dev)
            err = (r.samples.double() - t[None]).norm(dim=4)                             # (K,N,12,V)
            m_err = (r.mean.double() - t).norm(dim=3)                                     # (N,12,V)
            sums += [float(err.mean(dim=2).min(dim=0).values.cpu().numpy()[real].sum()),
                     float(err[:, :, -1].min(dim=0).values.cpu().numpy()[real].sum()),
                     float(m_err.mean(dim=1).cpu().numpy()[real].sum()), float(m_err[:, -1].cpu().numpy()[real].sum())]
            n_ped += int(counts.sum())
        ade, fde, m_ade, m_fde = (sums / n_ped).tolist()
        out.append({"split": split, "pattern": name, "seen": bits, "windows": len(win), "pedestrians": n_ped, "k": k,
                    "ade": round(ade, 4), "fde": round(fde, 4), "mean_ade": round(m_ade, 4),
                    "mean_fde": round(m_fde, 4)})
        out[-1]["mean_ade_ratio"] = round(m_ade / out[0]["mean_ade"], 4)
        out[-1]["ade_ratio"] = round(ade / out[0]["ade"], 4)
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--splits", default="eth,hotel,univ,zara1,zara2")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fill_quality needs a GPU (MI355X)")
    dev = torch.device("cuda", 0)
    for split in a.splits.split(","):
        split_case(split, a.k, a.seed, a.batch, dev)


if __name__ == "__main__":
    main()
