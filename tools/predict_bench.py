#!/usr/bin/env python3
"""Device time of the captured Predictor (observed absolute tracks -> K sampled trajectories, ONE graph) and of the
sampling kernel alone, from device events around graph replays.  One JSON line per case.

    python tools/predict_bench.py [--iters 200] [--cases bench,eth,kernel,risk,bestofk,metrics,calib]

  bench   Predictor replay at N = 2048, V = 32 (every slot a pedestrian), K = 20, eth weights
  eth     Predictor replay on eth/test: its 70 windows as one ragged batch, K = 20
  kernel  stg_sample_trajectories alone at K = 20 x N = 2048 x V = 32, P = 12 (63 MB written), captured
  risk    stg_sample_risk (radius 0.5, three rectangles, pair counts) against stg_sample_trajectories on the same
          arguments, both captured: K = 20 at N = 2048 x V = 32 with every slot full, and at N = 600 x V = 128 with the
          ragged scene sizes of the six test recordings (frame scenes taken at a fixed stride)
  bestofk stg_bestofk_eval alone at the kernel case's shape, in-kernel normals, captured
  metrics stg_dist_metrics alone at the kernel case's shape on the sampler's own samples, captured: with the K = 20
          samples, and the closed-form fields alone
  calib   stg_calib_fit (both modes, 2 + 8 P launches) and stg_calib_apply (in place) alone at the kernel case's shape,
          captured; the Predictor replay of the bench case with calibration=; and a 600-stream tick of
          frames.StreamsPredictor (frames_bench.py's streams case, 100 ticks) with and without calibration=

For the kernel's own time run this under `rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py`.
With the diagnostic library (STG_USE_DIAG_LIB=1, `make -C social_stgcnn_amd/csrc DIAG=1`) STG_SAMPLE_PEDS=1 forces
one pedestrian per lane (float2 stores) instead of a pair (float4): the A/B of the store width.
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


def eth_model(dev):
    from social_stgcnn_amd.model import social_stgcnn
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_eth.npz"))
    m = social_stgcnn(**CFG)
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    return m.to(dev).eval()


def time_replays(fn, iters, warmup=10):
    """ms per call of fn() (graph replays), from device events around `iters` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def predictor_case(name, m, obs, peds, k, iters):
    from social_stgcnn_amd.predict import Predictor
    n, _, v, _ = obs.shape
    pr = Predictor(m, k=k)
    replay = pr.capture(n, v, peds)
    replay(obs, seed=1)
    ms = time_replays(pr._graph.replay, iters)
    return {"case": name, "n": n, "v": v, "k": k, "ms_per_replay": round(ms, 5),
            "scenes_per_s": round(n / ms * 1e3, 1), "peds": int(peds.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cases", default="bench,eth,kernel")
    args = ap.parse_args()
    cases = args.cases.split(",")
    from social_stgcnn_amd import data, graphs, ops
    from social_stgcnn_amd import _lib
    dev = torch.device("cuda", 0)
    ops.OPTIONS["wave_path"] = True          # the wave-per-scene kernels for every batch size here
    m = eth_model(dev)
    k, n, v, p = 20, 2048, 32, 12
    info = {"lib": os.path.basename(_lib.LIB_PATH), "sample_peds_env": os.environ.get("STG_SAMPLE_PEDS")}
    if "bench" in cases:
        gen = torch.Generator().manual_seed(0)
        start = torch.rand((n, 1, v, 2), generator=gen) * 20 - 10
        obs = torch.cat([start, start + torch.cumsum(torch.randn((n, 7, v, 2), generator=gen) * 0.3, 1)], 1).to(dev)
        peds = torch.full((n,), v, dtype=torch.int32, device=dev)
        print(json.dumps(dict(predictor_case("predictor_bench", m, obs, peds, k, args.iters), **info)), flush=True)
    if "eth" in cases:
        win = data.load_windows(os.path.join(ROOT, "tests", "golden", "data", "eth_test"), 8, 12, 1,
                                with_non_linear=False)
        _, _, obs_abs, _, counts = data.pad_batch(win, np.arange(len(win)))
        obs, peds = torch.from_numpy(obs_abs).to(dev), torch.from_numpy(counts).to(dev)
        print(json.dumps(dict(predictor_case("predictor_eth_test", m, obs, peds, k, args.iters), **info)), flush=True)
    if "kernel" in cases:
        gen = torch.Generator().manual_seed(1)
        y = (torch.randn((n, p, v, 5), generator=gen) * 0.5).to(dev).permute(0, 3, 1, 2)    # the model's layout
        obs_last = torch.randn((n, v, 2), generator=gen).to(dev)
        seed_dev = torch.ones(1, dtype=torch.int64, device=dev)
        samples = torch.empty((k, n, p, v, 2), device=dev)
        mean = torch.empty((n, p, v, 2), device=dev)

        def run():
            ops.sample_trajectories(y, obs_last, None, k, None, 0, seed_dev, samples, mean)
        g, _ = graphs.warm_capture(run, 1)
        ms = time_replays(g.replay, args.iters)
        written = (samples.numel() + mean.numel()) * 4
        print(json.dumps(dict({"case": "sample_kernel", "k": k, "n": n, "v": v, "p": p, "ms_per_replay": round(ms, 5),
                               "mb_written": round(written / 1e6, 2), "read_mb": round(n * 5 * p * v * 4 / 1e6, 2),
                               "store_tb_per_s": round(written / (ms * 1e-3) / 1e12, 3)}, **info)), flush=True)
    if "bestofk" in cases:
        gen = torch.Generator().manual_seed(3)
        y = (torch.randn((n, p, v, 5), generator=gen) * 0.5).to(dev).permute(0, 3, 1, 2)
        obs_last = torch.randn((n, v, 2), generator=gen).to(dev)
        target_rel = (torch.randn((n, p, v, 2), generator=gen) * 0.5).to(dev)

        def run_best():
            ops.best_of_k(y, target_rel, obs_last, None, k, None, 1)
        ms = time_replays(graphs.warm_capture(run_best, 1)[0].replay, args.iters)
        print(json.dumps(dict({"case": "bestofk", "k": k, "n": n, "v": v, "p": p, "ms_per_replay": round(ms, 5)},
                              **info)), flush=True)
    if "metrics" in cases:
        gen = torch.Generator().manual_seed(4)
        y = (torch.randn((n, p, v, 5), generator=gen) * 0.5).to(dev).permute(0, 3, 1, 2)
        obs_last = torch.randn((n, v, 2), generator=gen).to(dev)
        samples, mean = ops.sample_trajectories(y, obs_last, None, k, None, 1)
        truth = (mean + torch.randn((n, p, v, 2), generator=gen).to(dev)).contiguous()
        for kk, smp in ((k, samples), (0, None)):
            out = ops.dist_buffers(n, p, v, dev, kk > 0)[0]

            def run_metrics():
                ops.dist_metrics(y, mean, smp, truth, None, out=out)
            ms = time_replays(graphs.warm_capture(run_metrics, 1)[0].replay, args.iters)
            print(json.dumps(dict({"case": "dist_metrics", "k": kk, "n": n, "v": v, "p": p, "ms_per_replay": round(ms, 5),
                                   "samples_mb": round(kk * n * p * v * 8 / 1e6, 2)}, **info)), flush=True)
    if "calib" in cases:
        from social_stgcnn_amd.calibrate import Calibration
        from social_stgcnn_amd.predict import Predictor
        gen = torch.Generator().manual_seed(5)
        y = (torch.randn((n, p, v, 5), generator=gen) * 0.5).to(dev).permute(0, 3, 1, 2)
        mean = torch.cumsum(torch.randn((n, p, v, 2), generator=gen) * 0.4, 1).to(dev)
        truth = (mean + torch.randn((n, p, v, 2), generator=gen).to(dev) * 2.0).contiguous()
        out, ws = ops.calib_buffers(n, p, v, dev)
        for mode in ("moment", "coverage"):
            def run_fit():
                ops.calib_fit(y, mean, truth, None, mode, 0.9, out=out, ws=ws)
            ms = time_replays(graphs.warm_capture(run_fit, 1)[0].replay, args.iters)
            print(json.dumps(dict({"case": "calib_fit", "mode": mode, "n": n, "v": v, "p": p, "launches": 2 + 8 * p,
                                   "ms_per_replay": round(ms, 5), "g": [round(float(x), 4) for x in out.g.cpu()],
                                   "ws_mb": round(ws.numel() * 8 / 1e6, 3)}, **info)), flush=True)
        cal = Calibration(out.g, "coverage", 0.9)
        shift = torch.from_numpy(cal.shift).to(dev)

        def run_apply():
            ops.calib_apply(y, shift)
        ms = time_replays(graphs.warm_capture(run_apply, 1)[0].replay, args.iters)
        print(json.dumps(dict({"case": "calib_apply", "n": n, "v": v, "p": p, "ms_per_replay": round(ms, 5),
                               "mb_moved": round(2 * n * 2 * p * v * 4 / 1e6, 2)}, **info)), flush=True)
        start = torch.rand((n, 1, v, 2), generator=gen) * 20 - 10
        obs = torch.cat([start, start + torch.cumsum(torch.randn((n, 7, v, 2), generator=gen) * 0.3, 1)], 1).to(dev)
        peds = torch.full((n,), v, dtype=torch.int32, device=dev)
        for c in (None, cal):
            pr = Predictor(m, k=k, calibration=c)
            pr.capture(n, v, peds)(obs, seed=1)
            ms = time_replays(pr._graph.replay, args.iters)
            print(json.dumps(dict({"case": "predictor_bench", "calibration": c is not None, "n": n, "v": v, "k": k,
                                   "ms_per_replay": round(ms, 5)}, **info)), flush=True)
        import frames_bench                                   # (tools/ is this script's directory)
        for c in (None, cal):
            res = frames_bench.streams_case(600, k, 100, dev, lone=False, calibration=c)
            print(json.dumps(dict(res, calibration=c is not None, **info)), flush=True)
    if "risk" in cases:
        from social_stgcnn_amd import frames
        counts = torch.cat([frames.recording_scenes(data.read_file(os.path.join(ROOT, "tests", "golden", "data", d, f)),
                                                    dev).num_peds
                            for d, f in (("eth_test", "biwi_eth.txt"), ("hotel_test", "biwi_hotel.txt"),
                                         ("univ_test", "students001.txt"), ("univ_test", "students003.txt"),
                                         ("zara1_test", "crowds_zara01.txt"), ("zara2_test", "crowds_zara02.txt"))])
        ragged = counts[torch.arange(600, device=dev) * (len(counts) // 600)].clamp(max=128).contiguous()
        zones = torch.tensor([[-1, -1, 1, 1], [0, 0, 4, 3], [-50, -50, 50, 50]], dtype=torch.float32, device=dev)
        for rn, rv, peds in ((2048, 32, None), (600, 128, ragged)):
            gen = torch.Generator().manual_seed(2)
            y = (torch.randn((rn, p, rv, 5), generator=gen) * 0.5).to(dev).permute(0, 3, 1, 2)
            obs_last = ((torch.rand((rn, rv, 2), generator=gen) * 2 - 1) * (rv ** 0.5)).to(dev)
            seed_dev = torch.ones(1, dtype=torch.int64, device=dev)
            samples = torch.empty((k, rn, p, rv, 2), device=dev)
            mean = torch.empty((rn, p, rv, 2), device=dev)
            risk = ops.sample_risk(y, obs_last, peds, k, 0.5, zones, seed_dev=seed_dev, pairs=True)

            def run_samples():
                ops.sample_trajectories(y, obs_last, peds, k, None, 0, seed_dev, samples, mean)

            def run_risk():
                ops.sample_risk(y, obs_last, peds, k, 0.5, zones, seed_dev=seed_dev, pairs=True, out=risk)
            ms_s = time_replays(graphs.warm_capture(run_samples, 1)[0].replay, args.iters)
            ms_r = time_replays(graphs.warm_capture(run_risk, 1)[0].replay, args.iters)
            vi = torch.full((rn,), rv, device=dev) if peds is None else peds
            print(json.dumps(dict({"case": "risk_kernel", "k": k, "n": rn, "v": rv, "p": p,
                                   "peds": int(vi.sum()), "pair_tests_m": round(float((vi.double() * (vi - 1) / 2).sum())
                                                                                * k * p / 1e6, 1),
                                   "sample_ms": round(ms_s, 5), "risk_ms": round(ms_r, 5),
                                   "ratio": round(ms_r / ms_s, 3),
                                   "risk_mb": round(sum(x.numel() for x in risk[1:]) * 4 / 1e6, 3),
                                   "samples_mb": round(samples.numel() * 4 / 1e6, 2)}, **info)), flush=True)


if __name__ == "__main__":
    main()
