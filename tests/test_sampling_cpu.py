"""CPU: the trajectory-sampling entry point (stg_sample_trajectories) is declared, exported and validates its
arguments without a GPU; the reference-trajectory fixture agrees with the committed reference evaluation; the numpy
replay of the in-kernel normal stream is sane."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
import philox_np


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_and_library_exports_sample_trajectories(L):
    from social_stgcnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r"\bint\s+stg_sample_trajectories\s*\(", hdr)
    assert "stg_sample_trajectories" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "stg_sample_trajectories")
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


def test_sample_trajectories_rejects_bad_arguments_without_a_gpu(L):
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call

    def call(pred=f, n=2, p=12, v=4, k=3, samples=f, mean=f):
        return L.stg_sample_trajectories(pred, 1, 1, 1, 1, None, None, None, 0, None, n, p, v, k, samples, mean,
                                         None)
    cases = {"N<0": dict(n=-1), "P=0": dict(p=0), "P<0": dict(p=-3), "V=0": dict(v=0), "V<0": dict(v=-1),
             "K<0": dict(k=-1), "pred NULL": dict(pred=None), "samples NULL, K>0": dict(samples=None),
             "no output": dict(k=0, samples=None, mean=None)}
    for name, kw in cases.items():
        assert call(**kw) == -1, name
        assert b"stg_sample_trajectories" in L.stg_last_error(), name
    assert b"null" in L.stg_last_error()
    # N == 0 is a no-op (nothing launched, so this runs without a GPU too)
    assert call(n=0, pred=None, samples=None, mean=None) == 0


def test_reference_samples_fixture_reproduces_the_reference_best_of_20():
    """samples_eth.npz (the reference test()'s raw_data_dict on eth/test, torch.manual_seed(0)): best-of-20 over its
    `pred` with metrics.ade / fde's arithmetic (float32 differences, float64 square root and sum) equals the
    per-pedestrian ADE / FDE of eval_splits.npz."""
    s, g = load_golden("samples_eth.npz"), load_golden("eval_splits.npz")
    assert s["obs"].shape == (8, 181, 2) and s["trgt"].shape == (12, 181, 2) and s["pred"].shape == (20, 12, 181, 2)
    assert np.array_equal(s["num_peds"], g["eth/num_peds"]) and int(s["num_peds"].sum()) == 181
    d = s["pred"] - s["trgt"][None]
    err = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float64))     # (20, 12, 181)
    ade = (err.sum(axis=1) / 12).min(axis=0)
    fde = err[:, -1].min(axis=0)
    np.testing.assert_allclose(ade, g["eth/per_ped_ade"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(fde, g["eth/per_ped_fde"], rtol=0, atol=1e-6)
    assert abs(ade.mean() - float(g["eth/ade"])) < 1e-6 and abs(fde.mean() - float(g["eth/fde"])) < 1e-6
    # the observed tracks end where the targets and every sample start from
    assert np.all(np.isfinite(s["pred"]))


def test_philox_replay_is_the_standard_generator_and_draws_normals():
    # Philox4x32-10 known answer (Salmon et al. 2011, counter 0 / key 0) through the same rounds with c3 = 0
    M0, M1 = 0xD2511F53, 0xCD9E8D57
    c, k = [0, 0, 0, 0], [0, 0]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    assert c == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # the vectorised replay runs the same rounds (with the library's fixed fourth counter word)
    words = philox_np.philox4x32_10(np.uint64(5) + (np.uint64(7) << np.uint64(32)), 11, 0x123456789ABCDEF)
    c, k = [5, 7, 11, 0x5354474E], [0x89ABCDEF, 0x01234567]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    assert [int(w) for w in words] == c
    z = philox_np.noise_tensor(3, 16, 8, 12, 20)                       # 46,080 normals
    assert z.shape == (16, 8, 12, 20, 2)
    se = 1.0 / math.sqrt(z.size)
    assert abs(z.mean()) < 5 * se and abs(z.var() - 1.0) < 5 * math.sqrt(2.0) * se
    assert abs(np.mean(z[..., 0] * z[..., 1])) < 5 * math.sqrt(2.0) * se
    assert not np.array_equal(z, philox_np.noise_tensor(4, 16, 8, 12, 20))


def test_sampling_argument_rules_on_cpu_tensors():
    """ops.sample_args (the checks best_of_k, sample_trajectories and sample_risk share), _lib.seed_u64 / seed_i64 and
    ops.risk_zones, on CPU tensors: N = 2, P = 3, V = 4, K = 2."""
    import torch
    from social_stgcnn_amd import _lib, ops
    n, p, v, k = 2, 3, 4, 2
    y = torch.zeros((n, p, v, 5), dtype=torch.float64).permute(0, 3, 1, 2)          # a strided (N,5,P,V) view
    ol, nz = torch.ones((n, v, 2)), torch.ones((k, n, p, v, 2))
    seed_dev = torch.zeros(1, dtype=torch.int64)
    bad = {"y (N,5,P,V)": [dict(y=torch.zeros((n, 4, p, v))), dict(y=torch.zeros((n, 5, p))),
                           dict(y=torch.zeros((n, p, v, 5)))],
           "obs_last (N,V,2)": [dict(obs_last=torch.zeros((n, v + 1, 2))), dict(obs_last=torch.zeros((n, v))),
                                dict(obs_last=torch.zeros((v, n, 2)))],
           "noise (K,N,P,V,2)": [dict(noise=torch.zeros((k + 1, n, p, v, 2))), dict(noise=torch.zeros((n, p, v, 2))),
                                 dict(noise=torch.zeros((k, n, v, p, 2)))],
           "seed_dev must be a one-element int64": [dict(seed_dev=torch.zeros(2, dtype=torch.int64)),
                                                    dict(seed_dev=torch.zeros(1, dtype=torch.int32))]}
    for what in ("best_of_k", "sample_trajectories", "sample_risk"):
        for msg, cases in bad.items():
            for kw in cases:
                args = {**dict(y=y, k=k, obs_last=ol, noise=nz, seed_dev=seed_dev), **kw}
                with pytest.raises(ValueError, match="^" + re.escape("%s: %s" % (what, msg))):
                    ops.sample_args(what, **args)
    # what comes back: float32 throughout, y with its strides, obs_last and noise contiguous, the sizes
    ol64 = torch.arange(2.0 * n * v, dtype=torch.float64).reshape(2, n, v).permute(1, 2, 0)
    nz16 = torch.ones((2, k, n, p, v), dtype=torch.float16).permute(1, 2, 3, 4, 0)
    assert not ol64.is_contiguous() and not nz16.is_contiguous()
    y2, ol2, nz2, *sizes = ops.sample_args("sample_risk", y, k, ol64, nz16, seed_dev)
    assert sizes == [n, p, v]
    assert y2.dtype == torch.float32 and y2.shape == y.shape and y2.stride() == y.stride()
    assert ol2.dtype == torch.float32 and ol2.is_contiguous() and torch.equal(ol2, ol64.to(torch.float32))
    assert nz2.dtype == torch.float32 and nz2.is_contiguous() and nz2.shape == (k, n, p, v, 2)
    yf = y.to(torch.float32)
    assert ops.sample_args("best_of_k", yf, k, None, None)[:3] == (yf, None, None)
    assert ops.sample_args("best_of_k", yf, k, ol, nz)[1] is ol                    # nothing to convert: no copy

    # one seed, the same 64 bits as the ABI's uint64 and as the int64 of a seed_dev tensor
    s = 2 ** 64 - 3
    assert _lib.seed_u64(s) == s and _lib.seed_i64(s) == -3
    assert ctypes.c_uint64(_lib.seed_i64(s)).value == _lib.seed_u64(s) == ctypes.c_uint64(s).value
    assert torch.tensor([_lib.seed_i64(s)], dtype=torch.int64).numpy().view(np.uint64)[0] == s
    for s in (0, 7, 2 ** 63 - 1, 2 ** 63, 2 ** 64 + 5, -1):
        assert _lib.seed_u64(s) == s % 2 ** 64 and (_lib.seed_i64(s) - s) % 2 ** 64 == 0
        assert -2 ** 63 <= _lib.seed_i64(s) < 2 ** 63

    # rectangles: (Z,4) for every scene (stride 0) or (N,Z,4) per scene (stride 4 Z); anything else is refused
    cpu = torch.device("cpu")
    assert ops.risk_zones(None, n, cpu) == (None, 0, 0)
    shared = np.arange(12, dtype=np.float64).reshape(3, 4)
    t, z, z_sn = ops.risk_zones(shared, n, cpu)
    assert (z, z_sn) == (3, 0) and t.dtype == torch.float32 and t.is_contiguous()
    assert np.array_equal(t.numpy(), shared.astype(np.float32))
    per = torch.from_numpy(np.stack([shared, shared + 1])).to(torch.float32)
    t, z, z_sn = ops.risk_zones(per, n, cpu)
    assert (z, z_sn) == (3, 12) and t is per                                       # a ready tensor is used as it is
    for empty in (np.zeros((0, 4)), np.zeros((n, 0, 4))):
        with pytest.raises(ValueError, match="holds no rectangle"):
            ops.risk_zones(empty, n, cpu)
    for wrong in (np.zeros((n + 1, 3, 4)), np.zeros((3, 5)), np.zeros(4), np.zeros((n, 3, 5))):
        with pytest.raises(ValueError, match=r"zones \(Z,4\) or \(N,Z,4\) expected"):
            ops.risk_zones(wrong, n, cpu)
