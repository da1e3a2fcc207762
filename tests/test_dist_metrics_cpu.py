"""CPU: the distribution metrics of DESIGN.md 5.31.  The restatement tests/dist_metrics_np.py against scipy's
gaussian_kde, against the score's own float32 and float64 arithmetic and against the properties of the joint errors; the
C ABI declares, exports and refuses what it should before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_edges as de
import dist_metrics_np as dm
import score_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _case(n, p, v, k, peds, seed, spread=1.0):
    """A random prediction: (v_pred (N,5,P,V), mean, samples (K,N,P,V,2), truth), float32."""
    rng = np.random.default_rng(seed)
    v_pred = rng.normal(0, 0.5, (n, 5, p, v)).astype(F)
    mean = np.cumsum(rng.normal(0, 0.4, (n, p, v, 2)), axis=1).astype(F)
    truth = (mean + rng.normal(0, spread, (n, p, v, 2))).astype(F)
    samples = (mean[None] + rng.normal(0, 1.0, (k, n, p, v, 2)) * np.sqrt(1 + np.arange(p))[None, None, :, None, None])
    return v_pred, mean, samples.astype(F), truth


def test_kde_is_scipys_gaussian_kde():
    """Scott's bandwidth, the unbiased covariance and the density as scipy.stats.gaussian_kde(...).logpdf has them, on
    non-degenerate samples: 1e-12 relative, float64 against float64."""
    stats = pytest.importorskip("scipy").stats
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in (3, 4, 20, 64):
        for trial in range(6):
            while True:                                       # non-degenerate: a sample correlation below 0.9
                a = rng.normal(size=(2, 2)) * 10.0 ** rng.uniform(-2, 2)
                pts = rng.normal(size=(k, 2)) @ a.T + rng.normal(size=2) * 5
                if abs(np.corrcoef(pts.T)[0, 1]) < 0.9:
                    break
            at = pts.mean(axis=0) + rng.normal(size=(5, 2)) @ a.T * 2.0
            want = stats.gaussian_kde(pts.T).logpdf(at.T)
            got = dm.kde_logpdf(np.broadcast_to(pts[:, None, :], (k, 5, 2)), at)
            worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
    assert worst <= 1e-12, worst


def test_closed_form_is_the_scores_arithmetic():
    """d2 / nll of the restatement are score_np.cumulative_cov followed by dist_edges.gauss32 in float32 and the float64
    rule in float64; lam is the larger eigenvalue of C_h (numpy's eigvalsh); the float32 values sit inside the bounds."""
    n, p, v, peds = 3, 12, 5, (5, 2, 0)
    v_pred, mean, _, truth = _case(n, p, v, 3, peds, 0)
    ref = dm.restate(v_pred, mean, None, truth, peds)
    d2, nll, lam, cov = dm.closed32(v_pred, mean, truth, peds)
    for b in range(n):
        c = peds[b]
        c32, c64 = score_np.cumulative_cov(v_pred[b], F)[:, :c], score_np.cumulative_cov(v_pred[b])[:, :c]
        dx, dy = mean[b, :, :c, 0] - truth[b, :, :c, 0], mean[b, :, :c, 1] - truth[b, :, :c, 1]
        _, w2, wn = de.gauss32(dx, dy, c32[..., 0], c32[..., 1], c32[..., 2])
        assert np.array_equal(d2[b, :, :c], w2) and np.array_equal(nll[b, :, :c], wn)
        assert np.array_equal(cov[b, :, :c], c32) and not cov[b, :, c:].any()
        x, y = (mean[b, :, :c, i].astype(np.float64) - truth[b, :, :c, i].astype(np.float64) for i in (0, 1))
        det = c64[..., 0] * c64[..., 2] - c64[..., 1] ** 2
        q = (c64[..., 2] * x * x - 2 * c64[..., 1] * x * y + c64[..., 0] * y * y) / det
        assert np.allclose(ref["d2"][b, :, :c], q, rtol=1e-13, atol=0)
        assert np.allclose(ref["nll"][b, :, :c], 0.5 * q + 0.5 * np.log(det) + score_np.LOG_2PI, rtol=1e-13, atol=0)
        m = np.stack([np.stack([c64[..., 0], c64[..., 1]], -1), np.stack([c64[..., 1], c64[..., 2]], -1)], -2)
        assert np.allclose(ref["lam"][b, :, :c], np.linalg.eigvalsh(m)[..., 1], rtol=1e-12, atol=0)
        d2_b, nll_b, r_d = de.score_bound(c64, x, y, ref["d2"][b, :, :c], p)
        assert (np.abs(d2[b, :, :c] - ref["d2"][b, :, :c]) <= d2_b).all() and (r_d < 0.5).all()
        assert (np.abs(nll[b, :, :c] - ref["nll"][b, :, :c]) <= nll_b).all()
        assert (np.abs(lam[b, :, :c] - ref["lam"][b, :, :c]) <= dm.LAM_EPS(p) * ref["lam"][b, :, :c]).all()
    for name in ("d2", "nll", "lam"):
        assert not ref[name][1, :, 2:].any() and not ref[name][2].any()
    assert not d2[2].any() and not lam[1, :, 2:].any()
    assert all(ref[name] is None for name in ("kde_nll", "ade", "fde", "jade", "jfde", "jbest"))


@pytest.mark.parametrize("k", (3, 20))
def test_joint_errors(k):
    """jade >= the scene's mean ade (one sample for everybody cannot beat each pedestrian's own best), with equality for
    a scene of one; K = 3 works; an empty scene gives zeros and jbest -1; jbest is the arg-min of the scene sums."""
    n, p, v, peds = 4, 12, 6, (6, 3, 0, 1)
    v_pred, mean, samples, truth = _case(n, p, v, k, peds, 1)
    r = dm.restate(v_pred, mean, samples, truth, peds)
    for b, c in enumerate(peds):
        if c == 0:
            assert r["jade"][b] == 0 and r["jfde"][b] == 0 and r["jbest"][b] == -1
            assert not r["ade"][b].any() and not r["kde_nll"][b].any()
            continue
        assert r["jade"][b] >= r["ade"][b, :c].mean() * (1 - 1e-15)
        assert r["jfde"][b] >= r["fde"][b, :c].mean() * (1 - 1e-15)
        assert 0 <= r["jbest"][b] < k and r["jbest"][b] == r["scene_sums"][:, b].argmin()
        assert np.isfinite(r["kde_nll"][b]).all() and not r["kde_nll"][b, :, c:].any()
    assert np.isclose(r["jade"][3], r["ade"][3, 0], rtol=1e-14) and np.isclose(r["jfde"][3], r["fde"][3, 0], rtol=1e-14)
    if k == 20:                                                # six pedestrians do not share their best of 20 samples
        assert r["jade"][0] > r["ade"][0].mean() * (1 + 1e-6) and r["jfde"][0] > r["fde"][0].mean() * (1 + 1e-6)
    s = dm.summary(r, peds, (0.5, 0.9))
    assert s["pedestrians"] == 10 and s["scenes"] == 3 and s["count"].tolist() == [10] * p
    assert s["jade"] >= s["ade"] * 0 and np.isfinite([s["amd"], s["amv"], s["nll"], s["kde_nll"], s["jade"]]).all()


def test_clip_and_collinear_samples():
    """Collinear samples leave a finite value (the determinant floor); a truth far away is clipped at kde_floor."""
    k = 20
    line = np.linspace(-1, 1, k)[:, None] * np.array([[1.0, 2.0]])                    # (K,2) on one line
    near = dm.kde_logpdf(line[:, None, :], np.array([[0.1, 0.2], [0.5, -0.5]]))
    assert np.isfinite(near).all()
    assert dm.clip_nll(near, 20.0)[1] == 20.0 and dm.clip_nll(near, 20.0)[0] < 20.0
    assert dm.clip_nll(np.array([np.nan, -np.inf, 3.0]), 20.0).tolist() == [20.0, 20.0, -3.0]


def test_the_metrics_header_its_binding_and_the_export(L):
    """include/stgcnn_hip_metrics.h -- which stgcnn_hip.h includes -- as _lib binds it from that header
    (tests/test_lib_cpu.py checks the binding of all eight): its one entry point by name, nothing but void * and four
    scalar types among its parameters; the ABI version 8."""
    from social_stgcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r'^#include "stgcnn_hip_metrics.h"$', main, re.M)
    assert main.index('#include "stgcnn_hip_metrics.h"') > main.index('extern "C" {')
    assert re.search(r"#define STG_ABI_VERSION 8\b", main)
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_metrics.h")).read()
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_dist_metrics"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_float}, p.name
        assert fn.restype == ctypes.c_int, p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


def test_the_entry_point_refuses_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    from social_stgcnn_amd import _lib
    f = ctypes.c_void_p(64)

    def call(n=2, p=12, v=5, k=20, v_pred=f, mean=f, samples=f, truth=f, d2=f, kde=f, jbest=f, ade_ref=None, fde_ref=None):
        return L.stg_dist_metrics(v_pred, 60 * v, 12 * v, v, 1, mean, samples, truth, f, n, p, v, k, 20.0, None, d2, f, f,
                                  kde, f, f, f, f, jbest, ade_ref, fde_ref, None)
    einval = {"K=1": dict(k=1), "K=2": dict(k=2), "K<0": dict(k=-1), "P=0": dict(p=0), "V=0": dict(v=0), "N<0": dict(n=-1),
              "null truth": dict(truth=None), "null mean": dict(mean=None), "null v_pred": dict(v_pred=None),
              "null d2": dict(d2=None), "null kde_nll with K": dict(kde=None), "null jbest with K": dict(jbest=None),
              "null samples with K": dict(samples=None), "samples without K": dict(k=0),
              "ade_ref alone": dict(ade_ref=f), "fde_ref alone": dict(fde_ref=f),
              "ade_ref without samples": dict(k=0, samples=None, ade_ref=f, fde_ref=f),
              "misaligned truth": dict(truth=ctypes.c_void_p(68)), "misaligned samples": dict(samples=ctypes.c_void_p(68))}
    for name, kw in einval.items():
        assert call(**kw) == -1, name
        assert b"stg_dist_metrics" in L.stg_last_error(), name
    for name, kw in {"K": dict(k=65), "P": dict(p=33), "V": dict(v=257)}.items():
        assert call(**kw) == _lib.EUNSUPPORTED, name
        assert (name + "=").encode() in L.stg_last_error() and b"STG_SCORE_MAX_" + name.encode() in L.stg_last_error()
    assert call(n=0) == 0 and call(n=0, truth=None, samples=None) == 0          # no scenes: a no-op, nothing is looked at
    assert call(n=0, k=2) == -1 and call(n=0, v=257) == _lib.EUNSUPPORTED       # ... but the sizes are


def test_ops_dist_metrics_checks_its_arguments():
    """Decided from the arguments on the host, ahead of any device work (meta tensors stand in for device memory)."""
    import torch
    from social_stgcnn_amd import ops
    assert ops.DistMetrics._fields == ("d2", "nll", "lam", "kde_nll", "ade", "fde", "jade", "jfde", "jbest")
    m, cov = ops.dist_buffers(2, 12, 5, "meta", samples=False, cov=True)
    assert m.kde_nll is None and m.jbest is None and tuple(cov.shape) == (2, 12, 5, 3)
    m, cov = ops.dist_buffers(2, 12, 5, "meta")
    assert cov is None and m.jbest.dtype == torch.int32 and tuple(m.ade.shape) == (2, 5) and tuple(m.jade.shape) == (2,)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dist_metrics(torch.zeros(1, 5, 12, 3), torch.zeros(1, 12, 3, 2), None, torch.zeros(1, 12, 3, 2))
