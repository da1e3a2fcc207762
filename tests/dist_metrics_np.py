"""numpy restatement of stg_dist_metrics (csrc/dist_metrics.hip): the float64 rule, the float32 emulation
of the closed-form fields, the bounds of the float32 kernel against the float64 rule, and the summary.  A test helper,
not the product path.  Shared by test_dist_metrics_cpu.py and test_gpu_dist_metrics.py.

    restate(v_pred, mean, samples, truth, num_peds)   every field in float64 on the float32 inputs
    closed32(v_pred, mean, truth, num_peds, cov)      d2, nll, lam in float32 as the kernel writes them (numpy fuses no
                                                      multiply-add); cov: the C_h to go on from (the device's own, as the
                                                      score tests do: numpy's float32 exp / tanh are not the device's)
    LAM_EPS, joint_eps                                the derived bounds below
    summary(res, num_peds, levels)                    metrics.dist_summary in numpy

Bounds (u = 2^-24, the assumptions of dist_edges.py).
  lam = 0.5 (cxx + cyy) + sqrt(0.25 (cxx - cyy)^2 + cxy^2).  With (a, b) = dist_edges.cov_eps(p): s = cxx + cyy is within
  (a + u) s, d = cxx - cyy within (a + u) s absolutely; r = sqrt((d/2)^2 + cxy^2) is a Euclidean norm, so it moves by at
  most |delta d| / 2 + |delta cxy| <= (a + u) s / 2 + b s / 2 (sqrt(cxx cyy) <= s / 2), and its own operations (two
  squares, a sum, the root) add 2.5 u r; the final sum one rounding.  s <= 2 lam and r <= lam:
      |lam32 - lam64| <= (2 a + b + 5.5 u) lam64                                                   (LAM_EPS(p))
  joint errors: a score_dist is within 4 u of itself (difference, two squares, their sum halved by the root, the root:
  dist_edges.best_of_k_reference charges the same); a float32 sum of m non-negative terms in ANY order is within
  (m - 1) u of itself to first order; the division by the exactly converted count adds u:
      |jade32 - jade64| <= (c P + 5) u jade64,   |jfde32 - jfde64| <= (c + 5) u jfde64             (joint_eps(m))
  and the same with m = P for a pedestrian's ade, m = 1 for its fde.  Every first-order term is inflated by SLOP."""
import numpy as np

import dist_edges as de
import score_np

F = np.float32
U = de.U
KDE_FLOOR = 20.0


def LAM_EPS(p):
    a, b = de.cov_eps(p)
    return (2 * a + b + 5.5 * U) * de.SLOP


def joint_eps(m):
    return (m + 5) * U * de.SLOP


def clamp_peds(num_peds, n, v):
    if num_peds is None:
        return np.full(n, v, np.int64)
    return np.clip(np.asarray(num_peds, np.int64).reshape(n), 0, v)


def cumulative_cov(v_pred, dtype=np.float64):
    """v_pred (N,5,P,V) float32 -> C (N,P,V,3) in `dtype`, score_np.cumulative_cov scene by scene."""
    return np.stack([score_np.cumulative_cov(np.asarray(y, F), dtype) for y in v_pred])


def gauss64(dx, dy, cxx, cxy, cyy):
    """The float64 rule of score_gauss, with its floor -> (d2, nll)."""
    with np.errstate(all="ignore"):
        pr = cxx * cyy
        det = np.maximum(pr - cxy * cxy, pr * de.DET_FLOOR)
        d2 = (cyy * dx * dx - 2.0 * cxy * dx * dy + cxx * dy * dy) / det
        return d2, 0.5 * d2 + 0.5 * np.log(det) + score_np.LOG_2PI


def kde_logpdf(points, at):
    """The log density at `at` (...,2) of the Gaussian KDE of points (K,...,2) with Scott's bandwidth as
    scipy.stats.gaussian_kde defines it, float64, with the determinant floor of the kernel: H = K^(-1/3) S, S the
    unbiased covariance about the sample mean, the K kernels summed about the nearest sample."""
    pts, at = np.asarray(points, np.float64), np.asarray(at, np.float64)
    k = pts.shape[0]
    dev = pts - pts.mean(axis=0)
    f = k ** (-1.0 / 3.0) / (k - 1)
    hxx, hxy, hyy = f * (dev[..., 0] ** 2).sum(0), f * (dev[..., 0] * dev[..., 1]).sum(0), f * (dev[..., 1] ** 2).sum(0)
    with np.errstate(all="ignore"):
        pr = hxx * hyy
        det = np.maximum(pr - hxy * hxy, pr * de.DET_FLOOR)
        dx, dy = at[..., 0] - pts[..., 0], at[..., 1] - pts[..., 1]
        q = (hyy * dx * dx - 2.0 * hxy * dx * dy + hxx * dy * dy) / det                # (K,...)
        qmin = q.min(axis=0)
        lse = -0.5 * qmin + np.log(np.exp(-0.5 * (q - qmin)).sum(axis=0))
        return lse - np.log(k) - score_np.LOG_2PI - 0.5 * np.log(det)


def clip_nll(logpdf, floor):
    """minus the log density, clipped from above at `floor` (a NaN is clipped too), as the kernel ends."""
    val = -np.asarray(logpdf, np.float64)
    return np.where(val < floor, val, floor)


def restate(v_pred, mean, samples, truth, num_peds=None, kde_floor=KDE_FLOOR):
    """The rule in float64 on the float32 inputs -> dict of the nine fields and cov; the sample-based ones None
    without samples.  Padded slots are zero."""
    v_pred, mean, truth = np.asarray(v_pred, F), np.asarray(mean, F), np.asarray(truth, F)
    n, _, p, v = v_pred.shape
    c = clamp_peds(num_peds, n, v)
    ok = (np.arange(v)[None, :] < c[:, None])                                           # (N,V)
    ok3 = np.broadcast_to(ok[:, None, :], (n, p, v))
    cov = cumulative_cov(v_pred) * ok3[..., None]
    d = mean.astype(np.float64) - truth.astype(np.float64)
    safe = np.where(ok3[..., None], cov, np.array([1.0, 0.0, 1.0]))
    d2, nll = gauss64(d[..., 0], d[..., 1], safe[..., 0], safe[..., 1], safe[..., 2])
    lam = 0.5 * (safe[..., 0] + safe[..., 2]) + np.sqrt(0.25 * (safe[..., 0] - safe[..., 2]) ** 2 + safe[..., 1] ** 2)
    out = dict(cov=cov, d2=d2 * ok3, nll=nll * ok3, lam=lam * ok3, kde_nll=None, ade=None, fde=None, jade=None,
               jfde=None, jbest=None)
    if samples is None:
        return out
    s = np.asarray(samples, F).astype(np.float64)
    t64 = truth.astype(np.float64)
    with np.errstate(all="ignore"):
        out["kde_nll"] = np.where(ok3, clip_nll(kde_logpdf(s, t64), kde_floor), 0.0)
    e = np.sqrt(((s - t64[None]) ** 2).sum(-1)) * ok3[None]                             # (K,N,P,V)
    out["ade"], out["fde"] = e.sum(axis=2).min(axis=0) / p, e[:, :, -1].min(axis=0)
    sa, sl = e.sum(axis=(2, 3)), e[:, :, -1].sum(axis=2)                                # (K,N)
    some = c > 0
    div = np.where(some, c, 1)
    out["jade"] = np.where(some, sa.min(axis=0) / (div * p), 0.0)
    out["jfde"] = np.where(some, sl.min(axis=0) / div, 0.0)
    out["jbest"] = np.where(some, sa.argmin(axis=0), -1).astype(np.int32)
    out["scene_sums"] = sa
    return out


def closed32(v_pred, mean, truth, num_peds=None, cov=None):
    """d2, nll, lam (N,P,V) float32 as the kernel writes them: C_h from numpy's float32 exp / tanh in ascending t (or the
    given float32 `cov` (N,P,V,3)), dist_edges.gauss32, the eigenvalue in float32 as written."""
    v_pred, mean, truth = np.asarray(v_pred, F), np.asarray(mean, F), np.asarray(truth, F)
    n, _, p, v = v_pred.shape
    c = clamp_peds(num_peds, n, v)
    ok3 = np.broadcast_to((np.arange(v)[None, :] < c[:, None])[:, None, :], (n, p, v))
    cov = cumulative_cov(v_pred, F) if cov is None else np.asarray(cov, F)
    cxx, cxy, cyy = (np.where(ok3, cov[..., i], F(j)) for i, j in ((0, 1), (1, 0), (2, 1)))
    dx, dy = mean[..., 0] - truth[..., 0], mean[..., 1] - truth[..., 1]
    _, d2, nll = de.gauss32(dx, dy, cxx, cxy, cyy)
    with np.errstate(all="ignore"):
        dd = cxx - cyy
        lam = F(0.5) * (cxx + cyy) + np.sqrt(F(0.25) * (dd * dd) + cxy * cxy)
    zero = F(0)
    return (np.where(ok3, d2, zero).astype(F), np.where(ok3, nll, zero).astype(F), np.where(ok3, lam, zero).astype(F),
            (cov * ok3[..., None]).astype(F))


def summary(res, num_peds, levels):
    """metrics.dist_summary in numpy float64 from a dict of the nine fields (any float dtype) -> dict."""
    from social_stgcnn_amd import ops
    d2 = np.asarray(res["d2"])
    n, p, v = d2.shape
    c = clamp_peds(num_peds, n, v)
    ok = np.arange(v)[None, :] < c[:, None]
    w = np.broadcast_to(ok[:, None, :], (n, p, v)).astype(np.float64)
    thr = np.asarray(ops.score_thresholds(levels), F)
    cnt = w.sum(axis=(0, 2))

    def mean_h(x):
        return (np.asarray(x, np.float64) * w).sum(axis=(0, 2)) / cnt

    def mean_all(x):
        return float((np.asarray(x, np.float64) * w).sum() / cnt.sum())
    inside = [(d2.astype(F) <= t).astype(np.float64) for t in thr]
    out = dict(count=cnt.astype(np.int64), amd_h=mean_h(np.sqrt(d2.astype(np.float64))), amv_h=mean_h(res["lam"]),
               nll_h=mean_h(res["nll"]), coverage_h=np.stack([mean_h(x) for x in inside], axis=-1),
               amd=mean_all(np.sqrt(d2.astype(np.float64))), amv=mean_all(res["lam"]), nll=mean_all(res["nll"]),
               coverage=np.array([mean_all(x) for x in inside]), pedestrians=int(ok.sum()), scenes=int((c > 0).sum()))
    if res.get("kde_nll") is not None:
        out["kde_nll_h"], out["kde_nll"] = mean_h(res["kde_nll"]), mean_all(res["kde_nll"])
        out["ade"] = float(np.asarray(res["ade"], np.float64)[ok].sum() / ok.sum())
        out["fde"] = float(np.asarray(res["fde"], np.float64)[ok].sum() / ok.sum())
        out["jade"] = float(np.asarray(res["jade"], np.float64)[c > 0].sum() / (c > 0).sum())
        out["jfde"] = float(np.asarray(res["jfde"], np.float64)[c > 0].sum() / (c > 0).sum())
    return out
