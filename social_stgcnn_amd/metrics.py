"""Drop-in `metrics.py` hot-path function: bivariate_loss on the fused `nll` HIP kernel
(reference metrics.py:84-113), plus the evaluation bookkeeping of metrics.py:21-75 in
vectorised host form for the repo's own eval harness."""
import collections

import numpy as np
import torch

from . import ops


def bivariate_loss(V_pred, V_trgt, num_peds=None):
    """metrics.py:84-113.  Reference call: V_pred (P,V,5), V_trgt (P,V,2) -> scalar (mean over P,V).
    Batched call: V_pred (N,P,V,5), V_trgt (N,P,V,2) [+ num_peds] -> per-scene losses (N,).
    V_pred may be any strided view (e.g. the model output permuted like train.py:52)."""
    if V_pred.dim() == 3:
        return ops.bivariate_nll(V_pred.unsqueeze(0), V_trgt.unsqueeze(0), None)[0]
    return ops.bivariate_nll(V_pred, V_trgt, num_peds)


def rel_to_abs(nodes, init_node):
    """metrics.py:66-75 (nodes_rel_to_nodes_abs): cumulative displacements + start position."""
    nodes = np.asarray(nodes)
    return np.cumsum(nodes, axis=0, dtype=nodes.dtype) + np.asarray(init_node)[None]


def ade(pred, target):
    """metrics.py:21-37 for one scene: mean over peds and time of the displacement error. (T,V,2)."""
    err = np.sqrt(((np.asarray(pred, np.float64) - np.asarray(target, np.float64)) ** 2).sum(axis=2))
    return float(err.mean())


def fde(pred, target):
    """metrics.py:40-53 for one scene: mean over peds of the final-step error."""
    err = np.sqrt(((np.asarray(pred, np.float64)[-1] - np.asarray(target, np.float64)[-1]) ** 2).sum(axis=1))
    return float(err.mean())


DistSummary = collections.namedtuple(
    "DistSummary", "levels count amd_h amv_h nll_h kde_nll_h coverage_h amd amv nll kde_nll coverage ade fde jade jfde "
                   "pedestrians scenes")
DistSummary.__doc__ = """ops.DistMetrics reduced (`dist_summary`), numpy float64 / Python numbers.  Per horizon (P,): count
(the elements behind each mean), amd_h (mean of sqrt(d2)), amv_h (mean of lam), nll_h, kde_nll_h, coverage_h (P,Q): the
share of elements with d2 inside the chi-square(2) ellipse of each level.  Over all elements: amd, amv, nll, kde_nll,
coverage (Q,).  ade / fde: the best-of-K errors averaged over `pedestrians`; jade / jfde: the joint errors averaged over
`scenes`, the scenes with at least one pedestrian.  A mean over nothing is nan; the sample-based figures are nan without
samples."""


def dist_sums(m, num_peds=None, levels=(0.5, 0.9, 0.99)):
    """The sums behind `dist_summary`, float64 on the device and without a synchronisation, so that several batches can
    be added before they are read: (per horizon (P,5+Q) = {count, sum sqrt(d2), sum lam, sum nll, sum kde_nll, #(d2 <=
    thr_q)}, (6,) = {pedestrians, sum ade, sum fde, scenes with a pedestrian, sum jade, sum jfde})."""
    n, p, v = m.d2.shape
    dev = m.d2.device
    if num_peds is None:
        c = torch.full((n,), v, device=dev, dtype=torch.int64)
    else:
        c = torch.as_tensor(num_peds).to(device=dev, dtype=torch.int64).reshape(n).clamp(0, v)
    ok = torch.arange(v, device=dev)[None, :] < c[:, None]                                       # (N,V)
    w = ok[:, None, :].to(torch.float64).expand(n, p, v)
    # the kernel's own comparison: float32 d2 against the float32 threshold
    thr = torch.tensor(ops.score_thresholds(levels), dtype=torch.float32, device=dev)
    zero = torch.zeros((n, p, v), dtype=torch.float64, device=dev)
    cols = [w, m.d2.double().sqrt() * w, m.lam.double() * w, m.nll.double() * w,
            zero if m.kde_nll is None else m.kde_nll.double() * w]
    cols += [(m.d2 <= t).double() * w for t in thr]
    per_h = torch.stack(cols, dim=-1).sum(dim=(0, 2))
    okd, some = ok.double(), (c > 0).double()
    if m.ade is None:
        traj = torch.stack([okd.sum(), zero.sum(), zero.sum(), some.sum(), zero.sum(), zero.sum()])
    else:
        traj = torch.stack([okd.sum(), (m.ade.double() * okd).sum(), (m.fde.double() * okd).sum(), some.sum(),
                            (m.jade.double() * some).sum(), (m.jfde.double() * some).sum()])
    return per_h, traj


def summary_of_sums(per_h, traj, levels, sampled=True):
    """`dist_sums` (of one batch, or added over several) -> DistSummary; reads the sums back (synchronises)."""
    per_h = np.asarray(per_h.cpu() if torch.is_tensor(per_h) else per_h, np.float64)
    traj = np.asarray(traj.cpu() if torch.is_tensor(traj) else traj, np.float64)
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = per_h[:, 0]
        mean_h = per_h[:, 1:] / cnt[:, None]
        tot = per_h.sum(axis=0)
        mean = tot[1:] / tot[0]
        peds, scenes = traj[0], traj[3]
        ade, fde = (traj[1] / peds, traj[2] / peds) if sampled else (nan, nan)
        jade, jfde = (traj[4] / scenes, traj[5] / scenes) if sampled else (nan, nan)
    return DistSummary(tuple(float(x) for x in levels), cnt.astype(np.int64), mean_h[:, 0], mean_h[:, 1], mean_h[:, 2],
                       mean_h[:, 3] if sampled else np.full(len(cnt), nan), mean_h[:, 4:], float(mean[0]), float(mean[1]),
                       float(mean[2]), float(mean[3]) if sampled else nan, mean[4:], float(ade), float(fde), float(jade),
                       float(jfde), int(peds), int(scenes))


def dist_summary(m, num_peds=None, levels=(0.5, 0.9, 0.99)):
    """ops.DistMetrics -> DistSummary (host-side plumbing in torch float64; synchronises only here): per-horizon means of
    sqrt(d2) (AMD), lam (AMV), nll and kde_nll, per-horizon coverage of the chi-square(2) ellipses at `levels` (thresholds
    as ScoreSpec.thresholds: -2 ln(1 - p)), the same over all elements, best-of-K ADE / FDE over the pedestrians and joint
    ADE / FDE over the scenes with at least one pedestrian, with the counts behind each mean.

    AMD / AMV here are the CLOSED-FORM counterparts of Social-Implicit's: that paper fits a Gaussian mixture to the
    samples and takes the Mahalanobis distance and the largest eigenvalue from the fit; here the predicted distribution
    is Gaussian and known (N(mean_h, C_h)), so both are computed from it exactly.  This is not that paper's procedure and
    the figures are not comparable with its tables."""
    per_h, traj = dist_sums(m, num_peds, levels)
    return summary_of_sums(per_h, traj, levels, m.kde_nll is not None)
