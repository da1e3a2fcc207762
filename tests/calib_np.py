"""numpy restatement of stg_calib_fit / stg_calib_apply (csrc/calibrate.hip): the second copy of the
rule.  A test helper, not the product path.  Shared by test_calib_cpu.py and test_gpu_calib.py.

    sig_terms(v_pred, dtype)                 [sx^2, rho sx sy, sy^2] per step (N,P,V,3): numpy's exp / tanh, for the CPU
                                             tests; the GPU tests start from the device's own sig, as the score tests
                                             start from the device's C_h (numpy's float32 exp / tanh are not the device's)
    kernel_sum(x)                            the float64 sum in the kernel's order
    fit(sig, mean, truth, num_peds, ...)     the sequential search; dtype float32: every bit as the kernel; float64: the
                                             rule itself
    shift_of(g), apply(v_pred, shift)        the apply step
    order_bound(...)                         what a float64 sum in ANOTHER order could differ by
    coverage_slack(...)                      the elements whose d2 after apply may fall on the other side of thr

The order of the sums.  The elements (n, v < num_peds[n]) are numbered in ascending (n, v).  Element i belongs to
workgroup i // 256, wave (i % 256) // 64, lane i % 64.  A wave's 64 values (zeros past the last element) are added by the
xor butterfly 32, 16, .. 1 of wave_sum(double) (dist_edges.butterfly_sum), the four waves of a workgroup as
((w0 + w1) + w2) + w3, the workgroups in ascending order starting from workgroup 0's sum.

Bounds (u = 2^-24, the assumptions of dist_edges.py).
  order_bound: a float64 sum of m non-negative terms in any order is within (m - 1) 2^-53 of its exact value S to first
  order; two orders differ by at most twice that, inflated by SLOP.  The moment predicate compares the sum with
  2 count, so a fit is decided by the rule alone -- whatever the order -- where |sum - 2 count| exceeds this bound at
  every candidate the search visits; the GPU tests assert that precondition on the restatement before they ask for
  equal bits.
  coverage_slack: dist_metrics behind stg_calib_apply computes sig'_t from expf(ls + shift_t) where the fit used
  g_t sig_t.  Against the exact g_t sx^2 a term of the fit carries 2 A_E + 2u (expf, the square, the product with g) and
  a term behind the apply 2 A_E + u + 2u |ls + shift| + 2u |shift| (expf, the square, the float32 sum ls + shift and the
  rounding of shift, both doubled by the square); the correlation channel is not touched, so tanhf returns the same
  bits on both sides, and the cross term's two factors sx, sy carry half of each of these.  Both C_h add (P - 1) u for
  their float32 sums.  With a = 2 A_E + 2u (1 + LS) + (P - 1) u, LS = max |ls + shift| + max |shift|, every component of
  either C_h is within a of the float64 sum of g_t sig_t (cxy within a sqrt(cxx cyy)), and d2 moves by at most
  d2_bound(..., a, a): dist_edges.score_bound's formula with these two numbers in place of cov_eps(p).  An element
  whose float64 d2 is further than that from thr is counted on the same side by the fit and by dist_metrics."""
import numpy as np

import dist_edges as de
import dist_metrics_np as dm

F = np.float32
U = de.U
MOMENT, COVERAGE = 0, 1
LOW, HIGH, EMPTY = 1, 2, 4
EXP_LO, EXP_HI, CAND, ROUNDS = -10, 21, 32, 4
WG, WAVE = 256, 64


def threshold(level):
    """The float32 d2 threshold of the float32 level: ScoreSpec.thresholds of it, rounded."""
    from social_stgcnn_amd import ops
    return F(ops.score_thresholds([float(F(level))])[0])


def sig_terms(v_pred, dtype=F):
    """v_pred (N,5,P,V) float32 -> (N,P,V,3) in `dtype`, as written in score_fn.hpp's score_sig."""
    y = np.asarray(v_pred, F).astype(dtype)
    sx, sy, rho = np.exp(y[:, 2]), np.exp(y[:, 3]), np.tanh(y[:, 4])
    return np.stack([sx * sx, rho * sx * sy, sy * sy], axis=-1).astype(dtype)


def live_index(num_peds, n, v):
    """(scene, column) of the elements in the kernel's order."""
    c = dm.clamp_peds(num_peds, n, v)
    ok = np.arange(v)[None, :] < c[:, None]
    return np.nonzero(ok)


def kernel_sum(x):
    """The float64 sum over the last axis in the order of the eval and pick kernels."""
    x = np.asarray(x, np.float64)
    e = x.shape[-1]
    if e == 0:
        return np.zeros(x.shape[:-1])
    groups = -(-e // WG)
    pad = np.zeros(x.shape[:-1] + (groups * WG,))
    pad[..., :e] = x
    waves = de.butterfly_sum(pad.reshape(x.shape[:-1] + (groups, WG // WAVE, WAVE)))        # (..., G, 4)
    wg = waves[..., 0]
    for w in range(1, WG // WAVE):
        wg = wg + waves[..., w]
    total = wg[..., 0]
    for b in range(1, groups):
        total = total + wg[..., b]
    return total


def candidates(rnd, lo, hi, dtype=F):
    """The 32 candidates of a round, ascending, in `dtype` as the kernel forms them in float32."""
    if rnd == 0:
        return np.ldexp(dtype(1), np.arange(EXP_LO, EXP_HI + 1)).astype(dtype)
    lo, hi = dtype(lo), dtype(hi)
    c = np.arange(1, CAND + 1).astype(dtype) * dtype(2.0 ** -5)
    out = (lo + (hi - lo) * c).astype(dtype)
    out[-1] = hi
    return out


def d2_of(off, base, sig_h, g, dtype=F):
    """d2 (len(g), E) of the offsets under base + g sig_h: multiply, then add, then score_gauss."""
    g = np.asarray(g, dtype)[:, None]
    c = [(base[:, i][None] + g * sig_h[:, i][None]).astype(dtype) for i in range(3)]
    if dtype == F:
        return de.gauss32(off[:, 0][None], off[:, 1][None], *c)[1]
    return dm.gauss64(off[:, 0][None], off[:, 1][None], *c)[0]


def fit(sig, mean, truth, num_peds=None, mode=COVERAGE, level=0.9, dtype=F):
    """The rule on sig (N,P,V,3), mean and truth (N,P,V,2): dict of g (P,), bracket (P,2), flags (P,), stats (P,3) and
    `visited`: per horizon and round the (sum d2, count, inside) of all 32 candidates, for the tests' preconditions."""
    sig, mean, truth = np.asarray(sig, F), np.asarray(mean, F), np.asarray(truth, F)
    n, p, v, _ = sig.shape
    at = live_index(num_peds, n, v)
    e = len(at[0])
    thr, lvl = threshold(level), float(F(level))
    g, bracket = np.ones(p, dtype), np.ones((p, 2), dtype)
    flags, stats, visited = np.zeros(p, np.int32), np.zeros((p, 3)), []
    if e == 0:
        flags[:] = EMPTY
        return dict(g=g, bracket=bracket, flags=flags, stats=stats, visited=visited)
    s = sig[at[0], :, at[1]].astype(dtype)                                               # (E,P,3)
    off = (mean[at[0], :, at[1]] - truth[at[0], :, at[1]]).astype(dtype)                 # float32 difference, (E,P,2)
    base = np.zeros((e, 3), dtype)
    for h in range(p):
        lo = hi = dtype(0)
        for rnd in range(ROUNDS):
            cand = candidates(rnd, lo, hi, dtype)
            d2 = d2_of(off[:, h], base, s[:, h], cand, dtype)                            # (32,E)
            with np.errstate(invalid="ignore"):
                sums = kernel_sum(d2)
                inside = (d2.astype(F) <= thr).sum(axis=1) if dtype == F else (d2 <= float(thr)).sum(axis=1)
                ok = sums <= 2.0 * e if mode == MOMENT else inside.astype(np.float64) >= lvl * e
            visited.append((h, rnd, sums, e, inside))
            first = int(np.argmax(ok)) if ok.any() else -1
            if rnd == 0 and (first == 0 or first < 0):
                first, flags[h] = (0, LOW) if first == 0 else (CAND - 1, HIGH)
                lo = hi = cand[first]
            else:
                first = CAND - 1 if first < 0 else first
                lo, hi = (cand[first - 1] if first > 0 else lo), cand[first]
            stats[h] = (e, sums[first], inside[first])
            if flags[h]:
                break
        g[h], bracket[h] = hi, (lo, hi)
        base = np.stack([(base[:, i] + hi * s[:, h, i]).astype(dtype) for i in range(3)], axis=-1)
    return dict(g=g, bracket=bracket, flags=flags, stats=stats, visited=visited)


def shift_of(g):
    """float32(0.5 log(float64 g))."""
    return (0.5 * np.log(np.asarray(g, F).astype(np.float64))).astype(F)


def apply(v_pred, shift):
    """v_pred (N,5,P,V) float32 with the shift added to the two log-sigma channels, a float32 add."""
    out = np.array(v_pred, F)
    out[:, 2:4] = out[:, 2:4] + np.asarray(shift, F)[None, None, :, None]
    return out


def coverage(sig, mean, truth, num_peds, g, levels, dtype=np.float64):
    """The share of the elements, all horizons together, whose d2 under sum_{t<=h} g_t sig_t is at most each level's
    threshold: what distribution_test reports as .coverage for a V_pred shifted by shift_of(g)."""
    sig = np.asarray(sig)
    n, p, v, _ = sig.shape
    at = live_index(num_peds, n, v)
    cov = np.cumsum(sig[at[0], :, at[1]].astype(dtype) * np.asarray(g, dtype)[None, :, None], axis=1, dtype=dtype)
    d = (np.asarray(mean, F)[at[0], :, at[1]] - np.asarray(truth, F)[at[0], :, at[1]]).astype(dtype)
    d2 = dm.gauss64(d[..., 0], d[..., 1], cov[..., 0], cov[..., 1], cov[..., 2])[0]
    return np.array([(d2 <= float(threshold(x))).mean() for x in levels])


def reference_set(weights, windows, count=None):
    """The float64 CPU reference model (oracle/) with the weights of tests/golden/<weights>.npz on the first `count`
    windows of a data.SceneWindows, one window at a time as test_frames_fill_cpu.py runs it: (v_pred (N,5,P,V) float32
    padded to the set's largest V, mean (N,P,V,2) float32, truth (N,P,V,2) float32, num_peds (N,))."""
    import os
    import torch
    from oracle import stgcnn_oracle as O
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", weights + ".npz"))
    state = {k: torch.from_numpy(np.array(w[k])).double() for k in w.files}
    spans = windows.seq_start_end[:count]
    peds = np.array([e0 - s0 for s0, e0 in spans], np.int32)
    n, v = len(spans), int(peds.max())
    v_pred, mean, truth = np.zeros((n, 5, 12, v), F), np.zeros((n, 12, v, 2), F), np.zeros((n, 12, v, 2), F)
    for i, (s0, e0) in enumerate(spans):
        obs = np.transpose(windows.seq[s0:e0, :, :8], (2, 0, 1))                          # (8,V,2) float64
        rel = np.zeros_like(obs)
        rel[1:] = obs[1:] - obs[:-1]
        rel = rel.astype(F).astype(np.float64)
        nodes, lap = O.seq_to_graph_np(np.transpose(rel, (1, 2, 0)))
        x = torch.from_numpy(np.asarray(nodes, np.float64)).unsqueeze(0).permute(0, 3, 1, 2)
        with torch.no_grad():
            y = O.social_stgcnn_forward(state, x, torch.from_numpy(np.asarray(lap, np.float64)), False)[0].numpy()
        c = e0 - s0
        v_pred[i, :, :, :c] = y
        mean[i, :, :c] = np.cumsum(np.transpose(y[:2], (1, 2, 0)), axis=0) + obs[-1][None]
        truth[i, :, :c] = np.transpose(windows.seq[s0:e0, :, 8:], (2, 0, 1))
    return v_pred, mean, truth, peds


# (N, P, V, num_peds) of the fit's cases: a handful of elements at P = 12, 1 and 32 (the limit); 169 elements in three
# waves, the last partial, over two scenes that are empty or nearly; 630 elements in three workgroups
CASES = ((3, 12, 5, (5, 2, 0)), (3, 1, 5, (5, 2, 0)), (3, 32, 5, (5, 2, 0)), (5, 12, 70, (65, 1, 0, 70, 33)),
         (9, 12, 70, None))
G_TRUE = (0.3, 0.8, 2.0, 5.0, 9.0, 14.0)


def case_inputs(i):
    """Case i of CASES: (base (N,P,V,5) float32 -- V_pred is its permuted view, as the model leaves it --, mean, truth
    (N,P,V,2) float32, num_peds): random log sigmas and correlations, the truth drawn from N(mean_h, sum_{t<=h} g*_t
    sig_t) with g*_t = G_TRUE[t % 6], so that a fit has something to find; 7.0 in the padded slots."""
    n, p, v, peds = CASES[i]
    rng = np.random.default_rng(40 + i)
    base = rng.normal(0, 0.5, (n, p, v, 5)).astype(F)
    mean = np.cumsum(rng.normal(0, 0.4, (n, p, v, 2)), axis=1).astype(F)
    sig = sig_terms(base.transpose(0, 3, 1, 2), np.float64)
    cov = np.cumsum(sig * np.resize(G_TRUE, p)[None, :, None, None], axis=1)
    l00 = np.sqrt(cov[..., 0])
    l10 = cov[..., 1] / l00
    l11 = np.sqrt(cov[..., 2] - l10 * l10)
    e = rng.standard_normal((n, p, v, 2))
    truth = (mean + np.stack([l00 * e[..., 0], l10 * e[..., 0] + l11 * e[..., 1]], axis=-1)).astype(F)
    ok = dm.clamp_peds(peds, n, v)[:, None] > np.arange(v)[None, :]
    for x in (base, mean, truth):
        np.moveaxis(x, 2, 1)[~ok] = F(7)
    return base, mean, truth, peds


def order_bound(sums, count):
    """What two float64 summation orders of `count` non-negative terms can differ by, for sums of this size."""
    return 2.0 * max(count - 1, 0) * 2.0 ** -53 * np.abs(np.asarray(sums, np.float64)) * de.SLOP


def moment_margin(res):
    """min over the visited candidates of |sum - 2 count| - order_bound: positive where the order cannot decide."""
    worst = np.inf
    for _, _, sums, e, _ in res["visited"]:
        fin = np.isfinite(sums)
        worst = min(worst, float((np.abs(sums[fin] - 2.0 * e) - order_bound(sums[fin], e)).min()))
    return worst


def d2_bound(cov, dx, dy, d2_ref, a, b):
    """dist_edges.score_bound's bound on |d2 - d2_ref| for a C_h whose components are within a (cxy: b sqrt(cxx cyy))
    of cov (...,3), the float64 one."""
    cxx, cxy, cyy = cov[..., 0], cov[..., 1], cov[..., 2]
    pr = cxx * cyy
    det = np.maximum(pr - cxy * cxy, pr * de.DET_FLOOR)
    e_d = (2 * a + 2 * b + 3 * U) * de.SLOP
    r_d = e_d * pr / det
    m = cyy * dx * dx + 2 * np.abs(cxy * dx * dy) + cxx * dy * dy
    e_n = (a + b + 11 * U) * de.SLOP
    d2_b = (e_n * m + np.abs(d2_ref) * e_d * pr) / (det * (1 - r_d))
    return d2_b + U * (np.abs(d2_ref) + d2_b), r_d


def coverage_slack(sig, v_pred, mean, truth, num_peds, g, thr):
    """(P,) the number of elements per horizon whose float64 d2 under sum_t g_t sig_t lies within d2_bound of thr (see the
    module docstring): what the coverage count of dist_metrics behind the apply may differ by from the fit's stats."""
    sig, v_pred = np.asarray(sig, F), np.asarray(v_pred, F)
    n, p, v, _ = sig.shape
    at = live_index(num_peds, n, v)
    shift = shift_of(g).astype(np.float64)
    ls = v_pred[:, 2:4].astype(np.float64)[at[0], :, :, at[1]]                            # (E,2,P)
    reach = float(np.abs(ls + shift[None, None, :]).max() + np.abs(shift).max()) if len(at[0]) else 0.0
    a = 2 * de.A_E + 2 * U * (1 + reach) + (p - 1) * U
    cov = np.cumsum(sig[at[0], :, at[1]].astype(np.float64) * np.asarray(g, np.float64)[None, :, None], axis=1)
    d = mean[at[0], :, at[1]].astype(np.float64) - truth[at[0], :, at[1]].astype(np.float64)
    d2 = dm.gauss64(d[..., 0], d[..., 1], cov[..., 0], cov[..., 1], cov[..., 2])[0]
    bound, r_d = d2_bound(cov, d[..., 0], d[..., 1], d2, a, a)
    assert (r_d < 0.5).all()
    return (np.abs(d2 - float(thr)) <= bound).sum(axis=0)
