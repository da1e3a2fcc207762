"""Saturated correlations and extreme sigmas for the kernels that read V_pred (N,5,P,V) at evaluation time
(stg_sample_trajectories, stg_bestofk_eval, stg_sample_risk, stg_score_push*, stg_score_push*_timed): the input grid, the
float64 reference, the float32 emulation of sample_draw.hpp and score_fn.hpp, and the bounds derived from the written
arithmetic.  Shared by test_dist_edges_cpu.py and test_gpu_dist_edges.py.

The grid.  Raw correlations RAW (both sides of wherever tanhf saturates), log-sigma pairs PAIRS = LOG_SIGMA^2, |mean|
<= 1.  A pedestrian column (n, v) keeps ONE sigma pair over all t and the raw correlation varies over t: a sampled
position is a running sum over t, so its bound is a sum of per-step bounds of one magnitude.

The bounds.  u = 2^-24.  The installed ROCm ships no accuracy table for its device library, so expf, tanhf, logf and
sincosf are ASSUMED within ULPS = 4 ulp (a relative error of 2 ULPS u = 8u); everything else is IEEE float32, one
rounding of u per operation.  A fused multiply-add drops a rounding and adds none, so a bound that charges every
operation its rounding holds for the contracted and the uncontracted form of every multiply-add alike.  First-order
terms are inflated by SLOP for the second order."""
import functools
import itertools

import numpy as np

import score_np
from frames_fill_np import round_pos

U = 2.0 ** -24
ULPS = 4                                               # assumed (see above)
A_E = A_T = A_LOG = A_SIN = 2 * ULPS * U               # relative error of expf / tanhf / logf / sincosf
SLOP = 1.0 + 2.0 ** -10
RAW = (0.0, 1.0, -1.0, 4.0, -4.0, 7.0, -7.0, 8.0, -8.0, 8.5, -8.5, 9.0, -9.0, 9.02, -9.02, 12.0, -12.0, 40.0, -40.0,
       88.0, -88.0)
LOG_SIGMA = (-10.0, -3.0, 0.0, 3.0, 10.0)
PAIRS = tuple(itertools.product(LOG_SIGMA, LOG_SIGMA))
MODERATE = (0.0, 1.0, -1.0, 4.0, -4.0)
SATURATED = (7.0, 8.0, 8.5, 9.0, 9.02, 12.0, 40.0, 88.0)
JUNK = 7.0                                             # what padded slots hold

# ---- sample_draw.hpp: relative errors of the Cholesky factor -------------------------------------------------------
R00 = A_E + 1.5 * U                                    # l00 = sqrtf(sx*sx): expf, the product halved by the root, the root
R10 = A_T + 2 * A_E + 2 * U + R00 + U                  # l10 = (rho*sx*sy)/l00: three inputs, two products, l00, the division
E_RAD = (2 * A_E + 2 * R10 + 3 * U) * SLOP             # |radicand - sy^2 (1 - rho^2)| <= E_RAD sy^2: sy^2 and l10^2 from
#                                                        their inputs, one rounding per product and one for the difference
R_EPS = A_LOG / 2 + U + A_SIN + U                      # an in-kernel normal against philox_np: logf under the root, the
#                                                        root, sincosf, the product


def valid(num_peds, v):
    return np.arange(v)[None, :] < np.asarray(num_peds)[:, None]                   # (N,V)


def edge_pred(n, p, v, num_peds, seed):
    """The (N,P,V,5) base of a V_pred whose valid columns, numbered j = 0, 1, ... in (n, v) order, hold the sigma pair
    PAIRS[j % 25] at every t and the raw correlations RAW[(12 (j // 25) + t) % 21]: with P = 12, fifty valid columns
    hold the whole cross RAW x PAIRS.  Means uniform in [-1, 1]; JUNK in the padded slots."""
    rng = np.random.default_rng(seed)
    base = np.full((n, p, v, 5), JUNK, np.float32)
    ok = valid(num_peds, v)
    j = 0
    for b in range(n):
        for c in range(v):
            if not ok[b, c]:
                continue
            base[b, :, c, 0:2] = rng.uniform(-1, 1, (p, 2))
            base[b, :, c, 2], base[b, :, c, 3] = PAIRS[j % len(PAIRS)]
            base[b, :, c, 4] = [RAW[(12 * (j // len(PAIRS)) + t) % len(RAW)] for t in range(p)]
            j += 1
    return base


def cross_of(base, num_peds):
    """The set of (raw correlation, log sigma x, log sigma y) over the valid elements of a base."""
    ok = valid(num_peds, base.shape[2])
    el = np.moveaxis(base, 2, 1)[ok][..., 2:5].reshape(-1, 3)
    return {(float(q), float(a), float(b)) for a, b, q in el}


# ---- the sampler: float64 reference and bound ------------------------------------------------------------------------
def _terms(y):
    """y (N,5,P,V) float32 -> the float64 terms of a step: mx, my, sx, sy, rho, sqrt(1 - rho^2) as 1 / cosh(q)."""
    y = np.asarray(y, np.float64)
    return y[:, 0], y[:, 1], np.exp(y[:, 2]), np.exp(y[:, 3]), np.tanh(y[:, 4]), 1.0 / np.cosh(y[:, 4])


def sample_reference(y, obs_last, noise):
    """obs_last + cumsum_t(mu_t + chol(cov_t) eps_t) in float64: y (N,5,P,V), obs_last (N,V,2) or None, noise
    (K,N,P,V,2) -> (K,N,P,V,2).  1 - rho^2 is 1 / cosh(q)^2, so the reference does not cancel."""
    mx, my, sx, sy, rho, omr = _terms(y)
    ex, ey = np.asarray(noise, np.float64)[..., 0], np.asarray(noise, np.float64)[..., 1]
    dx = mx + sx * ex
    dy = my + sy * (rho * ex + omr * ey)
    out = np.stack([np.cumsum(dx, axis=2), np.cumsum(dy, axis=2)], axis=-1)
    return out if obs_last is None else out + np.asarray(obs_last, np.float64)[None, :, None]


def l11_bound(sy, l11):
    """|l11 - l11_ref| before the root's own rounding: the radicand is within E_RAD sy^2 of sy^2 (1 - rho^2) >= 0 and the
    clamp at zero moves it towards that value; |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|)."""
    with np.errstate(divide="ignore", over="ignore"):
        return np.minimum(E_RAD * sy * sy / l11, np.sqrt(E_RAD) * sy)


def sample_bound(y, obs_last, noise, eps_rel=0.0):
    """(K,N,P,V,2) bound on |kernel sample - sample_reference| for every contraction of draw_chol / draw_step.  eps_rel:
    the relative error of the kernel's own normals against `noise` (0 for caller noise, R_EPS for the Philox replay).
    Per step, x: l00 ex within (R00 + u + eps_rel) |sx ex|, one rounding of mx + l00 ex; y: l10 ex within
    (R10 + u + eps_rel) |rho sy ex|, l11 ey within |ey| (l11_bound + (2u + eps_rel) l11), two roundings of sums.  The
    running sum adds u |c_t| per step and the final + obs_last one more rounding."""
    mx, my, sx, sy, rho, omr = _terms(y)
    ex, ey = np.abs(np.asarray(noise, np.float64)[..., 0]), np.abs(np.asarray(noise, np.float64)[..., 1])
    ref = sample_reference(y, None, noise)
    tx = sx * ex
    bx = tx * (R00 + U + eps_rel) + U * (np.abs(mx) + tx)
    l11 = sy * omr
    dl11 = l11_bound(sy, l11)
    t1, t2 = np.abs(rho) * sy * ex, (l11 + dl11) * ey
    by = t1 * (R10 + U + eps_rel) + ey * dl11 + (2 * U + eps_rel) * t2 + U * (t1 + t2) + U * (np.abs(my) + t1 + t2)
    step = np.stack([bx, by], axis=-1) * SLOP
    run = np.zeros(step.shape[:2] + step.shape[3:])
    out = np.zeros_like(step)
    for t in range(step.shape[2]):
        run = run + step[:, :, t]
        run = run + U * (np.abs(ref[:, :, t]) + run)                 # the rounding of c_t
        out[:, :, t] = run
    o = 0.0 if obs_last is None else np.asarray(obs_last, np.float64)[None, :, None]
    return out + U * (np.abs(ref + o) + out) * (obs_last is not None)


def best_of_k_reference(samples, target_rel, obs_last, sample_b):
    """min-over-K ADE / FDE (N,V) of float64 samples (K,N,P,V,2) and their bounds: a distance moves by at most the
    Euclidean norm of the sample's bound plus the kernel's float32 truth (P additions of at most the largest partial
    sum, one of obs_last on either side) and 4u of itself (difference, squares, sum, root); the mean over t adds
    (P + 1) u; |min a - min b| <= max |a - b|."""
    tg = np.asarray(target_rel, np.float64)
    p = tg.shape[1]
    o = np.zeros(tg.shape[:1] + tg.shape[2:]) if obs_last is None else np.asarray(obs_last, np.float64)
    gt = np.cumsum(tg, axis=1) + o[:, None]
    d = np.sqrt(((samples - gt[None]) ** 2).sum(-1))                                # (K,N,P,V)
    part = np.maximum.accumulate(np.abs(np.cumsum(tg, axis=1)), axis=1)
    db = np.sqrt((sample_b ** 2).sum(-1)) + np.sqrt(2.0) * U * ((p + 1) * part.max(-1) + np.abs(gt).max(-1))[None]
    db = (db + 4 * U * (d + db)) * SLOP
    ade, fde = d.mean(axis=2), d[:, :, -1]
    ade_b = db.mean(axis=2) + (p + 1) * U * (ade + db.mean(axis=2))
    return ade.min(axis=0), fde.min(axis=0), ade_b.max(axis=0), db[:, :, -1].max(axis=0)


# (N, P, V, num_peds) of the sampler's cases: V = 40 cuts scenes across waves, ragged, an empty scene; odd V and V = 8
# (written to an output view that is 8- but not 16-byte aligned) take the one-pedestrian kernel.  Each holds the cross
SHAPES = ((3, 12, 40, (40, 17, 0)), (8, 12, 7, (7, 7, 7, 7, 7, 7, 7, 1)), (7, 12, 8, (8, 8, 8, 8, 8, 8, 2)))
SAMPLES_K, SAMPLES_SEED = 8, 0x5EED0123456789AB


@functools.lru_cache(maxsize=None)
def sampler_case(i, philox):
    """Shape i of SHAPES: (base (N,P,V,5), obs_last, target_rel, noise float64 (K,N,P,V,2), valid (N,V), the float64
    reference samples and their bound).  philox: the noise is the numpy replay of the in-kernel stream under
    SAMPLES_SEED, and the bound takes on R_EPS."""
    import philox_np
    n, p, v, peds = SHAPES[i]
    rng = np.random.default_rng(100 + i)
    base = edge_pred(n, p, v, peds, 100 + i)
    obs = rng.uniform(-5, 5, (n, v, 2)).astype(np.float32)
    tgt = rng.normal(scale=0.4, size=(n, p, v, 2)).astype(np.float32)
    if philox:
        noise = philox_np.noise_tensor(SAMPLES_SEED, SAMPLES_K, n, p, v)
    else:
        noise = rng.standard_normal((SAMPLES_K, n, p, v, 2)).astype(np.float32).astype(np.float64)
    y = base.transpose(0, 3, 1, 2)
    ref = sample_reference(y, obs, noise)
    bound = sample_bound(y, obs, noise, R_EPS if philox else 0.0)
    return base, obs, tgt, noise, valid(peds, v), ref, bound


RISK_APART = 3.0e6


@functools.lru_cache(maxsize=None)
def risk_case(i, philox):
    """The geometry of the risk counts for sampler_case(i, philox): (obs_last, radii, zones, the reference's counts
    per radius).  Every pedestrian's allowance is the Euclidean norm of its bound at its worst step and sample.  A
    saturated step of a pedestrian with sigma e^3 or e^10 has an allowance of 2e-3 of its spread, and with thousands
    of (pair, sample, step) events near any radius some count would stay undecided; so those pedestrians start
    RISK_APART apart on a diagonal -- further than twelve steps of six sigma e^10 can close -- while the others
    (sigmas <= 1, allowances of 1e-5) start within +-5 of the origin and meet.  Two radii: the decided one with the
    most conflict counts strictly between 0 and K, and the smallest decided one at which every pedestrian has a partner
    at every step of every sample, so that each conflict count must be K (a NaN sample would leave it low).  The
    rectangles run from the scale of the cluster to one that holds everybody."""
    base, obs, _, noise, ok, _, _ = sampler_case(i, philox)
    obs = obs.copy()
    far = ok & (np.moveaxis(base, 2, 1)[:, :, 0, 2:4].max(axis=-1) > 0)            # (N,V): a log sigma of 3 or 10
    for b in range(far.shape[0]):
        at = RISK_APART * (1 + np.arange(int(far[b].sum())))
        obs[b, far[b]] = np.stack([at, -at], axis=-1)
    y = base.transpose(0, 3, 1, 2)
    ref = sample_reference(y, obs, noise)
    bound = sample_bound(y, obs, noise, R_EPS if philox else 0.0)
    pad = np.where(ok, np.sqrt((bound ** 2).sum(-1)).max(axis=(0, 2)), 0.0)
    return (obs,) + risk_geometry(ref, np.array(SHAPES[i][3]), pad)


# ---- float32 emulation of sample_draw.hpp ----------------------------------------------------------------------------
F = np.float32


def _fma(a, b, c):
    """fmaf through float64: the product of two float32 is exact there."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emu_radicand(sx, sy, rho, fma=False):
    """(l00, l10, radicand) of draw_chol in float32 as written, or with the subtraction contracted:
    fmaf(-l10, l10, sy*sy)."""
    sx, sy, rho = F(sx), F(sy), F(rho)
    c01 = (rho * sx) * sy
    l00 = np.sqrt(sx * sx)
    l10 = c01 / l00
    return l00, l10, (_fma(-l10, l10, sy * sy) if fma else sy * sy - l10 * l10)


def emu_samples(y, obs_last, noise, fixed=True, fma=False):
    """The kernels' samples (K,N,P,V,2) in numpy float32: numpy's float32 exp / tanh, draw_chol (fixed: the radicand
    clamped at zero; else the parent's), draw_step, every multiply-add contracted (fma) or none."""
    y = np.asarray(y, F)
    noise = np.asarray(noise, F)
    k, n, p, v, _ = noise.shape
    cx, cy = np.zeros((k, n, v), F), np.zeros((k, n, v), F)
    out = np.zeros((k, n, p, v, 2), F)
    o = np.zeros((n, v, 2), F) if obs_last is None else np.asarray(obs_last, F)
    with np.errstate(invalid="ignore"):
        for t in range(p):
            mx, my = y[:, 0, t], y[:, 1, t]
            l00, l10, rad = emu_radicand(np.exp(y[:, 2, t]), np.exp(y[:, 3, t]), np.tanh(y[:, 4, t]), fma)
            l11 = np.sqrt(np.maximum(rad, F(0)) if fixed else rad)
            ex, ey = noise[:, :, t, :, 0], noise[:, :, t, :, 1]
            if fma:
                cx = cx + _fma(l00[None] + 0 * ex, ex, mx[None] + 0 * ex)
                cy = cy + (my[None] + _fma(l10[None] + 0 * ex, ex, l11[None] * ey))
            else:
                cx = cx + (mx[None] + l00[None] * ex)
                cy = cy + (my[None] + (l10[None] * ex + l11[None] * ey))
            out[:, :, t, :, 0], out[:, :, t, :, 1] = cx + o[None, :, :, 0], cy + o[None, :, :, 1]
    return out


def random_sigmas(count, seed=0):
    """(sx, sy) float32 with log sigma uniform in [-3, 3]."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(-3, 3, (2, count)).astype(F))


# ---- score_fn.hpp: emulation, arrangements and bounds ----------------------------------------------------------------
DET_FLOOR = 2.0 ** -15
SCORE_MAX_P = 32


def cov_eps(p):
    """(a, b): |dcxx| <= a cxx, |dcyy| <= a cyy, |dcxy| <= b sqrt(cxx cyy) for the float32 C_h of h <= p steps: a term
    sx^2 within 2 A_E + u, a term rho sx sy within A_T + 2 A_E + 2u of sx sy, p - 1 additions of at most the final sum
    (Cauchy-Schwarz over the steps for cxy)."""
    return 2 * A_E + U + (p - 1) * U, A_T + 2 * A_E + 2 * U + (p - 1) * U


def det_eps(p):
    """|fl(det) - det| <= det_eps(p) cxx cyy for the plain difference: cxx cyy within 2a + u, cxy^2 within 2b + u, the
    difference's rounding u."""
    a, b = cov_eps(p)
    return 2 * a + 2 * b + 3 * U


def gauss32(dx, dy, cxx, cxy, cyy, floor=DET_FLOOR):
    """score_gauss in float32 as written (floor None: the parent's plain determinant) -> (det, d2, nll)."""
    dx, dy, cxx, cxy, cyy = (np.asarray(x, F) for x in (dx, dy, cxx, cxy, cyy))
    with np.errstate(all="ignore"):
        pr = cxx * cyy
        det = pr - cxy * cxy
        if floor is not None:
            det = np.maximum(det, pr * F(floor))
        d2 = ((cyy * (dx * dx) - F(2) * cxy * dx * dy) + cxx * (dy * dy)) / det
        nll = (F(0.5) * d2 + F(0.5) * np.log(det.astype(np.float64)).astype(F)) + F(score_np.LOG_2PI)
    return det, d2, nll


def score_bound(cov, dx, dy, d2_ref, p):
    """(bound on |d2 - d2_ref|, bound on |nll - nll_ref|, r_d) of the float32 rule against the float64 one, both with
    the floor.  cov (...,3): the float64 C_h; dx, dy: mean - truth in float64; p: the steps summed at the most.
    The floored det is within det_eps cxx cyy of the floored float64 one (max is 1-Lipschitz), a relative error r_d <=
    det_eps / DET_FLOOR < 1/2.  The numerator is bounded absolutely (on the degenerate line it cancels): each of its
    terms within a + b + 9u of m = cyy dx^2 + 2 |cxy dx dy| + cxx dy^2 in sum (dx, dy one rounding each, the products
    up to five more; 2 sqrt(cxx cyy) |dx dy| <= cyy dx^2 + cxx dy^2), two roundings of sums: e_n = a + b + 11u.  d2 = num / det
    carries (e_n m + d2_ref e_d cxx cyy) / (det (1 - r_d)) and the division's rounding; nll half of that, half of
    |log(1 - r_d)|, the rounding of the float32 logarithm and three of sums."""
    a, b = cov_eps(p)
    cxx, cxy, cyy = cov[..., 0], cov[..., 1], cov[..., 2]
    pr = cxx * cyy
    det = np.maximum(pr - cxy * cxy, pr * DET_FLOOR)
    e_d = det_eps(p) * SLOP
    r_d = e_d * pr / det
    m = cyy * dx * dx + 2 * np.abs(cxy * dx * dy) + cxx * dy * dy
    e_n = (a + b + 11 * U) * SLOP
    d2_b = (e_n * m + np.abs(d2_ref) * e_d * pr) / (det * (1 - r_d))
    d2_b = d2_b + U * (np.abs(d2_ref) + d2_b)
    mag = 0.5 * (np.abs(d2_ref) + d2_b) + 0.5 * np.abs(np.log(det)) + score_np.LOG_2PI
    nll_b = 0.5 * d2_b - 0.5 * np.log1p(-r_d) + 5 * U * (mag + 1.0)
    return d2_b, nll_b, r_d


ARRANGEMENTS = ("all_saturated", "first_saturated", "alternating", "moderate")


def arrangement(kind, p, m, sign):
    """The raw correlations over t of one column of the prediction made at push m."""
    sat = [SATURATED[(t + m) % len(SATURATED)] for t in range(p)]
    mod = [MODERATE[(t + 2 * m) % len(MODERATE)] for t in range(p)]
    if kind == "all_saturated":
        return [sign * q for q in sat]
    if kind == "first_saturated":
        return [sign * sat[0]] + mod[1:]
    if kind == "alternating":
        return [sign * (-1) ** t * q for t, q in enumerate(sat)]
    return mod


class ScoreCase:
    """n_push pushes of ns streams, every column a pedestrian that is detected at every push.  Column j of stream s at
    push m: arrangement (j + m) % 4, sigma pair PAIRS[(8 m + j + 13 s) % 25], the truth a slow walk, the mean at horizon
    h off the truth by sqrt(h) (alpha (sx, sg sy) + beta (sx, -sg sy)): beta = 0 -- the truth on the degenerate line of
    C_h -- where (m + h + j) is even.  Stream 1 holds v - 3 pedestrians and junk in the padded slots."""

    def __init__(self, ns=2, p=12, v=8, k=4, n_push=14, seed=5):
        rng = np.random.default_rng(seed)
        self.ns, self.p, self.v, self.k, self.n_push = ns, p, v, k, n_push
        self.num_peds = [v if s == 0 else v - 3 for s in range(ns)]
        self.ids = np.arange(1, v + 1, dtype=np.int64) + (1 << 33)
        start, vel = rng.uniform(-4, 4, (ns, v, 2)), rng.uniform(-0.3, 0.3, (ns, v, 2))
        self.truth = start[:, None] + vel[:, None] * np.arange(n_push + p + 1)[None, :, None, None]     # (ns,M,v,2)
        self.kinds, self.preds = {}, {}
        for s, m in itertools.product(range(ns), range(n_push)):
            c = self.num_peds[s]
            v_pred = np.full((5, p, v), JUNK, np.float32)
            mean, samples = np.full((p, v, 2), JUNK, np.float32), np.full((k, p, v, 2), JUNK, np.float32)
            for j in range(c):
                kind, sg = ARRANGEMENTS[(j + m) % 4], 1.0 if (j + m) % 8 < 4 else -1.0
                self.kinds[s, m, j] = kind
                lsx, lsy = PAIRS[(8 * m + j + 13 * s) % len(PAIRS)]
                v_pred[0:2, :, j] = rng.uniform(-1, 1, (2, p))
                v_pred[2, :, j], v_pred[3, :, j] = lsx, lsy
                v_pred[4, :, j] = arrangement(kind, p, m, sg)
                sx, sy = np.exp(lsx), np.exp(lsy)
                for h in range(1, p + 1):
                    al, be = rng.uniform(-1.5, 1.5, 2)
                    be = 0.0 if (m + h + j) % 2 == 0 else be
                    off = np.sqrt(h) * (al * np.array([sx, sg * sy]) + be * np.array([sx, -sg * sy]))
                    mean[h - 1, j] = self.truth[s, m + h, j] + off
                    samples[:, h - 1, j] = mean[h - 1, j] + np.sqrt(h) * np.array([sx, sy]) * rng.normal(size=(k, 2))
            cols = np.full(v, -1, np.int64)
            cols[:c] = self.ids[:c]
            self.preds[s, m] = score_np.Prediction(cols, c, mean, v_pred, samples)

    def detections(self, s, m):
        """(ids, positions float64) of stream s at push m: every pedestrian of the stream, the last one first."""
        c = self.num_peds[s]
        order = np.arange(c)[::-1]
        return self.ids[order], self.truth[s, m, order].copy()

    def offsets(self, s, m, h, decimals=None):
        """(dx, dy) float64 (c,): the float32 mean at horizon h of the prediction of push m minus the float32 truth."""
        c = self.num_peds[s]
        t = self.truth[s, m + h, :c]
        t = (t if decimals is None else round_pos(t, decimals)).astype(np.float32).astype(np.float64)
        d = self.preds[s, m].mean[h - 1, :c].astype(np.float64) - t
        return d[:, 0], d[:, 1]


@functools.lru_cache(maxsize=None)
def score_case():
    return ScoreCase()


def butterfly_sum(x):
    """The float64 sum over the last axis (at most 64 entries, one per lane) in the order of the score kernels'
    wave_sum: v += shfl_xor(v, o) for o = 32 .. 1, as lane 0 ends up with it."""
    x = np.asarray(x, np.float64)
    lanes = np.zeros(x.shape[:-1] + (64,))
    lanes[..., :x.shape[-1]] = x
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., np.arange(64) ^ o]
    return lanes[..., 0]


def push_sums(out, thr):
    """What one push of one stream adds to the totals, from its float32 per-element values (a dict with matched, err,
    d2, nll, best (P,V)): (P, 5 + Q), every column the butterfly sum over the pedestrians."""
    on = out["matched"] == 1
    cols = [on.astype(np.float64)] + [np.where(on, np.asarray(out[n], np.float32).astype(np.float64), 0.0)
                                      for n in ("err", "d2", "nll", "best")]
    cols += [(on & (np.asarray(out["d2"], np.float32) <= np.float32(t))).astype(np.float64) for t in thr]
    return np.stack([butterfly_sum(c) for c in cols], axis=-1)


def traj_sums(out, p):
    """What the retired record of one push adds to traj_totals (5,), from traj_steps and the four traj_* (V,)."""
    full = out["traj_steps"] == p
    cols = [full.astype(np.float64)] + [np.where(full, np.asarray(out[n], np.float32).astype(np.float64), 0.0)
                                        for n in ("traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")]
    return np.array([butterfly_sum(c) for c in cols])


# ---- the risk counts: a geometry the reference decides ---------------------------------------------------------------
def risk_geometry(samples, num_peds, pad):
    """Radii and rectangles at which risk_np.bounds, fed the per-pedestrian position bounds `pad` (N,V), leaves no
    count of the float64 samples undecided, from ladders of scales: the radius with the most conflict counts strictly
    between 0 and K and the smallest one at which every count is K; up to eight rectangles, the largest holding every
    sample.  The kernel's own float32 test dx*dx + dy*dy < r*r moves a distance near r by at most 4u r, which every
    pedestrian's allowance takes on.  Returns (radii, zones (Z,4) float32, [counts per radius]) or raises."""
    import risk_np
    k = samples.shape[0]
    vi = risk_np.clamp_peds(num_peds, samples.shape[1], samples.shape[3])
    some = (np.arange(samples.shape[3])[None, :] < vi[:, None]) & (vi[:, None] > 1)      # somebody to meet

    def decided(radius, zones):
        lo, hi = {}, {}
        if radius is not None:                  # (the radius test's own rounding is no part of the rectangle tests)
            lo, hi = risk_np.bounds(samples, num_peds, radius, None, pad + 4 * U * radius)
        if zones is not None:
            for d, part in zip((lo, hi), risk_np.bounds(samples, num_peds, None, zones, pad)):
                d.update(part)
        return lo if all(np.array_equal(lo[f], hi[f]) for f in lo) else None

    best, whole = None, None
    for e in np.arange(-4.0, 34.0, 0.5):
        radius = float(np.float32(2.0 ** e))
        lo = decided(radius, None)
        if lo is None:
            continue
        mixed = int(((lo["conflict"] > 0) & (lo["conflict"] < k)).sum())
        if best is None or mixed > best[0]:
            best = (mixed, radius)
        if whole is None and (lo["conflict"].transpose(0, 2, 1)[some] == k).all():
            whole = radius
    zones = []
    for e in np.arange(0.0, 34.0, 1.0):
        for cx, cy in ((0.0, 0.0), (1.5, -2.5)):
            half = 2.0 ** e
            z = np.array([[cx - half, cy - half, cx + half, cy + 0.75 * half]], np.float32)
            lo = decided(None, z)
            if lo is not None and lo["zone_count"].any():
                zones.append((int(lo["zone_count"].sum()), z[0]))
    if best is None or best[0] == 0 or whole is None or len(zones) < 2:
        raise AssertionError("no decided geometry: radius %s, whole %s, %d zones" % (best, whole, len(zones)))
    full = [z for c, z in zones if c == zones[-1][0]][0]                             # the first that holds everybody
    part = [z for c, z in zones if c < zones[-1][0]]
    zones = np.stack(part[:: max(1, len(part) // 7)][:7] + [full])
    radii = (best[1], whole)
    counts = [decided(r, zones) for r in radii]
    assert all(c is not None for c in counts)
    return radii, zones, counts
