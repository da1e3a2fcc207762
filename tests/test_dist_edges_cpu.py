"""CPU: the saturated-correlation grid of tests/dist_edges.py against the float32 emulation of sample_draw.hpp and
score_fn.hpp -- the parent's arithmetic fails on it (a negative radicand, a non-positive determinant), the present
arithmetic is finite everywhere and inside the bounds derived in DESIGN.md 2.4, for the contracted and the uncontracted
multiply-adds.  The bounds are validated here before test_gpu_dist_edges.py holds the kernels to them."""
import numpy as np

import dist_edges as de
import score_np

SHAPES = de.SHAPES


def test_every_shape_holds_the_whole_cross():
    full = {(float(np.float32(q)), a, b) for q in de.RAW for a, b in de.PAIRS}
    assert len(full) == 21 * 25
    for n, p, v, peds in SHAPES:
        base = de.edge_pred(n, p, v, peds, 1)
        assert de.cross_of(base, peds) == full, (n, v)
        assert np.all(np.moveaxis(base, 2, 1)[~de.valid(peds, v)] == de.JUNK)
        assert np.abs(np.moveaxis(base, 2, 1)[de.valid(peds, v)][..., 0:2]).max() <= 1.0


def _grid_case(shape, k=8, seed=3):
    n, p, v, peds = shape
    rng = np.random.default_rng(seed)
    y = np.ascontiguousarray(de.edge_pred(n, p, v, peds, seed).transpose(0, 3, 1, 2))
    obs = rng.uniform(-5, 5, (n, v, 2)).astype(np.float32)
    noise = rng.standard_normal((k, n, p, v, 2)).astype(np.float32)
    return y, obs, noise, de.valid(peds, v)


def _vp(a):
    return np.moveaxis(np.asarray(a), -3, -2)


def test_parent_radicand_goes_negative():
    """draw_chol as the parent wrote it, 200 k random sigmas (log sigma in [-3, 3]) and the grid's pairs: at raw
    correlation 12 (tanh = 1.0f) the radicand sy^2 - l10^2 is rounding noise of either sign -- negative for about half
    of the sigmas once the subtraction is contracted (the error of l10^2 is symmetric), for some as written; at 9 the
    contracted form already goes negative.  A negative radicand is a NaN sample, and every later step of it."""
    sx, sy = de.random_sigmas(200000)
    gx, gy = np.exp(np.array(de.PAIRS, np.float32)).T
    sx, sy = np.concatenate([sx, gx]), np.concatenate([sy, gy])
    share = {}
    for q in (9.0, 12.0):
        for fma in (False, True):
            rad = de.emu_radicand(sx, sy, np.tanh(np.float32(q)), fma)[2]
            share[q, fma] = float((rad < 0).mean())
    print("parent draw_chol, share of negative radicands:", {k: "%.1f %%" % (100 * x) for k, x in share.items()})
    assert share[12.0, True] > 0.25 and share[12.0, False] > 0 and share[9.0, True] > 0
    y, obs, noise, ok = _grid_case(SHAPES[0])
    nan = {fma: float(np.isnan(_vp(de.emu_samples(y, obs, noise, fixed=False, fma=fma))[:, ok]).mean())
           for fma in (False, True)}
    print("parent sampler on the grid, share of NaN positions (as written, contracted):", nan)
    assert max(nan.values()) > 0


def test_fixed_sampler_is_finite_and_inside_the_bound():
    """The clamped radicand on every shape of the GPU tests, both contraction forms, no element excluded; then every
    raw correlation of the grid against 200 k random sigmas, one step."""
    worst = 0.0
    for shape in SHAPES:
        y, obs, noise, ok = _grid_case(shape)
        ref = de.sample_reference(y, obs, noise)
        bound = de.sample_bound(y, obs, noise)
        assert np.isfinite(_vp(bound)[:, ok]).all() and (_vp(bound)[:, ok] > 0).all()
        for fma in (False, True):
            got = de.emu_samples(y, obs, noise, fixed=True, fma=fma)
            assert np.isfinite(_vp(got)[:, ok]).all()
            ratio = (_vp(np.abs(got - ref)) / _vp(bound))[:, ok]
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (shape[:3], fma, float(ratio.max()))
    sx, sy = de.random_sigmas(200000, seed=1)
    rng = np.random.default_rng(2)
    y = np.zeros((len(de.RAW), 5, 1, sx.size), np.float32)
    y[:, 0:2] = rng.uniform(-1, 1, (len(de.RAW), 2, 1, sx.size))
    y[:, 2], y[:, 3] = np.log(sx)[None, None], np.log(sy)[None, None]
    y[:, 4] = np.array(de.RAW, np.float32)[:, None, None]
    noise = rng.standard_normal((1,) + y.shape[:1] + y.shape[2:] + (2,)).astype(np.float32)
    ref, bound = de.sample_reference(y, None, noise), de.sample_bound(y, None, noise)
    for fma in (False, True):
        got = de.emu_samples(y, None, noise, fixed=True, fma=fma)
        assert np.isfinite(got).all()
        ratio = np.abs(got - ref) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (fma, float(ratio.max()))
    print("emulated sampler, worst error / bound: %.3f" % worst)


def test_best_of_k_bound_holds_for_the_emulation():
    y, obs, noise, ok = _grid_case(SHAPES[0])
    rng = np.random.default_rng(9)
    tgt = rng.normal(scale=0.4, size=y.shape[:1] + y.shape[2:] + (2,)).astype(np.float32)
    ref = de.sample_reference(y, obs, noise)
    ade, fde, ade_b, fde_b = de.best_of_k_reference(ref, tgt, obs, de.sample_bound(y, obs, noise))
    gt = (np.cumsum(tgt.astype(np.float64), axis=1) + obs[:, None]).astype(np.float32)
    for fma in (False, True):
        s = de.emu_samples(y, obs, noise, fma=fma)
        d = np.sqrt(((s - gt[None]) ** 2).sum(-1, dtype=np.float32))
        a, f = d.mean(axis=2, dtype=np.float32).min(axis=0), d[:, :, -1].min(axis=0)
        assert (np.abs(a - ade)[ok] <= ade_b[ok]).all() and (np.abs(f - fde)[ok] <= fde_b[ok]).all()


def test_the_floor_is_where_the_derivation_puts_it():
    """The relative error of the floored determinant is det_eps / floor at the floor: at most one half at 2^-15 up to
    the kernel's longest horizon, above one half one power of two lower, and 8.3 at 2^-20."""
    assert de.det_eps(12) / de.DET_FLOOR <= 0.5 and de.det_eps(de.SCORE_MAX_P) / de.DET_FLOOR <= 0.5
    assert de.det_eps(12) / (de.DET_FLOOR / 2) > 0.5
    assert 8.0 < de.det_eps(12) / 2.0 ** -20 < 8.5


def _covs(case, dtype):
    return {key: score_np.cumulative_cov(pr.v_pred, dtype) for key, pr in case.preds.items()}


def test_parent_determinant_fails_on_the_arrangements():
    """score_gauss with the parent's plain determinant on the float32 C_h of every arrangement: non-positive
    determinants (d2 infinite, NaN or negative, nll NaN) where every step, or step 1, is saturated; with the floor
    every determinant is positive and every value finite."""
    case = de.score_case()
    bad = {k: 0 for k in de.ARRANGEMENTS}
    total = 0
    for (s, m), cov in _covs(case, np.float32).items():
        c = case.num_peds[s]
        for h in range(1, case.p + 1):
            dx, dy = case.offsets(s, m, h)
            cc = cov[h - 1, :c]
            det, d2, nll = de.gauss32(dx, dy, cc[:, 0], cc[:, 1], cc[:, 2], floor=None)
            wrong = (det <= 0) | ~np.isfinite(d2) | ~np.isfinite(nll)
            for j in np.nonzero(wrong)[0]:
                bad[case.kinds[s, m, j]] += 1
            total += c
            det, d2, nll = de.gauss32(dx, dy, cc[:, 0], cc[:, 1], cc[:, 2])
            # (with the truth on the degenerate line the numerator cancels to rounding noise of either sign, so a d2 of
            # about zero may be a few ulps of its terms below it: finite, and inside score_bound of the float64 value)
            assert (det > 0).all() and np.isfinite(d2).all() and np.isfinite(nll).all()
    print("parent score_gauss: wrong values per arrangement %s of %d" % (bad, total))
    assert bad["all_saturated"] > 0 and bad["first_saturated"] > 0 and bad["moderate"] == 0


def test_float32_score_model_is_finite_and_inside_the_bound():
    """The float32 ScoreModel against the float64 one (both with the floor) over the 14 pushes of both streams: every
    value and total finite, d2 and nll inside score_bound, the relative error of the floored determinant below 1/2."""
    case = de.score_case()
    thr = (1.386, 4.605, 9.21)
    cov64 = _covs(case, np.float64)
    worst = dict(d2=0.0, nll=0.0, r_d=0.0)
    scored = 0
    for s in range(case.ns):
        m32 = score_np.ScoreModel(case.p, case.v, case.k, thr, 64, None, np.float32)
        m64 = score_np.ScoreModel(case.p, case.v, case.k, thr, 64, None, np.float64)
        for m in range(case.n_push):
            ids, xy = case.detections(s, m)
            a, b = m32.push(ids, xy, case.preds[s, m]), m64.push(ids, xy, case.preds[s, m])
            assert np.array_equal(a["matched"], b["matched"])
            for name in score_np.FIELDS:
                assert np.isfinite(a[name]).all() and np.isfinite(b[name]).all(), (s, m, name)
            c = case.num_peds[s]
            for h in range(1, min(m, case.p) + 1):
                assert a["matched"][h - 1, :c].all() and not a["matched"][h - 1, c:].any()
                dx, dy = case.offsets(s, m - h, h)
                d2_b, nll_b, r_d = de.score_bound(cov64[s, m - h][h - 1, :c], dx, dy, b["d2"][h - 1, :c], case.p)
                e2 = np.abs(a["d2"][h - 1, :c].astype(np.float64) - b["d2"][h - 1, :c])
                en = np.abs(a["nll"][h - 1, :c].astype(np.float64) - b["nll"][h - 1, :c])
                assert (r_d < 0.5).all()
                assert (e2 <= d2_b).all(), (s, m, h, e2 / d2_b)
                assert (en <= nll_b).all(), (s, m, h, en / nll_b)
                worst = dict(d2=max(worst["d2"], float((e2 / d2_b).max())), nll=max(worst["nll"], float((en / nll_b).max())),
                             r_d=max(worst["r_d"], float(r_d.max())))
                scored += c
        assert np.isfinite(m32.totals).all() and np.isfinite(m32.traj_totals).all() and m32.traj_totals[0] > 0
    print("float32 score model, worst error / bound over %d elements: %s" % (scored, worst))
    assert scored == (8 + 5) * (sum(range(1, 13)) + 12)


def test_a_geometry_exists_that_the_reference_decides():
    """The radii and rectangles of the GPU risk test: with every pedestrian's allowance no count is undecided; at the
    first radius conflict counts lie strictly between 0 and K, at the second every count is K; the last rectangle holds
    every sample."""
    for i in (0, 1):
        for philox in (False, True):
            _, radii, zones, (want, whole) = de.risk_case(i, philox)
            k, peds = de.SAMPLES_K, np.array(SHAPES[i][3])
            mixed = int(((want["conflict"] > 0) & (want["conflict"] < k)).sum())
            print("risk geometry %s philox=%s: radii %g and %g, %d rectangles, %d mixed conflict counts"
                  % (SHAPES[i][:3], philox, radii[0], radii[1], len(zones), mixed))
            assert mixed > 0 and len(zones) >= 3
            assert np.array_equal(whole["conflict_any"], k * (de.valid(peds, SHAPES[i][2]) & (peds[:, None] > 1)))
            assert np.array_equal(want["zone_count"][:, :, -1], np.repeat(k * peds[:, None], SHAPES[i][1], axis=1))
            assert 0 < want["zone_count"][:, :, 0].sum() < want["zone_count"][:, :, -1].sum()
