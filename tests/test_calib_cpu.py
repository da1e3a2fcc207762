"""CPU: the calibration of DESIGN.md 5.32.  The restatement tests/calib_np.py on its own -- the clamps, the recovery of
known factors, the two real-data rows of the design's table from the float64 CPU reference model --, the C ABI as
declared, bound, exported and refused before any launch, and the host side of the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import calib_np as cn
import dist_edges as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
F = np.float32


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_calib_header_its_binding_and_the_export(L):
    """include/stgcnn_hip_calib.h -- which stgcnn_hip.h includes behind the metrics header, inside its extern "C" block
    -- as _lib binds it from that header (tests/test_lib_cpu.py checks the binding of all eight): its three entry points
    by name, nothing but void * and four scalar types among their parameters; the constants of the header are those of
    ops and of the restatement; the ABI version 8."""
    from social_stgcnn_amd import _lib, ops
    main = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r'^#include "stgcnn_hip_calib.h"$', main, re.M)
    assert main.index('#include "stgcnn_hip_calib.h"') > main.index('#include "stgcnn_hip_metrics.h"') > \
        main.index('extern "C" {')
    assert re.search(r"#define STG_ABI_VERSION 8\b", main)
    raw_hdr = open(os.path.join(ROOT, "include", "stgcnn_hip_calib.h")).read()
    defs = dict(re.findall(r"^#define (STG_CALIB_[A-Z]+) (\d+)", raw_hdr, re.M))
    assert {k: int(x) for k, x in defs.items()} == {
        "STG_CALIB_MOMENT": ops.CALIB_MODES["moment"], "STG_CALIB_COVERAGE": ops.CALIB_MODES["coverage"],
        "STG_CALIB_LOW": ops.CALIB_LOW, "STG_CALIB_HIGH": ops.CALIB_HIGH, "STG_CALIB_EMPTY": ops.CALIB_EMPTY}
    assert (cn.MOMENT, cn.COVERAGE, cn.LOW, cn.HIGH, cn.EMPTY) == (0, 1, ops.CALIB_LOW, ops.CALIB_HIGH, ops.CALIB_EMPTY)
    protos = _lib.parse_header(raw_hdr)
    assert [p.name for p in protos] == ["stg_calib_fit_ws_bytes", "stg_calib_fit", "stg_calib_apply"]
    for p in protos:
        fn = getattr(L, p.name)
        assert _lib.PROTOTYPES[p.name] == p and len(fn.argtypes) == len(p.params), p.name
        assert set(fn.argtypes) <= {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_float}, p.name
        assert fn.restype == (ctypes.c_int64 if p.name == "stg_calib_fit_ws_bytes" else ctypes.c_int), p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


def test_the_entry_points_refuse_before_any_launch(L):
    """Every case fails validation before any HIP call: the pointers are never dereferenced."""
    from social_stgcnn_amd import _lib
    f = ctypes.c_void_p(64)
    need = L.stg_calib_fit_ws_bytes(2, 12, 5)
    assert need > 0 and need % 8 == 0 and L.stg_calib_fit_ws_bytes(0, 12, 5) >= 0
    # the partials of one workgroup, the element list and first[] of 2 x 5 slots, the search state
    assert need == 32 * 8 + 32 * 4 + 8 + 16 + 40 + 16

    def fit(n=2, p=12, v=5, mode=1, level=0.9, v_pred=f, mean=f, truth=f, g=f, bracket=f, flags=f, stats=f, sig=f, ws=f,
            ws_bytes=need):
        return L.stg_calib_fit(v_pred, 60 * v, 12 * v, v, 1, mean, truth, f, n, p, v, mode, level, g, bracket, flags,
                               stats, sig, ws, ws_bytes, None)
    einval = {"P=0": dict(p=0), "V=0": dict(v=0), "N<0": dict(n=-1), "mode 2": dict(mode=2), "mode -1": dict(mode=-1),
              "level 0": dict(level=0.0), "level 1": dict(level=1.0), "level nan": dict(level=float("nan")),
              "level < 0": dict(level=-0.5), "null v_pred": dict(v_pred=None), "null mean": dict(mean=None),
              "null truth": dict(truth=None), "null g": dict(g=None), "null bracket": dict(bracket=None),
              "null flags": dict(flags=None), "null stats": dict(stats=None), "null sig": dict(sig=None),
              "null ws": dict(ws=None), "small ws": dict(ws_bytes=need - 1), "misaligned mean": dict(mean=ctypes.c_void_p(68)),
              "misaligned truth": dict(truth=ctypes.c_void_p(68)), "misaligned ws": dict(ws=ctypes.c_void_p(68)),
              "misaligned stats": dict(stats=ctypes.c_void_p(68))}
    for name, kw in einval.items():
        assert fit(**kw) == -1, name
        assert b"stg_calib_fit" in L.stg_last_error(), name
    for name, kw in {"P": dict(p=33), "V": dict(v=257)}.items():
        assert fit(**kw) == _lib.EUNSUPPORTED, name
        assert (name + "=").encode() in L.stg_last_error() and b"STG_SCORE_MAX_" + name.encode() in L.stg_last_error()
        assert L.stg_calib_fit_ws_bytes(2, kw.get("p", 12), kw.get("v", 5)) == _lib.EUNSUPPORTED
    assert fit(n=1 << 23, v=256, ws_bytes=1 << 40) == _lib.EUNSUPPORTED and b"2^30" in L.stg_last_error()
    assert L.stg_calib_fit_ws_bytes(2, 0, 5) == -1
    assert fit(n=0) == 0 and fit(n=0, truth=None, ws=None, ws_bytes=0) == 0       # no scenes: nothing is launched
    assert fit(n=0, mode=7) == -1 and fit(n=0, v=257) == _lib.EUNSUPPORTED        # ... but the arguments are looked at

    def apply(n=2, p=12, v=5, v_pred=f, shift=f, out=None, o=(0, 0, 0, 0)):
        return L.stg_calib_apply(v_pred, 60 * v, 12 * v, v, 1, shift, n, p, v, out, *o, None)
    for name, kw in {"P=0": dict(p=0), "V=0": dict(v=0), "N<0": dict(n=-1), "null v_pred": dict(v_pred=None),
                     "null shift": dict(shift=None), "out is v_pred, other strides": dict(out=f, o=(300, 5, 25, 1))}.items():
        assert apply(**kw) == -1, name
        assert b"stg_calib_apply" in L.stg_last_error(), name
    assert apply(p=33) == _lib.EUNSUPPORTED and apply(v=257) == _lib.EUNSUPPORTED
    assert apply(n=0) == 0 and apply(n=0, v_pred=None) == 0


def test_ops_and_calibration_check_their_arguments(tmp_path):
    """Decided on the host ahead of any device work; a Calibration survives save / load bit for bit."""
    import torch
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.calibrate import Calibration
    assert ops.CalibFit._fields == ("g", "bracket", "flags", "stats", "sig")
    out, _ = ops.calib_buffers(2, 12, 5, "meta")
    assert [tuple(x.shape) for x in out] == [(12,), (12, 2), (12,), (12, 3), (2, 12, 5, 3)]
    assert (out.flags.dtype, out.stats.dtype) == (torch.int32, torch.float64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.calib_fit(torch.zeros(1, 5, 12, 3), torch.zeros(1, 12, 3, 2), torch.zeros(1, 12, 3, 2))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.calib_apply(torch.zeros(1, 5, 12, 3), torch.zeros(12))
    g = np.exp(np.random.default_rng(0).uniform(-3, 3, 12)).astype(F)
    c = Calibration(g, "moment", 0.5)
    assert np.array_equal(c.shift, cn.shift_of(g)) and c.shift.dtype == F
    assert np.array_equal(ops.calib_shift(torch.from_numpy(g)), c.shift)
    c.save(str(tmp_path / "calibration.npz"))
    with np.load(str(tmp_path / "calibration.npz")) as z:
        assert sorted(z.files) == ["g", "level", "mode"]
    d = Calibration.load(str(tmp_path / "calibration.npz"))
    assert np.array_equal(d.g, g) and (d.mode, d.level) == ("moment", 0.5) and np.array_equal(d.shift, c.shift)
    for bad in (dict(g=[1.0, 0.0]), dict(g=[1.0, -2.0]), dict(g=[np.inf]), dict(g=[1.0], mode="median"),
                dict(g=[1.0], level=1.0)):
        with pytest.raises(ValueError):
            Calibration(**bad)


def _synthetic(n, p, v, peds, seed, g_true=None):
    """A random prediction; the truth at horizon h drawn from N(mean_h, sum_{t<=h} g_true_t sig_t), float32 inputs."""
    rng = np.random.default_rng(seed)
    v_pred = rng.normal(0, 0.5, (n, 5, p, v)).astype(F)
    mean = np.cumsum(rng.normal(0, 0.4, (n, p, v, 2)), axis=1).astype(F)
    sig = cn.sig_terms(v_pred, np.float64)
    g_true = np.ones(p) if g_true is None else np.asarray(g_true, np.float64)
    cov = np.cumsum(sig * g_true[None, :, None, None], axis=1)
    l00 = np.sqrt(cov[..., 0])
    l10 = cov[..., 1] / l00
    l11 = np.sqrt(cov[..., 2] - l10 * l10)
    e = rng.standard_normal((n, p, v, 2))
    truth = mean + np.stack([l00 * e[..., 0], l10 * e[..., 0] + l11 * e[..., 1]], axis=-1)
    return v_pred, mean, truth.astype(F), peds


def test_kernel_sum_is_a_sum_in_the_documented_order():
    """169 and 630 terms (three waves, the last partial; three workgroups): within the order bound of math.fsum, and
    equal to the explicit loop over workgroups, waves and butterfly stages."""
    import math
    rng = np.random.default_rng(1)
    for e in (1, 64, 65, 169, 256, 257, 630):
        x = rng.chisquare(2, e)
        got = float(cn.kernel_sum(x))
        assert abs(got - math.fsum(x)) <= cn.order_bound(got, e) / 2 + 1e-300
        total = None
        for b in range(0, e, 256):
            wg = None
            for w in range(b, b + 256, 64):
                lanes = np.zeros(64)
                part = x[w:w + 64]
                lanes[:len(part)] = part
                for o in (32, 16, 8, 4, 2, 1):
                    lanes = lanes + lanes[np.arange(64) ^ o]
                wg = lanes[0] if wg is None else wg + lanes[0]
            total = wg if total is None else total + wg
        assert got == total
    assert cn.kernel_sum(np.zeros((3, 0))).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("mode", (cn.MOMENT, cn.COVERAGE))
def test_the_three_flags(mode):
    """truth == mean: every d2 is 0, 2^-10 is already ok -> LOW; the truth 1e4 sigma away: no candidate up to 2^21 is ok
    (d2 >= 1e8 / (12 2^21) > thr and > 2) -> HIGH; no pedestrians -> EMPTY, g = 1.  The float32 and the float64 rule
    agree."""
    v_pred, mean, truth, peds = _synthetic(3, 12, 5, (5, 2, 0), 0)
    sig = cn.sig_terms(v_pred)
    for dtype in (F, np.float64):
        r = cn.fit(sig, mean, mean, peds, mode, 0.9, dtype)
        assert (r["flags"] == cn.LOW).all() and (r["g"] == 2.0 ** -10).all() and (r["bracket"] == 2.0 ** -10).all()
        assert r["stats"].tolist() == [[7.0, 0.0, 7.0]] * 12
        far = mean + (1e4 * np.sqrt(12 * np.maximum(sig[..., 0], sig[..., 2]).max())).astype(F)
        r = cn.fit(sig, mean, far, peds, mode, 0.9, dtype)
        assert (r["flags"] == cn.HIGH).all() and (r["g"] == 2.0 ** 21).all() and (r["stats"][:, 2] == 0).all()
        r = cn.fit(sig, mean, truth, (0, 0, 0), mode, 0.9, dtype)
        assert (r["flags"] == cn.EMPTY).all() and (r["g"] == 1).all() and not r["stats"].any()
        r = cn.fit(sig, mean, truth, peds, mode, 0.9, dtype)
        # seven elements: a horizon whose predecessors came out large may find 2^-10 ok; elsewhere a proper bracket
        free = r["flags"] == 0
        assert free.any() and np.isin(r["flags"], (0, cn.LOW)).all() and (r["g"] == r["bracket"][:, 1]).all()
        assert (r["bracket"][free, 0] < r["g"][free]).all() and (r["stats"][:, 0] == 7).all()


def test_recovery_of_known_factors():
    """Truths drawn from N(mean, sum_t g*_t sig_t) with sig_t = w_t A_e -- one matrix A_e per element, scaled by w_t over
    the steps -- so that C_h = G_h A_e with G_h = sum_{t<=h} g_t w_t and d2_h = (G*_h / G_h) q, q chi-square with two
    degrees of freedom.  The moment fit solves mean d2 = 2: G_h = G*_h qbar_h / 2 up to the search's resolution, with
    qbar_h the mean of E independent q: relative deviation eps_h = qbar_h / 2 - 1 of standard deviation 1 / sqrt(E)
    (var q = 4).  Then g_h w_h = G_h - G_{h-1}, so
        |g_h - g*_h| <= (G*_h |eps_h| + G*_{h-1} |eps_{h-1}|) / w_h + res,   |eps| <= Z / sqrt(E) at Z = 5 sigma
    (a one-in-1.7e6 event per horizon).  res: the search returns the first ok candidate of a grid that three refinements
    of 32 steps make finer than 2^-15 of g_h (a bracket [lo, 2 lo] after round 0), and the float32 arithmetic moves a
    mean d2 by < 1e-5 relative (dist_edges.score_bound at these well-conditioned covariances): together 2^-14 (G*_h +
    G*_{h-1}) / w_h.  E = 4096 elements: |eps| <= 0.078."""
    n, p, v, z = 64, 6, 64, 5.0
    rng = np.random.default_rng(7)
    g_true = np.array([0.4, 1.0, 2.5, 6.0, 0.7, 12.0])
    w = np.array([1.0, 0.8, 1.3, 1.0, 2.0, 0.9])
    v_pred = np.zeros((n, 5, p, v), F)
    base = rng.normal(0, 0.5, (n, 3, v)).astype(F)
    # log sigma_t = base + 0.5 log w_t, the correlation constant over t: sig_t = w_t A_e up to float32 rounding
    v_pred[:, 2:4] = base[:, :2, None, :] + (0.5 * np.log(w)).astype(F)[None, None, :, None]
    v_pred[:, 4] = base[:, 2, None, :]
    mean = np.cumsum(rng.normal(0, 0.4, (n, p, v, 2)), axis=1).astype(F)
    sig = cn.sig_terms(v_pred, np.float64)
    cov = np.cumsum(sig * g_true[None, :, None, None], axis=1)
    l00 = np.sqrt(cov[..., 0])
    l10 = cov[..., 1] / l00
    l11 = np.sqrt(cov[..., 2] - l10 * l10)
    e = rng.standard_normal((n, p, v, 2))
    truth = (mean + np.stack([l00 * e[..., 0], l10 * e[..., 0] + l11 * e[..., 1]], axis=-1))
    # (the float32 rounding of the truth moves d2 by 1e-7 of the offset's length: inside res)
    r = cn.fit(sig.astype(F), mean, truth.astype(F), None, cn.MOMENT, 0.9, F)
    big_g = np.cumsum(g_true * w)
    prev = np.concatenate([[0.0], big_g[:-1]])
    eps = z / np.sqrt(n * v)
    tol = (eps + 2.0 ** -14) * (big_g + prev) / w
    print("g", r["g"], "g*", g_true, "tolerance", tol)
    assert not r["flags"].any() and (np.abs(r["g"] - g_true) <= tol).all(), (r["g"], tol)
    assert (tol < 0.35 * g_true.max()).all()
    # the coverage fit at any level recovers them too, more loosely: the empirical quantile of q at level L has standard
    # deviation sqrt(L (1 - L) / E) / f(thr), f the chi-square density 0.5 exp(-thr / 2) = (1 - L) / 2, relative to thr
    for level in (0.5, 0.9):
        thr = float(cn.threshold(level))
        eps_q = z * np.sqrt(level * (1 - level) / (n * v)) / (0.5 * (1 - level)) / thr
        r = cn.fit(sig.astype(F), mean, truth.astype(F), None, cn.COVERAGE, level, F)
        assert not r["flags"].any() and (np.abs(r["g"] - g_true) <= (eps_q + 2.0 ** -14) * (big_g + prev) / w).all(), r["g"]


@pytest.mark.parametrize("case", range(len(cn.CASES)))
def test_the_gpu_cases_are_decided_by_the_rule(case):
    """The inputs of test_gpu_calib.py's fit cases, with numpy's sig: 7, 169 and 630 elements as the issue counts them;
    at both levels the moment fit's |sum d2 - 2 count| exceeds the summation-order bound at every visited candidate by
    many orders of magnitude (so the device's own sig, a few ulp away, leaves the margin standing); no search ends at
    the upper clamp, some end at the lower one, so the GPU cases compare flagged horizons too."""
    base, mean, truth, peds = cn.case_inputs(case)
    n, p, v, _ = base.shape
    assert len(cn.live_index(peds, n, v)[0]) == (7, 7, 7, 169, 630)[case]
    sig = cn.sig_terms(base.transpose(0, 3, 1, 2))
    r = cn.fit(sig, mean, truth, peds, cn.MOMENT, 0.9)
    margin = cn.moment_margin(r)
    print("case", case, "g", r["g"], "margin", margin)
    assert margin > 1e-7 and np.isfinite(r["stats"]).all()
    for level in (0.5, 0.9):
        c = cn.fit(sig, mean, truth, peds, cn.COVERAGE, level)
        assert (c["stats"][:, 2] >= float(F(level)) * c["stats"][:, 0])[c["flags"] != cn.HIGH].all()
        assert np.isin(c["flags"], (0, cn.LOW)).all()
        if case == 4:
            # 630 elements: no clamp, and the first six factors -- each a sizeable part of its C_h -- are G_TRUE's within
            # a factor 1.5 (behind the drop from 14 to 0.3 a step is a sliver of C_h and its factor is loose)
            assert not c["flags"][:6].any() and not r["flags"].any()
            assert (np.abs(np.log(c["g"][:6] / cn.G_TRUE)) < np.log(1.5)).all(), c["g"]


def _windows(name, files=None):
    from social_stgcnn_amd import data
    return data.load_windows(os.path.join(DATA, name), 8, 12, 1, with_non_linear=False, files=files)


# the design's table: (weights, the set fitted on, its pedestrians in the first 300 windows, the test set, its pedestrians,
# uncalibrated coverage at 50 / 90 / 99 %, calibrated `moment`, calibrated `coverage` p = 0.9, (min, max) of g per mode)
ROWS = {
    "zara1": ("weights_zara1", ("eth_train", ["crowds_zara02_train.txt"]), 1200, ("zara1_test", None), 2253,
              (0.456, 0.759, 0.888), (0.687, 0.921, 0.967), (0.670, 0.914, 0.965), {"moment": (0.41, 12.0),
                                                                                    "coverage": (0.36, 10.5)}),
    "eth": ("weights_eth", ("eth_train", None), 1052, ("eth_test", None), 181,
            (0.156, 0.338, 0.516), (0.297, 0.576, 0.730), (0.281, 0.554, 0.706), {"moment": (1.03, 7.4),
                                                                                  "coverage": (1.04, 8.1)}),
}


@pytest.mark.parametrize("row", sorted(ROWS))
def test_the_real_data_rows_of_the_table(row):
    """The float64 rule on the float64 CPU reference model's predictions with the committed weights: the coverage of the
    test set before and after, to the table's three digits (half a unit of the last one), every factor strictly inside
    the clamps with flag 0, and the float32 rule fed the same sig finds the same factors.  The zara1 row is the input of
    the GPU tests' real-data case: by the reference alone its calibrated 90 % coverage lies inside their band
    |c - 0.90| <= 0.03."""
    weights, fit_on, fit_peds, test_on, test_peds, uncal, cal_moment, cal_cover, g_range = ROWS[row]
    fs = cn.reference_set(weights, _windows(*fit_on), 300)
    ts = cn.reference_set(weights, _windows(*test_on))
    assert int(fs[3].sum()) == fit_peds and int(ts[3].sum()) == test_peds and len(fs[3]) == 300
    levels = (0.5, 0.9, 0.99)
    sig_f, sig_t = cn.sig_terms(fs[0], np.float64), cn.sig_terms(ts[0], np.float64)
    got = cn.coverage(sig_t, ts[1], ts[2], ts[3], np.ones(12), levels)
    print(row, "uncalibrated", got)
    assert np.abs(got - uncal).max() <= 5.01e-4
    for mode, name, want in ((cn.MOMENT, "moment", cal_moment), (cn.COVERAGE, "coverage", cal_cover)):
        r = cn.fit(sig_f, fs[1], fs[2], fs[3], mode, 0.9, np.float64)
        got = cn.coverage(sig_t, ts[1], ts[2], ts[3], r["g"], levels)
        print(row, name, "g", r["g"], "coverage", got)
        assert not r["flags"].any() and (r["g"] > 2.0 ** -10).all() and (r["g"] < 2.0 ** 21).all()
        assert np.abs(got - want).max() <= 5.01e-4
        lo, hi = g_range[name]
        assert lo - 0.05 <= r["g"].min() <= lo + 0.05 and hi - 0.5 <= r["g"].max() <= hi + 0.5
        if row == "zara1":
            assert abs(got[1] - 0.90) <= 0.022                    # 0.014 / 0.021 of the band's 0.03
        r32 = cn.fit(sig_f.astype(F), fs[1], fs[2], fs[3], mode, 0.9, F)
        assert np.allclose(r32["g"], r["g"], rtol=2.0 ** -14, atol=0) and not r32["flags"].any()
