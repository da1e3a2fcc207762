"""CPU: the risk entry point (stg_sample_risk) is declared, exported and refuses bad arguments without a GPU; the numpy
statement of its outputs (tests/risk_np.py) agrees with its own loop restatement; the Python options that need no
device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import risk_np


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_and_library_exports_sample_risk(L):
    from social_stgcnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    assert re.search(r"\bint\s+stg_sample_risk\s*\(", hdr)
    assert "stg_sample_risk" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "stg_sample_risk")
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8
    limits = {m: int(x) for m, x in re.findall(r"#define STG_RISK_MAX_(\w) (\d+)", hdr)}
    assert limits["V"] >= 256 and limits["K"] >= 64 and limits["Z"] >= 16 and limits["P"] >= 32
    from social_stgcnn_amd import ops
    assert (ops.RISK_MAX_V, ops.RISK_MAX_K, ops.RISK_MAX_Z, ops.RISK_MAX_P) == tuple(limits[m] for m in "VKZP")


def test_sample_risk_refuses_bad_arguments_without_a_gpu(L):
    from social_stgcnn_amd import ops
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call
    odd = ctypes.c_void_p(68)        # 4-byte but not 8-byte aligned

    def call(pred=f, obs_last=None, noise=None, n=2, p=12, v=4, k=3, radius=0.5, zones=f, z=2, conflict=f,
             conflict_any=f, partner=f, pair=f, zone_any=f, zone_count=f, ped_zone=f):
        return L.stg_sample_risk(pred, 1, 1, 1, 1, obs_last, None, noise, 0, None, n, p, v, k,
                                 ctypes.c_float(radius), zones, 0, z, conflict, conflict_any, partner, pair, zone_any,
                                 zone_count, ped_zone, None)
    einval = {"N<0": dict(n=-1), "P=0": dict(p=0), "V=0": dict(v=0), "V<0": dict(v=-2), "K=0": dict(k=0),
              "K<0": dict(k=-1), "Z<0": dict(z=-1), "pred NULL": dict(pred=None),
              "nothing asked": dict(radius=0.0, z=0), "negative radius, no zones": dict(radius=-1.0, z=0),
              "conflict NULL": dict(conflict=None), "conflict_any NULL": dict(conflict_any=None),
              "partner NULL": dict(partner=None), "zones NULL": dict(zones=None), "zone_any NULL": dict(zone_any=None),
              "zone_count NULL": dict(zone_count=None), "ped_zone NULL": dict(ped_zone=None),
              "noise unaligned": dict(noise=odd), "obs_last unaligned": dict(obs_last=odd)}
    for name, kw in einval.items():
        assert call(**kw) == -1, name
        assert b"stg_sample_risk" in L.stg_last_error(), name
    # beyond the limits: refused before any launch, the message names the limit
    for name, kw in {"V": dict(v=ops.RISK_MAX_V + 1), "K": dict(k=ops.RISK_MAX_K + 1), "Z": dict(z=ops.RISK_MAX_Z + 1),
                     "P": dict(p=ops.RISK_MAX_P + 1)}.items():
        assert call(**kw) == -2, name
        msg = L.stg_last_error()
        assert b"stg_sample_risk" in msg and ("STG_RISK_MAX_%s" % name).encode() in msg, msg
    # N == 0 is a no-op (nothing launched, so this runs without a GPU too)
    assert call(n=0, pred=None, conflict=None, zones=None) == 0


def test_python_options_refused_without_a_device():
    from social_stgcnn_amd.predict import Predictor, RiskSpec
    with pytest.raises(ValueError, match="keep_samples"):
        Predictor(None, 20, None, False)
    with pytest.raises(ValueError, match="radius or zones"):
        Predictor(None, 20, RiskSpec())
    pr = Predictor(None, 5, RiskSpec(0.5), keep_samples=False)
    assert pr.spec == RiskSpec(0.5, None, False) and pr.risk is None and not pr.keep_samples
    from social_stgcnn_amd.predict_frames import build_parser, parse_zones
    a = build_parser().parse_args(["--checkpoint", "c", "--recording", "r", "--out", "o", "--radius", "0.5", "--zones",
                                   "-1,-1,1,1", "0,0,4,3"])
    assert a.radius == 0.5 and np.array_equal(parse_zones(a.zones), np.array([[-1, -1, 1, 1], [0, 0, 4, 3]], np.float32))
    a = build_parser().parse_args(["--checkpoint", "c", "--recording", "r", "--out", "o"])
    assert a.radius is None and a.zones is None


def test_risk_np_agrees_with_its_loop_restatement():
    """2 scenes (one ragged), positions on a 1/4 grid so that distances of exactly the radius and samples exactly on
    the rectangle edges occur; an inverted rectangle; shared and per-scene rectangles."""
    rng = np.random.default_rng(5)
    k, n, p, v = 3, 2, 4, 6
    s = rng.integers(-6, 7, size=(k, n, p, v, 2)) / 4.0
    peds = np.array([6, 4])
    zones = np.array([[-0.5, -0.5, 0.75, 0.75], [0.0, -1.0, 1.5, 0.25], [1.0, 1.0, -1.0, -1.0]])
    per_scene = np.stack([zones, zones[::-1] + 0.25])
    d = s[:, :, :, :, None] - s[:, :, :, None]
    assert np.any((d ** 2).sum(-1) == 0.75 ** 2)                         # the strict < is exercised
    assert np.any(s[..., 0] == -0.5) and np.any(s[..., 0] == 0.75)
    for z in (zones, per_scene):
        for pd in (peds, None, np.array([9, -2])):
            a, b = risk_np.risk(s, pd, 0.75, z), risk_np.risk_loops(s, pd, 0.75, z)
            assert sorted(a) == sorted(b) == sorted(risk_np.CONFLICT + risk_np.ZONE)
            for name in a:
                assert np.array_equal(a[name], b[name]), name
    a = risk_np.risk(s, peds, 0.75, zones)
    assert a["conflict"].max() > 0 and a["zone_count"].max() > 1 and not a["zone_any"][:, :, 2].any()
    assert np.array_equal(a["pair"], np.swapaxes(a["pair"], 1, 2)) and not np.einsum("nii->ni", a["pair"]).any()
    assert not a["conflict"][1, :, 4:].any() and np.all(a["partner"][1, 4:] == -1)
    lo, hi = risk_np.bounds(s, peds, 0.75, zones, 1e-4)
    for name in risk_np.CONFLICT[:3] + risk_np.ZONE:
        assert np.all(lo[name] <= a[name]) and np.all(a[name] <= hi[name]), name
    only = risk_np.risk(s, peds, None, zones)
    assert sorted(only) == sorted(risk_np.ZONE)
