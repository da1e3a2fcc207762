"""The stand-alone op kernels at their edges (-m gpu): every host-side dispatch branch and in-kernel guard of
stg_adj_build, stg_spatial_agg_fwd/bwd, stg_conv_t_fwd/bwd, stg_nll_fwd/bwd, stg_optim_step, stg_sgd_step,
stg_weighted_sum and stg_gather_windows against the float64 references of tests/ops_ref.py (DESIGN 2.2 has the branch
table).  Two kinds of check for the linear ops:

  exact     small-integer inputs: every partial sum is exactly representable (test_ops_ref_cpu.py asserts the sum of
            absolute terms < 2^24 for these very inputs), so the kernel must equal the reference bit for bit --
            `np.array_equal`, no tolerance.  Padded slots of the inputs hold a sentinel, padded outputs are exactly 0.
  rounding  randn inputs: |got - ref| <= (K + 2) 2^-24 sum|a_i b_i| per output element, K terms; derived, not measured.
"""
import numpy as np
import pytest
import torch

import ops_ref as R

pytestmark = pytest.mark.gpu

WORST = {}          # measured worst errors, printed when the module is done (pytest -s): the numbers of DESIGN 2.2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield torch.device("cuda", 0)
    for key in sorted(WORST):
        print("worst %-28s %.3e" % (key, WORST[key]))


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _oracle():
    from oracle import stgcnn_oracle as O
    return O


def _np(t):
    return t.detach().cpu().numpy()


def _as_trainer_view(x, dev):
    """(N,C,T,V) values stored as (N,V,C,T): the permuted view the trainer hands the kernels"""
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().to(dev).permute(0, 2, 3, 1)


def _offset_by_one_float(a, dev):
    """the values of `a` in device memory 4 bytes past a 16-byte boundary"""
    buf = torch.empty(a.size + 5, device=dev, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def _assert_exact(got, ref, what):
    assert np.array_equal(got, ref), "%s: %d of %d elements differ from the exact result" % (
        what, int((np.asarray(got, dtype=np.float64) != ref).sum()), ref.size)


def _assert_rounding(got, ref, k, s, what):
    """|got - ref| <= (K + 2) 2^-24 S elementwise (k broadcastable to ref); where S = 0 the output is exactly 0"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = R.rounding_bound(k, s)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    _note("rounding/" + what.split(":")[0], ratio.max() if ratio.size else 0.0)
    assert (err <= bound).all(), "%s: error %.3e of bound at %s" % (
        what, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


def _status(rc):
    from social_stgcnn_amd import _lib
    return rc, _lib.lib().stg_last_error().decode()


# ------------------------------------------------------------------------------------------------
# spatial_agg
# ------------------------------------------------------------------------------------------------
def _run_agg(case, x, adj, dy, dev):
    """(y, dx) of the kernels: through ops.spatial_agg, or the C ABI where the case misaligns an operand"""
    from social_stgcnn_amd import _lib, ops
    peds = case["peds"]
    xd = _as_trainer_view(x, dev)
    if "offset" not in case:
        xd.requires_grad_(True)
        y = ops.spatial_agg(xd, torch.from_numpy(adj).to(dev), peds)
        y.backward(torch.from_numpy(dy).to(dev))
        return _np(y), _np(xd.grad)
    n, c, t, v = x.shape
    ad = _offset_by_one_float(adj, dev) if case["offset"] == "adj" else torch.from_numpy(adj).to(dev)
    dyd = _offset_by_one_float(dy, dev) if case["offset"] == "dy" else torch.from_numpy(dy).to(dev)
    pd = _lib.peds_arg(peds, n, dev)
    y, dx = torch.full((n, c, t, v), np.nan, device=dev), torch.full((n, c, t, v), np.nan, device=dev)
    sn, sc, st, sv = xd.stride()
    L, P = _lib.lib(), _lib.ptr
    _lib.check(L.stg_spatial_agg_fwd(P(xd), sn, sc, st, sv, P(ad), t * v * v, P(pd), n, c, t, v, P(y), _lib.stream_ptr()),
               "stg_spatial_agg_fwd")
    _lib.check(L.stg_spatial_agg_bwd(P(dyd), P(ad), t * v * v, P(pd), n, c, t, v, P(dx), _lib.stream_ptr()),
               "stg_spatial_agg_bwd")
    return _np(y), _np(dx)


@pytest.mark.parametrize("case", R.AGG_CASES, ids=lambda c: c["id"])
def test_spatial_agg_exact(dev, case):
    x, adj, dy = R.agg_inputs(case, integer=True)
    y, dx = _run_agg(case, x, adj, dy, dev)
    _assert_exact(y, R.agg_fwd(x, adj, case["peds"]), "y")
    _assert_exact(dx, R.agg_dx(dy, adj, case["peds"]), "dx")
    for n, p in enumerate(R.clamp_peds(case["peds"], case["n"], case["v"])):
        assert not y[n, :, :, p:].any() and not dx[n, :, :, p:].any()


@pytest.mark.parametrize("case", R.AGG_CASES, ids=lambda c: c["id"])
def test_spatial_agg_rounding(dev, case):
    x, adj, dy = R.agg_inputs(case, integer=False)
    y, dx = _run_agg(case, x, adj, dy, dev)
    peds = case["peds"]
    k = R.clamp_peds(peds, case["n"], case["v"])[:, None, None, None]          # terms: the scene's valid pedestrians
    _assert_rounding(y, R.agg_fwd(x, adj, peds), k, R.agg_fwd(np.abs(x), np.abs(adj), peds), "agg_y: " + case["id"])
    _assert_rounding(dx, R.agg_dx(dy, adj, peds), k, R.agg_dx(np.abs(dy), np.abs(adj), peds), "agg_dx: " + case["id"])


def test_spatial_agg_refuses_more_than_160k_of_lds(dev):
    from social_stgcnn_amd import _lib
    c = R.AGG_REFUSED
    x = torch.zeros(c["n"], c["c"], c["t"], c["v"], device=dev)
    adj = torch.zeros(c["t"], c["v"], c["v"], device=dev)
    y = torch.zeros_like(x)
    L, P = _lib.lib(), _lib.ptr
    rc, msg = _status(L.stg_spatial_agg_fwd(P(x), *x.stride(), P(adj), 0, None, c["n"], c["c"], c["t"], c["v"], P(y),
                                            _lib.stream_ptr()))
    assert rc == -3 and "exceed LDS" in msg                    # STG_ELDS
    rc, msg = _status(L.stg_spatial_agg_bwd(P(x), P(adj), 0, None, c["n"], c["c"], c["t"], c["v"], P(y), _lib.stream_ptr()))
    assert rc == -3 and "exceed LDS" in msg


# ------------------------------------------------------------------------------------------------
# conv_t
# ------------------------------------------------------------------------------------------------
def _run_conv(case, x, w, b, dy, dev):
    """y, dx (None when x needs no gradient), dw, db (None without bias) through ops.conv_t"""
    from social_stgcnn_amd import ops
    xd = _as_trainer_view(x, dev) if case.get("strided") else torch.from_numpy(x).to(dev)
    xd.requires_grad_(case.get("need_dx", True))
    wd = torch.from_numpy(w).to(dev).requires_grad_(True)
    bd = torch.from_numpy(b).to(dev).requires_grad_(True) if b is not None else None
    y = ops.conv_t(xd, wd, bd, case["pad"], case["peds"])
    y.backward(torch.from_numpy(dy).to(dev))
    return (_np(y), _np(xd.grad) if xd.grad is not None else None, _np(wd.grad)[..., 0],
            _np(bd.grad) if bd is not None else None)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c["id"])
def test_conv_t_exact(dev, case):
    x, w, b, dy = R.conv_inputs(case, integer=True)
    y, dx, dw, db = _run_conv(case, x, w, b, dy, dev)
    peds = case["peds"]
    rdx, rdw, rdb = R.conv_bwd(x, w, dy, case["pad"], peds)
    _assert_exact(y, R.conv_fwd(x, w, b, case["pad"], peds), "y")
    _assert_exact(dw, rdw, "dw")
    assert (dx is None) == (not case.get("need_dx", True)) and (db is None) == (not case["bias"])
    if dx is not None:
        _assert_exact(dx, rdx, "dx")
    if db is not None:
        _assert_exact(db, rdb, "db")
    for n, p in enumerate(R.clamp_peds(peds, case["n"], case["v"])[:12]):
        assert not y[n, :, :, p:].any() and (dx is None or not dx[n, :, :, p:].any())


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c["id"])
def test_conv_t_rounding(dev, case):
    x, w, b, dy = R.conv_inputs(case, integer=False)
    y, dx, dw, db = _run_conv(case, x, w, b, dy, dev)
    peds, pad = case["peds"], case["pad"]
    rdx, rdw, rdb = R.conv_bwd(x, w, dy, pad, peds)
    sdx, sdw, sdb = R.conv_bwd(np.abs(x), np.abs(w), np.abs(dy), pad, peds)
    sy = R.conv_fwd(np.abs(x), np.abs(w), None if b is None else np.abs(b), pad, peds)
    k = R.conv_terms(int(R.clamp_peds(peds, case["n"], case["v"]).sum()), case["cin"], case["cout"], case["t"], case["kt"], pad)
    _assert_rounding(y, R.conv_fwd(x, w, b, pad, peds), k["y"], sy, "conv_y: " + case["id"])
    if dx is not None:
        _assert_rounding(dx, rdx, k["dx"], sdx, "conv_dx: " + case["id"])
    if k["dw"] <= 1024:                                        # beyond that the worst-case bound says little
        _assert_rounding(dw, rdw, k["dw"], sdw, "conv_dw: " + case["id"])
        if db is not None:
            _assert_rounding(db, rdb, k["db"], sdb, "conv_db: " + case["id"])


def _conv_abi(case, x, w, dy, dev, dw, db):
    """stg_conv_t_bwd through the C ABI, without dx, into the caller's dw / db; returns the status"""
    from social_stgcnn_amd import _lib
    xd, wd, dyd = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    pd = _lib.peds_arg(case.get("peds"), x.shape[0], dev)
    P = _lib.ptr
    return _lib.lib().stg_conv_t_bwd(P(xd), *xd.stride(), P(wd), P(dyd), P(pd), x.shape[0], w.shape[1], w.shape[0],
                                     x.shape[2], x.shape[3], w.shape[2], case["pad"], None, P(dw), P(db), _lib.stream_ptr())


def test_conv_t_dw_accumulates_into_the_callers_buffer(dev):
    """stg_conv_t_bwd adds to dw / db (the autograd wrapper zeroes them): two calls leave twice the exact value"""
    from social_stgcnn_amd import _lib
    case = R.conv_case("kt3_same")
    x, w, b, dy = R.conv_inputs(case, integer=True)
    dw, db = torch.zeros(w.shape, device=dev), torch.zeros(w.shape[0], device=dev)
    for _ in range(2):
        _lib.check(_conv_abi(case, x, w, dy, dev, dw, db), "stg_conv_t_bwd")
    _, rdw, rdb = R.conv_bwd(x, w, dy, case["pad"], case["peds"])
    _assert_exact(_np(dw)[..., 0], 2 * rdw, "dw")
    _assert_exact(_np(db), 2 * rdb, "db")


@pytest.mark.parametrize("shape", R.CONV_REFUSED, ids=lambda s: "w%d" % (s["cin"] * s["cout"] * s["kt"]))
def test_conv_t_bwd_refuses_what_its_accumulators_cannot_hold(dev, shape):
    x = np.zeros((1, shape["cin"], 4, 3), dtype=np.float32)
    w = np.zeros((shape["cout"], shape["cin"], shape["kt"], 1), dtype=np.float32)
    dy = np.zeros((1, shape["cout"], 4, 3), dtype=np.float32)
    dw, db = torch.full(w.shape, 5.0, device=dev), torch.full((shape["cout"],), 5.0, device=dev)
    rc, msg = _status(_conv_abi(dict(pad=0), x, w, dy, dev, dw, db))
    assert rc == -2 and "not supported" in msg                  # STG_EUNSUPPORTED, before any launch
    assert bool((dw == 5).all()) and bool((db == 5).all())


# ------------------------------------------------------------------------------------------------
# ConvTemporalGraphical: conv_t then spatial_agg, forward and backward, against the two references chained
# ------------------------------------------------------------------------------------------------
def _run_module(x, w, b, adj, dy, dev):
    from social_stgcnn_amd.model import ConvTemporalGraphical
    c = R.MODULE_CASE
    m = ConvTemporalGraphical(c["cin"], c["cout"], adj.shape[1], t_kernel_size=c["kt"], t_padding=c["pad"]).to(dev)
    with torch.no_grad():
        m.conv.weight.copy_(torch.from_numpy(w))
        m.conv.bias.copy_(torch.from_numpy(b))
    xd = _as_trainer_view(x, dev).requires_grad_(True)
    ad = torch.from_numpy(adj).to(dev)
    y, a_out = m(xd, ad, c["peds"])
    assert a_out is ad and y.is_contiguous()
    y.backward(torch.from_numpy(dy).to(dev))
    return dict(y=_np(y), dx=_np(xd.grad), dw=_np(m.conv.weight.grad)[..., 0], db=_np(m.conv.bias.grad))


def test_conv_temporal_graphical_exact(dev):
    args = R.module_inputs(integer=True)
    got, ref = _run_module(*args, dev), R.module_ref(*args)
    for key in ("y", "dx", "dw", "db"):
        _assert_exact(got[key], ref[key], key)


def test_conv_temporal_graphical_rounding(dev):
    """Chained bound: the second op sees the first one's rounded result, h' = h + e with |e| <= B1 (the first op's
    bound), so its error is at most (K2 + 2) u S2(|h| + B1) from its own sum plus S2(B1) carried through."""
    x, w, b, adj, dy = R.module_inputs(integer=False)
    c = R.MODULE_CASE
    peds, pad = c["peds"], c["pad"]
    got, ref = _run_module(x, w, b, adj, dy, dev), R.module_ref(x, w, b, adj, dy)
    ax, aw, ab, aa, ady = (np.abs(a) for a in (x, w, b, adj, dy))
    pk = R.clamp_peds(peds, c["n"], c["v"])
    k1 = R.conv_terms(int(pk.sum()), c["cin"], c["cout"], c["t"], c["kt"], pad)
    k2 = pk[:, None, None, None]
    # forward: conv, then the einsum over its rounded output
    b_h = R.rounding_bound(k1["y"], R.conv_fwd(ax, aw, ab, pad, peds))
    bound_y = R.rounding_bound(k2, R.agg_fwd(np.abs(ref["h"]) + b_h, aa, peds)) + R.agg_fwd(b_h, aa, peds)
    # backward: the einsum's dx, then the three convolution gradients over its rounded output
    b_dh = R.rounding_bound(k2, R.agg_dx(ady, aa, peds))
    s = R.conv_bwd(ax, aw, np.abs(ref["dh"]) + b_dh, pad, peds)
    carried = R.conv_bwd(ax, aw, b_dh, pad, peds)
    bounds = dict(y=bound_y, dx=R.rounding_bound(k1["dx"], s[0]) + carried[0],
                  dw=R.rounding_bound(k1["dw"], s[1]) + carried[1], db=R.rounding_bound(k1["db"], s[2]) + carried[2])
    for key in ("y", "dx", "dw", "db"):
        err = np.abs(got[key].astype(np.float64) - ref[key])
        _note("rounding/module_" + key, np.max(np.divide(err, bounds[key], out=np.zeros_like(err), where=bounds[key] > 0)))
        assert (err <= bounds[key]).all(), key


# ------------------------------------------------------------------------------------------------
# adj_build
# ------------------------------------------------------------------------------------------------
# (id, N, V, T, permuted strides): the six distinct ragged scenes are tiled to N where N picks the kernel
ADJ_CASES = [
    ("v1_t1", 6, 1, 1, False),                  # tile kernel, scalar stores
    ("v2_t8", 6, 2, 8, True),
    ("v31_t12", 6, 31, 12, False),              # T = 12: the reference's target-graph length
    ("v33_t8", 6, 33, 8, True),
    ("v64_t12", 6, 64, 12, False),              # tile kernel, 16-byte stores, 16 chunks on 16 lanes
    ("v100_t1", 6, 100, 1, True),               # 25 chunks on 32 lanes
    ("v130_t8", 6, 130, 8, False),
    ("v32_t8", 6, 32, 8, False),                # rows32<256>, one pass
    ("v32_t12", 6, 32, 12, True),               # rows32: T V = 384, a full pass and half of one (`live_row`)
    ("v32_t20", 6, 32, 20, False),              # three passes, the last half live
    ("v32_t27", 6, 32, 27, True),               # four passes, the last 96 rows live
    ("v32_t8_n2048", 2048, 32, 8, False),       # rows32<256> at its last batch size
    ("v32_t20_n2049", 2049, 32, 20, True),      # rows32<128>: two phases per pass, multi-pass
    ("v33_t8_n1023", 1023, 33, 8, False),       # the tile kernel's last batch size
    ("v33_t8_n1024", 1024, 33, 8, False),       # per-scene kernel, scalar stores
    ("v64_t12_n1024", 1024, 64, 12, True),      # per-scene kernel, 16-byte stores
    ("v100_t8_n1025", 1025, 100, 8, False),     # 25 chunks on 32 lanes: rows_per_pass = 8 does not divide V
    ("v130_t1_n1024", 1024, 130, 1, True),
    ("v2_t27_n1024", 1024, 2, 27, False),
    ("v1_t12_n1024", 1024, 1, 12, False),
]


def _adj_scenes(v, t):
    peds = R.ragged_counts(v)
    rel = R.adj_rel(np.random.default_rng([v, t]), 6, v, t)
    R.fill_padding(rel, peds, axes=(1,))
    return rel, peds


@pytest.mark.parametrize("name,n,v,t,permuted", ADJ_CASES, ids=[c[0] for c in ADJ_CASES])
def test_adj_build_normalised_and_raw(dev, name, n, v, t, permuted):
    from social_stgcnn_amd import ops
    O = _oracle()
    rel6, peds6 = _adj_scenes(v, t)
    which = torch.arange(n) % 6
    rel = torch.from_numpy(rel6)[which]                                         # (N,V,2,T), dense
    if permuted:
        rel = rel.permute(0, 3, 1, 2).contiguous().to(dev).permute(0, 2, 3, 1)  # stored (N,T,V,2)
        assert t == 1 or not rel.is_contiguous()                 # (at T = 1 the two layouts coincide)
    else:
        rel = rel.to(dev)
    peds = [peds6[i % 6] for i in range(n)]
    pk = R.clamp_peds(peds6, 6, v)
    for normalize in (True, False):
        nodes, adj = ops.adj_build(rel, num_peds=peds, normalize=normalize)
        if n > 6:       # every tiled copy equals the first six scenes, on the device
            assert torch.equal(adj, adj[:6][which.to(dev)]) and torch.equal(nodes, nodes[:6][which.to(dev)])
        if normalize:
            assert torch.equal(adj, adj.transpose(-1, -2)), "L is not bitwise symmetric"
        nodes, adj = _np(nodes[:6]), _np(adj[:6])
        for i, p in enumerate(pk):
            assert not adj[i, :, p:, :].any() and not adj[i, :, :, p:].any() and not nodes[i, :, p:].any()
            if p == 0:
                continue
            ref_nodes, ref_lap = O.seq_to_graph_np(rel6[i, :p])
            assert np.array_equal(nodes[i, :, :p], ref_nodes)
            got = adj[i, :, :p, :p].astype(np.float64)
            if normalize:
                _note("adj/normalised_abs", np.abs(got - ref_lap).max())
                assert np.abs(got - ref_lap).max() < 1e-6
            else:
                raw = R.adj_raw(rel6[i, :p])
                diag = np.eye(p, dtype=bool)[None].repeat(t, 0)
                assert np.array_equal(got[diag], raw[diag]) and (got[diag] == 1).all()
                assert np.array_equal(got == 0, raw == 0)                       # coincident pedestrians: no edge
                nz = raw != 0
                rel_err = np.abs(got[nz] - raw[nz]) / raw[nz]
                _note("adj/raw_rel_ulp24", rel_err.max() / R.U)
                # 2 roundings of s on each side, halved by the root, + 1 ulp of v_rsq_f32 + the final fp32 rounding
                assert rel_err.max() <= 8 * R.U


# ------------------------------------------------------------------------------------------------
# nll
# ------------------------------------------------------------------------------------------------
def _nll_inputs(p, v, wide):
    """pred (6,P,V,5), target (6,P,V,2), per-scene weights; ragged counts -1, 0, 1, V-1, V, V+2.  Today's draw
    (randn * 0.5) with one clamp-active and one NaN element, or the wide draw: log sigma in [-3, 3], correlation logit
    in [-4, 4], the target drawn from the predicted distribution itself (|z-score| of a few units, so
    -log pdf <= 25 + log(2 pi e^6) = 33 < -log 1e-20 = 46: the clamp is never near)."""
    rng = np.random.default_rng([p, v, int(wide)])
    n, peds = 6, R.ragged_counts(v)
    if wide:
        pred = rng.standard_normal((n, p, v, 5))
        pred[..., 2:4] = rng.uniform(-3, 3, size=(n, p, v, 2))
        pred[..., 4] = rng.uniform(-4, 4, size=(n, p, v))
        pred = pred.astype(np.float32)
        p64 = pred.astype(np.float64)
        sx, sy, rho = np.exp(p64[..., 2]), np.exp(p64[..., 3]), np.tanh(p64[..., 4])
        u, w = np.clip(rng.standard_normal((2, n, p, v)), -4, 4)
        tgt = np.stack([p64[..., 0] + sx * u, p64[..., 1] + sy * (rho * u + np.sqrt(1 - rho ** 2) * w)], -1).astype(np.float32)
    else:
        pred = (0.5 * rng.standard_normal((n, p, v, 5))).astype(np.float32)
        tgt = rng.standard_normal((n, p, v, 2)).astype(np.float32)
        tgt[4, 0, 0] = 100.0                     # pdf < 1e-20: the clamp is active, zero gradient (scene 4 has V pedestrians)
        pred[5, p - 1, v - 1, 4] = 20.0          # tanh saturates: 1 - rho^2 = 0, NaN loss and NaN gradient for that element
    R.fill_padding(pred, peds, axes=(2,))
    R.fill_padding(tgt, peds, axes=(2,))
    wts = np.array([0.3, 1.0, 2.0, -0.5, 1.5, 0.7], dtype=np.float32)
    return pred, tgt, peds, wts


def _nll_oracle(pred, tgt, peds, wts, dtype):
    """per-scene losses and d(sum_n w_n loss_n)/dpred of oracle.bivariate_loss in `dtype`; an empty scene has loss 0"""
    O = _oracle()
    pr = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    tg = torch.from_numpy(tgt).to(dtype)
    pk = R.clamp_peds(peds, pred.shape[0], pred.shape[2])
    losses = [O.bivariate_loss(pr[i, :, :k], tg[i, :, :k]) if k else pr.new_zeros(()) for i, k in enumerate(pk)]
    (torch.stack(losses) * torch.from_numpy(wts).to(dtype)).sum().backward()
    return torch.stack(losses).detach().double().numpy(), pr.grad.double().numpy()


def _nll_kernels(pred, tgt, peds, wts, strided, dev):
    """[(losses, gradient (N,P,V,5))] of the two routes to the kernel: autograd (stg_nll_fwd, then stg_nll_bwd with
    the upstream gradient) and the trainer's (stg_nll_fwd with grad_scale)"""
    from social_stgcnn_amd import ops
    from social_stgcnn_amd.metrics import bivariate_loss
    tg, wd = torch.from_numpy(tgt).to(dev), torch.from_numpy(wts).to(dev)
    if strided:
        store = torch.from_numpy(pred).permute(0, 3, 1, 2).contiguous().to(dev).requires_grad_(True)     # (N,5,P,V)
        view = store.permute(0, 2, 3, 1)
    else:
        store = torch.from_numpy(pred).to(dev).requires_grad_(True)
        view = store
    out = bivariate_loss(view, tg, peds)
    (out * wd).sum().backward()
    g1 = _np(store.grad.permute(0, 2, 3, 1) if strided else store.grad)
    y = view.detach().permute(0, 3, 1, 2)            # (N,5,P,V): contiguous when `strided`, a permuted view otherwise
    l2, g2 = ops.bivariate_nll_with_grad(y, tg, peds, wd)
    return [(_np(out), g1), (_np(l2), _np(g2.permute(0, 2, 3, 1)))]


def _nll_errors(loss, grad, ref_loss, ref_grad):
    """the asserted metrics: per-scene loss error / max(1, |ref|), gradient error / max(1, max |ref|); NaNs must coincide"""
    assert np.array_equal(np.isnan(loss), np.isnan(ref_loss)) and np.array_equal(np.isnan(grad), np.isnan(ref_grad))
    ok_l, ok_g = ~np.isnan(ref_loss), ~np.isnan(ref_grad)
    e_l = np.max(np.abs(loss[ok_l] - ref_loss[ok_l]) / np.maximum(1.0, np.abs(ref_loss[ok_l])))
    e_g = np.max(np.abs(grad[ok_g] - ref_grad[ok_g])) / max(1.0, np.abs(ref_grad[ok_g]).max())
    return float(e_l), float(e_g)


@pytest.mark.parametrize("p", (1, 12, 30))
@pytest.mark.parametrize("v", (1, 9, 57, 130))
def test_nll_todays_draw(dev, p, v):
    pred, tgt, peds, wts = _nll_inputs(p, v, wide=False)
    ref_loss, ref_grad = _nll_oracle(pred, tgt, peds, wts, torch.float64)
    pk = R.clamp_peds(peds, 6, v)
    assert np.isnan(ref_loss[5]) and np.isnan(ref_grad).sum() == 5 and not ref_grad[4, 0, 0].any()
    for loss, grad in _nll_kernels(pred, tgt, peds, wts, strided=(p + v) % 2 == 1, dev=dev):
        e_l, e_g = _nll_errors(loss.astype(np.float64), grad.astype(np.float64), ref_loss, ref_grad)
        _note("nll/today_loss", e_l)
        _note("nll/today_grad", e_g)
        assert e_l < 2e-6 and e_g < 2e-6
        assert not grad[4, 0, 0].any()                                          # clamp active: exactly zero
        for i, k in enumerate(pk):
            assert not grad[i, :, k:].any()                                     # padded slots: exactly zero
        assert loss[0] == 0 and loss[1] == 0                                    # empty scenes


@pytest.mark.parametrize("p,v", [(12, 57), (30, 130), (1, 9)])
def test_nll_wide_draw(dev, p, v):
    """log sigma in [-3, 3], correlation logit in [-4, 4]: the fp32 conditioning is measured, on the CPU, as the
    distance of the oracle run in fp32 from the oracle in fp64; the kernel gets 4 x that (libm against device
    transcendentals; nll_elem has no fma).  Never calibrated on the kernel's output."""
    pred, tgt, peds, wts = _nll_inputs(p, v, wide=True)
    ref_loss, ref_grad = _nll_oracle(pred, tgt, peds, wts, torch.float64)
    l32, g32 = _nll_oracle(pred, tgt, peds, wts, torch.float32)
    o_l, o_g = _nll_errors(l32, g32, ref_loss, ref_grad)
    assert np.isfinite(ref_loss).all() and np.isfinite(ref_grad).all()
    for loss, grad in _nll_kernels(pred, tgt, peds, wts, strided=True, dev=dev):
        e_l, e_g = _nll_errors(loss.astype(np.float64), grad.astype(np.float64), ref_loss, ref_grad)
        print("nll wide P=%d V=%d: loss %.3e (fp32 oracle %.3e)  grad %.3e (fp32 oracle %.3e)" % (p, v, e_l, o_l, e_g, o_g))
        _note("nll/wide_loss_over_fp32_oracle", e_l / o_l)
        _note("nll/wide_grad_over_fp32_oracle", e_g / o_g)
        _note("nll/wide_loss", e_l)
        _note("nll/wide_grad", e_g)
        _note("nll/wide_loss_fp32_oracle", o_l)
        _note("nll/wide_grad_fp32_oracle", o_g)
        assert e_l <= 4 * o_l and e_g <= 4 * o_g


# ------------------------------------------------------------------------------------------------
# optim_step / sgd_step / weighted_sum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", (None, 0.05, 1e6), ids=("noclip", "clip", "hugeclip"))
@pytest.mark.parametrize("count", R.COUNTS)
def test_optim_step_against_fp64_clip_and_sgd(dev, count, max_norm):
    """counts below / at / above one wave, 8192 = the last of the one-trip register branch, 8193 and 50000 the streaming
    branch; lr from the device and from the host"""
    from social_stgcnn_amd import ops
    p0, g0 = R.flat_inputs(count, integer=False)
    ref_p, ref_g, ref_norm = R.clip_sgd(p0, g0, 0.01, max_norm)
    for use_dev_lr in (True, False):
        p, g = torch.from_numpy(p0).to(dev), torch.from_numpy(g0).to(dev)
        nrm = torch.full((1,), -1.0, device=dev)
        lr_dev = torch.full((1,), 0.01, device=dev) if use_dev_lr else None
        ops.optim_step(p, g, lr=123.0 if use_dev_lr else 0.01, max_norm=max_norm, lr_dev=lr_dev, grad_norm=nrm)
        _note("optim/norm_rel", abs(float(nrm) - ref_norm) / ref_norm)
        _note("optim/param_abs", np.abs(_np(p) - ref_p).max())
        assert abs(float(nrm) - ref_norm) <= 1e-6 * ref_norm
        assert np.abs(_np(p) - ref_p).max() <= 5e-7
        # g' = g coef: the norm inside coef is within 1e-6 (above), the add, the division and the product round once each
        assert (np.abs(_np(g) - ref_g) <= 2e-6 * np.abs(ref_g)).all()
        if max_norm is None or max_norm > 1:
            assert np.array_equal(_np(g), g0)                                   # no clipping: the gradient is untouched
    # without a norm to report and without clipping the reduction is skipped altogether
    p = torch.from_numpy(p0).to(dev)
    ops.optim_step(p, torch.from_numpy(g0).to(dev), lr=0.01)
    assert np.abs(_np(p) - R.clip_sgd(p0, g0, 0.01)[0]).max() <= 5e-7


@pytest.mark.parametrize("count", R.COUNTS)
def test_optim_and_sgd_step_exact(dev, count):
    """integer parameters and gradients, power-of-two lr, no clipping: p - lr g is exact, with or without fma"""
    from social_stgcnn_amd import ops
    p0, g0 = R.flat_inputs(count, integer=True)
    for lr in (0.25, 4.0):
        ref = R.clip_sgd(p0, g0, lr)[0]
        p, g = torch.from_numpy(p0).to(dev), torch.from_numpy(g0).to(dev)
        nrm = torch.full((1,), -1.0, device=dev)
        ops.optim_step(p, g, lr=99.0, lr_dev=torch.full((1,), lr, device=dev), grad_norm=nrm)
        _assert_exact(_np(p), ref, "optim_step")
        assert np.array_equal(_np(g), g0)
        assert float(nrm) == np.float32(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))   # exact sum, correctly rounded root
        p = torch.from_numpy(p0).to(dev)
        ops.sgd_step(p, g, lr)
        _assert_exact(_np(p), ref, "sgd_step")
        # a huge max_norm turns the clip path on with coefficient exactly 1
        p = torch.from_numpy(p0).to(dev)
        ops.optim_step(p, g, lr=lr, max_norm=1e9)
        _assert_exact(_np(p), ref, "optim_step, coef 1")
        assert np.array_equal(_np(g), g0)


@pytest.mark.parametrize("count", R.COUNTS)
def test_sgd_step_rounding_and_zero_gradient_clip(dev, count):
    from social_stgcnn_amd import ops
    p0, g0 = R.flat_inputs(count, integer=False)
    p = torch.from_numpy(p0).to(dev)
    ops.sgd_step(p, torch.from_numpy(g0).to(dev), 0.01)
    assert np.abs(_np(p) - R.clip_sgd(p0, g0, 0.01)[0]).max() <= 5e-7
    # an all-zero gradient with clipping on: max_norm / (0 + 1e-6) clamps to 1; nothing moves, nothing becomes NaN
    p, g = torch.from_numpy(p0).to(dev), torch.zeros(count, device=dev)
    nrm = torch.full((1,), -1.0, device=dev)
    ops.optim_step(p, g, lr=0.01, max_norm=0.05, grad_norm=nrm)
    assert np.array_equal(_np(p), p0) and not _np(g).any() and float(nrm) == 0.0


@pytest.mark.parametrize("weighted", (True, False), ids=("weights", "plain"))
@pytest.mark.parametrize("n", R.WSUM_NS)
def test_weighted_sum(dev, n, weighted):
    from social_stgcnn_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    for integer in (True, False):
        v, w = R.flat_inputs(n, integer)
        vd, wd = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev)
        if n == 0:                      # an empty torch tensor has no address: any valid pointer, zero elements
            vd = wd = torch.zeros(1, device=dev)
        out = torch.full((1,), np.nan, device=dev)
        _lib.check(L.stg_weighted_sum(P(vd), P(wd) if weighted else None, n, P(out), _lib.stream_ptr()), "stg_weighted_sum")
        ref = R.weighted_sum(v, w if weighted else None)
        if integer:
            assert float(out) == ref
        else:
            s = R.weighted_sum(np.abs(v), np.abs(w) if weighted else None)
            assert abs(float(out) - ref) <= R.rounding_bound(n, s)


# ------------------------------------------------------------------------------------------------
# gather_windows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_pred", (12, 0))
@pytest.mark.parametrize("index", ([-3, 14, 1, 2, 4, 8, 0, 6], None), ids=("indexed", "in_order"))
def test_gather_windows_exact(dev, index, t_pred):
    """V = 6 against windows of up to 11 pedestrians (truncated), indices -3 and n_windows + 5 (clamped), an empty window,
    T_pred = 0, index = NULL (the first N windows in order)"""
    from social_stgcnn_amd import _lib
    t_obs, v = 8, 6
    rel_all, win_start = R.gather_inputs(t_obs, t_pred)
    n_windows = len(win_start) - 1
    assert index is None or (index[1] == n_windows + 5 and index[0] == -3)
    n = n_windows if index is None else len(index)
    ref_obs, ref_tgt, ref_peds = R.gather_windows(rel_all, win_start, index, n, v, t_obs, t_pred)
    rd, wd = torch.from_numpy(rel_all).to(dev), torch.from_numpy(win_start).to(dev)
    idx = torch.tensor(index, dtype=torch.int32, device=dev) if index is not None else None
    obs = torch.full((n, v, 2, t_obs), R.SENTINEL, device=dev)
    tgt = torch.full((n * t_pred * v * 2 + 4,), R.SENTINEL, device=dev)         # (+4: a valid address when T_pred = 0)
    peds = torch.full((n,), -7, device=dev, dtype=torch.int32)
    P = _lib.ptr
    _lib.check(_lib.lib().stg_gather_windows(P(rd), P(wd), P(idx), n_windows, n, v, t_obs, t_pred, P(obs), P(tgt), P(peds),
                                             _lib.stream_ptr()), "stg_gather_windows")
    assert np.array_equal(_np(peds), ref_peds)
    _assert_exact(_np(obs), ref_obs, "obs_rel")
    _assert_exact(_np(tgt)[:ref_tgt.size].reshape(ref_tgt.shape), ref_tgt, "target")
    assert (_np(tgt)[ref_tgt.size:] == R.SENTINEL).all()                        # nothing written past the target
