"""The host references of tests/ops_ref.py against torch's own float64 einsum / conv2d / clip_grad_norm_ autograd, and
the condition that lets tests/test_gpu_ops_edges.py demand bit equality: for every integer-valued case the sum of the
absolute terms of every output stays below 2^24, so every partial sum of any order is an exact fp32 integer."""
import numpy as np
import pytest
import torch

import ops_ref as R


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("case", [c for c in R.AGG_CASES if c["c"] <= 17 and c["v"] <= 68], ids=lambda c: c["id"])
def test_agg_reference_is_torch_einsum_on_the_valid_block(case):
    x, adj, dy = R.agg_inputs(case, integer=False)
    n, v = case["n"], case["v"]
    peds = R.clamp_peds(case["peds"], n, v)
    xt = _t(x).requires_grad_(True)
    at = _t(adj)
    ys = [torch.einsum("ctv,tvw->ctw", xt[i, :, :, :p], (at if case["shared"] else at[i])[:, :p, :p])
          for i, p in enumerate(peds)]
    sum((ys[i] * _t(dy)[i, :, :, :p]).sum() for i, p in enumerate(peds)).backward()
    y, dx = R.agg_fwd(x, adj, case["peds"]), R.agg_dx(dy, adj, case["peds"])
    for i, p in enumerate(peds):
        np.testing.assert_allclose(y[i, :, :, :p], ys[i].detach().numpy(), rtol=1e-13, atol=1e-13)
        assert not y[i, :, :, p:].any() and not dx[i, :, :, p:].any()
    # the padded slots of x hold the sentinel and receive no gradient: autograd on the slices says the same
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", [c for c in R.CONV_CASES if c["n"] <= 6], ids=lambda c: c["id"])
def test_conv_reference_is_conv2d_autograd_with_the_mask(case):
    x, w, b, dy = R.conv_inputs(case, integer=False)
    peds = R.clamp_peds(case["peds"], case["n"], case["v"])
    mask = torch.zeros(case["n"], 1, 1, case["v"], dtype=torch.float64)
    for i, p in enumerate(peds):
        mask[i, ..., :p] = 1
    xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
    bt = _t(b).requires_grad_(True) if b is not None else None
    yt = torch.nn.functional.conv2d(xt * mask, wt, bt, padding=(case["pad"], 0)) * mask
    (yt * _t(dy)).sum().backward()
    y = R.conv_fwd(x, w, b, case["pad"], case["peds"])
    dx, dw, db = R.conv_bwd(x, w, dy, case["pad"], case["peds"])
    kw = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(y, yt.detach().numpy(), **kw)
    np.testing.assert_allclose(dx, xt.grad.numpy(), **kw)
    np.testing.assert_allclose(dw, wt.grad.numpy()[..., 0], **kw)
    if b is not None:
        np.testing.assert_allclose(db, bt.grad.numpy(), **kw)
    to = case["t"] + 2 * case["pad"] - case["kt"] + 1
    assert y.shape == (case["n"], case["cout"], to, case["v"])


def test_module_reference_is_the_chained_torch_ops():
    x, w, b, adj, dy = R.module_inputs(integer=False)
    c = R.MODULE_CASE
    peds = R.clamp_peds(c["peds"], c["n"], c["v"])
    xt, wt, bt = (_t(a).requires_grad_(True) for a in (x, w, b))
    total = 0
    for i, p in enumerate(peds):
        if p == 0:
            continue
        h = torch.nn.functional.conv2d(xt[i:i + 1, :, :, :p], wt, bt)
        y = torch.einsum("nctv,tvw->nctw", h, _t(adj)[i, :, :p, :p])
        np.testing.assert_allclose(R.module_ref(x, w, b, adj, dy)["y"][i, :, :, :p], y[0].detach().numpy(), atol=1e-12)
        total = total + (y[0] * _t(dy)[i, :, :, :p]).sum()
    total.backward()
    ref = R.module_ref(x, w, b, adj, dy)
    np.testing.assert_allclose(ref["dx"], xt.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(ref["dw"], wt.grad.numpy()[..., 0], atol=1e-12)
    np.testing.assert_allclose(ref["db"], bt.grad.numpy(), atol=1e-12)


@pytest.mark.parametrize("max_norm", (None, 0.05, 1e6))
def test_clip_sgd_reference_is_clip_grad_norm_then_sgd(max_norm):
    p0, g0 = R.flat_inputs(8193, integer=False)
    ref_p = torch.nn.Parameter(_t(p0).clone())
    ref_p.grad = _t(g0).clone()
    total = torch.nn.utils.clip_grad_norm_([ref_p], max_norm) if max_norm is not None else ref_p.grad.norm()
    with torch.no_grad():
        ref_p -= 0.01 * ref_p.grad
    p, g, norm = R.clip_sgd(p0, g0, 0.01, max_norm)
    np.testing.assert_allclose(p, ref_p.detach().numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(g, ref_p.grad.numpy(), rtol=1e-14, atol=0)
    assert abs(norm - float(total)) <= 1e-14 * norm
    # an all-zero gradient with clipping on: coefficient max_norm / 1e-6 clamps to 1, nothing moves
    p, g, norm = R.clip_sgd(p0, np.zeros_like(g0), 0.01, 0.05)
    assert np.array_equal(p, p0.astype(np.float64)) and not g.any() and norm == 0.0


def test_raw_adjacency_is_the_oracles_first_half():
    """adj_raw follows the oracle's arithmetic: normalising it gives seq_to_graph_np's Laplacian bit for bit, and its
    entries are the reference's anorm on fp32 tensors"""
    from oracle import stgcnn_oracle as O
    rel = R.adj_rel(np.random.default_rng(3), 1, 7, 5)[0]
    raw = R.adj_raw(rel)
    deg = raw.sum(axis=2)
    dinv = 1.0 / np.sqrt(deg)
    lap = -raw * dinv[:, :, None] * dinv[:, None, :]
    idx = np.arange(7)
    lap[:, idx, idx] = (deg - 1.0) * dinv * dinv
    assert np.array_equal(lap.astype(np.float32), O.seq_to_graph_np(rel)[1])
    step = torch.from_numpy(rel)
    for t in range(5):
        for h in range(7):
            for k in range(7):
                want = 1.0 if h == k else O.anorm(step[h, :, t], step[k, :, t])
                assert raw[t, h, k] == want
    assert (raw == 0).sum() > 0                                # coincident pedestrians are in the draw


def test_weighted_sum_and_gather_references():
    v, w = R.flat_inputs(1025, integer=False)
    assert R.weighted_sum(v, w) == pytest.approx(float((_t(v) * _t(w)).sum()), rel=1e-13)
    assert R.weighted_sum(v) == pytest.approx(float(_t(v).sum()), rel=1e-13)
    assert R.weighted_sum(v[:0]) == 0.0
    rel_all, ws = R.gather_inputs(8, 12)
    idx = [-3, 14, 1, 2, 4]
    obs, tgt, peds = R.gather_windows(rel_all, ws, idx, len(idx), 6, 8, 12)
    assert list(peds) == [3, 5, 6, 0, 6]                       # clamped to window 0 and 8; 11 and 7 truncated to V = 6
    assert np.array_equal(obs[2], rel_all[3:9, :, :8]) and np.array_equal(tgt[2, 5, :, 1], rel_all[3:9, 1, 13])
    assert not obs[0, 3:].any() and not tgt[0, :, 3:].any() and not obs[3].any()
    _, tgt0, _ = R.gather_windows(rel_all[:, :, :8], ws, None, 9, 6, 8, 0)
    assert tgt0.shape == (9, 0, 6, 2)


def test_integer_cases_stay_exact_in_fp32():
    """Sum of |terms| < 2^24 for every output of every integer-valued case, computed from the inputs the GPU test uses
    (the dw accumulation case adds into the same buffer twice)."""
    worst = {}
    for case in R.AGG_CASES:
        worst["agg/" + case["id"]] = R.max_abs_term_sum(R.agg_term_sums(case))
    for case in R.CONV_CASES:
        worst["conv/" + case["id"]] = R.max_abs_term_sum(R.conv_term_sums(case, repeats=2))
    x, w, b, adj, dy = R.module_inputs(integer=True)
    worst["module"] = R.max_abs_term_sum(R.module_ref(*(np.abs(a) for a in (x, w, b, adj, dy))).values())
    for count in R.COUNTS:
        p, g = R.flat_inputs(count, integer=True)
        worst["sgd/%d" % count] = float(np.max(np.abs(p) + 4.0 * np.abs(g)))        # lr = 4 at the most
    for n in R.WSUM_NS:
        v, w = R.flat_inputs(n, integer=True)
        worst["wsum/%d" % n] = float(np.sum(np.abs(v * w)) + np.sum(np.abs(v)))
    assert max(worst.values()) < R.EXACT_LIMIT, worst
    assert worst["conv/n2049"] > 2.0 ** 15                      # the large-N sums are not trivially small either
    # the inputs of the exact checks are integers and the sentinel is in them
    x, adj, dy = R.agg_inputs(R.AGG_CASES[2], integer=True)
    assert np.array_equal(x, np.round(x)) and (x[0] == R.SENTINEL).all() and (adj[2, :, 1:, :] == R.SENTINEL).all()
    # ragged batches put the last valid pedestrian on every position of a four-wide strip; the grid-stride cases keep
    # the first workgroup's first and last scene non-empty
    assert {p % 4 for p in R.clamp_peds(R.AGG_CASES[5]["peds"], 7, 4) if p} == {0, 1, 2, 3}
    for name, last in (("n513", 512), ("n2049", 2048)):
        peds = R.clamp_peds(R.conv_case(name)["peds"], R.conv_case(name)["n"], R.conv_case(name)["v"])
        assert peds[0] > 0 and peds[last] > 0


def test_case_lists_cover_what_they_name():
    """the sizes the GPU file relies on to reach a branch, restated from the dispatch conditions of the entry points"""
    by = {c["id"]: c for c in R.AGG_CASES}
    lds = lambda c: 4 * c["c"] * c["t"] * c["v"]
    assert 64 * 1024 < lds(by["v32_c65_lds66k"]) <= 160 * 1024 and 64 * 1024 < lds(by["v132_c16_lds67k"]) <= 160 * 1024
    assert lds(R.AGG_REFUSED) > 160 * 1024
    assert all(lds(c) <= 64 * 1024 for c in R.AGG_CASES if c["v"] in (8, 16, 32, 64) and "lds" not in c["id"])
    assert {c["v"] for c in R.AGG_CASES} >= {1, 3, 4, 8, 12, 16, 31, 32, 33, 64, 68, 130}
    assert {c["t"] for c in R.AGG_CASES} >= {1, 5, 8, 12} and {c["c"] for c in R.AGG_CASES} >= {1, 8, 9, 17}
    cv = {c["id"]: c for c in R.CONV_CASES}
    big = cv["lds_over_64k"]
    fwd = 4 * (big["cout"] * big["cin"] * big["kt"] + big["cin"] * big["t"] * big["v"])
    assert 64 * 1024 < fwd <= 160 * 1024
    assert cv["w1024"]["cin"] * cv["w1024"]["cout"] * cv["w1024"]["kt"] == 1024 and cv["cout256"]["cout"] == 256
    assert {c["kt"] for c in R.CONV_CASES} >= {1, 2, 3, 5} and {c["n"] for c in R.CONV_CASES} >= {1, 513, 2049}
    assert [c["cin"] * c["cout"] * c["kt"] for c in R.CONV_REFUSED] == [1025, 257]
