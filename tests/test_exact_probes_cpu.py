"""CPU checks of the exact-class probes (tests/exact_probes.py): every probe of the table is valid (both conditions of
`probe_budget`, the oracle's result representable in float32), the probes of every focus are complete (each of the
six kept piece products is needed by at least one of them) and cover every K slot and every scene position, the three
dropped products vanish identically, and `conv6` over the six kept ones equals the oracle's pre-activation exactly.
Also the seeds of test_gpu_layouts.py's eval-mode backward cases (section 2b)."""
import numpy as np
import pytest
import torch

import exact_probes as EP
import layout_cases as LC

_CASES = EP.probe_cases()
_BUILT = {}


def _probe(case):
    """built once, shared by every test, left unchanged"""
    if case.id not in _BUILT:
        _BUILT[case.id] = case.build()
    return _BUILT[case.id]


def _by_focus():
    out = {}
    for c in _CASES:
        out.setdefault(c.focus, []).append(c)
    return out


def test_batchnorm_variances_give_exact_float32_scales():
    """running_var = float32(s - float32(1e-5)): var + eps == s in float32 and 1 / sqrt(s) is 2, 1, 0.5, 0.25; the
    double s - 1e-5 of the oracle gives the same scale to 1e-16."""
    eps = np.float32(1e-5)
    for s, scale in zip(EP.BN_S, (2.0, 1.0, 0.5, 0.25)):
        var = np.float32(np.float32(s) - eps)
        tot = np.float32(var + eps)
        assert tot == np.float32(s), (s, tot)
        assert np.float32(1.0) / np.sqrt(tot, dtype=np.float32) == np.float32(scale)
        assert abs(1.0 / np.sqrt((s - 1e-5) + 1e-5) - scale) < 1e-15


def test_split3_is_an_exact_truncation_split():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4096) * 2.0 ** rng.integers(-8, 8, 4096)).astype(np.float32)
    h, m, l = EP.split3(x)
    for p in (h, m, l):
        assert not np.any(p.view(np.uint32) & np.uint32(0xffff))              # each piece is a bf16
    assert np.all(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64) == x.astype(np.float64))
    assert np.all(np.abs(h) <= np.abs(x)) and np.all((h == 0) | (np.sign(h) == np.sign(x)))


def test_the_table_reaches_every_focus_and_class_on_generic_and_canon32():
    for name, layouts in (("generic", {(1, 1), (1, 3), (1, 8)}), ("canon32", {(1, 5)})):
        for layout in layouts:
            got = {(c.focus, c.cls) for c in _CASES if c.variant.name == name and c.variant.layout == layout}
            assert got == {(f, k) for f in EP.focuses(layout[1]) for k in EP.CLASSES}, (name, layout)
    for v in EP.variants():
        fs = set(v.focus_set or EP.focuses(v.layout[1]))
        assert {"txp0", "out"} <= fs and fs & {"gcn", "tcn", "res"}, v.name
        assert v.layout[1] < 3 or any(f.startswith("txp") and f != "txp0" for f in fs), v.name
    assert len({c.id for c in _CASES}) == len(_CASES)


@pytest.mark.parametrize("case", _CASES, ids=repr)
def test_probe_is_valid(case):
    """Built (the generator asserts that float32(oracle64) is the oracle's value), then both validity conditions for
    every operation of every scene; the operand classes hold at the focus; the data reach every row and column."""
    pr = _probe(case)
    used = EP.probe_budget(pr)
    assert 0 < used < 1
    assert not all(float(v) == 1.0 for k, v in pr.state.items() if "prelu" in k or "tcn.1" in k)
    for w, x, b, y in EP.focus_records(pr):
        tw, tx = EP.top_piece(w), EP.top_piece(x)
        want_w, want_x = {"w_wide": (2, 0), "data_wide": (0, 2), "medium": (1, 1)}[pr.cls]
        assert np.all(tw == want_w), (case, "focus weights dense and of the class")
        assert np.all(tx == want_x), (case, "focus data dense and of the class: every row, every column")
        if pr.cls == "w_wide":
            assert np.all(np.frexp(x)[0] == np.sign(x) * 0.5), (case, "one-bit data")
        if pr.cls == "data_wide":
            assert np.all(np.frexp(w)[0] == np.sign(w) * 0.5), (case, "one-bit weights")
    for i, sc in enumerate(pr.scenes):
        if sc is not None:
            assert pr.expected[i].shape == (EP.C_OUT, EP.T_PRED, sc[0].shape[2]) and np.all(np.isfinite(pr.expected[i]))


@pytest.mark.parametrize("case", _CASES, ids=repr)
def test_dropped_products_vanish_and_the_kept_six_are_the_oracle(case):
    pr = _probe(case)
    for w, x, b, y in EP.focus_records(pr):
        assert not np.any(EP.conv6(w, x, keep=EP.DROPPED)), case
        assert np.array_equal(EP.conv6(w, x, bias=b), y), case


@pytest.mark.parametrize("focus", sorted(_by_focus()))
def test_probes_of_a_focus_need_each_of_the_six_kept_products(focus):
    """Completeness: for each kept product there is a probe of the focus whose conv6 result moves by at least one
    float32 ulp of the expected pre-activation, in at least one element, when that product is left out."""
    need = set(EP.KEPT)
    for case in _by_focus()[focus]:
        pr = _probe(case)
        for w, x, b, y in EP.focus_records(pr):
            ulp = np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
            full = EP.conv6(w, x, bias=b)
            for prod in list(need):
                got = EP.conv6(w, x, keep=[p for p in EP.KEPT if p != prod], bias=b)
                if np.any(np.abs(got - full) >= ulp):
                    need.discard(prod)
        if not need:
            break
    assert not need, (focus, need)


@pytest.mark.parametrize("focus", sorted(_by_focus()))
def test_probes_of_a_focus_cover_every_weight_slot_and_scene_position(focus):
    """Accumulated over the probes of a focus: every (co, ci, kh, kw) of the focus weights -- every K slot of wp_value and
    every output row -- holds a wide weight in some W-wide probe, and wide data reach every channel and feature row, the
    first and the last column, interior columns and both sides of every team chunk bound in some data-wide probe."""
    wide_w, rows, cols = None, set(), set()
    for case in _by_focus()[focus]:
        pr = _probe(case)
        for w, x, b, y in EP.focus_records(pr):
            if pr.cls == "w_wide":
                hit = EP.top_piece(w) == 2
                wide_w = hit if wide_w is None else (wide_w | hit)
            if pr.cls == "data_wide":
                ci, r, v = np.nonzero(EP.top_piece(x) == 2)
                c = x.shape[2]
                rows |= set(zip(ci.tolist(), r.tolist()))
                edges = EP.dy_columns(c)
                cols |= {"first" if k == 0 else "last" if k == c - 1 else "edge" if k in edges else "interior"
                         for k in set(v.tolist())}
                n_ci, n_r = x.shape[0], x.shape[1]
    assert wide_w is not None and wide_w.all(), focus
    assert rows == {(a, b) for a in range(n_ci) for b in range(n_r)}, focus
    assert cols == {"first", "last", "edge", "interior"}, (focus, cols)


# ------------------------------------------------------------------------------------------
# backward probes
# ------------------------------------------------------------------------------------------
_BWD = EP.bwd_probe_cases()


def _bwd_by_focus():
    out = {}
    for c in _BWD:
        out.setdefault(c.focus, []).append(c)
    return out


def _bwd_probe(case):
    key = "bwd-" + case.id
    if key not in _BUILT:
        _BUILT[key] = case.build()
    return _BUILT[key]


def test_the_backward_table_reaches_every_focus_and_class_on_generic_and_canon32():
    for name, layouts in (("generic", {(1, 1), (1, 3), (1, 8)}), ("canon32", {(1, 5)})):
        for layout in layouts:
            got = {(c.focus, c.cls) for c in _BWD if c.variant.name == name and c.variant.layout == layout}
            assert got == {(f, k) for f in EP.bwd_focuses(layout[1]) for k in EP.CLASSES}, (name, layout)
    for v in {id(c.variant): c.variant for c in _BWD}.values():
        fs = {c.focus for c in _BWD if c.variant is v}
        assert {"txp0", "out", "tcn"} <= fs, v.name
        assert v.layout[1] < 3 or any(f.startswith("txp") and f != "txp0" for f in fs), v.name


@pytest.mark.parametrize("case", _BWD, ids=repr)
def test_backward_probe_is_valid(case):
    """Built (the generator asserts every gradient of the float64 oracle representable), then both validity conditions
    for every input-gradient convolution and every reduction over positions and scenes.  dy is non-zero in at most four
    scenes, the first and the last of the batch among them; the operand classes hold at the focus; the weight gradient of
    the cut convolution is non-zero (it is what sees the focus's result position by position)."""
    pr = _bwd_probe(case)
    used = EP.probe_budget_bwd(pr)
    assert 0 < used < 1
    n = pr.backward
    assert 1 <= len(pr.dy) <= 4 and 0 in pr.dy and n - 1 in pr.dy
    assert len(pr.dy) == min(n, 4)
    assert sum(len(v) for _, v in pr.dy.values()) == EP.N_DY
    want_w, want_x = {"w_wide": (2, 0), "data_wide": (0, 2), "medium": (1, 1)}[pr.cls]
    for wt, dz in EP.bwd_focus_records(pr):
        assert np.all(EP.top_piece(wt) == want_w), case
        assert np.all(EP.top_piece(dz)[dz != 0] == want_x) and np.any(dz), case
    cut = ["st_gcns.0.gcn.conv.weight", "st_gcns.0.residual.0.weight"] if pr.focus in ("tcn", "txp0") else ["tpcnns.0.weight"]
    for k in cut:
        assert np.any(pr.grads[k]), (case, k)
        assert np.any(pr.state[k].numpy()) == (not pr.cut), (case, k)
    # dx: zero behind a cut forward, not zero in the uncut family (the workgroup variants carry it)
    assert all(np.any(d) == (not pr.cut) for d in pr.dx.values()), case
    assert not all(float(v) == 1.0 for k, v in pr.state.items() if "prelu" in k or "tcn.1" in k)


@pytest.mark.parametrize("case", _BWD, ids=repr)
def test_backward_dropped_products_vanish_and_the_kept_six_are_the_whole_sum(case):
    """conv6 over the transposed, flipped focus weights (prep_dgrad_vector's arrangement) and the dz the oracle's autograd
    hands to the focus: the three dropped products are identically zero and the six kept ones are the float64
    convolution of the unsplit operands, which is not zero."""
    pr = _bwd_probe(case)
    for wt, dz in EP.bwd_focus_records(pr):
        assert not np.any(EP.conv6(wt, dz, keep=EP.DROPPED)), case
        d_in = EP.conv6(wt, dz)
        assert np.array_equal(d_in, EP._conv64(wt, dz)) and np.any(d_in), case


@pytest.mark.parametrize("focus", sorted(_bwd_by_focus()))
def test_backward_probes_of_a_focus_reach_every_row_and_column_class(focus):
    """Accumulated over the backward probes of a focus, the dz that meets the focus weights is non-zero in every channel,
    in every row of the feature axis, in the first and the last column, in interior columns, on both sides of a chunk
    bound of a two- and of a four-wave team (columns ceil(c/nch) k - 1 and ceil(c/nch) k), and in scenes of one
    pedestrian up to the widest; and no two probes of the focus use the same positions."""
    chans, rows, cols, sides, seen = set(), set(), set(), set(), []
    for case in _bwd_by_focus()[focus]:
        pr = _bwd_probe(case)
        seen.append(tuple(sorted((n, tuple(map(tuple, w.tolist()))) for n, (w, _) in pr.dy.items())))
        for wt, dz in EP.bwd_focus_records(pr):
            co, r, v = np.nonzero(dz)
            c = dz.shape[2]
            chans |= set(co.tolist())
            rows |= set(r.tolist())
            for k in set(v.tolist()):
                cols.add("first" if k == 0 else "last" if k == c - 1 else "interior")
                for nch in (2, 4):
                    wc = -(-c // nch)
                    if c > 32 and k % wc == wc - 1 and k + 1 < c:
                        sides.add((nch, "left"))
                    if c > 32 and k % wc == 0 and k > 0:
                        sides.add((nch, "right"))
    n_co = wt.shape[1]
    assert chans == set(range(n_co)) and rows == set(range(dz.shape[1])), (focus, chans, rows)
    assert cols == {"first", "last", "interior"}, (focus, cols)
    assert sides == {(2, "left"), (2, "right"), (4, "left"), (4, "right")}, (focus, sides)
    assert len(set(seen)) == len(seen), focus


def test_the_dx_family_runs_on_every_workgroup_variant():
    dx = [c for c in _BWD if not c.cut]
    wg = {id(c.variant) for c in _BWD if c.variant.name == "wg"}
    assert {id(c.variant) for c in dx} == wg and all(c.focus == "tcn" and c.cls in EP.DX_CLASSES for c in dx)
    for c in dx:
        pr = _bwd_probe(c)
        # the aggregation's backward runs on a non-identity adjacency wherever the scene has two pedestrians or more
        assert all(np.any(adj != np.eye(adj.shape[1], dtype=np.float32)) for sc in pr.scenes if sc is not None
                   for adj in [sc[1]] if adj.shape[1] > 1), c


@pytest.mark.parametrize("focus", sorted(_bwd_by_focus()))
def test_backward_probes_of_a_focus_need_each_of_the_six_kept_products(focus):
    need = set(EP.KEPT)
    for case in _bwd_by_focus()[focus]:
        pr = _bwd_probe(case)
        for wt, dz in EP.bwd_focus_records(pr):
            y = EP.conv6(wt, dz)
            ulp = np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
            for prod in list(need):
                got = EP.conv6(wt, dz, keep=[p for p in EP.KEPT if p != prod])
                if np.any((np.abs(got - y) >= ulp) & (y != 0)):
                    need.discard(prod)
        if not need:
            break
    assert not need, (focus, need)


def test_eval_backward_cases_fp32_oracle_inside_project_bars():
    """The eval-mode backward cases of tests/test_gpu_layouts.py (section 2b), as
    test_lib_cpu.py::test_layout_cases_fp32_oracle_inside_project_bars treats the training-step matrix: the float32
    oracle sits inside the project bars of the float64 oracle and no float64 pre-activation lies within KINK_MARGIN of
    the PReLU kink (layout_cases.SEED_SHIFT).  The eval forward does not depend on the new argument, and neither does a
    training step (first case: every result of training=True with eval_grads=True equals the default's)."""
    for case in LC.eval_backward_cases():
        _, state, b = case.build()
        r64 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, training=False, eval_grads=True)
        r32 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, dtype=torch.float32, training=False,
                                   eval_grads=True)
        p, l, g, s = LC.oracle_distance(r32, r64)
        print("%-28s V_pred %.1e  loss %.1e  grad %.1e  nearest pre-activation %.1e" % (case.id, p, l, g, r64.kink[0]))
        assert r64.kink[0] >= LC.KINK_MARGIN, (case, r64.kink[0])
        assert p < LC.BAR_PRED and l < LC.BAR_PRED and g < LC.BAR_GRAD and s == 0.0, (case, p, l, g)
        assert r64.after is None and r64.after_once is None
        live = [k for k, v in r64.grads.items() if v is not None]
        assert all(np.any(r64.grads[k]) for k in live if k.endswith(LC.ZERO_GRAD_BIASES))     # ordinary gradients
        fwd = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, training=False)
        assert fwd.grads is None and all(np.array_equal(fwd.pred[i], r64.pred[i]) for i in r64.pred)
    case = LC.eval_backward_cases()[0]
    _, state, b = case.build()
    t0 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn)
    t1 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, eval_grads=True)
    assert all(np.array_equal(t0.pred[i], t1.pred[i]) and t0.loss[i] == t1.loss[i] for i in t0.pred)
    assert all((t0.grads[k] is None and t1.grads[k] is None) or np.array_equal(t0.grads[k], t1.grads[k]) for k in t0.grads)
    assert all(torch.equal(t0.after[k], t1.after[k]) for k in t0.after)
