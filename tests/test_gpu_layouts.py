"""GPU (-m gpu): every model layout stg_model_desc accepts, at batch scale, against the float64 oracle
(oracle/stgcnn_oracle.py looped scene by scene).  No case runs on default-initialised weights: every parameter and
buffer is drawn distinct (layout_cases.randomise), so a read or write of the wrong slot changes a number.

Bars are the project's own (layout_cases.BAR_*: 5e-5 absolute on V_pred and the loss, 1e-4 relative on gradients under
`grad_errors`' scaling, 2e-6 on the running statistics).  Each case also runs the same oracle in float32 on the CPU and
measures its distance to the float64 oracle in the same metric; the bar of the case is max(project bar, 4 x that
distance) and both numbers are printed.  No element and no case is excluded from a comparison."""
import ctypes

import numpy as np
import pytest
import torch

import layout_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


def _set_options(monkeypatch, options):
    from social_stgcnn_amd import ops
    for k, val in options.items():
        monkeypatch.setitem(ops.OPTIONS, k, val)


def _check_step(dev, case, want_dx=False, txp_bar=None):
    """One training step of `case` on the device against the oracle: per-scene V_pred on the valid block and exact
    zeros on the padding, per-scene losses, every parameter gradient (dead ones None on both sides), dx where asked,
    BatchNorm running buffers and num_batches_tracked.  txp_bar: the bar of the TXP-CNN gradients in bf16 storage."""
    from social_stgcnn_amd.metrics import bivariate_loss
    model, state, b = case.build()
    r64 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, want_dx=want_dx)
    r32 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, dtype=torch.float32)
    own = LC.oracle_distance(r32, r64)
    bar_p, bar_l, bar_g, bar_s = LC.bars(own)
    m = model.to(dev).train()
    x, adj, tgt, peds, w = b.device(dev)
    if want_dx:
        x.requires_grad_(True)
    y, _ = m(x, adj, peds)
    losses = bivariate_loss(y.permute(0, 2, 3, 1), tgt, peds)
    (losses * w).sum().backward()
    yc, lc = y.detach().cpu().numpy(), losses.detach().cpu().numpy()
    dxc = x.grad.cpu().numpy() if want_dx else None
    e_pred = e_loss = e_dx = 0.0
    for i in range(b.unique):
        c = int(b.counts_u[i])
        sel = b.idx == i
        assert np.all(yc[sel][:, :, :, c:] == 0), (case, i, "V_pred padding")
        if c == 0:
            assert np.all(lc[sel] == 0), (case, i)
            continue
        ref = np.transpose(r64.pred[i], (2, 0, 1))[None]                      # (1,5,P,c)
        e_pred = max(e_pred, LC.maxdiff(yc[sel][:, :, :, :c], np.broadcast_to(ref, (int(sel.sum()),) + ref.shape[1:])))
        e_loss = max(e_loss, float(np.abs(lc[sel] - r64.loss[i]).max()))
        if want_dx:
            assert np.all(dxc[sel][:, :, :, c:] == 0), (case, i, "dx padding")
            scale = max(1e-3, float(np.abs(r64.dx[i]).max()))
            e_dx = max(e_dx, LC.maxdiff(dxc[sel][:, :, :, :c], np.broadcast_to(r64.dx[i][None], (int(sel.sum()),) +
                                                                               r64.dx[i].shape)) / scale)
    errs = LC.grad_errors(((name, p.grad) for name, p in m.named_parameters()), lambda name: r64.grads[name])
    e_stat = 0.0
    for k, val in m.state_dict().items():
        if "running" in k:
            e_stat = max(e_stat, LC.maxdiff(val.cpu().numpy(), r64.after[k].numpy()))
        if "num_batches" in k:
            assert int(val) == int(r64.after[k]), (case, k)
    worst = max(errs, key=errs.get)
    print("\n%-34s V_pred %.1e (fp32 oracle %.1e)  loss %.1e (%.1e)  grad %.1e (%.1e) %s  dx %.1e  stats %.1e (%.1e)"
          % (case.id, e_pred, own[0], e_loss, own[1], errs[worst], own[2], worst, e_dx, e_stat, own[3]))
    assert e_pred < bar_p and e_loss < bar_l, (case, e_pred, e_loss)
    if txp_bar is None:
        bad = {k: e for k, e in errs.items() if e > bar_g}
    else:
        # bf16 storage (test_bf16_storage_mode_measured_error's split): the st_gcn block gradients stay in the exact
        # class, the TXP weight / bias / slope gradients carry the bf16 rounding of the saved planes
        bad = {k: e for k, e in errs.items() if e > (bar_g if k.startswith("st_gcns") else txp_bar)}
    assert not bad, (case, bad)
    assert e_dx < bar_g, (case, e_dx)
    assert e_stat < bar_s, (case, e_stat)
    return m, b, r64


_SCENE = LC.scene_path_cases()


# ------------------------------------------------------------------------------------------
# 1. layout x batch geometry, one training step
# ------------------------------------------------------------------------------------------
@pytest.mark.auto_path
@pytest.mark.parametrize("case", [c for c in _SCENE if c.group in ("ragged", "small", "tiled")], ids=repr)
def test_scene_path_ragged_step(dev, case):
    """One st_gcn block, n_txpcnn 1..8, the planner choosing the path: ragged batches padded to 17..128 with counts
    0, 1, 2 .. V on both sides of every team-class bound (8/16 for these batch sizes; the `tiled` cases repeat 41
    distinct scenes to 400 and 1536 scenes for the 16/32 and 32/64 bounds, the oracle's gradient scaled by each scene's
    multiplicity), garbage in the padded slots of x, A and the target; and small batches of 1, 3, 8, 40 scenes."""
    _check_step(dev, case)


@pytest.mark.auto_path
@pytest.mark.parametrize("case", [c for c in _SCENE if c.group == "uniform"], ids=repr)
def test_scene_path_large_uniform_step(dev, case):
    """N = 1536 / 2048 at V = 32 without num_peds: the solo Generic kernel at both workgroup widths.  37 distinct
    scenes tiled (37 divides neither batch size): every scene's V_pred and loss against the oracle of its source, the
    gradient against the oracle's (each scene weighted by its multiplicity), the running statistics folded over the
    whole batch; and gradient additivity over the two half batches."""
    from social_stgcnn_amd.metrics import bivariate_loss
    m, b, _ = _check_step(dev, case)
    x, adj, tgt, _, w = b.device(dev)
    flat = lambda: torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None])
    g_all = flat().clone()
    parts = []
    for lo, hi in ((0, b.n // 2), (b.n // 2, b.n)):
        m.zero_grad(set_to_none=True)
        y, _ = m(x[lo:hi], adj[lo:hi])
        (bivariate_loss(y.permute(0, 2, 3, 1), tgt[lo:hi]) * w[lo:hi]).sum().backward()
        parts.append(flat().clone())
    err = float((parts[0] + parts[1] - g_all).abs().max()) / float(g_all.abs().max())
    print("additivity over batch halves: %.1e" % err)
    assert err < 1e-4                                   # test_full_size_properties' bound


@pytest.mark.parametrize("case", [c for c in _SCENE if c.group == "bf16"], ids=repr)
def test_scene_path_bf16_storage_step(dev, case, monkeypatch):
    """STG_OPT_BF16_STORE under a generic layout: V_pred and loss at the fp32 bars, block gradients in the exact class,
    TXP gradients at test_bf16_storage_mode_measured_error's 3e-3."""
    _set_options(monkeypatch, case.options)
    _check_step(dev, case, txp_bar=3e-3)


@pytest.mark.parametrize("case", [c for c in _SCENE if c.group == "wavef32"], ids=repr)
def test_scene_path_f32_mfma_and_split_bf16_step(dev, case, monkeypatch):
    """The WaveF32 branch (STG_OPT_F32_MFMA, STG_OPT_SPLIT_BF16) with a generic layout."""
    _set_options(monkeypatch, case.options)
    _check_step(dev, case)


@pytest.mark.auto_path
@pytest.mark.parametrize("case", [c for c in _SCENE if c.group == "wide"], ids=repr)
def test_one_block_model_beyond_the_team_limit(dev, case):
    """V = 130 > kTeamMaxV with a non-canonical one-block model: the workgroup-per-scene kernels, dx included."""
    _check_step(dev, case, want_dx=True)


@pytest.mark.parametrize("case", LC.stacked_cases(), ids=repr)
def test_stacked_layouts_step(dev, case, monkeypatch):
    """n_stgcnn 2..4 (the workgroup-per-scene kernels are their only path): ragged batches padded to 12, 57, 96, three
    scenes at V = 130, wg_waves 1 and 8; the gradient w.r.t. x included."""
    _set_options(monkeypatch, case.options)
    _check_step(dev, case, want_dx=True)


# ------------------------------------------------------------------------------------------
# 2. eval mode with the randomised running statistics; the Predictor
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(1, 3), (1, 8), (2, 5), (4, 8)], ids=lambda l: "%dx%d" % l)
def test_eval_forward_uses_the_running_statistics(dev, layout):
    n_st, n_tx = layout
    case = LC.Case("eval", n_st, n_tx, 57, LC.ragged(57, 20))
    model, state, b = case.build()
    r64 = LC.oracle_model_step(state, b, n_st, n_tx, training=False)
    r32 = LC.oracle_model_step(state, b, n_st, n_tx, dtype=torch.float32, training=False)
    own = LC.oracle_distance(r32, r64)
    m = model.to(dev).eval()
    x, adj, _, peds, _ = b.device(dev)
    with torch.no_grad():
        y, _ = m(x, adj, peds)
    assert m.last_ws_floats == 0
    yc = y.cpu().numpy()
    err = 0.0
    for i in range(b.unique):
        c = int(b.counts_u[i])
        assert np.all(yc[i, :, :, c:] == 0), i
        if c:
            err = max(err, LC.maxdiff(yc[i, :, :, :c], np.transpose(r64.pred[i], (2, 0, 1))))
    print("\neval %dx%d: V_pred %.1e (fp32 oracle %.1e)" % (n_st, n_tx, err, own[0]))
    assert err < LC.bars(own)[0]
    for k, val in m.state_dict().items():
        assert torch.equal(val.cpu(), state[k]), k                            # buffers (and parameters) untouched


# ------------------------------------------------------------------------------------------
# 2b. full-model backward in eval mode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.eval_backward_cases(), ids=repr)
def test_eval_backward_against_the_oracle(dev, case):
    """`.eval()` with requires_grad: stg_model_fwd with a workspace under bn_mode 0, then stg_model_bwd from the loss
    gradient the nll kernel hands back through autograd.  V_pred, per-scene losses and every parameter gradient of
    sum_n w_n loss_n against the float64 oracle at training=False; the bars are the file's own.  An eval-mode BatchNorm
    passes a per-channel shift through, so the conv biases in front of one have ordinary gradients and are compared like
    every other parameter.  The buffers do not move."""
    from social_stgcnn_amd.metrics import bivariate_loss
    model, state, b = case.build()
    r64 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, training=False, eval_grads=True)
    r32 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, dtype=torch.float32, training=False,
                               eval_grads=True)
    own = LC.oracle_distance(r32, r64)
    bar_p, bar_l, bar_g, _ = LC.bars(own)
    m = model.to(dev).eval()
    x, adj, tgt, peds, w = b.device(dev)
    y, _ = m(x, adj, peds)
    assert m.last_ws_floats > 0
    losses = bivariate_loss(y.permute(0, 2, 3, 1), tgt, peds)
    (losses * w).sum().backward()
    yc, lc = y.detach().cpu().numpy(), losses.detach().cpu().numpy()
    e_pred = e_loss = 0.0
    for i in range(b.unique):
        c = int(b.counts_u[i])
        assert np.all(yc[i, :, :, c:] == 0), (case, i, "V_pred padding")
        if c == 0:
            assert lc[i] == 0, (case, i)
            continue
        e_pred = max(e_pred, LC.maxdiff(yc[i, :, :, :c], np.transpose(r64.pred[i], (2, 0, 1))))
        e_loss = max(e_loss, abs(float(lc[i]) - r64.loss[i]))
    errs = LC.grad_errors(((name, p.grad) for name, p in m.named_parameters()), lambda name: r64.grads[name], ())
    worst = max(errs, key=errs.get)
    print("\n%-28s V_pred %.1e (fp32 oracle %.1e)  loss %.1e (%.1e)  grad %.1e (%.1e) %s"
          % (case.id, e_pred, own[0], e_loss, own[1], errs[worst], own[2], worst))
    assert e_pred < bar_p and e_loss < bar_l, (case, e_pred, e_loss)
    assert not {k: e for k, e in errs.items() if e > bar_g}, (case, errs)
    for k, val in m.state_dict().items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(val.cpu(), state[k]), k


def test_predictor_on_a_non_canonical_model(dev):
    """predict.Predictor with n_txpcnn = 3: V_pred against the oracle at training=False, the mean trajectory equal to
    the cumulative sum of V_pred's means from the last observed position (1e-6 on the device's own V_pred, as
    test_mean_trajectory_padding_k0_and_empty_batch asserts; against the oracle's V_pred the twelve summed steps each
    carry the V_pred bar on top), the captured replay bit-equal to eager."""
    from oracle import stgcnn_oracle as O
    from social_stgcnn_amd.predict import Predictor
    n_tx, n, v = 3, 12, 21
    model = LC.randomise(LC.make_model(1, n_tx), 91)
    state = LC.state_of(model)
    counts = LC.ragged_counts(v, n, 91)
    rng = np.random.default_rng(91)
    obs = np.zeros((n, LC.T_OBS, v, 2), np.float32)
    for i, c in enumerate(counts):
        start = rng.uniform(0.0, 4.0, (1, c, 2))
        steps = np.round(rng.uniform(-0.6, 0.6, (LC.T_OBS - 1, c, 2)), 4)
        obs[i, :, :c] = np.concatenate([start, start + np.cumsum(steps, axis=0)], axis=0).astype(np.float32)
    m = model.to(dev).train()
    pr = Predictor(m, k=5)
    obs_d, peds = torch.from_numpy(obs).to(dev), torch.from_numpy(counts).to(dev)
    res = pr.predict(obs_d, peds, seed=5)
    assert m.training
    yc, mean = res.v_pred.cpu().numpy(), res.mean.cpu().numpy()
    st64 = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in state.items()}
    e_pred = e_own = e_mean = 0.0
    for i, c in enumerate(counts):
        c = int(c)
        assert np.all(yc[i, :, :, c:] == 0) and np.all(mean[i, :, c:] == 0)
        if c == 0:
            continue
        rel = np.zeros((c, 2, LC.T_OBS), np.float32)
        rel[:, :, 1:] = np.transpose(obs[i, 1:, :c] - obs[i, :-1, :c], (1, 2, 0))       # float32 differences
        nodes, lap = O.seq_to_graph_np(rel)
        out = O.social_stgcnn_forward(dict(st64), torch.from_numpy(nodes).double().unsqueeze(0).permute(0, 3, 1, 2),
                                      torch.from_numpy(lap).double(), False, n_stgcnn=1, n_txpcnn=n_tx)[0].numpy()
        e_pred = max(e_pred, LC.maxdiff(yc[i, :, :, :c], out))
        last = obs[i, -1, :c].astype(np.float64)[None]
        own = last + np.cumsum(np.transpose(yc[i, 0:2, :, :c], (1, 2, 0)).astype(np.float64), axis=0)
        ref = last + np.cumsum(np.transpose(out[0:2], (1, 2, 0)), axis=0)
        e_own = max(e_own, LC.maxdiff(mean[i, :, :c], own))
        e_mean = max(e_mean, LC.maxdiff(mean[i, :, :c], ref))
    print("\nPredictor 1x3: V_pred %.1e, mean vs own V_pred %.1e, mean vs oracle %.1e" % (e_pred, e_own, e_mean))
    assert e_pred < LC.BAR_PRED and e_own < 1e-6 and e_mean < 1e-6 + LC.T_PRED * LC.BAR_PRED
    replay = pr.capture(n, v, peds)
    r = replay(obs_d, seed=5)
    assert torch.equal(r.samples, res.samples) and torch.equal(r.mean, res.mean) and torch.equal(r.v_pred, res.v_pred)


# ------------------------------------------------------------------------------------------
# 3. the stand-alone st_gcn module
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("use_mdn", (False, True), ids=("prelu", "mdn"))
@pytest.mark.parametrize("residual", (True, False), ids=("res", "nores"))
@pytest.mark.parametrize("c_in", (2, 5))
def test_standalone_st_gcn(dev, c_in, residual, use_mdn, training):
    """st_gcn(c_in, 5) alone (n_txpcnn = 0): residual kinds 0 (residual=False), 1 (identity, c_in = 5) and 2 (conv + BN,
    c_in = 2), with and without the block-final PReLU, train and eval mode, on ragged batches padded to 9 and 40 and one
    unpadded scene of 130 pedestrians, against oracle.st_gcn_forward in float64: output, dx, every parameter gradient
    (the block PReLU's is None or exactly zero under use_mdn, as torch leaves it), BatchNorm buffers."""
    kind = "zero" if not residual else ("identity" if c_in == 5 else "conv")
    seed = 300 + 8 * c_in + 4 * residual + 2 * use_mdn + training
    for vpad, counts, ragged in ((9, [9, 0, 1, 4, 8, 2], True), (40, [40, 17, 33, 0, 5, 39, 16], True),
                                 (130, [130], False)):
        blk = LC.randomise(LC.make_block(c_in, residual, use_mdn), seed + vpad)
        assert blk.residual_kind == {"zero": 0, "identity": 1, "conv": 2}[kind]
        state = LC.state_of(blk)
        b = LC.Batch(counts, vpad, seed + vpad, c_in=c_in, ragged=ragged)
        gy = np.random.default_rng(seed).standard_normal((b.n, 5, LC.T_OBS, vpad)).astype(np.float32)
        r64 = LC.oracle_block_step(state, b, gy, training, use_mdn, kind)
        r32 = LC.oracle_block_step(state, b, gy, training, use_mdn, kind, dtype=torch.float32)
        own_p = max(LC.maxdiff(r32.pred[i], r64.pred[i]) for i in r64.pred)
        own_g = max(LC.grad_errors(((k, r32.grads[k]) for k in r64.grads), lambda k: r64.grads[k]).values())
        own_s = max(LC.maxdiff(r32.after[k].numpy(), r64.after[k].numpy()) for k in r64.after if "running" in k)
        bar_p, bar_g, bar_s = (max(LC.BAR_PRED, LC.WIDEN * own_p), max(LC.BAR_GRAD, LC.WIDEN * own_g),
                               max(LC.BAR_STAT, LC.WIDEN * own_s))
        m = blk.to(dev).train(training)
        x, adj, _, peds, _ = b.device(dev)
        x.requires_grad_(True)
        y, _ = m(x, adj, peds)
        (y * torch.from_numpy(gy).to(dev)).sum().backward()
        yc, dxc = y.detach().cpu().numpy(), x.grad.cpu().numpy()
        e_y = e_dx = 0.0
        for i in range(b.unique):
            c = int(b.counts_u[i])
            assert np.all(yc[i, :, :, c:] == 0) and np.all(dxc[i, :, :, c:] == 0), (vpad, i)
            if c:
                e_y = max(e_y, LC.maxdiff(yc[i, :, :, :c], r64.pred[i]))
                e_dx = max(e_dx, LC.maxdiff(dxc[i, :, :, :c], r64.dx[i]) / max(1e-3, float(np.abs(r64.dx[i]).max())))
        got = dict(m.named_parameters())
        assert set(got) == set(r64.grads)
        if use_mdn:
            assert r64.grads["prelu.weight"] is None
            g = got.pop("prelu.weight").grad
            assert g is None or not bool(g.any())
        ref = {k: r64.grads[k] for k in got}
        if not training:
            # eval-mode BatchNorm passes a per-channel shift through: the conv-bias gradients are ordinary ones
            errs = {k: LC.maxdiff(p.grad.cpu().numpy(), ref[k]) / max(1e-3, float(np.abs(ref[k]).max()))
                    for k, p in got.items()}
        else:
            errs = LC.grad_errors(((k, p.grad) for k, p in got.items()), lambda k: ref[k])
        e_s = 0.0
        for k, val in m.state_dict().items():
            if "running" in k:
                e_s = max(e_s, LC.maxdiff(val.cpu().numpy(), r64.after[k].numpy()))
            if "num_batches" in k:
                assert int(val) == int(r64.after[k]), k
        worst = max(errs, key=errs.get)
        print("\nst_gcn(%d,5) %s%s %s V=%d: y %.1e (fp32 oracle %.1e)  dx %.1e  grad %.1e (%.1e) %s  stats %.1e (%.1e)"
              % (c_in, kind, " mdn" if use_mdn else "", "train" if training else "eval", vpad, e_y, own_p, e_dx,
                 errs[worst], own_g, worst, e_s, own_s))
        assert e_y < bar_p and e_dx < bar_g, (vpad, e_y, e_dx)
        assert not {k: e for k, e in errs.items() if e > bar_g}, (vpad, errs)
        assert e_s < bar_s, (vpad, e_s)
        if not training:
            for k in state:
                if "running" in k or "num_batches" in k:
                    assert torch.equal(m.state_dict()[k].cpu(), state[k]), k


# ------------------------------------------------------------------------------------------
# 4. fused training entry points on non-canonical parameter vectors
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", (None, 0.05), ids=("noclip", "clip"))
@pytest.mark.parametrize("case", LC.trainer_cases(), ids=repr)
def test_trainer_step_against_the_oracle_step(dev, case, clip):
    """Trainer.step on a ragged batch of 64 scenes with per-scene weights (0.5 .. 1.5, divided by N) --
    stg_model_bwd_step (no clipping) / stg_model_bwd_nll + stg_train_tail (clipping) on the scene path, stg_train_tail behind the workgroup kernels for
    (2,5) -- against the oracle's step: the forward / backward loop in float64, clip_grad_norm_ and SGD in torch
    float64.  Every parameter (compared as the update it received, on the scale of the tensor's largest update; dead
    parameters bit-unchanged), every BatchNorm buffer, the reported loss and the per-scene losses."""
    from social_stgcnn_amd.trainer import Trainer
    lr = 1.0                # (one step: the update is the gradient itself, large against the fp32 ulp of a parameter)
    model, state, b = case.build()
    r64 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn)
    r32 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, dtype=torch.float32)
    own = LC.oracle_distance(r32, r64)
    bar_p, bar_l, bar_g, bar_s = LC.bars(own)
    live = [torch.from_numpy(g).clone() for g in r64.grads.values() if g is not None]
    if clip is not None:
        holders = [torch.zeros_like(g).requires_grad_(True) for g in live]
        for h, g in zip(holders, live):
            h.grad = g
        torch.nn.utils.clip_grad_norm_(holders, clip)
        live = [h.grad for h in holders]
    it = iter(live)
    upd_ref = {k: (None if g is None else (-lr * next(it)).numpy()) for k, g in r64.grads.items()}
    total_ref = sum(float(b.weights_u[i]) * l for i, l in r64.loss.items())
    m = model.to(dev).train()
    x, adj, tgt, peds, w = b.device(dev)
    tr = Trainer(m, lr=lr, clip_grad=clip)
    total, losses, y = tr.step(x, adj, tgt, peds, w)
    lc = losses.cpu().numpy()
    e_loss = max(abs(float(lc[i]) - r64.loss.get(i, 0.0)) for i in range(b.n))
    e_tot = abs(float(total) - total_ref)
    errs = {}
    for k, p in m.named_parameters():
        if upd_ref[k] is None:
            assert torch.equal(p.detach().cpu(), state[k]), k                   # dead: bit-unchanged
            continue
        after, before = p.detach().cpu().double().numpy(), state[k].double().numpy()
        # the updated parameter is stored in fp32: half an ulp of it, element by element, on top of the update's own error
        ulp = np.maximum(np.abs(after), np.abs(before)) * 2.0 ** -24
        excess = np.maximum(0.0, np.abs((after - before) - upd_ref[k]) - ulp)
        scale = max(lr * 1e-3, float(np.abs(upd_ref[k]).max()))
        if k.endswith(LC.ZERO_GRAD_BIASES):
            scale = max(scale, float(np.abs(upd_ref[k[:-4] + "weight"]).max()))
        errs[k] = float(excess.max()) / scale / (10.0 if k.endswith(LC.ZERO_GRAD_BIASES) else 1.0)
    e_stat = 0.0
    for k, val in m.state_dict().items():
        if "running" in k:
            e_stat = max(e_stat, LC.maxdiff(val.cpu().numpy(), r64.after[k].numpy()))
        if "num_batches" in k:
            assert int(val) == int(r64.after[k]), k
    worst = max(errs, key=errs.get)
    print("\ntrainer %dx%d %s: losses %.1e (fp32 oracle %.1e)  total %.1e  update %.1e (%.1e) %s  stats %.1e (%.1e)"
          % (case.n_stgcnn, case.n_txpcnn, "clip" if clip else "noclip", e_loss, own[1], e_tot, errs[worst], own[2],
             worst, e_stat, own[3]))
    assert e_loss < bar_l and e_tot < bar_l * float(np.abs(b.weights_u).sum()), (e_loss, e_tot)
    assert not {k: e for k, e in errs.items() if e > bar_g}, errs
    assert e_stat < bar_s


@pytest.mark.parametrize("case", LC.trainer_cases(), ids=repr)
def test_captured_trainer_step_on_a_non_canonical_model(dev, case):
    """Trainer.capture + three replays == three eager steps from the same start (test_captured_step_equals_eager_step's
    bound on parameters and buffers); V_pred of the first replay bit-equal to the first eager step's."""
    from social_stgcnn_amd.trainer import Trainer
    states, first = [], []
    for captured in (False, True):
        model, _, b = case.build()
        m = model.to(dev).train()
        x, adj, tgt, peds, w = b.device(dev)
        tr = Trainer(m, lr=0.05)
        step = tr.capture(x, adj, tgt, peds, w) if captured else (lambda: tr.step(x, adj, tgt, peds, w))
        for k in range(3):
            out = step()
            if k == 0:
                first.append(out[2].clone())
        torch.cuda.synchronize()
        states.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, float(out[0])))
    (a, la), (c, lb) = states
    assert torch.equal(first[0], first[1])
    assert abs(la - lb) < 1e-6
    for k in a:
        if "num_batches" in k:
            assert int(a[k]) == int(c[k]), k
        else:
            assert float((a[k] - c[k]).abs().max()) < 1e-6 * max(1.0, float(a[k].abs().max())), k


# ------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------
def test_unsupported_layouts_raise_before_any_launch(dev):
    """n_stgcnn = 5, n_txpcnn = 9 and input_feat = 3 are outside what the kernels are built for: the module call raises
    RuntimeError (STG_EUNSUPPORTED from the first size query the forward makes) and nothing is launched."""
    for kw in (dict(n_stgcnn=5, n_txpcnn=5), dict(n_stgcnn=1, n_txpcnn=9), dict(n_stgcnn=1, n_txpcnn=5, input_feat=3)):
        m = LC.make_model(kw["n_stgcnn"], kw["n_txpcnn"], kw.get("input_feat", 2)).to(dev)
        x = torch.zeros(2, kw.get("input_feat", 2), LC.T_OBS, 4, device=dev)
        adj = torch.zeros(2, LC.T_OBS, 4, 4, device=dev)
        for training in (True, False):
            m.train(training)
            with pytest.raises(RuntimeError, match="status -2"):
                m(x, adj)
            with torch.no_grad(), pytest.raises(RuntimeError, match="status -2"):
                m(x, adj)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 6. planner and launcher agree
# ------------------------------------------------------------------------------------------
GUARD = 1024
PATTERN = -12345.678


def _guarded(n_floats, dev):
    """[guard | n_floats | guard] filled with a pattern; the middle is the buffer the entry point is given."""
    buf = torch.full((GUARD + n_floats + GUARD + 4,), PATTERN, device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n_floats]


def _guards_intact(buf, n_floats):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n_floats:] == PATTERN).all())


@pytest.mark.auto_path
@pytest.mark.parametrize("layout", LC.SCENE_LAYOUTS + LC.STACKED_LAYOUTS, ids=lambda l: "%dx%d" % l)
def test_size_queries_cover_what_the_launchers_write(dev, layout):
    """Every V in 1..130 at N in {1, 300, 2048}, with and without num_peds, through the C ABI with default flags: the
    sizes stg_model_ws_floats / _ws_tail_floats / _fwd_scratch_floats / _bwd_scratch_floats report are accepted by
    stg_model_fwd + stg_model_bwd (no STG_ELDS / STG_EINVAL from a launcher), and nothing is written outside them
    (pattern-filled guard bands on both sides of the workspace and of both scratch buffers)."""
    from social_stgcnn_amd import _lib, ops
    L = _lib.lib()
    n_st, n_tx = layout
    model = LC.randomise(LC.make_model(n_st, n_tx), 5).to(dev)
    params, bufs, _, _ = model._tensors()
    flat_p, flat_b = model._pp.ensure(params), model._pb.ensure(bufs)
    d = ops.make_desc(n_st, n_tx, 2, 5, LC.T_OBS, LC.T_PRED, 3, 2, False, True, options=ops.KernelOptions())
    ref = ctypes.byref(d)
    n_par, n_stat = int(L.stg_model_param_count(ref)), int(L.stg_model_stat_floats(ref))
    nmax, vmax = 2048, 130
    g = torch.Generator().manual_seed(3)
    x_pool = torch.zeros(nmax * 2 * LC.T_OBS * vmax, device=dev)
    a_pool = torch.zeros(nmax * LC.T_OBS * vmax * vmax, device=dev)
    dy_pool = torch.zeros(nmax * 5 * LC.T_PRED * vmax, device=dev)
    y_pool = torch.empty(nmax * 5 * LC.T_PRED * vmax, device=dev)
    stats = torch.empty(nmax * max(n_stat, 1), device=dev)
    grad = torch.empty(n_par, device=dev)
    live = LC.Batch([vmax], vmax, 11, garbage=False)
    dy_live = (torch.randn(5, LC.T_PRED, vmax, generator=g) * 0.1).to(dev)
    stream = _lib.stream_ptr()
    for v in list(range(1, 129)) + [129, 130]:
        xi, ai = live.x[0, :, :, :v].to(dev), live.adj[0, :, :v, :v].to(dev)
        for n in (1, 300, 2048):
            x = x_pool[:n * 2 * LC.T_OBS * v].view(n, 2, LC.T_OBS, v)
            adj = a_pool[:n * LC.T_OBS * v * v].view(n, LC.T_OBS, v, v)
            dy = dy_pool[:n * 5 * LC.T_PRED * v].view(n, 5, LC.T_PRED, v)
            y = y_pool[:n * 5 * LC.T_PRED * v].view(n, 5, LC.T_PRED, v)
            x[0], adj[0], dy[0] = xi, ai, dy_live[:, :, :v]
            sizes = (L.stg_model_ws_floats(ref, v), L.stg_model_ws_tail_floats(ref, n, v),
                     L.stg_model_fwd_scratch_floats(ref, n, v), L.stg_model_bwd_scratch_floats(ref, n, v))
            assert min(sizes) >= 0, (layout, n, v, sizes, L.stg_last_error())
            n_ws = n * sizes[0] + sizes[1]
            for ragged in (False, True):
                peds = None
                if ragged:
                    peds = ((torch.arange(n, dtype=torch.int32) * 7) % (v + 1))
                    peds[0] = v
                    peds = peds.to(dev)
                ws_all, ws = _guarded(n_ws, dev)
                fs_all, fs = _guarded(sizes[2], dev)
                bs_all, bs = _guarded(sizes[3], dev)
                sn, sc, st, sv = x.stride()
                rc = L.stg_model_fwd(ref, _lib.ptr(flat_p), _lib.ptr(flat_b), _lib.ptr(x), sn, sc, st, sv, _lib.ptr(adj),
                                     adj.stride(0), _lib.ptr(peds), n, v, _lib.ptr(y), _lib.ptr(ws), _lib.ptr(stats),
                                     _lib.ptr(fs), None, 0, stream)
                assert rc == 0, (layout, n, v, ragged, "fwd", rc, L.stg_last_error())
                rc = L.stg_model_bwd(ref, _lib.ptr(flat_p), _lib.ptr(flat_b), _lib.ptr(x), sn, sc, st, sv, _lib.ptr(adj),
                                     adj.stride(0), _lib.ptr(peds), n, v, _lib.ptr(dy), _lib.ptr(ws), _lib.ptr(bs),
                                     _lib.ptr(grad), None, None, 0, stream)
                assert rc == 0, (layout, n, v, ragged, "bwd", rc, L.stg_last_error())
                assert _guards_intact(ws_all, n_ws), (layout, n, v, ragged, "workspace")
                assert _guards_intact(fs_all, sizes[2]), (layout, n, v, ragged, "forward scratch")
                assert _guards_intact(bs_all, sizes[3]), (layout, n, v, ragged, "backward scratch")
                assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(y).all()), (layout, n, v, ragged)
            x[0], adj[0], dy[0] = 0.0, 0.0, 0.0
