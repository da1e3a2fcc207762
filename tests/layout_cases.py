"""Shared plain module of tests/test_gpu_layouts.py and tests/test_lib_cpu.py (not a test file, no GPU needed to import):
the model layouts the library accepts, parameters drawn so that no two slots hold the same number, ragged batches with
garbage in the padded slots, and the per-scene oracle loop (oracle/stgcnn_oracle.py) in float64 and in float32.

The comparison conventions are test_gpu_parity.py's: `_grad_errors` scaling, the zero-gradient-bias rule, fp64 as the
arbiter because of the PReLU kink.  They live here so that both files use one statement of them."""
import contextlib

import numpy as np
import torch

T_OBS, T_PRED = 8, 12

# the project's own bars (test_gpu_parity.py: the fp64-oracle tests): absolute on V_pred / loss, relative on gradients
# under `grad_errors`' scaling, absolute on the BatchNorm running statistics
BAR_PRED, BAR_GRAD, BAR_STAT = 5e-5, 1e-4, 2e-6
# a different but correct summation order can land on the other side of the fp64 value and once more beyond
WIDEN = 4.0

SCENE_LAYOUTS = [(1, k) for k in range(1, 9)]                    # generic-shape scene kernels (5 = the canonical control)
STACKED_LAYOUTS = [(2, 1), (2, 5), (3, 3), (4, 8), (4, 1)]       # workgroup-per-scene kernels

# Conv biases that feed a train-mode BatchNorm have an exactly-zero true gradient (the normalisation removes any
# per-channel shift): both sides hold fp32 rounding noise of the same sum there, so they are compared on the scale of
# the sibling weight gradient, with a 10x looser bar.
ZERO_GRAD_BIASES = ("gcn.conv.bias", "tcn.2.bias", "residual.0.bias")


def maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def grad_errors(named_got, ref_of, zero_biases=ZERO_GRAD_BIASES):
    """named_got: iterable of (name, grad tensor / array or None); ref_of(name) -> numpy array or None (dead).
    Returns {name: relative error} for live parameters; asserts dead ones are None on both sides.
    zero_biases: the name endings that get the zero-gradient-bias rule (train mode; () in eval mode, where those
    biases have ordinary gradients)."""
    named_got = list(named_got)
    refs = {name: ref_of(name) for name, _ in named_got}
    out = {}
    for name, got in named_got:
        ref = refs[name]
        if ref is None:
            assert got is None, name
            continue
        assert got is not None, name
        scale = max(1e-3, float(np.abs(ref).max()))
        zero = bool(zero_biases) and name.endswith(tuple(zero_biases))
        if zero:
            sib = refs.get(name[:-4] + "weight")
            if sib is not None:
                scale = max(scale, float(np.abs(sib).max()))
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
        err = maxdiff(got, ref) / scale
        out[name] = err / 10.0 if zero else err
    return out


# ------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------
def make_model(n_stgcnn, n_txpcnn, input_feat=2):
    from social_stgcnn_amd.model import social_stgcnn
    return social_stgcnn(n_stgcnn=n_stgcnn, n_txpcnn=n_txpcnn, input_feat=input_feat, output_feat=5, seq_len=T_OBS,
                         kernel_size=3, pred_seq_len=T_PRED)


def randomise(module, seed):
    """Every parameter and buffer of `module` (still on the CPU) drawn distinct from a seeded generator, so that a read
    or write of the wrong slot changes a number: conv weights / biases uniform at their init scale 1/sqrt(fan_in),
    BatchNorm gamma in [0.5, 1.5], beta in [-0.3, 0.3], running_mean in [-0.3, 0.3], running_var in [0.3, 3],
    num_batches_tracked different per BatchNorm, every PReLU slope different, every third one negative, one above 1."""
    g = torch.Generator().manual_seed(1000 + seed)

    def uni(shape, lo, hi):
        return torch.rand(shape, generator=g) * (hi - lo) + lo
    prelus, n_bn = [], 0
    with torch.no_grad():
        for mod in module.modules():
            if isinstance(mod, torch.nn.Conv2d):
                fan_in = mod.weight[0].numel()
                b = 1.0 / fan_in ** 0.5
                mod.weight.copy_(uni(mod.weight.shape, -b, b))
                mod.bias.copy_(uni(mod.bias.shape, -b, b))
            elif isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(uni(mod.weight.shape, 0.5, 1.5))
                mod.bias.copy_(uni(mod.bias.shape, -0.3, 0.3))
                mod.running_mean.copy_(uni(mod.running_mean.shape, -0.3, 0.3))
                mod.running_var.copy_(uni(mod.running_var.shape, 0.3, 3.0))
                mod.num_batches_tracked.fill_(3 + 7 * n_bn + seed % 5)
                n_bn += 1
            elif isinstance(mod, torch.nn.PReLU):
                prelus.append(mod)
        above = seed % len(prelus)
        base = (above + 1) % len(prelus)
        for i, mod in enumerate(prelus):
            s = 0.08 + 0.5 * (i + 1) / (len(prelus) + 1) + float(uni((), 0.0, 0.04))
            if i == above:
                s = 1.1 + float(uni((), 0.0, 0.3))
            elif (i - base) % 3 == 0:
                s = -0.5 * s
            mod.weight.fill_(s)
    return module


def state_of(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


# ------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------
def ragged_counts(v, n, seed):
    """n pedestrian counts in 0..v: 0, 1, 2, v and both sides of every team-class bound (8/16, 16/32, 32/64) that fits,
    the rest uniform; shuffled (the library sorts a ragged batch itself)."""
    rng = np.random.default_rng(seed)
    must = sorted({c for c in (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, v - 1, v) if 0 <= c <= v})
    must = must[:n]
    rest = rng.integers(1, v + 1, size=max(0, n - len(must))).tolist()
    counts = np.array(must + rest, dtype=np.int32)
    rng.shuffle(counts)
    return counts


def synthetic_rel(v, seed):
    """(v, 2, 20) relative displacements rounded to 4 decimals, zero first frame (the dataset's form)."""
    rng = np.random.default_rng(seed)
    rel = np.zeros((v, 2, T_OBS + T_PRED), np.float32)
    rel[:, :, 1:] = np.round(rng.uniform(-0.6, 0.6, (v, 2, T_OBS + T_PRED - 1)), 4).astype(np.float32)
    return rel


class Batch:
    """One padded batch on the host: x (N,C,T,V), adj (N,T,V,V), tgt (N,P,V,2), counts (N,) or None (every slot live),
    weights (N,).  The U `unique` scenes are tiled to n scenes (scene i of the batch is unique scene i % U, U a prime or
    at least no divisor of a power of two in the large cases), so that the oracle only runs U scenes however large N is.
    Padded slots hold garbage."""

    def __init__(self, counts, vpad, seed, n=None, c_in=2, ragged=True, garbage=True):
        from oracle import stgcnn_oracle as O
        counts = np.asarray(counts, dtype=np.int32)
        u = len(counts)
        rng = np.random.default_rng(seed + 17)
        fill = (lambda shape: rng.uniform(-40.0, 40.0, shape).astype(np.float32)) if garbage else \
            (lambda shape: np.zeros(shape, np.float32))
        x, adj, tgt = fill((u, c_in, T_OBS, vpad)), fill((u, T_OBS, vpad, vpad)), fill((u, T_PRED, vpad, 2))
        self.scenes = []
        for i, c in enumerate(counts):
            c = int(c)
            if c == 0:
                self.scenes.append(None)
                continue
            rel = synthetic_rel(c, seed * 1000 + i)
            nodes, lap = O.seq_to_graph_np(rel[:, :, :T_OBS])
            t_i, _ = O.seq_to_graph_np(rel[:, :, T_OBS:])
            xi = np.ascontiguousarray(np.transpose(nodes, (2, 0, 1)))          # (2,T,c)
            if c_in != 2:
                xi = rng.standard_normal((c_in, T_OBS, c)).astype(np.float32) * 0.5
            x[i, :, :, :c], adj[i, :, :c, :c], tgt[i, :, :c] = xi, lap, t_i
            self.scenes.append((xi, lap, t_i))
        n = u if n is None else n
        self.unique, self.vpad = u, vpad
        self.counts_u = counts
        self.weights_u = np.linspace(0.5, 1.5, u).astype(np.float32)
        self.ragged = ragged
        if not ragged:
            assert np.all(counts == vpad)
        idx = np.arange(n) % u
        self.idx = idx
        self.mult = np.bincount(idx, minlength=u)                              # copies of every unique scene
        self.x, self.adj, self.tgt = (torch.from_numpy(a[idx]) for a in (x, adj, tgt))
        self.counts = counts[idx]
        self.weights = torch.from_numpy(self.weights_u[idx])

    @property
    def n(self):
        return len(self.idx)

    def device(self, dev):
        peds = torch.from_numpy(self.counts).to(dev) if self.ragged else None
        return self.x.to(dev), self.adj.to(dev), self.tgt.to(dev), peds, self.weights.to(dev)


# ------------------------------------------------------------------------------------------
# the oracle loop
# ------------------------------------------------------------------------------------------
def _cast(state, dtype):
    return {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in state.items()}


class OracleResult:
    pass


KINK_MARGIN = 1e-6


@contextlib.contextmanager
def kink_watch(out):
    """Records in out[0] the smallest |pre-activation| any PReLU of the oracle sees inside the block.  PReLU's
    derivative jumps at 0: a pre-activation within fp32 rounding of zero lets two correct fp32 implementations disagree
    on a gradient by O(upstream gradient), so the cases' seeds keep every pre-activation KINK_MARGIN away from it."""
    import torch.nn.functional as F
    orig = F.prelu

    def prelu(x, w):
        out[0] = min(out[0], float(x.detach().abs().min()))
        return orig(x, w)
    F.prelu = prelu
    try:
        yield out
    finally:
        F.prelu = orig


def oracle_model_step(state, batch, n_stgcnn, n_txpcnn, dtype=torch.float64, training=True, want_dx=False,
                      eval_grads=False):
    """The reference's loop over the scenes of `batch` (oracle.scene_loss, one scene at a time, N = 1) in `dtype`:
    per-scene V_pred (P,c,5) and loss for the unique scenes, the parameter gradients of sum_n w_n loss_n over the whole
    (tiled) batch, dx per unique scene (for weight w_i), and the state after the batch: the running statistics folded
    scene by scene in batch order, zero-pedestrian scenes not counted (`after_once`: after one pass over the unique
    scenes, carried through the oracle's own BatchNorm calls; `after`: after the whole tiled batch).
    training=False: V_pred and losses from the running statistics; with eval_grads also the parameter gradients (and dx)
    of the same weighted sum -- the buffers do not move, `after` / `after_once` stay None."""
    from oracle import stgcnn_oracle as O
    with_grads = training or eval_grads
    st = _cast(state, dtype)
    keys = [k for k in O.state_dict_keys(n_stgcnn, n_txpcnn) if k in st and "running" not in k and "num_batches" not in k]
    params = {k: st[k].clone().requires_grad_(with_grads) for k in keys}
    stat_keys = [k for k in st if "running" in k]
    work = {k: v.clone() for k, v in st.items()}
    work.update(params)
    res = OracleResult()
    res.pred, res.loss, res.dx, stats = {}, {}, {}, {}
    res.grads, res.after, res.after_once = None, None, None
    total = None
    keep = 1 - O.BN_MOMENTUM
    kink = [float("inf")]
    res.kink = kink
    for i in range(batch.unique):
        if batch.scenes[i] is None:
            continue
        xi, lap, t_i = batch.scenes[i]
        before = {k: work[k].clone() for k in stat_keys}
        x = torch.from_numpy(xi).to(dtype).unsqueeze(0).requires_grad_(want_dx and with_grads)
        with kink_watch(kink):
            l, vp = O.scene_loss(work, x, torch.from_numpy(lap).to(dtype), torch.from_numpy(t_i).to(dtype), training,
                                 n_stgcnn=n_stgcnn, n_txpcnn=n_txpcnn)
        res.pred[i], res.loss[i] = vp.detach().numpy(), float(l.detach())
        if not with_grads:
            continue
        if training:
            # running' = (1 - m) running + m s: the scene's own statistic s (mean / unbiased variance), for the tiled fold
            stats[i] = {k: (work[k] - keep * before[k]) / O.BN_MOMENTUM for k in stat_keys}
        w_i = float(batch.weights_u[i])
        if want_dx:
            gx, = torch.autograd.grad(l * w_i, x, retain_graph=True)
            res.dx[i] = gx[0].numpy()
        w_i *= int(batch.mult[i])
        total = l * w_i if total is None else total + l * w_i
    if with_grads:
        total.backward()
        res.grads = {k: (None if params[k].grad is None else params[k].grad.numpy()) for k in keys}
    if training:
        res.after_once = {k: v.detach().clone() for k, v in work.items() if k not in params}
        after = {k: v.clone() for k, v in res.after_once.items()}
        if batch.n > batch.unique and dtype != torch.float64:
            after = None                               # (the recovered statistics need float64)
        elif batch.n > batch.unique:
            live = 0
            for i in batch.idx[batch.unique:]:
                if batch.scenes[i] is None:
                    continue
                live += 1
                for k in stat_keys:
                    after[k] = keep * after[k] + O.BN_MOMENTUM * stats[i][k]
            for k in after:
                if "num_batches" in k:
                    after[k] = after[k] + live
        res.after = after
    return res


def make_block(c_in, residual, use_mdn):
    from social_stgcnn_amd.model import st_gcn
    return st_gcn(c_in, 5, (3, T_OBS), use_mdn=use_mdn, residual=residual)


def oracle_block_step(state, batch, gy, training, use_mdn, residual, dtype=torch.float64):
    """oracle.st_gcn_forward over the scenes of `batch` (no tiling), loss_i = sum(y_i * gy[i]) on the valid block:
    per-scene output (5,T,c) and dx (C,T,c), summed parameter gradients (None where autograd never reaches the
    parameter), buffers after the batch.  residual: 'conv', 'identity' or 'zero'."""
    from oracle import stgcnn_oracle as O
    st = {"b." + k: v for k, v in _cast(state, dtype).items()}
    keys = [k for k in st if "running" not in k and "num_batches" not in k]
    params = {k: st[k].clone().requires_grad_(True) for k in keys}
    work = {k: v.clone() for k, v in st.items()}
    work.update(params)
    res = OracleResult()
    res.pred, res.dx, res.kink = {}, {}, [float("inf")]
    total = None
    for i in range(batch.unique):
        if batch.scenes[i] is None:
            continue
        xi, lap, _ = batch.scenes[i]
        c = xi.shape[2]
        x = torch.from_numpy(xi).to(dtype).unsqueeze(0).requires_grad_(True)
        with kink_watch(res.kink):
            y = O.st_gcn_forward(work, "b", x, torch.from_numpy(lap).to(dtype), training, use_mdn=use_mdn,
                                 residual=residual)
        l = (y[0] * torch.from_numpy(gy[i, :, :, :c]).to(dtype)).sum()
        gx, = torch.autograd.grad(l, x, retain_graph=True)
        res.pred[i], res.dx[i] = y[0].detach().numpy(), gx[0].numpy()
        total = l if total is None else total + l
    total.backward()
    res.grads = {k[2:]: (None if params[k].grad is None else params[k].grad.numpy()) for k in keys}
    res.after = {k[2:]: v.detach().clone() for k, v in work.items() if k not in params}
    return res


def oracle_distance(r32, r64):
    """The float32 oracle's distance to the float64 oracle in the metrics the tests assert:
    (V_pred abs, loss abs, gradient relative under grad_errors, running statistics abs)."""
    pred = max([maxdiff(r32.pred[i], r64.pred[i]) for i in r64.pred] + [0.0])
    loss = max([abs(r32.loss[i] - r64.loss[i]) for i in r64.loss] + [0.0])
    grad = stat = 0.0
    if r64.grads is not None:
        errs = grad_errors(((k, r32.grads[k]) for k in r64.grads), lambda k: r64.grads[k],
                           ZERO_GRAD_BIASES if r64.after_once is not None else ())
        grad = max(errs.values())
    if r64.after_once is not None:
        stat = max(maxdiff(r32.after_once[k].numpy(), r64.after_once[k].numpy()) for k in r64.after_once
                   if "running" in k)
    return pred, loss, grad, stat


def bars(dist):
    """(V_pred, loss, gradient, running statistics) bars of one case: max(project bar, 4 x the fp32 oracle's own
    distance to the fp64 oracle)."""
    p, l, g, s = dist
    return (max(BAR_PRED, WIDEN * p), max(BAR_PRED, WIDEN * l), max(BAR_GRAD, WIDEN * g), max(BAR_STAT, WIDEN * s))


# ------------------------------------------------------------------------------------------
# the case table of the training-step matrix: built on the CPU, run on the GPU
# ------------------------------------------------------------------------------------------
RAGGED_V = (17, 32, 57, 100, 128)
_TWO = {2: (17, 100), 4: (32, 128), 5: (57, 32), 6: (100, 17), 7: (128, 57)}
_RAGGED_N = {12: 16, 17: 24, 32: 28, 57: 32, 96: 20, 100: 36, 128: 40}


class Case:
    """One training-step case: layout, batch geometry, kernel options; `build()` -> (model on the CPU, its state, Batch)."""

    def __init__(self, group, n_stgcnn, n_txpcnn, vpad, counts, n=None, ragged=True, options=None, tag="",
                 mean_weights=False):
        self.group, self.n_stgcnn, self.n_txpcnn, self.vpad = group, n_stgcnn, n_txpcnn, vpad
        self.counts, self.n, self.ragged, self.options = counts, n, ragged, dict(options or {})
        self.mean_weights = mean_weights           # per-scene weights divided by N (a trainer's group mean)
        n_all = n or (counts.n if callable(counts) else len(counts))
        self.id = "%s-%dx%d-V%d-N%d%s" % (group, n_stgcnn, n_txpcnn, vpad, n_all, tag)
        key = [ord(c) for c in group] + [n_stgcnn, n_txpcnn, vpad, n_all]
        s = 7
        for k in key:
            s = (s * 131 + int(k)) % 100003
        self.seed = s + SEED_SHIFT.get(self.id, 0)

    def build(self):
        counts = self.counts(self.seed) if callable(self.counts) else self.counts
        model = randomise(make_model(self.n_stgcnn, self.n_txpcnn), self.seed)
        batch = Batch(counts, self.vpad, self.seed, n=self.n, ragged=self.ragged)
        if self.mean_weights:
            batch.weights_u = batch.weights_u / np.float32(batch.n)
            batch.weights = batch.weights / batch.n
        return model, state_of(model), batch

    def __repr__(self):
        return self.id


def ragged(v, n=None):
    def counts(seed):
        return ragged_counts(v, counts.n, seed)
    counts.n = n or _RAGGED_N[v]
    return counts


def scene_path_cases():
    """Every one-block case (the scene path and, beyond 128 pedestrians, the workgroup kernels under a generic layout)."""
    out = []
    # ragged, the planner chooses: all five geometries for n_txpcnn 1, 3, 8, two for every other layout
    for k in range(1, 9):
        for v in (RAGGED_V if k in (1, 3, 8) else _TWO[k]):
            out.append(Case("ragged", 1, k, v, ragged(v)))
    # small N: the weight-gradient item loop is one round
    for k in (1, 3, 8):
        out.append(Case("small", 1, k, 32, [32], ragged=False))
        out.append(Case("small", 1, k, 32, [32, 0, 11]))
        out.append(Case("small", 1, k, 32, ragged(32, 8)))
        out.append(Case("small", 1, k, 32, ragged(32, 40)))
    # large uniform batch, no num_peds: the solo Generic kernel at both workgroup widths (37 distinct scenes tiled)
    for k in (3, 8):
        for n in (1536, 2048):
            out.append(Case("uniform", 1, k, 32, [32] * 37, n=n, ragged=False))
    # ragged batches in the 16/32 and 32/64 team-class bounds (41 distinct scenes tiled)
    for k in (3, 8):
        for n in (400, 1536):
            out.append(Case("tiled", 1, k, 100, ragged(100, 41), n=n))
    # storage / MFMA variants of the wave-per-scene kernels under a generic layout
    for k in (3, 8):
        out.append(Case("bf16", 1, k, 57, ragged(57), options={"bf16_store": True, "wave_path": True}))
    for opt in ("f32_mfma", "split_bf16"):
        out.append(Case("wavef32", 1, 3, 57, ragged(57), options={opt: True, "wave_path": True}, tag="-" + opt))
    # beyond kTeamMaxV: the workgroup-per-scene kernels with a non-canonical one-block model
    out.append(Case("wide", 1, 3, 130, [130, 77, 129]))
    return out


def stacked_cases():
    out = []
    for (b, k) in STACKED_LAYOUTS:
        for v in (12, 57, 96):
            out.append(Case("stacked", b, k, v, ragged(v)))
    out.append(Case("stacked", 2, 5, 130, [130, 77, 129]))
    for w in (1, 8):
        out.append(Case("stacked", 2, 5, 57, ragged(57), options={"wg_waves": w}, tag="-w%d" % w))
    return out


def trainer_cases():
    """Trainer.step / Trainer.capture: a ragged batch of 64 scenes with per-scene weights, scene path and workgroup path."""
    return [Case("trainer", b, k, 40, ragged(40, 64), mean_weights=True) for (b, k) in ((1, 3), (1, 8), (2, 5))]


def eval_backward_cases():
    """Full-model backward in eval mode (running statistics, `bn_mode` 0): one ragged batch of 20 scenes per geometry,
    padded to 57 on the scene path and to 57 and 96 under the stacked layouts."""
    out = [Case("evalbwd", 1, k, 57, ragged(57, 20)) for k in (3, 5, 8)]
    for (b, k) in ((2, 5), (4, 8)):
        out += [Case("evalbwd", b, k, v, ragged(v, 20)) for v in (57, 96)]
    return out


# seeds moved off the PReLU kink: in the float64 oracle of every case no pre-activation lies within KINK_MARGIN of zero,
# and the float32 oracle sits inside the project bars (test_lib_cpu.py::test_layout_cases_fp32_oracle_inside_project_bars)
SEED_SHIFT = {
    "bf16-1x8-V57-N32": 1, "ragged-1x1-V128-N40": 1, "ragged-1x3-V100-N36": 2, "ragged-1x3-V128-N40": 9,
    "ragged-1x4-V128-N40": 8, "ragged-1x6-V100-N36": 8, "ragged-1x7-V128-N40": 30, "ragged-1x8-V100-N36": 20,
    "ragged-1x8-V128-N40": 67, "ragged-1x8-V32-N28": 2, "ragged-1x8-V57-N32": 2, "small-1x3-V32-N40": 2,
    "stacked-2x1-V12-N16": 1, "stacked-2x1-V96-N20": 2, "stacked-2x5-V12-N16": 1, "stacked-2x5-V57-N32": 3,
    "stacked-2x5-V57-N32-w1": 3, "stacked-2x5-V57-N32-w8": 3, "stacked-3x3-V96-N20": 3, "stacked-4x1-V96-N20": 1,
    "stacked-4x8-V12-N16": 2, "stacked-4x8-V57-N32": 5, "stacked-4x8-V96-N20": 7, "tiled-1x3-V100-N1536": 4,
    "tiled-1x3-V100-N400": 2, "tiled-1x8-V100-N1536": 14, "tiled-1x8-V100-N400": 37, "trainer-1x8-V40-N64": 10,
    "trainer-2x5-V40-N64": 5, "uniform-1x3-V32-N1536": 3, "uniform-1x3-V32-N2048": 3, "uniform-1x8-V32-N1536": 26,
    "uniform-1x8-V32-N2048": 2,
    # eval-mode backward (test_exact_probes_cpu.py::test_eval_backward_cases_fp32_oracle_inside_project_bars)
    "evalbwd-1x3-V57-N20": 1, "evalbwd-2x5-V96-N20": 2, "evalbwd-4x8-V96-N20": 1,
}
