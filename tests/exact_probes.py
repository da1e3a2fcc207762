"""Shared plain module of tests/test_exact_probes_cpu.py and tests/test_gpu_exact_probes.py (not a test file, no GPU
needed to import): EXACT-CLASS PROBES of the convolutions inside the scene kernels.

The scene kernels run their convolutions on the bf16 matrix pipe with every fp32 operand split into three bf16 pieces
(txp_conv_bf16.hpp) and six of the nine piece products kept.  A probe is a full set of model parameters, running
statistics and a batch (x, adj, num_peds) built so that, in eval mode, the float64 oracle's V_pred is exactly
representable in float32 and is reached exactly by ANY float32 evaluation order -- so the device result is compared
with torch.equal, and a lost low-order product, a wrong piece in one K slot or an image read at the wrong offset
changes a bit.

Construction:
  * BatchNorm: running_var = float32(s - float32(1e-5)), s in {0.25, 1, 4, 16}: var + eps == s in float32, the scale
    1/sqrt(s) is 2, 1, 0.5, 0.25 exactly, and gamma = +-sqrt(s) makes the net scale +-1.  The float64 oracle gets the
    double s - 1e-5.  Means, betas and biases sit on the grid 0.25 Z.
  * every convolution but the FOCUS is transparent: a 1x1 / centre-tap selection with weights +-1, or all zero (a
    residual TXP layer, or the h branch of a stacked st_gcn block, then passes its input on);
  * upstream of the focus every additive constant is zero and every data-carrying PReLU slope is +-1, so the data that
    meets the focus weights is +-x element by element; downstream the constants are non-zero grid values and the first
    data-carrying slope is 0.5 or 2;
  * at the focus the weights are dense and (weights, data) come from one operand class (CLASSES below).

`probe_budget` checks on the host, per convolution / aggregation / BatchNorm / residual add of the model, the two
conditions that make a probe valid: dropped products vanish, and sum |W| |x| + |bias| < 2^24 q.

BACKWARD probes (make_probe(..., backward=N)) put the class on the focus's input-gradient convolution: (weights, dz).
Their dy is sparse -- every parameter gradient is a sum over positions and scenes and has its own budget
(`probe_budget_bwd`) -- and the expectation is torch autograd on the float64 oracle from that dy.

Outside the exact class by design: `split_bf16` (two-piece operands) and `bf16_store` (bf16 saved planes); train mode.
"""
import contextlib

import numpy as np
import torch

T_OBS, T_PRED, C_OUT = 8, 12, 5
GRID = 0.25
BN_S = (0.25, 1.0, 4.0, 16.0)
SLOPES = (1.0, 0.5, 2.0, -1.0)
CLASSES = ("w_wide", "data_wide", "medium")
KEPT = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))          # (W piece, x piece): h = 0, m = 1, l = 2
DROPPED = ((1, 2), (2, 1), (2, 2))


# ------------------------------------------------------------------------------------------
# host arithmetic of the kernels' operands
# ------------------------------------------------------------------------------------------
def split3(x):
    """txp_conv_bf16.hpp split3 in numpy float32: truncation splits, x == h + m + l exactly."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = (x - h).astype(np.float32)
    m = (r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    l = (r - m).astype(np.float32)
    return h, m, l


def _conv64(W, x):
    """sum_{ci,kh,kw} W[co,ci,kh,kw] x[ci, h + kh - ph, w + kw - pw] in float64, zero padding ((kh-1)/2, (kw-1)/2)."""
    W, x = np.asarray(W, np.float64), np.asarray(x, np.float64)
    co, ci, kh, kw = W.shape
    _, H, Wd = x.shape
    xp = np.zeros((ci, H + kh - 1, Wd + kw - 1))
    xp[:, kh // 2:kh // 2 + H, kw // 2:kw // 2 + Wd] = x
    out = np.zeros((co, H, Wd))
    for a in range(kh):
        for b in range(kw):
            out += np.einsum("oc,chw->ohw", W[:, :, a, b], xp[:, a:a + H, b:b + Wd])
    return out


def conv6(W, x, keep=KEPT, bias=None, absolute=False):
    """The kernels' convolution as the sum of the selected piece products, in float64.  W (co,ci,kh,kw) and
    x (ci,H,W) are float32 values; keep: pairs (W piece, x piece)."""
    wp, xp = split3(W), split3(x)
    f = np.abs if absolute else (lambda a: a)
    out = None
    for (i, j) in keep:
        t = _conv64(f(wp[i]), f(xp[j]))
        out = t if out is None else out + t
    if bias is not None:
        out = out + f(np.asarray(bias, np.float64))[:, None, None]
    return out


def quantum(*arrays):
    """The largest power of two dividing every non-zero element (inf for all-zero input)."""
    q = np.inf
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        a = a[a != 0]
        if a.size == 0:
            continue
        m, e = np.frexp(np.abs(a))                       # a = m 2^e, m in [0.5, 1): m 2^53 is an integer
        mi = (m * 2.0 ** 53).astype(np.int64)
        tz = np.zeros(mi.shape, np.int64)
        for s in (32, 16, 8, 4, 2, 1):
            z = (mi & ((1 << s) - 1)) == 0
            tz += np.where(z, s, 0)
            mi = np.where(z, mi >> s, mi)
        q = min(q, float(2.0 ** (e - 53 + tz).min()))
    return q


def top_piece(a):
    """index of the last non-zero piece of every element (0: h only .. 2: l non-zero; -1 for zero)"""
    h, m, l = split3(a)
    return np.where(l != 0, 2, np.where(m != 0, 1, np.where(h != 0, 0, -1)))


# ------------------------------------------------------------------------------------------
# operand classes
# ------------------------------------------------------------------------------------------
def _values(rng, shape, kind, exp):
    """kind 'bit': +-2^exp; 'wide': +-(h + m + l) 2^exp, h = 1 + a/128 (a < 32), m = 2^-8 (1 + b/128), l = 2^-16
    (17 significant bits, all three pieces non-zero); 'medium': +-(h + 2^-8) 2^exp (9 bits, h and m non-zero)."""
    sign = rng.choice([-1.0, 1.0], size=shape)
    if kind == "bit":
        mag = np.ones(shape)
    else:
        mag = 1.0 + rng.integers(0, 32, size=shape) / 128.0
        if kind == "wide":
            mag = mag + 2.0 ** -8 * (1.0 + rng.integers(0, 128, size=shape) / 128.0) + 2.0 ** -16
        else:
            mag = mag + 2.0 ** -8
    v = (sign * mag * 2.0 ** exp).astype(np.float32)
    assert np.all(v.astype(np.float64) == sign * mag * 2.0 ** exp)
    return v


W_KIND = {"w_wide": "wide", "data_wide": "bit", "medium": "medium"}
X_KIND = {"w_wide": "bit", "data_wide": "wide", "medium": "medium"}


def focuses(n_txpcnn):
    """the convolutions a probe can focus on: the first block's three, every live TXP layer, the output conv"""
    return ["gcn", "tcn", "res"] + ["txp%d" % j for j in range(max(1, n_txpcnn - 1))] + ["out"]


def _stage(focus):
    return {"gcn": 0, "res": 0, "tcn": 1, "out": 1000}.get(focus) if not focus.startswith("txp") else 10 + int(focus[3:])


class Probe:
    """state: float32 state_dict (what the device model loads); state64: the oracle's (running_var = s - 1e-5 in
    double); scenes[i] = (x (2,T,c) float32, adj (T,c,c) float32) or None for an empty scene; expected[i]: float32
    V_pred (5,P,c)."""

    def __repr__(self):
        return self.id


def bwd_focuses(n_txpcnn):
    """backward probes: the input-gradient convolution of every live TXP layer and of the output conv, and the block's
    backward through its temporal conv (the gcn and residual convs have no input gradient but dx)"""
    return ["tcn"] + ["txp%d" % j for j in range(max(1, n_txpcnn - 1))] + ["out"]


N_DY = 8             # non-zero elements of dy in one backward probe (see make_probe)


def dy_columns(c):
    """the columns of a scene of c pedestrians where addressing changes: the two borders and both sides of every chunk
    bound of a team of two or four waves (chunks of ceil(c / nch) columns, scene_team.hpp)"""
    cols = {0, c - 1}
    for nch in (2, 4):
        wc = -(-c // nch)
        for k in range(1, nch):
            cols |= {e for e in (k * wc - 1, k * wc) if 0 <= e < c}
    return sorted(cols)


def _dy_positions(rng, c, m):
    """m distinct elements (c_out, t, v) of V_pred (5,P,c): the column from dy_columns(c) or anywhere in the scene, the
    channel and the row of the (12, 5, c) image the output conv writes (V_pred is a view of it) drawn"""
    where = []
    while len(where) < m:
        v = int(rng.choice(dy_columns(c))) if rng.random() < 0.6 else int(rng.integers(c))
        flat = int(rng.integers(T_PRED)) * C_OUT + int(rng.integers(C_OUT))
        pos = (flat // T_PRED, flat % T_PRED, v)
        if pos not in where:
            where.append(pos)
    return where


def make_probe(n_stgcnn, n_txpcnn, focus, cls, counts, seed, backward=None, cut=True):
    """backward: None for a forward probe, or the batch size N of a backward probe (scene n of the batch is unique
    scene n % len(counts)).

    A BACKWARD probe puts the operand class on (focus weights, dz at the focus).  Every parameter gradient is a sum over
    positions and scenes, and a sum of 17- to 24-bit gradients over a dense scene cannot stay below 2^24 quanta, so dy
    is sparse: N_DY non-zero elements in at most four scenes (the first, the last, two interior ones), at positions drawn
    anew for every probe and scene (_dy_positions: every channel and row, the border columns, both sides of the team
    chunk bounds, interior columns; test_exact_probes_cpu.py asserts the coverage over the probes of a focus).  The forward
    is cut by an all-zero convolution below the focus (the first block's gcn and residual convs for the focuses tcn and
    txp0, TXP layer 0 otherwise): below the cut the activations are +-x (one bit), from the cut to the focus they are
    zero, behind the focus they are per-channel constants.  The gradient that leaves the focus convolution reaches the
    cut unchanged but for signs and power-of-two slopes, and the weight gradient of the cut convolution --
    sum_pos dz[co,pos] x[ci,pos+tap], non-zero although the weights are zero -- sees every element of it by position.
    cut=False (focus tcn only) leaves the +-1 selections of the gcn and residual convs in place: the forward carries +-x
    through the focus, and dx is not zero."""
    from oracle import stgcnn_oracle as O
    assert focus in (focuses(n_txpcnn) if backward is None else bwd_focuses(n_txpcnn)) and cls in CLASSES
    rng = np.random.default_rng([seed, n_stgcnn, n_txpcnn, focuses(8).index(focus) if focus != "out" else 99,
                                 CLASSES.index(cls)] + ([] if backward is None else [1 if cut else 2]))
    fs = _stage(focus)
    kx = int(rng.integers(-1, 3))                        # data exponent
    ew = -kx + int(rng.integers(0, 3))                   # focus-weight exponent: products at 2^0 .. 2^2
    if focus.startswith("txp") and focus != "txp0":
        # a residual layer adds its 108-term sum to its own input: the sum must stay below 2^24 quanta of the DATA, so
        # the weights are of size 1 or 0.5 (and the data of size 1 .. 4, the grid constants small beside them)
        kx, ew = int(rng.integers(0, 3)), int(rng.integers(-1, 1))
    st = {}

    def const(shape, stage):
        """additive constants: zero upstream of the focus, non-zero grid values from the focus on"""
        if stage < fs:
            return np.zeros(shape, np.float32)
        return (rng.choice([-1.0, 1.0], size=shape) * rng.integers(1, 5, size=shape) * GRID).astype(np.float32)

    def bn(prefix, stage):
        s = rng.choice(BN_S, size=C_OUT)
        st[prefix + ".running_var"] = (s.astype(np.float32) - np.float32(1e-5)).astype(np.float32)
        st[prefix + ".running_var64"] = s - 1e-5
        st[prefix + ".weight"] = (rng.choice([-1.0, 1.0], size=C_OUT) * np.sqrt(s)).astype(np.float32)
        st[prefix + ".bias"] = const(C_OUT, stage)
        st[prefix + ".running_mean"] = const(C_OUT, stage)
        st[prefix + ".num_batches_tracked"] = np.int64(rng.integers(1, 50))

    def select(shape, src):
        """a 1x1 / centre-tap selection: output row r takes input channel src[r] with weight +-1"""
        w = np.zeros(shape, np.float32)
        for r in range(shape[0]):
            w[(r, src[r]) + tuple(k // 2 for k in shape[2:])] = rng.choice([-1.0, 1.0])
        return w

    def cover(n_out, n_in):
        src = np.concatenate([rng.permutation(n_in), rng.integers(0, n_in, size=max(0, n_out - n_in))])[:n_out]
        return rng.permutation(src)

    def dense(shape):
        return _values(rng, shape, W_KIND[cls], ew)

    def slope(stage, carries_data):
        if not carries_data:
            return float(rng.choice(SLOPES))
        if stage < fs:
            return float(rng.choice([1.0, -1.0]))
        return None                                       # (filled below: the first one downstream is 0.5 or 2)

    data_slopes = []                                      # (stage, key) of the data-carrying PReLUs from the focus on
    for b in range(n_stgcnn):
        p = "st_gcns.%d." % b
        cin = 2 if b == 0 else C_OUT
        first = b == 0
        if first:
            st[p + "gcn.conv.weight"] = dense((C_OUT, cin, 1, 1)) if focus == "gcn" else select((C_OUT, cin, 1, 1), cover(C_OUT, cin))
            st[p + "tcn.2.weight"] = dense((C_OUT, C_OUT, 3, 1)) if focus == "tcn" else select((C_OUT, C_OUT, 3, 1), cover(C_OUT, C_OUT))
            sg, stc, sb = 0, 1, 1
        else:
            # a stacked block passes its input on through the identity residual: the h branch carries constants only
            st[p + "gcn.conv.weight"] = np.zeros((C_OUT, cin, 1, 1), np.float32)
            st[p + "tcn.2.weight"] = select((C_OUT, C_OUT, 3, 1), cover(C_OUT, C_OUT))
            sg = stc = sb = 2
        st[p + "gcn.conv.bias"] = const(C_OUT, sg)
        bn(p + "tcn.0", sg)
        s1 = slope(sg, first)
        if s1 is None:
            data_slopes.append(p + "tcn.1.weight")
        st[p + "tcn.1.weight"] = np.float32(s1 if s1 is not None else 1.0)
        st[p + "tcn.2.bias"] = const(C_OUT, stc)
        bn(p + "tcn.3", stc)
        if first:
            # the residual branch runs beside gcn / tcn: it carries +-x only where the focus is inside the block
            if focus == "res":
                st[p + "residual.0.weight"] = dense((C_OUT, cin, 1, 1))
            elif fs <= 1:
                st[p + "residual.0.weight"] = select((C_OUT, cin, 1, 1), cover(C_OUT, cin))
            else:
                st[p + "residual.0.weight"] = np.zeros((C_OUT, cin, 1, 1), np.float32)
            st[p + "residual.0.bias"] = const(C_OUT, 0 if focus == "res" else sb)
            bn(p + "residual.1", 0 if focus == "res" else sb)
        s2 = slope(sb, True)
        if s2 is None:
            data_slopes.append(p + "prelu.weight")
        st[p + "prelu.weight"] = np.float32(s2 if s2 is not None else 1.0)
    hidden = max(1, n_txpcnn - 1)
    for j in range(n_txpcnn):
        cin = T_OBS if j == 0 else T_PRED
        name = "txp%d" % j
        live = j < hidden
        if focus == name:
            w = dense((T_PRED, cin, 3, 3))
        elif j == 0:
            w = select((T_PRED, cin, 3, 3), cover(T_PRED, cin))
        elif live:
            w = np.zeros((T_PRED, cin, 3, 3), np.float32)
        else:
            w = (rng.integers(-3, 4, size=(T_PRED, cin, 3, 3)) * GRID).astype(np.float32)     # never read
        st["tpcnns.%d.weight" % j] = w
        st["tpcnns.%d.bias" % j] = const(T_PRED, 10 + j)
        carries = live and (j == 0 or focus == name)
        sj = slope(10 + j, carries)
        if sj is None:
            data_slopes.append("prelus.%d.weight" % j)
        st["prelus.%d.weight" % j] = np.float32(sj if sj is not None else 1.0)
    st["tpcnn_ouput.weight"] = dense((T_PRED, T_PRED, 3, 3)) if focus == "out" else \
        select((T_PRED, T_PRED, 3, 3), rng.permutation(T_PRED))
    st["tpcnn_ouput.bias"] = const(T_PRED, 1000)
    # data-carrying slopes from the focus on: the first is 0.5 or 2, the others +-1 -- every slope off +-1 costs one bit
    # of the 24, and a dense residual TXP layer (108 terms of 17 bits, its output added to its input) has none to
    # spare: its slope is -1
    for i, key in enumerate(data_slopes):
        if i == 0:
            hidden_focus = focus.startswith("txp") and focus != "txp0"
            st[key] = np.float32(-1.0 if hidden_focus else rng.choice([0.5, 2.0]))
        else:
            st[key] = np.float32(rng.choice([1.0, -1.0]))
    if not data_slopes:
        # (focus = output conv: no PReLU behind it) one upstream data slope is -1, so that not all are 1
        st["prelus.0.weight"] = np.float32(-1.0)
    if backward is not None:
        p0 = "st_gcns.0."
        cut_keys = [p0 + "gcn.conv.weight", p0 + "residual.0.weight"] if focus in ("tcn", "txp0") else ["tpcnns.0.weight"]
        assert cut or focus == "tcn"
        for key in (cut_keys if cut else []):
            st[key] = np.zeros_like(st[key])
        # slopes: any of the four (below the focus z == 0 everywhere: the slope scales the whole gradient image; behind it
        # z is a per-channel constant); the focus layer's own is +-1, the one place where two scalings would mix in a sum
        keys = [k for k in st if k.endswith(("prelu.weight", "tcn.1.weight")) or k.startswith("prelus.")]
        for key in keys:
            st[key] = np.float32(rng.choice(SLOPES))
        if focus.startswith("txp"):
            st["prelus.%d.weight" % int(focus[3:])] = np.float32(rng.choice([1.0, -1.0]))
        if all(float(st[k]) == 1.0 for k in keys):
            st[keys[0]] = np.float32(2.0)

    pr = Probe()
    pr.n_stgcnn, pr.n_txpcnn, pr.focus, pr.cls, pr.seed = n_stgcnn, n_txpcnn, focus, cls, seed
    pr.counts = np.asarray(counts, np.int32)
    pr.id = "%dx%d-%s-%s-s%d%s" % (n_stgcnn, n_txpcnn, focus, cls, seed, "" if backward is None else "-bwd")
    pr.backward, pr.cut = backward, cut
    pr.kx, pr.ew = kx, ew
    pr.state, pr.state64 = {}, {}
    for k, v in st.items():
        if k.endswith("running_var64"):
            continue
        t = torch.from_numpy(np.atleast_1d(np.asarray(v))).clone()
        if "num_batches" in k:
            t = t.reshape(())
        pr.state[k] = t
        pr.state64[k] = t.double() if t.is_floating_point() else t.clone()
        if k.endswith("running_var"):
            pr.state64[k] = torch.from_numpy(st[k + "64"]).clone()
    # (the oracle's key list names a residual conv for every block; the model only builds the first block's)
    assert set(pr.state) <= set(O.state_dict_keys(n_stgcnn, n_txpcnn))
    pr.focus_key = {"gcn": "st_gcns.0.gcn.conv.weight", "tcn": "st_gcns.0.tcn.2.weight", "res": "st_gcns.0.residual.0.weight",
                    "out": "tpcnn_ouput.weight"}.get(focus) or "tpcnns.%d.weight" % int(focus[3:])
    # scenes: x of the class's data kind at one exponent, dense (every row and column of the scene carries data);
    # adjacency: identity, or sparse small integers where the focus is the graph convolution and in the uncut backward
    # family (the aggregation's backward then runs on a non-identity adjacency)
    pr.scenes = []
    for c in pr.counts:
        c = int(c)
        if c == 0:
            pr.scenes.append(None)
            continue
        x = _values(rng, (2, T_OBS, c), X_KIND[cls] if backward is None else "bit", kx)
        adj = np.broadcast_to(np.eye(c, dtype=np.float32), (T_OBS, c, c)).copy()
        if (focus == "gcn" or not cut) and c > 1:
            for t in range(T_OBS):
                for w in range(c):
                    v = int(rng.integers(0, c))
                    if v != w:
                        adj[t, v, w] = float(rng.choice([-1.0, 1.0, 2.0] if focus == "gcn" else [-1.0, 1.0]))
        pr.scenes.append((x, adj))
    if backward is None:
        _oracle(pr)
        return pr
    # dy: N_DY elements of the class's data kind in at most four scenes of the batch
    n, u = int(backward), len(pr.counts)
    assert pr.counts[0] > 0 and pr.counts[(n - 1) % u] > 0, "the first and the last scene of the batch carry dy"
    inner = [k for k in range(1, n - 1) if pr.counts[k % u] > 0]
    chosen = sorted({0, n - 1} | set(int(k) for k in rng.choice(inner, size=min(2, len(inner)), replace=False)))
    kd = int(rng.integers(-1, 3))
    pr.dy = {}
    for s_i, k in enumerate(chosen):
        c = int(pr.counts[k % u])
        m = N_DY // len(chosen) + (1 if s_i < N_DY % len(chosen) else 0)
        where = _dy_positions(rng, c, m)
        pr.dy[k] = (np.array(where, np.int64), _values(rng, (len(where),), X_KIND[cls], kd))
    _oracle_bwd(pr)
    return pr


# ------------------------------------------------------------------------------------------
# the oracle run: expectation and the record of every operation
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recording(state, log):
    """Records what every conv2d / matmul / batch_norm of the oracle sees (float64 numpy) while the block runs."""
    import torch.nn.functional as F
    names = {id(v): k for k, v in state.items()}
    o_conv, o_mm, o_bn, o_prelu = F.conv2d, torch.matmul, F.batch_norm, F.prelu

    def hooked(y):
        """the gradient that reaches y (when the oracle runs under autograd), left in the record's last field"""
        holder = {}
        if y.requires_grad:
            y.register_hook(lambda g: holder.__setitem__("g", g.detach().numpy().copy()))
        return holder

    def conv2d(x, w, b=None, *a, **kw):
        y = o_conv(x, w, b, *a, **kw)
        log.append(("conv", names[id(w)], w.detach().numpy(), x.detach()[0].numpy(),
                    None if b is None else b.detach().numpy(), y.detach()[0].numpy(), hooked(y)))
        return y

    def prelu(x, w):
        y = o_prelu(x, w)
        log.append(("prelu", names[id(w)], w.detach().numpy(), x.detach()[0].numpy(), None, y.detach()[0].numpy(),
                    hooked(y)))
        return y

    def matmul(g, a):
        y = o_mm(g, a)
        log.append(("agg", "agg", a.detach().numpy(), g.detach().numpy(), None, y.detach().numpy(), hooked(y)))
        return y

    def batch_norm(x, mean, var, weight, bias, training, momentum, eps):
        y = o_bn(x, mean, var, weight, bias, training, momentum, eps)
        log.append(("bn", names[id(weight)], (weight / torch.sqrt(var + eps)).detach().numpy(), x.detach()[0].numpy(),
                    (mean.detach().numpy(), bias.detach().numpy()), y.detach()[0].numpy(), hooked(y)))
        return y
    F.conv2d, torch.matmul, F.batch_norm, F.prelu = conv2d, matmul, batch_norm, prelu
    try:
        yield log
    finally:
        F.conv2d, torch.matmul, F.batch_norm, F.prelu = o_conv, o_mm, o_bn, o_prelu


def _check_log(pr, log):
    """the record holds exactly the operations of the model, each under its own parameter's name: a matmul or a
    convolution the recorder did not expect (every matmul is logged as the aggregation) fails here"""
    hidden = max(1, pr.n_txpcnn - 1)
    kinds = [e[0] for e in log]
    want = {"conv": 2 * pr.n_stgcnn + 1 + hidden + 1, "agg": pr.n_stgcnn, "bn": 2 * pr.n_stgcnn + 1,
            "prelu": 2 * pr.n_stgcnn + hidden}
    assert {k: kinds.count(k) for k in want} == want and len(log) == sum(want.values()), (pr, kinds)
    named = [e[1] for e in log if e[0] != "agg"]
    assert len(set(named)) == len(named) and all(n in pr.state for n in named), (pr, named)


def _oracle(pr):
    """float64 oracle over the scenes: pr.expected (float32, asserted representable), pr.logs (the operation records)."""
    from oracle import stgcnn_oracle as O
    pr.expected, pr.logs = {}, {}
    for i, sc in enumerate(pr.scenes):
        if sc is None:
            continue
        x, adj = sc
        log = []
        with torch.no_grad(), _recording(pr.state64, log):
            y = O.social_stgcnn_forward(pr.state64, torch.from_numpy(x).double().unsqueeze(0),
                                        torch.from_numpy(adj).double(), False, n_stgcnn=pr.n_stgcnn,
                                        n_txpcnn=pr.n_txpcnn)[0].numpy()
        _check_log(pr, log)
        y32 = y.astype(np.float32)
        assert np.all(np.abs(y - y32.astype(np.float64)) <= 1e-12 * np.abs(y).max()), (pr, i, "not representable")
        pr.expected[i], pr.logs[i] = y32, log


def _oracle_bwd(pr):
    """float64 oracle forward and torch autograd from the probe's dy, over the scenes of the batch that carry dy:
    pr.grads[name] = float32 gradient of sum_n <V_pred_n, dy_n> (None for the parameters the forward never reads),
    asserted representable; pr.blogs[n] = the operation records of batch scene n with the gradient reaching every
    output; pr.dx[n] = float32 gradient with respect to x of batch scene n."""
    from oracle import stgcnn_oracle as O
    keys = [k for k in pr.state64 if "running" not in k and "num_batches" not in k]
    params = {k: pr.state64[k].clone().requires_grad_(True) for k in keys}
    work = dict(pr.state64)
    work.update(params)
    pr.blogs, pr.dx, xs = {}, {}, {}
    total = None
    for n, (where, vals) in pr.dy.items():
        x, adj = pr.scenes[n % len(pr.scenes)]
        log = []
        xs[n] = torch.from_numpy(x).double().unsqueeze(0).requires_grad_(True)
        with _recording(work, log):
            y = O.social_stgcnn_forward(work, xs[n], torch.from_numpy(adj).double(), False, n_stgcnn=pr.n_stgcnn,
                                        n_txpcnn=pr.n_txpcnn)[0]
        dy = torch.zeros_like(y)
        dy[where[:, 0], where[:, 1], where[:, 2]] = torch.from_numpy(vals).double()
        l = (y * dy).sum()
        total = l if total is None else total + l
        _check_log(pr, log)
        pr.blogs[n] = log
    total.backward()

    def r32(g, what):
        g = g.numpy()
        g32 = g.astype(np.float32)
        assert np.all(np.abs(g - g32.astype(np.float64)) <= 1e-12 * np.abs(g).max()), (pr, what, "not representable")
        return g32
    pr.grads = {k: (None if params[k].grad is None else r32(params[k].grad, k)) for k in keys}
    pr.dx = {n: r32(xs[n].grad[0], "dx") for n in xs}


def focus_records(pr):
    """[(W float32, data float32 (ci,H,W), bias, the oracle's pre-activation float64)] of the focus conv, per scene"""
    out = []
    for i, log in pr.logs.items():
        for kind, name, w, x, b, y, _ in log:
            if kind == "conv" and name == pr.focus_key:
                w32, x32 = w.astype(np.float32), x.astype(np.float32)
                assert np.all(w32 == w) and np.all(x32 == x), (pr, name)
                out.append((w32, x32, b, y))
    assert out
    return out


# ------------------------------------------------------------------------------------------
# validity
# ------------------------------------------------------------------------------------------
def _within(q, bound, what):
    assert bound < 2.0 ** 24 * q, (what, bound, q, bound / q / 2.0 ** 24)


def _r32(a, what):
    """the value is a float32 (up to the 1e-16 of the oracle's BatchNorm scale)"""
    a32 = np.asarray(a, np.float64).astype(np.float32)
    assert np.all(np.abs(a - a32) <= 1e-12 * max(1e-30, float(np.abs(a).max()))), what
    return a32


def probe_budget(pr):
    """The two validity conditions, for every operation of every scene.
    1. dropped products vanish: the convolution of the ABSOLUTE piece images over the three dropped piece pairs is zero
       (every pair (W, x) meeting in a sum has top pieces i + j <= 2), for every conv and for the aggregation;
    2. order-independent exactness: sum |W| |x| + |bias| < 2^24 q with q the product of the operands' quanta (and no
       coarser than the bias's), for every conv, the aggregation, every BatchNorm ((|v| + |mean|) |k| + |beta|) and every
       residual add; every recorded value is a float32.
    Returns the largest fraction of the budget any operation uses."""
    used = 0.0
    for i, log in pr.logs.items():
        outs = {}
        for kind, name, w, x, b, y, _ in log:
            if kind == "prelu":
                continue
            what = (pr.id, i, kind, name)
            x32, y32 = _r32(x, what), _r32(y, what)
            if kind == "bn":
                k32 = _r32(w, what)[:, None, None]
                mean, beta = b
                q = min(quantum(x32, mean) * quantum(k32), quantum(beta))
                bound = float(((np.abs(x32) + np.abs(mean)[:, None, None]) * np.abs(k32)
                               + np.abs(beta)[:, None, None]).max())
            elif kind == "agg":
                # y[t,c,w] = sum_v g[t,c,v] A[t,v,w]
                wp, xp = split3(w.astype(np.float32)), split3(x32)
                for (a, c) in DROPPED:
                    assert not np.any(np.matmul(np.abs(xp[c]).astype(np.float64), np.abs(wp[a]).astype(np.float64))), what
                q = quantum(w) * quantum(x32)
                bound = float(np.matmul(np.abs(x32).astype(np.float64), np.abs(w)).max())
            else:
                w32 = _r32(w, what)
                assert not np.any(conv6(w32, x32, keep=DROPPED, absolute=True)), what
                q = quantum(w32) * quantum(x32)
                if b is not None and np.any(b):
                    q = min(q, quantum(b))
                bound = float(_conv64(np.abs(w32), np.abs(x32)).max() + (0.0 if b is None else np.abs(b).max()))
            if np.isfinite(q):
                _within(q, bound, what)
                used = max(used, bound / q / 2.0 ** 24)
            outs[name] = (x32, y32)
        # residual adds: h + res in the first block, PReLU(h + x) inputs of the stacked blocks, PReLU(z) + v in the TXP
        st = pr.state64
        for b_ in range(pr.n_stgcnn):
            p = "st_gcns.%d." % b_
            h = outs[p + "tcn.3.weight"][1]
            res = outs[p + "residual.1.weight"][1] if b_ == 0 else outs[p + "gcn.conv.weight"][0]
            _within(min(quantum(h), quantum(res)), float((np.abs(h) + np.abs(res)).max()), (pr.id, i, "add", p))
        for j in range(1, max(1, pr.n_txpcnn - 1)):
            v, z = outs["tpcnns.%d.weight" % j]
            al = float(st["prelus.%d.weight" % j])
            a = np.where(z > 0, z, al * z)
            _within(min(quantum(a), quantum(v)), float((np.abs(a) + np.abs(v)).max()), (pr.id, i, "add", "txp%d" % j))
    return used


def dgrad_weights(w):
    """the weights of the input-gradient convolution: Wt[ci][co][kh][kw] = W[co][ci][K-1-kh][K-1-kw]
    (d in[ci][pos] = sum Wt[ci][co][tap] dz[co][pos + tap], as prep_dgrad_vector arranges them)"""
    return np.ascontiguousarray(np.transpose(w, (1, 0, 2, 3))[:, :, ::-1, ::-1])


def bwd_focus_records(pr):
    """[(Wt float32, dz float32 (co,H,W))] of the focus's input-gradient convolution, per scene that carries dy"""
    out = []
    for n, log in pr.blogs.items():
        for kind, name, w, x, b, y, gh in log:
            if kind == "conv" and name == pr.focus_key:
                g = gh["g"][0]
                w32, g32 = w.astype(np.float32), g.astype(np.float32)
                assert np.all(w32 == w) and np.all(g32 == g), (pr, name)
                out.append((dgrad_weights(w32), g32))
    assert out
    return out


def probe_budget_bwd(pr):
    """The two validity conditions for every operation of the backward, over the scenes that carry dy:
    every input-gradient convolution and the aggregation's (dropped products vanish on the absolute piece images;
    sum |Wt| |dz| -- plus the skip gradient a residual TXP layer adds to it -- < 2^24 q), and every reduction over
    positions and scenes: weight gradients sum |dz| |x| per slot (the operands' top pieces i + j <= 2), bias gradients
    sum |dz|, slope gradients sum |dv| |z|, BatchNorm sum |dy| (|x| + |mean|) / sqrt(s) and sum |dy|.
    Returns the largest fraction of the budget any of them uses."""
    import torch.nn.grad as G_
    acc = {}
    used = [0.0]

    def within(q, bound, what):
        if np.isfinite(q) and bound > 0:
            _within(q, bound, what)
            used[0] = max(used[0], bound / q / 2.0 ** 24)

    def add(key, bound, q):
        """one reduction per output channel (or one in all): bounds add up over the scenes, the quantum is the finest"""
        bound, q = np.atleast_1d(np.asarray(bound, np.float64)), np.atleast_1d(np.asarray(q, np.float64))
        a = acc.setdefault(key, [np.zeros_like(bound), np.full_like(q, np.inf)])
        a[0], a[1] = a[0] + bound, np.minimum(a[1], q)

    def rows(a):
        return np.array([quantum(r) for r in a])
    hidden = max(1, pr.n_txpcnn - 1)
    for n, log in pr.blogs.items():
        by_name = {(e[0], e[1]): e for e in log}
        for kind, name, w, x, b, y, gh in log:
            what = (pr.id, n, kind, name)
            g = gh.get("g")
            if g is None or not np.any(g):
                continue
            if kind != "agg":
                g = g[0]
            g32, x32 = _r32(g, what), _r32(x, what)
            if kind == "conv":
                w32 = _r32(w, what)
                wt = dgrad_weights(w32)
                assert not np.any(conv6(wt, g32, keep=DROPPED, absolute=True)), what
                q, bound = quantum(w32) * quantum(g32), float(_conv64(np.abs(wt), np.abs(g32)).max())
                if name.startswith("tpcnns.") and 1 <= int(name.split(".")[1]) < hidden:
                    skip = by_name[("prelu", "prelus.%s.weight" % name.split(".")[1])][6]["g"][0]
                    q, bound = min(q, quantum(skip)), bound + float(np.abs(skip).max())
                within(q, bound, what + ("dx",))
                if np.any(x32):
                    assert _top_of(g32) + _top_of(x32) <= 2, what + ("dW pieces",)
                    kh, kw = w32.shape[2:]
                    slot = G_.conv2d_weight(torch.from_numpy(np.abs(x32).astype(np.float64))[None], w32.shape,
                                            torch.from_numpy(np.abs(g32).astype(np.float64))[None],
                                            padding=(kh // 2, kw // 2))
                    add(name, slot.numpy().reshape(w32.shape[0], -1).max(axis=1), rows(g32) * quantum(x32))
                add(name[:-6] + "bias", np.abs(g32).sum(axis=(1, 2)), rows(g32))
            elif kind == "agg":
                # y = g A: d g = dy A^T
                a32 = w.astype(np.float32)
                ap, gp = split3(a32), split3(g32)
                for (i, j) in DROPPED:
                    assert not np.any(np.matmul(np.abs(gp[j]).astype(np.float64),
                                                np.swapaxes(np.abs(ap[i]).astype(np.float64), -1, -2))), what
                within(quantum(a32) * quantum(g32),
                       float(np.matmul(np.abs(g32).astype(np.float64), np.swapaxes(np.abs(w), -1, -2)).max()), what)
            elif kind == "bn":
                prefix = name[:-len(".weight")]
                s = (pr.state[prefix + ".running_var"].numpy() + np.float32(1e-5)).astype(np.float64)
                rs = 1.0 / np.sqrt(s)
                mean, beta = b
                add(name, (np.abs(g32) * (np.abs(x32) + np.abs(mean)[:, None, None]) * rs[:, None, None]).sum(axis=(1, 2)),
                    rows(g32) * np.array([quantum(x32[c], mean[c]) for c in range(len(rs))]) * rs)
                add(prefix + ".bias", np.abs(g32).sum(axis=(1, 2)), rows(g32))
            elif kind == "prelu":
                if np.any(x32):
                    add(name, float((np.abs(g32) * np.abs(x32)).sum()), quantum(g32) * quantum(x32))
    for key, (bound, q) in acc.items():
        for c in range(len(bound)):
            within(q[c], bound[c], (pr.id, "sum over positions and scenes", key, c))
    return used[0]


def _top_of(a):
    """the highest piece index any non-zero element of `a` reaches"""
    return int(top_piece(a).max())


# ------------------------------------------------------------------------------------------
# the case table: compiled variant x batch geometry x (layout, focus) pairs
# ------------------------------------------------------------------------------------------
class Variant:
    def __init__(self, name, layout, options, vpad, counts, n=None, ragged=True, focus_set=None, why="", bwd_seeds=1):
        self.name, self.layout, self.options, self.vpad = name, layout, dict(options), vpad
        self.counts, self.n, self.ragged = list(counts), n, ragged
        self.focus_set = focus_set                    # None: every focus of the layout
        self.why = why
        self.bwd_seeds = bwd_seeds                    # backward probes per (focus, class): dy positions drawn anew each


def _some(n_txpcnn):
    """layer 0, one hidden layer (where the layout has one), the output conv and one block focus"""
    f = ["txp0", "out", "tcn"]
    if n_txpcnn >= 3:
        f.insert(1, "txp%d" % (n_txpcnn - 2))
    return f


def variants():
    """How each compiled variant of the scene kernels is reached (by batch geometry and options, as
    test_gpu_canon_shape.py and test_gpu_step_one_launch.py establish it) and which focuses run on it."""
    small17 = [17, 1, 2, 16, 0, 9, 17, 5]
    small32 = [32, 1, 2, 16, 17, 31, 0, 32, 8, 25]
    team57 = [57, 1, 8, 9, 16, 17, 32, 33, 0, 56]
    team100 = [100, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 99]
    team128 = [128, 2, 32, 33, 64, 65, 127, 96, 0, 7]
    out = []
    # small ragged batches of non-canonical layouts: below 384 scenes every scene of more than 8 pedestrians is cut into a
    # team (team_geom in txp_x6.hip: v1 = 8, v2 = 16), whatever `wave_path` says -- the team kernels, every focus x class
    for k, v, cnt in ((1, 17, small17), (3, 32, small32), (8, 17, small17), (8, 32, small32)):
        out.append(Variant("team", (1, k), {"wave_path": True}, v, cnt, why="small-batch teams (1 / 2 / 4 waves)"))
    # solo wave, the canonical model at V = 32: Shape::Canon (num_peds given) and Shape::Canon32 (no num_peds)
    out.append(Variant("canon32", (1, 5), {}, 32, [32] * 7, n=1536, ragged=False, why="N = 1536 uniform, no num_peds"))
    out.append(Variant("canon", (1, 5), {}, 32, [32] * 7, n=1536, ragged=True, focus_set=_some(5),
                       why="N = 1536 uniform, num_peds = 32"))
    # teams of two and four waves: scenes beyond 32 pedestrians, and the small-batch teams at V = 32
    out.append(Variant("team", (1, 5), {}, 57, team57, focus_set=_some(5), why="two-wave teams"))
    out.append(Variant("team", (1, 3), {}, 100, team100, focus_set=_some(3), why="four-wave teams"))
    out.append(Variant("team", (1, 5), {}, 128, team128, focus_set=_some(5), why="four-wave teams"))
    out.append(Variant("team", (1, 3), {}, 32, [32, 17, 5], focus_set=_some(3), why="small-batch teams"))
    # workgroup-per-scene kernels
    out.append(Variant("wg", (1, 5), {"wg_path": True, "wg_waves": 1}, 12, [12, 1, 0, 7, 11], focus_set=_some(5)))
    out.append(Variant("wg", (1, 5), {"wg_path": True, "wg_waves": 8}, 57, team57, focus_set=_some(5)))
    out.append(Variant("wg", (2, 5), {"wg_waves": 8}, 12, [12, 1, 0, 7, 11], focus_set=_some(5)))
    out.append(Variant("wg", (2, 5), {"wg_waves": 1}, 57, team57, focus_set=_some(5)))
    out.append(Variant("wg", (4, 1), {}, 57, team57, focus_set=["txp0", "out", "tcn"]))
    out.append(Variant("wg", (2, 5), {}, 130, [130], ragged=False, focus_set=_some(5)))
    # fp32-MFMA wave kernels (condition 1 is not needed there; the same probes serve)
    out.append(Variant("f32mfma", (1, 3), {"f32_mfma": True, "wave_path": True}, 32, small32, focus_set=_some(3)))
    # solo wave, Shape::Generic: a non-canonical layout at N >= 1536 (team_geom: v1 = 32) and V <= 32 -- as
    # layout_cases' `uniform` group and test_gpu_canon_shape.py reach the solo kernels.  Seven unique scenes tiled; every
    # focus x class on the ragged batches (appended last: the seeds of the variants above derive from their place)
    gen32, gen17 = [32, 1, 2, 16, 17, 31, 0], [17, 1, 2, 16, 9, 0, 5]
    for k in (1, 3, 8):
        out.append(Variant("generic", (1, k), {}, 32, gen32, n=1536, why="N = 1536 ragged, solo generic"))
    out.append(Variant("generic", (1, 3), {}, 32, [32] * 7, n=1536, ragged=False, focus_set=_some(3),
                       why="N = 1536 uniform, no num_peds"))
    out.append(Variant("generic", (1, 8), {}, 17, gen17, n=1536, focus_set=_some(8), why="N = 1536 ragged, padded to 17"))
    # every hidden layer once on two- and four-wave teams of wide scenes
    out.append(Variant("team", (1, 8), {}, 100, team100, why="two- and four-wave teams, every focus",
                       bwd_seeds=3))
    return out


class ProbeCase:
    def __init__(self, variant, focus, cls, seed, backward=False, cut=True, rep=0):
        self.variant, self.focus, self.cls, self.seed, self.backward = variant, focus, cls, seed, backward
        self.cut = cut
        v = variant
        opt = "".join("-%s%s" % (k, "" if val is True else val) for k, val in sorted(v.options.items()))
        self.id = "%s-%dx%d-V%d-N%d%s%s-%s-%s" % (v.name, v.layout[0], v.layout[1], v.vpad, v.n or len(v.counts), opt,
                                                  "" if v.ragged else "-uniform", focus, cls)
        self.id += ("" if cut else "-dx") + ("-r%d" % rep if rep else "")

    def build(self):
        v = self.variant
        return make_probe(v.layout[0], v.layout[1], self.focus, self.cls, v.counts, self.seed,
                          backward=(v.n or len(v.counts)) if self.backward else None, cut=self.cut)

    def __repr__(self):
        return self.id


def probe_cases():
    out = []
    for vi, v in enumerate(variants()):
        for focus in (v.focus_set or focuses(v.layout[1])):
            for cls in CLASSES:
                out.append(ProbeCase(v, focus, cls, 100 + vi))
    return out


def bwd_probe_cases():
    """backward probes: the same variants; every backward focus x class on the solo Generic batches (N = 1536) and on Canon32, the
    variant's own focuses (those with an input-gradient convolution) elsewhere"""
    out = []
    for vi, v in enumerate(variants()):
        fs = [f for f in (v.focus_set or focuses(v.layout[1])) if f in bwd_focuses(v.layout[1])]
        for focus in fs:
            for cls in CLASSES:
                for r in range(v.bwd_seeds):
                    case = ProbeCase(v, focus, cls, 300 + vi + 50 * r, backward=True, rep=r)
                    case.seed += 1000 * BWD_SEED_SHIFT.get(case.id, 0)
                    out.append(case)
        # the workgroup kernels also hand back dx: the tcn focus once more with the forward left uncut, so that dx is not zero
        if v.name == "wg":
            for cls in DX_CLASSES:
                case = ProbeCase(v, "tcn", cls, 300 + vi, backward=True, cut=False)
                case.seed += 1000 * BWD_SEED_SHIFT.get(case.id, 0)
                out.append(case)
    return out


# the uncut forward carries multi-bit activations behind the focus: the slope and weight gradients there are sums of
# (dz x activation) products, inside the budget only where dz has one bit, i.e. in the W-wide class
DX_CLASSES = ("w_wide",)


# seeds moved until every reduction of the backward is inside its budget (test_exact_probes_cpu.py asserts it for every
# case; the draws of a few cases put most of dy's elements on one output channel)
BWD_SEED_SHIFT = {"canon32-1x5-V32-N1536-uniform-txp3-medium": 1, "wg-2x5-V57-N10-wg_waves1-txp3-w_wide": 2,
                  "wg-2x5-V130-N1-uniform-out-medium": 1, "wg-4x1-V57-N10-tcn-w_wide-dx": 2}


def batch_tensors(pr, variant, seed=5):
    """(x (N,2,T,V), adj (N,T,V,V), counts (N,), idx): the probe's unique scenes tiled to the variant's batch size as
    layout_cases.Batch tiles them (scene i of the batch is unique scene i % U), garbage in the padded slots."""
    u, v = len(pr.scenes), variant.vpad
    rng = np.random.default_rng(seed)
    x = rng.uniform(-40.0, 40.0, (u, 2, T_OBS, v)).astype(np.float32)
    adj = rng.uniform(-40.0, 40.0, (u, T_OBS, v, v)).astype(np.float32)
    for i, sc in enumerate(pr.scenes):
        if sc is not None:
            c = sc[0].shape[2]
            x[i, :, :, :c], adj[i, :, :c, :c] = sc
    n = variant.n or u
    idx = np.arange(n) % u
    return torch.from_numpy(x), torch.from_numpy(adj), pr.counts[idx], idx
