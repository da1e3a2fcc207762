"""Plain float64 restatements of the stand-alone ops behind the C ABI, and the edge cases they are checked at.

Written for reading, not speed, and sharing no code with `social_stgcnn_amd/ops.py`.  `tests/test_ops_ref_cpu.py` pins the
references to torch.einsum / F.conv2d autograd; `tests/test_gpu_ops_edges.py` holds the HIP kernels to them.

Every linear reference is a sum of products, so the same function applied to the ABSOLUTE inputs gives, per output
element, S = sum_i |a_i b_i|.  Two bounds hang on S:
  * integer inputs: every partial sum of any summation order is an integer of magnitude <= S, exactly representable in
    fp32 while S < 2^24 -- the kernel must then return the fp64 result bit for bit (`EXACT_LIMIT`);
  * real inputs: |fp32 sum - exact| <= (K + 2) 2^-24 S for K terms in any order, with or without fma (`rounding_bound`).
"""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32
EXACT_LIMIT = 2.0 ** 24         # integers below it are exact in fp32
SENTINEL = 7.0                  # what the padded slots of x, A, dy and rel hold: must never reach an output


def clamp_peds(num_peds, n, v):
    """the pedestrian counts the kernels use: None = all V, otherwise clamped to [0, V]"""
    if num_peds is None:
        return np.full(n, v, dtype=np.int64)
    return np.clip(np.asarray(num_peds, dtype=np.int64), 0, v)


def ragged_counts(v):
    """num_peds of the six-scene ragged batch every op is run on: -1, 0, 1, V-1, V, V+2 (as passed, unclamped)"""
    return [-1, 0, 1, v - 1, v, v + 2]


def rounding_bound(k, s):
    """worst-case fp32 error of a K-term sum of products whose absolute terms add up to `s`"""
    return (np.asarray(k, dtype=np.float64) + 2.0) * U * s


# ------------------------------------------------------------------------------------------------
# spatial aggregation: y[n,c,t,w] = sum_v x[n,c,t,v] A[n,t,v,w] on the valid block of every scene
# ------------------------------------------------------------------------------------------------
def _scene_adj(adj, n):
    return adj if adj.ndim == 3 else adj[n]


def agg_fwd(x, adj, num_peds=None):
    x, adj = np.asarray(x, dtype=np.float64), np.asarray(adj, dtype=np.float64)
    n_scenes, _, _, v = x.shape
    y = np.zeros_like(x)
    for n, p in enumerate(clamp_peds(num_peds, n_scenes, v)):
        y[n, :, :, :p] = np.einsum("ctv,tvw->ctw", x[n, :, :, :p], _scene_adj(adj, n)[:, :p, :p])
    return y


def agg_dx(dy, adj, num_peds=None):
    dy, adj = np.asarray(dy, dtype=np.float64), np.asarray(adj, dtype=np.float64)
    n_scenes, _, _, v = dy.shape
    dx = np.zeros_like(dy)
    for n, p in enumerate(clamp_peds(num_peds, n_scenes, v)):
        dx[n, :, :, :p] = np.einsum("ctw,tvw->ctv", dy[n, :, :, :p], _scene_adj(adj, n)[:, :p, :p])
    return dx


# ------------------------------------------------------------------------------------------------
# (kt, 1) convolution, stride 1, zero padding `pad` in time; padded pedestrians are zero on input and output
# ------------------------------------------------------------------------------------------------
def _mask(a, num_peds):
    """a (N, ., ., V) with the slots v >= num_peds[n] zeroed"""
    a = np.array(a, dtype=np.float64)
    for n, p in enumerate(clamp_peds(num_peds, a.shape[0], a.shape[-1])):
        a[n, ..., p:] = 0.0
    return a


def _pad_time(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (0, 0)))


def conv_fwd(x, w, b, pad, num_peds=None):
    """x (N,Cin,T,V), w (Cout,Cin,kt), b (Cout) or None -> y (N,Cout,To,V), To = T + 2 pad - kt + 1"""
    w = np.asarray(w, dtype=np.float64).reshape(w.shape[0], w.shape[1], -1)
    kt = w.shape[2]
    xp = _pad_time(_mask(x, num_peds), pad)
    to = xp.shape[2] - kt + 1
    y = np.zeros((xp.shape[0], w.shape[0], to, xp.shape[3]))
    for dt in range(kt):
        y += np.einsum("oc,nctv->notv", w[:, :, dt], xp[:, :, dt:dt + to])
    if b is not None:
        y += np.asarray(b, dtype=np.float64)[None, :, None, None]
    return _mask(y, num_peds)


def conv_bwd(x, w, dy, pad, num_peds=None):
    """-> dx (N,Cin,T,V), dw (Cout,Cin,kt), db (Cout) of sum(y * dy)"""
    w = np.asarray(w, dtype=np.float64).reshape(w.shape[0], w.shape[1], -1)
    kt = w.shape[2]
    xp = _pad_time(_mask(x, num_peds), pad)
    dym = _mask(dy, num_peds)
    to = dym.shape[2]
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for dt in range(kt):
        dxp[:, :, dt:dt + to] += np.einsum("oc,notv->nctv", w[:, :, dt], dym)
        dw[:, :, dt] = np.einsum("notv,nctv->oc", dym, xp[:, :, dt:dt + to])
    dx = dxp[:, :, pad:dxp.shape[2] - pad]
    return np.ascontiguousarray(dx), dw, dym.sum(axis=(0, 2, 3))


def conv_terms(n_valid, cin, cout, t, kt, pad):
    """K, the number of terms of one output element (an upper count: taps in the zero padding included):
    y, dx, dw, db; n_valid = sum over scenes of their valid pedestrians"""
    to = t + 2 * pad - kt + 1
    return {"y": cin * kt + 1, "dx": cout * kt, "dw": to * n_valid, "db": to * n_valid}


# ------------------------------------------------------------------------------------------------
# flat clip_grad_norm_ + SGD, weighted sum, window gather
# ------------------------------------------------------------------------------------------------
def clip_sgd(p, g, lr, max_norm=None):
    """-> (p - lr g', g', ||g||) with g' = g min(1, max_norm / (||g|| + 1e-6)), g' = g without max_norm"""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    norm = float(np.sqrt(np.sum(g * g)))
    if max_norm is not None and max_norm > 0:
        g = g * min(1.0, float(max_norm) / (norm + 1e-6))
    return p - float(lr) * g, g, norm


def weighted_sum(v, w=None):
    v = np.asarray(v, dtype=np.float64)
    return float(np.sum(v if w is None else v * np.asarray(w, dtype=np.float64)))


def gather_windows(rel_all, win_start, index, n, v, t_obs, t_pred):
    """rel_all (P_total, 2, T_obs + T_pred), windows [win_start[w], win_start[w+1]) -> obs_rel (N,V,2,T_obs),
    target (N,T_pred,V,2), num_peds (N); an index outside [0, n_windows) is clamped, a window larger than V truncated"""
    n_windows = len(win_start) - 1
    obs = np.zeros((n, v, 2, t_obs))
    tgt = np.zeros((n, t_pred, v, 2))
    peds = np.zeros(n, dtype=np.int32)
    for i in range(n):
        w = i if index is None else int(index[i])
        w = min(max(w, 0), n_windows - 1)
        s = int(win_start[w])
        c = min(max(int(win_start[w + 1]) - s, 0), v)
        peds[i] = c
        win = np.asarray(rel_all[s:s + c], dtype=np.float64)
        obs[i, :c] = win[:, :, :t_obs]
        tgt[i, :, :c] = np.transpose(win[:, :, t_obs:], (2, 0, 1))
    return obs, tgt, peds


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def draw(rng, shape, integer):
    """fp32 inputs: small integers in -2..2 (exact check) or standard normals (rounding check)"""
    if integer:
        return rng.integers(-2, 3, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def fill_padding(a, num_peds, axes=(-1,)):
    """SENTINEL into the slots >= num_peds[n] along each of `axes` of a (N, ...) array (in place)"""
    for n, p in enumerate(clamp_peds(num_peds, a.shape[0], a.shape[axes[0]])):
        for ax in axes:
            idx = [slice(None)] * (a.ndim - 1)
            idx[ax if ax < 0 else ax - 1] = slice(p, None)
            a[n][tuple(idx)] = SENTINEL
    return a


def agg_inputs(case, integer, seed=0):
    """x (N,C,T,V), A (T,V,V) | (N,T,V,V), dy (N,C,T,V) of a spatial_agg case; padded slots hold SENTINEL"""
    rng = np.random.default_rng([seed, case["c"], case["t"], case["v"], int(integer)])
    n, c, t, v = case["n"], case["c"], case["t"], case["v"]
    x, dy = draw(rng, (n, c, t, v), integer), draw(rng, (n, c, t, v), integer)
    adj = draw(rng, (t, v, v) if case["shared"] else (n, t, v, v), integer)
    peds = case["peds"]
    if peds is not None:
        fill_padding(x, peds)
        fill_padding(dy, peds)
        if not case["shared"]:
            fill_padding(adj, peds, axes=(-1, -2))
    return x, adj, dy


def conv_inputs(case, integer, seed=0):
    """x (N,Cin,T,V), w (Cout,Cin,kt,1), b (Cout) | None, dy (N,Cout,To,V) of a conv_t case"""
    rng = np.random.default_rng([seed, case["cin"], case["cout"], case["kt"], case["n"], int(integer)])
    n, cin, cout, t, v, kt, pad = (case[k] for k in ("n", "cin", "cout", "t", "v", "kt", "pad"))
    to = t + 2 * pad - kt + 1
    x, dy = draw(rng, (n, cin, t, v), integer), draw(rng, (n, cout, to, v), integer)
    w = draw(rng, (cout, cin, kt, 1), integer)
    b = draw(rng, (cout,), integer) if case["bias"] else None
    if case["peds"] is not None:
        fill_padding(x, case["peds"])
        fill_padding(dy, case["peds"])
    return x, w, b, dy


# ------------------------------------------------------------------------------------------------
# cases: every one names the host-side branch or kernel guard it is there for
# ------------------------------------------------------------------------------------------------
def _agg(name, n, c, t, v, shared=False, ragged=True, **kw):
    """ragged: the six counts plus V-2 -- with V-1 and 1 it puts the last valid pedestrian on every position of a
    four-wide strip, so each of the kernels' three per-component masks decides an output"""
    peds = None
    if ragged:
        peds = ragged_counts(v) + [max(v - 2, 0)]
        assert n == len(peds)
    return dict(id=name, n=n, c=c, t=t, v=v, shared=shared, peds=peds, **kw)


AGG_CASES = [
    # V not a multiple of 4: the VEC = 1 kernels, forward and backward
    _agg("v1", 7, 1, 1, 1),
    _agg("v3", 7, 9, 5, 3),                    # C = 9: a second channel pass of one channel
    _agg("v31", 7, 8, 8, 31),
    _agg("v33", 7, 9, 1, 33),
    _agg("v130", 7, 9, 8, 130),                # V > 64, more (t, v) rows than lanes
    # V % 4 == 0, not 8 / 16 / 32 / 64: strip forward <4>, generic backward <4> (wq strips, partial last strip)
    _agg("v4", 7, 8, 8, 4),
    _agg("v12", 7, 1, 12, 12),
    _agg("v68", 7, 8, 12, 68),                 # wq = 17 > U = 8: three trips of the in-flight loop
    # V = 8 / 16 / 32 / 64: bwd_rows<LPR>; T = 5, 12 are no multiple of TB = 4 (`t < T`) nor of the quarters' 8 (`live`)
    _agg("v8_t5", 7, 17, 5, 8),
    _agg("v8_t12", 7, 8, 12, 8),
    _agg("v16_t5", 7, 1, 5, 16),
    _agg("v16_t12", 7, 9, 12, 16),
    _agg("v32_t5", 7, 17, 5, 32),              # quarters forward: one partial pass of 8 time steps
    _agg("v32_t12", 7, 9, 12, 32),             # quarters forward: a full pass and a partial one
    _agg("v32_t1", 7, 8, 1, 32),
    _agg("v64_t5", 7, 9, 5, 64),               # bwd_rows<16>: G = 4 row groups, TB = 1
    _agg("v64_t12", 7, 17, 12, 64),
    # shared adjacency (a_sn = 0), without and with num_peds
    _agg("shared_v32", 2, 9, 8, 32, shared=True, ragged=False),
    _agg("shared_v12", 2, 17, 5, 12, shared=True, ragged=False),
    _agg("shared_v130", 2, 1, 1, 130, shared=True, ragged=False),
    _agg("shared_v64", 2, 8, 8, 64, shared=True, ragged=False),
    _agg("shared_v16_ragged", 7, 8, 8, 16, shared=True),
    # adj / dy one float off 16-byte alignment at V = 32 (through the C ABI): VEC = 1 forward and backward for adj,
    # the generic backward <4> in place of bwd_rows<8> for dy
    _agg("v32_adj_offset", 7, 9, 5, 32, offset="adj"),
    _agg("v32_dy_offset", 7, 9, 5, 32, offset="dy"),
    # C T V 4 bytes just over 64 KiB: strip forward <4> at V = 32 instead of the quarters, generic backward, both with
    # the kernel's dynamic-LDS limit raised
    _agg("v32_c65_lds66k", 2, 65, 8, 32, ragged=False) | dict(peds=[31, 34]),
    _agg("v132_c16_lds67k", 2, 16, 8, 132, ragged=False) | dict(peds=[131, 134]),
]
AGG_REFUSED = dict(n=1, c=41, t=8, v=128)          # 167,936 bytes > 160 KiB: STG_ELDS, forward and backward


def _conv(name, n, cin, cout, t, v, kt, pad, bias=True, ragged=True, **kw):
    """ragged: the six counts, cycled over N starting at V-1 -- the first and the last scene of the first workgroup of a
    grid-stride launch (scenes 0 and 512, 0 and 2048) are then both non-empty"""
    peds = [ragged_counts(v)[(i + 3) % 6] for i in range(n)] if ragged else None
    return dict(id=name, n=n, cin=cin, cout=cout, t=t, v=v, kt=kt, pad=pad, bias=bias, peds=peds, **kw)


CONV_CASES = [
    # kt and pad: To = T, To < T, To > T, even kt
    _conv("kt1", 6, 2, 5, 8, 9, 1, 0),
    _conv("kt2_shorter", 6, 3, 4, 8, 5, 2, 0),                # To = T - 1
    _conv("kt2_longer", 6, 3, 4, 8, 5, 2, 1),                 # To = T + 1
    _conv("kt3_same", 6, 5, 5, 8, 32, 3, 1),
    _conv("kt3_shorter", 6, 3, 7, 8, 5, 3, 0),                # To = T - 2
    _conv("kt3_longer", 6, 3, 7, 5, 6, 3, 2),                 # To = T + 2
    _conv("kt5_same", 6, 4, 3, 12, 7, 5, 2),
    _conv("kt5_longer", 6, 2, 3, 3, 4, 5, 3),                 # kt > T: taps in the padding on both sides at once
    # weight-gradient accumulators gacc[1..3]: 500 weights (two of them), 1024 = 64 * 16 * 1 (all four, the limit)
    _conv("w500", 6, 10, 10, 6, 5, 5, 2),
    _conv("w1024", 6, 16, 64, 3, 5, 1, 0),
    _conv("cout256", 6, 4, 256, 3, 5, 1, 0),                  # db by 256 threads, 1024 weights
    # no bias (b == NULL, db == NULL), x without gradient (dx == NULL), the strided x the trainer passes, no num_peds
    _conv("no_bias", 6, 3, 4, 8, 5, 3, 1, bias=False),
    _conv("no_dx", 6, 3, 4, 8, 5, 3, 1, need_dx=False),
    _conv("strided_x", 6, 3, 4, 8, 5, 3, 1, strided=True),
    _conv("no_peds", 3, 3, 4, 8, 5, 3, 1, ragged=False),
    # x[n] alone over 64 KiB (forward 67 KiB, backward 88 KiB of LDS): the raised dynamic-LDS limit
    _conv("lds_over_64k", 2, 16, 5, 8, 130, 3, 1) | dict(peds=[129, 132]),
    # grid-stride scene loops, weight gradient carried in registers across scenes: backward N > 512, forward N > 2048
    _conv("n1", 1, 3, 4, 4, 5, 3, 1, ragged=False),
    _conv("n513", 513, 3, 4, 4, 5, 3, 1),
    _conv("n2049", 2049, 3, 4, 4, 5, 3, 1),
]
CONV_REFUSED = [dict(cin=25, cout=41, kt=1),          # 1025 weights
                dict(cin=1, cout=257, kt=1)]          # Cout > 256


def conv_case(name):
    return next(c for c in CONV_CASES if c["id"] == name)


def max_abs_term_sum(outputs):
    return max(float(np.max(o)) if np.size(o) else 0.0 for o in outputs)


def agg_term_sums(case):
    """S of every output of the integer-valued run of a spatial_agg case (y, dx)"""
    x, adj, dy = agg_inputs(case, integer=True)
    return [agg_fwd(np.abs(x), np.abs(adj), case["peds"]), agg_dx(np.abs(dy), np.abs(adj), case["peds"])]


def conv_term_sums(case, repeats=1):
    """S of every output of the integer-valued run of a conv_t case (y, dx, dw, db); `repeats` calls accumulate"""
    x, w, b, dy = conv_inputs(case, integer=True)
    y = conv_fwd(np.abs(x), np.abs(w), None if b is None else np.abs(b), case["pad"], case["peds"])
    dx, dw, db = conv_bwd(np.abs(x), np.abs(w), np.abs(dy), case["pad"], case["peds"])
    return [y, dx, repeats * dw, repeats * db]


# the ConvTemporalGraphical case: conv (3 -> 5, kt 3, no padding: T 8 -> 6) then the einsum with A of length 6, ragged
MODULE_CASE = dict(n=6, cin=3, cout=5, t=8, v=9, kt=3, pad=0, peds=ragged_counts(9))


def module_inputs(integer, seed=0):
    c = MODULE_CASE
    rng = np.random.default_rng([seed, 77, int(integer)])
    to = c["t"] - c["kt"] + 1
    x = draw(rng, (c["n"], c["cin"], c["t"], c["v"]), integer)
    w, b = draw(rng, (c["cout"], c["cin"], c["kt"], 1), integer), draw(rng, (c["cout"],), integer)
    adj = draw(rng, (c["n"], to, c["v"], c["v"]), integer)
    dy = draw(rng, (c["n"], c["cout"], to, c["v"]), integer)
    fill_padding(x, c["peds"])
    fill_padding(dy, c["peds"])
    fill_padding(adj, c["peds"], axes=(-1, -2))
    return x, w, b, adj, dy


def module_ref(x, w, b, adj, dy):
    """the two references chained: h = conv(x), y = agg(h); dh = agg_dx(dy), (dx, dw, db) = conv_bwd(dh)"""
    c = MODULE_CASE
    h = conv_fwd(x, w, b, c["pad"], c["peds"])
    y = agg_fwd(h, adj, c["peds"])
    dh = agg_dx(dy, adj, c["peds"])
    dx, dw, db = conv_bwd(x, w, dh, c["pad"], c["peds"])
    return dict(h=h, y=y, dh=dh, dx=dx, dw=dw, db=db)


# ------------------------------------------------------------------------------------------------
# adjacency build: displacements drawn like the dataset; the raw adjacency in the oracle's arithmetic
# ------------------------------------------------------------------------------------------------
def adj_rel(rng, n, v, t):
    """seq_rel (N,V,2,T): |rel| <= 1 rounded to 1e-4 like the dataset files; pedestrian 1 moves exactly like pedestrian 0
    in every odd scene (all steps) and pedestrian 2 like pedestrian 0 at step 0 of every scene (coincident points)"""
    rel = np.round(rng.uniform(-1.0, 1.0, size=(n, v, 2, t)), 4).astype(np.float32)
    if v >= 2:
        rel[1::2, 1] = rel[1::2, 0]
    if v >= 3:
        rel[:, 2, :, 0] = rel[:, 0, :, 0]
    return rel


def adj_raw(seq_rel):
    """the un-normalised adjacency (T,V,V) of one scene (V,2,T), float64, in the arithmetic of
    oracle.seq_to_graph_np: fp32 differences, squares and sum, then sqrt and reciprocal in float64; 0 for coincident
    points, 1 on the diagonal"""
    p = np.transpose(np.asarray(seq_rel, dtype=np.float32), (2, 0, 1))
    diff = p[:, :, None, :] - p[:, None, :, :]
    sq = (diff ** 2).astype(np.float32)
    dist = np.sqrt((sq[..., 0] + sq[..., 1]).astype(np.float32).astype(np.float64))
    with np.errstate(divide="ignore"):
        a = np.where(dist == 0, 0.0, 1.0 / dist)
    a[:, np.arange(p.shape[1]), np.arange(p.shape[1])] = 1.0
    return a


# flat-buffer ops
COUNTS = (1, 63, 64, 65, 1023, 8192, 8193, 50000)       # below / at / above one wave; 8192 = 8 x 1024 ends the register branch
WSUM_NS = (0, 1, 1025)


def flat_inputs(count, integer, seed=0):
    rng = np.random.default_rng([seed, count, int(integer)])
    if integer:
        return draw(rng, (count,), True), draw(rng, (count,), True)
    return rng.standard_normal(count).astype(np.float32), (0.01 * rng.standard_normal(count)).astype(np.float32)


def gather_inputs(t_obs, t_pred, seed=0):
    """a ragged dataset of 9 windows with 0..11 pedestrians (integers: the gather moves values, exact by construction)"""
    rng = np.random.default_rng([seed, t_obs, t_pred])
    counts = np.array([3, 11, 0, 1, 7, 4, 9, 2, 5])
    win_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rel_all = rng.integers(-50, 51, size=(int(counts.sum()), 2, t_obs + t_pred)).astype(np.float32)
    return rel_all, win_start
