"""Host-side operator layer: torch.autograd.Functions over the C ABI (include/stgcnn_hip.h).

Every function here launches hand-written HIP kernels on the current torch stream and
raises if the library or a GPU tensor is missing -- there is no eager fallback.
"""
import collections
import ctypes
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import ModelDesc, call, check, lib, peds_arg, ptr, require_gpu, seed_u64      # noqa: F401 (lib: for callers)


@functools.lru_cache(maxsize=None)
def _stride_names(prefix, axes):
    return tuple("%s_s%s" % (prefix, a) for a in axes)


def _strides(prefix, x, axes):
    """The strides of x by the names the C ABI gives them: <prefix>_s<axis> for every letter of `axes`."""
    return dict(zip(_stride_names(prefix, axes), x.stride()))


def _adj_layout(adj, n, t, v):
    """adjacency (T,V,V) shared or (N,T,V,V) -> (contiguous-per-scene tensor, batch stride)."""
    if adj.dim() == 3:
        if tuple(adj.shape) != (t, v, v):
            raise ValueError("adjacency %s does not match x (T=%d, V=%d)" % (tuple(adj.shape), t, v))
        return adj.contiguous(), 0
    if adj.dim() == 4:
        if tuple(adj.shape) != (n, t, v, v):
            raise ValueError("adjacency %s does not match x (N=%d, T=%d, V=%d)" % (tuple(adj.shape), n, t, v))
        if adj.stride()[1:] != (v * v, v, 1):
            adj = adj.contiguous()
        return adj, adj.stride(0)
    raise ValueError("adjacency must be (T,V,V) or (N,T,V,V), got %d dims" % adj.dim())


# --------------------------------------------------------------------------------------------
# R1/R2 adjacency build
# --------------------------------------------------------------------------------------------
def adj_build(seq_rel, num_peds=None, normalize=True, out=None):
    """seq_rel (N,V,2,T) fp32 device tensor (any strides) -> nodes (N,T,V,2), adj (N,T,V,V).
    Counterpart of utils.seq_to_graph (utils.py:29-53).  `out` = (nodes, adj) to fill existing buffers (a captured
    step keeps the graph build inside the hipGraph this way)."""
    require_gpu(seq_rel)
    _lib.as_f32(seq_rel, "seq_rel")
    n, v, c, t = seq_rel.shape
    if c != 2:
        raise ValueError("seq_rel must be (N,V,2,T)")
    peds = peds_arg(num_peds, n, seq_rel.device)
    if out is not None:
        nodes, adj = out
        if tuple(nodes.shape) != (n, t, v, 2) or tuple(adj.shape) != (n, t, v, v) or not (
                nodes.is_contiguous() and adj.is_contiguous()):
            raise ValueError("adj_build: out = (nodes (N,T,V,2), adj (N,T,V,V)), contiguous")
    else:
        nodes = torch.empty((n, t, v, 2), device=seq_rel.device, dtype=torch.float32)
        adj = torch.empty((n, t, v, v), device=seq_rel.device, dtype=torch.float32)
    call("stg_adj_build", rel=ptr(seq_rel), **_strides("rel", seq_rel, "nvct"), num_peds=ptr(peds), N=n, V=v, T=t,
         normalize=1 if normalize else 0, nodes=ptr(nodes), adj=ptr(adj))
    return nodes, adj


# --------------------------------------------------------------------------------------------
# R3 spatial aggregation einsum('nctv,ntvw->nctw')
# --------------------------------------------------------------------------------------------
class _SpatialAgg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, num_peds):
        require_gpu(x, adj)
        _lib.as_f32(x, "x")
        _lib.as_f32(adj, "adj")
        n, c, t, v = x.shape
        adj_c, a_sn = _adj_layout(adj, n, t, v)
        peds = peds_arg(num_peds, n, x.device)
        y = torch.empty((n, c, t, v), device=x.device, dtype=torch.float32)
        call("stg_spatial_agg_fwd", x=ptr(x), **_strides("x", x, "nctv"), adj=ptr(adj_c), a_sn=a_sn, num_peds=ptr(peds),
             N=n, C=c, T=t, V=v, y=ptr(y))
        ctx.save_for_backward(adj_c, peds if peds is not None else torch.empty(0))
        ctx.a_sn = a_sn
        ctx.has_peds = peds is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        adj_c, peds = ctx.saved_tensors
        dy = dy.contiguous()
        n, c, t, v = dy.shape
        dx = torch.empty_like(dy)
        call("stg_spatial_agg_bwd", dy=ptr(dy), adj=ptr(adj_c), a_sn=ctx.a_sn,
             num_peds=ptr(peds) if ctx.has_peds else None, N=n, C=c, T=t, V=v, dx=ptr(dx))
        return dx, None, None


def spatial_agg(x, adj, num_peds=None):
    """y[n,c,t,w] = sum_v x[n,c,t,v] A[n,t,v,w]   (model.py:67); adj (T,V,V) or (N,T,V,V)."""
    return _SpatialAgg.apply(x, adj, num_peds)


# --------------------------------------------------------------------------------------------
# temporal / 1x1 convolution (kt x 1)
# --------------------------------------------------------------------------------------------
class _ConvT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad, num_peds):
        require_gpu(x, weight, bias)
        _lib.as_f32(x, "x")
        n, cin, t, v = x.shape
        cout, cin_w, kt, kw = weight.shape
        if cin_w != cin or kw != 1:
            raise ValueError("weight %s does not match input channels %d" % (tuple(weight.shape), cin))
        to = t + 2 * pad - kt + 1
        peds = peds_arg(num_peds, n, x.device)
        w = weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.empty((n, cout, to, v), device=x.device, dtype=torch.float32)
        call("stg_conv_t_fwd", x=ptr(x), **_strides("x", x, "nctv"), w=ptr(w), b=ptr(b), num_peds=ptr(peds), N=n,
             Cin=cin, Cout=cout, T=t, V=v, kt=kt, pad=pad, y=ptr(y))
        ctx.save_for_backward(x, w, peds if peds is not None else torch.empty(0))
        ctx.has_peds = peds is not None
        ctx.has_bias = bias is not None
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, peds = ctx.saved_tensors
        dy = dy.contiguous()
        n, cin, t, v = x.shape
        cout, _, kt, _ = w.shape
        dx = torch.empty((n, cin, t, v), device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dw = torch.zeros_like(w)
        db = torch.zeros(cout, device=x.device, dtype=torch.float32) if ctx.has_bias else None
        call("stg_conv_t_bwd", x=ptr(x), **_strides("x", x, "nctv"), w=ptr(w), dy=ptr(dy),
             num_peds=ptr(peds) if ctx.has_peds else None, N=n, Cin=cin, Cout=cout, T=t, V=v, kt=kt, pad=ctx.pad,
             dx=ptr(dx), dw=ptr(dw), db=ptr(db))
        return dx, dw, db, None, None


def conv_t(x, weight, bias, pad=0, num_peds=None):
    """nn.Conv2d(Cin, Cout, (kt,1), padding=(pad,0)) forward/backward (model.py:55-62)."""
    return _ConvT.apply(x, weight, bias, pad, num_peds)


# --------------------------------------------------------------------------------------------
# R4/R5 fused st_gcn / social_stgcnn
# --------------------------------------------------------------------------------------------
def flat_walk(items):
    """(index, offset, count) of every entry of `items` (tensors or shapes) laid end to end in one flat buffer."""
    off = 0
    for i, it in enumerate(items):
        cnt = it.numel() if torch.is_tensor(it) else math.prod(it)
        yield i, off, cnt
        off += cnt


class FlatPack:
    """Keeps a list of tensors as views of ONE flat fp32 device buffer (the layout the fused
    kernels read).  `ensure()` is cheap when nothing moved; it re-packs after .to(), a
    load_state_dict that replaced storage, or a child module packing itself."""

    def __init__(self):
        self.flat = None

    def ensure(self, tensors):
        total = sum(t.numel() for t in tensors)
        dev = tensors[0].device
        flat = self.flat
        if (flat is not None and flat.device == dev and flat.numel() == total
                and all(tensors[i].data_ptr() == flat.data_ptr() + 4 * off and tensors[i].is_contiguous()
                        for i, off, _ in flat_walk(tensors))):
            return flat
        flat = torch.empty(total, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for i, off, n in flat_walk(tensors):
                t = tensors[i]
                flat[off:off + n].copy_(t.detach().reshape(-1))
                t.data = flat[off:off + n].view(t.shape)
        self.flat = flat
        return flat


# Launch options of the fused model entry points (stg_model_desc.flags / .wg_waves).  Host-side switches: the
# library itself reads no environment and keeps no state, every choice travels in the descriptor.
#   wg_path     run the workgroup-per-scene kernels even where the wave-per-scene path fits (tests cover both)
#   split_bf16  TXP input-gradient GEMMs on bf16 MFMAs with hi/lo-split operands (opt-in, fp32 in / out)
#   wg_waves    0 = auto, or 1 / 2 / 4 / 8 waves per scene in the workgroup-per-scene kernels
#   wave_path   keep the wave-per-scene kernels where the library would pick the workgroup-per-scene ones for a small batch
#               (only reachable with f32_mfma / split_bf16: the exact-bf16 kernels serve small batches with finer teams)
#   bf16_store  bf16 storage of the saved TXP activations and of the dz hand-off (STG_OPT_BF16_STORE): fp32 forward
#               result, ~1e-3 relative error in the TXP weight / slope gradients; wave-per-scene path only
#   f32_mfma    the fp32-MFMA kernels where the default runs the exact bf16-pipe ones (STG_OPT_F32_MFMA): A/B measurements
#   separate_fb the training step (stg_model_step) keeps the forward and the backward scene kernels as two launches where
#               one launch serves both (STG_OPT_SEPARATE_FB): same results bit for bit, A/B measurements and tests
#   generic_wgrad keeps the generic weight-gradient kernel where the one compiled for the canonical model with uniform scenes
#               of 32 pedestrians serves the batch (STG_OPT_GENERIC_WGRAD): same results bit for bit, A/B measurements and tests
class KernelOptions(dict):
    """The launch options of ONE model: `model.options = ops.KernelOptions(bf16_store=True)` makes that model (and the
    Trainer / EpochRunner driving it) run with its own choices, whatever other models in the process do.  A model without
    an `options` attribute of its own uses the process-wide defaults, `ops.OPTIONS`."""
    DEFAULTS = {"wg_path": False, "split_bf16": False, "wg_waves": 0, "wave_path": False, "bf16_store": False,
                "f32_mfma": False, "separate_fb": False, "generic_wgrad": False}

    def __init__(self, **kw):
        bad = set(kw) - set(self.DEFAULTS)
        if bad:
            raise KeyError("unknown kernel options %s" % sorted(bad))
        super().__init__(self.DEFAULTS)
        self.update(kw)


OPTIONS = KernelOptions()           # process-wide defaults (models without their own `options`)


def make_desc(n_stgcnn, n_txpcnn, c_in, c_out, t_obs, t_pred, kt, residual0, use_mdn, training,
              eps=1e-5, momentum=0.1, options=None):
    o = OPTIONS if options is None else options
    flags = ((_lib.OPT_WG_PATH if o["wg_path"] else 0) | (_lib.OPT_SPLIT_BF16 if o["split_bf16"] else 0)
             | (_lib.OPT_WAVE_PATH if o["wave_path"] else 0)
             | (_lib.OPT_BF16_STORE if o["bf16_store"] else 0)
             | (_lib.OPT_F32_MFMA if o["f32_mfma"] else 0)
             | (_lib.OPT_SEPARATE_FB if o["separate_fb"] else 0)
             | (_lib.OPT_GENERIC_WGRAD if o["generic_wgrad"] else 0))
    return ModelDesc(n_stgcnn, n_txpcnn, c_in, c_out, t_obs, t_pred, kt, residual0, 1 if use_mdn else 0,
                     1 if training else 0, eps, momentum, flags, int(o["wg_waves"]))


class KernelTimer:
    """Per-kernel device time of the fused forward / backward entry points: HIP events recorded by the library
    itself on the launch stream between its kernels (`events` argument of stg_model_fwd / stg_model_bwd).
    Attached to ONE model (`model.timer = ops.KernelTimer()`, bench.py's roofline leg); no timer, no events."""
    MAX_KERNELS = 8

    def __init__(self):
        self.calls = {"model_fwd": [], "model_bwd": []}

    def events(self, name):
        ev = _lib.HipEvents(self.MAX_KERNELS + 1)
        self.calls[name].append(ev)
        return ev

    def kernel_ms(self, name):
        """mean duration (ms) of the k-th kernel of entry point `name` over the recorded calls; events the entry
        point did not reach are dropped (their interval cannot be read)."""
        rows = []
        for ev in self.calls[name]:
            row = []
            hip = ev.hip()
            hip.hipEventSynchronize(ev.arr[0])
            for k in range(1, ev.n):
                ms = ctypes.c_float()
                if hip.hipEventElapsedTime(ctypes.byref(ms), ev.arr[k - 1], ev.arr[k]) != 0:
                    hip.hipGetLastError()          # (an unrecorded handle: clear the runtime's sticky error)
                    break
                row.append(ms.value)
            rows.append(row)
        if not rows:
            return []
        n = min(len(r) for r in rows)
        return [sum(r[k] for r in rows) / len(rows) for k in range(n)]

    def mean_ms(self, name):
        return sum(self.kernel_ms(name))


def _timer_of(holder):
    return getattr(holder, "timer", None) if holder is not None else None


def _size(name, **kw):
    """the value of a size query of the C ABI; a negative one is a status"""
    n = int(call(name, **kw))
    if n < 0:
        check(n, name)
    return n


def _ptr_array(tensors):
    """one device pointer per tensor, as the `void* const*` arguments of the C ABI take them (None for no tensors)"""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]) if len(tensors) else None


@dataclasses.dataclass(eq=False)
class FwdRecord:
    """What ONE fused forward leaves behind for the backward and the step tail that follow it: `ctx` of the autograd
    node holds it, and so does `holder._fwd_state`, from a forward that saved activations until a backward ran."""
    desc: ModelDesc                 # the descriptor actually used (the workgroup flag may have been added)
    a_sn: int
    dead: frozenset                 # indices of the parameters forward() never touches (grad stays None)
    shapes: list                    # parameter shapes in kernel order
    flat_params: torch.Tensor
    flat_buffers: torch.Tensor
    x: torch.Tensor
    adj_c: torch.Tensor
    peds: torch.Tensor
    ws: torch.Tensor                # saved activations; None = nothing to run a backward from
    # the BatchNorm fold this forward left to the step's tail (train_tail / stg_model_bwd_step); None = folded or eval
    stats: torch.Tensor = None
    nbt: list = None
    n: int = 0


def _check_model_input(x, adj, desc, flat_params, flat_buffers):
    """the checks every fused forward starts with; returns the sizes (n, c_in, t, v) of x"""
    require_gpu(x, adj, flat_params, flat_buffers)
    _lib.as_f32(x, "x")
    _lib.as_f32(adj, "adj")
    n, cin, t, v = x.shape
    if cin != desc.c_in or t != desc.t_obs:
        raise ValueError("input (N,%d,%d,V) does not match the model (input_feat=%d, seq_len=%d)"
                         % (cin, t, desc.c_in, desc.t_obs))
    return n, cin, t, v


def _fwd_buffers(desc, n, v, dev, save, training, holder):
    """The arrays stg_model_fwd writes, sized by the library: (y, ws, stats, scratch).  ws (the saved activations) only
    when `save`, stats only when `training`, scratch only where the path needs one."""
    d = ctypes.byref(desc)
    out_t = desc.t_pred if desc.n_txpcnn > 0 else desc.t_obs
    y = torch.empty((n, desc.c_out, out_t, v), device=dev, dtype=torch.float32)
    ws = None                      # (its size is a diagnostic: last_ws_floats, 0 = inference)
    if save:
        wsf = _size("stg_model_ws_floats", d=d, V=v)
        tail = _size("stg_model_ws_tail_floats", d=d, N=n, V=v)
        ws = torch.empty(n * wsf + tail, device=dev, dtype=torch.float32)
    stats = None
    if training:
        sf = call("stg_model_stat_floats", d=d)
        stats = torch.empty((n, max(int(sf), 1)), device=dev, dtype=torch.float32)
    scr = None
    nscr = _size("stg_model_fwd_scratch_floats", d=d, N=n, V=v)
    if nscr > 0:
        scr = torch.empty(nscr, device=dev, dtype=torch.float32)
    if holder is not None:
        holder.last_ws_floats = ws.numel() if save else 0
        holder._last_fwd_scratch = scr  # diagnostics only (STG_STAMPS=1 reads the stamps in it)
    return y, ws, stats, scr


def _bwd_buffers(desc, n, v, dev):
    """The arrays the fused backward writes, sized by the library: (scratch, flat gradient)."""
    d = ctypes.byref(desc)
    np_ = int(call("stg_model_param_count", d=d))
    n_scratch = _size("stg_model_bwd_scratch_floats", d=d, N=n, V=v)
    slabs = torch.empty(n_scratch, device=dev, dtype=torch.float32)
    grad = torch.empty(np_, device=dev, dtype=torch.float32)
    return slabs, grad


def _step_tail(flat_params, flat_buffers, step, stats, nbt):
    """The tail of a single-rank step (stg_step_tail) for step = (lr, lr_dev): SGD on the flat parameters, the reported
    loss and, with `stats`, the BatchNorm fold the forward deferred.  Returns (tail, total, what must stay alive until
    the call has been made)."""
    lr, lr_dev = step
    total = torch.empty(1, device=flat_params.device, dtype=torch.float32)
    tail = _lib.StepTail()
    tail.params, tail.lr_dev, tail.lr = ptr(flat_params), ptr(lr_dev), float(lr)
    tail.total = ptr(total)
    arr = None
    if stats is not None:
        arr = _ptr_array(nbt)
        tail.stats, tail.buffers, tail.nbt, tail.n_bn = ptr(stats), ptr(flat_buffers), arr, len(nbt)
    return tail, total, arr


def _grad_views(grad, shapes, dead, holder):
    """per-parameter views of the flat gradient (None for the dead ones); the flat gradient goes to the holder"""
    if holder is not None:
        holder._flat_grad = grad           # the trainer all-reduces / applies this buffer directly
        holder._fwd_state = None
    return [None if i in dead else grad[off:off + cnt].view(shapes[i]) for i, off, cnt in flat_walk(shapes)]


def _model_head(desc, flat_params, flat_buffers, x, adj_c, a_sn, peds):
    """The arguments every fused model entry point starts with: descriptor, packed tensors, input, adjacency, sizes."""
    return dict(d=ctypes.byref(desc), params=ptr(flat_params), buffers=ptr(flat_buffers), x=ptr(x),
                **_strides("x", x, "nctv"), adj=ptr(adj_c), a_sn=a_sn, num_peds=ptr(peds), N=x.shape[0], V=x.shape[3])


def _unless_unsupported(name, **kw):
    """call(); False, in the place of the refusal, where the library has no such form (STG_EUNSUPPORTED)."""
    try:
        call(name, **kw)
    except _lib.StatusError as e:
        if e.status != _lib.EUNSUPPORTED:
            raise
        return False
    return True


class _FusedModel(torch.autograd.Function):
    """x (N,Cin,T,V), adj -> y.  Extra (non-differentiable) arguments carry the packed buffers."""

    @staticmethod
    def forward(ctx, x, adj, num_peds, desc, flat_params, flat_buffers, nbt, dead, holder, grad_on, defer_bn_fold,
                *params):
        n, cin, t, v = _check_model_input(x, adj, desc, flat_params, flat_buffers)
        adj_c, a_sn = _adj_layout(adj, n, t, v)
        peds = peds_arg(num_peds, n, x.device)
        training = desc.bn_mode == 1
        # needs_input_grad reflects requires_grad, not the grad mode (and forward() itself always runs with grad
        # disabled): the caller's grad mode comes in as `grad_on`, so that under no_grad nothing is saved
        need_grad = grad_on and any(ctx.needs_input_grad)
        if need_grad and ctx.needs_input_grad[0] and not (desc.flags & _lib.OPT_WG_PATH):
            # an input gradient is only computed by the workgroup-per-scene kernels (both passes must agree)
            fields = {f: getattr(desc, f) for f, _ in ModelDesc._fields_}
            fields["flags"] |= _lib.OPT_WG_PATH
            desc = ModelDesc(**fields)
        y, ws, stats, scr = _fwd_buffers(desc, n, v, x.device, need_grad, training, holder)
        timer = _timer_of(holder)
        ev = timer.events("model_fwd") if timer is not None else None
        call("stg_model_fwd", **_model_head(desc, flat_params, flat_buffers, x, adj_c, a_sn, peds), y=ptr(y), ws=ptr(ws),
             stats=ptr(stats), scratch=ptr(scr), events=ev.arr if ev else None, n_events=ev.n if ev else 0)
        rec = FwdRecord(desc, a_sn, dead, [tuple(p.shape) for p in params], flat_params, flat_buffers, x, adj_c, peds,
                        ws)
        if training and defer_bn_fold:
            # the trainer folds the running statistics in the step's tail launch (train_tail / stg_model_bwd_step)
            rec.stats, rec.nbt, rec.n = stats, nbt, n
        elif training:
            # nbt[k] counts forwards of BatchNorm k; buffers are interleaved (mean, var) per BatchNorm, the
            # kernel bumps counter i for statistic row i < len(nbt): pass one pointer per BatchNorm.
            call("stg_bn_fold", d=ctypes.byref(desc), stats=ptr(stats), num_peds=ptr(peds), N=n, buffers=ptr(flat_buffers),
                 nbt=_ptr_array(nbt), n_bn=len(nbt))
        if holder is not None:
            holder._fwd_state = rec if need_grad else None
        ctx.rec = rec
        ctx.holder = holder
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.rec.ws is None:
            raise RuntimeError("backward through a forward that saved no activations")
        grads, dx = _launch_backward(ctx.rec, ctx.holder, dy=dy.contiguous(), need_dx=ctx.needs_input_grad[0])
        return (dx, None, None, None, None, None, None, None, None, None, None, *grads)


def _launch_backward(rec, holder, dy=None, need_dx=False, y=None, target=None, weights=None, step=None):
    """The ONE launcher of the fused backward of the forward `rec` records.  It starts from `dy` (stg_model_bwd; also
    the input gradient when `need_dx`), or from the model output `y`, `target` and the per-scene `weights`
    (stg_model_bwd_nll), with step = (lr, lr_dev) also running the tail of a single-rank step (stg_model_bwd_step).
    Returns (per-parameter gradient views, None for the dead ones; dx | losses | (losses, total)), with the flat
    gradient left in `holder._flat_grad` -- or None, nothing launched, where the library has no form that starts from
    the target."""
    desc, x = rec.desc, rec.x
    n, cin, t, v = x.shape
    slabs, grad = _bwd_buffers(desc, n, v, x.device)
    timer = _timer_of(holder)
    ev = timer.events("model_bwd") if timer is not None else None
    common = dict(_model_head(desc, rec.flat_params, rec.flat_buffers, x, rec.adj_c, rec.a_sn, rec.peds), ws=ptr(rec.ws),
                  scratch=ptr(slabs), grad_params=ptr(grad), events=ev.arr if ev else None, n_events=ev.n if ev else 0)
    if dy is not None:
        out = torch.empty((n, cin, t, v), device=x.device, dtype=torch.float32) if need_dx else None
        call("stg_model_bwd", **common, dy=ptr(dy), dx=ptr(out))
    else:
        out = losses = torch.empty(n, device=x.device, dtype=torch.float32)
        mid = dict(y=ptr(y), target=ptr(target), weights=ptr(weights), losses=ptr(losses))
        if step is None:
            done = _unless_unsupported("stg_model_bwd_nll", **common, **mid)
        else:
            tail, total, keep = _step_tail(rec.flat_params, rec.flat_buffers, step, rec.stats, rec.nbt)
            done = _unless_unsupported("stg_model_bwd_step", **common, **mid, tail=ctypes.addressof(tail))
            out = (losses, total[0])
        if not done:
            if ev is not None:
                timer.calls["model_bwd"].pop()
            return None
    return _grad_views(grad, rec.shapes, rec.dead, holder), out


def backward_from_target(holder, y, target, weights=None, step=None):
    """Loss + backward of the fused forward `holder` (a model) just ran, in the backward's own launches
    (stg_model_bwd_nll): per-scene bivariate losses (N,) are returned, the parameter gradients of
    sum_n weights[n] * loss_n land in `holder._flat_grad` and in every live parameter's .grad (views of it).
    Returns None -- nothing launched -- where the library has no fused form (STG_OPT_SPLIT_BF16, a model without a
    TXP-CNN): the caller then takes the separate loss kernel + autograd backward.

    step = (lr, lr_dev): the rest of a single-rank training step rides in the same launches (stg_model_bwd_step: SGD
    without clipping on the flat parameters, the BatchNorm fold a forward with a deferred fold left in its record, and
    the reported loss); returns (losses, total) then."""
    rec = getattr(holder, "_fwd_state", None)
    if rec is None:
        raise RuntimeError("backward_from_target: no fused forward with saved activations to start from")
    n, _, _, v = rec.x.shape
    if tuple(y.shape) != (n, 5, rec.desc.t_pred, v) or not y.is_contiguous():
        return None
    target = target.to(torch.float32).contiguous()
    if tuple(target.shape) != (n, rec.desc.t_pred, v, 2):
        raise ValueError("backward_from_target: target (N,P,V,2) expected, got %s" % (tuple(target.shape),))
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    res = _launch_backward(rec, holder, y=y, target=target, weights=w, step=step)
    if res is None:
        return None
    for p, g in zip(holder._tensors()[0], res[0]):
        p.grad = g
    return res[1]


def fused_step(x, adj, num_peds, desc, flat_params, flat_buffers, nbt, dead, params, holder, target, weights, lr,
               lr_dev):
    """One single-rank training step without clipping in ONE library call (stg_model_step): the training forward, the
    loss, the backward and the step's tail (SGD, running-statistics fold, reported loss) -- what `fused_model` with a
    deferred fold followed by `backward_from_target(step=...)` runs, bit for bit, with the forward and the backward scene
    kernels as one launch where the library has that form.  No autograd graph is built.  Returns (V_pred (N,5,P,V),
    per-scene losses, the reported loss, per-parameter gradient views), the flat gradient left in `holder._flat_grad` --
    or None, nothing launched, where the library has no such step (the caller then takes the two calls)."""
    n, cin, t, v = _check_model_input(x, adj, desc, flat_params, flat_buffers)
    if desc.bn_mode != 1 or desc.n_txpcnn < 1 or n == 0 or (desc.flags & _lib.OPT_SPLIT_BF16):
        return None
    target = target.to(torch.float32).contiguous()
    if tuple(target.shape) != (n, desc.t_pred, v, 2):
        raise ValueError("fused_step: target (N,P,V,2) expected, got %s" % (tuple(target.shape),))
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    adj_c, a_sn = _adj_layout(adj, n, t, v)
    peds = peds_arg(num_peds, n, x.device)
    y, ws, stats, scr = _fwd_buffers(desc, n, v, x.device, True, True, holder)
    slabs, grad = _bwd_buffers(desc, n, v, x.device)
    if holder is not None:
        holder._last_bwd_scratch = slabs  # diagnostics only (STG_STAMPS=1 reads the stamps in it)
    losses = torch.empty(n, device=x.device, dtype=torch.float32)
    tail, total, keep = _step_tail(flat_params, flat_buffers, (lr, lr_dev), stats, nbt)
    timer = _timer_of(holder)
    ev_f = timer.events("model_fwd") if timer is not None else None
    ev_b = timer.events("model_bwd") if timer is not None else None
    if not _unless_unsupported(
            "stg_model_step", **_model_head(desc, flat_params, flat_buffers, x, adj_c, a_sn, peds), y=ptr(y), ws=ptr(ws),
            stats=ptr(stats), fwd_scratch=ptr(scr), target=ptr(target), weights=ptr(w), losses=ptr(losses),
            bwd_scratch=ptr(slabs), grad_params=ptr(grad), tail=ctypes.addressof(tail),
            fwd_events=ev_f.arr if ev_f else None, n_fwd_events=ev_f.n if ev_f else 0,
            bwd_events=ev_b.arr if ev_b else None, n_bwd_events=ev_b.n if ev_b else 0):
        if timer is not None:
            timer.calls["model_fwd"].pop()
            timer.calls["model_bwd"].pop()
        return None
    return y, losses, total[0], _grad_views(grad, [tuple(p.shape) for p in params], dead, holder)


def fused_model(x, adj, num_peds, desc, flat_params, flat_buffers, nbt, dead, params, holder=None,
                defer_bn_fold=False):
    """defer_bn_fold: leave the running-statistics fold of a training forward to the step's tail launch (the trainer's
    request); the statistics then travel in the forward's record (`holder._fwd_state`)."""
    return _FusedModel.apply(x, adj, num_peds, desc, flat_params, flat_buffers, nbt, dead, holder,
                             torch.is_grad_enabled(), defer_bn_fold, *params)


# --------------------------------------------------------------------------------------------
# R6 bivariate Gaussian NLL
# --------------------------------------------------------------------------------------------
class _BivariateNLL(torch.autograd.Function):
    """pred (N,P,V,5) (any strides), target (N,P,V,2) -> loss (N,)."""

    @staticmethod
    def forward(ctx, pred, target, num_peds):
        require_gpu(pred, target)
        _lib.as_f32(pred, "V_pred")
        n, p, v, f = pred.shape
        if f != 5 or tuple(target.shape) != (n, p, v, 2):
            raise ValueError("bivariate_loss: V_pred (..,P,V,5) / V_trgt (..,P,V,2) expected, got %s / %s"
                             % (tuple(pred.shape), tuple(target.shape)))
        target = target.to(torch.float32).contiguous()
        peds = peds_arg(num_peds, n, pred.device)
        loss = torch.empty(n, device=pred.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        grad = torch.empty((n, 5, p, v), device=pred.device, dtype=torch.float32) if need else None
        call("stg_nll_fwd", pred=ptr(pred), **_strides("p", pred, "npvf"), target=ptr(target), num_peds=ptr(peds),
             grad_scale=None, N=n, P=p, V=v, loss=ptr(loss), grad=ptr(grad))
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gloss):
        grad = ctx.grad
        n, _, p, v = grad.shape
        gloss = gloss.to(torch.float32).contiguous()
        out = torch.empty_like(grad)
        call("stg_nll_bwd", grad=ptr(grad), gloss=ptr(gloss), N=n, P=p, V=v, out=ptr(out))
        # (N,5,P,V) buffer viewed in the caller's (N,P,V,5) index order
        return out.permute(0, 2, 3, 1), None, None


def bivariate_nll(pred, target, num_peds=None):
    return _BivariateNLL.apply(pred, target, num_peds)


def bivariate_nll_with_grad(y, target, num_peds=None, weights=None):
    """Trainer fast path: y (N,5,P,V) model output (contiguous), target (N,P,V,2) ->
    (per-scene losses (N,), d(sum_n w_n loss_n)/dy (N,5,P,V)) from ONE nll_fwd launch."""
    require_gpu(y, target)
    n, f, p, v = y.shape
    if f != 5 or tuple(target.shape) != (n, p, v, 2):
        raise ValueError("bivariate_nll_with_grad: y (N,5,P,V) / target (N,P,V,2) expected")
    target = target.to(torch.float32).contiguous()
    peds = peds_arg(num_peds, n, y.device)
    loss = torch.empty(n, device=y.device, dtype=torch.float32)
    grad = torch.empty((n, 5, p, v), device=y.device, dtype=torch.float32)
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    call("stg_nll_fwd", pred=ptr(y), **_strides("p", y, "nfpv"), target=ptr(target), num_peds=ptr(peds),
         grad_scale=ptr(w), N=n, P=p, V=v, loss=ptr(loss), grad=ptr(grad))
    return loss, grad


def sgd_step(flat_params, flat_grads, lr):
    """p -= lr * g on the flat buffers (train.py:197 SGD without momentum)."""
    require_gpu(flat_params, flat_grads)
    call("stg_sgd_step", params=ptr(flat_params), grads=ptr(flat_grads), count=flat_params.numel(), lr=float(lr))


def optim_step(flat_params, flat_grads, lr, max_norm=None, lr_dev=None, grad_norm=None):
    """clip_grad_norm_(max_norm) + SGD(lr) on the flat buffers in one launch (train.py:71-74,197).  `lr_dev`
    (1-element device tensor) overrides `lr` -- the form a captured hipGraph needs to follow StepLR; `grad_norm`
    (1-element device tensor) receives the unclipped gradient norm.  The gradients are scaled in place."""
    require_gpu(flat_params, flat_grads)
    call("stg_optim_step", params=ptr(flat_params), grads=ptr(flat_grads), count=flat_params.numel(), lr_dev=ptr(lr_dev),
         lr=float(lr), max_norm=float(max_norm) if max_norm is not None else 0.0, grad_norm=ptr(grad_norm))


def train_tail(rec, losses, weights, flat_params, flat_grads, lr, max_norm=None, lr_dev=None):
    """The tail of a single-rank step in one launch (stg_train_tail): the BatchNorm fold that the forward of record
    `rec` deferred, the reported loss sum_n w_n loss_n, clip + SGD.  Returns the loss as a 0-d device tensor."""
    require_gpu(losses, flat_params, flat_grads)
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    out = torch.empty(1, device=losses.device, dtype=torch.float32)
    call("stg_train_tail", d=ctypes.byref(rec.desc), stats=ptr(rec.stats), num_peds=ptr(rec.peds), N=rec.n,
         buffers=ptr(rec.flat_buffers), nbt=_ptr_array(rec.nbt), n_bn=len(rec.nbt), losses=ptr(losses), weights=ptr(w),
         total=ptr(out), params=ptr(flat_params), grads=ptr(flat_grads), count=flat_params.numel(), lr_dev=ptr(lr_dev),
         lr=float(lr), max_norm=float(max_norm) if max_norm is not None else 0.0, grad_norm=None)
    return out[0]


def dp_pack(flat_grad, bn_before, bn_after, num_peds, n_scenes, momentum, rank, world, pack):
    """[gradient | this rank's BatchNorm contribution and scene count] into the ONE buffer a data-parallel step
    all-reduces (stg_dp_pack).  pack: n_params + world * (n_buffers + 1) floats."""
    require_gpu(flat_grad, bn_before, bn_after, pack)
    peds = peds_arg(num_peds, n_scenes, flat_grad.device)
    call("stg_dp_pack", grads=ptr(flat_grad), bn_before=ptr(bn_before), bn_after=ptr(bn_after), num_peds=ptr(peds),
         N=int(n_scenes), momentum=float(momentum), rank=int(rank), world=int(world), n_params=flat_grad.numel(),
         n_buffers=bn_before.numel(), pack=ptr(pack))


def dp_fold(pack, bn_before, momentum, rank, world, n_params, buffers, nbt=()):
    """the exact sequential fold of the running statistics over the ranks from the all-reduced pack (stg_dp_fold);
    `nbt` (the num_batches_tracked tensors) also receive the other ranks' scene counts from the pack."""
    require_gpu(pack, bn_before, buffers)
    call("stg_dp_fold", pack=ptr(pack), bn_before=ptr(bn_before), momentum=float(momentum), rank=int(rank),
         world=int(world), n_params=int(n_params), n_buffers=bn_before.numel(), buffers=ptr(buffers), nbt=_ptr_array(nbt),
         n_bn=len(nbt))


def weighted_sum(values, weights=None):
    """sum_n w_n v_n as a 1-element device tensor (one launch, fixed summation order)."""
    require_gpu(values)
    values = values.contiguous()
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    out = torch.empty(1, device=values.device, dtype=torch.float32)
    call("stg_weighted_sum", values=ptr(values), weights=ptr(w), N=values.numel(), out=ptr(out))
    return out[0]


def sample_args(what, y, k, obs_last, noise, seed_dev=None):
    """The argument rule of the sampling family (best_of_k, sample_trajectories, sample_risk; `what` names the caller
    in the messages): y (N,5,P,V), obs_last (N,V,2) or None, noise (k,N,P,V,2) or None, seed_dev a one-element int64
    device tensor or None.  Returns (y as float32, obs_last and noise as contiguous float32 on y's device, N, P, V)."""
    if y.dim() != 4 or y.shape[1] != 5:
        raise ValueError("%s: y (N,5,P,V) expected" % what)
    n, _, p, v = y.shape
    y = y.to(torch.float32)
    if obs_last is not None:
        if tuple(obs_last.shape) != (n, v, 2):
            raise ValueError("%s: obs_last (N,V,2) expected" % what)
        obs_last = obs_last.to(device=y.device, dtype=torch.float32).contiguous()
    if noise is not None:
        if tuple(noise.shape) != (k, n, p, v, 2):
            raise ValueError("%s: noise (K,N,P,V,2) expected" % what)
        noise = noise.to(device=y.device, dtype=torch.float32).contiguous()
    if seed_dev is not None and (seed_dev.numel() != 1 or seed_dev.dtype != torch.int64):
        raise ValueError("%s: seed_dev must be a one-element int64 device tensor" % what)
    return y, obs_last, noise, n, p, v


def _sampler_head(y, obs_last, peds, noise, seed, seed_dev, k):
    """What stg_sample_trajectories and stg_sample_risk take alike: the model output, the draws and the sizes."""
    n, _, p, v = y.shape
    return dict(pred=ptr(y), **_strides("p", y, "nfpv"), obs_last=ptr(obs_last), num_peds=ptr(peds), noise=ptr(noise),
                seed=seed_u64(seed), seed_dev=ptr(seed_dev), N=n, P=p, V=v, K=k)


def best_of_k(y, target_rel, obs_last=None, num_peds=None, k=20, noise=None, seed=0):
    """Evaluation tail of test.py:59-123 on the device: y (N,5,P,V) model output (any strides), target_rel
    (N,P,V,2), obs_last (N,V,2) or None, noise (K,N,P,V,2) standard normals or None (in-kernel Philox stream keyed
    by `seed`).  Returns per-pedestrian (min ADE, min FDE), each (N,V) with zeros in padded slots."""
    require_gpu(y, target_rel)
    k = int(k)
    y, obs_last, noise, n, p, v = sample_args("best_of_k", y, k, obs_last, noise)
    if tuple(target_rel.shape) != (n, p, v, 2):
        raise ValueError("best_of_k: target_rel (N,P,V,2) expected")
    target_rel = target_rel.to(torch.float32).contiguous()
    peds = peds_arg(num_peds, n, y.device)
    ade = torch.empty((n, v), device=y.device, dtype=torch.float32)
    fde = torch.empty((n, v), device=y.device, dtype=torch.float32)
    call("stg_bestofk_eval", pred=ptr(y), **_strides("p", y, "nfpv"), target_rel=ptr(target_rel), obs_last=ptr(obs_last),
         num_peds=ptr(peds), noise=ptr(noise), seed=seed_u64(seed), N=n, P=p, V=v, K=k, ade=ptr(ade), fde=ptr(fde))
    return ade, fde


DistMetrics = collections.namedtuple("DistMetrics", "d2 nll lam kde_nll ade fde jade jfde jbest")
DistMetrics.__doc__ = """A batch of predictions judged against the truth (`stg_dist_metrics`, DESIGN.md 5.31), float32 device
tensors, zeros in padded slots.  (N,P,V): d2 (squared Mahalanobis distance of the truth under N(mean_h, C_h), C_h the
cumulative covariance of the live score), nll (of that Gaussian), lam (the larger eigenvalue of C_h), kde_nll (minus the
log density at the truth of the Gaussian KDE of the K samples at that horizon, Scott's bandwidth, clipped from above at
kde_floor).  (N,V): ade, fde, the best-of-K errors over the given samples.  (N,): jade, jfde -- the minimum over k of
the scene's mean error, ONE sample for every pedestrian of the scene -- and jbest int32, the k of jade (-1 for an empty
scene).  The sample-based fields (kde_nll and after) are None without samples."""
_DIST_SAMPLED = ("kde_nll", "ade", "fde", "jade", "jfde", "jbest")


def dist_buffers(n, p, v, device, samples=True, cov=False):
    """Empty outputs for dist_metrics on n scenes: (DistMetrics, cov (N,P,V,3) or None)."""
    def f32(*shape):
        return torch.empty(shape, device=device, dtype=torch.float32)
    s = bool(samples)
    m = DistMetrics(f32(n, p, v), f32(n, p, v), f32(n, p, v), f32(n, p, v) if s else None, f32(n, v) if s else None,
                    f32(n, v) if s else None, f32(n) if s else None, f32(n) if s else None,
                    torch.empty((n,), device=device, dtype=torch.int32) if s else None)
    return m, (f32(n, p, v, 3) if cov else None)


def dist_metrics(v_pred, mean, samples, truth, num_peds=None, kde_floor=20.0, out=None, cov=None, ref_errors=None):
    """Distribution metrics of a batch of predictions on the device (`stg_dist_metrics`): v_pred (N,5,P,V) model output
    (any strides), mean (N,P,V,2) and samples (K,N,P,V,2) as `sample_trajectories` / `Predictor.predict` leave them
    (samples None: the closed-form fields only; else 3 <= K <= 64), truth (N,P,V,2) absolute positions, num_peds (N,) or
    None.  kde_floor: kde_nll is clipped from above at this value (the log density from below at -kde_floor).
    out: an earlier DistMetrics of the same call to fill, cov: a contiguous float32 (N,P,V,3) tensor that receives C_h
    (graph capture: nothing is allocated then).  ref_errors: a pair of contiguous float64 (N,V) device tensors that
    receive the best-of-K ADE / FDE in the reference's own arithmetic (float32 differences and squares, float64 root and
    sum over t: what predict.sample_test computes on the host from the same samples); needs samples.
    Returns a DistMetrics."""
    require_gpu(v_pred, mean, samples, truth, cov)
    if ref_errors is not None:
        if samples is None or len(ref_errors) != 2:
            raise ValueError("dist_metrics: ref_errors is a pair (ade, fde) and needs samples")
        require_gpu(*ref_errors)
        for x in ref_errors:
            if tuple(x.shape) != tuple(v_pred.shape[::3]) or x.dtype != torch.float64 or not x.is_contiguous():
                raise ValueError("dist_metrics: ref_errors must be contiguous float64 (N,V) tensors")
    if v_pred.dim() != 4 or v_pred.shape[1] != 5:
        raise ValueError("dist_metrics: v_pred (N,5,P,V) expected")
    n, _, p, v = v_pred.shape
    _lib.as_f32(v_pred, "v_pred")
    k = 0 if samples is None else int(samples.shape[0])
    for name, x, shape in (("mean", mean, (n, p, v, 2)), ("truth", truth, (n, p, v, 2)),
                           ("samples", samples, (k, n, p, v, 2)), ("cov", cov, (n, p, v, 3))):
        if x is not None and (tuple(x.shape) != shape or x.dtype != torch.float32 or not x.is_contiguous()):
            raise ValueError("dist_metrics: %s must be a contiguous float32 %s tensor" % (name, shape))
    if samples is not None and not 3 <= k <= SCORE_MAX_K:
        raise ValueError("dist_metrics: K=%d samples (3 <= K <= %d, or samples=None)" % (k, SCORE_MAX_K))
    for what, got, most in (("V", v, SCORE_MAX_V), ("P", p, SCORE_MAX_P)):
        if got > most:
            raise ValueError("dist_metrics: %s=%d above the kernel's limit of %d" % (what, got, most))
    if not float(kde_floor) == float(kde_floor):
        raise ValueError("dist_metrics: kde_floor must be a number")
    if out is None:
        out = dist_buffers(n, p, v, v_pred.device, k > 0)[0]
    else:
        want = dist_buffers(n, p, v, "meta", k > 0)[0]
        for name, o, w in zip(DistMetrics._fields, out, want):
            if (o is None) != (w is None) or (o is not None and (
                    tuple(o.shape) != tuple(w.shape) or o.dtype != w.dtype or not o.is_contiguous() or not o.is_cuda)):
                raise ValueError("dist_metrics: out.%s does not fit this call (%s)"
                                 % (name, "None" if w is None else "contiguous %s %s" % (w.dtype, tuple(w.shape))))
    peds = peds_arg(num_peds, n, v_pred.device)
    ade_ref, fde_ref = ref_errors or (None, None)
    call("stg_dist_metrics", v_pred=ptr(v_pred), **_strides("p", v_pred, "nfpv"), mean=ptr(mean), samples=ptr(samples),
         truth=ptr(truth), num_peds=ptr(peds), N=n, P=p, V=v, K=k, kde_floor=float(kde_floor), cov=ptr(cov),
         **{name: ptr(o) for name, o in out._asdict().items()}, ade_ref=ptr(ade_ref), fde_ref=ptr(fde_ref))
    return out


CalibFit = collections.namedtuple("CalibFit", "g bracket flags stats sig")
CalibFit.__doc__ = """What `stg_calib_fit` leaves on the device (DESIGN.md 5.32): g float32 (P,), the fitted factor on the
covariance of every predicted step; bracket float32 (P,2), the search's final (lo, hi) with g = hi; flags int32 (P,), 0
or CALIB_LOW / CALIB_HIGH (the search ran into its clamp 2^-10 / 2^21) / CALIB_EMPTY (no element, g = 1); stats float64
(P,3) = the number of elements, the sum of d2 at g and the number with d2 <= thr at g; sig float32 (N,P,V,3), the
per-step covariance terms [sx^2, rho sx sy, sy^2] as the kernel computed them."""
CALIB_MODES = {"moment": 0, "coverage": 1}                                  # STG_CALIB_MOMENT, STG_CALIB_COVERAGE
CALIB_LOW, CALIB_HIGH, CALIB_EMPTY = 1, 2, 4                                # STG_CALIB_*


def calib_buffers(n, p, v, device):
    """Empty outputs and the scratch buffer of calib_fit on n scenes: (CalibFit, ws uint8)."""
    def e(dtype, *shape):
        return torch.empty(shape, device=device, dtype=dtype)
    nbytes = _size("stg_calib_fit_ws_bytes", N=n, P=p, V=v) if str(device) != "meta" else 0
    # (float64 storage: the scratch buffer is 8-byte aligned whatever the allocator hands out)
    ws = torch.empty(((nbytes + 7) // 8,), device=device, dtype=torch.float64)
    return CalibFit(e(torch.float32, p), e(torch.float32, p, 2), e(torch.int32, p), e(torch.float64, p, 3),
                    e(torch.float32, n, p, v, 3)), ws


def calib_fit(v_pred, mean, truth, num_peds=None, mode="coverage", level=0.9, out=None, ws=None):
    """Fit one factor per predicted step on a set of predictions against the truth (`stg_calib_fit`): v_pred (N,5,P,V)
    model output (any strides), mean (N,P,V,2) as the sampler leaves it, truth (N,P,V,2) absolute positions, num_peds
    (N,) or None.  mode "moment": the smallest searched g_h at which the mean d2 at horizon h is at most 2; "coverage":
    at which the ellipse of probability `level` (a float32) holds at least that share of the truths.  The fit is
    sequential over the horizons and needs the whole set in ONE call.  out, ws: calib_buffers(N, P, V, device) of an
    earlier call (graph capture: nothing is allocated then).  Returns a CalibFit of device tensors; nothing is
    synchronised."""
    require_gpu(v_pred, mean, truth)
    if v_pred.dim() != 4 or v_pred.shape[1] != 5:
        raise ValueError("calib_fit: v_pred (N,5,P,V) expected")
    n, _, p, v = v_pred.shape
    _lib.as_f32(v_pred, "v_pred")
    for name, x in (("mean", mean), ("truth", truth)):
        if tuple(x.shape) != (n, p, v, 2) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("calib_fit: %s must be a contiguous float32 %s tensor" % (name, (n, p, v, 2)))
    if mode not in CALIB_MODES:
        raise ValueError("calib_fit: mode must be one of %s, got %r" % (sorted(CALIB_MODES), mode))
    level = float(np.float32(level))
    if not 0.0 < level < 1.0:
        raise ValueError("calib_fit: level must lie in (0, 1), got %r" % (level,))
    for what, got, most in (("V", v, SCORE_MAX_V), ("P", p, SCORE_MAX_P)):
        if got > most:
            raise ValueError("calib_fit: %s=%d above the kernel's limit of %d" % (what, got, most))
    if (out is None) != (ws is None):
        raise ValueError("calib_fit: out and ws go together (calib_buffers)")
    if out is None:
        out, ws = calib_buffers(n, p, v, v_pred.device)
    else:
        want = calib_buffers(n, p, v, "meta")[0]
        for name, o, w in zip(CalibFit._fields, out, want):
            if tuple(o.shape) != tuple(w.shape) or o.dtype != w.dtype or not o.is_contiguous() or not o.is_cuda:
                raise ValueError("calib_fit: out.%s does not fit this call (contiguous %s %s)"
                                 % (name, w.dtype, tuple(w.shape)))
        require_gpu(ws)
    peds = peds_arg(num_peds, n, v_pred.device)
    if n == 0:                                              # nothing to launch: the result of a fit without elements
        out.g.fill_(1.0)
        out.bracket.fill_(1.0)
        out.flags.fill_(CALIB_EMPTY)
        out.stats.zero_()
        return out
    call("stg_calib_fit", v_pred=ptr(v_pred), **_strides("p", v_pred, "nfpv"), mean=ptr(mean), truth=ptr(truth),
         num_peds=ptr(peds), N=n, P=p, V=v, mode=CALIB_MODES[mode], level=level,
         **{name: ptr(o) for name, o in out._asdict().items()}, ws=ptr(ws), ws_bytes=ws.numel() * ws.element_size())
    return out


def calib_shift(g):
    """The log-sigma shift of the factors g: float32(0.5 log(float64 g)), on the host."""
    g = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g, np.float32)
    if g.ndim != 1 or not (np.isfinite(g).all() and (g > 0).all()):
        raise ValueError("calib_shift: g must be a vector of positive finite factors")
    return (0.5 * np.log(g.astype(np.float64))).astype(np.float32)


def calib_apply(v_pred, shift, out=None):
    """v_pred[:, 2:4, t, :] += shift[t] on the device (`stg_calib_apply`), one launch over every V slot: v_pred
    (N,5,P,V) float32 (any strides), shift (P,) float32 device tensor (calib_shift).  out None: in place; else a float32
    (N,5,P,V) tensor (any strides) that receives all five fields.  Returns the tensor written."""
    require_gpu(v_pred, shift, out)
    if v_pred.dim() != 4 or v_pred.shape[1] != 5:
        raise ValueError("calib_apply: v_pred (N,5,P,V) expected")
    n, _, p, v = v_pred.shape
    _lib.as_f32(v_pred, "v_pred")
    if tuple(shift.shape) != (p,) or shift.dtype != torch.float32 or not shift.is_contiguous():
        raise ValueError("calib_apply: shift must be a contiguous float32 (%d,) tensor" % p)
    if out is not None and (tuple(out.shape) != (n, 5, p, v) or out.dtype != torch.float32):
        raise ValueError("calib_apply: out must be a float32 %s tensor" % ((n, 5, p, v),))
    o_strides = _strides("o", out, "nfpv") if out is not None else dict(o_sn=0, o_sf=0, o_sp=0, o_sv=0)
    call("stg_calib_apply", v_pred=ptr(v_pred), **_strides("p", v_pred, "nfpv"), shift=ptr(shift), N=n, P=p, V=v,
         out=ptr(out), **o_strides)
    return v_pred if out is None else out


def sample_trajectories(y, obs_last=None, num_peds=None, k=20, noise=None, seed=0, seed_dev=None, samples=None,
                        mean=None):
    """The sampled trajectories of test.py:59-91 on the device (`stg_sample_trajectories`): y (N,5,P,V) model output
    (any strides), obs_last (N,V,2) or None (trajectories from the origin), noise (K,N,P,V,2) standard normals or None
    (in-kernel Philox stream keyed by `seed`, or by the one-element int64 device tensor `seed_dev`, read when the kernel
    runs).  The draws are `best_of_k`'s for the same seed / noise.  samples / mean: preallocated outputs (graph
    capture), contiguous float32.  Returns (samples (K,N,P,V,2), mean (N,P,V,2)), zeros in padded slots."""
    require_gpu(y, seed_dev, samples, mean)
    k = int(k)
    if k < 0:
        raise ValueError("sample_trajectories: k must be >= 0")
    y, obs_last, noise, n, p, v = sample_args("sample_trajectories", y, k, obs_last, noise, seed_dev)
    for name, out, shape in (("samples", samples, (k, n, p, v, 2)), ("mean", mean, (n, p, v, 2))):
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError("sample_trajectories: %s must be a contiguous float32 %s tensor" % (name, shape))
    peds = peds_arg(num_peds, n, y.device)
    if samples is None:
        samples = torch.empty((k, n, p, v, 2), device=y.device, dtype=torch.float32)
    if mean is None:
        mean = torch.empty((n, p, v, 2), device=y.device, dtype=torch.float32)
    call("stg_sample_trajectories", **_sampler_head(y, obs_last, peds, noise, seed, seed_dev, k),
         samples=ptr(samples) if k > 0 else None, mean=ptr(mean))
    return samples, mean


Risk = collections.namedtuple("Risk", "k conflict conflict_any partner pair zone_any zone_count ped_zone")
Risk.__doc__ = """int32 counts over the k samples (`stg_sample_risk`): conflict (N,P,V), conflict_any (N,V), partner (N,V)
(-1: nobody), pair (N,V,V), zone_any (N,P,Z), zone_count (N,P,Z), ped_zone (N,V,Z); a count / k is the estimated
probability.  Fields that were not asked for are None.  Padded slots are 0 (-1 in partner)."""
RISK_MAX_V, RISK_MAX_K, RISK_MAX_Z, RISK_MAX_P = 256, 64, 16, 32          # STG_RISK_MAX_*


def risk_buffers(n, p, v, k, radius, z, pairs, device):
    """An empty Risk for n scenes: the outputs sample_risk fills for this radius (None / <= 0: no conflict outputs),
    z rectangles (0: no zone outputs) and pairs (the (N,V,V) pair counts)."""
    def i32(*shape):
        return torch.empty(shape, device=device, dtype=torch.int32)
    conf = radius is not None and radius > 0
    return Risk(int(k), i32(n, p, v) if conf else None, i32(n, v) if conf else None, i32(n, v) if conf else None,
                i32(n, v, v) if conf and pairs else None, i32(n, p, z) if z else None, i32(n, p, z) if z else None,
                i32(n, v, z) if z else None)


def risk_zones(zones, n, device):
    """The rule for sample_risk's rectangles: (Z,4) shared by the n scenes or (n,Z,4) per scene, Z >= 1, or None.
    Returns (contiguous float32 tensor on `device` or None, Z, the scene stride z_sn the kernel takes: 0 = shared)."""
    if zones is None:
        return None, 0, 0
    zones = torch.as_tensor(zones, dtype=torch.float32).to(device=device).contiguous()
    if zones.dim() == 2 and zones.shape[1] == 4:
        z, z_sn = zones.shape[0], 0
    elif zones.dim() == 3 and zones.shape[0] == n and zones.shape[2] == 4:
        z, z_sn = zones.shape[1], zones.shape[1] * 4
    else:
        raise ValueError("sample_risk: zones (Z,4) or (N,Z,4) expected, got %s" % (tuple(zones.shape),))
    if z < 1:
        raise ValueError("sample_risk: zones holds no rectangle (pass None)")
    return zones, z, z_sn


def sample_risk(y, obs_last=None, num_peds=None, k=20, radius=None, zones=None, noise=None, seed=0, seed_dev=None,
                pairs=False, out=None):
    """Conflict and zone-occupancy counts over the k samples `sample_trajectories` would write for the same arguments,
    reduced on the device without writing the samples (`stg_sample_risk`).  y, obs_last, num_peds, noise, seed and
    seed_dev as there.  radius: two pedestrians of a sample conflict at a step when they are closer than this (strictly;
    None: no conflict outputs); zones: (Z,4) rectangles [x0,y0,x1,y1] shared by the scenes or (N,Z,4) per scene
    (x0 <= x < x1 and y0 <= y < y1 is inside; None: no zone outputs); pairs: also the (N,V,V) pair counts.
    out: an earlier Risk of the same call to fill (graph capture).  Returns a Risk."""
    require_gpu(y, seed_dev)
    k = int(k)
    if k < 1:
        raise ValueError("sample_risk: k must be >= 1")
    radius = None if radius is None else float(radius)
    if radius is not None and not radius > 0:
        raise ValueError("sample_risk: radius must be > 0 (None: no conflict outputs), got %r" % (radius,))
    if radius is None and zones is None:
        raise ValueError("sample_risk: nothing to compute (neither a radius nor zones)")
    if pairs and radius is None:
        raise ValueError("sample_risk: pairs=True needs a radius")
    y, obs_last, noise, n, p, v = sample_args("sample_risk", y, k, obs_last, noise, seed_dev)
    zones, z, z_sn = risk_zones(zones, n, y.device)
    for what, got, most in (("V", v, RISK_MAX_V), ("k", k, RISK_MAX_K), ("Z", z, RISK_MAX_Z), ("P", p, RISK_MAX_P)):
        if got > most:
            raise ValueError("sample_risk: %s=%d above the kernel's limit of %d" % (what, got, most))
    want = risk_buffers(n, p, v, k, radius, z, pairs, "meta")
    if out is None:
        out = risk_buffers(n, p, v, k, radius, z, pairs, y.device)
    else:
        if out.k != k:
            raise ValueError("sample_risk: out was made for k=%d, not %d" % (out.k, k))
        for name, o, w in zip(Risk._fields[1:], out[1:], want[1:]):
            if (o is None) != (w is None) or (o is not None and (
                    tuple(o.shape) != tuple(w.shape) or o.dtype != torch.int32 or not o.is_contiguous()
                    or not o.is_cuda)):
                raise ValueError("sample_risk: out.%s does not fit this call (%s)"
                                 % (name, "None" if w is None else "contiguous int32 %s" % (tuple(w.shape),)))
    peds = peds_arg(num_peds, n, y.device)
    call("stg_sample_risk", **_sampler_head(y, obs_last, peds, noise, seed, seed_dev, k),
         radius=radius if radius is not None else 0.0, zones=ptr(zones), z_sn=z_sn, Z=z,
         **{name: ptr(o) for name, o in out._asdict().items() if name != "k"})
    return out


ScoreState = collections.namedtuple("ScoreState", "rec_ids rec_peds rec_mean rec_cov rec_samples acc acc_mean steps head "
                                                 "totals traj_totals")
ScoreState.__doc__ = """The device state of `score_push` (stg_score_state), NS leading: the ring of P records per stream
-- rec_ids (NS,P,V) int64, rec_peds (NS,P) int32, rec_mean (NS,P,P,V,2), rec_cov (NS,P,P,V,3), rec_samples
(NS,P,K,P,V,2) and the accumulators acc (NS,P,K,V), acc_mean (NS,P,V) float32, steps (NS,P,V) int32 --, head (NS,2) int32
{ring row of the next push, records that exist}, and the running totals: totals (NS,P,5+Q) float64 = per horizon
{matched, sum err, sum d2, sum nll, sum best, #(d2 <= thr_q)}, traj_totals (NS,5) float64 = {full trajectories, the sums of
their traj_ade, traj_fde, traj_ade_mean, traj_fde_mean}.  rec_samples and acc are None when samples are not scored."""
Score = collections.namedtuple("Score", "rec_ids matched err d2 nll best traj_steps traj_ade traj_fde traj_ade_mean "
                                        "traj_fde_mean")
Score.__doc__ = """One push scored (`stg_score_push`), NS leading.  Row h-1 of the (NS,P,V) fields is the prediction made
h pushes ago, scored at its step h against this push's detections: rec_ids int64 (the id where matched, else -1),
matched int32, err (displacement of the mean trajectory), d2 (squared Mahalanobis distance under the predicted
Gaussian, its determinant floored at 2^-15 cxx cyy so that a saturated correlation gives a large finite value), nll
and best (min over the K samples) float32.  The (NS,V) fields are the record that turned P pushes old:
traj_steps int32 (the steps at which its pedestrian was matched), traj_ade / traj_fde (best-of-K; the reference's ADE /
FDE where traj_steps == P) and traj_ade_mean / traj_fde_mean (the zero-noise trajectory).  Unmatched and padded entries
are 0.  best, traj_ade and traj_fde are None when samples are not scored."""
SCORE_MAX_V, SCORE_MAX_K, SCORE_MAX_P, SCORE_MAX_Q = 256, 64, 32, 4          # STG_SCORE_MAX_*
SCORE_MAX_PENDING = 1024                                                     # STG_SCORE_MAX_PENDING
_SCORE_SAMPLED = ("rec_samples", "acc")                                      # the fields that are None without samples
_SCORE_DTYPES = dict(rec_t=torch.int64, rec_ids=torch.int64, counters=torch.int64, totals=torch.float64,
                     traj_totals=torch.float64)                              # (every other field is float32)
_SCORE_DTYPES.update({n: torch.int32 for n in ("rec_status", "rec_peds", "steps", "head", "matched", "traj_steps")})


# ---- what score_push and score_timed_push share: `what` is the caller's name, `kind` its state's namedtuple and
# `sampled` the fields of it that are None when samples are not scored
def _score_shapes(ns, p, v, k, q):
    return dict(rec_ids=(ns, p, v), rec_peds=(ns, p), rec_mean=(ns, p, p, v, 2), rec_cov=(ns, p, p, v, 3),
                rec_samples=(ns, p, k, p, v, 2), acc=(ns, p, k, v), acc_mean=(ns, p, v), steps=(ns, p, v), head=(ns, 2),
                totals=(ns, p, 5 + q), traj_totals=(ns, 5))


def _score_limits(what, **sizes):
    most = dict(v=SCORE_MAX_V, k=SCORE_MAX_K, p=SCORE_MAX_P, q=SCORE_MAX_Q, pending=SCORE_MAX_PENDING)
    for name, got in sizes.items():
        if got > most[name.lower()]:
            raise ValueError("%s: %s=%d above the kernel's limit of %d" % (what, name, got, most[name.lower()]))


def _score_cleared(kind, sampled, shapes, k, device):
    return kind(*[None if (k == 0 and n in sampled) else
                  torch.full(shapes[n], -1 if n == "rec_ids" else 0, device=device,
                             dtype=_SCORE_DTYPES.get(n, torch.float32)) for n in kind._fields])


def _score_prediction(what, state, mean, v_pred, samples, ids, num_peds):
    """The prediction as the chain leaves it -> (ns, p, v, k); k = 0 where no samples are scored."""
    if v_pred.dim() != 4 or v_pred.shape[1] != 5:
        raise ValueError("%s: v_pred (NS,5,P,V) expected" % what)
    ns, _, p, v = v_pred.shape
    _lib.as_f32(v_pred, "v_pred")
    if tuple(mean.shape) != (ns, p, v, 2) or mean.dtype != torch.float32 or not mean.is_contiguous():
        raise ValueError("%s: mean must be a contiguous float32 (NS,P,V,2) tensor" % what)
    k = 0 if samples is None or state.rec_samples is None else samples.shape[0]
    if k and (tuple(samples.shape) != (k, ns, p, v, 2) or samples.dtype != torch.float32 or not samples.is_contiguous()):
        raise ValueError("%s: samples must be a contiguous float32 (K,NS,P,V,2) tensor" % what)
    if ids.numel() != ns * v or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise ValueError("%s: ids must be a contiguous int64 (NS,V) tensor" % what)
    if num_peds.numel() != ns or num_peds.dtype != torch.int32:
        raise ValueError("%s: num_peds must be an int32 (NS,) tensor" % what)
    return ns, p, v, k


def _score_state_fits(what, sampled, state, want, k, thr, q):
    for name, x in zip(state._fields, state):
        if k == 0 and name in sampled:
            continue
        if x is None or tuple(x.shape) != want[name] or not x.is_contiguous():
            raise ValueError("%s: state.%s does not fit this call (%s expected)" % (what, name, want[name]))
    if q and (thr is None or thr.numel() != q or thr.dtype != torch.float32 or not thr.is_cuda):
        raise ValueError("%s: thr must be a float32 device tensor of %d thresholds" % (what, q))


def _score_out_fits(what, out, fresh, device):
    """`out`, or fresh(device) when there is none; an `out` must look like fresh("meta") field for field."""
    if out is None:
        return fresh(device)
    for name, o, w in zip(out._fields, out, fresh("meta")):
        if (o is None) != (w is None) or (o is not None and (
                tuple(o.shape) != tuple(w.shape) or o.dtype != w.dtype or not o.is_contiguous() or not o.is_cuda)):
            raise ValueError("%s: out.%s does not fit this call" % (what, name))
    return out


def _score_tail(structs, sampled, state, out, thr, mean, v_pred, samples, ids, num_peds, p, v, k, q):
    """The arguments every score entry point takes alike: the prediction, its sizes, the state and the outputs."""
    st = structs[0](*[None if (x is None or (k == 0 and name in sampled)) else x.data_ptr()
                      for name, x in zip(state._fields, state)])
    so = structs[1](*[None if o is None else o.data_ptr() for o in out])
    return dict(mean=ptr(mean), v_pred=ptr(v_pred), **_strides("p", v_pred, "nfpv"), samples=ptr(samples) if k else None,
                ids=ptr(ids), num_peds=ptr(num_peds), P=p, V=v, K=k, state=ctypes.byref(st), thr=ptr(thr) if q else None,
                Q=q, out=ctypes.byref(so))


def score_thresholds(levels):
    """Probability levels -> the d2 thresholds of a bivariate Gaussian: P(d2 <= thr) = p for thr = -2 ln(1 - p) (d2 is
    chi-square with two degrees of freedom).  At most SCORE_MAX_Q levels, each in (0, 1)."""
    levels = [float(x) for x in levels]
    if len(levels) > SCORE_MAX_Q:
        raise ValueError("score: at most %d levels, got %d" % (SCORE_MAX_Q, len(levels)))
    for x in levels:
        if not 0.0 < x < 1.0:
            raise ValueError("score: a level must lie in (0, 1), got %r" % (x,))
    return [-2.0 * math.log1p(-x) for x in levels]


def score_state(ns, p, v, k, device, samples=True, q=3):
    """A cleared ScoreState for ns streams, horizons p, scenes padded to v pedestrians, k samples and q coverage
    thresholds.  samples=False (or k = 0): the samples are not kept and nothing sample-based is scored.
    Size: with samples P*V*(8 + 20P + 8KP + 4K + 8) bytes per stream -- about 3.5 MB at P 12, V 128, K 20, so 600
    streams hold about 2.1 GB --, about 0.4 MB per stream without samples; the totals add 8P(5+q) + 40 bytes."""
    ns, p, v, k, q = int(ns), int(p), int(v), int(k) if samples else 0, int(q)
    _score_limits("score_state", V=v, k=k, P=p, q=q)
    if ns < 1 or p < 1 or v < 1 or k < 0 or q < 0:
        raise ValueError("score_state: bad sizes ns=%d p=%d v=%d k=%d q=%d" % (ns, p, v, k, q))
    return _score_cleared(ScoreState, _SCORE_SAMPLED, _score_shapes(ns, p, v, k, q), k, device)


def score_reset(state, streams=None):
    """Clear records and totals of every stream, or of the stream indices in the int64 device tensor `streams`."""
    for name, x in zip(state._fields, state):
        if x is None:
            continue
        fill = -1 if name == "rec_ids" else 0
        if streams is None:
            x.fill_(fill)
        else:
            x.index_fill_(0, streams, fill)


def score_buffers(ns, p, v, device, samples=True):
    """An empty Score for ns streams (graph capture: the outputs `score_push(out=...)` fills)."""
    def e(dtype, *shape):
        return torch.empty(shape, device=device, dtype=dtype)
    f32, i32 = torch.float32, torch.int32
    return Score(e(torch.int64, ns, p, v), e(i32, ns, p, v), e(f32, ns, p, v), e(f32, ns, p, v), e(f32, ns, p, v),
                 e(f32, ns, p, v) if samples else None, e(i32, ns, v), e(f32, ns, v) if samples else None,
                 e(f32, ns, v) if samples else None, e(f32, ns, v), e(f32, ns, v))


def _dev_ptr(x):
    return x if x is None or isinstance(x, ctypes.c_void_p) else ptr(x)


def score_push(state, thr, mean, v_pred, samples, ids, num_peds, det_id, det_xy, m_max, scale, det_count=None,
               det_start=None, pushed=None, id_stride=1, xy_stride=2, m_total=None, out=None):
    """Score the pending predictions of every stream against one push of detections, then enqueue this push's
    prediction (`stg_score_push` / `stg_score_push_streams`; the rule: DESIGN.md 5.17).  state: a ScoreState; thr: (Q,)
    float32 device tensor of d2 thresholds (score_thresholds) or None; the prediction as the chain leaves it: mean
    (NS,P,V,2), v_pred (NS,5,P,V) (any strides), samples (K,NS,P,V,2) or None, ids (NS,V) int64, num_peds (NS,) int32;
    scale = 10^decimals of the push's rounding (0: none).  The detections are device memory, tensors or raw pointers:
    with det_count ((1,) int32) one stream's det_id (m_max,), det_xy (m_max,2) as stg_track_push reads them; with
    det_start (NS+1,) and pushed (NS,) int32 the packed tick of stg_track_push_streams (id_stride, xy_stride, m_total).
    out: an earlier Score to fill (graph capture).  No host synchronisation.  Returns a Score."""
    require_gpu(mean, v_pred, samples, ids, num_peds, *[x for x in state if x is not None])
    ns, p, v, k = _score_prediction("score_push", state, mean, v_pred, samples, ids, num_peds)
    q = state.totals.shape[2] - 5
    _score_state_fits("score_push", _SCORE_SAMPLED, state, _score_shapes(ns, p, v, k, q), k, thr, q)
    _score_limits("score_push", V=v, K=k, P=p, Q=q)
    out = _score_out_fits("score_push", out, lambda dev: score_buffers(ns, p, v, dev, k > 0), mean.device)
    pred = _score_tail((_lib.ScoreState, _lib.ScoreOut), _SCORE_SAMPLED, state, out, thr, mean, v_pred, samples, ids,
                       num_peds, p, v, k, q)
    det = dict(det_id=_dev_ptr(det_id), det_xy=_dev_ptr(det_xy), M_max=int(m_max), scale=scale)
    if (det_count is None) == (det_start is None):
        raise ValueError("score_push: pass det_count (one stream) or det_start and pushed (a packed tick)")
    if det_count is not None:
        if ns != 1:
            raise ValueError("score_push: det_count serves one stream, the prediction holds %d" % ns)
        call("stg_score_push", **det, det_count=_dev_ptr(det_count), **pred)
    else:
        if pushed is None or m_total is None:
            raise ValueError("score_push: det_start needs pushed and m_total")
        call("stg_score_push_streams", **det, id_stride=int(id_stride), xy_stride=int(xy_stride), M_total=int(m_total),
             det_start=_dev_ptr(det_start), pushed=_dev_ptr(pushed), NS=ns, **pred)
    return out


ScoreTimedState = collections.namedtuple(
    "ScoreTimedState", "rec_t rec_status rec_peds rec_ids rec_mean rec_cov rec_samples acc acc_mean steps matched err d2 "
                       "nll best traj_steps traj_ade traj_fde traj_ade_mean traj_fde_mean counters totals traj_totals")
ScoreTimedState.__doc__ = """The device state of `score_timed_push` (stg_score_timed_state), NS leading: the ring of Rp
records per stream, indexed by time (DESIGN.md 5.25) -- rec_t (NS,Rp) int64 the time of the push that made the record,
rec_status (NS,Rp) int32 {0 empty, 1 pending, 2 retired}, rec_peds (NS,Rp) int32, rec_ids (NS,Rp,V) int64, rec_mean
(NS,Rp,P,V,2), rec_cov (NS,Rp,P,V,3), rec_samples (NS,Rp,K,P,V,2), the accumulators acc (NS,Rp,K,V), acc_mean (NS,Rp,V)
float32 and steps (NS,Rp,V) int32 --, the record's own tables matched int32, err, d2, nll, best float32 (NS,Rp,P,V)
(row h-1: the record scored at t_r + h * step), the retired rows traj_steps int32, traj_ade, traj_fde, traj_ade_mean,
traj_fde_mean float32 (NS,Rp,V), counters (NS,2) int64 {accepted pushes, evictions} and the running totals: totals
(NS,P,5+Q), traj_totals (NS,5) float64 with ScoreState's columns.  Columns v >= rec_peds of a row are not part of the
contract.  rec_samples, acc, best, traj_ade and traj_fde are None when samples are not scored."""
ScoreTimed = collections.namedtuple("ScoreTimed", "push_totals push_traj")
ScoreTimed.__doc__ = """What one timed push added to the running totals (`stg_score_push_timed`), NS leading: push_totals
(NS,P,5+Q) and push_traj (NS,5) float64, all zero for a stream not pushed or refused."""
_SCORE_TIMED_SAMPLED = ("rec_samples", "acc", "best", "traj_ade", "traj_fde")


def _score_timed_shapes(ns, p, v, k, q, rp):
    rpv = (ns, rp, p, v)
    return dict(rec_t=(ns, rp), rec_status=(ns, rp), rec_peds=(ns, rp), rec_ids=(ns, rp, v), rec_mean=rpv + (2,),
                rec_cov=rpv + (3,), rec_samples=(ns, rp, k, p, v, 2), acc=(ns, rp, k, v), acc_mean=(ns, rp, v),
                steps=(ns, rp, v), matched=rpv, err=rpv, d2=rpv, nll=rpv, best=rpv, traj_steps=(ns, rp, v),
                traj_ade=(ns, rp, v), traj_fde=(ns, rp, v), traj_ade_mean=(ns, rp, v), traj_fde_mean=(ns, rp, v),
                counters=(ns, 2), totals=(ns, p, 5 + q), traj_totals=(ns, 5))


def score_timed_state(ns, p, v, k, pending, device, samples=True, q=3):
    """A cleared ScoreTimedState for ns streams, horizons p, scenes padded to v pedestrians, k samples, `pending` record
    rows and q coverage thresholds.  samples=False (or k = 0): the samples are not kept, nothing sample-based is scored.
    Size per stream: pending*V*(28 + 36P) bytes, and pending*V*(8KP + 4K + 4P + 8) more with samples -- at pending 128,
    V 128, K 20, P 12 about 7.5 MB without and 41 MB with the samples (31.5 MB of it the samples themselves), so 64
    streams hold 2.6 GB; the totals add 8P(5+q) + 40 bytes."""
    ns, p, v, k, q, rp = int(ns), int(p), int(v), int(k) if samples else 0, int(q), int(pending)
    _score_limits("score_timed_state", V=v, k=k, P=p, q=q, pending=rp)
    if ns < 1 or p < 1 or v < 1 or k < 0 or q < 0 or rp < 1:
        raise ValueError("score_timed_state: bad sizes ns=%d p=%d v=%d k=%d q=%d pending=%d" % (ns, p, v, k, q, rp))
    return _score_cleared(ScoreTimedState, _SCORE_TIMED_SAMPLED, _score_timed_shapes(ns, p, v, k, q, rp), k, device)


score_timed_reset = score_reset


def score_timed_buffers(ns, p, q, device):
    """An empty ScoreTimed for ns streams (graph capture: the outputs `score_timed_push(out=...)` fills)."""
    return ScoreTimed(torch.empty((ns, p, 5 + q), device=device, dtype=torch.float64),
                      torch.empty((ns, 5), device=device, dtype=torch.float64))


def score_timed_push(state, thr, mean, v_pred, samples, ids, num_peds, tracks, step, max_dt, scale, pushed=None,
                     out=None):
    """Score the pending timed predictions of every stream against the track samples of the timed push that has just
    run, retire those whose last instant has arrived, then enqueue this push's prediction (`stg_score_push_timed` /
    `stg_score_push_streams_timed`; the rule: DESIGN.md 5.25).  state: a ScoreTimedState; thr: (Q,) float32 device tensor
    of d2 thresholds or None; the prediction as the chain leaves it, as `score_push` takes it; tracks: the timed push's
    state (slot_id (NS,S), t_ring (NS,S,R), xy_ring (NS,S,R,2), slot_head (NS,S,2), clock (NS,2), head_flags (NS,2)),
    read only; step, max_dt and scale as that push was given them.  pushed: (NS,) int32 device tensor (the packed tick's)
    -- None: one stream, always pushed.  out: an earlier ScoreTimed to fill (graph capture).  No host synchronisation.
    Returns a ScoreTimed."""
    require_gpu(mean, v_pred, samples, ids, num_peds, *tracks, *[x for x in state if x is not None])
    ns, p, v, k = _score_prediction("score_timed_push", state, mean, v_pred, samples, ids, num_peds)
    slot_id, t_ring, xy_ring, slot_head, clock, head_flags = tracks
    if t_ring.dim() < 2 or slot_id.numel() % ns:
        raise ValueError("score_timed_push: tracks do not fit %d streams" % ns)
    s, r = slot_id.numel() // ns, t_ring.shape[-1]
    track_want = ((slot_id, ns * s, torch.int64), (t_ring, ns * s * r, torch.int64), (xy_ring, ns * s * r * 2, torch.float64),
                  (slot_head, ns * s * 2, torch.int32), (clock, ns * 2, torch.int64), (head_flags, ns * 2, torch.int32))
    for x, n, dt in track_want:
        if x.numel() != n or x.dtype != dt or not x.is_contiguous():
            raise ValueError("score_timed_push: the track state does not fit this call (S=%d, R=%d)" % (s, r))
    q, rp = state.totals.shape[2] - 5, state.rec_t.shape[1]
    _score_state_fits("score_timed_push", _SCORE_TIMED_SAMPLED, state, _score_timed_shapes(ns, p, v, k, q, rp), k, thr, q)
    _score_limits("score_timed_push", V=v, K=k, P=p, Q=q, pending=rp)
    out = _score_out_fits("score_timed_push", out, lambda dev: score_timed_buffers(ns, p, q, dev), mean.device)
    read = dict(slot_id=ptr(slot_id), t_ring=ptr(t_ring), xy_ring=ptr(xy_ring), slot_head=ptr(slot_head), clock=ptr(clock),
                head_flags=ptr(head_flags), S=s, R=r, scale=scale, step=int(step), max_dt=int(max_dt), Rp=rp)
    pred = _score_tail((_lib.ScoreTimedState, _lib.ScoreTimedOut), _SCORE_TIMED_SAMPLED, state, out, thr, mean, v_pred,
                       samples, ids, num_peds, p, v, k, q)
    if pushed is None:
        if ns != 1:
            raise ValueError("score_timed_push: %d streams need `pushed`" % ns)
        call("stg_score_push_timed", **read, **pred)
    else:
        if pushed.numel() != ns or pushed.dtype != torch.int32 or not pushed.is_cuda:
            raise ValueError("score_timed_push: pushed must be an int32 (NS,) device tensor")
        call("stg_score_push_streams_timed", **read, pushed=ptr(pushed), NS=ns, **pred)
    return out


def scene_order(num_peds, v):
    """Scene indices sorted by pedestrian count (clamped to [0, v]) descending, stable: the schedule the fused
    kernels use for ragged batches (`stg_scene_order`).  num_peds: int32 device tensor (N,).
    Returns (order (N,), key_start (v+2,)): scenes with at most x pedestrians are order[key_start[v-x]:]."""
    require_gpu(num_peds)
    n = num_peds.numel()
    peds = peds_arg(num_peds, n, num_peds.device)
    order = torch.empty(n, device=peds.device, dtype=torch.int32)
    key_start = torch.empty(int(v) + 2, device=peds.device, dtype=torch.int32)
    if n < 2:
        order.zero_()
        key_start.fill_(n)
        if n == 1:
            key_start[: int(v) - max(0, min(int(v), int(peds[0]))) + 1] = 0
        return order, key_start
    call("stg_scene_order", num_peds=ptr(peds), N=n, V=int(v), order=ptr(order), key_start=ptr(key_start))
    return order, key_start
