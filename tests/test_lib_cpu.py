"""CPU: the C-ABI library builds, loads and exports every symbol include/stgcnn_hip.h declares;
argument validation that needs no GPU; host-side layout arithmetic."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_symbols_are_exported(L):
    from social_stgcnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "stgcnn_hip.h")).read()
    declared = set(re.findall(r"\b(stg_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert L.stg_abi_version() == _lib.ABI_VERSION


def _headers():
    """(text of include/stgcnn_hip.h, {part header: text} for the part headers it includes, in its order)"""
    inc = os.path.join(ROOT, "include")
    main = open(os.path.join(inc, "stgcnn_hip.h")).read()
    parts = re.findall(r'^#include "(stgcnn_hip_\w+\.h)"$', main, re.M)
    assert sorted(os.listdir(inc)) == sorted(["stgcnn_hip.h"] + parts) and len(parts) == 7
    return main, {f: open(os.path.join(inc, f)).read() for f in parts}


def test_every_prototype_of_the_headers_is_bound(L):
    """The eight headers are the only copy of the C ABI: _lib derives restype / argtypes and the parameter names from
    them.  51 prototypes in include/stgcnn_hip.h and 65 with its seven part headers, every one bound with as many
    argtypes as it has parameters and exported by the library; ABI version 8."""
    from social_stgcnn_amd import _lib
    main, parts = _headers()
    in_main = _lib.parse_header(main)
    assert len(in_main) == 51 and [p.name for p in in_main] == list(_lib.EXPORTS), \
        "%d prototypes parsed, 51 pinned: a new entry point changes this count on purpose" % len(in_main)
    protos = in_main + [p for text in parts.values() for p in _lib.parse_header(text)]
    assert len(protos) == 65 and len({p.name for p in protos}) == 65, \
        "%d prototypes parsed, 65 pinned: a new entry point changes this count on purpose" % len(protos)
    assert {p.name: p for p in protos} == _lib.PROTOTYPES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for p in protos:
        assert hasattr(raw, p.name), p.name
        fn = getattr(L, p.name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(p.params), p.name
        assert list(fn.argtypes) == [_lib.ctype_of(c, p.name) for _, c in p.params], p.name
        assert fn.restype == _lib.ctype_of(p.ret, p.name), p.name
        assert len({n for n, _ in p.params}) == len(p.params), p.name
    assert L.stg_abi_version() == _lib.ABI_VERSION == 8


SYNTHETIC = """
/* a comment that holds a prototype:  int stg_in_a_comment(int n);  */
#ifndef X_H
#define STG_SOME_LIMIT 4            /* int stg_behind_a_define(int n); */
typedef struct stg_model_desc { int32_t n_stgcnn; } stg_model_desc;
int stg_every_kind(const stg_model_desc *d, int n, int32_t n32, int64_t n64, uint64_t seed,   // int stg_in_a_line(int n);
                   float lr, double scale, const float *x, void *y, const int64_t *const *rows, void **events,
                   const stg_score_state *state, const stg_score_out *out, const stg_step_tail *tail,
                   const struct stg_score_timed_state *timed, stg_score_timed_out *timed_out, const char *text,
                   void *stream);
int64_t stg_a_size(void);
const char *stg_a_text(void);
#endif
"""


def test_parser_and_type_map_on_a_synthetic_header():
    """One parameter of every kind the C ABI has -- each scalar, `const T *`, `T *const *`, each struct pointer, `char *`,
    `void` -- against ctypes written out here; comments and preprocessor lines hold no prototype."""
    from social_stgcnn_amd import _lib
    void_p, c = ctypes.c_void_p, ctypes
    protos = _lib.parse_header(SYNTHETIC)
    assert [(p.name, p.ret) for p in protos] == [("stg_every_kind", "int"), ("stg_a_size", "int64_t"),
                                                 ("stg_a_text", "const char *")]
    assert protos[1].params == () and protos[2].params == ()
    want = [("d", c.POINTER(_lib.ModelDesc)), ("n", c.c_int), ("n32", c.c_int), ("n64", c.c_int64), ("seed", c.c_uint64),
            ("lr", c.c_float), ("scale", c.c_double), ("x", void_p), ("y", void_p), ("rows", c.POINTER(void_p)),
            ("events", c.POINTER(void_p)), ("state", c.POINTER(_lib.ScoreState)), ("out", c.POINTER(_lib.ScoreOut)),
            ("tail", void_p), ("timed", void_p), ("timed_out", void_p), ("text", c.c_char_p), ("stream", void_p)]
    assert [n for n, _ in protos[0].params] == [n for n, _ in want]
    assert [_lib.ctype_of(t, "stg_every_kind") for _, t in protos[0].params] == [t for _, t in want]
    assert protos[0].params[0][1] == "const stg_model_desc *" and protos[0].params[9][1] == "const int64_t * const *"
    assert [_lib.ctype_of(p.ret, p.name) for p in protos] == [c.c_int, c.c_int64, c.c_char_p]


def test_the_load_refuses_what_it_cannot_bind():
    """Each refusal names the prototype: a type outside the map, a parameter without a name, a name twice, a declared
    symbol the library does not export, and a prototype declared in two headers."""
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    load = lambda *texts: _lib.bind(raw, _lib.collect(texts))       # noqa: E731
    for text in ("int stg_abi_version(unsigned n);", "int stg_abi_version(long n);", "long stg_abi_version(void);",
                 "int stg_abi_version(float **p, stg_model_desc **d);", "int stg_abi_version(stg_model_desc d);"):
        with pytest.raises(_lib.HeaderError, match=r"stg_abi_version.*no ctypes type"):
            load(text)
    with pytest.raises(_lib.HeaderError, match=r"stg_abi_version: parameter 1, `float \*`"):
        load("int stg_abi_version(int n, float *, void *stream);")
    with pytest.raises(_lib.HeaderError, match=r"stg_abi_version: two parameters are called `n`"):
        load("int stg_abi_version(int n, float *x, const float *n);")
    with pytest.raises(_lib.HeaderError, match=r"stg_not_in_the_library is declared in the headers but not exported"):
        load("int stg_abi_version(void);\nint stg_not_in_the_library(int n);")
    one, two = "int stg_abi_version(void);\nint stg_twice(int n);", "const char *stg_last_error(void);\nint stg_twice(int n);"
    with pytest.raises(_lib.HeaderError, match=r"stg_twice is declared twice"):
        load(one, two)
    assert sorted(load(one.split("\n")[0], two.split("\n")[0])) == ["stg_abi_version", "stg_last_error"]


def _ragged_size_rows():
    import json
    rows = json.load(open(os.path.join(ROOT, "tests", "size_queries.json")))["rows"]
    rows = [r for r in rows if r[1] != r[2]]
    assert {(7, 64), (100, 32)} <= {(r[1], r[2]) for r in rows}
    return rows


def test_calls_go_by_parameter_name(L):
    """_lib.call orders its keywords by the prototype: stg_model_ws_tail_floats with (V, N, d) in reversed order returns
    the recorded value wherever N != V, which a call that ignored the names would not.  A missing name, an unknown one
    and both together are a TypeError that names them, and the library is not entered: stg_last_error() stays."""
    from social_stgcnn_amd import _lib, ops
    distinct = 0
    for f, n, v, tail, _, _ in _ragged_size_rows():
        d = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
        d.flags = f
        assert _lib.call("stg_model_ws_tail_floats", V=v, N=n, d=ctypes.byref(d)) == tail, (f, n, v)
        distinct += L.stg_model_ws_tail_floats(ctypes.byref(d), v, n) != tail
    assert distinct > 100                                  # (the swapped call does give another value)
    assert L.stg_adj_build(None, 0, 0, 0, 0, None, 1, 4, 8, 1, None, None, None) == -1
    before = L.stg_last_error()
    assert b"null" in before
    r = ctypes.byref(d)
    for kw, said in ((dict(d=r, N=7), "missing: V"), (dict(d=r, N=7, V=64, n=7), "unknown: n"),
                     (dict(desc=r, N=7, V=64), "missing: d; unknown: desc"), (dict(), "missing: d, N, V")):
        with pytest.raises(TypeError, match="^stg_model_ws_tail_floats: %s$" % said):
            _lib.call("stg_model_ws_tail_floats", **kw)
        assert L.stg_last_error() == before
    with pytest.raises(TypeError, match="^stg_adj_build: missing: rel, .*, adj$"):      # (stream alone has a default)
        _lib.call("stg_adj_build")
    # a status is checked inside the call, a size query returns its value (a negative one included)
    with pytest.raises(_lib.StatusError, match="stg_selftest_mfma failed .status -1.") as e:
        _lib.call("stg_selftest_mfma", a=None, b=None, K=3, c=None, stream=None)
    assert e.value.status == -1
    bad = ops.make_desc(1, 5, 2, 5, 6, 12, 3, 2, False, False)
    assert _lib.call("stg_model_param_count", d=ctypes.byref(bad)) == -2


def test_a_prebound_call_is_complete_when_it_is_built(L):
    """_lib.Bound: the fixed arguments and the names of the varying ones must together be the prototype's parameters
    when it is built, not at the first launch; a launch names exactly the varying ones, in any order."""
    from social_stgcnn_amd import _lib, ops
    d = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
    name, r = "stg_model_ws_tail_floats", ctypes.byref(d)
    for varying, fixed, said in ((("N",), dict(d=r), "missing: V"), (("N", "V"), dict(), "missing: d"),
                                 (("N", "V"), dict(d=r, T=8), "unknown: T"), (("N", "V"), dict(d=r, V=64), "repeated: V"),
                                 (("N", "V", "stream"), dict(d=r), "unknown: stream")):
        with pytest.raises(TypeError, match="^%s: %s$" % (name, said)):
            _lib.Bound(name, varying, **fixed)
    with pytest.raises(TypeError, match="^stg_scene_order: missing: key_start$"):         # (stream: the default)
        _lib.Bound("stg_scene_order", ("order",), num_peds=None, N=2, V=3)
    bound = _lib.Bound(name, ("N", "V"), d=r)
    for f, n, v, tail, _, _ in _ragged_size_rows():
        if f == 0:
            assert bound(V=v, N=n) == tail, (n, v)
    before = L.stg_last_error()
    for kw, said in ((dict(N=7), "missing: V"), (dict(N=7, V=64, d=r), "unknown: d"), (dict(N=7, v=64), "missing: V; unknown: v")):
        with pytest.raises(TypeError, match="^%s: %s$" % (name, said)):
            bound(**kw)
    assert L.stg_last_error() == before


def test_layout_queries_match_reference_counts(L):
    from social_stgcnn_amd import ops
    d = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
    assert L.stg_model_param_count(ctypes.byref(d)) == 7563          # 7,563 parameters
    assert L.stg_model_buffer_count(ctypes.byref(d)) == 30           # 3 BatchNorm x (mean, var) x 5
    assert L.stg_model_stat_floats(ctypes.byref(d)) == 30
    assert L.stg_model_ws_floats(ctypes.byref(d), 32) == 64 + 32 * (16 + 8 + 40 + 40 + 40 + 4 * 60) + 5 * 12 * 240
    # batch tail of the workspace: the prepared bf16 A operands of the five input-gradient convs (24 x 64 lanes x 16 bytes
    # each) when the exact-bf16 backward serves the batch (V <= 128: one wave per scene up to 32 pedestrians, teams of two
    # or four waves beyond), nothing otherwise; behind them the scene order of a ragged batch (N indices, V + 2 tier
    # offsets, N sorted counts, rounded up to 4)
    order = lambda n, v: (2 * n + v + 2 + 3) & ~3
    assert L.stg_model_ws_tail_floats(ctypes.byref(d), 100, 32) == 5 * 24 * 64 * 4 + order(100, 32)
    assert L.stg_model_ws_tail_floats(ctypes.byref(d), 7, 64) == 5 * 24 * 64 * 4 + order(7, 64)
    assert L.stg_model_ws_tail_floats(ctypes.byref(d), 7, 128) == 5 * 24 * 64 * 4 + order(7, 128)
    assert L.stg_model_ws_tail_floats(ctypes.byref(d), 7, 129) == order(7, 129)
    d_f32 = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
    from social_stgcnn_amd import _lib as lib_mod
    d_f32.flags |= lib_mod.OPT_F32_MFMA
    assert L.stg_model_ws_tail_floats(ctypes.byref(d_f32), 0, 32) == order(0, 32)
    d2 = ops.make_desc(2, 3, 2, 5, 8, 12, 3, 2, False, False)
    # second block: identity residual -> no residual conv / BN parameters
    blk0 = 10 + 5 + 10 + 1 + 75 + 5 + 10 + 10 + 5 + 10 + 1
    blk1 = 25 + 5 + 10 + 1 + 75 + 5 + 10 + 1
    txp = (12 * 8 * 9 + 12) + 2 * (12 * 12 * 9 + 12) + (12 * 12 * 9 + 12) + 3
    assert L.stg_model_param_count(ctypes.byref(d2)) == blk0 + blk1 + txp
    d3 = ops.make_desc(1, 0, 5, 5, 8, 0, 3, 1, False, False)          # stand-alone st_gcn, identity residual
    assert L.stg_model_param_count(ctypes.byref(d3)) == blk1


def test_size_queries_match_the_recorded_table(L):
    """stg_model_ws_tail_floats / stg_model_fwd_scratch_floats / stg_model_bwd_scratch_floats (error codes included) over
    path flags x batch sizes x padded crowd sizes, against tests/size_queries.json: the answers of the library built
    from commit 28a5f63, the last one before the host-side step plan (csrc/step_plan.hpp).  Buffer sizes are ABI
    behaviour: callers allocate by them."""
    import json
    from social_stgcnn_amd import _lib, ops
    table = json.load(open(os.path.join(ROOT, "tests", "size_queries.json")))["rows"]
    flags = [0, _lib.OPT_WAVE_PATH, _lib.OPT_WG_PATH, _lib.OPT_F32_MFMA, _lib.OPT_SPLIT_BF16,
             _lib.OPT_BF16_STORE | _lib.OPT_WAVE_PATH]
    cases = [(f, n, v) for f in flags for n in (1, 7, 100, 287, 288, 2048) for v in (3, 32, 33, 40, 41, 64, 128, 129, 400)]
    assert [tuple(r[:3]) for r in table] == cases
    for f, n, v, tail, fwd, bwd in table:
        d = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
        d.flags = f
        got = (L.stg_model_ws_tail_floats(ctypes.byref(d), n, v), L.stg_model_fwd_scratch_floats(ctypes.byref(d), n, v),
               L.stg_model_bwd_scratch_floats(ctypes.byref(d), n, v))
        assert got == (tail, fwd, bwd), (f, n, v)
    assert sum(1 for r in table if r[5] == -3) == 36 and all(r[2] == 400 for r in table if r[5] == -3)


def test_invalid_arguments_return_status_not_abort(L):
    from social_stgcnn_amd import ops
    assert L.stg_adj_build(None, 0, 0, 0, 0, None, 1, 4, 8, 1, None, None, None) == -1
    assert b"null" in L.stg_last_error()
    bad = ops.make_desc(1, 5, 2, 5, 6, 12, 3, 2, False, False)       # seq_len the kernels are not built for
    assert L.stg_model_param_count(ctypes.byref(bad)) == -2
    assert b"seq_len" in L.stg_last_error()
    assert L.stg_selftest_mfma(None, None, 3, None, None) == -1
    d = ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True)
    assert L.stg_model_bwd_scratch_floats(ctypes.byref(d), 2048, 32) > 0
    assert L.stg_model_bwd_scratch_floats(ctypes.byref(d), 16, 400) == -3     # does not fit 160 KiB of LDS


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "social_stgcnn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("no CPU or eager", ""), os.path.join(dirpath, f)


def test_module_surface_matches_reference_state_dict():
    import numpy as np
    import torch
    from social_stgcnn_amd.model import ConvTemporalGraphical, social_stgcnn, st_gcn   # noqa: F401
    g = np.load(os.path.join(ROOT, "tests", "golden", "init_seed0.npz"))
    torch.manual_seed(0)
    m = social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)
    sd = m.state_dict()
    assert list(sd.keys()) == list(g.files)
    for k in g.files:                 # same constructor RNG order -> identical default initialisation
        assert np.array_equal(sd[k].numpy(), g[k]), k
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_eth.npz"))
    m.load_state_dict({k: torch.from_numpy(np.array(w[k])) for k in w.files})
    with pytest.raises(RuntimeError):          # a CPU tensor must fail loudly, not fall back
        m.eval()(torch.zeros(1, 2, 8, 3), torch.zeros(8, 3, 3))


def test_weight_gradient_kernel_keeps_its_loads_in_flight_and_tracked(tmp_path):
    """Compile-only ISA check of txp_wgrad_bf16: its staging loads are issued one item ahead.  They
    must be loads the COMPILER tracks (no global_load in inline assembly: a destination register with data in flight must
    never be visible to the register allocator as if it were ready), they must survive the per-scene barrier (no
    s_waitcnt vmcnt(0) between a staging load and the loop's s_barrier), and the kernel must not address memory through
    flat_*."""
    import subprocess
    src = os.path.join(ROOT, "social_stgcnn_amd", "csrc", "txp_wgrad_bf16.hip")
    text = open(src).read()
    assert not re.search(r'asm[^;]*global_load', text), "staging loads must not be inline assembly"
    out = str(tmp_path / "wgrad.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-S",
                           src, "-o", out])
    lines = open(out).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN3stg.*txp_wgrad_bf16_kernel.*:", l)]
    assert len(starts) == 4
    for st in starts:
        end = next(i for i in range(st, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
        body = [l.strip() for l in lines[st:end] if l.strip() and not l.strip().startswith((";", "."))]
        assert not any(l.startswith("flat_") for l in body)
        assert not any(l.startswith("scratch_") for l in body), "spilled registers in " + lines[st]
        loads = [i for i, l in enumerate(body) if l.startswith("global_load")]
        bars = [i for i, l in enumerate(body) if l.startswith("s_barrier")]
        assert loads and bars
        # a barrier with a staging load a few instructions in front of it and no full vmcnt drain in between: the load is
        # still in flight when the workgroup meets
        in_flight = [b for b in bars
                     if any(0 < b - ld <= 40 and not any("vmcnt(0)" in body[k] for k in range(ld, b)) for ld in loads)]
        assert in_flight, lines[st]


# ------------------------------------------------------------------------------------------
# every layout stg_model_desc accepts: host arithmetic and refusals (the GPU side is tests/test_gpu_layouts.py)
# ------------------------------------------------------------------------------------------
def _layout_desc(n_st, n_tx, c_in, training=True):
    from social_stgcnn_amd import ops
    return ops.make_desc(n_st, n_tx, c_in, 5, 8, 12 if n_tx else 0, 3, 1 if c_in == 5 else 2, False, training)


@pytest.mark.parametrize("c_in", (2, 5))
def test_param_and_buffer_counts_match_the_modules(L, c_in):
    """stg_model_param_count / stg_model_buffer_count for n_stgcnn 1..4 x n_txpcnn 0..8 == the sums of numel() over the
    module's named_parameters() / running statistics (n_txpcnn = 0: the st_gcn blocks alone, as the stand-alone module
    packs them)."""
    import layout_cases as LC
    for n_st in range(1, 5):
        for n_tx in range(0, 9):
            m = LC.make_model(n_st, max(n_tx, 1), c_in)
            mod = m if n_tx else m.st_gcns
            n_par = sum(p.numel() for _, p in mod.named_parameters())
            n_buf = sum(b.numel() for k, b in mod.named_buffers() if "running" in k)
            d = _layout_desc(n_st, n_tx, c_in)
            assert L.stg_model_param_count(ctypes.byref(d)) == n_par, (n_st, n_tx)
            assert L.stg_model_buffer_count(ctypes.byref(d)) == n_buf, (n_st, n_tx)
            if n_tx:
                params, bufs, nbt, _ = m._tensors()
                assert sum(p.numel() for p in params) == n_par and sum(b.numel() for b in bufs) == n_buf
                assert [id(p) for p in params] == [id(p) for _, p in m.named_parameters()]      # the kernels' order
                assert len(nbt) == sum(1 for k, _ in m.named_buffers() if "num_batches" in k)


@pytest.mark.parametrize("c_in", (2, 5))
def test_dead_parameters_are_the_ones_the_forward_never_touches(c_in):
    """social_stgcnn._tensors()'s dead set (gradients the kernels report as None) for n_stgcnn 1..4 x n_txpcnn 1..8 ==
    the parameters autograd never reaches through the oracle's forward (model.py:191 skips tpcnns / prelus from
    max(1, n_txpcnn - 1) on); n_txpcnn 1 and 2 have other dead sets than 5."""
    import torch
    import layout_cases as LC
    from oracle import stgcnn_oracle as O
    seen = {}
    for n_st in range(1, 5):
        for n_tx in range(1, 9):
            m = LC.randomise(LC.make_model(n_st, n_tx, c_in), 3)
            params, _, _, dead = m._tensors()
            name_of = {id(p): k for k, p in m.named_parameters()}
            dead_names = {name_of[id(params[i])] for i in dead}
            state = {k: v.detach().clone() for k, v in m.state_dict().items()}
            leaves = {k: state[k].requires_grad_(True) for k, _ in m.named_parameters()}
            g = torch.Generator().manual_seed(1)
            y = O.social_stgcnn_forward(state, torch.randn(1, c_in, 8, 3, generator=g), torch.randn(8, 3, 3, generator=g),
                                        True, n_stgcnn=n_st, n_txpcnn=n_tx)
            y.square().sum().backward()
            untouched = {k for k, p in leaves.items() if p.grad is None}
            assert dead_names == untouched, (n_st, n_tx, dead_names ^ untouched)
            seen[n_tx] = len(untouched)
    assert seen[1] == 0 and seen[2] == 3 and seen[5] == 3


def test_layouts_outside_the_kernels_are_refused_by_every_size_query(L):
    for n_st, n_tx, c_in in ((5, 5, 2), (1, 9, 2), (1, 5, 3)):
        d = _layout_desc(n_st, n_tx, c_in)
        r = ctypes.byref(d)
        got = (L.stg_model_param_count(r), L.stg_model_buffer_count(r), L.stg_model_ws_floats(r, 32),
               L.stg_model_ws_tail_floats(r, 64, 32), L.stg_model_stat_floats(r), L.stg_model_fwd_scratch_floats(r, 64, 32),
               L.stg_model_bwd_scratch_floats(r, 64, 32))
        assert got == (-2,) * 7, (n_st, n_tx, c_in, got)
        assert L.stg_last_error()


def test_layout_cases_fp32_oracle_inside_project_bars():
    """Every case of tests/test_gpu_layouts.py's training-step matrix and of its trainer tests: the float32 oracle sits
    inside the project bars of the float64 oracle (5e-5 on V_pred and the loss, 1e-4 on gradients, 2e-6 on running
    statistics) and no pre-activation of the float64 oracle lies within layout_cases.KINK_MARGIN of the PReLU kink, so no
    case leans on the widened bar for that reason (the seeds were chosen for it: layout_cases.SEED_SHIFT).  Every PReLU
    slope of every case is different, one negative, one above 1."""
    import torch
    import layout_cases as LC
    for case in LC.scene_path_cases() + LC.stacked_cases() + LC.trainer_cases():
        _, state, b = case.build()
        r64 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn)
        r32 = LC.oracle_model_step(state, b, case.n_stgcnn, case.n_txpcnn, dtype=torch.float32)
        p, l, g, s = LC.oracle_distance(r32, r64)
        print("%-34s V_pred %.1e  loss %.1e  grad %.1e  stats %.1e  nearest pre-activation %.1e"
              % (case.id, p, l, g, s, r64.kink[0]))
        assert r64.kink[0] >= LC.KINK_MARGIN, (case, r64.kink[0])
        assert p < LC.BAR_PRED and l < LC.BAR_PRED and g < LC.BAR_GRAD and s < LC.BAR_STAT, (case, p, l, g, s)
        slopes = [float(v) for k, v in state.items() if k.endswith(("prelu.weight", "tcn.1.weight")) or "prelus" in k]
        assert len(set(slopes)) == len(slopes) and min(slopes) < 0 and max(slopes) > 1
