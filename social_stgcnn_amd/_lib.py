"""ctypes binding of libstgcnn_hip.so (C ABI: include/stgcnn_hip.h).

Plumbing only: torch supplies device memory (`tensor.data_ptr()`) and the current HIP stream;
every compute call goes to a hand-written HIP kernel.  There is no CPU / eager fallback: if the
library is missing or a tensor is not on a GPU, the call raises.
"""
import collections
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")     # where csrc/Makefile finds the headers: ../../include
# STG_USE_DIAG_LIB=1 (tools/ only) loads the diagnostic build `make -C csrc DIAG=1` produces; the product
# library reads no environment variable itself
DIAG = os.environ.get("STG_USE_DIAG_LIB", "0") not in ("", "0")
LIB_PATH = os.path.join(CSRC, "libstgcnn_hip_diag.so" if DIAG else "libstgcnn_hip.so")
ABI_VERSION = 8
OPT_WG_PATH, OPT_SPLIT_BF16, OPT_WAVE_PATH, OPT_BF16_STORE, OPT_F32_MFMA, OPT_SEPARATE_FB = 1, 2, 4, 8, 16, 32
OPT_GENERIC_WGRAD = 64
EUNSUPPORTED = -2            # STG_EUNSUPPORTED

class ModelDesc(ctypes.Structure):
    """stg_model_desc (include/stgcnn_hip.h)."""
    _fields_ = [("n_stgcnn", ctypes.c_int32), ("n_txpcnn", ctypes.c_int32), ("c_in", ctypes.c_int32),
                ("c_out", ctypes.c_int32), ("t_obs", ctypes.c_int32), ("t_pred", ctypes.c_int32),
                ("kt", ctypes.c_int32), ("residual0", ctypes.c_int32), ("use_mdn", ctypes.c_int32),
                ("bn_mode", ctypes.c_int32), ("bn_eps", ctypes.c_float), ("bn_momentum", ctypes.c_float),
                ("flags", ctypes.c_int32), ("wg_waves", ctypes.c_int32)]


class ScoreState(ctypes.Structure):
    """stg_score_state (include/stgcnn_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("rec_ids", "rec_peds", "rec_mean", "rec_cov", "rec_samples", "acc",
                                               "acc_mean", "steps", "head", "totals", "traj_totals")]


class ScoreOut(ctypes.Structure):
    """stg_score_out (include/stgcnn_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("rec_ids", "matched", "err", "d2", "nll", "best", "traj_steps",
                                               "traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")]


class ScoreTimedState(ctypes.Structure):
    """stg_score_timed_state (include/stgcnn_hip_score_time.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("rec_t", "rec_status", "rec_peds", "rec_ids", "rec_mean", "rec_cov",
                                               "rec_samples", "acc", "acc_mean", "steps", "matched", "err", "d2", "nll",
                                               "best", "traj_steps", "traj_ade", "traj_fde", "traj_ade_mean",
                                               "traj_fde_mean", "counters", "totals", "traj_totals")]


class ScoreTimedOut(ctypes.Structure):
    """stg_score_timed_out (include/stgcnn_hip_score_time.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("push_totals", "push_traj")]


class StepTail(ctypes.Structure):
    """stg_step_tail (include/stgcnn_hip.h)."""
    _fields_ = [("params", ctypes.c_void_p), ("lr_dev", ctypes.c_void_p), ("lr", ctypes.c_float),
                ("stats", ctypes.c_void_p), ("buffers", ctypes.c_void_p), ("nbt", ctypes.POINTER(ctypes.c_void_p)),
                ("n_bn", ctypes.c_int), ("total", ctypes.c_void_p)]


Prototype = collections.namedtuple("Prototype", "name ret params")
Prototype.__doc__ = """One entry point as a header declares it: its name, the C type it returns and its parameters in
order, ((parameter name, C type), ...)."""
_Entry = collections.namedtuple("_Entry", "fn names nameset status")


class HeaderError(RuntimeError):
    """A prototype the binding cannot be derived from; the message names it."""


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double}
# the structs Python fills field by field travel typed; every other pointer (device memory, and the structs handed over
# with ctypes.byref / addressof: stg_step_tail, stg_score_timed_state, stg_score_timed_out) is a void *
_STRUCTS = {"stg_model_desc": ctypes.POINTER(ModelDesc), "stg_score_state": ctypes.POINTER(ScoreState),
            "stg_score_out": ctypes.POINTER(ScoreOut)}
_QUALIFIERS = ("const", "struct")


def _words(decl):
    """A declaration -> (its words without qualifiers, the number of `*`)."""
    words = decl.replace("*", " * ").split()
    return [w for w in words if w != "*" and w not in _QUALIFIERS], words.count("*")


def parse_header(text):
    """The prototypes of the entry points (stg_*) that the text of a C header declares, in its order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    protos = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(stg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        pairs = []
        for decl in ([] if params.strip() == "void" else params.split(",")):
            words, _ = _words(decl)
            if len(words) != 2:
                raise HeaderError("%s: parameter %d, `%s`, is not `<type> <name>`" % (name, len(pairs), decl.strip()))
            pname = words[1]
            if any(pname == n for n, _ in pairs):
                raise HeaderError("%s: two parameters are called `%s`" % (name, pname))
            pairs.append((pname, " ".join(decl.replace("*", " * ").split()[:-1])))
        protos.append(Prototype(name, " ".join(ret.split()), tuple(pairs)))
    return protos


def ctype_of(ctype, where):
    """The ctypes type an argument or a result of the C type `ctype` is bound with; `where` names it in the refusal."""
    words, stars = _words(ctype)
    base = words[0] if len(words) == 1 else None
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in _STRUCTS:
        return _STRUCTS[base]
    if stars == 1 and base == "char":
        return ctypes.c_char_p
    if stars == 2 and base is not None and base not in _STRUCTS:      # a host array of device pointers
        return ctypes.POINTER(ctypes.c_void_p)
    if stars == 1 and base is not None:
        return ctypes.c_void_p
    raise HeaderError("%s: no ctypes type for `%s`" % (where, ctype))


def collect(texts):
    """{name: Prototype} over the texts of several headers; a name declared twice is refused."""
    protos = {}
    for text in texts:
        for p in parse_header(text):
            if p.name in protos:
                raise HeaderError("%s is declared twice" % p.name)
            protos[p.name] = p
    return protos


def bind(handle, protos):
    """Set restype / argtypes of every prototype on the loaded library `handle`; -> {name: _Entry}, what call() needs.
    An `int` result is a status (check() raises on it) but for the version query."""
    entries = {}
    for p in protos.values():
        res = ctype_of(p.ret, p.name)
        args = [ctype_of(c, "%s(%s)" % (p.name, n)) for n, c in p.params]
        fn = getattr(handle, p.name, None)
        if fn is None:
            raise HeaderError("%s is declared in the headers but not exported by %s" % (p.name, handle._name))
        fn.restype, fn.argtypes = res, args
        names = tuple(n for n, _ in p.params)
        entries[p.name] = _Entry(fn, names, frozenset(names), res is ctypes.c_int and p.name != "stg_abi_version")
    return entries


def header_texts():
    """The text of include/stgcnn_hip.h and of the part headers it #includes, in that order."""
    main = open(os.path.join(INCLUDE, "stgcnn_hip.h")).read()
    parts = re.findall(r'^\s*#\s*include\s+"([^"]+)"', main, flags=re.M)
    return [main] + [open(os.path.join(INCLUDE, f)).read() for f in parts]


# THE binding: the headers are its only copy.  EXPORTS: the names the main header declares.
_texts = header_texts()
PROTOTYPES = collect(_texts)
EXPORTS = tuple(p.name for p in parse_header(_texts[0]))

_lib = None
_entries = None


def build(verbose=False):
    """Compile libstgcnn_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"] + (["DIAG=1"] if DIAG else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libstgcnn_hip.so failed (exit %d)" % res.returncode)
    return LIB_PATH


def lib():
    """The loaded library (raises if it has not been built: there is no fallback path)."""
    global _lib, _entries
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "social_stgcnn_amd: %s is missing -- build it with `make -C %s` (hipcc, "
                "--offload-arch=gfx950) or `python -c 'import __graft_entry__ as g; g.build()'`. "
                "There is no CPU or eager-PyTorch fallback for this path." % (LIB_PATH, CSRC))
        h = ctypes.CDLL(LIB_PATH)
        entries = bind(h, PROTOTYPES)
        if h.stg_abi_version() != ABI_VERSION:
            raise RuntimeError("libstgcnn_hip.so ABI %d != binding ABI %d" % (h.stg_abi_version(), ABI_VERSION))
        _lib, _entries = h, entries
    return _lib


def _entry(name):
    lib()
    return _entries[name]


def _refuse(name, names, given):
    given = list(given)
    kinds = (("missing", [n for n in names if n not in given]), ("unknown", [n for n in given if n not in names]),
             ("repeated", sorted({n for n in given if given.count(n) > 1})))
    raise TypeError("%s: %s" % (name, "; ".join("%s: %s" % (what, ", ".join(ns)) for what, ns in kinds if ns)))


def call(name, **kw):
    """Call the entry point `name` with its arguments by the names its prototype gives them: exactly those, in any
    order (a missing or an unknown one is a TypeError, and the library is not entered).  `stream` alone has a default,
    the current torch stream.  A status is checked (RuntimeError with stg_last_error()); a size query returns its value."""
    fn, names, nameset, status = _entry(name)
    current = "stream" in nameset and "stream" not in kw
    if current:
        kw["stream"] = None
    if kw.keys() != nameset:
        _refuse(name, names, kw)
    if current:
        kw["stream"] = stream_ptr()
    res = fn(*[kw[n] for n in names])
    if status:
        check(res, name)
    return res


class Bound:
    """An entry point with the arguments that never change fixed and put in order once, for a caller that launches it
    over and over: Bound(name, varying, **fixed), then bound(**varying).  `fixed` and the names `varying` must together
    be exactly the prototype's parameters (`stream` apart, as in call()); that is checked here, when it is built, so a
    launch orders its few varying arguments and does nothing else."""

    def __init__(self, name, varying, **fixed):
        self.fn, names, _, self.status = _entry(name)
        self.name, varying = name, tuple(varying)
        given = tuple(fixed) + varying
        self.stream = names.index("stream") if "stream" in names and "stream" not in given else None
        if sorted(given + ("stream",) * (self.stream is not None)) != sorted(names):
            _refuse(name, [n for n in names if n != "stream" or self.stream is None], given)
        self.args = [fixed.get(n) for n in names]
        self.slots, self.varying = tuple((names.index(n), n) for n in varying), frozenset(varying)

    def __call__(self, **kw):
        args = list(self.args)
        if kw.keys() != self.varying:
            _refuse(self.name, [n for _, n in self.slots], kw)
        for i, n in self.slots:
            args[i] = kw[n]
        if self.stream is not None:
            args[self.stream] = stream_ptr()
        res = self.fn(*args)
        if self.status:
            check(res, self.name)
        return res


class HipEvents:
    """hipEvent_t handles for the per-kernel device timing the fused entry points offer (`events` argument of
    stg_model_fwd / stg_model_bwd): created through the HIP runtime torch already loaded, recorded by the library on
    the launch stream, read back here."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            h = ctypes.CDLL("libamdhip64.so")
            h.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
            h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
            h.hipEventSynchronize.argtypes = [ctypes.c_void_p]
            h.hipEventDestroy.argtypes = [ctypes.c_void_p]
            cls._hip = h
        return cls._hip

    def __init__(self, n):
        self.n = n
        self.arr = (ctypes.c_void_p * n)()
        for i in range(n):
            ev = ctypes.c_void_p()
            if self.hip().hipEventCreate(ctypes.byref(ev)) != 0:
                raise RuntimeError("hipEventCreate failed")
            self.arr[i] = ev

    def intervals_ms(self):
        """[t(events[k]) - t(events[k-1]) for k = 1..n-1] after the stream has drained."""
        out = []
        self.hip().hipEventSynchronize(self.arr[self.n - 1])
        for k in range(1, self.n):
            ms = ctypes.c_float()
            if self.hip().hipEventElapsedTime(ctypes.byref(ms), self.arr[k - 1], self.arr[k]) != 0:
                raise RuntimeError("hipEventElapsedTime failed")
            out.append(ms.value)
        return out

    def __del__(self):
        try:
            for i in range(self.n):
                self.hip().hipEventDestroy(self.arr[i])
        except Exception:
            pass


class StatusError(RuntimeError):
    """An entry point returned a status other than 0: `.status` holds it."""

    def __init__(self, what, status, msg):
        super().__init__("%s failed (status %d): %s" % (what, status, msg))
        self.status = status


def check(rc, what):
    if rc != 0:
        raise StatusError(what, rc, lib().stg_last_error().decode("utf-8", "replace"))


def stream_ptr():
    """The current torch HIP stream as a void* (kernels are enqueued on it)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("social_stgcnn_amd runs on MI355X only: got a %s tensor (no CPU fallback)"
                               % t.device.type)


def seed_u64(seed):
    """A Python integer seed as the uint64 the C ABI takes (its low 64 bits)."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def seed_i64(seed):
    """The same 64 bits as the int64 a `seed_dev` device tensor holds."""
    s = seed_u64(seed)
    return s - (1 << 64) if s >= 1 << 63 else s


def as_f32(t, what):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (what, t.dtype))
    return t


def peds_arg(num_peds, n, device):
    """num_peds -> contiguous int32 device tensor of shape (N,) or None."""
    if num_peds is None:
        return None
    if not torch.is_tensor(num_peds):
        num_peds = torch.as_tensor(num_peds, dtype=torch.int32)
    num_peds = num_peds.to(device=device, dtype=torch.int32).contiguous()
    if num_peds.numel() != n:
        raise ValueError("num_peds has %d entries for a batch of %d scenes" % (num_peds.numel(), n))
    return num_peds
