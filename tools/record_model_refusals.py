"""Records tests/model_refusals.json: status and stg_last_error text of every refusal that stg_model_fwd,
stg_model_bwd, stg_model_bwd_nll, stg_model_bwd_step and stg_model_step answer ahead of their first HIP runtime call.

    python tools/record_model_refusals.py [--lib path/to/libstgcnn_hip.so] [--out tests/model_refusals.json]

Run once on the library of the commit whose answers are to be pinned (the table in the repository: commit 7703007, the
last one before the call records of csrc/step_plan.hpp).  tests/test_model_args_cpu.py imports cases() and run_case()
from this file and replays the table on the library under test; it needs no GPU.

A case names an entry point and what differs from a well-formed call on the canonical training descriptor with N = 2
scenes padded to V = 32: descriptor fields, N, V, pointer arguments that are null or 4 bytes off a 16-byte boundary,
fields of the step tail.  Every pointer argument is a 16-byte slice of one small host buffer: no case dereferences
one, because every case is refused (or, for the empty forward, answered) before anything is launched.  The recorder
refuses to write a table with any other status in it: a case that went on to a launch would show a HIP error here and
would read host memory from a kernel on a machine with a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEAD = ["d", "params", "buffers", "x", "x_sn", "x_sc", "x_st", "x_sv", "adj", "a_sn", "num_peds", "N", "V"]
ARGS = {
    "stg_model_fwd": HEAD + ["y", "ws", "stats", "scratch", "events", "n_events", "stream"],
    "stg_model_bwd": HEAD + ["dy", "ws", "scratch", "grad_params", "dx", "events", "n_events", "stream"],
    "stg_model_bwd_nll": HEAD + ["y", "target", "weights", "losses", "ws", "scratch", "grad_params", "events", "n_events",
                                 "stream"],
    "stg_model_bwd_step": HEAD + ["y", "target", "weights", "losses", "ws", "scratch", "grad_params", "tail", "events",
                                  "n_events", "stream"],
    "stg_model_step": HEAD + ["y", "ws", "stats", "fwd_scratch", "target", "weights", "losses", "bwd_scratch",
                              "grad_params", "tail", "fwd_events", "n_fwd_events", "bwd_events", "n_bwd_events", "stream"],
}
BACKWARD = ("stg_model_bwd", "stg_model_bwd_nll", "stg_model_bwd_step")
NULL_BY_DEFAULT = ("num_peds", "weights", "dx", "events", "fwd_events", "bwd_events", "stream")
WG_PATH, SPLIT_BF16, WAVE_PATH, BF16_STORE = 1, 2, 4, 8          # STG_OPT_* (include/stgcnn_hip.h)
MAX_BLOCKS = 4                                                   # STG_MAX_BLOCKS
STATUSES = (-1, -2, -3)                                          # STG_EINVAL, STG_EUNSUPPORTED, STG_ELDS
# what stg_last_error holds when a case starts: left there by a refused size query, so that the refusals that leave the
# message alone have a known one to leave
SENTINEL = "stg_model_ws_floats: V=0"


def case(entry, what, **diff):
    return dict(id="%s: %s" % (entry[4:], what), entry=entry, **diff)


def cases():
    out = []
    for e in ARGS:
        out += [case(e, "seq_len = 6", desc={"t_obs": 6}), case(e, "N = -1", N=-1), case(e, "V = 0", V=0)]
    f = "stg_model_fwd"
    pointers = ("params", "buffers", "x", "adj", "num_peds", "y", "ws", "stats", "scratch", "events", "stream")
    out.append(case(f, "N = 0, every pointer null", N=0, args={a: "null" for a in pointers}))
    out += [case(f, "null " + a, args={a: "null"}) for a in ("params", "buffers", "x", "adj", "y", "scratch")]
    out += [case(f, a + " at +4 bytes", args={a: "+4"}) for a in ("scratch", "ws")]
    out.append(case(f, "BF16_STORE | WG_PATH", desc={"flags": BF16_STORE | WG_PATH}))
    for e in BACKWARD:
        out.append(case(e, "null grad_params", args={"grad_params": "null"}))
        out.append(case(e, "null dy", args={"dy" if e == "stg_model_bwd" else "y": "null"}))
        out += [case(e, a + " at +4 bytes", args={a: "+4"}) for a in ("ws", "scratch")]
        out.append(case(e, "V = 400", V=400))
        out.append(case(e, "BF16_STORE | WG_PATH", desc={"flags": BF16_STORE | WG_PATH}))
        out.append(case(e, "BF16_STORE | SPLIT_BF16 | WAVE_PATH", desc={"flags": BF16_STORE | SPLIT_BF16 | WAVE_PATH}))
    out.append(case("stg_model_bwd", "dx on the scene path", args={"dx": "buffer"}))
    n = "stg_model_bwd_nll"
    out.append(case(n, "SPLIT_BF16 (no message)", desc={"flags": SPLIT_BF16}))
    out.append(case(n, "n_txpcnn = 0 (no message)", desc={"n_txpcnn": 0, "t_pred": 0}))
    out += [case(n, "null " + a, args={a: "null"}) for a in ("target", "losses")]
    for e in ("stg_model_bwd_step", "stg_model_step"):
        out.append(case(e, "null tail", tail="null"))
        out.append(case(e, "tail.params null", tail={"params": "null"}))
        out.append(case(e, "tail.stats without tail.buffers", tail={"buffers": "null"}))
        out.append(case(e, "tail.n_bn = -1", tail={"n_bn": -1}))
        out.append(case(e, "tail.n_bn = 3 * STG_MAX_BLOCKS + 1", tail={"n_bn": 3 * MAX_BLOCKS + 1}))
        out.append(case(e, "N = 0 (no message)", N=0))
    s = "stg_model_step"
    out += [case(s, "null " + a, args={a: "null"}) for a in ("target", "losses", "y", "ws")]
    out.append(case(s, "a bad tail ahead of a bad descriptor", tail="null", desc={"t_obs": 6}))
    out.append(case(s, "SPLIT_BF16 (no message)", desc={"flags": SPLIT_BF16}))
    out += [case(s, "null " + a, args={a: "null"}) for a in ("grad_params", "bwd_scratch")]
    out.append(case(s, "null params: the forward's message", args={"params": "null"}))
    out.append(case(s, "fwd_scratch at +4 bytes: the forward's message", args={"fwd_scratch": "+4"}))
    # (bwd_scratch at +4 bytes is refused by the backward only after the forward has launched: not in the table)
    return out


def bind(path):
    """The five entry points, stg_model_ws_floats and stg_last_error of the library at `path`, typed as _lib types them."""
    from social_stgcnn_amd import _lib
    h = ctypes.CDLL(path)
    _lib.bind(h, {name: _lib.PROTOTYPES[name] for name in list(ARGS) + ["stg_model_ws_floats", "stg_last_error"]})
    return h


def run_case(h, c):
    """(status, stg_last_error text) of case `c` on the bound library `h`."""
    from social_stgcnn_amd import _lib
    N, V = c.get("N", 2), c.get("V", 32)
    fields = dict(n_stgcnn=1, n_txpcnn=5, c_in=2, c_out=5, t_obs=8, t_pred=12, kt=3, residual0=2, use_mdn=0, bn_mode=1,
                  bn_eps=1e-5, bn_momentum=0.1, flags=0, wg_waves=0)
    d = _lib.ModelDesc(**dict(fields, **c.get("desc", {})))
    names = ARGS[c["entry"]]
    raw = ctypes.create_string_buffer(16 * (len(names) + 8) + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    slot = lambda k: base + 16 * k                                   # a 16-byte aligned host address of its own
    tail = None
    if c.get("tail") != "null":
        t = dict(params=slot(len(names)), lr_dev=None, lr=0.01, stats=slot(len(names) + 1), buffers=slot(len(names) + 2),
                 nbt=None, n_bn=0, total=slot(len(names) + 3))
        t.update({k: None if v == "null" else v for k, v in c.get("tail", {}).items()})
        tail = _lib.StepTail(**t)
    sizes = dict(x_sn=2 * 8 * V, x_sc=8 * V, x_st=V, x_sv=1, a_sn=8 * V * V, N=N, V=V, n_events=0, n_fwd_events=0,
                 n_bwd_events=0)
    call = []
    for k, a in enumerate(names):
        how = c.get("args", {}).get(a, "null" if a in NULL_BY_DEFAULT else "buffer")
        if a == "d":
            call.append(ctypes.byref(d))
        elif a in sizes:
            call.append(sizes[a])
        elif a == "tail":
            call.append(ctypes.addressof(tail) if tail is not None else None)
        else:
            call.append({"null": None, "buffer": slot(k), "+4": slot(k) + 4}[how])
    canon = _lib.ModelDesc(**fields)
    assert h.stg_model_ws_floats(ctypes.byref(canon), 0) == -1 and h.stg_last_error().decode() == SENTINEL
    rc = getattr(h, c["entry"])(*call)
    return rc, h.stg_last_error().decode()


def main():
    from social_stgcnn_amd import _lib
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "model_refusals.json"))
    a = ap.parse_args()
    h = bind(a.lib)
    rows = []
    for c in cases():
        rc, msg = run_case(h, c)
        answered = rc == 0 and c["id"] == "model_fwd: N = 0, every pointer null"
        assert answered or rc in STATUSES, "%s: status %d (%s) is no refusal ahead of a launch" % (c["id"], rc, msg)
        rows.append(dict(c, status=rc, message=msg))
        print("%-64s %3d  %s" % (c["id"], rc, msg))
    with open(a.out, "w") as f:
        json.dump({"rows": rows}, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(rows), a.out))


if __name__ == "__main__":
    main()
