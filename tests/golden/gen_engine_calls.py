#!/usr/bin/env python3
"""Generate tests/golden/engine_calls.json: what every public Engine / MsmBases method hands to the C ABI and what it
returns, observed on a recording stand-in for the library (no GPU, nothing computed).  Per call: the symbol and each argument
as "ctx", "in<i>" / "out<i>" (the pointer of the i-th array passed / returned), "None", a plain value or a tagged ctypes
value; per result: type, dtype and shape.  tests/test_engine_calls.py replays `observe()` and compares with the file.

    python tests/golden/gen_engine_calls.py            # rewrites the file from the package in this tree
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "engine_calls.json")
N, T = 3, 2

# methods that need a GPU, a communicator or pinned memory to mean anything (msm_partial: only its out=None form, which
# allocates on the current CUDA device, is left out)
LEFT_OUT = {"comm_unique_id", "comm_init", "comm_destroy", "comm_size", "host_register", "host_unregister"}

U64, U8 = "u64", "u8"


def cases():
    """(method, kind of every array argument as (lead shape, width, dtype), keyword / by-value arguments)."""
    r = lambda w, dt=U64: ((N,), w, dt)
    r3 = lambda w, dt=U64: ((N, T), w, dt)
    c = []
    add = lambda name, arrays, **kw: c.append((name, arrays, kw))
    for pre in ("fe", "sc"):
        for op in ("add", "sub", "mul", "pow"):
            add("%s_%s" % (pre, op), [r(5), r(5)])
        for op in ("neg", "square", "half"):
            add("%s_%s" % (pre, op), [r(5)])
    add("fe_invert", [r(5)])
    add("fe_div", [r(5), r(5)])
    add("fe_legendre_symbol", [r(5)])
    add("fe_is_positive", [r(5)])
    add("fe_mod_sqrt", [r(5)], sign=1)
    add("fe_from_bytes", [r(32, U8)])
    add("fe_to_bytes", [r(5)])
    add("fe_sqrt_ratio_i", [r(5), r(5)])
    add("fe_inv_sqrt", [r(5)])
    add("sc_shr", [r(5)], shift=7)
    add("sc_into_bits", [r(5)])
    add("sc_compute_naf", [r(5)])
    add("sc_compute_naf", [r(5)], width=5)
    add("sc_from_bytes", [r(32, U8)])
    add("sc_to_bytes", [r(5)])
    for op in ("add", "sub"):
        add("ed_" + op, [r(20), r(20)])
        add("proj_" + op, [r(15), r(15)])
    for op in ("double", "neg"):
        add("ed_" + op, [r(20)])
        add("proj_" + op, [r(15)])
    add("ed_scalar_mul", [r(20), r(5)])
    add("ed_scalar_mul", [r(20), r(5)], flags=16)
    add("ed_scalar_mul", [r(20), r(5), r(20)], _names=("p", "k", "out"), flags=1)
    add("ed_lincomb", [r3(20), r3(5)])
    add("ed_mul_by_pow_2", [r(20)], kexp=9)
    add("ed_mul_by_cofactor", [r(20)])
    add("ed_to_affine", [r(20)])
    add("ed_eq", [r(20), r(20)])
    add("ed_compress", [r(20)])
    add("ed_decompress", [r(32, U8)])
    add("ris_compress", [r(20)])
    add("ris_decompress", [r(32, U8)])
    add("ris_eq", [r(20), r(20)])
    add("ris_roundtrip_mul", [r(32, U8), r(5)])
    add("ris_roundtrip_mul", [r(32, U8), r(5), r(32, U8)], _names=("b", "k", "out"))
    add("ris_lincomb", [r3(32, U8), r3(5)])
    add("ris_lincomb", [r3(32, U8), r3(5), r(5)])
    add("ed_is_valid", [r(20)])
    add("ris_is_valid", [r(20)])
    add("ris_elligator", [r(5)])
    add("ris_from_uniform_bytes", [r(64, U8)])
    add("proj_to_extended", [r(15)])
    add("proj_eq", [r(15), r(15)])
    add("proj_is_valid", [r(15)])
    add("proj_scalar_mul", [r(15), r(5)])
    add("ed_coset4", [r(20)])
    add("ed_mul_base", [r(5)])
    add("ed_mul_base_wnaf", [r(5)], width=4)
    add("ris_mul_base_compress", [r(5)])
    add("msm", [r(20), r(5)])
    add("msm_sharded", [r(20), r(5)])
    add("msm_batch", [r3(20), r3(5)])
    add("ed_fold_ordered", [r(20)])
    add("msm_partial", [r(20), r(5), ((1,), 20, U64)], _names=("points", "scalars", "out"), _torch_only=(2,))
    add("msm_bases", [r(20)])
    add("msm_bases", [r(20)], window_bits=8)
    add("MsmBases.msm", [r(5)])
    add("MsmBases.msm", [((T, N), 5, U64)])
    add("MsmBases.close", [])
    add("msm_plan", [], n=1000)
    add("msm_fixed_plan", [], n=1000, window_bits=8)
    add("msm_batch_plan", [], n=100, batch=4)
    add("synchronize", [])
    add("set_stream", [], stream_handle=0x5000)
    add("set_stream_dev", [], slot=0, stream_handle=0x6000)
    add("use_own_stream", [])
    add("close", [])
    return c


# methods that only take numbers (or nothing): no tensor form to replay
NO_ARRAYS = {"MsmBases.close", "msm_plan", "msm_fixed_plan", "msm_batch_plan", "synchronize", "set_stream", "set_stream_dev", "use_own_stream", "close"}


def _ptr(x):
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr() if hasattr(x, "data_ptr") else None


def _make(spec, kind, seed):
    lead, width, dt = spec
    dtype = np.uint64 if dt == U64 else np.uint8
    a = (np.arange(int(np.prod(lead)) * width, dtype=np.uint64) + seed).astype(dtype).reshape(tuple(lead) + (width,))
    if kind == "numpy":
        return a
    import torch
    if dtype == np.uint8:
        return torch.from_numpy(a)
    t = torch.from_numpy(a.view(np.int64))
    return t.to(torch.float64) if kind == "torch_f64" else t


class Recorder:
    """Stands in for the ctypes library: every zc_* call is recorded and answers ZC_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("zc_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "zc_msm_bases_create":
                args[-1]._obj.value = 77                    # the table id the library would hand out
            return 0
        return fn


def _describe_arg(a, ctx, ins, outs):
    if a is ctx:
        return "ctx"
    if a is None:
        return "None"
    if isinstance(a, bool) or isinstance(a, (int, np.integer)):
        for i, x in enumerate(ins):
            if _ptr(x) == a:
                return "in%d" % i
        for i, x in enumerate(outs):
            if _ptr(x) == a:
                return "out%d" % i
        return int(a)
    if isinstance(a, C.c_void_p):
        return ["c_void_p", a.value]
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, a.value]
    if isinstance(a, C.Array):
        return ["array", type(a)._type_.__name__, len(a)]
    if type(a).__name__ == "CArgObject":
        return ["byref", type(a._obj).__name__]
    raise TypeError("unexpected argument %r" % (a,))


def _describe_result(x):
    if isinstance(x, np.ndarray):
        return ["ndarray", str(x.dtype), list(x.shape)]
    if hasattr(x, "data_ptr"):
        return ["Tensor", str(x.dtype), list(x.shape)]
    if isinstance(x, dict):
        return ["dict", sorted(x)]
    return [type(x).__name__]


def public_methods(engine_module):
    names = set()
    for cls, pre in ((engine_module.Engine, ""), (engine_module.MsmBases, "MsmBases.")):
        names |= {pre + k for k, v in vars(cls).items() if not k.startswith("_") and (callable(v) or isinstance(v, staticmethod))}
    return names


def new_engine(engine_module):
    rec = Recorder()
    e = engine_module.Engine.__new__(engine_module.Engine)
    e.lib, e.ctx, e._pinned_stream, e._last_torch_stream, e._devices = rec, C.c_void_p(0x1234), False, {}, [0]
    e._follow_torch_stream = lambda t: None               # CPU tensors stand in for device tensors: no stream to follow
    return e, rec


def observe(engine_module):
    """{"<method>[<kwargs>]/<kind>": {"calls": [...], "results": [...]}} for every case and array kind."""
    table = {}
    for name, specs, kw in cases():
        kw = dict(kw)
        names = kw.pop("_names", None)
        torch_only = kw.pop("_torch_only", ())
        kinds = ["numpy"] if name in NO_ARRAYS else ["numpy", "torch"] + (["torch_f64"] if name == "fe_add" else [])
        for kind in kinds:
            e, rec = new_engine(engine_module)
            target = e
            if name.startswith("MsmBases."):
                target = e.msm_bases(_make(((N,), 20, U64), "numpy", 1))
                del rec.calls[:]
            ins = [_make(s, "torch" if i in torch_only else kind, 100 * (i + 1)) for i, s in enumerate(specs)]
            if names:
                args, kwargs = ins[:len(names) - 1], dict(kw, **{names[-1]: ins[-1]})
            else:
                args, kwargs = ins, kw
            ctx = e.ctx
            got = getattr(target, name.split(".")[-1])(*args, **kwargs)
            outs = list(got) if isinstance(got, tuple) else [got]
            shapes = ",".join("x".join(str(d) for d in tuple(lead) + (w,)) for lead, w, _ in specs)
            key = "%s(%s)%s/%s" % (name, shapes, json.dumps(kw, sort_keys=True) if kw else "", kind) + ("+out" if names else "")
            assert key not in table, key
            table[key] = {"calls": [[sym] + [_describe_arg(a, ctx, ins, outs) for a in cargs] for sym, cargs in rec.calls],
                          "results": [_describe_result(x) for x in outs]}
            for h in (got, target):
                if hasattr(h, "id"):
                    h.id = 0                                # a table handle: nothing to free on the stand-in
            e.ctx = None
    return table


def covered():
    return {name for name, _, _ in cases()} | {"msm_partial"}


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("ZC_RECORD_FROM") or os.path.dirname(os.path.dirname(HERE)))     # another checkout: the parent commit's
    from dusk_zerocaf_amd import engine
    with open(OUT, "w") as f:
        json.dump(observe(engine), f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT)
