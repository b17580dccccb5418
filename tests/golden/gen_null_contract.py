#!/usr/bin/env python3
"""Generate tests/golden/null_contract.json: which pointers of every batched entry point are required and how the library
names them.  The library loads without a GPU and checks its pointers before it touches the context, so every entry point is
called with ctx = NULL, valid by-value arguments and dummy non-NULL pointers, then with each pointer NULL in turn; the status
and zc_last_error() of every call are the table.  tests/test_null_contract.py replays `observe()` and compares with the file.

    python tests/golden/gen_null_contract.py           # rewrites the file from the library built in this tree
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "null_contract.json")

# the entry points that do not move rows through the batched staging (own pipelines: MSM, exchange, context)
NOT_BATCHED = ("zc_msm", "zc_comm", "zc_ctx", "zc_ed_fold_ordered")

# valid by-value arguments by (symbol, position after ctx); every other size_t is a count of 1, every other integer 0
BY_VALUE = {("zc_sc_shr", 1): 3, ("zc_sc_compute_naf", 1): 4, ("zc_ed_mul_by_pow_2", 1): 3, ("zc_ed_mul_base_wnaf", 1): 4,
            ("zc_fe_mod_sqrt", 1): 1}
# zc_ed_scalar_mul takes another path per flag value (STRICT, LTR_BIN, BINARY_NAF, FAST)
VARIANTS = {"zc_ed_scalar_mul": [{4: f} for f in (0, 1, 2, 16)]}


def batched_symbols(signatures):
    return [s for s in signatures if not s.startswith(NOT_BATCHED)]


def observe(lib, signatures):
    """{"<symbol>[<variant>]": {"none": [status, message], "<position>": [status, message] per pointer}}"""
    dummy = C.create_string_buffer(4096)
    addr = C.addressof(dummy)
    table = {}
    for sym in batched_symbols(signatures):
        sig = signatures[sym]
        for variant in VARIANTS.get(sym, [{}]):
            args = []
            for i, t in enumerate(sig):
                if t is C.c_void_p:
                    args.append(addr)
                else:
                    args.append(variant.get(i, BY_VALUE.get((sym, i), 1 if t is C.c_size_t else 0)))

            def call(a):
                rc = getattr(lib, sym)(None, *a)
                return [rc, lib.zc_last_error().decode()]
            row = {"none": call(args)}
            for i, t in enumerate(sig):
                if t is C.c_void_p:
                    row[str(i)] = call(args[:i] + [None] + args[i + 1:])
            table[sym + (json.dumps(variant, sort_keys=True) if variant else "")] = row
    return table


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from dusk_zerocaf_amd import _lib
    lib = _lib._bind(os.environ["ZC_RECORD_FROM"]) if os.environ.get("ZC_RECORD_FROM") else _lib.load()     # another build: the parent commit's
    with open(OUT, "w") as f:
        json.dump(observe(lib, _lib.SIGNATURES), f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT)
