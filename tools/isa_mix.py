#!/usr/bin/env python3
"""Instruction mix of the unified-step loop of k_ed_scalar_mul, from the compiler's own ISA.

Compiles the library source to gfx950 assembly (hipcc -S --offload-device-only, no GPU needed), finds
the largest backward-branch loop of the kernel and counts opcodes.  Writes the JSON named by --out (profiles/rNN_isa_mix.json),
which tools/make_roofline_inputs.py uses to split the PMC instruction count into the multiplier-rate class
(v_mad_u64_u32, v_mul_lo_u32, 64-bit shifts: ~5 cycles per wave-instruction per SIMD) and the rest.
`kernel:steps` (k_ed_scalar_mul_pw) counts the generic step and the doubling step of the step loop apart, see steps().
Usage: python tools/isa_mix.py [kernel[:whole|:inner|:steps] ...] [--asm saved.s] [--out profiles/rNN_isa_mix.json]
"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zerocaf_hip.hip")
SLOW = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_lshrrev_b64", "v_lshlrev_b64", "v_lshl_add_u64")


def compile_asm():
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "zc.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--offload-device-only",
                        "-o", asm, SRC], check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def mix(text, kernel, whole=False, inner=False):
    """Opcode counts of the kernel's largest inner loop (whole=True: of the whole kernel body, every
    instruction counted once -- for kernels whose time is spread over several loops of the same make-up;
    inner=True: the smallest loop that still holds >= 1000 v_mad_u64_u32 -- the step loop of a kernel
    whose outermost loop walks tiles)."""
    i0 = text.index("\n%s:" % kernel)
    body = text[i0:text.index(".Lfunc_end", i0)]
    lines = []
    for l in body.split("\n"):
        l = l.split(";")[0].strip()
        if l and not l.startswith((".p2align", ".section", ".type", ".globl", "#")):
            lines.append(l)
    labels = {l[:-1]: i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            loops.append((i - labels[m.group(1)], labels[m.group(1)], i))
    # the step loop: the largest loop that is nested in the (slightly larger) per-block loop, if any
    loops.sort(reverse=True)
    size, a, b = loops[1] if len(loops) > 1 and loops[1][0] > 0.9 * loops[0][0] else loops[0]
    if inner:
        cands = [(sz, x, y) for sz, x, y in loops if sum(1 for l in lines[x:y] if l.startswith("v_mad_u64_u32")) >= 1000]
        size, a, b = min(cands)
    if whole:
        a, b = 0, len(lines)
    ops = collections.Counter(l.split()[0] for l in lines[a:b] if not l.endswith(":"))
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    slow = {k: v for k, v in ops.items() if k in SLOW}
    return {"kernel": kernel, "source": "hipcc -S --offload-device-only, " + ("whole kernel body" if whole else "largest inner loop"),
            "valu_per_step": valu, "multiplier_rate_class_per_step": sum(slow.values()), "multiplier_rate_class": slow,
            "multiplier_rate_share": round(sum(slow.values()) / valu, 4),
            "s_nop_per_step": ops.get("s_nop", 0),
            "other_valu": {k: v for k, v in ops.most_common() if k.startswith("v_") and k not in SLOW}}


def _counts(ops):
    ops = collections.Counter(ops)
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    slow = sum(v for k, v in ops.items() if k in SLOW)
    return {"valu": valu, "multiplier_rate_class": slow, "other_valu": valu - slow,
            "v_mov": sum(v for k, v in ops.items() if k.startswith("v_mov_")), "v_cndmask": sum(v for k, v in ops.items() if k.startswith("v_cndmask_")),
            "s_nop": ops.get("s_nop", 0), "opcodes": {k: v for k, v in ops.most_common() if k.startswith("v_")}}


def steps(text, kernel):
    """The generic step and the doubling step of k_ed_scalar_mul_pw's step loop, counted apart (mode `:steps`).

    The step loop is the kernel's depth-2 loop.  The doubling step starts at the block behind the last wave-uniform branch
    in front of the stash write (the first ds_write of the loop) and consists of every block of the loop that can be reached
    from there without passing the loop header, wherever the compiler laid it out (its tail stands in front of the header);
    the generic step is the rest of the loop.  So the ballots that decide on a doubling step count with the generic step,
    the test whether a lane stashes its addend with the doubling step.  Also given: the blocks of the tile loop in front of
    the step loop (loads, the gate) and behind it (ptm_to_pt, the stores), which run once per tile."""
    i0 = text.index("\n%s:" % kernel)
    body = text[i0:text.index(".Lfunc_end", i0)].split("\n")
    blocks = []
    for raw in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", raw) or re.match(r"^; (%bb\.\d+):\s*(;.*)?$", raw)
        if m:
            blocks.append({"name": m.group(1), "cmt": m.group(2) or "", "lines": []})
        elif blocks:
            if raw.strip().startswith(";") and "Loop" in raw and not blocks[-1]["lines"]:
                blocks[-1]["cmt"] += raw
            l = raw.split(";")[0].strip()
            if l and not l.startswith("."):
                blocks[-1]["lines"].append(l)
    index = {b["name"]: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        b["ops"] = [l.split()[0] for l in b["lines"]]
        b["succ"] = {index[l.split()[1]] for l in b["lines"] if re.match(r"s_c?branch\w* \.LBB", l)}
        if i + 1 < len(blocks) and (b["ops"] or [""])[-1] not in ("s_branch", "s_endpgm"):
            b["succ"].add(i + 1)
    hdr = next(i for i, b in enumerate(blocks) if "Inner Loop Header: Depth=2" in b["cmt"])
    tag = "Header=%s Depth=2" % blocks[hdr]["name"].lstrip(".L")
    inner = [i for i, b in enumerate(blocks) if i == hdr or tag in b["cmt"]]
    stash = next(i for i in inner if any(o.startswith("ds_write") for o in blocks[i]["ops"]))
    start = max(i for i in inner if i <= stash and (blocks[i - 1]["ops"] or [""])[-1].startswith(("s_cbranch_vcc", "s_cbranch_scc")))
    d_blocks, todo = set(), [start]
    while todo:
        i = todo.pop()
        if i in d_blocks or i == hdr or i not in inner:
            continue
        d_blocks.add(i)
        todo += blocks[i]["succ"]
    g_blocks = [i for i in inner if i not in d_blocks]
    ops_of = lambda idx: [o for i in idx for o in blocks[i]["ops"]]
    return {"kernel": kernel, "source": "hipcc -S --offload-device-only, the depth-2 loop split at the doubling step's first block",
            "g_step": dict(_counts(ops_of(g_blocks)), blocks=[blocks[i]["name"] for i in g_blocks]),
            "d_step": dict(_counts(ops_of(sorted(d_blocks))), blocks=[blocks[i]["name"] for i in sorted(d_blocks)]),
            "tile_prologue": _counts(ops_of(range(0, min(inner)))), "tile_epilogue": _counts(ops_of(range(max(inner) + 1, len(blocks))))}


def main():
    """python tools/isa_mix.py [kernel[:whole|:inner|:steps] ...] [--out profiles/rNN_isa_mix.json]"""
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    asm_path = None
    if "--asm" in args:                       # count a saved assembly file (another commit's, for a side-by-side) instead of compiling
        i = args.index("--asm")
        asm_path = args[i + 1]
        del args[i:i + 2]
    kernels = args or ["k_ed_scalar_mul"]
    text = open(asm_path).read() if asm_path else compile_asm()
    res = {}
    for k in kernels:
        name, _, mode = k.partition(":")
        if mode == "steps":
            res[name + ":steps"] = s = steps(text, name)
            for part in ("g_step", "d_step", "tile_prologue", "tile_epilogue"):
                print(json.dumps(dict({"kernel": name, "part": part}, **{x: s[part][x] for x in ("valu", "multiplier_rate_class", "other_valu", "v_mov", "v_cndmask", "s_nop")})))
            continue
        res[name] = mix(text, name, whole=(mode == "whole"), inner=(mode == "inner"))
        print(json.dumps({x: res[name][x] for x in ("kernel", "valu_per_step", "multiplier_rate_class_per_step", "multiplier_rate_share", "multiplier_rate_class")}))
    if out_path:
        json.dump(res, open(out_path if os.path.isabs(out_path) else os.path.join(ROOT, out_path), "w"), indent=1)


if __name__ == "__main__":
    main()
