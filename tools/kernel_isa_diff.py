#!/usr/bin/env python3
"""Compare the gfx950 instruction stream of every kernel between a base checkout and this tree.

    python tools/kernel_isa_diff.py BASE_TREE [--files a.hip b.hip ...]

Both trees' sources (default: every file of build.SOURCES) are compiled with build.FLAGS + build.FILE_FLAGS, device
pass only, to assembly (at most 16 compilers at a time; no GPU is used; a source that one tree lacks gives that tree no
kernels).  Kernels are matched by mangled name across all files, local label numbers are normalised, comment-only lines dropped, and each kernel is put into one class:

    identical          same instruction text and same .amdhsa_ descriptor
    commuted           every differing line has the same opcode and destination and the same sources in another order
    reordered-address  same opcode multiset, same descriptor, and the memory operations, MFMAs, waits and barriers
                       (PINNED below) are the same lines in the same order: only address arithmetic moved between them
    different          anything else

One line per kernel; the unified diff of every kernel that is not identical.  Exit status 1 if a kernel is different
or exists on one side only.  This is how a change to the hand-scheduled kernels (csrc/nqa_regw.h and its users) is
judged: see DESIGN.md.  The comparison is of instruction text only.
"""
from __future__ import annotations

import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# opcodes that must not move or change for `reordered-address`
PINNED = ("v_mfma", "ds_", "buffer_", "global_", "flat_", "scratch_", "s_waitcnt", "s_barrier", "s_setprio", "s_sleep")
_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse_kernels(asm: str) -> dict:
    """Assembly text of one device pass -> {mangled kernel name: (instruction lines, descriptor lines)}, comments and
    blank lines dropped, whitespace collapsed, labels as they are."""
    funcs, out = set(), {}
    name, body, desc, in_desc = None, [], [], False
    for raw in asm.splitlines():
        line = " ".join(raw.split(";", 1)[0].split())
        if not line:
            continue
        m = re.match(r"\.type (\S+),@function$", line)
        if m:
            funcs.add(m.group(1))
            continue
        if name is None:
            if line.endswith(":") and line[:-1] in funcs:
                name, body, desc = line[:-1], [], []
            continue
        if line == f".amdhsa_kernel {name}":
            in_desc = True
        elif line == ".end_amdhsa_kernel":
            out[name] = (body, desc)
            name, in_desc = None, False
        elif in_desc:
            desc.append(line)
        elif re.match(r"\.Lfunc_end\d+:$", line):  # a device function that is no kernel
            name = None
        elif not line.startswith(".section"):
            body.append(line)
    return out


def normalize(lines: list) -> list:
    """Local labels (.LBB<f>_<n>, .Ltmp<n>, ...) renumbered in order of first appearance inside the kernel."""
    names: dict = {}
    return [_LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), ln) for ln in lines]


def _split(line: str):
    op, _, rest = line.partition(" ")
    return (".label" if op.endswith(":") else op), [a.strip() for a in rest.split(",")] if rest else []


def classify(base, new) -> str:
    """base, new: (instruction lines, descriptor lines) of one kernel, as parse_kernels returns them."""
    a, b = normalize(base[0]), normalize(new[0])
    same_desc = base[1] == new[1]
    if a == b and same_desc:
        return "identical"
    if not same_desc:
        return "different"
    if len(a) == len(b):
        for x, y in zip(a, b):
            if x != y:
                (ox, ax), (oy, ay) = _split(x), _split(y)
                if ox != oy or not ax or ax[0] != ay[0] or sorted(ax[1:]) != sorted(ay[1:]):
                    break
        else:
            return "commuted"
    ops = lambda ls: collections.Counter(_split(ln)[0] for ln in ls)  # noqa: E731
    pinned = lambda ls: [ln for ln in ls if ln.startswith(PINNED)]    # noqa: E731
    if ops(a) == ops(b) and pinned(a) == pinned(b):
        return "reordered-address"
    return "different"


def unified(base, new, name: str) -> str:
    a, b = normalize(base[0]) + base[1], normalize(new[0]) + new[1]
    return "\n".join(difflib.unified_diff(a, b, f"base/{name}", f"head/{name}", lineterm="", n=2))


def compile_one(build, tree: str, src: str, outdir: str):
    """Device pass of tree/nerf_qa_amd/csrc/src to assembly -> (src, parse_kernels of it)."""
    if not os.path.exists(os.path.join(tree, "nerf_qa_amd", "csrc", src)):
        return src, {}  # a source only the other tree has: its kernels, if any, show as "head only" / "base only"
    os.makedirs(outdir, exist_ok=True)
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    cmd = [build.HIPCC, *build.FLAGS, *build.FILE_FLAGS.get(src, []), "--cuda-device-only", "-S",
           os.path.join(tree, "nerf_qa_amd", "csrc", src), "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}: {src}\n" + "\n".join(
            ln for ln in p.stdout.splitlines() if "-Rpass-analysis" not in ln))
    with open(out) as f:
        return src, parse_kernels(f.read())


def main(argv=None) -> int:
    sys.path.insert(0, ROOT)
    from nerf_qa_amd import build

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("base_tree", help="a checkout of the commit to compare against")
    ap.add_argument("--files", nargs="+", default=list(build.SOURCES), help="sources of csrc/ (default: all)")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files in DIR/base and DIR/head")
    args = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        trees = {"base": args.base_tree, "head": ROOT}
        jobs = [(side, src) for side in trees for src in args.files]
        with ThreadPoolExecutor(max_workers=16) as pool:  # one compiler per job
            done = list(pool.map(lambda j: compile_one(build, trees[j[0]], j[1], os.path.join(work, j[0])), jobs))
    base, head = {}, {}
    for (side, _), (src, ks) in zip(jobs, done):
        for k, v in ks.items():
            (base if side == "base" else head)[k] = (src, *v)
    bad, diffs = 0, []
    for name in sorted(set(base) | set(head)):
        if name not in base or name not in head:
            cls, src = ("head only" if name in head else "base only"), (head.get(name) or base[name])[0]
            bad += 1
        else:
            cls, src = classify(base[name][1:], head[name][1:]), head[name][0]
            bad += cls == "different"
            if cls != "identical":
                diffs.append(unified(base[name][1:], head[name][1:], name))
        print(f"{cls:18s} {src:24s} {name}")
    for d in diffs:
        print("\n" + d)
    print(f"\n{len(set(base) | set(head))} kernels, {bad} not accepted")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
