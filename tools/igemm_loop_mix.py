"""Instruction mix of the implicit GEMM's stage loop (nqa_conv.hip conv3x3_igemm_tile), read off the compiler's assembly; no
GPU needed.  nqa_conv.hip is compiled for gfx950 with the flags of nerf_qa_amd/build.py (device pass only, -S); in each
named kernel instantiation every loop that holds MFMAs -- the stage loop; the mixed kernel has two, its 32-wide and its
16-wide body -- is taken from its header label to its back edge and its instructions are counted by kind:
  mfma   v_mfma_*                      ds_read  ds_read_* / ds_load_*
  dma    buffer loads with `lds`       scalar   s_*
  valu   every other v_* (what a SIMD issues beside its MFMAs: address arithmetic, moves)
  other  whatever is left (ds_write, plain memory instructions)
usage: python tools/igemm_loop_mix.py [--source PATH/nqa_conv.hip] [--label TEXT] [--max-valu N]
--max-valu N exits 1 if a stage loop of an M16 instance listed below holds more than N `valu` instructions."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_qa_amd import build as nqa_build  # noqa: E402


def _plain(p, wn, wm, tn, tm, tw, nterm):
    return (f"conv3x3_igemm_kernel<{p}, {wn},{wm},{tn},{tm}, {tw}, true, {nterm}>",
            f"conv3x3_igemm_kernelINS_{len(p)}{p}ELi{wn}ELi{wm}ELi{tn}ELi{tm}ELi{tw}ELb1ELi{nterm}ELb0EE")


def _mixed(p, wn, wm, tn, tm, nterm):
    return (f"conv3x3_igemm_mixed_kernel<{p}, {wn},{wm},{tn},{tm}, true, {nterm}>",
            f"conv3x3_igemm_mixed_kernelINS_{len(p)}{p}ELi{wn}ELi{wm}ELi{tn}ELi{tm}ELb1ELi{nterm}EE")


# (printed name, fragment of the mangled name)
INSTANCES = [_plain("PrecF16", 2, 4, 4, 2, tw, nt) for tw in (32, 16) for nt in (1, 2)] + \
            [_plain("PrecF16", 2, 2, 2, 2, 32, nt) for nt in (1, 2)] + \
            [_mixed("PrecF16", 2, 4, 4, 2, nt) for nt in (1, 2)] + \
            [_plain("PrecBF16", 2, 4, 4, 2, 32, 1), _plain("PrecF16", 2, 4, 2, 4, 32, 1), _mixed("PrecF16", 2, 2, 2, 2, 1)]
KINDS = ("mfma", "ds_read", "dma", "scalar", "valu", "other")


def assembly(source):
    flags = [f for f in nqa_build.FLAGS if not f.startswith("-Rpass")] + nqa_build.FILE_FLAGS.get("nqa_conv.hip", [])
    cmd = [nqa_build.HIPCC, *flags, "-I", nqa_build.CSRC, "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
           source, "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def kind(mnemonic, operands):
    if mnemonic.startswith("v_mfma"):
        return "mfma"
    if mnemonic.startswith(("ds_read", "ds_load")):
        return "ds_read"
    if mnemonic.startswith("buffer_load") and re.search(r"\blds\b", operands):
        return "dma"
    if mnemonic.startswith("s_"):
        return "scalar"
    if mnemonic.startswith("v_"):
        return "valu"
    return "other"


def mfma_loops(body):
    """[(counts by kind, {valu mnemonic: count})] of every loop of one function's lines that holds MFMAs, in source order."""
    labels = {m.group(1): i for i, ln in enumerate(body) if (m := re.match(r"(\.LBB\d+_\d+):", ln))}
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(?:\S+,\s*)?(\.LBB\d+_\d+)", ln)
        if not m or labels.get(m.group(1), i) >= i:
            continue
        counts, valu = dict.fromkeys(KINDS, 0), {}
        for ins in body[labels[m.group(1)]:i + 1]:
            mm = re.match(r"\s+([a-z][a-z0-9_]*)\s*(.*)", ins)
            if not mm:
                continue
            k = kind(mm.group(1), mm.group(2))
            counts[k] += 1
            if k == "valu":
                valu[mm.group(1)] = valu.get(mm.group(1), 0) + 1
        if counts["mfma"]:
            loops.append((counts, valu))
    return loops


def main():
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default  # noqa: E731
    source = opt("--source", os.path.join(nqa_build.CSRC, "nqa_conv.hip"))
    max_valu = int(opt("--max-valu", -1))
    lines = assembly(source).splitlines()
    starts = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r"(_Z\w+):", ln))}
    print(f"# {opt('--label', os.path.relpath(source, ROOT))}: instructions of one stage of one wave, stage-loop header to "
          f"back edge")
    print(f"{'kernel':72s} " + " ".join(f"{k:>7s}" for k in KINDS) + "  valu by mnemonic")
    over = 0
    for shown, frag in INSTANCES:
        name = next((n for n in starts if frag in n), None)
        if name is None:
            print(f"{shown:72s} (not instantiated)")
            continue
        end = next(i for i in range(starts[name], len(lines)) if lines[i].startswith(".Lfunc_end"))
        for n_loop, (counts, valu) in enumerate(mfma_loops(lines[starts[name]:end])):
            tag = shown + (f" loop {n_loop}" if "mixed" in shown else "")
            print(f"{tag:72s} " + " ".join(f"{counts[k]:7d}" for k in KINDS) + "  " +
                  ", ".join(f"{v} {k}" for k, v in sorted(valu.items(), key=lambda kv: -kv[1])))
            over += 0 <= max_valu < counts["valu"]
    if over:
        sys.exit(f"{over} stage loop(s) hold more than {max_valu} non-MFMA vector instructions")


if __name__ == "__main__":
    main()
