"""ctypes binding of libnqa_hip.so, read from include/nqa.h.

The library is the product: if it is missing or does not load, importing this module's
`lib()` raises.  There is no CPU or eager-PyTorch fallback anywhere in nerf_qa_amd.

The header is the only statement of the ABI: `_SIGNATURES` and the constants below are parsed from it when this
module is imported (`parse_header`), by these rules, and whatever they do not cover is refused with an NqaError that
names the declaration -- the parser never guesses:
  - comments go first, then preprocessor lines (a trailing backslash continues one).  `#define NQA_X v` with an integer
    v is a constant; function-like macros and the includes are skipped; the include guard and the `#ifdef __cplusplus`
    blocks (dropped whole, this is the C reading) are the only conditionals allowed;
  - `enum { NQA_X = v, ... };` blocks give constants, every enumerator with its own integer value;
  - every other statement is a declaration `ret nqa_name(params);`, which may span lines;
  - a parameter containing `*` or `[` is a pointer: c_void_p, host or device alike (the header cannot tell them apart;
    c_void_p takes ctypes arrays, pointers, byref(), integers and None);
  - any other parameter is `[const] type name` with type one of int, long, size_t, double, float;
  - the return type is one of those five, or `const char *`: c_char_p;
  - a struct, union or enum type, a function pointer, `...`, an unnamed parameter, any other type: refused.
tests/test_cpu_abi_from_header.py holds this reading to the compiler's own.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch  # noqa: F401  (loads the HIP runtime the library binds to; must come first)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NQA_LIB") or os.path.join(_HERE, "libnqa_hip.so")  # NQA_LIB: development builds only
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nqa.h"))


class NqaError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}
_NOT_A_NAME = set(_SCALARS) | {"unsigned", "signed", "short", "char", "void", "const"}


def _int(text: str, what: str) -> int:
    try:
        return int(text.strip(), 0)
    except ValueError:
        raise NqaError(f"nqa.h: {what}: {text.strip()!r} is not an integer literal") from None


def _scalar(words: str, decl: str):
    """`[const] type [name]` without the name -> ctypes type."""
    names = [w for w in words.split() if w != "const"]
    if len(names) != 1 or names[0] not in _SCALARS:
        raise NqaError(f"nqa.h: type {words.strip()!r} is not one the binding knows, in `{decl}`")
    return _SCALARS[names[0]]


def parse_header(text: str):
    """The text of nqa.h -> ({name: (restype, [argtypes])}, {NQA_X: value}), by the module docstring's rules."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    consts, code, in_cxx = {}, [], False
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            if not in_cxx:
                code.append(line)
            continue
        word = line.replace("#", " ", 1).split() or [""]
        if word[0] == "endif":  # closes the guard or a __cplusplus block: every other conditional is refused below
            in_cxx = False
        elif word[:2] == ["ifdef", "__cplusplus"]:
            in_cxx = True
        elif word[0] in ("if", "ifdef", "ifndef", "else", "elif") and word[:2] != ["ifndef", "NQA_H"]:
            raise NqaError(f"nqa.h: conditional `{line.strip()}`: the binding reads every declaration unconditionally")
        elif word[0] == "define" and len(word) > 2 and re.fullmatch(r"NQA_\w+", word[1]):
            consts[word[1]] = _int(" ".join(word[2:]), f"#define {word[1]}")
    code = " ".join(" ".join(code).split())

    def enum(m):
        for item in m.group(1).split(","):
            name, eq, value = item.partition("=")
            if not eq or not re.fullmatch(r"NQA_\w+", name.strip()):
                raise NqaError(f"nqa.h: enumerator `{item.strip()}` is not `NQA_X = value`")
            consts[name.strip()] = _int(value, f"enumerator {name.strip()}")
        return " "
    code = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, code)

    sigs = {}
    for decl in filter(None, (d.strip() for d in code.split(";"))):
        m = re.fullmatch(r"([\w\s\*]+?)\b(nqa_\w+)\s*\(([^()]*)\)", decl)
        if not m or re.search(r"\b(struct|union|enum)\b", decl) or "..." in decl:
            raise NqaError(f"nqa.h: `{decl}` is not a plain C declaration `ret nqa_name(params)` the binding can read")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if name in sigs:
            raise NqaError(f"nqa.h: {name} is declared twice")
        restype = C.c_char_p if ret.split() == ["const", "char", "*"] else _scalar(ret, decl)
        argtypes = []
        for p in ([] if params == "void" else params.split(",")):
            if "*" in p or "[" in p:
                argtypes.append(C.c_void_p)
                continue
            typ, _, pname = p.strip().rpartition(" ")
            if pname in _NOT_A_NAME or not re.fullmatch(r"[A-Za-z_]\w*", pname):
                raise NqaError(f"nqa.h: parameter `{p.strip()}` of `{decl}` has no name")
            argtypes.append(_scalar(typ, decl))
        sigs[name] = (restype, argtypes)
    return sigs, consts


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            sigs, consts = parse_header(f.read())
        if not sigs:
            raise NqaError("nqa.h: no declaration found")
    except (OSError, NqaError) as e:
        raise NqaError(f"{HEADER_PATH}: the C ABI is read from this header and it cannot be: {e}") from None
    return sigs, consts


_SIGNATURES, CONSTANTS = _read_header()
EXPORTS = tuple(_SIGNATURES)

(PREC_F32, PREC_BF16, PREC_F16, PREC_F32S, PREC_F32M, PREC_F32M2, PREC_F32M4, PREC_F16W) = (
    CONSTANTS["NQA_PREC_" + n] for n in ("F32", "BF16", "F16", "F32S", "F32M", "F32M2", "F32M4", "F16W"))
PREC_NAMES = {"f32": PREC_F32, "fp32": PREC_F32, "bf16": PREC_BF16, "f16": PREC_F16, "fp16": PREC_F16,
              "f32s": PREC_F32S, "f32m": PREC_F32M, "f32m2": PREC_F32M2, "f32m4": PREC_F32M4, "f16w": PREC_F16W}
PREC_DTYPE = {PREC_F32: torch.float32, PREC_BF16: torch.bfloat16, PREC_F16: torch.float16, PREC_F32S: torch.float32}
# NQA_MIXED_STAGES (a function-like macro, restated; the tests hold it to the compiler's): the mixed modes run their
# first pyramid stages as f16 kernels on two-term weights, the rest as f32s
MIXED_STAGES = {PREC_F32M: 3, PREC_F32M2: 2, PREC_F32M4: 4, PREC_F16W: 5}


def stage_prec(prec: int, stage: int) -> int:
    """Kernel precision of pyramid stage `stage` (0-based) / of tap stage+1 in mode `prec` (include/nqa.h)."""
    if prec not in MIXED_STAGES:
        return prec
    return PREC_F16 if stage < MIXED_STAGES[prec] else PREC_F32S
NUM_CONVS, NUM_TAPS, TOTAL_CHNS = CONSTANTS["NQA_NUM_CONVS"], CONSTANTS["NQA_NUM_TAPS"], CONSTANTS["NQA_TOTAL_CHNS"]
K_NAMES = ("conv1_1", "conv_igemm", "l2pool", "stats", "adists", "prep", "pool_seam")
assert len(K_NAMES) == CONSTANTS["NQA_K_COUNT"], "K_NAMES names every timing class of nqa.h"

_lib = None


def lib() -> C.CDLL:
    """Load libnqa_hip.so once; raise if it is not there (build with `python -m nerf_qa_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NqaError(f"{LIB_PATH} not found: the HIP library is required "
                           "(run `python -m nerf_qa_amd.build`); there is no fallback path")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the ABI is incomplete
            fn.restype, fn.argtypes = res, args
        if handle.nqa_version() != CONSTANTS["NQA_VERSION"]:
            raise NqaError("libnqa_hip.so: ABI version mismatch")
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise NqaError(f"libnqa_hip error {rc}: {lib().nqa_last_error().decode()}")


def prec_id(prec) -> int:
    if isinstance(prec, str):
        return PREC_NAMES[prec.lower()]
    return int(prec)


def ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream
