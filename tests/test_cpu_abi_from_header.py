"""include/nqa.h is the only statement of the C ABI: nerf_qa_amd/_lib.py parses its signatures and constants from it,
and libnqa_hip.so exports what it declares and nothing else (csrc/nqa_exports.map).  CPU only, no device is touched.

(a) the parser's reading of every declaration against the compiler's own (`-ast-dump=json` of the project's compiler
    driver): the same names, parameter counts, per-position classes and return classes;
(b) every parsed constant, MIXED_STAGES and stage_prec against the compiler's values;
(c) the library's defined dynamic symbols are exactly the declared functions;
(d) altered header text: what could fool the parser parses right or is refused, and a swapped int / long or a dropped
    parameter makes (a)'s comparison fail;
(e) host arrays still marshal through c_void_p: ctypes array, byref / pointer object, None.
"""
import ctypes as C
import json
import os
import struct
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
CLASS = {C.c_int: "int", C.c_long: "long", C.c_size_t: "size_t", C.c_double: "double", C.c_float: "float",
         C.c_void_p: "pointer", C.c_char_p: "pointer"}
CHNS = (3, 64, 128, 256, 512, 512)


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(INCLUDE, "nqa.h")).read()


def _c_class(qual):
    """Class of a C type as the compiler spells it."""
    if "*" in qual or "[" in qual:
        return "pointer"
    # (LP64, the only data model the library is built for: should the compiler ever spell size_t out, it is unsigned
    # long; the parser itself refuses `unsigned long`, so this row can only ever match a size_t of the header)
    words = tuple(w for w in qual.split() if w != "const")
    return {("int",): "int", ("long",): "long", ("size_t",): "size_t", ("unsigned", "long"): "size_t",
            ("double",): "double", ("float",): "float"}[words]  # KeyError: a type the ABI does not use


@pytest.fixture(scope="module")
def compiler(tmp_path_factory):
    """The compiler's reading of nqa.h: ({nqa_* function: (return class, [parameter classes])}, {enum constant:
    value}), with every parsed constant and NQA_MIXED_STAGES(0..7) evaluated through enum constants of a probe file.
    A compiler that cannot be run FAILS the tests that need it: the build needs it anyway."""
    from nerf_qa_amd import build, _lib
    probe = tmp_path_factory.mktemp("abi") / "probe.c"
    probe.write_text('#include "nqa.h"\nenum {\n' + "".join(f"  PROBE_{n} = {n},\n" for n in _lib.CONSTANTS) +
                     "".join(f"  PROBE_MIXED_{p} = NQA_MIXED_STAGES({p}),\n" for p in range(8)) + "};\n")
    run = subprocess.run([build.HIPCC, "-x", "c", "-fsyntax-only", "-I", INCLUDE, "-Xclang", "-ast-dump=json",
                          str(probe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    funcs, enums = {}, {}
    for node in json.loads(run.stdout)["inner"]:
        if node["kind"] == "FunctionDecl" and node["name"].startswith("nqa_"):
            params = [p["type"]["qualType"] for p in node.get("inner", []) if p["kind"] == "ParmVarDecl"]
            assert not node.get("variadic"), node["name"]
            funcs[node["name"]] = (_c_class(node["type"]["qualType"].split("(")[0]), [_c_class(q) for q in params])
        elif node["kind"] == "EnumDecl":
            for e in node["inner"]:
                enums[e["name"]] = int(next(i for i in e["inner"] if i["kind"] == "ConstantExpr")["value"])
    return funcs, enums


def _mismatches(sigs, funcs):
    """(a)'s comparison: the parser's table against the compiler's declarations -> what differs, by name."""
    bad = [f"{n}: declared to one reader only" for n in sorted(set(sigs) ^ set(funcs))]
    for name in sorted(set(sigs) & set(funcs)):
        mine = (CLASS[sigs[name][0]], [CLASS[a] for a in sigs[name][1]])
        if mine != funcs[name]:
            bad.append(f"{name}: parser {mine}, compiler {funcs[name]}")
    return bad


def test_parser_agrees_with_the_compiler(compiler):
    from nerf_qa_amd import _lib
    funcs, _ = compiler
    assert len(funcs) > 100 and tuple(_lib._SIGNATURES) == _lib.EXPORTS
    assert _mismatches(_lib._SIGNATURES, funcs) == []


def test_constants_agree_with_the_compiler(compiler, header):
    from nerf_qa_amd import _lib
    _, enums = compiler
    for name, value in _lib.CONSTANTS.items():
        assert enums["PROBE_" + name] == value, name
    in_header = {n for n in enums if n.startswith("NQA_")}
    assert len(in_header) >= 21 and in_header <= set(_lib.CONSTANTS)
    assert {"NQA_VERSION", "NQA_NUM_CONVS", "NQA_NUM_TAPS", "NQA_TOTAL_CHNS"} <= set(_lib.CONSTANTS) - in_header
    # the Python names keep their values
    assert [_lib.CONSTANTS["NQA_PREC_" + n.upper()] for n in ("f32", "bf16", "f16", "f32s", "f32m", "f32m2", "f32m4",
            "f16w")] == [_lib.PREC_NAMES[n] for n in ("f32", "bf16", "f16", "f32s", "f32m", "f32m2", "f32m4", "f16w")]
    assert (_lib.NUM_CONVS, _lib.NUM_TAPS, _lib.TOTAL_CHNS) == (enums["PROBE_NQA_NUM_CONVS"],
                                                                enums["PROBE_NQA_NUM_TAPS"], enums["PROBE_NQA_TOTAL_CHNS"])
    assert len(_lib.K_NAMES) == enums["NQA_K_COUNT"]
    # NQA_MIXED_STAGES is a function-like macro, restated in _lib.py
    for prec in range(8):
        stages = enums[f"PROBE_MIXED_{prec}"]
        assert _lib.MIXED_STAGES.get(prec, 0) == stages, prec
        for stage in range(5):
            want = prec if stages == 0 else _lib.PREC_F16 if stage < stages else _lib.PREC_F32S
            assert _lib.stage_prec(prec, stage) == want, (prec, stage)


def _defined_dynamic_symbols(path):
    """Names of the defined entries of an ELF64 little-endian file's .dynsym."""
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    (_, _, _, _, off, size, link, _, _, entsize), = [s for s in sections if s[1] == 11]  # SHT_DYNSYM
    stroff = sections[link][4]
    names = []
    for at in range(off + entsize, off + size, entsize):  # entry 0 is the null symbol
        st_name, _, _, st_shndx = struct.unpack_from("<IBBH", blob, at)
        if st_shndx != 0:  # SHN_UNDEF: an import
            names.append(blob[stroff + st_name:blob.index(b"\0", stroff + st_name)].decode())
    return names


def test_library_exports_exactly_the_declared_functions(lib):
    from nerf_qa_amd import _lib
    names = _defined_dynamic_symbols(_lib.LIB_PATH)
    foreign = sorted(n for n in names if not n.startswith("nqa_"))
    assert not foreign, f"{len(foreign)} exported symbols outside the ABI, e.g. {foreign[:5]}"
    assert sorted(names) == sorted(_lib.EXPORTS), set(names) ^ set(_lib.EXPORTS)


TRICKY = """
/* a comment that talks about nqa_foo( and ends here */
#define NQA_NUM_TAPS 6   // and nqa_bar( in a line comment
#define NQA_TWICE(x) \\
  ((x) + nqa_baz(x))
enum { NQA_A = 0x10, NQA_B = -2 };
int
nqa_three(const float *const fx[NQA_NUM_TAPS],
          const void *const *x_taps, int out[5]);
size_t nqa_mid(int a, long b, const int c, double d, float e);
const char *nqa_text(void);
"""


def test_parser_reads_what_could_fool_it():
    from nerf_qa_amd._lib import parse_header
    vp = C.c_void_p
    sigs, consts = parse_header(TRICKY)
    assert sigs == {"nqa_three": (C.c_int, [vp, vp, vp]),
                    "nqa_mid": (C.c_size_t, [C.c_int, C.c_long, C.c_int, C.c_double, C.c_float]),
                    "nqa_text": (C.c_char_p, [])}
    assert consts == {"NQA_NUM_TAPS": 6, "NQA_A": 16, "NQA_B": -2}


@pytest.mark.parametrize("decl", [
    "int nqa_bad(unsigned x);",                    # an unknown scalar type
    "int nqa_bad(int64_t x);",
    "int nqa_bad(long long x);",
    "int nqa_bad(struct nqa_s s);",                # a struct, by value or behind a pointer
    "int nqa_bad(const struct nqa_s *s);",
    "int nqa_bad(int n, ...);",                    # varargs
    "int nqa_bad(void (*done)(int), int n);",      # a function pointer
    "int nqa_bad(int, long);",                     # unnamed parameters
    "void *nqa_bad(int n);",                       # a pointer return other than const char *
    "void nqa_bad(int n);",
    "typedef int nqa_t;",                          # not a declaration of a function
    "#ifdef NQA_EXTRAS\nint nqa_bad(int n);\n#endif",  # a declaration only some readers see
    "enum { NQA_X };",                             # an enumerator without its value
    "#define NQA_X (1 << 4)",                      # a constant that is not a literal
    "int nqa_bad(int n);\nint nqa_bad(int n);",
], ids=lambda d: d.split("\n")[0][:40])
def test_parser_refuses_what_it_does_not_understand(decl):
    from nerf_qa_amd._lib import NqaError, parse_header
    assert parse_header("int nqa_good(int n);")[0] == {"nqa_good": (C.c_int, [C.c_int])}
    with pytest.raises(NqaError, match="nqa.h"):
        parse_header("int nqa_good(int n);\n" + decl)


def test_unreadable_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    from nerf_qa_amd import _lib
    for path, text in ((tmp_path / "absent.h", None), (tmp_path / "empty.h", "/* nothing */\n"),
                       (tmp_path / "odd.h", "int nqa_bad(unsigned x);\n")):
        if text is not None:
            path.write_text(text)
        monkeypatch.setattr(_lib, "HEADER_PATH", str(path))
        with pytest.raises(_lib.NqaError, match=path.name):
            _lib._read_header()


@pytest.mark.parametrize("old,new,who", [
    ("long pixels, int C, void *out, void *stream", "int pixels, long C, void *out, void *stream", "nqa_split16_encode"),
    ("int nqa_l2pool(const void *in_nhwc, int n, int H, int W, int C, int prec,",
     "int nqa_l2pool(const void *in_nhwc, int n, int H, int W, int prec,", "nqa_l2pool"),
    ("size_t nqa_workspace_bytes(", "int nqa_workspace_bytes(", "nqa_workspace_bytes"),
    ("int nqa_timing_enable(int on);", "", "nqa_timing_enable"),
], ids=["swapped_int_long", "dropped_parameter", "return_type", "dropped_declaration"])
def test_a_wrong_reading_fails_the_comparison(compiler, header, old, new, who):
    """Deliberately wrong replays: the header as the compiler read it against the parse of an altered text."""
    from nerf_qa_amd._lib import parse_header
    funcs, _ = compiler
    assert header.count(old) == 1
    bad = _mismatches(parse_header(header.replace(old, new))[0], funcs)
    assert len(bad) == 1 and bad[0].startswith(who + ":"), bad


def _ints(v):
    return (C.c_int * len(v))(*v)


def test_host_arrays_still_marshal(lib):
    """Three host-only entry points, each with a ctypes array, with byref / a pointer object, and with None where the
    function refuses it; the figures are those the hand-typed POINTER(c_int) positions gave."""
    hk = wk = (8, 8, 4, 2, 1, 1)
    assert lib.nqa_stats_scratch_bytes(2, _ints(CHNS), _ints(hk), _ints(wk)) == 118016
    c, h, w = _ints(CHNS), _ints(hk), _ints(wk)
    assert lib.nqa_stats_scratch_bytes(2, C.byref(c), C.pointer(h), C.cast(w, C.POINTER(C.c_int))) == 118016
    assert lib.nqa_stats_scratch_bytes(2, C.addressof(c), h, w) == 118016
    assert lib.nqa_stats_scratch_bytes(2, None, h, w) == 0

    # (70, 45) under a 9-tap window: taps 70x45, 70x45, 35x23, 18x12, 9x6, 5x3; the last two are under the window
    want = (4, [62, 62, 27, 10, 1, 1], [37, 37, 15, 4, 1, 1])
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    assert (lib.nqa_adists_chain_dims_n(70, 45, 9, mh, mw), list(mh), list(mw)) == want
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    assert (lib.nqa_adists_chain_dims_n(70, 45, 9, C.byref(mh), C.pointer(mw)), list(mh), list(mw)) == want
    assert lib.nqa_adists_chain_dims_n(70, 45, 9, None, mw) == -1
    assert lib.nqa_last_error() == b"adists_chain_dims: null pointer"

    g = (C.c_int * 3)()
    assert (lib.nqa_stats_nhwc_grid(2, 35, 64, 0, g), list(g)) == (0, [64, 1, 16])
    g = (C.c_int * 3)()
    assert (lib.nqa_stats_nhwc_grid(2, 35, 64, 0, C.byref(g)), list(g)) == (0, [64, 1, 16])
    assert lib.nqa_stats_nhwc_grid(2, 35, 64, 0, None) == -1
    assert lib.nqa_last_error() == b"stats_nhwc_grid: null pointer"
