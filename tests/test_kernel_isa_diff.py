"""tools/kernel_isa_diff.py: the normaliser and the classifier on hand-written assembly (no compiler, no GPU)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "kernel_isa_diff", os.path.join(os.path.dirname(__file__), "..", "tools", "kernel_isa_diff.py"))
kid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kid)


def _asm(body: str, fn: int = 0, vgprs: int = 8) -> str:
    body = body.replace("@", f".LBB{fn}_")
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.section\t.text.toy,"axG",@progbits,toy,comdat
\t.globl\ttoy
\t.p2align\t8
\t.type\ttoy,@function
toy:                                    ; @toy
; %bb.0:
{body}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel toy
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
\t.section\t.text.toy,"axG",@progbits,toy,comdat
.Lfunc_end{fn}:
\t.size\ttoy, .Lfunc_end{fn}-toy
; NumVgprs: {vgprs}
"""


BASE = """\ts_load_dword s4, s[0:1], 0x0
\ts_mul_i32 s5, s2, s3
\ts_add_i32 s6, s5, 16
\tds_read_b128 v[0:3], v4 offset:64
\ts_add_i32 s7, s5, 32
\ts_cbranch_scc1 @2
; %bb.1:
\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]
@2:
\ts_waitcnt lgkmcnt(0)"""


def _cls(new_body: str, **kw) -> str:
    base, new = kid.parse_kernels(_asm(BASE))["toy"], kid.parse_kernels(_asm(new_body, **kw))["toy"]
    return kid.classify(base, new)


def test_parse_keeps_instructions_and_descriptor_apart():
    body, desc = kid.parse_kernels(_asm(BASE))["toy"]
    assert body[0] == "s_load_dword s4, s[0:1], 0x0" and body[-1] == "s_endpgm"
    assert not any(ln.startswith(";") or "amdhsa" in ln for ln in body)
    assert desc == [".amdhsa_next_free_vgpr 8", ".amdhsa_next_free_sgpr 16"]


def test_label_numbers_and_comments_do_not_count():
    new = BASE.replace("@2", "@7").replace("; %bb.1:", "; %bb.3:\n                    ; implicit-def: $vgpr9")
    assert new != BASE
    assert _cls(new, fn=5) == "identical"


def test_commuted_sources():
    assert _cls(BASE.replace("s_mul_i32 s5, s2, s3", "s_mul_i32 s5, s3, s2")) == "commuted"
    # another operation on the same registers is no commutation
    assert _cls(BASE.replace("s_mul_i32 s5, s2, s3", "s_mul_hi_i32 s5, s3, s2")) == "different"


def test_address_arithmetic_moved_around_a_fixed_lds_read():
    lines = BASE.split("\n")
    i6, rd, i7 = lines[2], lines[3], lines[4]
    assert "s_add_i32 s6" in i6 and "ds_read_b128" in rd and "s_add_i32 s7" in i7
    lines[2:5] = [i7, rd, i6]
    assert _cls("\n".join(lines)) == "reordered-address"
    # the same move with the descriptor changed is not accepted
    assert _cls("\n".join(lines), vgprs=9) == "different"


def test_lds_read_from_another_address_register():
    assert _cls(BASE.replace("ds_read_b128 v[0:3], v4 offset:64", "ds_read_b128 v[0:3], v5 offset:64")) == "different"
    # nor may a memory operation move, even with every opcode still there
    lines = BASE.split("\n")
    lines.insert(7, lines.pop(3))  # the read goes behind the MFMA
    assert "v_mfma" in lines[6] and "ds_read" in lines[7]
    assert _cls("\n".join(lines)) == "different"
