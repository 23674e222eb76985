"""tools/isa_same.py on two short listings written here (no GPU, no compiler): the order of the kernels in a listing and the
function numbers in its labels do not count, one changed operand does, a missing kernel does."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(__file__), "..", "tools", "isa_same.py")


@pytest.fixture(scope="module")
def isa_same():
    spec = importlib.util.spec_from_file_location("isa_same", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel(name, fn, operand="v1", vgprs=8):
    """One kernel as `make asm` lists it, the fn-th function of its file: a loop, a forward branch, its descriptor."""
    return """\t.text
\t.protected\t{n} ; -- Begin function {n}
\t.globl\t{n}
\t.p2align\t8
\t.type\t{n},@function
{n}:          ; @{n}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_u32_e32 vcc, 4, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB{f}_3
.LBB{f}_1:                                ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v0, v0, {op}
\tv_cmp_lt_u32_e32 vcc, 63, v0
\ts_cbranch_vccz .LBB{f}_1
; %bb.2:                                ;   in Loop: Header=BB{f}_1 Depth=1
\tv_mov_b32_e32 v1, 0
.LBB{f}_3:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {n}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_kernarg_size 8
\t\t.amdhsa_next_free_vgpr {v}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{f}:
\t.size\t{n}, .Lfunc_end{f}-{n}
                                        ; -- End function
\t.set {n}.num_vgpr, {v}
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
; NumVgprs: {v}
""".format(n=name, f=fn, op=operand, v=vgprs)


HEAD = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n'
TAIL = '\t.type\t__hip_cuid_0,@object\n__hip_cuid_0:\n\t.byte\t0\n\t.amdgpu_metadata\n---\namdhsa.kernels: []\n...\n\t.end_amdgpu_metadata\n'
A, B = "_Z8a_kernelPj", "_Z8b_kernelILi2EEvPj"


def listing(*parts):
    return HEAD + "".join(parts) + TAIL


def test_order_and_label_numbers_do_not_count(isa_same):
    old = listing(kernel(A, 0), kernel(B, 1, operand="v2"))
    new = listing(kernel(B, 0, operand="v2"), kernel(A, 1))
    assert sorted(isa_same.kernels(old)) == [A, B]
    assert ".LBB0_" not in isa_same.kernels(old)[A] and ".LBB_3" in isa_same.kernels(old)[A]
    assert isa_same.compare(old, new) == (True, 2, [], [], [])
    # (and the two kernels are not each other: the comparison is by symbol)
    assert isa_same.kernels(old)[A] != isa_same.kernels(old)[B]


def test_label_comment_column_does_not_count(isa_same):
    """The printer pads a block label's comment to a fixed column: a function number with one more digit leaves one blank fewer."""
    old = listing(kernel(A, 9), kernel(B, 99))
    new = listing(kernel(A, 10).replace(".LBB10_1:  ", ".LBB10_1: "), kernel(B, 100).replace(".LBB100_1:  ", ".LBB100_1: "))
    assert ".LBB10_1:   " in new and ".LBB10_1:" + " " * 31 + ";" in new and ".LBB9_1:" + " " * 32 + ";" in old
    assert isa_same.compare(old, new) == (True, 2, [], [], [])
    # (blanks elsewhere still count: an instruction's operands are not a label's comment)
    assert isa_same.compare(old, listing(kernel(A, 9).replace("v0, v0, v1", "v0,  v0, v1"), kernel(B, 99))) == (False, 2, [A], [], [])


def test_one_changed_operand_names_its_kernel(isa_same):
    old = listing(kernel(A, 0), kernel(B, 1))
    assert isa_same.compare(old, listing(kernel(A, 0), kernel(B, 1, operand="v3"))) == (False, 2, [B], [], [])
    # ... and so does a descriptor that differs while the code is the same
    assert isa_same.compare(old, listing(kernel(A, 0, vgprs=16), kernel(B, 1))) == (False, 2, [A], [], [])


def test_missing_kernel(isa_same):
    old = listing(kernel(A, 0), kernel(B, 1))
    assert isa_same.compare(old, listing(kernel(A, 0))) == (False, 1, [], [B], [])
    assert isa_same.compare(listing(kernel(A, 0)), old) == (False, 1, [], [], [B])
    assert isa_same.compare(listing(), listing())[0] is False   # (nothing to compare is not "equal")


def test_command_line(isa_same, tmp_path, capsys):
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(listing(kernel(A, 0), kernel(B, 1)))
    new.write_text(listing(kernel(B, 0), kernel(A, 1)))
    assert isa_same.main(["isa_same.py", str(old), str(new)]) == 0
    assert "EQUAL — 2 kernels" in capsys.readouterr().out
    new.write_text(listing(kernel(B, 0, operand="v3"), kernel(A, 1)))
    assert isa_same.main(["isa_same.py", str(old), str(new)]) == 1
    out = capsys.readouterr().out
    assert "differs: " + B in out and "differs: " + A not in out and "DIFFERENT — 1 kernels differ" in out
