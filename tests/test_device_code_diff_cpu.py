"""tools/device_code_diff.py on two short disassembly texts: the parser and the comparer behind the "no kernel changed" proof of a refactor.
Equal texts pass (addresses and encodings may differ), one changed operand is reported under its kernel's name with the instruction, and a
kernel that only one side has is listed.  No compile, no GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_code_diff as dcd  # noqa: E402

# llvm-objdump -d of a gfx950 code object: a label per symbol, then "mnemonic operands // address: encoding words"
TEXT = """
a.o:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001000 <_Z6kernelPf>:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0                         // 000000001000: C0060000 00000000
\ts_waitcnt lgkmcnt(0)                                       // 000000001008: BF8CC07F
\tglobal_load_lds_dwordx4 v[2:3], off                        // 00000000100C: DDF48000 007F0002
\ts_waitcnt vmcnt(2)                                         // 000000001014: BF8C0F72
\ts_barrier                                                  // 000000001018: BF8A0000
\ts_endpgm                                                   // 00000000101C: BF810000

0000000000001100 <_Z5otherPf>:
\tv_mov_b32_e32 v0, 0                                        // 000000001100: 7E000280
\ts_endpgm                                                   // 000000001104: BF810000
"""


def test_parser_reads_both_kernels():
    code = dcd.kernel_code(TEXT)
    assert sorted(code) == ["_Z5otherPf", "_Z6kernelPf"]
    assert code["_Z6kernelPf"][3] == ("s_waitcnt", "vmcnt(2)")
    assert [len(v) for _, v in sorted(code.items())] == [2, 6]


def test_equal_texts_pass_whatever_their_addresses():
    moved = TEXT.replace("0000000010", "0000000020").replace("00000000000010", "00000000000020").replace("00000000000011", "00000000000021")
    assert moved != TEXT
    a, b = dcd.kernel_code(TEXT), dcd.kernel_code(moved)
    assert dcd.compare(a, b) == ([], [], ["_Z5otherPf", "_Z6kernelPf"], [])
    text, bad = dcd.report(a, b)
    assert bad == 0
    assert "kernel symbols: A 2, B 2" in text and "2 kernels compared, 2 identical" in text
    assert "only in A (0):" in text and "only in B (0):" in text and "DIFFERS" not in text


def test_a_changed_operand_is_reported_under_its_kernel():
    a, b = dcd.kernel_code(TEXT), dcd.kernel_code(TEXT.replace("vmcnt(2)", "vmcnt(0)"))
    only_a, only_b, common, differing = dcd.compare(a, b)
    assert (only_a, only_b, len(common)) == ([], [], 2)
    assert differing == [("_Z6kernelPf", 3, ("s_waitcnt", "vmcnt(2)"), ("s_waitcnt", "vmcnt(0)"))]
    text, bad = dcd.report(a, b, "parent", "this commit")
    assert bad == 1
    assert "2 kernels compared, 1 identical" in text
    assert "DIFFERS _Z6kernelPf" in text and "first at instruction 3" in text
    assert "parent: s_waitcnt vmcnt(2)" in text and "this commit: s_waitcnt vmcnt(0)" in text
    assert "_Z5otherPf" not in text


def test_a_shorter_kernel_differs_at_its_end():
    cut = TEXT.replace("\ts_barrier                                                  // 000000001018: BF8A0000\n", "")
    _, _, _, differing = dcd.compare(dcd.kernel_code(TEXT), dcd.kernel_code(cut))
    assert differing == [("_Z6kernelPf", 4, ("s_barrier", ""), ("s_endpgm", ""))]
    only_tail = {"k": [("s_nop", "0")]}, {"k": [("s_nop", "0"), ("s_endpgm", "")]}
    assert dcd.compare(*only_tail)[3] == [("k", 1, None, ("s_endpgm", ""))]
    assert "(end of kernel)" in dcd.report(*only_tail)[0]


def test_a_kernel_missing_on_one_side_is_listed():
    a = dcd.kernel_code(TEXT)
    b = dcd.kernel_code(TEXT[: TEXT.index("0000000000001100")])
    assert sorted(b) == ["_Z6kernelPf"]
    text, bad = dcd.report(a, b)
    assert bad == 1
    assert "only in A (1):\n  _Z5otherPf" in text and "only in B (0):" in text
    assert "1 kernels compared, 1 identical" in text
    text, bad = dcd.report(b, a)
    assert bad == 1 and "only in B (1):\n  _Z5otherPf" in text
