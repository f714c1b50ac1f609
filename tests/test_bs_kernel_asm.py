"""The per-base op budget of the bit-sliced count kernel's NFA step (bs_nfa.h / bs_count.inc), from
the compiler's assembly of the plain K = 16 kernel: one more row of tests/test_generated_blocks.py's
table, for code that is plain C++ instead of generated inline asm.

The kernel holds one copy of the NFA code, a block of 4 bases (bs_block4).  Per base the transposed
recurrence is 15 v_or_b32 (row 0) and 58 three-input ops (rows 1 and 2: (a|b)&c, then a&b&c; two of
the 58 have a constant-zero input and come out as plain v_and_b32), plus 1.5 v_bitop3_b32 of hit
accumulation (bases go in pairs): 74.5, against the word-parallel kernel's 9.5 per base for 2
candidates -- 2.3 against 4.75 per candidate and base.  The lane's table address (its character from
the 2-bit code and the N bit) is 4 more ops per base, two of which the compiler may also emit as
v_or_b32 / v_bitop3_b32.  Only those two mnemonics are counted."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
K = 16
BASES = 4  # per block (bs_block4)


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    """Basic blocks (lists of mnemonics) of bs_count_kernel<16, false>."""
    out = str(tmp_path_factory.mktemp("asm") / "wm_count.s")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                    "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "--cuda-device-only", "-S", os.path.join(CSRC, "wm_count.hip"), "-o", out], check=True)
    text = open(out).read()
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if f.startswith("_ZN5acamd15bs_count_kernelILi16ELb0E")]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    out = []
    for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body):
        out.append([ln.split()[0] for ln in b.split("\n")[1:]
                    if ln.startswith("\t") and not ln.strip().startswith((".", ";"))])
    return out


def test_one_copy_of_the_nfa_and_its_op_budget(blocks):
    count = lambda b, m: sum(1 for i in b if i.startswith(m))  # noqa: E731
    nfa = [b for b in blocks if count(b, "v_bitop3_b32") >= 56]  # a base's rows 1 and 2
    assert len(nfa) == 1, "one copy of the NFA code"
    b = nfa[0]
    ors, bitops = count(b, "v_or_b32"), count(b, "v_bitop3_b32")
    print(f"per block of {BASES} bases: v_or_b32 {ors}, v_bitop3_b32 {bitops}, all VALU {count(b, 'v_')}")
    # rows 1-2 (56 with two live inputs besides nE) + hits (1.5), and row 0's ORs: nothing dropped ...
    assert bitops >= BASES * (56 + 1.5) and ors >= BASES * (K - 1)
    # ... and the budget: 74.5 NFA ops per base, and at most 2 of the 4 address ops in these mnemonics
    assert ors + bitops <= BASES * (74.5 + 2)
    # K / 4 table reads per base, 16 bytes each, and no scratch access inside the per-base code
    assert count(b, "ds_read_b128") == BASES * K // 4
    assert not any(i.startswith(("scratch_", "buffer_")) for i in b)
