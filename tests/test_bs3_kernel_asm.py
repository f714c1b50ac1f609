"""The bit-sliced count kernels for an edit budget of 3 (bs3_count.hip: bs_count.inc's body over the four
NFA rows of bs_nfa_r.h; DESIGN.md §4e "Edit budget"), from one compile of their translation unit: the
assembly, and the compiler's kernel-resource-usage remarks.

Residency: bs_waves_per_simd(family, K) of the E = 3 counting family (wm_count.h) is what __launch_bounds__
and the LDS allocation declare
and what the host assumes when it sizes a launch; for every listed k, plain and staged, it equals the
occupancy the compiler reports.

Op budget, for K = 16, 22 and 32: the kernel has one copy of the NFA code, a block of 4 bases.  Per base
the recurrence is K - 1 v_or_b32 and 2 (3K - 6) three-input ops for rows 1..3 (three of them with a
constant-zero input: plain v_and_b32), plus 2 v_bitop3_b32 of hit accumulation (four levels, bases in
pairs); the lane's table address is 4 more ops per base, of which the compiler may emit 2 in these two
mnemonics -- the slack tests/test_bs_kernel_k_asm.py allows.  The table is read in ceil(K / 4) quads per
base, and nothing inside the block touches scratch."""
import os
import re
import subprocess

import pytest

from tests.test_bs_nfa_k import LISTED_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
BASES = 4  # per block (bs_block4)
ASM_K = [k for k in (16, 22, 32) if k in LISTED_K]
NAME = r"_ZN5acamd16bs3_count_kernelILi(\d+)ELb([01])E"

DECLARED_SRC = """
#include <cstdio>
#include "bs_nfa.h"
#include "wm_count.h"
int main() {
#define AC_SHOW(KK) std::printf("%d %d\\n", KK, acamd::bs_waves_per_simd(acamd::bs_family(false, false, false, 3), KK));
    AC_BS_K_LIST(AC_SHOW)
    return 0;
}
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly text, {(K, staged): occupancy}) of the bs3_count_kernel instantiations."""
    out = str(tmp_path_factory.mktemp("asm") / "bs3_count.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "bs3_count.hip"), "-o", out,
                        "-Rpass-analysis=kernel-resource-usage"], check=True, capture_output=True, text=True)
    occ, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.match(NAME, m.group(1))
            cur = (int(k.group(1)), k.group(2) == "1") if k else None
            continue
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur is not None:
            occ[cur] = int(m.group(1))
    return open(out).read(), occ


@pytest.fixture(scope="module")
def declared(tmp_path_factory):
    """{K: bs_waves_per_simd(family, K)} from a host program that includes the kernel's header."""
    d = tmp_path_factory.mktemp("decl")
    src, exe = str(d / "declared.cpp"), str(d / "declared")
    with open(src, "w") as fh:
        fh.write(DECLARED_SRC)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    return {int(a): int(b) for a, b in (ln.split() for ln in out.splitlines())}


def test_declared_residency_is_the_compilers_occupancy(compiled, declared):
    _, occ = compiled
    assert sorted(declared) == sorted(LISTED_K)
    assert sorted(occ) == sorted((k, s) for k in LISTED_K for s in (False, True))
    for k in LISTED_K:
        for staged in (False, True):
            print(f"K {k} staged {int(staged)}: declared {declared[k]}, occupancy {occ.get((k, staged))}")
            assert occ[(k, staged)] == declared[k], (k, staged)


def nfa_blocks(text, k, staged):
    """Basic blocks (lists of mnemonics) of bs3_count_kernel<k, staged>."""
    name = f"_ZN5acamd16bs3_count_kernelILi{k}ELb{int(staged)}E"
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if f.startswith(name)]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    return [[ln.split()[0] for ln in b.split("\n")[1:] if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
            for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body)]


@pytest.mark.parametrize("staged", [False, True], ids=["plain", "staged"])
@pytest.mark.parametrize("k", ASM_K)
def test_one_copy_of_the_nfa_and_its_op_budget(compiled, k, staged):
    count = lambda b, m: sum(1 for i in b if i.startswith(m))  # noqa: E731
    blocks = nfa_blocks(compiled[0], k, staged)
    nfa = [b for b in blocks if count(b, "v_bitop3_b32") >= 4 * k - 8]  # at least a base's rows 1 and 2
    assert len(nfa) == 1, "one copy of the NFA code"
    b = nfa[0]
    ors, bitops = count(b, "v_or_b32"), count(b, "v_bitop3_b32")
    print(f"K {k} staged {int(staged)}, per block of {BASES} bases: v_or_b32 {ors}, v_bitop3_b32 {bitops}, "
          f"all VALU {count(b, 'v_')}, v_accvgpr {count(b, 'v_accvgpr')}, ds_read_b128 {count(b, 'ds_read_b128')}")
    # nothing dropped: row 0's ORs; rows 1-3 with two live inputs besides nE, and the hits ...
    assert ors >= BASES * (k - 1)
    assert bitops >= BASES * (2 * (3 * k - 6) - 3 + 2)
    # ... and the budget: (K - 1) + 2 (3K - 6) + 2 per base, and at most 2 of the 4 address ops in these mnemonics
    assert ors + bitops <= BASES * ((k - 1) + 2 * (3 * k - 6) + 2 + 2)
    # ceil(K / 4) table reads per base, 16 bytes each, and no scratch access inside the per-base code
    assert count(b, "ds_read_b128") == BASES * -(-k // 4)
    assert not any(i.startswith(("scratch_", "buffer_")) for i in b)
