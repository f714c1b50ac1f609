"""The hits-writing family of the bit-sliced count kernels (bsh_count.hip: bs_count.inc's body with HITS on,
over three NFA rows for the edit budgets 0..2 and over four for budget 3; DESIGN.md §4e "Hit levels"), from
one compile of their translation unit: the assembly, and the compiler's kernel-resource-usage remarks.

Residency: bs_waves_per_simd(family, K) of the plain hits-writing family (wm_count.h) is what
__launch_bounds__ and the LDS allocation declare
and what the host assumes when it sizes a launch; for every listed k and both row counts it equals the
occupancy the compiler reports.

Op budget, for K = 16, 22 and 32: the hit words are stored where a row's masks become counts, outside the
block of 4 bases, so the block is the counting kernel's -- one copy of the NFA code, within the op budget
tests/test_bs_kernel_k_asm.py (three rows) and tests/test_bs3_kernel_asm.py (four) hold the counting
kernels to, the table read in ceil(K / 4) quads per base, and no scratch or buffer access inside it.  The
stores themselves are ordinary vector stores (global_store_dword), one per level."""
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
NAME = r"_ZN5acamd16bsh_count_kernelILi(\d+)ELi([34])E"

DECLARED_SRC = """
#include <cstdio>
#include "bs_nfa.h"
#include "wm_count.h"
int main() {
#define AC_WAVES(KK, E) acamd::bs_waves_per_simd(acamd::bs_family(false, true, false, E), KK)
#define AC_SHOW(KK) std::printf("%d %d %d\\n", KK, AC_WAVES(KK, 2), AC_WAVES(KK, 3));
    AC_BS_K_LIST(AC_SHOW)
    return 0;
}
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly text, {(K, R): occupancy}) of the bsh_count_kernel instantiations."""
    out = str(tmp_path_factory.mktemp("asm") / "bsh_count.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "bsh_count.hip"), "-o", out,
                        "-Rpass-analysis=kernel-resource-usage"], check=True, capture_output=True, text=True)
    occ, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.match(NAME, m.group(1))
            cur = (int(k.group(1)), int(k.group(2))) if k else None
            continue
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur is not None:
            occ[cur] = int(m.group(1))
    return open(out).read(), occ


@pytest.fixture(scope="module")
def declared(tmp_path_factory):
    """{(K, R): bs_waves_per_simd(family, K)} from a host program that includes the kernel's header."""
    d = tmp_path_factory.mktemp("decl")
    src, exe = str(d / "declared.cpp"), str(d / "declared")
    with open(src, "w") as fh:
        fh.write(DECLARED_SRC)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    table = {}
    for ln in out.splitlines():
        k, r3, r4 = (int(x) for x in ln.split())
        table[(k, 3)], table[(k, 4)] = r3, r4
    return table


def test_declared_residency_is_the_compilers_occupancy(compiled, declared):
    _, occ = compiled
    assert sorted(declared) == sorted((k, r) for k in LISTED_K for r in (3, 4))
    assert sorted(occ) == sorted(declared)
    for key in sorted(declared):
        print(f"K {key[0]} R {key[1]}: declared {declared[key]}, occupancy {occ[key]}")
        assert occ[key] == declared[key], key


def kernel_blocks(text, k, rows):
    """Basic blocks (lists of mnemonics) of bsh_count_kernel<k, rows>."""
    name = f"_ZN5acamd16bsh_count_kernelILi{k}ELi{rows}E"
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if f.startswith(name)]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    return [[ln.split()[0] for ln in b.split("\n")[1:] if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
            for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body)]


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("k", ASM_K)
def test_the_nfa_block_is_the_counting_kernels(compiled, k, rows):
    count = lambda b, m: sum(1 for i in b if i.startswith(m))  # noqa: E731
    blocks = kernel_blocks(compiled[0], k, rows)
    nfa = [b for b in blocks if count(b, "v_bitop3_b32") >= 4 * k - 8]  # at least a base's rows 1 and 2
    assert len(nfa) == 1, "one copy of the NFA code"
    b = nfa[0]
    ors, bitops = count(b, "v_or_b32"), count(b, "v_bitop3_b32")
    print(f"K {k} R {rows}, per block of {BASES} bases: v_or_b32 {ors}, v_bitop3_b32 {bitops}, "
          f"all VALU {count(b, 'v_')}, v_accvgpr {count(b, 'v_accvgpr')}, ds_read_b128 {count(b, 'ds_read_b128')}")
    assert ors >= BASES * (k - 1)
    if rows == 3:  # tests/test_bs_kernel_k_asm.py's bounds
        assert bitops >= BASES * (4 * k - 8 + 1.5)
        assert ors + bitops <= BASES * ((k - 1) + (4 * k - 6) + 1.5 + 2)
    else:  # tests/test_bs3_kernel_asm.py's
        assert bitops >= BASES * (2 * (3 * k - 6) - 3 + 2)
        assert ors + bitops <= BASES * ((k - 1) + 2 * (3 * k - 6) + 2 + 2)
    assert count(b, "ds_read_b128") == BASES * -(-k // 4)
    assert not any(i.startswith(("scratch_", "buffer_", "global_")) for i in b)
    # the hit words: vector stores outside the block, at least one per level
    stores = sum(count(x, "global_store_dword") for x in blocks)
    print(f"K {k} R {rows}: global_store_dword {stores}")
    assert stores >= rows
