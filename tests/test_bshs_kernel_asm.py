"""The staged hits-writing and hits-and-positions families of the bit-sliced count kernels (bshs_count.hip,
bsps_count.hip: bs_count.inc's body with STAGED and HITS, and POS, on; DESIGN.md §4e "Hits from the jobs
stage"), from one compile of each translation unit: the assembly, and the compiler's kernel-resource-usage
remarks.

Residency: bs_waves_per_simd(family, K) of the two staged families (wm_count.h) is what __launch_bounds__ and
the LDS allocation declare and what the host assumes when it sizes a launch; for every listed k and both row
counts it equals the occupancy the compiler reports.

Op budget, for K = 16, 22 and 32: the block of 4 bases -- one copy of the NFA code -- stays within the budget
its plain twin is held to (tests/test_bsh_kernel_asm.py: the counting kernels' op bounds;
tests/test_bsp_kernel_asm.py: the hits kernel's VALU count plus the per-base accumulation and the planes),
reads the table in ceil(K / 4) quads per base, and holds no scratch, buffer or global access.  Nothing else
about the instruction stream is checked."""
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
FAMILIES = ("bshs", "bsps")

DECLARED_SRC = """
#include <cstdio>
#include "bs_nfa.h"
#include "wm_count.h"
int main() {
#define AC_WAVES(KK, POS, E) acamd::bs_waves_per_simd(acamd::bs_family(true, true, POS, E), KK)
#define AC_SHOW(KK) std::printf("%d %d %d %d %d\\n", KK, AC_WAVES(KK, false, 2), AC_WAVES(KK, false, 3), \\
                                AC_WAVES(KK, true, 2), AC_WAVES(KK, true, 3));
    AC_BS_K_LIST(AC_SHOW)
    return 0;
}
"""


def name_of(fam, k=r"(\d+)", rows="([34])"):
    return rf"_ZN5acamd17{fam}_count_kernelILi{k}ELi{rows}E"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{family: (assembly text, {(K, R): occupancy})} of the two families' instantiations."""
    d = tmp_path_factory.mktemp("asm")
    procs = {}
    for fam in FAMILIES:
        out = str(d / f"{fam}_count.s")
        procs[fam] = (out, subprocess.Popen(
            [os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-mllvm",
             "-amdgpu-atomic-optimizer-strategy=None", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "--cuda-device-only", "-S", os.path.join(CSRC, f"{fam}_count.hip"), "-o", out,
             "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = {}
    for fam, (out, p) in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err[-3000:]
        occ, cur = {}, None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                k = re.match(name_of(fam), m.group(1))
                cur = (int(k.group(1)), int(k.group(2))) if k else None
                continue
            m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
            if m and cur is not None:
                occ[cur] = int(m.group(1))
        res[fam] = (open(out).read(), occ)
    return res


@pytest.fixture(scope="module")
def declared(tmp_path_factory):
    """{family: {(K, R): waves per SIMD}} from a host program that includes the kernels' header."""
    d = tmp_path_factory.mktemp("decl")
    src, exe = str(d / "declared.cpp"), str(d / "declared")
    with open(src, "w") as fh:
        fh.write(DECLARED_SRC)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    table = {"bshs": {}, "bsps": {}}
    for ln in out.splitlines():
        k, h3, h4, p3, p4 = (int(x) for x in ln.split())
        table["bshs"][(k, 3)], table["bshs"][(k, 4)] = h3, h4
        table["bsps"][(k, 3)], table["bsps"][(k, 4)] = p3, p4
    return table


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_declared_residency_is_the_compilers_occupancy(compiled, declared, fam):
    occ, decl = compiled[fam][1], declared[fam]
    assert sorted(decl) == sorted((k, r) for k in LISTED_K for r in (3, 4))
    assert sorted(occ) == sorted(decl)
    for key in sorted(decl):
        print(f"{fam} K {key[0]} R {key[1]}: declared {decl[key]}, occupancy {occ[key]}")
        assert occ[key] == decl[key], key


def nfa_block(text, fam, k, rows):
    """The one basic block (a list of mnemonics) of the family's kernel <k, rows> that holds the NFA code."""
    name = name_of(fam, k, rows)
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if re.match(name, f)]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    blocks = [[ln.split()[0] for ln in b.split("\n")[1:] if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
              for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body)]
    nfa = [b for b in blocks if sum(1 for i in b if i.startswith("v_bitop3_b32")) >= 4 * k - 8]  # a base's rows 1 and 2
    assert len(nfa) == 1, "one copy of the NFA code"
    return nfa[0]


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("k", ASM_K)
def test_the_nfa_blocks_stay_within_their_twins_budget(compiled, k, rows):
    count = lambda b, m: sum(1 for i in b if i.startswith(m))  # noqa: E731
    h = nfa_block(compiled["bshs"][0], "bshs", k, rows)
    p = nfa_block(compiled["bsps"][0], "bsps", k, rows)
    ors, bitops = count(h, "v_or_b32"), count(h, "v_bitop3_b32")
    print(f"K {k} R {rows}, per block of {BASES} bases: hits v_or_b32 {ors}, v_bitop3_b32 {bitops}, all VALU {count(h, 'v_')}; "
          f"positions all VALU {count(p, 'v_')}")
    if rows == 3:  # tests/test_bs_kernel_k_asm.py's bound
        assert ors + bitops <= BASES * ((k - 1) + (4 * k - 6) + 1.5 + 2)
    else:  # tests/test_bs3_kernel_asm.py's
        assert ors + bitops <= BASES * ((k - 1) + 2 * (3 * k - 6) + 2 + 2)
    # tests/test_bsp_kernel_asm.py's: the hits kernel's block plus the per-base accumulation and the planes
    assert count(p, "v_") - count(h, "v_") <= BASES * (1.5 * rows + 8) + 8
    for b in (h, p):
        assert count(b, "ds_read_b128") == BASES * -(-k // 4)
        assert not any(i.startswith(("scratch_", "buffer_", "global_")) for i in b)
