"""The co-occurrence kernels (hit_cooc.hip; DESIGN.md §4e "Co-occurrence"), from one device-only compile of their
translation unit: the compiler's kernel-resource-usage remarks and the assembly.

No kernel of the file uses scratch or spills a VGPR.  The product kernel's occupancy is the one its launch
rule assumes (hit_cooc.h CO_WAVES_PER_SIMD: what __launch_bounds__ declares and co_splits sizes a launch's
workgroups by), read from the header by a small host program.  Its inner product is the popcount form:
v_bcnt_u32_b32, whose add operand carries the sum."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
KERNELS = ("hit_cooc_transpose_kernel", "hit_cooc_product_kernel", "hit_window_counts_kernel")

DECLARED_SRC = """
#include <cstdio>
#include "hit_cooc.h"
int main() {
    std::printf("%d\\n", acamd::bs::CO_WAVES_PER_SIMD);
    return 0;
}
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly text, {kernel: {remark: value}}) of hit_cooc.hip."""
    out = str(tmp_path_factory.mktemp("asm") / "hit_cooc.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hit_cooc.hip"), "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                       check=True, capture_output=True, text=True)
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = next((k for k in KERNELS if k in m.group(1)), None)
            if cur:
                usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = int(m.group(2))
    return open(out).read(), usage


@pytest.fixture(scope="module")
def declared(tmp_path_factory):
    d = tmp_path_factory.mktemp("decl")
    src, exe = str(d / "declared.cpp"), str(d / "declared")
    with open(src, "w") as fh:
        fh.write(DECLARED_SRC)
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, src, "-o", exe], check=True)
    return int(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout)


def test_no_scratch_and_no_spills(compiled):
    _, usage = compiled
    assert sorted(usage) == sorted(KERNELS)
    for k in KERNELS:
        print(k, usage[k])
        assert usage[k]["ScratchSize [bytes/lane]"] == 0, k
        assert usage[k]["VGPRs Spill"] == 0, k


def test_declared_residency_is_the_compilers_occupancy(compiled, declared):
    _, usage = compiled
    occ = usage["hit_cooc_product_kernel"]["Occupancy [waves/SIMD]"]
    print(f"declared {declared}, occupancy {occ}")
    assert occ == declared


def test_the_product_is_the_popcount_form(compiled):
    text, _ = compiled
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if "hit_cooc_product_kernel" in f.split(":")[0]]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    n = len(re.findall(r"^\s+v_bcnt_u32_b32", body, flags=re.M))
    print(f"v_bcnt_u32_b32 in the product kernel: {n}")
    assert n >= 16
