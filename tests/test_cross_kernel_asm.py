"""The cross co-occurrence product kernel (hit_cross.hip; DESIGN.md §4e "Cross co-occurrence"), from one
device-only compile of its translation unit: the compiler's kernel-resource-usage remarks and the assembly.

The kernel uses no scratch and spills no VGPR; its occupancy is the one its __launch_bounds__ declares
(hit_cross.h CX_WAVES_PER_SIMD, read from the header by a small host program); its inner product is the
popcount form, v_bcnt_u32_b32."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
KERNEL = "hit_cross_product_kernel"

DECLARED_SRC = """
#include <cstdio>
#include "hit_cross.h"
int main() {
    std::printf("%d\\n", acamd::bs::CX_WAVES_PER_SIMD);
    return 0;
}
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly text, {remark: value} of the product kernel) of hit_cross.hip."""
    out = str(tmp_path_factory.mktemp("asm") / "hit_cross.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hit_cross.hip"), "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                       check=True, capture_output=True, text=True)
    usage, cur = {}, False
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = KERNEL in m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and cur:
            usage[m.group(1).strip()] = int(m.group(2))
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
    print(usage)
    assert usage["ScratchSize [bytes/lane]"] == 0
    assert usage["VGPRs Spill"] == 0


def test_declared_residency_is_the_compilers_occupancy(compiled, declared):
    _, usage = compiled
    occ = usage["Occupancy [waves/SIMD]"]
    print(f"declared {declared}, occupancy {occ}")
    assert occ == declared


def test_the_product_is_the_popcount_form(compiled):
    text, _ = compiled
    funcs = [f for f in re.split(r"\n(?=_Z\w+:)", text) if f.startswith("_Z") and KERNEL in f.split(":")[0]]
    assert len(funcs) == 1
    body = funcs[0].split(".Lfunc_end")[0]
    n = len(re.findall(r"^\s+v_bcnt_u32_b32", body, flags=re.M))
    print(f"v_bcnt_u32_b32 in the product kernel: {n}")
    assert n >= 16
