"""The flank-profile kernel (hit_flank.hip; DESIGN.md §4e "Flank profiles"), from one device-only compile of
its translation unit for gfx950: the compiler's kernel-resource-usage remarks.

The flank kernels use no scratch and spill no VGPR, and their LDS -- the chunk's work list, which the remarks
report, and the tile's histogram, which the launch sizes for its depth: 2 sides x 32 k-mers x (5 D | 1) words, at
most 41216 bytes at D = 32 (hit_flank.hip fl_hist_bytes, held to the same bound there by a static_assert) -- is
at most half of a CU's 160 KiB, so two workgroups are resident on a CU at any depth.  Nothing else about the
assembly is asserted."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CU_LDS = 160 * 1024
HIST_MAX = 4 * 2 * 32 * ((5 * 32) | 1)  # the dynamic part at the largest depth


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel name: {remark: value}} of every kernel of hit_flank.hip."""
    out = str(tmp_path_factory.mktemp("asm") / "hit_flank.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hit_flank.hip"), "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                       check=True, capture_output=True, text=True)
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = found.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {name: u for name, u in found.items() if "flank" in name}


def test_no_scratch_no_spills_and_half_a_cus_lds(usage):
    assert usage, "no flank kernel in hit_flank.hip"
    for name, u in usage.items():
        print(name, u)
        assert u["ScratchSize [bytes/lane]"] == 0, name
        assert u["VGPRs Spill"] == 0, name
        assert 0 < u["LDS Size [bytes/block]"] + HIST_MAX <= CU_LDS // 2, name
