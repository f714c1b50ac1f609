"""The edit-profile kernel (hit_edit.hip; DESIGN.md §4e "Edit profiles"), from one device-only compile of its
translation unit for gfx950: the compiler's kernel-resource-usage remarks.

The edit kernel uses no scratch -- the alignment's seven mismatch masks and its packed rows stay in registers,
no array is indexed dynamically -- and spills no VGPR, and its LDS -- the chunk's work list, which the remarks
report, and the word column's histogram, which the launch sizes for its k: 32 k-mers x (12 k | 1) words, at
most 49280 bytes at k = 32 (hit_edit.hip ep_hist_bytes, held to the same bound there by a static_assert) -- is
at most half of a CU's 160 KiB, so two workgroups are resident on a CU at any k.  Nothing else about the
assembly is asserted."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CU_LDS = 160 * 1024
HIST_MAX = 4 * 32 * ((12 * 32) | 1)  # the dynamic part at the largest k


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel name: {remark: value}} of every kernel of hit_edit.hip."""
    out = str(tmp_path_factory.mktemp("asm") / "hit_edit.s")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hit_edit.hip"), "-o", out, "-Rpass-analysis=kernel-resource-usage"],
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
    return {name: u for name, u in found.items() if "edit" in name}


def test_no_scratch_no_spills_and_half_a_cus_lds(usage):
    assert usage, "no edit kernel in hit_edit.hip"
    assert HIST_MAX == 49280
    for name, u in usage.items():
        print(name, u)
        assert u["ScratchSize [bytes/lane]"] == 0, name
        assert u["VGPRs Spill"] == 0, name
        assert 0 < u["LDS Size [bytes/block]"] + HIST_MAX <= CU_LDS // 2, name
