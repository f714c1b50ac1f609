"""CPU tests of the hit levels and end positions from the jobs stage (ac_window_hits_jobs and its siblings;
DESIGN.md §4e "Hits from the jobs stage"): the exports and their Python mirror, and -- through
tools/jobs_hits_plan_check.cpp, a stand-alone program built here with the sanitizers on -- what the jobs
stage's planner answers when hits or positions are asked for: which launches it accepts, which it refuses and
in which words, and where the parts of a DMA-path call write their rows."""
import inspect
import os
import re
import subprocess

import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SYMBOLS = ["ac_window_hits_jobs", "ac_window_positions_jobs", "ac_window_hits_jobs_submit",
           "ac_window_positions_jobs_submit"]


# ---- the exports ----------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "approx_counter_amd.h")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"\bac_status {name}\(ac_ctx\* ctx, uint32_t k, const ac_job\* jobs, uint32_t n_jobs,", header), name
        assert hasattr(L, name), name
    assert "#define AC_ABI_VERSION 8" in header and L.ac_abi_version() == 8
    testing = open(os.path.join(ROOT, "include", "approx_counter_amd_testing.h")).read()
    assert "#define AC_TESTING_TWO_PARTS 16u" in testing


def test_null_ctx_is_rejected():
    L = _lib.load()
    for name, extra in zip(SYMBOLS, ((None,), (None, None), (None, None, None), (None, None, None, None))):
        assert getattr(L, name)(None, 16, None, 0, *extra) == _lib.AC_ERR_INVALID, name
        assert b"ctx" in L.ac_last_error(None)


def test_python_mirror():
    assert callable(ac.ApproxCounter.window_hits_jobs) and callable(ac.error_levels) and "error_levels" in ac.__all__
    p = inspect.signature(ac.ApproxCounter.window_hits_jobs).parameters
    assert list(p) == ["self", "k", "jobs", "positions"] and p["positions"].default is False
    p = inspect.signature(ac.ApproxCounter.submit_jobs).parameters
    assert p["hits"].default is None and p["positions"].default is None
    assert list(inspect.signature(ac.error_levels).parameters) == list(inspect.signature(ac.error_count).parameters)
    assert ac.error_levels([], []) == {}


# ---- the planner ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jobs_hits") / "jobs_hits_plan_check")
    subprocess.run(["g++"] + SANITIZE + ["-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                         os.path.join(ROOT, "tools", "jobs_hits_plan_check.cpp"),
                                         os.path.join(CSRC, "stage_plan.cpp"), os.path.join(CSRC, "host_pack.cpp"),
                                         "-o", exe], check=True)
    return exe


def plan(exe, E, k, *jobs, early=1, multi=0, pos=0, parts=1, **env):
    r = subprocess.run([exe, str(E), str(k), str(early), str(multi), str(pos), str(parts)] + list(jobs),
                       capture_output=True, text=True, timeout=60, check=True, env=dict(os.environ, **env))
    return r.stdout.strip().splitlines()


@pytest.mark.parametrize("early", [0, 1])
def test_plan_accepts(tool, early):
    """k = 16 and 22, E = 0..3, equal jobs of 100 and 101 bases, hits and positions: accepted, on the route
    asked for."""
    for k in (16, 22):
        for E in range(4):
            for pos in (0, 1):
                out = plan(tool, E, k, "40:100:37", "70:101:41", early=early, pos=pos)
                assert out[0] == f"part 0: ok early={early} tag={early}", (k, E, pos, out)
    # a job without k-mers or without windows is no work: it changes nothing, positions matrix or not
    assert plan(tool, 2, 16, "40:100:37", "5:100:0", "0:r:9", early=early, pos=2)[0].startswith("part 0: refused")
    assert plan(tool, 2, 16, "0:r:9", "5:300:0", "40:100:37", early=early, pos=1)[0].startswith("part 0: ok")


@pytest.mark.parametrize("early", [0, 1])
def test_plan_refuses_in_the_existing_words(tool, early):
    for pos in (0, 1):
        one = lambda *a, **kw: plan(tool, *a, early=early, pos=pos, **kw)[0]  # noqa: E731
        assert "refused: window hits need equal windows" in one(2, 16, "40:r:37") and "ragged" in one(2, 16, "40:r:37")
        assert "ragged" in one(2, 16, "40:100:37", "40:r:37")
        assert "1..256" in one(2, 22, "40:300:9") and "longer" in one(2, 22, "40:300:9")
        for k in (15, 17):
            assert "k = 16 or 18..32" in one(2, k, "40:100:37")
        assert "single-device" in one(2, 16, "40:100:37", multi=1)
        assert "AC_BITSLICE" in one(2, 16, "40:100:37", AC_BITSLICE="0")
        assert "max_errors must be 0..3" in one(4, 16, "40:100:37")
    out = plan(tool, 2, 16, "40:100:37", "70:101:41", early=early, pos=2)
    assert out[0] == "part 0: refused: window positions: pos[i] is NULL for a segment with work"


def test_part_rows(tool):
    """A job of 37 windows and 40 k-mers (2 words per row) in two parts is cut at 19: row offsets 0 and 19 x 2
    words, plane stride 37 x 2 in both; the parts' row ranges tile [0, n) without overlap, in two parts and four."""
    out = plan(tool, 2, 16, "40:100:37", early=0, parts=2)
    assert out == ["part 0: ok early=0 tag=0", "part 0 job 0: rows 0..19 row_off 0 plane 74 mat_windows 37",
                   "part 1: ok early=0 tag=0", "part 1 job 0: rows 19..37 row_off 38 plane 74 mat_windows 37"]
    for parts in (2, 4):
        for pos in (0, 1):
            out = plan(tool, 3, 22, "40:100:37", "300:101:70", "33:13:1", early=0, parts=parts, pos=pos)
            assert sum(ln.endswith("ok early=0 tag=0") for ln in out) == parts
            for j, (nk, nw) in enumerate(((40, 37), (300, 70), (33, 1))):
                rows = [re.match(rf"part (\d+) job {j}: rows (\d+)\.\.(\d+) row_off (\d+) plane (\d+) mat_windows (\d+)", ln)
                        for ln in out]
                rows = [tuple(int(x) for x in m.groups()) for m in rows if m]
                assert [r[0] for r in rows] == list(range(parts))
                words, at = (nk + 31) // 32, 0
                for _, lo, hi, off, plane, mat in rows:
                    assert lo == at and hi >= lo and off == lo * words and plane == nw * words and mat == nw
                    at = hi
                assert at == nw
