"""The plan of a jobs-stage launch (approx_counter_amd/csrc/stage_plan.cpp) on the CPU: how
ac_error_count_jobs cuts a call's windows into packing tasks and where every array lies in the
staging block that the host stage fills and the count kernel reads.  tools/stage_plan_dump.cpp is
built with g++ under the address and undefined-behaviour sanitizers and run as a child process; what
it planned is compared with the layout rules restated here from DESIGN.md §4c/§4d and the comments
of stage_plan.h, wm_count.h and nrec.h -- not transcribed from the C++."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

MAX_JOBS = 4
NO_ULEN = 0xFFFFFFFF
CHUNK = 4096  # bytes of a staging chunk
ALL_AHEAD = 2  # AC_TESTING_ALL_AHEAD
PLAN_SCALARS = ["early", "tag", "total_w", "off_err", "total", "off_gerr", "n_gerr", "pre", "tickets"]
PLAN_PER_JOB = ["lo", "hi", "n_bases", "no_bases", "off_kmers", "off_codes", "off_nmask", "off_start", "off_len",
                "off_counts", "ulen", "nrec", "region", "chunks", "codes_off"]
TASK_FIELDS = ["job", "w0", "w1", "first", "span", "first_len", "len_diff"]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "stage_plan_dump")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "stage_plan_dump.cpp"),
                    os.path.join(CSRC, "stage_plan.cpp"), os.path.join(CSRC, "host_pack.cpp"), "-o", exe], check=True)
    return exe


def job(n_kmers, lengths, lo=0, hi=None):
    return dict(n_kmers=n_kmers, lengths=list(lengths), lo=lo, hi=len(lengths) if hi is None else hi)


def run_plan(exe, tmp_path, jobs, k=16, early=True, have_d_counts=False, participants=1, min_task=1280, early_mode=1,
             hooks=0):
    src, dst = tmp_path / "case.bin", tmp_path / "plan.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<7IQ", k, early, have_d_counts, participants, early_mode, hooks, len(jobs), min_task))
        for b in jobs:
            fh.write(struct.pack("<4I", b["n_kmers"], len(b["lengths"]), b["lo"], b["hi"]))
            fh.write(struct.pack(f"<{len(b['lengths'])}I", *b["lengths"]))
    subprocess.run([exe, "plan", str(src), str(dst)], check=True, timeout=60)
    words = list(struct.unpack(f"<{os.path.getsize(dst) // 8}Q", open(dst, "rb").read()))
    got = {name: words.pop(0) for name in PLAN_SCALARS}
    for name in PLAN_PER_JOB:
        got[name], words = words[:MAX_JOBS], words[MAX_JOBS:]
    n_tasks = words.pop(0)
    assert len(words) == n_tasks * len(TASK_FIELDS)
    got["tasks"] = [dict(zip(TASK_FIELDS, words[i * 7:(i + 1) * 7])) for i in range(n_tasks)]
    return got


# ---- the rules, restated --------------------------------------------------------------------------

def up(x, a):
    return (x + a - 1) // a * a


def nrec_bits(L):  # nrec.h: record bits of equal windows of L bases, 0 = no room
    S = up(L, 32)
    R = 2 * min(S - L, 16)
    return 0 if (L == 0 or L > 256 or R < 3 + (7 if S <= 128 else 8)) else R


def cands_per_staged_wave(k):  # wm_count.h: 64 lanes x P candidates per lane word x lane words
    P = min(32 // k, 4)
    return 64 * P * (2 if P in (1, 2) else 1)


def expect_plan(jobs, k=16, early=True, have_d_counts=False, early_mode=1, hooks=0):
    """The staging block of DESIGN.md §4c: per job k-mers | codes | N bitmap | starts | lengths, then
    the error word, every job's counts and the tagged launch's group words, each at a 256-byte
    boundary; an early launch pads the k-mers to whole chunks."""
    n = len(jobs)
    e = {name: [0] * MAX_JOBS for name in PLAN_PER_JOB}
    tag = early and not have_d_counts
    off = 0
    for j, b in enumerate(jobs):
        lens = b["lengths"][b["lo"]:b["hi"]] if b["n_kmers"] else []  # a job without candidates sends no windows
        bases = sum(up(l, 32) for l in lens)
        e["lo"][j], e["hi"][j] = b["lo"], b["hi"]
        e["no_bases"][j] = int(bases == 0)
        e["n_bases"][j] = max(32, bases)
        e["ulen"][j] = lens[0] if lens and len(set(lens)) == 1 else NO_ULEN
        e["nrec"][j] = int(e["ulen"][j] != NO_ULEN and nrec_bits(e["ulen"][j]) != 0)
        e["off_kmers"][j] = off
        off = off + up(8 * b["n_kmers"], CHUNK) if early else up(off + 8 * b["n_kmers"], 256)
        for name, size in (("off_codes", e["n_bases"][j] // 4), ("off_nmask", e["n_bases"][j] // 8),
                           ("off_start", 8 * len(lens)), ("off_len", 4 * len(lens))):
            e[name][j] = off
            off = up(off + size, 256)
    e["off_err"] = off
    off = up(off + 4, 256)
    for j, b in enumerate(jobs):
        e["off_counts"][j] = off
        off = up(off + (8 if tag else 4) * b["n_kmers"], 256)
    e["off_gerr"] = off
    e["n_gerr"] = 0
    if tag:  # one word per candidate group of the jobs that have work
        e["n_gerr"] = sum(-(-b["n_kmers"] // cands_per_staged_wave(k)) for b in jobs if b["n_kmers"] and b["hi"] > b["lo"])
        off = up(off + 8 * e["n_gerr"], 256)
    e["total"] = off
    e["total_w"] = sum(b["hi"] - b["lo"] for b in jobs if b["n_kmers"])
    if early and off >= 1 << 31:  # the early launch counts a block's bytes in 31 bits
        early = tag = False
    e["early"], e["tag"] = int(early), int(tag)
    e["pre"] = e["tickets"] = 0
    if early:  # a job's region: to its descriptors when its windows are equal, else all of it
        e["pre"] = n if hooks & ALL_AHEAD else 1 if (early_mode == 2 and n > 1) else 0
        for j in range(n):
            end = e["off_start"][j] if e["ulen"][j] != NO_ULEN else (e["off_kmers"][j + 1] if j + 1 < n else e["off_err"])
            e["region"][j] = end - e["off_kmers"][j]
            e["chunks"][j] = 0 if j < e["pre"] else -(-e["region"][j] // CHUNK)
            e["codes_off"][j] = e["off_codes"][j] - e["off_kmers"][j]
            e["tickets"] += e["chunks"][j] + 1 if e["chunks"][j] else 0
    return e


def expect_tasks(jobs, early, participants=1, min_task=1280):
    total_w = sum(b["hi"] - b["lo"] for b in jobs if b["n_kmers"])
    per = max(min_task, min(max(2048, min_task) if early else 65536, total_w // (4 * participants) + 1))
    tasks = []
    for j, b in enumerate(jobs):
        if not b["n_kmers"]:
            continue
        first = 0
        for w0 in range(b["lo"], b["hi"], per):
            lens = b["lengths"][w0:min(b["hi"], w0 + per)]
            span = sum(up(l, 32) for l in lens)
            tasks.append(dict(job=j, w0=w0, w1=w0 + len(lens), first=first, span=span, first_len=lens[0]))
            first += span
    return tasks


def check(got, jobs, **kw):
    """The plan against the restated rules, and the invariants every plan keeps."""
    want = expect_plan(jobs, **{k: v for k, v in kw.items() if k not in ("participants", "min_task")})
    for name in PLAN_SCALARS + PLAN_PER_JOB:
        assert got[name] == want[name], (name, got[name], want[name])
    want_tasks = expect_tasks(jobs, kw.get("early", True), kw.get("participants", 1), kw.get("min_task", 1280))
    assert len(got["tasks"]) == len(want_tasks)
    for g, w in zip(got["tasks"], want_tasks):
        assert {f: g[f] for f in w} == w
        lens = jobs[g["job"]]["lengths"][g["w0"]:g["w1"]]
        assert (g["len_diff"] == 0) == (len(set(lens)) == 1)
    # invariants: every offset 256-aligned, the sections disjoint and in order, total = the last one's end
    n = len(jobs)
    sections = []
    for j in range(n):
        nw = jobs[j]["hi"] - jobs[j]["lo"] if jobs[j]["n_kmers"] else 0
        sections += [(got["off_kmers"][j], 8 * jobs[j]["n_kmers"]), (got["off_codes"][j], got["n_bases"][j] // 4),
                     (got["off_nmask"][j], got["n_bases"][j] // 8), (got["off_start"][j], 8 * nw), (got["off_len"][j], 4 * nw)]
    sections.append((got["off_err"], 4))
    # (a launch that fell back from the early path keeps the block planned for tagged counts)
    count_bytes = 8 if (kw.get("early", True) and not kw.get("have_d_counts", False)) else 4
    sections += [(got["off_counts"][j], count_bytes * jobs[j]["n_kmers"]) for j in range(n)]
    sections.append((got["off_gerr"], 8 * got["n_gerr"]))
    end = 0
    for off, size in sections:
        assert off % 256 == 0 and off >= end, (off, end)
        end = off + size
    assert got["total"] % 256 == 0 and got["total"] == up(end, 256)
    assert got["n_bases"][:n] == [max(32, b) for b in got["n_bases"][:n]] and all(b % 32 == 0 for b in got["n_bases"])
    return want


TWO_ENDS = [job(3, [100] * 5), job(3, [101] * 5)]
MIXED = [job(3, [100, 100, 37, 100, 100]), job(3, [101] * 5)]


def test_two_equal_window_jobs_tagged(dump, tmp_path):
    got = run_plan(dump, tmp_path, TWO_ENDS)
    check(got, TWO_ENDS)
    assert got["early"] == 1 and got["tag"] == 1
    for j in range(2):
        assert got["off_codes"][j] - got["off_kmers"][j] == CHUNK  # the k-mers: one whole chunk
        assert got["n_bases"][j] == 640
        assert (got["off_nmask"][j] - got["off_codes"][j] == got["off_start"][j] - got["off_nmask"][j]
                == got["off_len"][j] - got["off_start"][j] == 256)
        assert got["chunks"][j] == -(-(got["off_start"][j] - got["off_kmers"][j]) // CHUNK) == 2
    assert got["off_kmers"][1] - got["off_len"][0] == 256
    assert got["off_counts"][1] - got["off_counts"][0] == 256 and got["off_gerr"] - got["off_counts"][1] == 256  # 24 B each
    assert cands_per_staged_wave(16) == 256 and got["n_gerr"] == 2
    assert got["ulen"][:2] == [100, 101] and got["nrec"][:2] == [int(nrec_bits(100) != 0), int(nrec_bits(101) != 0)] == [1, 1]
    assert got["pre"] == 0 and got["tickets"] == 6


def test_mixed_lengths_dma_untagged(dump, tmp_path):
    got = run_plan(dump, tmp_path, MIXED, early=False)
    check(got, MIXED, early=False)
    assert got["early"] == 0 and got["tag"] == 0 and got["n_gerr"] == 0
    assert got["ulen"][:2] == [NO_ULEN, 101] and got["nrec"][:2] == [0, 1]
    assert got["n_bases"][:2] == [576, 640]
    assert got["off_codes"][0] == 256 and got["off_kmers"][1] % CHUNK != 0  # k-mers 256-aligned, not chunk-aligned
    assert got["off_counts"][1] - got["off_counts"][0] == 256 and got["total"] - got["off_counts"][1] == 256  # 12 B each
    assert got["region"] == [0] * MAX_JOBS and got["chunks"] == [0] * MAX_JOBS  # (an early launch's only)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["mixed_first", "mixed_last"])
def test_mixed_lengths_region(dump, tmp_path, order):
    """An early launch into device counts (a submit: untagged).  A job of mixed lengths sends its
    descriptors: its region runs to the next job's k-mers, or to the error word for the last job."""
    jobs = [MIXED[order[0]], MIXED[order[1]]]
    got = run_plan(dump, tmp_path, jobs, have_d_counts=True)
    check(got, jobs, have_d_counts=True)
    m = order.index(0)
    assert got["early"] == 1 and got["tag"] == 0 and got["n_gerr"] == 0
    assert got["off_kmers"][m] + got["region"][m] == (got["off_kmers"][1] if m == 0 else got["off_err"])
    assert got["off_kmers"][1 - m] + got["region"][1 - m] == got["off_start"][1 - m]


def test_idle_jobs(dump, tmp_path):
    jobs = [job(0, [100] * 7), job(2, []), job(2, [50, 60])]
    got = run_plan(dump, tmp_path, jobs)
    check(got, jobs)
    assert [t["job"] for t in got["tasks"]] == [2]  # no candidates / no windows: no task
    assert got["off_len"][0] == got["off_start"][0] == got["off_kmers"][1]  # no windows of job 0 in the layout
    assert got["n_bases"][:3] == [32, 32, 128] and got["no_bases"][:3] == [1, 1, 0]
    assert got["ulen"][:3] == [NO_ULEN, NO_ULEN, NO_ULEN]
    assert got["n_gerr"] == 1 and got["total_w"] == 2


@pytest.mark.parametrize("early", [True, False], ids=["early", "dma"])
def test_task_cutting(dump, tmp_path, early):
    jobs = [job(4, [100] * 3000)]
    got = run_plan(dump, tmp_path, jobs, early=early)
    check(got, jobs, early=early)
    assert [(t["w0"], t["w1"]) for t in got["tasks"]] == [(0, 1280), (1280, 2560), (2560, 3000)]
    jobs = [job(4, [100] * 12000), job(4, [101] * 8000)]
    got = run_plan(dump, tmp_path, jobs, early=early)
    check(got, jobs, early=early)
    per = 2048 if early else 5001
    assert all(t["w1"] - t["w0"] == per or t["w1"] == jobs[t["job"]]["hi"] for t in got["tasks"])
    assert len(got["tasks"]) == -(-12000 // per) + -(-8000 // per)
    for j in range(2):  # a task's first image base: the earlier tasks' spans of its job
        first = 0
        for t in (t for t in got["tasks"] if t["job"] == j):
            assert t["first"] == first
            first += t["span"]
        assert first == got["n_bases"][j]


def test_part_ranges_and_participants(dump, tmp_path):
    """A part of a call (lo / hi inside the job) and a larger pool: the share of a task shrinks, not
    below the smallest task."""
    jobs = [job(3, [100] * 9000 + [37], lo=2000, hi=9001)]
    got = run_plan(dump, tmp_path, jobs, early=False, participants=4, min_task=300)
    check(got, jobs, early=False, participants=4, min_task=300)
    assert got["tasks"][0]["w0"] == 2000 and got["tasks"][0]["w1"] - 2000 == 7001 // 16 + 1
    assert got["ulen"][0] == NO_ULEN and got["tasks"][-1]["len_diff"] != 0


def test_jobs_sent_ahead(dump, tmp_path):
    got = run_plan(dump, tmp_path, TWO_ENDS, early_mode=2)
    check(got, TWO_ENDS, early_mode=2)
    assert got["pre"] == 1 and got["chunks"][:2] == [0, 2] and got["tickets"] == 3
    got = run_plan(dump, tmp_path, TWO_ENDS, hooks=ALL_AHEAD)
    check(got, TWO_ENDS, hooks=ALL_AHEAD)
    assert got["pre"] == 2 and got["chunks"][:2] == [0, 0] and got["tickets"] == 0


def test_two_gib_block_leaves_the_early_path(dump, tmp_path):
    jobs = [job(1 << 28, [100] * 5)]
    got = run_plan(dump, tmp_path, jobs)
    check(got, jobs)
    assert got["total"] >= 1 << 31 and got["early"] == 0 and got["tag"] == 0


def test_cuts(dump, tmp_path):
    src, dst = tmp_path / "cuts.bin", tmp_path / "cuts.out"
    totals = [(1 << 17) - 1, 1 << 17, 1 << 19]
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I10IdII3Q", 10, *([100] * 10), 0.5, 4, len(totals), *totals))
    subprocess.run([dump, "cuts", str(src), str(dst)], check=True, timeout=60)
    out = struct.unpack("<9I", open(dst, "rb").read())
    assert out[0] == 5
    assert list(out[1:6]) == [0, 3, 5, 8, 10]
    assert list(out[6:]) == [1, 2, 4]
