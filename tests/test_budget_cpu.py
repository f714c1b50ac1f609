"""The edit budget of the approximate count (ac_set_max_errors; DESIGN.md §4e "Edit budget") on the CPU.

Contract M1(E): count(kmer) = sum over windows of max(0, E + 1 - d(kmer, w)), E in 0..3, d the oracle's
semi-global Levenshtein distance (N matches nothing).  count_e below is the expected value of every
budget test, here and in tests/test_gpu_budget.py: d from the oracle's C symbol oracle_distance_dp with
cap = E + 1 (the Python oracle.distance caps at 3); at E = 2 it is pinned to oracle.count_myers.

Here: the NFA of R = E + 1 rows and the generalised bit-plane counters (bs_nfa_r.h) through
tools/bs_nfa_r_check.cpp, built with g++ under the address and undefined-behaviour sanitizers and run as
a child process; the two C-ABI symbols; the command line's checks; and the plan layer's refusals
(stage_plan.cpp budget_refusal through plan_stage, tools/budget_plan_check.cpp)."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.test_bs_nfa_k import LISTED_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# ---- expected values ------------------------------------------------------------------------------

def distances(k, kmers, windows, cap):
    """min(d(kmer, window), cap) for every pair, from the oracle's plain DP: an (n_kmers, n_windows) array.
    `windows`: strings, or a 2-D Dna5 array of equal windows."""
    L = oracle.lib()
    p8 = ctypes.POINTER(ctypes.c_uint8)
    texts = [np.ascontiguousarray(oracle.encode_dna5(w)) for w in windows]
    d = np.zeros((len(kmers), len(texts)), np.int64)
    one = np.zeros(1, np.uint8)
    for j, t in enumerate(texts):
        buf = (t if t.size else one).ctypes.data_as(p8)
        for i, km in enumerate(kmers):
            d[i, j] = L.oracle_distance_dp(int(km), k, buf, int(t.size), cap)
    assert (d >= 0).all()
    return d


def count_e(E, k, kmers, windows):
    """M1(E): sum over the windows of max(0, E + 1 - min(d, E + 1)), uint64 per k-mer."""
    d = np.minimum(distances(k, kmers, windows, E + 1), E + 1)
    return (E + 1 - d).sum(axis=1).astype(np.uint64)


def counts_from(d4, E):
    """count_e for E <= 3 from distances capped at 4 (one DP pass for every budget)."""
    return np.maximum(0, E + 1 - d4).sum(axis=1).astype(np.uint64)


@pytest.mark.parametrize("k", [16, 22, 32])
def test_count_e_at_two_is_the_oracle(k):
    """The helper at E = 2 equals oracle.count_myers (ragged windows, N, empty and short windows); and
    the planted cases hold windows at distance exactly 3, so E = 3 differs from E = 2."""
    km, w = cases.planted_case(900 + k, k, 37, 60, win_len=(k - 4, 110), p_n=0.01)
    w += ["", "A", "N" * k, cases.kmer_string(km[0], k)]
    np.testing.assert_array_equal(count_e(2, k, km, w), oracle.count_myers(k, km, w))
    np.testing.assert_array_equal(counts_from(distances(k, km, w, 4), 2), oracle.count_myers(k, km, w))
    assert (count_e(3, k, km, w) != count_e(2, k, km, w)).any()
    assert (count_e(1, k, km, w) != count_e(2, k, km, w)).any() and count_e(0, k, km, w).any()


# ---- the NFA of R rows and the plane counters ---------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bsr") / "bs_nfa_r_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "bs_nfa_r_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_case(path, k, kmers, windows):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<3I", k, len(kmers), len(windows)))
        fh.write(struct.pack(f"<{len(kmers)}Q", *kmers))
        for w in windows:
            fh.write(struct.pack("<I", len(w)))
            fh.write(bytes("ACGT".index(c) if c in "ACGT" else 4 for c in w))


def run_count(exe, tmp_path, form, E, k, kmers, windows):
    src, dst = tmp_path / "case.bin", tmp_path / f"out_{form}_{E}.bin"
    write_case(src, k, kmers, windows)
    subprocess.run([exe, "count", form, str(E), str(src), str(dst)], check=True, timeout=120)
    out = np.fromfile(dst, dtype=np.uint32)
    assert len(out) == len(kmers) + 1
    return out[:-1].astype(np.uint64), int(out[-1])


def nfa_case(k):
    """40 candidates (a partial second block); ragged windows of k - 4 .. 60 bases, most with a planted
    occurrence of 0..3 edits, 2 % N; every length 1 .. k + 4 as a candidate's prefix or the candidate with
    a few more bases, unchanged and with one base changed; all-N windows and an N inside an occurrence."""
    rng = random.Random(k)
    km, w = cases.planted_case(700 + k, k, 40, 40, win_len=(k - 4, 60), p_n=0.02)
    for L in range(1, k + 5):
        s = cases.kmer_string(km[L % len(km)], k) + cases.rand_seq(rng, 4)
        w.append(s[:L])
        p = rng.randrange(L)
        w.append(s[:p] + rng.choice([c for c in "ACGT" if c != s[p]]) + s[p + 1:L])
    s = cases.kmer_string(km[3], k)
    w += ["N" * (k + 3), "N", s[:5] + "N" + s[6:], "N" + s, s + "N", s[:7] + "N" + s[7:]]
    return km, w


@pytest.mark.parametrize("k", LISTED_K)
def test_nfa_counts_at_every_budget(tool, tmp_path, k):
    """Every listed K x E in {0, 1, 3} (and 2) against count_e, in both forms: what the kernels run (three
    rows and the levels chosen at vc_add_e for E <= 2, four rows for E = 3) and E + 1 generic rows."""
    km, w = nfa_case(k)
    d4 = distances(k, km, w, 4)
    assert (d4 == 3).any() and (d4 == 0).any()
    for E in (0, 1, 2, 3):
        want = counts_from(d4, E)
        for form in ("kernel", "rows"):
            got, _ = run_count(tool, tmp_path, form, E, k, km, w)
            np.testing.assert_array_equal(got, want, err_msg=f"K {k} E {E} {form}")
    assert (counts_from(d4, 3) != counts_from(d4, 2)).any()


def run_vc(exe, tmp_path, R, adds):
    src, dst = tmp_path / "vc.bin", tmp_path / "vc.out"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(adds)))
        for a in adds:
            fh.write(struct.pack("<5I", *a))
    subprocess.run([exe, "vc", str(R), str(src), str(dst)], check=True, timeout=60)
    out = np.fromfile(dst, dtype=np.uint32)
    return int(out[0]), int(out[1]), out[2:2 + len(adds)], out[2 + len(adds):]


M = 0xFFFFFFFF


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_plane_counters_up_to_the_flush_threshold(tool, tmp_path, R):
    """vc_windows(R) windows of R levels each fill the planes (31 // R: 7 windows at R = 4): bit s of
    the words adds s per window (s = 0..R: the nested levels a[R - s ..] hit), bit 8 would add R but
    sits in a lane without a window.  vc_full_r turns true at the threshold and not before; every count
    is exact there, and one add past it -- at R = 4 the first that overflows five planes -- no longer is."""
    planes, windows, _, _ = run_vc(tool, tmp_path, R, [])
    assert planes == 5 and windows == 31 // R and R * windows <= 31 < R * (windows + 1)
    # level r (0 = exact) is hit by the bits s with r >= R - s, i.e. s >= R - r
    a = [M & ~sum(1 << s for s in list(range(R - r, R + 1)) + [8]) for r in range(R)] + [M] * (4 - R)
    add = tuple(a) + (M & ~(1 << 8),)
    _, _, full, counts = run_vc(tool, tmp_path, R, [add] * windows)
    assert list(full) == [0] * (windows - 1) + [1]
    assert list(counts[:R + 1]) == [s * windows for s in range(R + 1)] and not counts[R + 1:].any()
    _, _, full, counts = run_vc(tool, tmp_path, R, [add] * (windows + 1))
    assert list(full[-2:]) == [1, 1]
    assert list(counts[:R]) == [s * (windows + 1) for s in range(R)]  # (the smaller sums still fit)
    assert int(counts[R]) == (R * (windows + 1)) % 32
    # mixed adds of 0..R in every order the levels allow, against plain sums
    rng = random.Random(R)
    sums = np.zeros(32, np.int64)
    adds = []
    for _ in range(windows):
        s = [rng.randint(0, R) for _ in range(32)]
        live = rng.getrandbits(32)
        lv = [M & ~sum(1 << j for j in range(32) if r >= R - s[j]) for r in range(R)] + [0] * (4 - R)
        adds.append(tuple(lv) + (live,))
        sums += np.array([s[j] if live >> j & 1 else 0 for j in range(32)])
    _, _, _, counts = run_vc(tool, tmp_path, R, adds)
    np.testing.assert_array_equal(counts.astype(np.int64), sums)


def test_flushes_at_the_threshold(tool, tmp_path):
    """The counting loop at E = 3 flushes once per 7 windows and block; at E <= 2 in the kernels' form
    once per 10 (VC_WINDOWS: the levels dropped add less, never more); the all-T k-mer over all-T windows
    counts E + 1 per window."""
    for k in (16, 32):
        km = [cases.kmer_value("T" * k)] * 3
        for n in (6, 7, 8, 15, 21):
            got, flushes = run_count(tool, tmp_path, "kernel", 3, k, km, ["T" * (k + 5)] * n)
            assert list(got) == [4 * n] * 3 and flushes == (n + 6) // 7
        for E in (0, 1):
            got, flushes = run_count(tool, tmp_path, "kernel", E, k, km, ["T" * (k + 5)] * 21)
            assert list(got) == [(E + 1) * 21] * 3 and flushes == 3
            got, flushes = run_count(tool, tmp_path, "rows", E, k, km, ["T" * (k + 5)] * 32)
            assert list(got) == [(E + 1) * 32] * 3 and flushes == -(-32 // (31 // (E + 1)))


def test_only_listed_k_and_budgets(tool, tmp_path):
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<3I", 17, 0, 0))
    assert subprocess.run([tool, "count", "kernel", "3", str(src), str(dst)], timeout=60).returncode == 3
    src.write_bytes(struct.pack("<3I", 16, 0, 0))
    assert subprocess.run([tool, "count", "kernel", "4", str(src), str(dst)], timeout=60).returncode == 2


# ---- C ABI ----------------------------------------------------------------------------------------

def test_abi_symbols_and_null_context():
    """Both symbols are declared in the header and exported; a NULL context is refused whatever the
    value; the ABI version stays 8 (additive exports)."""
    L = _lib.load()
    assert {"ac_set_max_errors", "ac_max_errors"} <= set(_lib.header_functions())
    assert hasattr(L, "ac_set_max_errors") and hasattr(L, "ac_max_errors")
    assert L.ac_set_max_errors(None, 3) == _lib.AC_ERR_INVALID
    assert L.ac_set_max_errors(None, 4) == _lib.AC_ERR_INVALID
    assert L.ac_max_errors(None) == 2
    assert L.ac_abi_version() == 8


def test_python_signatures():
    """error_count keeps the mirror signature's first five arguments and gains max_errors = 2;
    ApproxCounter takes max_errors = 2."""
    import inspect

    import approx_counter_amd as ac

    sig = inspect.signature(ac.error_count)
    assert list(sig.parameters) == ["sequences", "exact_count", "nb_thread", "k", "v", "max_errors"]
    assert sig.parameters["max_errors"].default == 2 and sig.parameters["v"].default == 0
    assert inspect.signature(ac.ApproxCounter.__init__).parameters["max_errors"].default == 2
    assert isinstance(ac.ApproxCounter.max_errors, property) and callable(ac.ApproxCounter.set_max_errors)


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_rejects_bad_budgets():
    r = cli("--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr
    r = cli("--max-errors", "x")
    assert r.returncode == 1 and "cannot be casted to integer" in r.stderr


def test_cli_names_the_allowed_k_before_anything_is_opened():
    """k = 17 at another budget than 2 fails with the message that names the allowed k -- before the
    input is parsed (the file does not exist: parsing it would throw) or a device opened (none here)."""
    for k in ("17", "15"):
        r = cli("--max-errors", "3", "-k", k)
        assert r.returncode == 1 and "16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--max-errors", "1", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "at most 255" in r.stderr
    r = cli("--max-errors", "0", "-k", "22", "-g", "2")
    assert r.returncode == 1 and "one GPU" in r.stderr


def test_cli_help_lists_the_extension():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--max-errors INTEGER" in r.stdout and "--seed INTEGER" in r.stdout


# ---- the plan layer's refusals ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("budget") / "budget_plan_check")
    subprocess.run(["g++"] + SANITIZE + ["-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                         os.path.join(ROOT, "tools", "budget_plan_check.cpp"),
                                         os.path.join(CSRC, "stage_plan.cpp"), os.path.join(CSRC, "host_pack.cpp"),
                                         "-o", exe], check=True)
    return exe


def plan(exe, E, k, *jobs, early=1, **env):
    r = subprocess.run([exe, str(E), str(k), str(early)] + list(jobs), capture_output=True, text=True, timeout=60,
                       check=True, env=dict(os.environ, **env))
    return r.stdout.strip()


def test_plan_accepts_and_refuses(plan_tool):
    """Where the plan decides the route it decides the budget: E = 3 is accepted for equal windows at
    k = 22 -- unless AC_BITSLICE=0 -- and refused for a ragged job, an equal job beside a ragged one,
    k = 17, k = 15 and windows over 256 bases; E = 2 is never refused."""
    on = dict(AC_BITSLICE="1")
    for early in (0, 1):
        assert plan(plan_tool, 3, 22, "300:100x37", early=early, **on) == "ok"
        assert plan(plan_tool, 3, 22, "300:100x37", "40:101x9", early=early, **on) == "ok"
        assert plan(plan_tool, 0, 16, "1:256x3", early=early, **on) == "ok"
        # (a job without candidates or without windows is not live: its windows do not matter)
        assert plan(plan_tool, 3, 22, "300:100x37", "0:90,91", early=early, **on) == "ok"
        assert "ragged" in plan(plan_tool, 3, 22, "300:100x37,99", early=early, **on)
        assert "ragged" in plan(plan_tool, 3, 22, "300:100x37", "5:100x3,101", early=early, **on)
        assert "k = 16 or 18..32" in plan(plan_tool, 3, 17, "300:100x37", early=early, **on)
        assert "k = 16 or 18..32" in plan(plan_tool, 1, 15, "300:100x37", early=early, **on)
        assert "1..256" in plan(plan_tool, 3, 22, "300:300x5", early=early, **on)
        assert "AC_BITSLICE" in plan(plan_tool, 3, 22, "300:100x37", early=early, AC_BITSLICE="0")
        for spec, k in (("300:100x37,99", 22), ("300:100x37", 17), ("300:300x5", 22)):
            assert plan(plan_tool, 2, k, spec, early=early, **on) == "ok"
            assert plan(plan_tool, 2, k, spec, early=early, AC_BITSLICE="0") == "ok"
    assert plan(plan_tool, 4, 22, "300:100x37", **on).startswith("refused: max_errors must be 0..3")
