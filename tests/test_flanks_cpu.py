"""Flank profiles (ac_hit_flank_profile_device, ac_window_flanks_samples; DESIGN.md §4e "Flank profiles") on
the CPU: the definition by hand, the host build of the hit word's walk and the per-pair step (hit_flank.h)
through tools/hit_flank_check.cpp -- a stand-alone program built with g++ under the address and
undefined-behaviour sanitizers -- on real and on hostile planes, the marginals against the position profiles,
flank_consensus, the three C-ABI symbols, the Python surface and the command line's preconditions."""
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.flank_cases import (assert_properties, expected_spans, flank_profile_of, matrices, pack_hits, pack_positions,
                               pack_starts)
from tests.positions_cases import profile_of
from tests.test_spans_cpu import hostile_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
A, C, G, T, N = range(5)


# ---- the definition ---------------------------------------------------------------------------------

def test_flanks_by_hand():
    """ACGT at D = 3: in the middle of TTACGTTT (two bases on either side: the third column is outside), at
    the start of ACGTAAAA (no left flank), at the end of AAAAACGT (no right flank) and in TNACGTNA (an N on
    both sides)."""
    w = ["TTACGTTT", "ACGTAAAA", "AAAAACGT", "TNACGTNA"]
    hit, pos, start, _, _ = expected_spans(4, [cases.kmer_value("ACGT")], w, 0)
    assert hit[0, :, 0].all() and pos[:, 0].tolist() == [6, 4, 8, 6] and start[:, 0].tolist() == [2, 0, 4, 2]
    got = flank_profile_of(w, hit[0], pos, start, 3)
    assert got.shape == (2, 1, 3, 5) and got.dtype == np.uint32
    want = np.zeros((2, 1, 3, 5), np.uint32)
    want[0, 0, 0, [T, A, N]] = 1      # the base after: T, A, -, N
    want[0, 0, 1, T], want[0, 0, 1, A] = 1, 2
    want[0, 0, 2, A] = 1              # (only ACGTAAAA has a third base)
    want[1, 0, 0, [T, A, N]] = 1      # the base before: T, -, A, N
    want[1, 0, 1, T], want[1, 0, 1, A] = 2, 1
    want[1, 0, 2, A] = 1
    np.testing.assert_array_equal(got, want)
    # without a start matrix: the right side alone
    np.testing.assert_array_equal(flank_profile_of(w, hit[0], pos, None, 3)[0], want[0])
    assert not flank_profile_of(w, hit[0], pos, None, 3)[1].any()


# ---- the walk and the step --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flank") / "hit_flank_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_flank_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, tmp_path, w, n_kmers, plane, pos_m, start_m, depth):
    """`plane`: (n_windows, words) hit words; `pos_m`, `start_m` (or None): (8, n_windows, words) words."""
    src, dst = tmp_path / "flank.bin", tmp_path / "flank.out"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<5I", n_kmers, len(w), len(w[0]), depth, int(start_m is not None)))
        for x in w:
            fh.write(bytes("ACGT".index(c) if c in "ACGT" else 4 for c in x))
        fh.write(np.ascontiguousarray(plane, "<u4").tobytes())
        fh.write(np.ascontiguousarray(pos_m, "<u4").tobytes())
        if start_m is not None:
            fh.write(np.ascontiguousarray(start_m, "<u4").tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    return np.fromfile(dst, dtype="<u4").reshape(2, n_kmers, depth, 5)


def k_cases(k):
    """Every (L, E) of one k: [(L, E, kmers, windows, hit, pos, start)], built once (tests.flank_cases.matrices)."""
    out = []
    for L in sorted({1, k, 63, 65, 256}):
        for E in (0, 1, 2, 3):
            km, w, hit, pos, start, _ = matrices(k * 1000 + L + (E if k in (5, 17) else 0), k, 40, 14 if L < 256 else 8, L, E)
            out.append((L, E, km, w, hit, pos, start))
    return out


@pytest.mark.parametrize("k", [5, 16, 17, 22, 32])
def test_walk_and_step_against_the_definition(tool, tmp_path, k):
    """k = 5, 16, 17, 22, 32 x E = 0..3 x window lengths 1, k, 63, 65 and 256, 1 % N, 40 candidates (a partial
    second word), D = 1, 8 and 32: the profile from hit_flank.h's walk and step equals the definition's, word
    for word, under the sanitizers.  Over the k's cases: more than 300 hit pairs, every symbol seen on both
    sides, a start at 0, an end at L and a flank cut short by either edge of the window."""
    all_cases = k_cases(k)
    assert_properties([(w, hit[E], pos, start) for _, E, _, w, hit, pos, start in all_cases], 8, k)
    for L, E, km, w, hit, pos, start in all_cases:
        for D in (1, 8, 32):
            got = run_tool(tool, tmp_path, w, len(km), pack_hits(hit)[E], pack_positions(pos), pack_starts(start, hit[E]), D)
            np.testing.assert_array_equal(got, flank_profile_of(w, hit[E], pos, start, D), err_msg=f"k {k} L {L} E {E} D {D}")
    # a lower plane selects the pairs within fewer edits; no start matrix: a zero left half
    L, E, km, w, hit, pos, start = next(c for c in all_cases if c[0] == 65 and c[1] == 2)
    got = run_tool(tool, tmp_path, w, len(km), pack_hits(hit)[0], pack_positions(pos), pack_starts(start, hit[E]), 8)
    np.testing.assert_array_equal(got, flank_profile_of(w, hit[0], pos, start, 8))
    got = run_tool(tool, tmp_path, w, len(km), pack_hits(hit)[E], pack_positions(pos), None, 8)
    np.testing.assert_array_equal(got, flank_profile_of(w, hit[E], pos, None, 8))
    assert got[0].any() and not got[1].any()


def hostile_flank_planes(k, seed=3):
    """tests.test_spans_cpu.hostile_planes -- hit bits where the position planes store 0, stored positions past
    the window, level bits without the top level's -- plus a start matrix that holds the real pairs' starts and,
    for every other bit of the top plane, a start at or past the stored end.  Returns (km, w, top plane, position
    planes, start planes, real hit, real pos, real start)."""
    km, w, m, planes, starts = hostile_planes(k, seed)
    hit, pos, start, _, _ = expected_spans(k, km, w, 2)
    top = ac.unpack_hits(m, len(km))[2]
    fake = top & ~hit[2]
    assert fake.sum() >= 20
    at_end = ac.unpack_positions(planes, top, len(km))  # (the stored end of every bit of the top plane)
    rng = np.random.default_rng(seed)
    bad_start = np.minimum(at_end + rng.integers(0, 3, size=at_end.shape), 255)
    starts = starts | pack_starts(np.where(fake, bad_start, -1), fake)
    return km, w, m[2], planes, starts, hit, pos, start


@pytest.mark.parametrize("k", [5, 17])
def test_hostile_planes_count_nothing(tool, tmp_path, k):
    """(and a clean sanitizer run: the tool's second pass has every window in buffers of exactly its size)"""
    km, w, plane, planes, starts, hit, pos, start = hostile_flank_planes(k)
    want = flank_profile_of(w, hit[2], pos, start, 8)
    assert want[0].any() and want[1].any()
    np.testing.assert_array_equal(run_tool(tool, tmp_path, w, len(km), plane, planes, starts, 8), want)
    # stray bits past n_kmers in every plane are not walked either
    stray = np.uint32((0xFFFFFFFF << (40 % 32)) & 0xFFFFFFFF)
    plane, planes, starts = plane.copy(), planes.copy(), starts.copy()
    plane[:, -1] |= stray
    planes[:, :, -1] |= stray
    starts[:, :, -1] |= stray
    np.testing.assert_array_equal(run_tool(tool, tmp_path, w, len(km), plane, planes, starts, 8), want)


def test_tool_refuses_malformed_input(tool, tmp_path):
    src = tmp_path / "bad.bin"
    src.write_bytes(struct.pack("<5I", 1, 1, 8, 33, 1))  # (depth 33)
    assert subprocess.run([tool, str(src), str(tmp_path / "o.bin")], timeout=60).returncode == 2


# ---- marginals --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 22])
def test_marginals_are_the_position_profiles_tails(k):
    """The sum over the symbols of right[c][j] is the number of hit windows whose occurrence ends at or before
    base L - j - 1 (the position profile's head), of left[c][j] the number whose occurrence starts at base
    j + 1 or later (the start profile's tail)."""
    D = 32
    for L in (63, 100):
        km, w, hit, pos, start, _ = matrices(k * 1000 + L, k, 40, 14 if L == 63 else 30, L, 2)
        got = flank_profile_of(w, hit[2], pos, start, D).sum(axis=3)
        ends = profile_of(hit, pos, L).sum(axis=0)          # (n_kmers, L): index p - 1
        starts = profile_of(hit, start + 1, L).sum(axis=0)  # (n_kmers, L): index s
        assert ends.sum() == hit[2].sum() > 50
        for j in range(D):
            np.testing.assert_array_equal(got[0, :, j], ends[:, : max(L - j - 1, 0)].sum(axis=1), err_msg=f"right {j}")
            np.testing.assert_array_equal(got[1, :, j], starts[:, j + 1:].sum(axis=1), err_msg=f"left {j}")


# ---- flank_consensus --------------------------------------------------------------------------------

def planted_profile(n_windows=60, depth=16, seed=5):
    """One k-mer, exact occurrences at base 20 of windows of 100 bases whose next 12 bases are EXT and whose
    12 bases before are PRE in all but a few windows; everything else uniform."""
    rng = np.random.default_rng(seed)
    kmer, ext, pre = "ACGTTGCAAGCTTACG", "GATTACAGATTC", "CCATGGTTAACC"
    w = []
    for i in range(n_windows):
        t = list("".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=100)))
        t[20:36] = kmer
        t[36:48] = ext
        t[8:20] = pre
        if i % 10 == 0:
            t[40] = "N"
        w.append("".join(t))
    hit = np.ones((n_windows, 1), bool)
    return flank_profile_of(w, hit, np.full((n_windows, 1), 36), np.full((n_windows, 1), 20), depth), ext, pre


def test_consensus_recovers_a_planted_extension_and_stops_at_its_end():
    prof, ext, pre = planted_profile()
    (left, right), = ac.flank_consensus(prof)
    assert right == ext and left == pre  # (the left one in reading order; 60 uniform bases have no majority)
    # min_windows: more than there are windows gives nothing
    assert ac.flank_consensus(prof, min_windows=61) == [("", "")]
    assert ac.flank_consensus(prof, min_windows=60) == [(pre, ext)]
    # the column with six N in 60: 54 / 60 = 0.9 is not more than 0.9
    assert ac.flank_consensus(prof, min_share=0.9) == [(pre, ext[:4])]
    assert ac.flank_consensus(prof, min_share=0.89) == [(pre, ext)]


def test_consensus_edges():
    p = np.zeros((2, 3, 4, 5), np.uint32)
    p[0, 0, 0] = [5, 5, 0, 0, 0]       # a tie: 5 is not more than half of 10
    p[0, 1, :, G] = [4, 3, 0, 9]       # stops at the empty column; what lies past it is not looked at
    p[1, 1, :, T] = 2
    p[1, 1, 0, N] = 3                  # N counts in the total: 2 of 5
    p[0, 2, :, C] = [3, 2, 1, 1]
    p[1, 2, 0:2, A], p[1, 2, 2:4, C] = 7, 7
    got = ac.flank_consensus(p)
    assert got == [("", ""), ("", "GG"), ("CCAA", "CCCC")], got
    assert ac.flank_consensus(p, min_windows=2)[2] == ("CCAA", "CC")
    assert ac.flank_consensus(p, min_windows=0)[0] == ("", "")  # (an empty column never extends)
    assert ac.flank_consensus(np.zeros((2, 0, 4, 5), np.uint32)) == []
    with pytest.raises(ValueError):
        ac.flank_consensus(np.zeros((2, 3, 4), np.uint32))


# ---- surface ----------------------------------------------------------------------------------------

def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    names = {"ac_hit_flank_words", "ac_hit_flank_profile_device", "ac_window_flanks_samples"}
    assert names <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.ac_abi_version() == 8
    assert L.ac_hit_flank_words(40, 8) == 2 * 40 * 8 * 5 == ac.flank_words(40, 8)
    assert L.ac_hit_flank_words(0xFFFFFFFF, 32) == 2 * 0xFFFFFFFF * 32 * 5  # (computed in 64 bits)
    assert L.ac_hit_flank_profile_device(None, None, 100, None, None, None, 40, 8, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_window_flanks_samples(None, 16, None, 0, 8, None, None, None, None) == _lib.AC_ERR_INVALID


def test_python_surface():
    assert {"flank_words", "flank_consensus"} <= set(ac.__all__)
    assert callable(ac.ApproxCounter.hit_flank_profile) and callable(ac.WindowHits.flank_profile)
    sig = inspect.signature(ac.ApproxCounter.window_hits).parameters
    assert sig["flanks"].default == 0 and sig["spans"].default is False and sig["positions"].default is False
    assert list(inspect.signature(ac.ApproxCounter.hit_flank_profile).parameters)[1:] == [
        "sample", "window_len", "hit_plane", "pos", "start", "n_kmers", "n_windows", "depth", "out", "stream"]
    assert "flanks" not in inspect.signature(ac.ApproxCounter.window_hits_jobs).parameters
    wh = ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, np.zeros((8, 4, 1), np.uint32), 100)
    with pytest.raises(ValueError, match="flanks="):
        wh.flank_profile()
    prof = np.arange(2 * 32 * 4 * 5, dtype=np.uint32).reshape(2, 32, 4, 5)
    wh = ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, flanks=prof)
    assert wh.flank_profile().dtype == np.uint32 and wh.flank_profile().shape == (2, 32, 4, 5)
    np.testing.assert_array_equal(wh.flank_profile(), prof)


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_flanks_is_refused_before_anything_is_opened():
    for d in ("0", "33"):
        r = cli("--flanks", d)
        assert r.returncode == 1 and "--flanks needs a depth of 1 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    for k in ("17", "15"):
        r = cli("--flanks", "8", "-k", k)
        assert r.returncode == 1 and "--flanks needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--flanks", "8", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "--flanks needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--flanks", "8", "-g", "2")
    assert r.returncode == 1 and "--flanks needs one GPU" in r.stderr
    r = cli("--flanks", "8", "--host-exact")
    assert r.returncode == 1 and "--flanks cannot be combined with --host-exact" in r.stderr
    r = cli("--flanks", "8", "--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr


def test_cli_help_lists_flanks():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --flanks INTEGER\n" in r.stdout and ".flanks" in r.stdout and "a,c,g,t,n" in r.stdout
