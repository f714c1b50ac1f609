"""Edit profiles (ac_hit_edit_profile_device, ac_window_edits_samples; DESIGN.md §4e "Edit profiles") on the
CPU: the definition by hand, the host build of the per-pair alignment and traceback (hit_edit.h) through
tools/hit_edit_check.cpp -- a stand-alone program built with g++ under the address and undefined-behaviour
sanitizers -- on real and on hostile planes, the marginals against the level counts and the distances,
edit_consensus, the three C-ABI symbols, the Python surface and the command line's preconditions."""
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.edit_cases import (alignments, assert_properties, distances, edit_matrices, edit_profile_of, expected_spans,
                              pack_hits, pack_positions, pack_starts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MATCH, SUB_A, SUB_C, SUB_G, SUB_T, SUB_N, DEL, INS_A, INS_C, INS_G, INS_T, INS_N = range(12)
# the cases the definition was checked on when it was written: (k, E, L)
DEFINITION_CASES = [(16, 2, 100), (22, 3, 150), (5, 1, 33), (32, 3, 64), (17, 2, 96), (16, 0, 100)]


# ---- the definition ---------------------------------------------------------------------------------

def by_hand(kmer, text):
    """The profile (k, 12) of `kmer` against the occurrence `text`, set between two bases of other text."""
    w = "T" + text + "G"
    hit = np.ones((1, 1), bool)
    got = edit_profile_of(len(kmer), [cases.kmer_value(kmer)], [w], hit, np.array([[1 + len(text)]]), np.array([[1]]))
    assert got.shape == (1, len(kmer), 12) and got.dtype == np.uint32
    return got[0]


def expect(k, ops):
    want = np.zeros((k, 12), np.uint32)
    for i in range(k):
        for op in ops.get(i, (MATCH,)):
            want[i, op] = 1
    return want


def test_edits_by_hand():
    # one substitution: base 2 (G) is read as C
    np.testing.assert_array_equal(by_hand("ACGTAC", "ACCTAC"), expect(6, {2: (SUB_C,)}))
    # an N of the window matches nothing: substituted by N
    np.testing.assert_array_equal(by_hand("ACGTAC", "ACNTAC"), expect(6, {2: (SUB_N,)}))
    # one deletion: base 2 is missing from the read
    np.testing.assert_array_equal(by_hand("ACGTAC", "ACTAC"), expect(6, {2: (DEL,)}))
    # one insertion: a T after base 2, which itself matches; and an inserted N
    np.testing.assert_array_equal(by_hand("ACGAAC", "ACGTAAC"), expect(6, {2: (MATCH, INS_T)}))
    np.testing.assert_array_equal(by_hand("ACGTAC", "ACGNTAC"), expect(6, {2: (MATCH, INS_N)}))
    # a tie: ACGGTA against ACGTA lost one of its two G.  At cell (4, 3) the diagonal (G = G) and the deletion
    # both hold; the diagonal is taken, so base 3 matches and base 2 is the deleted one
    np.testing.assert_array_equal(by_hand("ACGGTA", "ACGTA"), expect(6, {2: (DEL,)}))
    # an insertion before the first base is counted nowhere; one after the last base on the last base
    np.testing.assert_array_equal(by_hand("ACGTAC", "GACGTAC"), expect(6, {}))
    np.testing.assert_array_equal(by_hand("ACGTAC", "ACGTACT"), expect(6, {5: (MATCH, INS_T)}))
    # farther than 3 edits, or a length more than 3 from k: nothing
    assert not by_hand("ACGTAC", "TGCATG").any()
    assert not by_hand("ACGTACGT", "ACGT").any() and by_hand("ACGTACGT", "ACGTA").any()


# ---- the walk and the step --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("edit") / "hit_edit_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_edit_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, tmp_path, k, km, w, plane, pos_m, start_m):
    """`plane`: (n_windows, words) hit words; `pos_m`, `start_m`: (8, n_windows, words) words."""
    src, dst = tmp_path / "edit.bin", tmp_path / "edit.out"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4I", len(km), len(w), len(w[0]), k))
        fh.write(np.ascontiguousarray(km, "<u8").tobytes())
        for x in w:
            fh.write(bytes("ACGT".index(c) if c in "ACGT" else 4 for c in x))
        fh.write(np.ascontiguousarray(plane, "<u4").tobytes())
        fh.write(np.ascontiguousarray(pos_m, "<u4").tobytes())
        fh.write(np.ascontiguousarray(start_m, "<u4").tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    return np.fromfile(dst, dtype="<u4").reshape(len(km), k, 12)


def k_cases(k):
    """Every (L, E) of one k: [(L, E, kmers, windows, hit, pos, start)], built once (tests.edit_cases.edit_matrices)."""
    out = []
    for L in (33, 64, 100, 150, 256):
        for E in (0, 1, 2, 3):
            km, w, hit, pos, start, _ = edit_matrices(k * 1000 + L + E, k, 40, 14 if L < 256 else 8, L, E)
            out.append((L, E, km, w, hit, pos, start))
    return out


@pytest.mark.parametrize("k", [5, 16, 17, 22, 32])
def test_walk_and_step_against_the_definition(tool, tmp_path, k):
    """k = 5, 16, 17, 22, 32 x E = 0..3 x window lengths 33, 64, 100, 150 and 256, 40 candidates (a partial
    second word): the profile from hit_edit.h's pass over 7 diagonals and its traceback equals the full
    table's, word for word, under the sanitizers.  Over the k's cases: more than 300 hit pairs, every one of the 12 operations seen, a
    start at 0 and an end at L."""
    all_cases = k_cases(k)
    assert_properties([(k, km, w, hit[E], pos, start) for _, E, km, w, hit, pos, start in all_cases], k)
    for L, E, km, w, hit, pos, start in all_cases:
        got = run_tool(tool, tmp_path, k, km, w, pack_hits(hit)[E], pack_positions(pos), pack_starts(start, hit[E]))
        np.testing.assert_array_equal(got, edit_profile_of(k, km, w, hit[E], pos, start), err_msg=f"k {k} L {L} E {E}")
    # a lower plane selects the pairs within fewer edits
    L, E, km, w, hit, pos, start = next(c for c in all_cases if c[0] == 100 and c[1] == 2)
    got = run_tool(tool, tmp_path, k, km, w, pack_hits(hit)[0], pack_positions(pos), pack_starts(start, hit[E]))
    want = edit_profile_of(k, km, w, hit[0], pos, start)
    np.testing.assert_array_equal(got, want)
    assert want[:, :, MATCH].any() and not want[:, :, 1:].any()


def hostile_edit_planes(k, seed=3):
    """A real case's pairs (E = 2, 100 bases) and, on pairs WITHOUT a hit, bits of the plane whose stored end
    and start are, in turn: a stored position of 0 (pos = 1) with start 0; an end past the window; a start at
    or past the end; a length more than 3 from k; a substring of k bases of unrelated text.  Returns (km, w,
    real hit plane, fake hit plane, pos, start): pos and start hold both kinds' values."""
    L = 100
    km, w, hit, pos, start, _ = edit_matrices(seed, k, 40, 14, L, 2)
    real = hit[2]
    rng = np.random.default_rng(seed)
    fake = ~real & (rng.random(real.shape) < 0.2)
    P, S = np.where(real, pos, 0).astype(np.int64), np.where(real, start, 0).astype(np.int64)
    for n, (wi, c) in enumerate(np.argwhere(fake)):
        kind = n % 5
        if kind == 0:
            p, s = 1, 0
        elif kind == 1:
            p = int(rng.integers(L + 1, 257))
            s = p - k
        elif kind == 2:
            p = int(rng.integers(1, L + 1))
            s = p + int(rng.integers(0, 3))
        elif kind == 3:
            p = int(rng.integers(k + 8, L + 1))
            s = p - (k + 4 + int(rng.integers(0, 3)) if n % 2 else k - 4)
        else:
            p = int(rng.integers(k, L + 1))
            s = p - k
        P[wi, c], S[wi, c] = p, s
    return km, w, real, fake, P, S


@pytest.mark.parametrize("k", [16, 17, 32])
def test_hostile_planes_count_nothing(tool, tmp_path, k):
    """Every hostile pair gives zeros -- a pair of unrelated text that happens to lie within 3 edits would be no
    hostile pair: the definition counts it -- and the sanitizers see no read outside a window (the tool's second
    pass has every window in buffers of exactly its size).  (Not at k = 5: 100 bases hold every 5-mer within 2
    edits, so no pair is free.)"""
    km, w, real, fake, P, S = hostile_edit_planes(k)
    al = alignments(k, km, w, fake, P, S)
    assert fake.sum() >= 50 and (al["dist"] > 3).sum() >= 5
    dead = fake.copy()
    dead[al["ws"][al["counted"]], al["cs"][al["counted"]]] = False  # (within 3 edits by chance: counted, by the definition)
    assert dead.sum() >= 40

    def planes(h):
        return pack_hits(h[None])[0], pack_positions(np.where(h, P, -1)), pack_starts(np.where(h, S, -1), h)

    assert not run_tool(tool, tmp_path, k, km, w, *planes(dead)).any()
    want = edit_profile_of(k, km, w, real, P, S)
    assert want[:, :, 1:].any()
    np.testing.assert_array_equal(run_tool(tool, tmp_path, k, km, w, *planes(real | dead)), want)
    np.testing.assert_array_equal(run_tool(tool, tmp_path, k, km, w, *planes(real | fake)),
                                  edit_profile_of(k, km, w, real | fake, P, S))
    # stray bits past n_kmers in every plane are not walked
    stray = np.uint32((0xFFFFFFFF << (40 % 32)) & 0xFFFFFFFF)
    plane, pm, sm = (a.copy() for a in planes(real | dead))
    plane[:, -1] |= stray
    pm[:, :, -1] |= stray
    sm[:, :, -1] |= stray
    np.testing.assert_array_equal(run_tool(tool, tmp_path, k, km, w, plane, pm, sm), want)


def test_tool_refuses_malformed_input(tool, tmp_path):
    src = tmp_path / "bad.bin"
    src.write_bytes(struct.pack("<4I", 1, 1, 8, 33))  # (k = 33)
    assert subprocess.run([tool, str(src), str(tmp_path / "o.bin")], timeout=60).returncode == 2


# ---- marginals --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,E,L", DEFINITION_CASES)
def test_marginals(k, E, L):
    """For matrices that come from the count launch and the span pass: no pair is skipped and D[k][m] is the
    pair's distance; no alignment begins or ends with an insertion; per k-mer and base the operations 0..6 sum
    to the plane's level count; the operations 1..11 of a k-mer sum to the sum of its hit windows' distances."""
    km, w, hit, pos, start, _ = edit_matrices(k * 1000 + L, k, 40, 14, L, E)
    al = alignments(k, km, w, hit[E], pos, start)
    d = distances(hit)
    assert al["ws"].size > 50
    assert al["counted"].all()
    np.testing.assert_array_equal(al["dist"], d[al["ws"], al["cs"]])
    assert not al["begins_ins"].any() and not al["ends_ins"].any()
    prof = al["profile"].astype(np.int64)
    level_counts = hit.sum(axis=1)  # (levels, n_kmers)
    np.testing.assert_array_equal(prof[:, :, :7].sum(axis=2), np.repeat(level_counts[E][:, None], k, axis=1))
    np.testing.assert_array_equal(prof[:, :, 1:].sum(axis=(1, 2)), np.where(hit[E], d, 0).sum(axis=0))
    assert not prof[np.arange(len(km))[:, None], np.arange(k)[None, :],
                    1 + np.array([[(int(v) >> (2 * (k - 1 - i))) & 3 for i in range(k)] for v in km])].any(), \
        "substituted by the k-mer's own base"


# ---- edit_consensus ---------------------------------------------------------------------------------

def test_consensus_corrects_a_planted_variant():
    """An erroneous variant of a k-mer -- base 3 read as A, base 8 missing, a C after base 11 -- in 24 windows,
    the k-mer itself in 6: the profile from the definition over the real matrices gives the variant back."""
    k, kmer = 16, "ACGTCGATGCTAGCAT"
    variant = kmer[:3] + "A" + kmer[4:8] + kmer[9:12] + "C" + kmer[12:]
    rng = np.random.default_rng(7)
    w = []
    for i in range(30):
        t = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=60))
        occ = variant if i < 24 else kmer
        at = int(rng.integers(0, 60 - len(occ)))
        w.append(t[:at] + occ + t[at + len(occ):])
    km = [cases.kmer_value(kmer)]
    hit, pos, start, _, _ = expected_spans(k, km, w, 3)
    assert hit[3].all()
    prof = edit_profile_of(k, km, w, hit[3], pos, start)
    assert ac.edit_consensus(prof, km, k) == [variant]
    assert ac.edit_consensus(prof, km, k, min_share=0.79) == [variant]  # 24 of 30 is 0.8
    assert ac.edit_consensus(prof, km, k, min_share=0.8) == [kmer]      # (not more than 0.8)
    assert ac.edit_consensus(prof, km, k, min_windows=30) == [variant]
    assert ac.edit_consensus(prof, km, k, min_windows=31) == [kmer]


def test_consensus_edges():
    k, kmers = 4, [cases.kmer_value(s) for s in ("ACGT", "TTTT", "GATC")]
    p = np.zeros((3, 4, 12), np.uint32)
    p[:, :, MATCH] = 10
    # k-mer 0: ties at exactly min_share -- 5 of 10 is not more than half -- change nothing
    p[0, 1, MATCH], p[0, 1, SUB_T] = 5, 5
    p[0, 2, MATCH], p[0, 2, DEL] = 5, 5
    p[0, 3, INS_G] = 5
    # k-mer 1: a deleted base still takes its insertion; substitution by N and an inserted N never win
    p[1, 0, MATCH], p[1, 0, DEL], p[1, 0, INS_C] = 2, 8, 7
    p[1, 1, MATCH], p[1, 1, SUB_N] = 1, 9
    p[1, 2, INS_N] = 9
    p[1, 3, MATCH], p[1, 3, SUB_A], p[1, 3, INS_A] = 4, 6, 6
    # k-mer 2: no windows at all
    p[2] = 0
    assert ac.edit_consensus(p, kmers, k) == ["ACGT", "CTTAA", "GATC"]
    assert ac.edit_consensus(p, kmers, k, min_share=0.6)[1] == "CTTT"   # (6 of 10 is not more than 0.6)
    assert ac.edit_consensus(p, kmers, k, min_windows=11) == ["ACGT", "TTTT", "GATC"]
    assert ac.edit_consensus(p, kmers, k, min_windows=0)[2] == "GATC"   # (nothing is more than 0 of 0)
    assert ac.edit_consensus(np.zeros((0, 4, 12), np.uint32), [], 4) == []
    for bad in (0.49, 1.0, -1.0):
        with pytest.raises(ValueError, match="min_share"):
            ac.edit_consensus(p, kmers, k, min_share=bad)
    for shape in ((3, 4), (3, 4, 11), (2, 4, 12), (3, 5, 12)):
        with pytest.raises(ValueError, match="edit profile"):
            ac.edit_consensus(np.zeros(shape, np.uint32), kmers, k)


# ---- surface ----------------------------------------------------------------------------------------

def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    names = {"ac_hit_edit_words", "ac_hit_edit_profile_device", "ac_window_edits_samples"}
    assert names <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.ac_abi_version() == 8
    assert L.ac_hit_edit_words(40, 16) == 40 * 16 * 12 == ac.edit_words(40, 16)
    assert L.ac_hit_edit_words(0xFFFFFFFF, 32) == 0xFFFFFFFF * 32 * 12  # (computed in 64 bits)
    assert L.ac_hit_edit_profile_device(None, 16, None, 40, None, 100, None, None, None, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_window_edits_samples(None, 16, None, 0, 0, None, None, None, None, None) == _lib.AC_ERR_INVALID


def test_python_surface():
    assert {"edit_words", "edit_consensus"} <= set(ac.__all__)
    assert callable(ac.ApproxCounter.hit_edit_profile) and callable(ac.WindowHits.edit_profile)
    sig = inspect.signature(ac.ApproxCounter.window_hits).parameters
    assert list(sig)[-1] == "edits" and sig["edits"].default is False
    assert sig["flanks"].default == 0 and sig["spans"].default is False and sig["positions"].default is False
    assert list(inspect.signature(ac.ApproxCounter.hit_edit_profile).parameters)[1:] == [
        "k", "kmers", "n_kmers", "sample", "window_len", "hit_plane", "pos", "start", "n_windows", "out", "stream"]
    assert "edits" not in inspect.signature(ac.ApproxCounter.window_hits_jobs).parameters
    assert list(inspect.signature(ac.WindowHits.__init__).parameters)[-2:] == ["flanks", "edits"]
    sig = inspect.signature(ac.edit_consensus).parameters
    assert list(sig) == ["profile", "kmers", "k", "min_windows", "min_share"]
    assert sig["min_windows"].default == 1 and sig["min_share"].default == 0.5
    wh = ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, np.zeros((8, 4, 1), np.uint32), 100)
    with pytest.raises(ValueError, match="edits="):
        wh.edit_profile()
    prof = np.arange(32 * 16 * 12, dtype=np.uint32).reshape(32, 16, 12)
    wh = ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, edits=prof)
    assert wh.edit_profile().dtype == np.uint32 and wh.edit_profile().shape == (32, 16, 12)
    np.testing.assert_array_equal(wh.edit_profile(), prof)


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_edits_is_refused_before_anything_is_opened():
    for k in ("17", "15"):
        r = cli("--edits", "-k", k)
        assert r.returncode == 1 and "--edits needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--edits", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "--edits needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--edits", "-g", "2")
    assert r.returncode == 1 and "--edits needs one GPU" in r.stderr
    r = cli("--edits", "--host-exact")
    assert r.returncode == 1 and "--edits cannot be combined with --host-exact" in r.stderr
    r = cli("--edits", "--flanks", "33")
    assert r.returncode == 1 and "--flanks needs a depth of 1 to 32" in r.stderr
    r = cli("--edits", "--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr


def test_cli_help_lists_edits():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --edits\n" in r.stdout and ".edits" in r.stdout and "12 counts" in r.stdout
