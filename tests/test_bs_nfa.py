"""The bit-sliced NFA and its bit-plane counters (approx_counter_amd/csrc/bs_nfa.h) on the CPU.

The header compiles for the device (the bit-sliced count kernel, bs_count.inc) and for the host;
tools/bs_nfa_check.cpp drives the host build -- with g++ under the address and undefined-behaviour
sanitizers, as a child process -- the way the kernel does: candidates in blocks of 32, a window's
bases in pairs (step2) and an odd last base (step), hits summed in a VCount that is flushed when
vc_full says so.  Its counts are compared with the CPU oracle (oracle.count_myers) for k = 16."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import oracle
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
K = 16


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bs") / "bs_nfa_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tools", "bs_nfa_check.cpp"), "-o", exe], check=True)
    return exe


def run_count(exe, tmp_path, kmers, windows, k=K):
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<3I", k, len(kmers), len(windows)))
        fh.write(struct.pack(f"<{len(kmers)}Q", *kmers))
        for w in windows:
            fh.write(struct.pack("<I", len(w)))
            fh.write(bytes("ACGT".index(c) if c in "ACGT" else 4 for c in w))
    subprocess.run([exe, "count", str(src), str(dst)], check=True, timeout=120)
    out = np.fromfile(dst, dtype=np.uint32)
    assert len(out) == len(kmers) + 1
    return out[:-1], int(out[-1])


def edit_variants(rng, kmer):
    """The k-mer with 0..3 edits of each kind at random places: (edits, kind, string)."""
    out = [(0, "none", kmer)]
    for n in (1, 2, 3):
        for kind in ("sub", "ins", "del"):
            s = list(kmer)
            for _ in range(n):
                if kind == "sub":
                    p = rng.randrange(len(s))
                    s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
                elif kind == "ins":
                    s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
                else:
                    del s[rng.randrange(len(s))]
            out.append((n, kind, "".join(s)))
    return out


def test_random_windows_match_the_oracle(tool, tmp_path):
    """Random candidates (more than one block of 32, a partial last block) over random windows of
    k - 2 .. 100 bases, most with a planted occurrence of 0..3 edits, 1 % N."""
    kmers, wins = cases.planted_case(11, K, 70, 150, win_len=(K - 2, 100), p_n=0.01)
    got, _ = run_count(tool, tmp_path, kmers, wins)
    np.testing.assert_array_equal(got, oracle.count_myers(K, kmers, wins))


def test_planted_edits_at_both_window_ends(tool, tmp_path):
    """Occurrences with 0 / 1 / 2 / 3 substitutions, insertions or deletions that start at a window's
    first base and that end at its last base -- where the free start and the last position's hit
    accumulation are decided -- and as the whole window."""
    rng = random.Random(5)
    kmers = [cases.kmer_value(cases.rand_seq(rng, K)) for _ in range(33)]
    wins = []
    for v in kmers[:6]:
        for _, _, occ in edit_variants(rng, cases.kmer_string(v, K)):
            pad = cases.rand_seq(rng, rng.randint(1, 40))
            wins += [occ + pad, pad + occ, occ]
    got, _ = run_count(tool, tmp_path, kmers, wins)
    want = oracle.count_myers(K, kmers, wins)
    assert want.sum() > 0
    np.testing.assert_array_equal(got, want)


def test_n_bases(tool, tmp_path):
    """N matches nothing: inside an occurrence, at a window's first and last base, all-N windows."""
    rng = random.Random(6)
    kmers = [cases.kmer_value(cases.rand_seq(rng, K)) for _ in range(5)] + [cases.kmer_value("A" * K)]
    wins = []
    for v in kmers:
        s = cases.kmer_string(v, K)
        for p in (0, 7, K - 1):
            wins += [s[:p] + "N" + s[p + 1:], "N" + s, s + "N", "ACGT" + s[:p] + "N" + s[p:] + "TT"]
    wins += ["N" * 40, "N" * K, "A" * 8 + "N" + "A" * 8, "A" * 30]
    got, _ = run_count(tool, tmp_path, kmers, wins)
    np.testing.assert_array_equal(got, oracle.count_myers(K, kmers, wins))


def test_counter_flush_threshold(tool, tmp_path):
    """VC_WINDOWS windows of 3 levels each fill the planes exactly (2^VC_PLANES - 1 >= 3 VC_WINDOWS):
    vc_full turns true at the VC_WINDOWS-th add and not before, and every count is still exact there;
    the counting loop flushes once per VC_WINDOWS windows and block."""
    def vc(adds):
        src, dst = tmp_path / "vc.bin", tmp_path / "vc.out"
        with open(src, "wb") as fh:
            fh.write(struct.pack("<I", len(adds)))
            for a in adds:
                fh.write(struct.pack("<4I", *a))
        subprocess.run([tool, "vc", str(src), str(dst)], check=True, timeout=60)
        out = np.fromfile(dst, dtype=np.uint32)
        return int(out[0]), int(out[1]), out[2:2 + len(adds)], out[2 + len(adds):]

    planes, windows, _, _ = vc([])
    assert 3 * windows <= 2 ** planes - 1 < 3 * (windows + 1)
    # bit 0: all three levels every window; bit 1: level 2 only; bit 2: levels 1 and 2; bit 3: nothing;
    # bit 4: three levels, but in a lane without a window (live clear)
    a0, a1, a2, live = ~0b10001 & 0xFFFFFFFF, ~0b10101 & 0xFFFFFFFF, ~0b10111 & 0xFFFFFFFF, ~0b10000 & 0xFFFFFFFF
    _, _, full, counts = vc([(a0, a1, a2, live)] * windows)
    assert list(full) == [0] * (windows - 1) + [1]
    assert list(counts[:5]) == [3 * windows, windows, 2 * windows, 0, 0] and not counts[5:].any()
    # the loop: one block of candidates that all hit every window, windows at, below and above the threshold
    kmers = [cases.kmer_value("ACGTACGTTGCAAGCT")] * 3
    for n in (windows - 1, windows, windows + 1, 2 * windows + 1):
        got, flushes = run_count(tool, tmp_path, kmers, ["ACGTACGTTGCAAGCT"] * n)
        assert list(got) == [3 * n] * 3
        assert flushes == (n + windows - 1) // windows


def test_only_listed_k(tool, tmp_path):
    """k = 16 is the one instantiation (AC_BS_K_LIST): another k is refused, not miscounted."""
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<3I", 15, 0, 0))
    assert subprocess.run([tool, "count", str(src), str(dst)], timeout=60).returncode == 3
