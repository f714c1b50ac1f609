"""The bit-sliced NFA (approx_counter_amd/csrc/bs_nfa.h) on the CPU for the pattern lengths above 16
in AC_BS_K_LIST: tools/bs_nfa_check.cpp, built with g++ under the address and undefined-behaviour
sanitizers and run as a child process (as tests/test_bs_nfa.py does for k = 16), against the CPU oracle
(oracle.count_myers), bit-exactly.  The tool refuses an unlisted k with exit status 3.

Every list of cases is written over the k in AC_BS_K_LIST (LISTED_K, read from the header): a k taken
off the list takes its cases with it."""
import os
import random
import re

import numpy as np
import pytest

import oracle
from tests import cases
from tests.test_bs_nfa import edit_variants, run_count, tool  # noqa: F401  (tool: the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")


def listed_k():
    """The pattern lengths of AC_BS_K_LIST (bs_nfa.h), the one place routing and instantiation read."""
    text = open(os.path.join(CSRC, "bs_nfa.h")).read()
    m = re.search(r"#define AC_BS_K_LIST\(X\)((?:.*\\\n)*.*)\n", text)
    assert m, "AC_BS_K_LIST not found"
    return [int(x) for x in re.findall(r"X\((\d+)\)", m.group(1))]


LISTED_K = listed_k()
NEW_K = [k for k in LISTED_K if k > 16]
EDGE_K = [k for k in (22, 32) if k in LISTED_K]


def test_the_list_is_read():
    assert 16 in LISTED_K and 15 not in LISTED_K and 17 not in LISTED_K
    assert all(3 <= k <= 32 for k in LISTED_K) and len(set(LISTED_K)) == len(LISTED_K)


@pytest.mark.parametrize("k", NEW_K)
def test_random_windows_match_the_oracle(tool, tmp_path, k):
    """70 candidates (two blocks of 32 and a partial third) over 150 windows of k - 2 .. 100 bases,
    most with a planted occurrence of 0..3 edits, 1 % N."""
    kmers, wins = cases.planted_case(100 + k, k, 70, 150, win_len=(k - 2, 100), p_n=0.01)
    got, _ = run_count(tool, tmp_path, kmers, wins, k=k)
    want = oracle.count_myers(k, kmers, wins)
    assert want.sum() > 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", EDGE_K)
def test_planted_edits_at_both_window_ends(tool, tmp_path, k):
    """Occurrences with 0..3 substitutions, insertions or deletions that start at a window's first
    base, that end at its last base, and that are the whole window."""
    rng = random.Random(k)
    kmers = [cases.kmer_value(cases.rand_seq(rng, k)) for _ in range(33)]
    wins = []
    for v in kmers[:6]:
        for _, _, occ in edit_variants(rng, cases.kmer_string(v, k)):
            pad = cases.rand_seq(rng, rng.randint(1, 40))
            wins += [occ + pad, pad + occ, occ]
    got, _ = run_count(tool, tmp_path, kmers, wins, k=k)
    want = oracle.count_myers(k, kmers, wins)
    assert want.sum() > 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", EDGE_K)
def test_n_inside_an_occurrence(tool, tmp_path, k):
    """N matches nothing: inside an occurrence (at its first, a middle, its 17th and its last base), at a
    window's first and last base, all-N windows."""
    rng = random.Random(60 + k)
    kmers = [cases.kmer_value(cases.rand_seq(rng, k)) for _ in range(5)] + [cases.kmer_value("A" * k)]
    wins = []
    for v in kmers:
        s = cases.kmer_string(v, k)
        for p in (0, 7, 16, k - 1):
            wins += [s[:p] + "N" + s[p + 1:], "N" + s, s + "N", "ACGT" + s[:p] + "N" + s[p:] + "TT"]
    wins += ["N" * 40, "N" * k, "A" * (k // 2) + "N" + "A" * (k // 2), "A" * (k + 14)]
    got, _ = run_count(tool, tmp_path, kmers, wins, k=k)
    want = oracle.count_myers(k, kmers, wins)
    assert want.sum() > 0
    assert np.array_equal(got, want)


def shared_prefix_case(k, seed=9):
    """Candidates that share their first 16 bases and differ at position 16, at position k - 1 or at both
    (everything past the first table pass of 16 positions, up to the hit position), a control that
    differs at position 0, and windows holding each of them exactly, with one edit and with two."""
    rng = random.Random(seed + k)
    base = cases.rand_seq(rng, k)

    def with_base(s, p, c):
        return s[:p] + c + s[p + 1:]

    others = [c for c in "ACGT" if c != base[16]]
    last = [c for c in "ACGT" if c != base[k - 1]]
    strings = [base] + [with_base(base, 16, c) for c in others] + [with_base(base, k - 1, c) for c in last]
    strings += [with_base(with_base(base, 16, others[0]), k - 1, last[0]), with_base(base, 0, "ACGT"["ACGT".index(base[0]) ^ 1])]
    assert len(set(strings)) == len(strings) and len({s[:16] for s in strings[:-1]}) == 1
    wins = []
    for s in strings:
        pad = cases.rand_seq(rng, 11)
        wins += [s, pad + s, s + pad, pad + cases.mutate(rng, s, 1) + pad, cases.mutate(rng, s, 2) + pad]
    return [cases.kmer_value(s) for s in strings], wins


@pytest.mark.parametrize("k", EDGE_K)
def test_candidates_sharing_their_first_16_bases(tool, tmp_path, k):
    kmers, wins = shared_prefix_case(k)
    got, _ = run_count(tool, tmp_path, kmers, wins, k=k)
    want = oracle.count_myers(k, kmers, wins)
    assert len(set(want.tolist())) > 1  # the candidates are told apart
    assert np.array_equal(got, want)


def all_t_case(k, seed=4):
    """The all-T k-mer (every 2-bit code 3: at k = 32 all 64 bits of the word), the all-A one (the
    word 0), a k-mer whose first base is T (the word's highest code) and random ones; windows of T runs
    around k, with a break, and with occurrences of the others."""
    rng = random.Random(seed + k)
    t_first = "T" + cases.rand_seq(rng, k - 1)
    strings = ["T" * k, "A" * k, t_first, "T" * (k - 1) + "A", "A" + "T" * (k - 1)] + [cases.rand_seq(rng, k) for _ in range(3)]
    wins = ["T" * n for n in (k - 3, k - 2, k - 1, k, k + 1, 60)] + ["T" * (k // 2) + "G" + "T" * (k // 2), "A" * (k + 5)]
    wins += ["T" * 9 + "C" + "T" * (k - 1), t_first, "GG" + t_first[:-1], t_first[1:] + "ACGT", "N" + "T" * k, "T" * (k - 1) + "N"]
    return [cases.kmer_value(s) for s in strings], wins


@pytest.mark.parametrize("k", EDGE_K)
def test_the_all_t_kmer(tool, tmp_path, k):
    kmers, wins = all_t_case(k)
    assert k < 32 or kmers[0] == 2 ** 64 - 1
    got, _ = run_count(tool, tmp_path, kmers, wins, k=k)
    want = oracle.count_myers(k, kmers, wins)
    assert want[0] > 0 and want[2] > 0
    assert np.array_equal(got, want)
