"""Cases of tests/test_gpu_bs_short_launch.py (the bit-sliced count kernel's table build and flush by plane
merge), built without a GPU so that tests/test_short_launch_cases.py can
show that each has the property it is there for."""
import random

import numpy as np

from tests import cases

TABLE_COUNTS = (1, 33, 65, 129, 256, 257, 500)


def variants(k):
    """The all-A k-mer and its single-base variants at every position: 3 k + 1 strings."""
    base = "A" * k
    return [base] + [base[:i] + c + base[i + 1:] for i in range(k) for c in "CGT"]


def table_case(k, n):
    """n candidates: the first n of the 3 k + 1 variants, then random k-mers -- every (position, base) of the
    ~Eq table is some candidate's once n >= 3 k + 1, and each non-A one belongs to exactly one variant.
    Windows of k + 10 bases: every variant among the candidates planted once between random flanks."""
    rng = random.Random(1000 * k + n)
    v = variants(k)
    cand = v[:n]
    while len(cand) < n:
        s = cases.rand_seq(rng, k)
        if s not in cand:
            cand.append(s)
    wins = [cases.rand_seq(rng, 5) + s + cases.rand_seq(rng, 5) for s in cand[:len(v)]]
    return np.array([cases.kmer_value(s) for s in cand], np.uint64), wins


THRESHOLD_TEXTS = ("ACGTACGTTGCAAGCTACGT", "TGACGTACGTTGCAAGCTCA")  # both hold candidate 0, once, exactly


def threshold_case(n_windows, seed=7):
    """32 candidates of k = 16 (two lanes per window, rows of 32 windows; the second lane's block is empty):
    candidate 0 is in every window exactly, so every window adds E + 1 to it and a lane's counter for it
    stands at its threshold whenever the wave flushes at the threshold; candidates 1..15 are candidate 0 with
    one base changed, 16..23 with two, 24 a k-mer of the second text alone, the rest random.  Windows: the
    two texts, 30 % the second, so rows differ.  -> (k-mers, 2-D Dna5 windows, windows of each text)"""
    rng = random.Random(seed)
    c0 = THRESHOLD_TEXTS[0][:16]
    cand = [c0]
    for i in range(1, 24):
        s = list(c0)
        for p in ((i,) if i < 16 else (i - 16, i - 8)):
            s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + i % 3) % 4]
        cand.append("".join(s))
    cand += [THRESHOLD_TEXTS[1][1:17]] + [cases.rand_seq(rng, 16) for _ in range(7)]  # (24: exact in the second text only)
    pick = np.random.default_rng(seed).random(n_windows) < 0.3
    texts = np.array([["ACGT".index(c) for c in t] for t in THRESHOLD_TEXTS], np.uint8)
    return np.array([cases.kmer_value(s) for s in cand], np.uint64), texts[pick.astype(int)], \
        (int((~pick).sum()), int(pick.sum()))


def lanes_per_window(n):
    """LW of a candidate group of n (<= 256) candidates, and the windows of its rows."""
    lw = 2
    while 32 * lw < n:
        lw *= 2
    return lw, 64 // lw
