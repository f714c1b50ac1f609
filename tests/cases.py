"""Seeded (k, kmers, windows) cases shared by the oracle and the GPU parity tests."""
from __future__ import annotations

import random

ALPH = "ACGT"


def rand_seq(rng, n, p_n=0.0):
    return "".join("N" if (p_n and rng.random() < p_n) else rng.choice(ALPH) for _ in range(n))


def mutate(rng, s, n_edits):
    s = list(s)
    for _ in range(n_edits):
        op = rng.randrange(3)
        if op == 0 and s:
            s[rng.randrange(len(s))] = rng.choice(ALPH)
        elif op == 1:
            s.insert(rng.randrange(len(s) + 1), rng.choice(ALPH))
        elif s:
            del s[rng.randrange(len(s))]
    return "".join(s)


def kmer_value(s):
    v = 0
    for ch in s:
        v = (v << 2) | ALPH.index(ch)
    return v


def kmer_string(v, k):
    return "".join(ALPH[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def planted_case(seed, k, n_kmers, n_windows, win_len=(20, 120), p_n=0.01, p_plant=0.7,
                 max_edits=3):
    """Random candidates and windows; most windows carry a candidate with 0..max_edits
    edits planted at the start, the end or the middle (edges stress end indels)."""
    rng = random.Random(seed)
    kmers = [kmer_value(rand_seq(rng, k)) for _ in range(n_kmers)]
    windows = []
    for _ in range(n_windows):
        L = rng.randint(*win_len)
        w = rand_seq(rng, L, p_n)
        if kmers and rng.random() < p_plant:
            pl = mutate(rng, kmer_string(rng.choice(kmers), k), rng.randint(0, max_edits))
            where = rng.randrange(3)
            if where == 0:
                w = pl + w[len(pl):]
            elif where == 1:
                w = w[: max(0, len(w) - len(pl))] + pl
            else:
                p = rng.randrange(len(w) + 1)
                w = w[:p] + pl + w[p + len(pl):]
        windows.append(w)
    return kmers, windows


N_PER_TEXT = (0, 0, 0, 1, 2, 3, 4, 5, 7)  # N bases per text, for texts of ~100 bases
SHORT_N = (0, 0, 0, 1, 0, 0, 1, 0, 2)     # for texts of 16..40 bases: more N leave too few of them a hit


def dictionary_case(seed, n_kmers, L, n_texts=61, n_per_text=N_PER_TEXT, k=16):
    """A dictionary for samples too large for an oracle pass over every window: `n_kmers` random
    candidates and `n_texts` distinct texts of exactly L bases (a 2-D Dna5 array), each with the oracle's
    count vector (`per_text`, n_texts x n_kmers, uint64).  Every text carries an occurrence of a random
    candidate -- of candidate block t % (blocks of 32) for text t, so that every block is hit -- with
    0..3 edits, cut to L, at the start, the end and the middle in turn, and n_per_text[t % len] N bases
    at random places (5 or more overflow an inline N record at L = 100).  A sample of these texts has
    the counts bincount(idx) @ per_text (dictionary_sample).
    Asserts that a sum over a sample's windows can tell the texts apart: at least 3/4 of them have a
    nonzero count vector and at least half a vector no other text has, so a row counted twice in place
    of another, or skipped, changes the sum."""
    import numpy as np

    import oracle

    rng = random.Random(seed)
    kmers = [kmer_value(rand_seq(rng, k)) for _ in range(n_kmers)]
    n_blocks = (n_kmers + 31) // 32
    texts, seen = [], set()
    while len(texts) < n_texts:
        t = len(texts)
        blk = t % n_blocks
        cand = kmers[rng.randrange(32 * blk, min(n_kmers, 32 * blk + 32))]
        pl = mutate(rng, kmer_string(cand, k), rng.randint(0, 3))[:L]
        w = rand_seq(rng, L)
        if t % 3 == 0:
            w = pl + w[len(pl):]
        elif t % 3 == 1:
            w = w[: L - len(pl)] + pl
        else:
            p = rng.randrange(L - len(pl) + 1)
            w = w[:p] + pl + w[p + len(pl):]
        w = list(w)
        for p in rng.sample(range(L), min(L, n_per_text[t % len(n_per_text)])):
            w[p] = "N"
        w = "".join(w)
        assert len(w) == L
        if w not in seen:
            seen.add(w)
            texts.append(w)
    kmers = np.array(kmers, np.uint64)
    per_text = np.stack([oracle.count_myers(k, kmers, [w]) for w in texts]).astype(np.uint64)
    dna5 = np.array([["ACGTN".index(c) for c in w] for w in texts], np.uint8)
    nonzero = int((per_text.sum(axis=1) > 0).sum())
    assert 4 * nonzero >= 3 * n_texts, f"{nonzero} of {n_texts} texts have a nonzero count vector"
    _, inverse, times = np.unique(per_text, axis=0, return_inverse=True, return_counts=True)
    unique = int((times[inverse.reshape(-1)] == 1).sum())
    assert 2 * unique >= n_texts, f"{unique} of {n_texts} texts have a count vector of their own"
    return kmers, dna5, per_text


def dictionary_sample(texts, per_text, n_windows, seed):
    """`n_windows` windows drawn uniformly (seeded) from a dictionary_case's texts, as a 2-D Dna5 array,
    and their expected counts, bincount(idx) @ per_text in uint64.  Asserts that every block of 32
    candidates holds one with a nonzero expected count (no lane word of the bit-sliced kernel is
    checked against zeros alone)."""
    import numpy as np

    idx = np.random.default_rng(seed).integers(0, len(texts), size=n_windows)
    want = np.bincount(idx, minlength=len(texts)).astype(np.uint64) @ per_text
    for b in range(0, len(want), 32):
        assert want[b:b + 32].any(), f"candidates {b}..{b + 31} expect no hit"
    return texts[idx], want


def edge_cases():
    """Hand-built edge cases: (name, k, kmers, windows)."""
    k16 = [kmer_value("ACGTACGTTGCAAGCT"), kmer_value("A" * 16), kmer_value("T" * 16)]
    out = [
        ("no_windows", 16, k16, []),
        ("empty_windows", 16, k16, ["", "", ""]),
        ("shorter_than_k", 16, k16, ["ACGTACGTTGCAAG", "ACG", "A" * 13, "A" * 14, "A" * 15]),
        ("exactly_k", 16, k16, ["ACGTACGTTGCAAGCT", "A" * 16, "T" * 15 + "A"]),
        ("all_n", 16, k16, ["N" * 100, "N" * 16]),
        ("n_inside", 16, k16, ["ACGTACGTNGCAAGCT", "ACGTACGTTGCAAGCN", "NCGTACGTTGCAAGCT",
                               "ACGTANNTTGCAAGCT", "AAAAAAAANAAAAAAAA"]),
        ("lowercase_iupac", 16, k16, ["acgtacgttgcaagct", "ACGTRYKMTGCAAGCT"]),
        ("long_window", 16, k16, ["ACGT" * 300 + "ACGTACGTTGCAAGCT"]),
        ("duplicate_kmers", 16, k16 + k16, ["ACGTACGTTGCAAGCT", "AAAAAAAAAAAAAAAAAAAA"]),
        ("k32", 32, [kmer_value("ACGT" * 8), kmer_value("A" * 32)],
         ["ACGT" * 8, "ACGT" * 7 + "ACG", "TTACGT" * 10, "A" * 31]),
        ("k2", 2, [kmer_value("AC"), kmer_value("GG")], ["A", "T", "AC", "GT", "", "N"]),
        ("k3", 3, [kmer_value("ACG"), kmer_value("TTT")], ["A", "AC", "ACG", "TT", "NNN", "CCCC"]),
        ("k4_many", 4, [kmer_value(a + b + c + d) for a in ALPH for b in ALPH for c in ALPH for d in ALPH],
         ["ACGTTGCA", "AAAA", "N", "GATTACA", "CCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCC"]),
    ]
    return out
