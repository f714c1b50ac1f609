"""Designed samples for the exact count's edges (tests/test_gpu_exact_edges.py), and the Python
mirrors of the partition's hash (approx_counter_amd/csrc/exact_count.h) they are built with.

Everything here runs on the CPU; tests/test_exact_cases.py checks the mirrors and, for every
designed sample, the condition its GPU test relies on, so that no GPU test passes vacuously.
"""
from __future__ import annotations

import functools
import random

import numpy as np

import approx_counter_amd as ac
from oracle import host_ref
from tests import cases

M32 = 0xFFFFFFFF
_C1, _C2 = 0x7FEB352D, 0x846CA68B
_C1_INV, _C2_INV = pow(_C1, -1, 1 << 32), pow(_C2, -1, 1 << 32)
BUCKET_SLOTS = 4096  # EXACT_BUCKET_SLOTS: the per-bucket LDS table
COUNT_PROBES = 64    # AC_COUNT_PROBES: probes of that table before a key overflows


# ---- mirrors of exact_count.h and of the host's geometry rule (capi_exact.cpp) -------------------

def part_hash32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * _C1) & M32
    x ^= x >> 15
    x = (x * _C2) & M32
    x ^= x >> 16
    return x


def inv_part_hash32(h: int) -> int:
    """The mixer is a bijection of 32-bit words: every step undone in reverse order."""
    h &= M32
    h ^= h >> 16
    h = (h * _C2_INV) & M32
    h ^= h >> 15
    h ^= h >> 30
    h = (h * _C1_INV) & M32
    h ^= h >> 16
    return h


def part_hash64(x: int) -> int:
    return part_hash32((x & M32) ^ part_hash32(((x >> 32) + 0x9E3779B9) & M32))


def part_hash(kmer: int, k: int) -> int:
    """The hash of a k-mer as the partition keys it: a 32-bit key for k <= 16, 64-bit above."""
    return part_hash32(kmer) if k <= 16 else part_hash64(kmer)


def bucket_of(kmer: int, k: int, nb_log2: int) -> int:
    return part_hash(kmer, k) >> (32 - nb_log2)


def home_slot(kmer: int, k: int) -> int:
    return part_hash(kmer, k) & (BUCKET_SLOTS - 1)


def nb_log2_for(n_bases: int) -> int:
    nb_log2 = 6
    while nb_log2 < 16 and (max(32, n_bases) >> nb_log2) > 2048:
        nb_log2 += 1
    return nb_log2


def s_log2_for(nb_log2: int) -> int:
    return max(min(nb_log2, 7), nb_log2 - 7 if nb_log2 > 7 else 0)


def min_bases_for(nb_log2: int) -> int:
    """The smallest image (a multiple of 32 bases) for which the host picks nb_log2 (7..16):
    the step from nb_log2 - 1 is taken when n_bases >> (nb_log2 - 1) exceeds 2048."""
    return (2049 << (nb_log2 - 1)) if nb_log2 > 6 else 32


def all_t(k: int) -> int:
    return (1 << (2 * k)) - 1


# ---- generators ------------------------------------------------------------------------------------

def crafted_keys(k: int, nb_log2: int, bucket: int, slots, per_slot: int):
    """Distinct k-mers (16 <= k <= 32) whose hash has `bucket` in its top nb_log2 bits and, for each
    s of `slots`, per_slot of them s in its low 12 bits; the bits between make them distinct.  k = 16
    inverts the 32-bit hash; above, the high half hi < 4^(k-16) is picked and the low half solved for.
    The all-T k-mer (counted apart from the table) is never returned."""
    assert 16 <= k <= 32 and 0 <= bucket < (1 << nb_log2)
    mid_bits = 32 - nb_log2 - 12
    assert mid_bits >= 0 and per_slot <= (1 << mid_bits) - 1
    out = []
    for s in slots:
        assert 0 <= s < BUCKET_SLOTS
        got, mid = 0, 0
        while got < per_slot:
            h = (bucket << (32 - nb_log2)) | (mid << 12) | s
            mid += 1
            if k == 16:
                key = inv_part_hash32(h)
            else:
                hi = (len(out) * 2654435761 + mid) % (1 << (2 * (k - 16)))
                key = (hi << 32) | (inv_part_hash32(h) ^ part_hash32((hi + 0x9E3779B9) & M32))
            if key == all_t(k):
                continue
            out.append(key)
            got += 1
    return out


def kmer_rows(keys, k: int) -> np.ndarray:
    """(len(keys), k) Dna5 ordinals: row i spells k-mer keys[i] (first base in the top bits)."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 1)
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    return ((keys >> sh) & np.uint64(3)).astype(np.uint8)


def one_kmer_windows(keys, k: int, copies) -> np.ndarray:
    """Windows of exactly k bases, one k-mer each: key i in copies[i] windows (an (n, k) array)."""
    copies = np.asarray(copies, dtype=np.int64)
    assert copies.size == len(keys)
    return np.repeat(kmer_rows(keys, k), copies, axis=0)


def strings(win2d) -> list:
    return ["".join("ACGTN"[v] for v in row) for row in win2d]


def placed(parts, n_bases: int) -> "ac.PackedSample":
    """One image of n_bases bases (a multiple of 32) holding the packed samples of `parts`,
    [(PackedSample, first base), ...], each moved to its 32-aligned first base; zeros elsewhere."""
    assert n_bases % 32 == 0
    codes = np.zeros(n_bases // 16, np.uint32)
    nmask = np.zeros(n_bases // 32, np.uint32)
    starts, lengths, end = [], [], 0
    for smp, at in sorted(parts, key=lambda p: p[1]):
        assert at % 32 == 0 and at >= end and at + smp.n_bases <= n_bases
        end = at + smp.n_bases
        codes[at // 16: at // 16 + smp.codes.size] = smp.codes
        nmask[at // 32: at // 32 + smp.nmask.size] = smp.nmask
        starts.append(smp.start + np.uint64(at))
        lengths.append(smp.length)
    return ac.PackedSample(codes, nmask, np.concatenate(starts).astype(np.uint64),
                           np.concatenate(lengths).astype(np.uint32), n_bases)


def padded(sample, n_bases: int) -> "ac.PackedSample":
    """`sample` with codes and nmask zero-extended to n_bases: a small sample chooses its nb_log2.
    The uncovered bases hold no windows, so they add no k-mers."""
    return placed([(sample, 0)], n_bases)


def window_kmers(w: str, k: int):
    """The N-free k-mers of a window (strings over ACGTN)."""
    for i in range(len(w) - k + 1):
        s = w[i:i + k]
        if "N" not in s:
            yield cases.kmer_value(s)


def ragged_reference(windows, k: int, threshold, forbidden=()):
    """count_kmers of ragged windows through host_ref.count_kmers_dense: the windows as rows padded
    with N to one length.  A padded row's extra k-mer positions all hold a padding N and are taken
    off the N-skip count again.  (kept k-mers ascending, counts, N-skips)"""
    L = max([len(w) for w in windows] + [k])
    arr = np.full((len(windows), L), 4, np.uint8)
    extra = 0
    for i, w in enumerate(windows):
        arr[i, :len(w)] = ac.to_dna5(w)
        extra += (L - k + 1) - max(0, len(w) - k + 1)
    uk, cnt, had = host_ref.count_kmers_dense(arr, k, threshold, forbidden)
    return uk, cnt, had - extra


def lc_threshold(k: int) -> float:
    return float(host_ref.adjust_threshold(1.0, 16, k))


# ---- C: geometry ------------------------------------------------------------------------------------

DENSE_NB = (7, 8, 9, 10, 11, 12)
SPARSE_NB = (9, 14, 15)


def dense_windows_n(nb_log2: int) -> int:
    """2^(3 + nb_log2) + 8 windows of 100 bases in 128-base slots put the image 1,024 bases above
    2^(10 + nb_log2); the host's rule needs 2^(nb_log2 - 1) above it, so nb_log2 = 12 takes 16 more."""
    return (1 << (3 + nb_log2)) + (8 if nb_log2 < 12 else 1 << (nb_log2 - 8))


@functools.lru_cache(maxsize=None)
def dense_windows(nb_log2: int) -> np.ndarray:
    from tools.synth import make_windows_fast

    return make_windows_fast(dense_windows_n(nb_log2), 100, seed=100 + nb_log2, at_end=False)[0]


@functools.lru_cache(maxsize=None)
def dense_reference(nb_log2: int, k: int):
    return host_ref.count_kmers_dense(dense_windows(nb_log2), k, np.float32(lc_threshold(k)))


@functools.lru_cache(maxsize=None)
def sparse_windows():
    """About 2,000 ragged windows (0 to 300 bases, 1 % N; every third of 40 bases or more begins with
    a shared 30-mer, so some k-mers repeat) in three groups."""
    rng = random.Random(2024)
    wins = [cases.rand_seq(rng, rng.randint(0, 300), p_n=0.01) for _ in range(1995)]
    motif = cases.rand_seq(rng, 30)
    wins = [motif + w[30:] if i % 3 == 0 and len(w) >= 40 else w for i, w in enumerate(wins)]
    wins += ["A" * 60, "ACACACACACACACACACACACACACAC", "T" * 40, "", "ACG"]
    return wins[:700], wins[700:1400], wins[1400:]


def sparse_sample(nb_log2: int):
    """The three groups at the first slots, the middle and the very last slots of the smallest
    image that makes the host choose nb_log2."""
    n_bases = min_bases_for(nb_log2)
    a, b, c = (ac.pack_windows(g) for g in sparse_windows())
    mid = (n_bases // 2) // 32 * 32
    return placed([(a, 0), (b, mid), (c, n_bases - c.n_bases)], n_bases)


@functools.lru_cache(maxsize=None)
def sparse_tail_windows():
    """Seven windows: the first 40 bases of two random ones and the hand-made low-complexity, all-T,
    empty and short ones."""
    last = sparse_windows()[2]
    return [w[:40] for w in last[-7:-5]] + last[-5:]


def sparse_tail_sample(nb_log2: int):
    """Those few windows alone, in the very last slots of the image: many super-buckets hold no key
    (their level-2 chunk ranges are empty and share one first chunk)."""
    n_bases = min_bases_for(nb_log2)
    smp = ac.pack_windows(sparse_tail_windows())
    return placed([(smp, n_bases - smp.n_bases)], n_bases)


@functools.lru_cache(maxsize=None)
def sparse_reference(k: int):
    a, b, c = sparse_windows()
    return ragged_reference(a + b + c, k, np.float32(lc_threshold(k)))


# ---- D: overflow fallback and table limits -------------------------------------------------------------

OVERFLOW_NB = 7
# name -> (bucket, keys crafted, partitioned path expected)
OVERFLOW_CASES = {
    "full_table": (127, lambda k: crafted_keys(k, OVERFLOW_NB, 127, range(BUCKET_SLOTS), 1), 1),
    "pigeonhole": (0, lambda k: crafted_keys(k, OVERFLOW_NB, 0, range(BUCKET_SLOTS), 1)
                   + crafted_keys(k, OVERFLOW_NB, 0, [4095], 2)[1:], 0),
    # the shared home slot sits 10 below the table's end: the probe sequence wraps
    "probe_limit": (77, lambda k: crafted_keys(k, OVERFLOW_NB, 77, [BUCKET_SLOTS - 10], COUNT_PROBES), 1),
    "probe_limit_exceeded": (77, lambda k: crafted_keys(k, OVERFLOW_NB, 77, [BUCKET_SLOTS - 10], COUNT_PROBES + 1), 0),
}


def filler_windows(k: int, n: int, seed: int, avoid_bucket=None, nb_log2: int = OVERFLOW_NB, p_n: float = 0.02):
    """n short random windows, some with N's; none of their k-mers falls in avoid_bucket."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        w = cases.rand_seq(rng, rng.randint(k, k + 25), p_n=p_n)
        if avoid_bucket is None or all(bucket_of(v, k, nb_log2) != avoid_bucket for v in window_kmers(w, k)):
            out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def overflow_case(name: str, k: int):
    """(windows, crafted keys, their copies, bucket, expected path): one-k-mer windows of the crafted
    keys (a few of them in two or three copies) among 300 random windows that stay out of the bucket."""
    bucket, make, path = OVERFLOW_CASES[name]
    keys = make(k)
    copies = [1 + (i % 29 == 0) + (i % 57 == 0) for i in range(len(keys))]
    fill = filler_windows(k, 300, seed=k * 7 + len(name), avoid_bucket=bucket)
    crafted = strings(one_kmer_windows(keys, k, copies))
    wins = fill[:150] + crafted + fill[150:]
    return wins, keys, copies, bucket, path


def overflow_sample(wins):
    """The windows packed, in an image of at least the size at which the host picks OVERFLOW_NB."""
    smp = ac.pack_windows(wins)
    return padded(smp, max(smp.n_bases, min_bases_for(OVERFLOW_NB)))


# ---- E: count bins ---------------------------------------------------------------------------------------

BIN_COPIES = (1, 1, 2, 2, 31, 32, 32, 33, 34, 4094, 4095, 4095, 4096, 5000, 5000, 70000)
BIN_FILLER = 24
BIN_LIMITS = (1, 2, 3, 4, 5, sum(c >= 33 for c in BIN_COPIES), sum(c >= 33 for c in BIN_COPIES) + 1, 10**6)
BIN_SOLIDS = (1, 2, 32, 33, 4095, 4096, 5000, 5001, 70001)
BIN_N_WINDOWS = 3


@functools.lru_cache(maxsize=None)
def count_bins_case(k: int):
    """(windows (n, k), keys, copies): 40 distinct random k-mers that pass the low-complexity filter,
    as one-k-mer windows in BIN_COPIES copies plus singletons, shuffled; three more windows hold an N."""
    rng = random.Random(500 + k)
    thr = np.float32(lc_threshold(k))
    keys = []
    while len(keys) < len(BIN_COPIES) + BIN_FILLER:
        v = rng.randrange(1 << (2 * k))
        if v not in keys and v != all_t(k) and not host_ref.have_low_complexity(v, k, thr):
            keys.append(v)
    copies = list(BIN_COPIES) + [1] * BIN_FILLER
    w = one_kmer_windows(keys, k, copies)
    with_n = kmer_rows([rng.randrange(1 << (2 * k)) for _ in range(BIN_N_WINDOWS)], k)
    with_n[np.arange(BIN_N_WINDOWS), [0, k // 2, k - 1]] = 4
    w = np.concatenate([w, with_n])
    return w[np.random.default_rng(k).permutation(w.shape[0])], keys, copies


@functools.lru_cache(maxsize=None)
def count_bins_reference(k: int):
    return host_ref.count_kmers_dense(count_bins_case(k)[0], k, np.float32(lc_threshold(k)))


# ---- F: all-T key, N positions, score equality ---------------------------------------------------------------

ALL_T_KS = (16, 32)
ALL_T_COUNTS = (1, 2, 33, 4096)


@functools.lru_cache(maxsize=None)
def all_t_case(k: int, count: int):
    """(windows, other k-mers of the sample): `count` all-T k-mers -- half from one long T run, the
    rest from one-k-mer windows -- among 40 random windows."""
    fill = filler_windows(k, 40, seed=k + count, p_n=0.01)
    run = count // 2
    wins = fill[:20] + (["T" * (k + run - 1)] if run else []) + ["T" * k] * (count - run) + fill[20:]
    others = sorted({v for w in fill for v in window_kmers(w, k)} - {all_t(k)})
    return wins, others


N_POSITION_KS = (5, 16, 17, 32)


@functools.lru_cache(maxsize=None)
def n_position_case(k: int):
    """One random window of 80 bases 80 times, copy p with its only N at position p; two more copies
    with an N at both ends."""
    rng = random.Random(900 + k)
    w = cases.rand_seq(rng, 80)
    wins = [w[:p] + "N" + w[p + 1:] for p in range(80)]
    return wins + ["N" + w[1:-1] + "N"] * 2


SCORE_KS = (3, 4, 8, 15, 16, 17, 22, 31, 32)


def dimer_sum(kmer: int, k: int) -> int:
    """Sum of v (v - 1) over the 16 dimer counts of the k-mer (the numerator of getComplexity)."""
    counts = [0] * 16
    for _ in range(k - 1):
        counts[kmer & 15] += 1
        kmer >>= 2
    return sum(v * (v - 1) for v in counts)


@functools.lru_cache(maxsize=None)
def score_case(k: int):
    """(windows (n, k), thresholds): k-mers by construction -- homopolymers, period-2 and period-3
    repeats, a repeat followed by a random tail -- and 2,000 random ones, one window each; for three
    dimer sums S attained in the set, the threshold float32(S) / float32(2 (k - 2)) at which exactly
    the k-mers of sum S score equal, and the float32 just below and just above it.  Where the set
    attains five sums or more, the three are inner ones (the second smallest, the median, the second
    largest), so that every threshold keeps some k-mers and drops others; k = 3 attains only 0 and 2,
    k = 4 only 0, 2 and 6: those are taken as they are."""
    rng = random.Random(1300 + k)
    seqs = [b * k for b in "ACGT"]
    seqs += [((a + b) * k)[:k] for a in "ACGT" for b in "ACGT" if a != b]
    seqs += [((a + b + c) * k)[:k] for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    for unit in ("A", "C", "G", "T", "AC", "GT", "TA", "CG", "ACG", "TTG", "CAT", "GGA"):
        for head in sorted({k // 2, k - 2, k - 1, max(1, k // 3)}):
            for _ in range(2):
                seqs.append((unit * k)[:head] + cases.rand_seq(rng, k - head))
    seqs += [cases.rand_seq(rng, k) for _ in range(2000)]
    keys = [cases.kmer_value(s) for s in seqs]
    sums = sorted({dimer_sum(v, k) for v in keys})
    picked = [sums[1], sums[len(sums) // 2], sums[-2]] if len(sums) >= 5 else sums
    thresholds = []
    for s in picked:
        t = np.float32(s) / np.float32(2 * (k - 2))
        thresholds += [np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))]
    order = np.random.default_rng(k).permutation(len(keys))
    return one_kmer_windows(keys, k, [1] * len(keys))[order], thresholds, picked
