"""Case builders of the word-parallel count kernel's equal-window tests (tests/test_gpu_word_parallel.py),
shared with their CPU companion (tests/test_word_cases.py), which shows on the oracle alone that every
case has the property its GPU test relies on.  Builders are cached: a case and its oracle counts are
computed once per process and must not be changed by a test.

The kernel is wm2_count_kernel<P, STAGED, EQ> (approx_counter_amd/csrc/wm_count.hip): P candidates per
lane word, P = 1, 2, 3, 4 for k = 17..32, 11..16, 9..10, 2..8 (wm_count.h pack_factor)."""
import functools
import os
import re

import numpy as np

import approx_counter_amd as ac
import oracle
from tests import cases
from tests.test_gpu_bitslice import equal_case
from tests.test_gpu_bs_routes import chunk_of
from tests.test_gpu_jobs import _kmers_from, _n_record_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WP_K = (8, 10, 15, 17)  # one k per P, each a k at which this kernel is the production kernel
EDGE_K = (10, 15, 17)   # 15 and 17 skip hit accumulation over a window's first bases (skip_first)


# ---- the kernel's geometry (wm_count.h) and the inline N records (nrec.h), restated ----

def pack_factor(k):
    return min(32 // k, 4)


def group_size(k, staged):
    """cands_per_wave: 64 lanes x P candidates x lane words (two for P = 2, and for staged P = 1)."""
    P = pack_factor(k)
    return 64 * P * (2 if P == 2 or (P == 1 and staged) else 1)


def groups_of(k, n_kmers, staged):
    return -(-n_kmers // group_size(k, staged))


def nrec_bits(L):
    S = (L + 31) & ~31
    pad = S - L
    R, pb = 2 * min(pad, 16), (7 if S <= 128 else 8)
    return 0 if (L == 0 or L > 256 or R < 3 + pb) else R


def nrec_cap(L):
    """N positions that a window's inline record holds; a window with more overflows it."""
    R, pb = nrec_bits(L), (7 if ((L + 31) & ~31) <= 128 else 8)
    return min(4, (R - 3) // pb) if R else 0


def nrec_header_claims():
    """[(function name, L, value)] of the nrec_bits(L) == v and nrec_cap(L) == v terms in nrec.h's
    static_assert lines."""
    text = open(os.path.join(ROOT, "approx_counter_amd", "csrc", "nrec.h")).read()
    lines = [ln for ln in text.splitlines() if ln.startswith("static_assert")]
    found = [m for ln in lines for m in re.findall(r"nrec_(bits|cap)\((\d+)\) == (\d+)", ln)]
    return lines, [(f, int(L), int(v)) for f, L, v in found]


# ---- 1: every EQ instantiation ----

@functools.lru_cache(maxsize=None)
def basic_case(k):
    """300 candidates, 37 windows of 100 bases with 1 % N: (kmers, windows, oracle counts)."""
    km, w = equal_case(7100 + k, 300, 37, 100, k=k)
    return km, w, oracle.count_myers(k, km, w)


# ---- 2: window lengths ----

def lengths_for(k):
    return sorted({k - 3, k - 2, k, k + 2, 14, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100, 101, 127, 128, 129,
                   150, 151, 255, 256, 257, 300, 512, 513})


LONG_L = (257, 300, 512)  # more than one 256-base fetch: the word-parallel kernel at k = 16 and 22 too


def short_occurrence(kmer, k):
    """Candidate `kmer` with two bases deleted: k - 2 bases, exactly 2 edits from it."""
    s = cases.kmer_string(int(kmer), k)
    a, b = k // 3, 2 * k // 3
    return s[:a] + s[a + 1:b] + s[b + 1:]


@functools.lru_cache(maxsize=None)
def length_case(k, L):
    """100 candidates, 70 windows of L bases with 2 % N.  The first window starts with candidate 0 less
    two bases (cut to L), so that occurrence ends at base k - 3 of the window; the last window ends
    with the same k - 2 bases.  (kmers, windows, oracle counts)."""
    km, w = equal_case(7300 + 600 * k + L, 100, 70, L, p_n=0.02, k=k)
    occ = short_occurrence(km[0], k)
    w[0] = (occ + w[0][len(occ):])[:L]
    w[-1] = (w[-1][:max(0, L - len(occ))] + occ)[-L:]
    assert all(len(x) == L for x in w)
    return km, w, oracle.count_myers(k, km, w)


# ---- 3: inline N records ----

RECORD_L = (100, 101, 150, 151, 128, 16, 40)
RECORD_COUNTS = (0, 1, 0, 2, 0, 3, 4, 0, 5, 6, 1)


def record_spots(L):
    return (0, 15, 16, 31, 32, 63, 64, L - 1)


def edge_spots(L):
    return [p for p in dict.fromkeys(record_spots(L)) if p < L]


@functools.lru_cache(maxsize=None)
def record_jobs(k, L):
    """The three jobs of test_gpu_jobs.py::test_inline_n_records with k-mers of k bases: windows with 0..6 N
    (the first ones on the N-mask words' edges), a job whose only N-holders overflow, an N-free job (its
    k-mers: 44 of its own windows and 20 of the first job's).  In the first job a record that holds its
    window's N holds the first spots only (0 and 15 where it holds one or two); so a fourth job has, per
    spot, windows with one N there and windows with two, there and at the next spot: records that hold
    every spot, in every N-mask word, at both position widths.  [(kmers, 2-D windows, oracle counts)]."""
    ws = _n_record_windows(L, 3000, L, list(RECORD_COUNTS), spots=record_spots(L))
    over = _n_record_windows(L + 1, 900, L, [0, 0, 7])
    clean = _n_record_windows(L + 2, 700, L, [0])
    sp = edge_spots(L)
    edges = np.concatenate([_n_record_windows(L + 10 + i, 30, L, [1, 2, 0], spots=(p, sp[(i + 1) % len(sp)]))
                            for i, p in enumerate(sp)])
    kmers = _kmers_from(ws, 300, seed=L + k, k=k)
    km2 = np.concatenate([_kmers_from(over, 100, seed=L + k + 1, k=k), kmers[:20]])
    km3 = np.concatenate([_kmers_from(clean, 44, seed=L + k + 2, k=k), kmers[:20]])
    km4 = _kmers_from(edges, 100, seed=L + k + 3, k=k)
    return [(km, w, oracle.count_myers(k, km, np.minimum(w, 4), 16))
            for km, w in ((kmers, ws), (km2, over), (km3, clean), (km4, edges))]


# ---- 4: candidate-group and window-count edges ----

CAND_COUNTS = {17: (1, 33, 63, 64, 65, 127, 128, 129, 257), 15: (1, 33, 255, 256, 257, 513),
               10: (1, 33, 191, 192, 193, 385), 8: (1, 33, 255, 256, 257, 513)}
WINDOW_COUNTS = (1, 2, 3, 4, 5, 65)


@functools.lru_cache(maxsize=None)
def group_case(k, n_kmers, n_windows=37, L=100):
    """n_kmers candidates over equal windows of L bases, 1 % N; window 0 holds the last candidate and the
    last window the first one, so the first lane of the first group and the last lane of the last group
    expect hits.  (kmers, windows, oracle counts)."""
    km, w = equal_case(7500 + 40 * n_kmers + k + n_windows, n_kmers, n_windows, L, k=k)
    w[0] = w[0][:10].replace("N", "A") + cases.kmer_string(int(km[-1]), k) + w[0][10 + k:]
    w[-1] = w[-1][:L - k - 5] + cases.kmer_string(int(km[0]), k) + w[-1][L - 5:].replace("N", "C")
    assert all(len(x) == L for x in w)
    return km, w, oracle.count_myers(k, km, w)


# ---- 5: items of more than one window ----

# (k, candidates, L): (seed, n_texts) at which dictionary_case's own assertions hold
DICT_SEEDS = {(17, 640, 20): (1, 121), (15, 1300, 20): (1, 247), (17, 40, 33): (3, 61),
              (17, 1300, 100): (1, 247), (10, 2600, 100): (1, 247)}


@functools.lru_cache(maxsize=None)
def item_dictionary(k, n_kmers, L):
    seed, n_texts = DICT_SEEDS[(k, n_kmers, L)]
    return cases.dictionary_case(seed, n_kmers, L, n_texts=n_texts,
                                 n_per_text=cases.SHORT_N if L < 100 else cases.N_PER_TEXT, k=k)


def item_windows(W, chunk, groups):
    """The window count of a sample over `groups` candidate groups whose launch of W waves takes items of
    `chunk` windows: 13 + 64 x chunk items per wave and more (an item of this kernel is one window of
    one group), not a multiple of chunk, so the last item of every group is partial."""
    n = -(-(W * (64 * chunk + 13) + 1) // groups)
    while chunk > 1 and n % chunk == 0:
        n += 1
    assert chunk_of(groups * n, W) == chunk, (W, chunk, groups, n)
    return n


def fused_windows(W, chunk, groups_a, groups_b):
    """Window counts (na, na // 10) of two fused segments at `chunk`, neither a multiple of it."""
    first = (W * (64 * chunk + 13) + 1) * 10 // (10 * groups_a + groups_b)
    for na in range(first, first + 4096):
        if chunk_of(groups_a * na + groups_b * (na // 10), W) == chunk and na % chunk and (na // 10) % chunk:
            return na, na // 10
    raise AssertionError("no window counts with these properties")


# ---- 6: device packing ----

PACK_K = (10, 15, 17)
PACK_L = (33, 100, 101, 128, 151, 256)


@functools.lru_cache(maxsize=None)
def pack_case(k, L):
    """300 candidates, 1,500 windows of L bases with 2 % N: (kmers, windows, oracle counts)."""
    km, w = equal_case(7700 + 300 * k + L, 300, 1500, L, p_n=0.02, k=k)
    return km, w, oracle.count_myers(k, km, w, 16)


@functools.lru_cache(maxsize=None)
def pack_overflow_case(k, L=100):
    """The shape of test_gpu_device_pack.py::test_device_pack_record_overflow_and_n_runs at k: 6 % N, an
    all-N window, a run of 40 N, N at both ends, N bytes of 4, 5, 77 and 255.
    (kmers, windows as strings, the Dna5 sample with those bytes, oracle counts)."""
    km, w = equal_case(7900 + k, 400, 2000, L, p_n=0.06, k=k)
    w[5] = "N" * L
    w[6] = w[6][:30] + "N" * 40 + w[6][70:]
    w[7] = "N" + w[7][1:-1] + "N"
    s = ac.Dna5Sample.from_windows(w)
    b = s.bases.copy()
    b[b == 4] = np.array([4, 5, 77, 255], np.uint8)[np.arange(int((b == 4).sum())) % 4]  # any ordinal >= 4 is N
    return km, w, ac.Dna5Sample(b, s.offset, s.length), oracle.count_myers(k, km, w, 16)


TAIL_SHAPES = ((1, 151), (2, 101), (3, 150), (1, 100))


def tail_case(k, n_windows, L):
    """test_gpu_device_pack_tail.py's case at k: every window ends with the k-mer, which then ends the block."""
    kmer = "ACGTACGTTGCAAGCTGATTACAGGCATTCAG"[:k]
    km = np.array([cases.kmer_value(kmer), cases.kmer_value("T" * k)], np.uint64)
    return km, [("C" * L)[:L - k] + kmer for _ in range(n_windows)]
