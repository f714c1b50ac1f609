"""Designed contents for the approximate count's kernels (DESIGN.md §4e "Which file covers which kernel"):
near-misses at distance exactly E + 1, low-complexity and periodic candidates, and related candidates (the
overlapping k-mers of one adapter), shared by tests/test_nfa_cases.py (CPU: each builder's property, the
host harnesses) and tests/test_gpu_nfa_cases.py (GPU).  The other case builders draw random candidates and
random text, where a pair sits within the planted 3 edits or far above 4; these place pairs on the boundary,
keep every row of the automaton busy and reach a window's minimum at many end positions.

Everything is deterministic (seeded by k and the shape).  Every expected value is the plain DP's:
tests.test_budget_cpu.distances / counts_from (the oracle's distance, pinned at E = 2 to oracle.count_myers),
tests.positions_cases.expected_positions (a Sellers DP's last row, its minimum pinned to that distance) and
oracle.count_dp.  A builder asserts the population its GPU test relies on; if one falls short at some k,
enlarge the case, not the threshold."""
import functools
import itertools
import random

import numpy as np

import oracle
from tests import cases
from tests.positions_cases import expected_positions, last_rows
from tests.test_budget_cpu import counts_from, distances

ALPH = "ACGT"
KINDS = ("sub", "ins", "del")
PLACEMENTS = ("head", "tail", "split", "spread", "middle")
UNITS = {2: "AC", 3: "ACG", 4: "ACGT", 5: "AACGT", 6: "AACCGT", 7: "AACGGTT", 8: "AACCGGTT"}
MIN_PAIRS, MIN_PADDED, MIN_TIED, MIN_OVERWRITTEN, MAX_TIE_WINDOWS = 200, 100, 500, 100, 800


# ---- edits ------------------------------------------------------------------------------------------

def _other(c, n=0):
    """A base that is not c: the n-th of the other three."""
    return ALPH[(ALPH.index(c) + 1 + n % 3) % 4]


def apply_edits(s, edits):
    """`edits`: (kind, position in s, base) with distinct positions; "sub" replaces s[p] by the base, "del"
    removes s[p], "ins" puts the base in front of s[p] (p = len(s): at the end)."""
    t = list(s)
    for kind, p, b in sorted(edits, key=lambda e: -e[1]):
        if kind == "sub":
            t[p] = b
        elif kind == "del":
            del t[p]
        else:
            t.insert(p, b)
    return "".join(t)


def single_edits(s):
    """(kind, position, string) of every single edit: the 3 substitutions and the deletion of every position,
    the 4 insertions at every gap 0..k.  The edited (or inserted) base is string[position]; for a deletion
    string[position] is the base after the gap."""
    out = []
    for p, c in enumerate(s):
        out += [("sub", p, apply_edits(s, [("sub", p, _other(c, n))])) for n in range(3)]
    out += [("del", p, apply_edits(s, [("del", p, "")])) for p in range(len(s))]
    out += [("ins", p, apply_edits(s, [("ins", p, b)])) for p in range(len(s) + 1) for b in ALPH]
    return out


def placement(k, n, where):
    """The n positions (n <= k - 2) of a placement."""
    if where == "head":
        return list(range(n))
    if where == "tail":
        return list(range(k - n, k))
    if where == "split":
        h = (n + 1) // 2
        return list(range(h)) + list(range(k - (n - h), k))
    if where == "spread":
        return [1 + i * (k - 3) // (n - 1) for i in range(n)]
    return list(range((k - n) // 2, (k - n) // 2 + n))


def multi_edits(s, n_max):
    """(name, string) for n = 2..n_max edits: every combination of kinds at the five placements.  A substitute
    is another base than the one replaced, an inserted base another than the one it goes in front of."""
    k = len(s)
    out = []
    for n in range(2, min(n_max, k - 2) + 1):
        for where in PLACEMENTS:
            pos = placement(k, n, where)
            assert len(set(pos)) == n and 0 <= min(pos) and max(pos) < k, (k, n, where)
            for kinds in itertools.product(KINDS, repeat=n):
                edits = [(kd, p, _other(s[p], i + p)) for i, (kd, p) in enumerate(zip(kinds, pos))]
                out.append((f"{where}:{'+'.join(kinds)}", apply_edits(s, edits)))
    return out


def neighbourhood(s, n_max):
    """Strings at a designed small distance from the k-mer string s (see single_edits and multi_edits), in a
    fixed order, without duplicates."""
    return list(dict.fromkeys([t for _, _, t in single_edits(s)] + [t for _, t in multi_edits(s, n_max)]))


# ---- candidates -------------------------------------------------------------------------------------

def periodic(unit, phase, n):
    return "".join(unit[(phase + i) % len(unit)] for i in range(n))


def low_complexity(k):
    """Homopolymers, every phase of a repeat of period 2..8, two-run k-mers X^i Y^(k - i), and a homopolymer
    with one foreign base in the middle: k-mer strings, duplicates removed."""
    out = [c * k for c in ALPH]
    for p, unit in UNITS.items():
        out += [periodic(unit, ph, k) for ph in range(p)]
    out += ["A" * i + "C" * (k - i) for i in (1, 2, 3, k // 2, k - 3, k - 2, k - 1) if 0 < i < k]
    out.append("G" * (k // 2) + "T" + "G" * (k - k // 2 - 1))
    return list(dict.fromkeys(out))


def tiles(adapter, k):
    return [adapter[i:i + k] for i in range(len(adapter) - k + 1)]


def adapter_of(k):
    return cases.rand_seq(random.Random(7100 + k), k + 12)


def randoms_of(k, n=6):
    rng = random.Random(7200 + k)
    return [cases.rand_seq(rng, k) for _ in range(n)]


def candidates(k):
    """K-mer strings: low_complexity(k), 6 random k-mers and the 13 tiles of adapter_of(k), ordered so that the
    tiles are neighbours (they share lane words of the word-parallel kernel) and a second copy of them lies 32
    places further on (the same bits of the next block of the bit-sliced kernel)."""
    lc, rnd, tl = low_complexity(k), randoms_of(k), tiles(adapter_of(k), k)
    rest = lc + rnd
    at = len(rest) - 32 + len(tl)  # the tiles' place: the copy, 32 further on, ends the list
    assert at >= 0 and len(tl) <= 32
    out = rest[:at] + tl + rest[at:] + tl
    assert out[at:at + 13] == out[at + 32:at + 45] == tl and len(out) <= 80
    return out, at


def probes(k):
    """The k-mer strings whose neighbourhoods become windows: two random k-mers, A^k, a period-2 and a period-3
    k-mer and a two-run k-mer."""
    return randoms_of(k)[:2] + ["A" * k, periodic("AC", 0, k), periodic("ACG", 1, k), "A" * (k // 2) + "C" * (k - k // 2)]


def near_miss_inputs(k):
    """(k-mer values, windows) of near_miss_case, without the DP pass."""
    km, _ = candidates(k)
    w = []
    for s in probes(k):
        w += neighbourhood(s, 4)
    for s in low_complexity(k):
        w += [(s * 3)[:n] for n in range(max(k - 4, 1), k + 5)]
    ad = adapter_of(k)
    w += [ad[i:] for i in range(len(ad))] + [ad[:len(ad) - i] for i in range(len(ad))]
    w = [x for x in dict.fromkeys(w) if x]
    return [cases.kmer_value(s) for s in km], w


def populations(d):
    """Pairs at each exact distance 0..4."""
    return [int((d == e).sum()) for e in range(5)]


def assert_boundaries(k, km, w, d, least=MIN_PAIRS):
    pop = populations(d)
    assert min(pop) >= least, (k, pop)
    for E in range(4):
        lower = counts_from(d, E - 1) if E else np.zeros(len(km), np.uint64)
        assert 2 * int((counts_from(d, E) != lower).sum()) >= len(km), (k, E)


@functools.lru_cache(maxsize=None)
def near_miss_case(k):
    """(kmers, windows, d): candidates(k) against ragged windows of 1..k + 12 bases -- the neighbourhoods of
    probes(k), every low-complexity k-mer repeated three times and cut to k - 4..k + 4 bases, and the adapter
    cut at every offset from both ends; d = distances(..., 5).  At most 80 k-mers by 5,000 windows.
    Asserts at least 200 pairs at each exact distance 0..4, that every budget's count differs from the one
    below it for at least half of the k-mers, and that the DP at E = 2 is oracle.count_myers."""
    km, w = near_miss_inputs(k)
    assert len(km) <= 80 and len(w) <= 5000, (k, len(km), len(w))
    d = distances(k, km, w, 5)
    assert_boundaries(k, km, w, d)
    np.testing.assert_array_equal(counts_from(d, 2), oracle.count_myers(k, km, w))
    d.setflags(write=False)
    return km, w, d


# ---- equal windows ----------------------------------------------------------------------------------

def equalised(windows, L, side):
    """Every window at exactly L bases: seeded random bases after it (side "start": the occurrence begins at
    base 0) or in front of it ("end": it ends at base L); a longer window keeps that end's L bases."""
    assert side in ("start", "end")
    rng = random.Random(7300 + L + (side == "end"))
    out = []
    for w in windows:
        pad = cases.rand_seq(rng, max(L - len(w), 0))
        out.append((w + pad)[:L] if side == "start" else (pad + w)[-L:] if L else "")
    return out


def assert_padded(k, d, least=MIN_PADDED):
    for E in range(4):
        assert int((d == E + 1).sum()) >= least and int((d <= E).sum()) >= least, (k, E, populations(d))


@functools.lru_cache(maxsize=None)
def equalised_case(k, side):
    """near_miss_case(k) with its windows equalised to k + 9 bases: (kmers, windows, d), the DP run again on the
    padded windows.  Asserts at least 100 pairs at d = E + 1 (and within E) for every E."""
    km, w, _ = near_miss_case(k)
    w = equalised(w, k + 9, side)
    d = distances(k, km, w, 5)
    assert_padded(k, d)
    d.setflags(write=False)
    return km, w, d


def whole_window_groups(windows):
    """{L: windows of exactly L bases}: each group is an equal-window part of its own, the window being the
    whole occurrence (below k bases only deletions can hit)."""
    out = {}
    for w in windows:
        out.setdefault(len(w), []).append(w)
    return out


@functools.lru_cache(maxsize=None)
def whole_window_case(k):
    """(kmers, [(L, windows, d)]) of near_miss_case(k)'s windows of k - 4..k + 4 bases.  Asserts that every group
    holds windows, that at k - 4 bases nothing is within 3 edits, and the boundary populations over the groups."""
    km, w, d = near_miss_case(k)
    at = {x: i for i, x in enumerate(w)}
    by_len = whole_window_groups(w)
    groups = [(L, by_len[L], d[:, [at[x] for x in by_len[L]]]) for L in range(k - 4, k + 5)]
    assert all(len(ws) >= 20 for _, ws, _ in groups), [(L, len(ws)) for L, ws, _ in groups]
    assert groups[0][0] == k - 4 and (groups[0][2] >= 4).all() and (groups[1][2] >= 3).all()
    assert_padded(k, np.concatenate([g[2] for g in groups], axis=1))
    return km, groups


# ---- ties --------------------------------------------------------------------------------------------

def thinned(k, step=7):
    """Every `step`-th neighbourhood string of one random and one periodic k-mer."""
    return (neighbourhood(randoms_of(k)[0], 4) + neighbourhood(periodic("ACG", 1, k), 4))[::step]


def occurrences(k):
    """thinned(k), the two k-mers themselves and the 13 tiles: what the seam and block-end windows hold."""
    return thinned(k) + [randoms_of(k)[0], periodic("ACG", 1, k)] + tiles(adapter_of(k), k)


def tie_inputs(k, L):
    km, _ = candidates(k)
    rng = random.Random(7400 + 300 * k + L)
    fill = lambda n: cases.rand_seq(rng, max(n, 0))  # noqa: E731
    w = []
    for s in low_complexity(k):
        text = (s * (L // k + 2))
        w.append(text[:L])
        w.append((text[:L // 2] + text[L // 2 + 1:])[:L])
        w.append(text[:L // 3] + _other(text[L // 3]) + text[L // 3 + 1:L])
        w.append((fill(L - (k - 1)) + s[:-1])[-L:])
        w.append((s[1:] + fill(L - (k - 1)))[:L])
    for t in thinned(k):
        w.append((t + fill(L - len(t)))[:L])
        w.append((fill(L - len(t)) + t)[-L:])
    ad = adapter_of(k)
    for off in range(max(L - len(ad), 0) + 1):
        w.append((fill(off) + ad + fill(L - off - len(ad)))[:L])
    w = list(dict.fromkeys(w))
    assert all(len(x) == L for x in w)
    return [cases.kmer_value(s) for s in km], w


def tie_counts(e, E):
    """(tied, overwritten) pairs of last rows e (n_windows, n_kmers, L + 1) at budget E: within E and at their
    minimum at more than one end; an end within E but worse than the best before the first best end."""
    d = e.min(axis=2)
    hit = d <= E
    best = e == d[:, :, None]
    first = best.argmax(axis=2)
    before = np.arange(e.shape[2])[None, None, :] < first[:, :, None]
    return int((hit & (best.sum(axis=2) > 1)).sum()), int((hit & ((e <= E) & before).any(axis=2)).sum())


@functools.lru_cache(maxsize=None)
def tie_rows(k, L):
    """last_rows of tie_inputs(k, L): int16 (n_windows, n_kmers, L + 1)."""
    e = last_rows(k, *tie_inputs(k, L))
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def tie_case(k, L):
    """(kmers, windows, hit, pos, tied, overwritten): at most 800 equal windows of L bases -- per low-complexity
    k-mer its periodic text, that text with a base deleted at L / 2 and with a base changed at L / 3, the k-mer
    without its last base at the window's end and without its first at the start; every seventh neighbourhood
    string at both ends; the adapter at every offset -- with expected_positions at E = 3 (expected(...) cuts it
    down to a smaller budget).  tied / overwritten: tie_counts per E = 0..3.  Asserts at least 500 pairs within 3
    edits that reach their minimum at more than one end and at least 100 with a worse earlier end within E; and
    a tie at every budget, an overwritten position at every budget but 0 (where there is none)."""
    km, w = tie_inputs(k, L)
    assert len(w) <= MAX_TIE_WINDOWS and len(km) <= 80, (k, L, len(w))
    hit, pos, _ = expected_positions(k, km, w, 3)
    e = tie_rows(k, L)
    both = [tie_counts(e, E) for E in range(4)]
    tied, over = [b[0] for b in both], [b[1] for b in both]
    assert tied[3] >= MIN_TIED and over[3] >= MIN_OVERWRITTEN, (k, L, tied, over)
    assert min(tied) > 0 and min(over[1:]) > 0 and over[0] == 0, (k, L, tied, over)
    return km, w, hit, pos, tied, over


def expected(case, E):
    """(hit, pos, counts) of a tie_case at budget E <= 3: the levels up to E; the position -- the first end at
    the least distance, whatever the budget -- where that distance is within E."""
    hit, pos = case[2][:E + 1], np.where(case[2][E], case[3], -1).astype(np.int16)
    return hit, pos, hit.sum(axis=(0, 1)).astype(np.uint64)


def last_end_positions(e, E):
    """The mutated rule on last rows e: the last end at the least distance instead of the first."""
    d = e.min(axis=2)
    last = e.shape[2] - 1 - (e[:, :, ::-1] == d[:, :, None]).argmax(axis=2)
    return np.where(d <= E, last, -1).astype(np.int16)


# ---- seams and block ends ---------------------------------------------------------------------------

SEAM_ENDS = ((300, (254, 255, 256, 257, 258)), (520, (510, 512, 513)), (257, (257,)))


def seam_inputs(k):
    rng = random.Random(7500 + k)
    w = []
    for t in occurrences(k):
        for L, ends in SEAM_ENDS:
            for end in ends:
                w.append(cases.rand_seq(rng, end - len(t)) + t + cases.rand_seq(rng, L - end))
    assert all(len(x) in (300, 520, 257) for x in w) and len(w) <= 5000
    return w


@functools.lru_cache(maxsize=None)
def seam_case(k):
    """(kmers, windows, counts at E = 2) for the word-parallel kernel: occurrences(k) inside windows of 300 and
    520 random bases, ending exactly at base 254..258 and 510, 512, 513 -- both sides of the 256-base fetch seam
    and of the second one -- and at the very end of a 257-base window.  Ragged."""
    km, at = candidates(k)
    km = [cases.kmer_value(s) for s in km]
    w = seam_inputs(k)
    want = oracle.count_dp(k, km, w)
    assert (want[at:at + 13] > 0).all() and (want[at + 32:at + 45] > 0).all() and int((want > 0).sum()) >= 30
    return km, w, want


def block_end_lengths(k):
    L0 = 4 * ((k + 20 + 3) // 4) + 1
    return [L0, L0 + 1, L0 + 2, L0 + 3]


def block_end_inputs(k):
    rng = random.Random(7600 + k)
    out = []
    for L in block_end_lengths(k):
        w = []
        for t in occurrences(k):
            w += [cases.rand_seq(rng, L - back - len(t)) + t + cases.rand_seq(rng, back) for back in range(4)]
            w.append(t + cases.rand_seq(rng, L - len(t)))
        assert all(len(x) == L for x in w)
        out.append((L, w))
    return out


@functools.lru_cache(maxsize=None)
def block_end_case(k):
    """(kmers, [(L, windows, d)]) for the bit-sliced kernel: four consecutive window lengths from
    4 ceil((k + 20) / 4) + 1 on -- every fill of the last 4-base block, both parities of the base pairs -- each
    an equal-window part; every string of occurrences(k) ends at base L, L - 1, L - 2 and L - 3, and starts
    at base 0.  Asserts per part pairs at d = E + 1 and within E for every E."""
    km, _ = candidates(k)
    km = [cases.kmer_value(s) for s in km]
    parts = []
    for L, w in block_end_inputs(k):
        d = distances(k, km, w, 5)
        assert_padded(k, d, 50)
        parts.append((L, w, d))
    return km, parts


# ---- N ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def n_case(k, L=100):
    """(kmers, windows, d, d_clean): every fifth single-edit string of a random and a periodic k-mer (and every
    ninth of their strings of 2..4 edits, the two k-mers and the tiles, for the other distances) in the middle
    of L random bases, with an N at the edited base (of those: the middle one), at the base before the occurrence,
    at the base after it, and with 5 and 6 N in the window (the edited base, both neighbours of the occurrence and
    bases further out: more than a 100-base window's inline N record holds).  d_clean: the distances of the same windows before the
    N went in.  Asserts that the N change the counts at every budget, and the boundary populations."""
    km, _ = candidates(k)
    km = [cases.kmer_value(s) for s in km]
    w, clean = n_inputs(k, L)
    assert max(x.count("N") for x in w) == 6 and sum(x.count("N") == 5 for x in w) >= 10
    d, d_clean = distances(k, km, w, 5), distances(k, km, clean, 5)
    for E in range(4):
        assert (counts_from(d, E) != counts_from(d_clean, E)).any(), (k, E)
        assert int((d == E + 1).sum()) >= 20 and int((d <= E).sum()) >= 20, (k, E, populations(d))
    return km, w, d, d_clean


def n_inputs(k, L=100):
    """(windows, the same windows before the N went in) of n_case."""
    rng = random.Random(7700 + k)
    w, clean = [], []
    held = [(len(t) // 2, t) for t in tiles(adapter_of(k), k)]
    for s in (randoms_of(k)[0], periodic("ACG", 1, k)):
        held += [(k // 2, s)] + [(p, t) for _, p, t in single_edits(s)[::5]]
        held += [(len(t) // 2, t) for _, t in multi_edits(s, 4)[::9]]
    for p, t in held:
        a = (L - len(t)) // 2
        text = cases.rand_seq(rng, a) + t + cases.rand_seq(rng, L - a - len(t))
        at, far = a + min(p, len(t) - 1), [a - 1, a + len(t), 0, L - 1, a - 9, a + len(t) + 8]
        for spots in ([at], [a - 1], [a + len(t)], [at] + far[:4], [at] + far[:5]):
            assert len(set(spots)) == len(spots) and all(0 <= x < L for x in spots)
            clean.append(text)
            w.append("".join("N" if i in spots else c for i, c in enumerate(text)))
    return w, clean


# ---- exhaustive ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exhaustive_small(k):
    """(kmers, windows, counts at E = 2), k = 2, 3, 4: all 4^k candidates against every ACGT text of 0..k + 3
    bases and every text of k + 1 bases with one base replaced by N; the counts are oracle.count_dp's."""
    assert 2 <= k <= 4
    km = list(range(4 ** k))
    w = ["".join(t) for n in range(k + 4) for t in itertools.product(ALPH, repeat=n)]
    for p in range(k + 1):
        w += ["".join(t[:p]) + "N" + "".join(t[p:]) for t in itertools.product(ALPH, repeat=k)]
    return km, w, oracle.count_dp(k, km, w)
