"""Case builders and expected values of the hit-level tests (ac_window_hits_*; DESIGN.md §4e "Hit levels"),
shared by tests/test_hits_cpu.py and tests/test_gpu_hits.py.

Expected values come from the oracle's plain DP distance (oracle.distance's C symbol, through
tests/test_budget_cpu.distances, which lifts oracle.distance's cap of 3 to E + 1):
hit_e[w][c] = d(kmer c, window w) <= e."""
import numpy as np

from tests import cases
from tests.test_budget_cpu import distances
from tests.test_gpu_bitslice import equal_case
from tests.test_gpu_budget import budget_case

GUARD = 64          # guard words after every hits buffer
FILL = 0xFFFFFFFF   # what every hits buffer holds before the launch


def expected_hits(k, kmers, windows, E):
    """(hit, counts): hit is bool (E + 1, n_windows, n_kmers), hit[e][w][c] = d(c, w) <= e; counts the
    M1(E) counts, their sum over levels and windows."""
    d = distances(k, kmers, windows, E + 1).T if len(kmers) and len(windows) else np.zeros((len(windows), len(kmers)), np.int64)
    hit = np.stack([d <= e for e in range(E + 1)])
    return hit, hit.sum(axis=(0, 1)).astype(np.uint64)


def pack_hits(hit):
    """bool (levels, n_windows, n_kmers) -> the matrix layout, uint32 (levels, n_windows, ceil(n_kmers / 32)):
    bit c % 32 of word c // 32."""
    hit = np.asarray(hit, dtype=bool)
    lv, nw, nk = hit.shape
    words = (nk + 31) // 32
    padded = np.zeros((lv, nw, words * 32), np.uint8)
    padded[:, :, :nk] = hit
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(lv, nw, words).astype(np.uint32)


def hits_case(seed, k, n_kmers, n_windows, L, E, p_n=0.01):
    """budget_case (equal windows, 1 % N, windows at exactly 3 edits where they fit) with its expected
    levels; at E = 3 the case must hold a pair at distance exactly 3 (asserted here, on the CPU)."""
    km, w = budget_case(seed, k, n_kmers, n_windows, L, p_n=p_n)
    hit, counts = expected_hits(k, km, w, E)
    if E == 3 and L >= k - 3:
        assert (hit[3] & ~hit[2]).any(), "no window at distance exactly 3"
    return km, w, hit, counts


__all__ = ["GUARD", "FILL", "expected_hits", "pack_hits", "hits_case", "equal_case", "budget_case", "cases"]
