"""Case builders and expected values of the flank-profile tests (ac_hit_flank_profile_device,
ac_window_flanks_samples; DESIGN.md §4e "Flank profiles"), shared by tests/test_flanks_cpu.py and
tests/test_gpu_flanks.py.

Expected values: the definition in plain numpy, over the window strings and the matrices of
tests.span_cases.expected_spans (hit levels and end positions pinned to the oracle's distance, starts from the
plain DP)."""
import functools
import random

import numpy as np

from tests import cases
from tests.span_cases import _codes, expected_spans, pack_hits, pack_positions, pack_starts, plain_case, spans_case
from tests.test_bs_nfa_k import LISTED_K


def flank_profile_of(windows, hit_e, pos, start, depth):
    """uint32 (2, n_kmers, depth, 5): side 0 = right, 1 = left; A C G T N.  `hit_e` bool (n_windows, n_kmers),
    one level plane; `pos` int (n_windows, n_kmers) the exclusive end; `start` the inclusive start, or None:
    the left half is zeros.  A base outside [0, L) is not counted; a pair with pos outside 1..L or start
    outside 0..pos - 1 contributes to neither side."""
    hit_e = np.asarray(hit_e, bool)
    nw, nk = hit_e.shape
    out = np.zeros((2, nk, depth, 5), np.uint32)
    ws, cs = np.nonzero(hit_e)
    if not ws.size:
        return out
    txt = _codes(windows)
    L = txt.shape[1]
    p = np.asarray(pos)[ws, cs].astype(np.int64)
    ok = (p >= 1) & (p <= L)
    if start is not None:
        s = np.asarray(start)[ws, cs].astype(np.int64)
        ok &= (s >= 0) & (s < p)
    for j in range(depth):
        q = p + j
        m = ok & (q < L)
        np.add.at(out[0], (cs[m], j, txt[ws[m], q[m]]), 1)
        if start is not None:
            q = s - 1 - j
            m = ok & (q >= 0)
            np.add.at(out[1], (cs[m], j, txt[ws[m], q[m]]), 1)
    return out


def noisy_windows(seed, k, kmers, n_windows, L, E, p_n):
    """n_windows windows of L random bases, N at p_n, each with up to three of `kmers` at up to E random edits
    written over them side by side (plain_case's recipe over given k-mers)."""
    rng = random.Random(seed)
    out, slot = [], k + E + 2
    for _ in range(n_windows):
        w = cases.rand_seq(rng, L, p_n)
        for r in range(min(max(L // slot, 1), 3)):
            t = cases.mutate(rng, cases.kmer_string(rng.choice(list(kmers)), k), rng.randint(0, E))[:L]
            at = min(r * slot + rng.randint(0, 2), L - len(t))
            w = w[:at] + t + w[at + len(t):]
        out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def matrices(seed, k, n_kmers, n_windows, L, E, p_n=0.03):
    """(kmers, windows, hit, pos, start, counts) of one case, built once and shared (left unchanged by its
    users): plain_case at any k, after spans_case's windows at a k with a count kernel; the matrices are
    expected_spans' over all of them.  3 % N: at 1 % the bases beside the occurrences of some k hold none."""
    if k in LISTED_K:
        # spans_case's windows (occurrences at the word seams and the window's edges, inserted and missing bases;
        # almost no N near them), then as many with N at p_n beside occurrences of the same k-mers
        km, w = spans_case(seed, k, n_kmers, n_windows, L, E, p_n=p_n)[:2]
        w = list(w) + noisy_windows(seed + 17, k, km, n_windows, L, E, p_n)
    else:
        km, w = plain_case(seed, k, n_kmers, n_windows, L, E, p_n=p_n)
    hit, pos, start, counts, _ = expected_spans(k, km, w, E)
    for a in (hit, pos, start):
        a.setflags(write=False)
    return np.asarray(km, np.uint64), tuple(w), hit, pos, start, counts


def properties(cases_, depth):
    """What the cases [(windows, hit_e, pos, start)] hold for depth `depth`, summed: the hit pairs, the symbol
    totals of both sides (2, 5), and the pairs with start = 0, with pos = L, with a right flank cut by the
    window's end at 0 < j < depth and with a left flank cut by its start."""
    pairs, sym = 0, np.zeros((2, 5), np.uint64)
    edge = dict(start0=0, posL=0, right_cut=0, left_cut=0)
    for w, hit_e, pos, start in cases_:
        L = len(w[0])
        pairs += int(hit_e.sum())
        sym += flank_profile_of(w, hit_e, pos, start, depth).sum(axis=(1, 2), dtype=np.uint64)
        p, s = pos[hit_e].astype(int), start[hit_e].astype(int)
        edge["start0"] += int((s == 0).sum())
        edge["posL"] += int((p == L).sum())
        edge["right_cut"] += int(((L - p > 0) & (L - p < depth)).sum())
        edge["left_cut"] += int(((s > 0) & (s < depth)).sum())
    return pairs, sym, edge


def assert_properties(cases_, depth, what):
    """The conditions that keep a test from passing on nothing (tests/test_flanks_cpu.py)."""
    pairs, sym, edge = properties(cases_, depth)
    assert pairs > 300, (what, pairs)
    assert (sym > 0).all(), (what, sym)
    assert all(v > 0 for v in edge.values()), (what, edge)
    return pairs, sym, edge


__all__ = ["flank_profile_of", "matrices", "properties", "assert_properties", "expected_spans", "pack_hits", "pack_positions",
           "pack_starts", "plain_case", "spans_case"]
