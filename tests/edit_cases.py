"""Case builders and expected values of the edit-profile tests (ac_hit_edit_profile_device,
ac_window_edits_samples; DESIGN.md §4e "Edit profiles"), shared by tests/test_edits_cpu.py and
tests/test_gpu_edits.py.

Expected values: the definition as a plain full-table DP and the canonical traceback, every hit pair at once in
numpy, over the window strings and the matrices of tests.span_cases.expected_spans (hit levels and end
positions pinned to the oracle's distance, starts from the plain DP)."""
import functools
import random

import numpy as np

from tests import cases
from tests.flank_cases import matrices
from tests.span_cases import _codes, expected_spans, pack_hits, pack_positions, pack_starts

OPS = 12
BOUND = 3  # the pass's constant: |m - k| <= 3 and D[k][m] <= 3
MATCH, SUB, DEL, INS = 0, 1, 6, 7


def alignments(k, kmers, windows, hit_e, pos, start):
    """The definition over every pair of `hit_e` (bool (n_windows, n_kmers), one level plane; `pos` the
    exclusive end, `start` the inclusive start, int (n_windows, n_kmers), anything where there is no hit).
    Returns a dict: profile uint32 (n_kmers, k, 12); ws, cs the pairs' windows and k-mers; counted (bool per
    pair: every condition holds); dist D[k][m] (-1 where the text fails a condition before the table);
    begins_ins / ends_ins (bool per pair: the alignment's first / last operation in reading order is an
    insertion)."""
    hit_e = np.asarray(hit_e, bool)
    nw, nk = hit_e.shape
    out = np.zeros((nk, k, OPS), np.uint32)
    ws, cs = np.nonzero(hit_e)
    txt, pos, start = _codes(windows), np.asarray(pos), np.asarray(start)
    parts = [_aligned(k, kmers, txt, pos, start, ws[a:a + 4096], cs[a:a + 4096], out) for a in range(0, ws.size, 4096)]
    res = dict(profile=out, ws=ws, cs=cs)
    for x, name in enumerate(("counted", "dist", "begins_ins", "ends_ins")):
        res[name] = np.concatenate([pt[x] for pt in parts]) if parts else np.zeros(0, bool if name != "dist" else np.int64)
    return res


def _aligned(k, kmers, txt, pos, start, ws, cs, out):
    """alignments' body for the pairs (ws, cs): adds into `out`, returns (counted, dist, begins_ins, ends_ins)."""
    n, nk, L = ws.size, out.shape[0], txt.shape[1]
    p = pos[ws, cs].astype(np.int64)
    s = start[ws, cs].astype(np.int64)
    m = p - s
    ok = (p >= 1) & (p <= L) & (s >= 0) & (s < p) & (np.abs(m - k) <= BOUND)
    M = k + BOUND
    idx = s[:, None] + np.arange(M)[None, :]
    t = np.where(ok[:, None] & (idx < p[:, None]), txt[ws[:, None], np.clip(idx, 0, L - 1)], 9)  # (n, M); 9: past the text
    pat = np.array([[(int(v) >> (2 * (k - 1 - i))) & 3 for i in range(k)] for v in kmers], np.int64).reshape(nk, k)[cs]
    neq = (pat[:, :, None] != t[:, None, :]).astype(np.int64)  # (an N, 4, and the 9 match nothing)
    D = np.zeros((n, k + 1, M + 1), np.int64)
    D[:, 0, :] = np.arange(M + 1)
    D[:, :, 0] = np.arange(k + 1)
    for i in range(1, k + 1):
        for j in range(1, M + 1):
            D[:, i, j] = np.minimum(np.minimum(D[:, i - 1, j - 1] + neq[:, i - 1, j - 1], D[:, i - 1, j] + 1), D[:, i, j - 1] + 1)
    ar = np.arange(n)
    mm = np.where(ok, m, 0)
    dist = np.where(ok, D[ar, k, mm], -1)
    ok &= D[ar, k, mm] <= BOUND
    counted = ok.copy()
    i, j = np.full(n, k), mm.copy()
    ends_ins = np.zeros(n, bool)
    first = True
    while (ok & (i > 0)).any():
        act = ok & (i > 0)
        cur = D[ar, i, j]
        i1, j1 = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
        sym = np.minimum(t[ar, j1], 4)
        diag = act & (j > 0) & (D[ar, i1, j1] + neq[ar, i1, j1] == cur)
        dele = act & ~diag & (D[ar, i1, j] + 1 == cur)
        ins = act & ~diag & ~dele
        assert (j[ins] > 0).all()
        op = np.where(diag, np.where(neq[ar, i1, j1] == 0, MATCH, SUB + sym), np.where(dele, DEL, INS + sym))
        np.add.at(out, (cs[act], i1[act], op[act]), 1)
        if first:
            ends_ins, first = ins.copy(), False
        i = np.where(diag | dele, i - 1, i)
        j = np.where(diag | ins, j - 1, j)
    # (column j > 0 of row 0: bases inserted before the k-mer's first, not counted)
    return counted, dist, ok & (j > 0), ends_ins


def edit_profile_of(k, kmers, windows, hit_e, pos, start):
    """uint32 (n_kmers, k, 12): the definition (see alignments)."""
    return alignments(k, kmers, windows, hit_e, pos, start)["profile"]


def planted_windows(seed, k, kmers, n, L):
    """n windows of L random bases (no N), each holding one of `kmers` with its middle base replaced by an N
    (even windows) or with an N inserted before its middle base (odd windows), at a random place -- at base 0
    and at the window's end in the first four."""
    rng = random.Random(seed)
    out = []
    for x in range(n):
        c = cases.kmer_string(rng.choice(list(kmers)), k)
        h = k // 2
        t = (c[:h] + "N" + c[h + 1:]) if x % 2 == 0 else (c[:h] + "N" + c[h:])
        t = t[:L]
        at = 0 if x in (0, 1) else L - len(t) if x in (2, 3) else rng.randint(0, L - len(t))
        w = cases.rand_seq(rng, L)
        out.append(w[:at] + t + w[at + len(t):])
    return out


@functools.lru_cache(maxsize=None)
def edit_matrices(seed, k, n_kmers, n_windows, L, E, plants=6):
    """(kmers, windows, hit, pos, start, counts) of one case, built once and shared (left unchanged by its
    users): tests.flank_cases.matrices' windows and matrices, followed by `plants` planted_windows and
    theirs."""
    km, w, hit, pos, start, counts = matrices(seed, k, n_kmers, n_windows, L, E)
    if not plants or L < k + 1:
        return km, w, hit, pos, start, counts
    pw = planted_windows(seed + 29, k, [int(v) for v in km], plants, L)
    h2, p2, s2, c2, _ = expected_spans(k, [int(v) for v in km], pw, E)
    hit, pos, start = np.concatenate([hit, h2], axis=1), np.concatenate([pos, p2], axis=0), np.concatenate([start, s2], axis=0)
    for a in (hit, pos, start):
        a.setflags(write=False)
    return km, tuple(w) + tuple(pw), hit, pos, start, np.asarray(counts) + np.asarray(c2)


def distances(hit):
    """int (n_windows, n_kmers): the pair's distance from the level planes (levels where it is no hit)."""
    return hit.shape[0] - hit.sum(axis=0)


def properties(cases_):
    """What the cases [(k, kmers, windows, hit_e, pos, start)] hold, summed: the hit pairs, the totals of the
    12 op columns, and the pairs with start = 0 and with pos = L."""
    pairs, ops, edge = 0, np.zeros(OPS, np.uint64), dict(start0=0, posL=0)
    for k, km, w, hit_e, pos, start in cases_:
        L = len(w[0])
        pairs += int(hit_e.sum())
        ops += edit_profile_of(k, km, w, hit_e, pos, start).sum(axis=(0, 1), dtype=np.uint64)
        edge["start0"] += int((start[hit_e] == 0).sum())
        edge["posL"] += int((pos[hit_e] == L).sum())
    return pairs, ops, edge


def assert_properties(cases_, what):
    """The conditions that keep a test from passing on nothing: more than 300 pairs, every one of the 12 op
    columns non-zero over the case set, pairs with start = 0 and with pos = L."""
    pairs, ops, edge = properties(cases_)
    assert pairs > 300, (what, pairs)
    assert (ops > 0).all(), (what, ops)
    assert all(v > 0 for v in edge.values()), (what, edge)
    return pairs, ops, edge


__all__ = ["OPS", "alignments", "edit_profile_of", "planted_windows", "edit_matrices", "distances", "properties",
           "assert_properties", "expected_spans", "pack_hits", "pack_positions", "pack_starts", "matrices"]
