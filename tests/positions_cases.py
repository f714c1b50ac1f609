"""Case builders and expected values of the match-end-position tests (ac_window_positions_*; DESIGN.md §4e
"Match end positions"), shared by tests/test_positions_cpu.py and tests/test_gpu_positions.py.

Expected values come from a numpy Sellers DP that keeps its whole last row: e(j), j = 0..L, the least edit
distance of the whole k-mer against a substring of the window that ends at base j (an N matches nothing).
Its minimum over j is asserted equal to tests.test_budget_cpu.distances -- the oracle's plain DP -- on every
case built here: that assertion is the anchor to the oracle.  pos = the first j at which e(j) is that minimum."""
import numpy as np

from tests import cases
from tests.hits_cases import FILL, GUARD, pack_hits
from tests.test_budget_cpu import distances
from tests.test_gpu_budget import budget_case

CODE = {c: i for i, c in enumerate("ACGT")}


def last_rows(k, kmers, windows):
    """int16 (n_windows, n_kmers, L + 1): the last row of the Sellers DP of every (window, k-mer) pair;
    `windows` are strings, or Dna5 arrays (4 = N), of one length L.  Vectorised over the pairs; the column recurrence's in-column
    term (a deletion from the k-mer's side) is a running minimum."""
    nk, nw = len(kmers), len(windows)
    L = len(windows[0]) if nw else 0
    pat = np.array([[(int(v) >> (2 * (k - 1 - i))) & 3 for i in range(k)] for v in kmers], np.int16).reshape(nk, k)
    txt = np.array([[CODE.get(c, 4) for c in w] if isinstance(w, str) else np.asarray(w) for w in windows],
                   np.int16).reshape(nw, L)
    col = np.broadcast_to(np.arange(k + 1, dtype=np.int16), (nw, nk, k + 1)).copy()
    out = np.zeros((nw, nk, L + 1), np.int16)
    out[:, :, 0] = k
    idx = np.arange(k + 1, dtype=np.int16)
    for j in range(L):
        neq = (pat[None, :, :] != txt[:, j, None, None]).astype(np.int16)  # (an N, 4, differs from every base)
        a = np.empty_like(col)
        a[:, :, 0] = 0
        a[:, :, 1:] = np.minimum(col[:, :, :-1] + neq, col[:, :, 1:] + 1)
        col = np.minimum.accumulate(a - idx, axis=2) + idx
        out[:, :, j + 1] = col[:, :, k]
    return out


def expected_positions(k, kmers, windows, E):
    """(hit, pos, counts): hit bool (E + 1, n_windows, n_kmers); pos int16 (n_windows, n_kmers), 1..L, -1
    where d > E; counts the M1(E) counts.  The DP's minimum is pinned to the oracle's distance here."""
    nk, nw = len(kmers), len(windows)
    if not (nk and nw):
        return np.zeros((E + 1, nw, nk), bool), np.zeros((nw, nk), np.int16), np.zeros(nk, np.uint64)
    e = last_rows(k, kmers, windows)
    d = e.min(axis=2)
    np.testing.assert_array_equal(np.minimum(d, E + 1), distances(k, kmers, windows, E + 1).T,
                                  err_msg="the Sellers DP's minimum is not the oracle's distance")
    hit = np.stack([d <= lv for lv in range(E + 1)])
    pos = np.where(d <= E, (e == d[:, :, None]).argmax(axis=2), -1).astype(np.int16)
    assert not ((pos == 0) & (d <= E)).any()
    return hit, pos, hit.sum(axis=(0, 1)).astype(np.uint64)


def pack_positions(pos):
    """int (n_windows, n_kmers), -1 = none -> the matrix layout, uint32 (8, n_windows, ceil(n_kmers / 32))."""
    pos = np.asarray(pos)
    v = np.where(pos > 0, pos - 1, 0)
    return pack_hits(np.stack([((v >> b) & 1).astype(bool) & (pos > 0) for b in range(8)]))


def profile_of(hit, pos, L):
    """uint32 (levels, n_kmers, L): the windows at distance exactly d whose best occurrence ends at p + 1."""
    lv, nw, nk = hit.shape
    prof = np.zeros((lv, nk, L), np.uint32)
    for d in range(lv):
        exact = hit[d] & ~(hit[d - 1] if d else np.zeros_like(hit[0]))
        ws, cs = np.nonzero(exact)
        np.add.at(prof[d], (cs, pos[ws, cs] - 1), 1)
    return prof


def _subst(rng, s, n):
    t = list(s)
    for p in sorted(rng.choice(np.arange(1, len(s) - 1), size=n, replace=False).tolist()):
        t[p] = "ACGT"[(CODE[t[p]] + 1 + int(rng.integers(3))) % 4]
    return "".join(t)


def _rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=max(n, 0)))


def positions_case(seed, k, n_kmers, n_windows, L, E, p_n=0.01):
    """budget_case with occurrences planted so that the position rule is exercised, each property asserted
    here on the CPU wherever the shape has room for it (returned in `did`):
      a  two occurrences at different distances, the worse one first (E >= 1, L >= 2 k + 3): overwritten
      b  two occurrences at the best distance (L >= 2 k + 3): the first wins
      c  a best occurrence ending at base L with the k-mer's last base missing there (E >= 1, L >= k - 1)
      d  a best occurrence ending at j with j % 4 != 0 and j > 4 (L // 4) (L % 4 != 0, L >= k)
      e  ends at 16, 17 and 32 (those with k <= j <= L)
      f  L > 128: ends at 128, 129 and L (plane 7)
      g  E = 3 (L >= k - 3): a pair at distance exactly 3
      h  at least a tenth of the pairs hit (8 < n_kmers <= 64, L >= 2 k, n_windows >= 24: the k-mers from 8
         on tile an adapter that every other window holds a stretch of, anchored at its start or end)
    Returns (kmers, windows, hit, pos, counts, did)."""
    km, w = budget_case(seed, k, n_kmers, n_windows, L, p_n=p_n)
    km, w = list(km), list(w)
    rng = np.random.default_rng(seed + 7)
    tiles = n_kmers - 8 if 8 < n_kmers <= 64 else 0
    if tiles:
        adapter = _rand(rng, k + tiles - 1)
        for i in range(tiles):
            km[8 + i] = cases.kmer_value(adapter[i:i + k])
        assert len(set(km)) == len(km)
    s = [cases.kmer_string(v, k) for v in km]
    plants = []  # (name, k-mer, text builder's result, expected pos, expected d)
    c0, c1 = 0, min(1, n_kmers - 1)
    if E >= 1 and L >= 2 * k + 3:
        worse = _subst(rng, s[c0], min(E, 2))
        plants.append(("a", c0, worse + _rand(rng, 3) + s[c0] + _rand(rng, L - 2 * k - 3), 2 * k + 3, 0))
    if L >= 2 * k + 3:
        plants.append(("b", c1, s[c1] + _rand(rng, 3) + s[c1] + _rand(rng, L - 2 * k - 3), k, 0))
    if E >= 1 and L >= k - 1:
        plants.append(("c", c1, _rand(rng, L - (k - 1)) + s[c1][:k - 1], L, 1))
    if L % 4 and L >= k:
        plants.append(("d", c0, _rand(rng, L - k) + s[c0], L, 0))
    for j in (16, 17, 32):
        if k <= j <= L:
            plants.append((f"e{j}", c0, _rand(rng, j - k) + s[c0] + _rand(rng, L - j), j, 0))
    if L > 128:
        for j in (128, 129, L):
            plants.append((f"f{j}", c1, _rand(rng, j - k) + s[c1] + _rand(rng, L - j), j, 0))
    free = list(range(1, max(n_windows - 1, 1)))  # (budget_case's own plants sit in the first and last window)
    placed = []
    for pl in plants:
        if free:
            wi = free.pop(0)
            assert len(pl[2]) == L, pl[0]
            w[wi] = pl[2]
            placed.append((wi,) + pl)
    if tiles and L >= 2 * k:
        for n, wi in enumerate(free[::2]):
            ln = min(L, len(adapter))
            a0 = int(rng.integers(0, len(adapter) - ln + 1))
            part = adapter[a0:a0 + ln]
            w[wi] = part + _rand(rng, L - ln) if n % 2 == 0 else _rand(rng, L - ln) + part
    hit, pos, counts = expected_positions(k, km, w, E)
    e = last_rows(k, km, w) if placed else None
    did = set()
    for wi, name, c, _, want_pos, want_d in placed:
        d = int(e[wi, c].min())
        assert (d, int(pos[wi, c])) == (want_d, want_pos), (name, d, int(pos[wi, c]), want_d, want_pos)
        if name == "a":  # some level was hit before the best one: the position is overwritten
            assert (e[wi, c, :want_pos] <= E).any() and (e[wi, c, :want_pos] > want_d).all()
        if name == "b":  # the best distance is reached again later
            assert (e[wi, c, want_pos + 1:] == want_d).any()
        if name == "d":
            assert want_pos % 4 and want_pos > 4 * (L // 4)
        did.add(name[0] if name[0] != "e" and name[0] != "f" else name)
    if E == 3 and L >= k - 3:
        assert (hit[3] & ~hit[2]).any(), "no window at distance exactly 3"
        did.add("g")
    if tiles and L >= 2 * k and n_windows >= 24:
        assert hit[E].mean() >= 0.1, hit[E].mean()
        did.add("h")
    return km, w, hit, pos, counts, did


__all__ = ["FILL", "GUARD", "last_rows", "expected_positions", "pack_positions", "pack_hits", "profile_of",
           "positions_case"]
