"""Case builders and expected values of the match-span tests (ac_hit_start_positions_device,
ac_window_spans_samples; DESIGN.md §4e "Match spans"), shared by tests/test_spans_cpu.py and
tests/test_gpu_spans.py.

Expected values: from tests.positions_cases.expected_positions -- whose minimum is pinned to the oracle's
distance -- every hit pair (d <= E, pos) gets the plain global DP of the reversed k-mer against the reversed
text before pos, column by column; the least column j whose bottom cell is d is the occurrence's length and
start = pos - j.  A qualifying j is asserted to exist and to lie in k - d .. k + d."""
import numpy as np

from tests import cases
from tests.hits_cases import pack_hits
from tests.positions_cases import CODE, _rand, expected_positions, last_rows, pack_positions, positions_case
from tests.test_gpu_bitslice import equal_case


def _codes(windows):
    nw = len(windows)
    L = len(windows[0]) if nw else 0
    return np.array([[CODE.get(c, 4) for c in w] if isinstance(w, str) else np.asarray(w) for w in windows],
                    np.int16).reshape(nw, L)


def starts_of(k, kmers, windows, hit, pos):
    """(start, nqual) from the windows and the expected hit levels / end positions: start int16
    (n_windows, n_kmers), 0-based inclusive, -1 where d > E; nqual the number of starts that qualify
    (ed(c, w[s, pos)) = d), 0 where there is no hit."""
    lv, nw, nk = hit.shape
    E = lv - 1
    start = np.full((nw, nk), -1, np.int16)
    nqual = np.zeros((nw, nk), np.int16)
    ws, cs = np.nonzero(hit[E])
    if not ws.size:
        return start, nqual
    d = (lv - hit.sum(axis=0))[ws, cs].astype(np.int16)
    p = pos[ws, cs].astype(np.int64)
    pat = np.array([[(int(v) >> (2 * (k - 1 - i))) & 3 for i in range(k)] for v in kmers], np.int16).reshape(nk, k)
    rp = pat[cs][:, ::-1]                                    # the reversed k-mers, one row per pair
    txt = _codes(windows)
    J = k + E
    idx = p[:, None] - 1 - np.arange(J)[None, :]            # the reversed text's bases, -1.. : before the window
    rt = np.where(idx >= 0, txt[ws[:, None], np.maximum(idx, 0)], 9)
    ar = np.arange(k + 1, dtype=np.int16)
    col = np.broadcast_to(ar, (ws.size, k + 1)).copy()       # column 0 of a global alignment: 0, 1, .., k
    length = np.zeros(ws.size, np.int16)
    n = np.zeros(ws.size, np.int16)
    for j in range(J):
        neq = (rp != rt[:, j, None]).astype(np.int16)        # (an N, 4, and the 9 past the edge match nothing)
        a = np.empty_like(col)
        a[:, 0] = j + 1                                      # its top row: 0, 1, 2, ..
        a[:, 1:] = np.minimum(col[:, :-1] + neq, col[:, 1:] + 1)
        col = np.minimum.accumulate(a - ar, axis=1) + ar
        ok = (col[:, k] == d) & (idx[:, j] >= 0)
        length = np.where(ok & (length == 0), j + 1, length)
        n += ok
    assert (length > 0).all(), "a hit pair without a qualifying start"
    assert ((length >= k - d) & (length <= k + d)).all()
    start[ws, cs] = p - length
    nqual[ws, cs] = n
    assert (start[ws, cs] >= 0).all()
    return start, nqual


def expected_spans(k, kmers, windows, E):
    """(hit, pos, start, counts, nqual): expected_positions plus starts_of."""
    hit, pos, counts = expected_positions(k, kmers, windows, E)
    if not (len(kmers) and len(windows)):
        return hit, pos, np.zeros(pos.shape, np.int16), counts, np.zeros(pos.shape, np.int16)
    start, nqual = starts_of(k, kmers, windows, hit, pos)
    return hit, pos, start, counts, nqual


def pack_starts(start, hit_E):
    """int (n_windows, n_kmers), -1 = none -> the matrix layout, uint32 (8, n_windows, ceil(n_kmers / 32)):
    the value as it is (pack_positions stores p - 1)."""
    start = np.asarray(start)
    return pack_positions(np.where(hit_E, start + 1, -1))


def length_profile_of(hit, pos, start, k):
    """uint32 (levels, n_kmers, 2 E + 1): the windows at distance exactly d with len = k - E .. k + E."""
    lv, nw, nk = hit.shape
    E = lv - 1
    prof = np.zeros((lv, nk, 2 * E + 1), np.uint32)
    for d in range(lv):
        exact = hit[d] & ~(hit[d - 1] if d else np.zeros_like(hit[0]))
        ws, cs = np.nonzero(exact)
        np.add.at(prof[d], (cs, (pos[ws, cs] - start[ws, cs]) - (k - E)), 1)
    return prof


def plain_case(seed, k, n_kmers, n_windows, L, E, p_n=0.01):
    """Equal windows with planted occurrences and, in every window, up to four more candidates mutated by up
    to E random edits each, side by side: nothing asserted, any k (the k outside the listed ones)."""
    km, w = equal_case(seed, n_kmers, n_windows, L, p_n=p_n, k=k)
    km, w = list(km), list(w)
    rng = np.random.default_rng(seed + 11)
    slot = k + E + 2
    for wi in range(n_windows):
        for r in range(min(max(L // slot, 1), 4)):
            t = list(cases.kmer_string(km[int(rng.integers(n_kmers))], k))
            for _ in range(int(rng.integers(0, E + 1))):
                kind, at = int(rng.integers(3)), int(rng.integers(len(t)))
                if kind == 0:
                    t[at] = "ACGT"[int(rng.integers(4))]
                elif kind == 1:
                    t.insert(at, "ACGT"[int(rng.integers(4))])
                elif len(t) > 1:
                    del t[at]
            t = "".join(t)[:L]
            at = min(r * slot + int(rng.integers(0, 3)), L - len(t))
            w[wi] = w[wi][:at] + t + w[wi][at + len(t):]
    return km, w


def spans_case(seed, k, n_kmers, n_windows, L, E, p_n=0.01):
    """positions_case with windows APPENDED (the windows that give its property h their density stay) that
    plant what the span rule has to get right; every property is asserted here on the CPU wherever the shape
    has room for it and returned in `did`:
      ins1..insE   e bases inserted inside the occurrence: len = k + e
      del1..delE   e of the k-mer's bases missing: len = k - e
      lead         the first base substituted: two starts qualify, the shorter wins, len = k - 1   (E >= 1)
      leadN        the same with an N
      clip         the k-mer's first base missing at the window's first base: start 0, pos k - 1   (E >= 1)
      s0 s15 s16 s17 s31 s32 s33 sEnd   exact occurrences starting at the code-word and bitmap-word seams and
                   at L - k;  for L > 128 also s127 s128 s129 (plane 7)
      len          a pair at every length k - E .. k + E
      multi        at least two pairs where more than one start qualifies (E >= 1)
    and positions_case's own (h: at least a tenth of all pairs hit, over the appended windows too).
    Returns (kmers, windows, hit, pos, start, counts, did); len(windows) >= n_windows."""
    km, w, _, _, _, did = positions_case(seed, k, n_kmers, n_windows, L, E, p_n=p_n)
    km, w = list(km), list(w)
    rng = np.random.default_rng(seed + 13)
    s = [cases.kmer_string(v, k) for v in km]
    other = lambda c: "ACGT"[(CODE[c] + 1 + int(rng.integers(3))) % 4]  # noqa: E731

    def around(text, at):
        """`text` at base `at` of a window of random bases; the base before it is not text's first one."""
        left = _rand(rng, at)
        if left and left[-1] == text[0]:
            left = left[:-1] + other(text[0])
        return (left + text + _rand(rng, L - at - len(text)))[:L]

    plants = []  # (name, k-mer, window, want start, want pos, want d)

    def plant(name, c, make, want_start, want_pos, want_d):
        """Draws the window until this pair alone has the span stated (a k-mer with a repeat near an edit can
        explain it another way); the whole case asserts it again below."""
        for _ in range(32):
            text = make()
            e = last_rows(k, [km[c]], [text])
            d = int(e.min())
            if d > E:
                continue
            h1 = np.array([[[d <= lv]] for lv in range(E + 1)])
            p1 = np.array([[int((e[0, 0] == d).argmax())]], np.int16)
            s1, _ = starts_of(k, [km[c]], [text], h1, p1)
            if (int(s1[0, 0]), int(p1[0, 0]), d) == (want_start, want_pos, want_d):
                plants.append((name, c, text, want_start, want_pos, want_d))
                return
        raise AssertionError(f"{name}: no window with the stated span for k-mer {s[c]}")

    def inserted(c, e):
        t = s[c]
        for i, at in enumerate(sorted(rng.choice(np.arange(5, k - 4, 3), size=e, replace=False).tolist())):
            x = next(b for b in "ACGT" if b != t[at + i - 1] and b != t[at + i])
            t = t[:at + i] + x + t[at + i:]
        return t

    def missing(c, e):
        cut = sorted(rng.choice(np.arange(5, k - 4, 3), size=e, replace=False).tolist())
        return "".join(b for i, b in enumerate(s[c]) if i not in cut)

    nk = n_kmers
    for e in range(1, E + 1):
        if L >= k + e + 2:
            plant(f"ins{e}", (2 * e) % nk, lambda: around(inserted((2 * e) % nk, e), 1), 1, 1 + k + e, e)
        if L >= k + 2:
            plant(f"del{e}", (2 * e + 1) % nk, lambda: around(missing((2 * e + 1) % nk, e), 2), 2, 2 + k - e, e)
    if E >= 1 and L >= k + 4:
        c = 1 % nk
        plant("lead", c, lambda: around(other(s[c][0]) + s[c][1:], 3), 4, 3 + k, 1)
        plant("leadN", c, lambda: around("N" + s[c][1:], 3), 4, 3 + k, 1)
    if E >= 1 and L >= k - 1:
        plant("clip", 0, lambda: (s[0][1:] + _rand(rng, L))[:L], 0, k - 1, 1)
    seams = [("s0", 0), ("s15", 15), ("s16", 16), ("s17", 17), ("s31", 31), ("s32", 32), ("s33", 33), ("sEnd", L - k)]
    if L > 128:
        seams += [("s127", 127), ("s128", 128), ("s129", 129)]
    for name, at in seams:
        if 0 <= at <= L - k:
            plant(name, 1 % nk, lambda: around(s[1 % nk], at), at, at + k, 0)
    first = len(w)
    w += [pl[2] for pl in plants]
    assert all(len(x) == L for x in w)
    hit, pos, start, counts, nqual = expected_spans(k, km, w, E)
    dist = hit.shape[0] - hit.sum(axis=0)
    for i, (name, c, _, want_start, want_pos, want_d) in enumerate(plants):
        got = (int(start[first + i, c]), int(pos[first + i, c]), int(dist[first + i, c]))
        assert got == (want_start, want_pos, want_d), (name, got, (want_start, want_pos, want_d))
        if name in ("lead", "leadN"):
            assert nqual[first + i, c] >= 2, name
        did.add(name)
    lens = (pos - start)[hit[E]]
    if "s0" in did and all(f"{n}{e}" in did for n in ("ins", "del") for e in range(1, E + 1)):
        assert set(range(k - E, k + E + 1)) <= set(lens.tolist()), sorted(set(lens.tolist()))
        did.add("len")
    if E >= 1 and "lead" in did:
        assert (nqual > 1).sum() >= 2
        did.add("multi")
    if "h" in did:
        assert hit[E].mean() >= 0.1, hit[E].mean()
    return km, w, hit, pos, start, counts, did


__all__ = ["starts_of", "expected_spans", "pack_starts", "pack_hits", "pack_positions", "length_profile_of", "plain_case",
           "spans_case"]
