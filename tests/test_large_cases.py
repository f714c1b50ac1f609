"""CPU companion of tests/test_gpu_large_image.py: on a scaled-down image built by the same functions
(tests/large_cases.py, numpy path) every case has the property its GPU test relies on -- the bincount formula
gives the oracle's counts, every boundary window holds a marker text whose loss changes the sums, the expanded
per-text rows are the references' matrices, the per-text flank and edit profiles summed through bincount(idx) are
the references' profiles and change under an index fault, the sparse windows sit where the docstrings say -- and the window
index arithmetic names the code bytes it claims to."""
import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from tests import large_cases as lc
from tests.hits_cases import pack_hits
from tests.positions_cases import expected_positions, pack_positions, profile_of
from tests.span_cases import pack_starts, starts_of

OLD_TOP = (1 << 34) - 32  # the largest image the ABI accepted before the bound was lowered
SMALL_WINDOWS = 300


def small_shape(L):
    """A dense image of SMALL_WINDOWS windows and three slots more, with scaled-down boundaries (the last one
    the image's size) and sentinel."""
    S = lc.slot(L)
    n_bases = (SMALL_WINDOWS + 3) * S
    return S, n_bases, (64 * S, 128 * S + 32, n_bases), 200 * S // 4


def test_bound_is_the_header_s():
    assert lc.header_bound() == lc.MAX_IMAGE_BASES == (1 << 34) - 4096
    assert lc.TOP_BASES % 32 == 0 and lc.TOP_BASES < lc.MAX_IMAGE_BASES <= lc.TOP_BASES + 32
    assert lc.BOUNDARIES == (1 << 32, 1 << 33, lc.TOP_BASES)
    # every accepted image's code bytes, and so every slot, end below the kernel's no-window offset
    assert lc.MAX_IMAGE_BASES // 4 <= lc.SENTINEL_BYTE


@pytest.mark.parametrize("L", [20, 33, 100, 200, 256])
def test_window_index_arithmetic(L):
    S = lc.slot(L)
    for top in (OLD_TOP, lc.TOP_BASES):
        nw = lc.windows_in(top, L)
        assert nw * S <= top < (nw + 1) * S + S
        ws = lc.boundary_windows(nw, S, (1 << 32, 1 << 33, top))
        assert ws == sorted(set(ws)) and ws[0] == 0 and ws[-1] == nw - 1
        for b, byte in ((1 << 32, 1 << 30), (1 << 33, 1 << 31)):
            w = b // S
            assert {w - 1, w, w + 1} <= set(ws)
            # window w holds base b: it starts at the boundary where the slot divides it, else it straddles it
            assert lc.code_byte(w, S) == w * S // 4 <= byte < lc.code_byte(w + 1, S) and w * S <= b < (w + 1) * S
            assert (lc.code_byte(w, S) == byte) == (b % S == 0) and (b % S == 0) == (S in (32, 64, 128, 256))
        assert lc.code_byte(nw - 1, S) + S // 4 <= top // 4 < 1 << 32
    # the window at the kernel's no-window offset: real under the old bound, in no accepted image
    at = lc.SENTINEL_BYTE * 4 // S
    assert lc.code_byte(at, S) <= lc.SENTINEL_BYTE < lc.code_byte(at + 1, S)
    # (slots of 8, 16, 32 and 64 bytes start exactly there; so do those of 56 bytes, L = 193..224)
    assert (lc.code_byte(at, S) == lc.SENTINEL_BYTE) == (S in (32, 64, 128, 224, 256))
    old = lc.boundary_windows(lc.windows_in(OLD_TOP, L), S, (1 << 32, 1 << 33, OLD_TOP))
    assert at < lc.windows_in(OLD_TOP, L) and {at - 1, at, at + 1} <= set(old)
    assert at >= lc.windows_in(lc.TOP_BASES, L)
    assert lc.code_byte(lc.windows_in(lc.TOP_BASES, L), S) <= lc.SENTINEL_BYTE
    if L == 100:
        assert (at, lc.windows_in(OLD_TOP, L)) == (134217720, 134217727)


def test_top_sizes_named_in_the_gpu_tests():
    assert lc.windows_in(lc.TOP_BASES, 100) == (1 << 27) - 33
    assert lc.windows_in(lc.TOP_BASES, 200) == lc.TOP_BASES // 224 == 76695826  # slots of 56 bytes
    assert lc.windows_in(lc.TOP_BASES, 256) == (1 << 26) - 17                     # slots of 64 bytes
    words = 8 * lc.windows_in(lc.TOP_BASES, 100) * 2  # the position matrix of 64 candidates
    assert 1 << 32 < 4 * words < 1 << 33  # 8.59 GB: its byte offsets pass 2^32
    assert words < 1 << 31 < words + 1024  # ... its word offsets end 528 short of 2^31 (they passed it in no image)


def small_dense(k, n_kmers, L):
    km, texts, per, markers = lc.dense_dictionary(k, n_kmers, L)
    S, n_bases, bounds, sentinel = small_shape(L)
    marks = lc.boundary_windows(SMALL_WINDOWS, S, bounds, sentinel)
    idx, held = lc.dense_index(SMALL_WINDOWS, len(texts), 11, marks, markers)
    return km, texts, per, markers, S, n_bases, marks, idx, held


@pytest.mark.parametrize("k,n_kmers,L", sorted(lc.DENSE_SEEDS))
def test_small_dense_image_gives_the_oracle_s_counts(k, n_kmers, L):
    km, texts, per, markers, S, n_bases, marks, idx, held = small_dense(k, n_kmers, L)
    # the boundary windows: both sides of each boundary, the ends, the sentinel's three -- each a marker text
    assert len(marks) >= 11 and {0, SMALL_WINDOWS - 1, 63, 64, 65, 127, 128, 129, 199, 200, 201} <= set(marks)
    assert len(markers) >= 3 and set(held) == set(marks)
    for w in marks:
        t = int(idx[w])
        assert t == held[w] and t in markers
        assert per[t].any() and sum((per == per[t]).all(axis=1)) == 1
    assert all(idx[a] != idx[b] for a, b in zip(marks, marks[1:]) if b == a + 1)  # neighbours differ
    # the image is the packed sample, zeros after the last slot
    codes, nmask = lc.dense_image(*lc.text_tables(texts), idx, n_bases)
    img = ac.pack_windows(texts[idx])
    assert img.equal_window_len() == L and img.n_bases == SMALL_WINDOWS * S
    assert np.array_equal(codes[:img.codes.size].view(np.uint32), img.codes) and not codes[img.codes.size:].any()
    assert np.array_equal(nmask[:img.nmask.size].view(np.uint32), img.nmask) and not nmask[img.nmask.size:].any()
    assert codes.size == n_bases // 16 and nmask.size == n_bases // 32
    # the bincount formula is the oracle on every window
    want = lc.expected_counts(idx, per)
    assert want.dtype == np.uint64 and np.array_equal(want, oracle.count_myers(k, km, texts[idx]))
    # losing any one boundary window, or counting its neighbour in its place, changes the counts
    for w in marks:
        assert not np.array_equal(lc.expected_counts(np.delete(idx, w), per), want), w
        other = idx.copy()
        other[w] = idx[w - 1] if w else idx[w + 1]
        assert not np.array_equal(lc.expected_counts(other, per), want), w


@pytest.mark.parametrize("E", [2, 3])
def test_expanded_rows_are_the_references_matrices(E):
    k, n_kmers, L = 16, 64, 100
    km, texts, per, markers, S, n_bases, marks, idx, held = small_dense(k, n_kmers, L)
    rows = lc.text_rows(k, n_kmers, L, E)
    win = texts[idx]
    hit, pos, counts = expected_positions(k, km, win, E)
    start, _ = starts_of(k, km, win, hit, pos)
    u32 = lambda a: a.view(np.uint32)  # noqa: E731
    for e in range(E + 1):
        assert np.array_equal(u32(rows["hits"][e][idx]), pack_hits(hit)[e])
        assert lc.first_mismatch(pack_hits(hit)[e].view(np.int32), rows["hits"][e], idx, S) is None
    for b in range(8):
        assert np.array_equal(u32(rows["pos"][b][idx]), pack_positions(pos)[b])
        assert np.array_equal(u32(rows["start"][b][idx]), pack_starts(start, hit[E])[b])
    n = lc.text_counts(idx, len(texts))
    assert np.array_equal(np.einsum("t,etc->ec", n, rows["hit"].astype(np.uint64)), hit.sum(axis=1))
    assert np.array_equal(rows["hit"].sum(axis=2)[:, idx], hit.sum(axis=2))
    assert np.array_equal(np.einsum("t,tecp->ecp", n, rows["prof"]), profile_of(hit, pos, L))
    if E == 2:  # the levels sum to the counts of the bincount formula
        assert np.array_equal(counts, lc.expected_counts(idx, per))
    # every boundary window's hit row is nonzero at the top level: a row left unwritten, or zero, shows
    for w in marks:
        assert rows["hits"][E][int(idx[w])].any(), w
    # a mismatch is reported with its window and code byte
    broken = rows["hits"][E][idx].copy()
    broken[200, 1] ^= 4
    msg = lc.first_mismatch(broken, rows["hits"][E], idx, S)
    assert msg.startswith(f"window 200 (code byte {200 * S // 4:#x}, text {int(idx[200])})"), msg


def test_dictionary_profiles_are_not_trivial():
    """What tests/test_gpu_large_image.py's flank and edit tests rely on in the (16, 64, 100) dictionary at E = 2,
    so that a change of dictionary cannot empty them."""
    k, n_kmers, L, E = 16, 64, 100, 2
    km, texts, per, markers = lc.dense_dictionary(k, n_kmers, L)
    p = lc.text_profiles(k, n_kmers, L, E)
    hit, pos, start = p["hit"], p["pos"], p["start"]
    top = hit[E]
    dist = (E + 1 - hit.sum(axis=0))
    assert len(texts) == 61 and int(top.any(axis=1).sum()) == 48
    assert [int(((dist == d) & top).any(axis=1).sum()) for d in range(E + 1)] == [12, 18, 18]
    assert len(markers) == 36
    for name, a in (("flank, D = 8", p["flank"][8, E, True]), ("flank, D = 32", p["flank"][32, E, True]), ("edit", p["edit"][E])):
        a = a.reshape(len(texts), -1)
        for t in markers:  # a nonzero profile that no other text has
            assert a[t].any() and int((a == a[t]).all(axis=1).sum()) == 1, (name, t)
    assert p["edit"][E].sum(axis=(0, 1, 2)).tolist() == [727, 5, 8, 3, 6, 10, 9, 1, 4, 3, 3, 2]
    assert p["counted"][top].all() and not p["counted"][~top].any()  # no pair fails the edit pass's conditions
    assert int((pos[top].astype(int) + 8 > L).sum()) == 18 and int((start[top] < 8).sum()) == 18  # cut at D = 8
    # the other forms the GPU tests run: plane 0 holds fewer pairs, and without starts only the left half goes
    assert 0 < p["edit"][0].sum() < p["edit"][E].sum() and 0 < p["flank"][8, 0, True].sum() < p["flank"][8, E, True].sum()
    for D in lc.PROFILE_DEPTHS:
        with_s, without = p["flank"][D, E, True], p["flank"][D, E, False]
        assert np.array_equal(with_s[:, 0], without[:, 0]) and with_s[:, 1].any() and not without[:, 1].any()
        assert with_s.shape == (61, 2, n_kmers, D, 5)
    assert p["flank"][32, E, True][:, :, :, 8:].any()  # (columns only the deeper profile has)
    # operations 0..6 of a base sum to the pairs counted for its k-mer
    assert np.array_equal(p["edit"][E][..., :7].sum(axis=3), np.repeat(top[:, :, None], k, axis=2))


def test_small_dense_image_profiles():
    """The einsum over bincount(idx) is the references' profile of the expanded windows; and an index fault shows:
    any one boundary window reading a neighbour's text, or every window reading the text of the window a
    (scaled-down) 2^32 bases below it, changes the expected flank sum and the expected edit sum."""
    from tests.edit_cases import edit_profile_of
    from tests.flank_cases import flank_profile_of

    k, n_kmers, L, E = 16, 64, 100, 2
    km, texts, per, markers, S, n_bases, marks, idx, held = small_dense(k, n_kmers, L)
    p = lc.text_profiles(k, n_kmers, L, E)
    n = lc.text_counts(idx, len(texts))
    win = texts[idx]
    hit, pos, _ = expected_positions(k, km, win, E)
    start, _ = starts_of(k, km, win, hit, pos)
    for plane in (0, E):
        want = lc.image_profile(n, p["edit"][plane])
        assert want.dtype == np.uint64 and np.array_equal(want, edit_profile_of(k, km, win, hit[plane], pos, start))
        for D in lc.PROFILE_DEPTHS:
            for with_start in (True, False):
                want = lc.image_profile(n, p["flank"][D, plane, with_start])
                assert np.array_equal(want, flank_profile_of(win, hit[plane], pos, start if with_start else None, D))
    sums = lambda i: [lc.image_profile(lc.text_counts(i, len(texts)), a)  # noqa: E731
                      for a in (p["flank"][8, E, True], p["flank"][32, E, True], p["flank"][8, 0, True], p["edit"][E])]
    want = sums(idx)
    for w in marks:
        other = idx.copy()
        other[w] = idx[w - 1] if w else idx[w + 1]
        got = sums(other)  # (plane 0 aside: a marker text's pair may lie at distance 1 or 2)
        assert not any(np.array_equal(a, b) for a, b in zip(got[:2] + got[3:], want[:2] + want[3:])), w
    below = 64  # windows in the first scaled-down boundary, 64 S bases: what 2^32 / S is to the large image
    shifted = idx.copy()
    shifted[below:] = idx[:-below]
    assert not any(np.array_equal(a, b) for a, b in zip(sums(shifted), want))
    # a difference is reported with its cell
    broken = want[0].copy()
    broken[1, 5, 3, 2] += 1
    msg = lc.first_cell(broken, want[0], ("side", "k-mer", "column", "symbol"))
    assert msg.startswith("1 cells differ, first at {'side': 1, 'k-mer': 5, 'column': 3, 'symbol': 2}"), msg
    assert lc.first_cell(want[0], want[0], ("side", "k-mer", "column", "symbol")) is None


def decode(codes, nmask, start, length):
    b = np.arange(start, start + length)
    c = (codes.view(np.uint32)[b // 16] >> (2 * (b % 16)).astype(np.uint32)) & 3
    n = (nmask.view(np.uint32)[b // 32] >> (b % 32).astype(np.uint32)) & 1
    return "".join("N" if x else "ACGT"[int(y)] for x, y in zip(n, c))


def check_sparse_layout(windows, regions, n_bases, boundaries):
    assert 30 <= len(windows) <= 60 and all(s % 32 == 0 and n >= 1 and s + n <= n_bases for s, n in windows)
    for b in boundaries:
        assert any(s + n == b for s, n in windows)                      # ends exactly at the boundary
        assert any(s == b for s, n in windows)                          # starts exactly at it
        assert any(s < b < s + n and n <= 300 for s, n in windows)      # straddles it
        assert any(s < b < s + n and n >= 600 and (b - s) % 256 == 0 for s, n in windows)  # ... a fetch seam on it
    assert any(s == 0 for s, n in windows) and any(s + n == n_bases for s, n in windows)
    lens = sorted(n for _, n in windows)
    assert lens[0] <= 33 and sum(600 <= n <= 1500 for n in lens) >= 4 and sum(20 <= n <= 300 for n in lens) >= 20
    texts = lc.sparse_windows(regions, windows)
    assert any("N" in t for t in texts) and any("N" not in t for t in texts)
    return texts


@pytest.mark.parametrize("k", [10, 16, 22, 32])
def test_sparse_case(k):
    # the layout the GPU test uses: arithmetic only
    km, regions, windows = lc.sparse_case(k)
    check_sparse_layout(windows, regions, lc.TOP_BASES, lc.BOUNDARIES[:2])
    assert len(km) == lc.SPARSE_KMERS == 64
    want = lc.sparse_expected(k)
    assert (want > 0).sum() >= len(km) // 2 and all(want[b:b + 32].any() for b in (0, 32))
    # a scaled-down one through the same functions: the image holds the windows' texts where they are said to be
    n_bases, bounds = (1 << 17) - 4128, (1 << 15, 1 << 16)
    km, regions, windows = lc.sparse_case(k, n_bases, bounds)
    texts = check_sparse_layout(windows, regions, n_bases, bounds)
    codes, nmask = lc.sparse_image(regions, n_bases)
    assert codes.size == n_bases // 16 and nmask.size == n_bases // 32
    for (s, n), t in zip(windows, texts):
        assert decode(codes, nmask, s, n) == t
    covered = np.zeros(n_bases, bool)
    for s, t in regions:
        covered[s:s + (len(t) + 31) // 32 * 32] = True
    assert not codes[~covered[::16]].any() and not nmask[~covered[::32]].any()
    # the image as ac_windows gives the oracle's counts through the host entry point's own reference
    start = np.array([s for s, _ in windows], np.uint64)
    length = np.array([n for _, n in windows], np.uint32)
    smp = ac.PackedSample(codes.view(np.uint32), nmask.view(np.uint32), start, length, n_bases)
    assert smp.n_windows == len(windows)
    assert np.array_equal(lc.sparse_expected(k, n_bases, bounds), oracle.count_myers(k, km, texts))
