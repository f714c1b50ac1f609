"""Case builders of the large-image tests (tests/test_gpu_large_image.py: window images up to the size bound
the ABI accepts), shared with their CPU companion (tests/test_large_cases.py), which shows on a scaled-down
image that every case has the property its GPU test relies on.

The edge these cases reach is an address, not a length: base indices past 2^32, code-byte offsets past 2^31
(the sign bit of the 32-bit size every buffer descriptor is made with) and the top of the accepted range.
So the images are built on the device -- `device` below is a torch device, or None for the numpy path the
CPU test takes through the same functions -- and no host array is sized by the window count.

Dense image: equal windows drawn from a dictionary (tests/cases.py dictionary_case: 61 texts of exactly L
bases, each with the oracle's count vector).  The texts are packed once into a (61, S / 16) code table and
a (61, S / 32) N table (S = the slot, L rounded up to 32 bases); an index tensor `idx` says which text
every window holds and image = table[idx].  Expected counts are bincount(idx) @ per_text; expected hit,
position and start matrices are the per-text rows expanded by the same idx; expected flank and edit profiles are the
per-text profiles summed through bincount(idx).  The windows at every boundary
hold MARKER texts -- a nonzero count vector that no other text has -- so a boundary window that is skipped,
or counted in a neighbour's place, changes the sums.

Sparse image: zeros, with a few dozen ragged windows at chosen places; expected counts are the oracle's on
those windows."""
import functools
import os
import random
import re

import numpy as np

import approx_counter_amd as ac
import oracle
from tests import cases
from tests.hits_cases import pack_hits
from tests.positions_cases import expected_positions, pack_positions, profile_of
from tests.span_cases import pack_starts, starts_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The bound on an image's bases (exclusive; wm_count.h AC_MAX_IMAGE_BASES, pinned by test_large_cases.py)
# and the largest image under it: n_bases is a multiple of 32.
MAX_IMAGE_BASES = (1 << 34) - 4096
TOP_BASES = MAX_IMAGE_BASES - 32
BOUNDARIES = (1 << 32, 1 << 33, TOP_BASES)
# The slot offset the bit-sliced kernel gives a lane without a window (bs_count.inc NO_WINDOW): a window
# whose slot starts at this code byte would be taken for none, so no accepted image reaches it.
SENTINEL_BYTE = 0xFFFFFF00
CHUNK = 1 << 24  # windows expanded at a time (a (CHUNK, 8) int32 temporary is 512 MiB)


def header_bound():
    """AC_MAX_IMAGE_BASES as wm_count.h defines it."""
    text = open(os.path.join(ROOT, "approx_counter_amd", "csrc", "wm_count.h")).read()
    m = re.search(r"#define AC_MAX_IMAGE_BASES \(\(1ull << (\d+)\) - (\d+)ull\)", text)
    assert m, "AC_MAX_IMAGE_BASES is not ((1ull << a) - b ull)"
    return (1 << int(m.group(1))) - int(m.group(2))


# ---- window index arithmetic ----

def slot(L):
    """Bases of an equal window's slot: L rounded up to 32."""
    return (L + 31) // 32 * 32


def windows_in(n_bases, L):
    return n_bases // slot(L)


def code_byte(w, S):
    """Byte offset of window w's slot of S bases in the code words (2 bits per base)."""
    return w * S // 4


def boundary_windows(n_windows, S, boundaries=BOUNDARIES, sentinel_byte=SENTINEL_BYTE):
    """The windows of a dense image of slots of S bases that an index fault would lose or misplace: the
    first and the last, those on each side of every boundary (in bases), and the one at code byte
    `sentinel_byte` with its neighbours -- those of them the image holds, ascending."""
    ws = {0, n_windows - 1}
    for b in boundaries:
        ws |= {b // S - 1, b // S, b // S + 1}
    at = sentinel_byte * 4 // S
    ws |= {at - 1, at, at + 1}
    return sorted(w for w in ws if 0 <= w < n_windows)


# ---- the dense image ----

# (k, candidates, L): the seed at which dictionary_case's own assertions hold
DENSE_SEEDS = {(16, 32, 100): 8, (22, 32, 100): 5, (16, 32, 200): 1, (22, 32, 200): 7, (16, 32, 256): 4, (16, 64, 100): 2,
               (10, 32, 100): 1, (16, 32, 300): 3}


@functools.lru_cache(maxsize=None)
def dense_dictionary(k, n_kmers, L):
    """(kmers, texts, per_text, markers): a dictionary_case and the indices of its marker texts."""
    km, texts, per = cases.dictionary_case(DENSE_SEEDS[(k, n_kmers, L)], n_kmers, L, k=k)
    return km, texts, per, marker_texts(per)


def marker_texts(per_text):
    """The texts whose count vector is nonzero and no other text's."""
    _, inverse, times = np.unique(per_text, axis=0, return_inverse=True, return_counts=True)
    own = times[inverse.reshape(-1)] == 1
    return [int(t) for t in np.flatnonzero(own & (per_text.sum(axis=1) > 0))]


def text_tables(texts):
    """The texts packed once (ac_pack_windows): int32 views (n_texts, S / 16) of their code words and
    (n_texts, S / 32) of their N bitmap words."""
    n, L = texts.shape
    img = ac.pack_windows(texts)
    S = slot(L)
    assert img.n_bases == n * S
    return img.codes.view(np.int32).reshape(n, S // 16).copy(), img.nmask.view(np.int32).reshape(n, S // 32).copy()


def _torch_dtype(dt):
    import torch

    return {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[np.dtype(dt)]


def zeros(n, dtype, device):
    if device is None:
        return np.zeros(n, dtype)
    import torch

    return torch.zeros(n, dtype=_torch_dtype(dtype), device=device)


def on(a, device):
    """A host array on `device` (itself on the numpy path)."""
    if device is None:
        return np.ascontiguousarray(a)
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def dense_index(n_windows, n_texts, seed, marks, markers, device=None):
    """int64 idx (n_windows): a seeded uniform draw of texts, then the windows `marks` overwritten with the
    `markers` texts in turn (neighbours hold different markers).  Returns (idx, {window: text})."""
    if device is None:
        idx = np.random.default_rng(seed).integers(0, n_texts, size=n_windows, dtype=np.int64)
    else:
        import torch

        g = torch.Generator(device=device)
        g.manual_seed(seed)
        idx = torch.randint(0, n_texts, (n_windows,), generator=g, device=device, dtype=torch.int64)
    held = {w: markers[i % len(markers)] for i, w in enumerate(marks)}
    for w, t in held.items():
        idx[w] = t
    return idx, held


def dense_image(tcodes, tnmask, idx, n_bases, device=None):
    """(codes, nmask) of n_bases: window w's slot holds text idx[w]; what lies past the last slot is zero."""
    nw = len(idx)
    cw, nm = tcodes.shape[1], tnmask.shape[1]
    assert nw * cw <= n_bases // 16 and n_bases % 32 == 0
    codes, nmask = zeros(n_bases // 16, np.int32, device), zeros(n_bases // 32, np.int32, device)
    tc, tn = on(tcodes, device), on(tnmask, device)
    cv, nv = codes[:nw * cw].reshape(nw, cw), nmask[:nw * nm].reshape(nw, nm)
    for c0 in range(0, nw, CHUNK):
        part = idx[c0:c0 + CHUNK]
        cv[c0:c0 + CHUNK] = tc[part]
        nv[c0:c0 + CHUNK] = tn[part]
    return codes, nmask


def text_counts(idx, n_texts):
    """bincount(idx) where idx lives, as uint64 on the host."""
    if isinstance(idx, np.ndarray):
        return np.bincount(idx, minlength=n_texts).astype(np.uint64)
    import torch

    return torch.bincount(idx, minlength=n_texts).cpu().numpy().astype(np.uint64)


def expected_counts(idx, per_text):
    return text_counts(idx, len(per_text)) @ per_text.astype(np.uint64)


def first_mismatch(got, rows, idx, S):
    """None if got (n_windows, words) == rows[idx], else a message naming the first differing window, its
    code byte offset, what it holds and what it should."""
    for c0 in range(0, len(idx), CHUNK):
        want = rows[idx[c0:c0 + CHUNK]]
        have = got[c0:c0 + CHUNK]
        if isinstance(have, np.ndarray):
            if np.array_equal(have, want):
                continue
            bad = np.flatnonzero((have != want).reshape(len(want), -1).any(axis=1))
        else:
            import torch

            if torch.equal(have, want):
                continue
            bad = torch.nonzero((have != want).reshape(len(want), -1).any(dim=1)).reshape(-1)
        w = c0 + int(bad[0])
        return (f"window {w} (code byte {code_byte(w, S):#x}, text {int(idx[w])}): got {have[int(bad[0])].tolist()} "
                f"want {want[int(bad[0])].tolist()}; {len(bad)} rows differ in its chunk")
    return None


@functools.lru_cache(maxsize=None)
def text_rows(k, n_kmers, L, E):
    """Per-text expected rows at edit budget E, from the CPU references of the hits, positions and spans
    tests: dict of
      hits (E + 1, n_texts, words), pos / start (8, n_texts, words)   int32 views of the matrix layouts
      hit bool (E + 1, n_texts, n_kmers), prof uint64 (n_texts, E + 1, n_kmers, L): each text's own profile."""
    km, texts, _, _ = dense_dictionary(k, n_kmers, L)
    hit, pos, _ = expected_positions(k, km, texts, E)
    start, _ = starts_of(k, km, texts, hit, pos)
    prof = np.stack([profile_of(hit[:, t:t + 1], pos[t:t + 1], L) for t in range(len(texts))]).astype(np.uint64)
    i32 = lambda a: np.ascontiguousarray(a, np.uint32).view(np.int32)  # noqa: E731
    return {"hits": i32(pack_hits(hit)), "pos": i32(pack_positions(pos)), "start": i32(pack_starts(start, hit[E])),
            "hit": hit, "prof": prof}


PROFILE_DEPTHS = (8, 32)  # 32: the depth at which hit_flank.h fl_run takes three code words


@functools.lru_cache(maxsize=None)
def text_profiles(k, n_kmers, L, E):
    """Per-text flank and edit profiles at edit budget E, each text alone with its own hits, end positions and
    starts_of starts (the CPU references of the flank and edit tests): dict of
      flank[D, plane, with_start] uint64 (n_texts, 2, n_kmers, D, 5)   D in PROFILE_DEPTHS, plane in (0, E);
                                                                       without starts the left half is zeros
      edit[plane]                 uint64 (n_texts, n_kmers, k, 12)
      hit bool (E + 1, n_texts, n_kmers), pos / start int16 (n_texts, n_kmers)
      counted bool (n_texts, n_kmers): the top-level pairs that meet the edit pass's conditions.
    An image's expected profile is image_profile(bincount(idx), per_text): a cell is at most the window count."""
    from tests.edit_cases import alignments
    from tests.flank_cases import flank_profile_of

    km, texts, _, _ = dense_dictionary(k, n_kmers, L)
    hit, pos, _ = expected_positions(k, km, texts, E)
    start, _ = starts_of(k, km, texts, hit, pos)
    one = lambda a, t: a[t:t + 1]  # noqa: E731
    flank, edit = {}, {}
    counted = np.zeros(hit.shape[1:], bool)
    for plane in (0, E):
        al = [alignments(k, km, one(texts, t), one(hit[plane], t), one(pos, t), one(start, t)) for t in range(len(texts))]
        edit[plane] = np.stack([a["profile"] for a in al]).astype(np.uint64)
        if plane == E:
            for t, a in enumerate(al):
                counted[t, a["cs"]] = a["counted"]
        for D in PROFILE_DEPTHS:
            for with_start in (True, False):
                flank[D, plane, with_start] = np.stack(
                    [flank_profile_of(one(texts, t), one(hit[plane], t), one(pos, t), one(start, t) if with_start else None, D)
                     for t in range(len(texts))]).astype(np.uint64)
    return {"flank": flank, "edit": edit, "hit": hit, "pos": pos, "start": start, "counted": counted}


def image_profile(n, per_text):
    """The profile of an image whose texts occur n = text_counts(idx, ...) times: uint64, exact."""
    return np.einsum("t,t...->...", n.astype(np.uint64), per_text.astype(np.uint64))


def first_cell(got, want, axes):
    """None if got == want, else a message naming the first differing cell by its axes."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    at = tuple(int(x) for x in bad[0])
    return f"{len(bad)} cells differ, first at {dict(zip(axes, at))}: got {int(got[at])} want {int(want[at])}"


# ---- the sparse image ----

SPARSE_KMERS = 64


def _region(rng, kmers, k, n, p_n):
    """n bases with p_n N; a candidate with 0..3 edits every ~70 bases, one at the first base and one at
    the end."""
    s = list(cases.rand_seq(rng, n, p_n))
    at = 0
    while at + k + 3 <= n:
        pl = cases.mutate(rng, cases.kmer_string(rng.choice(kmers), k), rng.randint(0, 3))
        s[at:at + len(pl)] = pl
        at += len(pl) + rng.randint(20, 90)
    pl = cases.mutate(rng, cases.kmer_string(rng.choice(kmers), k), rng.randint(0, 2))[:n]
    s[n - len(pl):] = pl
    return "".join(s[:n])


@functools.lru_cache(maxsize=None)
def sparse_case(k, n_bases=TOP_BASES, boundaries=BOUNDARIES[:2], seed=5):
    """(kmers, regions, windows): `regions` [(start, text)] are written into a zero image (start a multiple
    of 32, disjoint); `windows` [(start, length)] lie inside them (they may overlap one another -- ac_windows
    allows it -- and what follows a window in its last slot is the region's next bases, not zeros).
    Per boundary b: a window ending exactly at b, one starting at b, a short one and a long one straddling it,
    the long one (1000 bases from b - 512) with a 256-base fetch seam on b; ragged windows of 20..300 bases
    elsewhere, some of 600..1500; a window at base 0; one whose last base is base n_bases - 1.  About 1 % N
    in most regions."""
    rng = random.Random(seed * 1000 + k)
    kmers = [cases.kmer_value(cases.rand_seq(rng, k)) for _ in range(SPARSE_KMERS)]
    regions, windows = [], []

    def region(start, n, p_n=0.01):
        assert start % 32 == 0 and 0 <= start and start + n <= n_bases, (start, n)
        assert all(start + n <= s or s + len(t) <= start for s, t in regions), "regions overlap"
        regions.append((start, _region(rng, kmers, k, n, p_n)))

    region(0, 300)
    windows += [(0, 133), (160, 20)]
    for b in boundaries:
        region(b - 512, 1536)
        windows += [(b - 96, 96), (b - 256, 256), (b, 77), (b, 300), (b - 32, 50), (b - 512, 1000), (b - 480, 1500 - 32),
                    (b + 320, 299), (b + 640, 33)]
    region(n_bases - 1024, 1024)
    windows += [(n_bases - 288, 288), (n_bases - 1024, 700), (n_bases - 32, 32), (n_bases - 64, 41)]
    for i in range(14):  # elsewhere, wherever the draw falls clear of the regions above
        n = rng.randint(600, 1500) if i % 5 == 4 else rng.randint(20, 300)
        while True:
            start = rng.randrange(0, n_bases - n) // 32 * 32
            if all(start + n <= s or s + len(t) <= start for s, t in regions):
                break
        region(start, n, p_n=0.02 if i % 2 else 0.0)
        windows.append((start, n))
    return np.array(kmers, np.uint64), regions, windows


def window_text(regions, start, length):
    for s, t in regions:
        if s <= start and start + length <= s + len(t):
            return t[start - s:start - s + length]
    raise AssertionError("a window outside every region")


def sparse_windows(regions, windows):
    return [window_text(regions, s, n) for s, n in windows]


def sparse_image(regions, n_bases, device=None):
    """(codes, nmask) of n_bases, zero but for the regions, each packed on the host and written by slice
    assignment."""
    codes, nmask = zeros(n_bases // 16, np.int32, device), zeros(n_bases // 32, np.int32, device)
    for s, t in regions:
        img = ac.pack_windows([t])
        codes[s // 16:s // 16 + img.codes.size] = on(img.codes.view(np.int32), device)
        nmask[s // 32:s // 32 + img.nmask.size] = on(img.nmask.view(np.int32), device)
    return codes, nmask


@functools.lru_cache(maxsize=None)
def sparse_expected(k, n_bases=TOP_BASES, boundaries=BOUNDARIES[:2]):
    km, regions, windows = sparse_case(k, n_bases, boundaries)
    return oracle.count_myers(k, km, sparse_windows(regions, windows))
