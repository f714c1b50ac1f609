"""Host-side mirror of the reference's approximate-count interface.

``error_count(sequences, exact_count, nb_thread, k, v)`` has the argument
meaning of ``errorCount`` (approx_counter.cpp:531): ``sequences`` is the
sampled window set, ``exact_count`` the (k-mer, exact count) pairs kept by
get_most_frequent / get_solid_kmers (887-899), and the result maps every
candidate k-mer to its approximate count (``results[kmer] = total``, 596).
``nb_thread`` and ``v`` are accepted for signature parity; the work runs on the
GPU through the C ABI of include/approx_counter_amd.h.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import ACDna5Windows, ACJob, ACSampleJob, ACSegment, ACWindows, check

_DNA5 = np.full(256, 4, dtype=np.uint8)
for _c, _v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"U", 3)):
    _DNA5[_c[0]] = _v
    _DNA5[_c.lower()[0]] = _v


def to_dna5(seq) -> np.ndarray:
    """Dna5 ordinal bytes (A0 C1 G2 T3, anything else 4), as SeqAn's Dna5String."""
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq, dtype=np.uint8)
    if isinstance(seq, str):
        seq = seq.encode()
    return _DNA5[np.frombuffer(bytes(seq), dtype=np.uint8)]


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


class PackedSample:
    """Host window image (see ac_windows in include/approx_counter_amd.h)."""

    def __init__(self, codes, nmask, start, length, n_bases):
        self.codes, self.nmask, self.start, self.length = codes, nmask, start, length
        self.n_bases = int(n_bases)

    @property
    def n_windows(self) -> int:
        return int(self.length.size)

    @property
    def total_bases(self) -> int:
        return int(self.length.sum(dtype=np.uint64))

    def as_struct(self) -> ACWindows:
        return ACWindows(_ptr(self.codes, ctypes.c_uint32), _ptr(self.nmask, ctypes.c_uint32),
                         _ptr(self.start, ctypes.c_uint64), _ptr(self.length, ctypes.c_uint32),
                         self.n_windows, self.n_bases)

    def equal_window_len(self):
        """The common window length when every window has it and window w starts at base
        w * ceil32(length) (the layout ac_error_count_device reads without descriptors when given window_len),
        else None."""
        n = self.n_windows
        if n == 0:
            return None
        ln = int(self.length[0])
        stride = (ln + 31) // 32 * 32
        if not np.all(self.length == ln):
            return None
        if not np.array_equal(self.start, np.arange(n, dtype=np.uint64) * np.uint64(stride)):
            return None
        return ln


def pack_windows(windows) -> PackedSample:
    """Pack Dna5 windows into the 2-bit + N-mask image with ac_pack_windows.
    `windows` is a sequence of strings / byte strings / Dna5 ordinal arrays, or a
    2-D uint8 array of equal-length windows (Dna5 ordinals, one per row)."""
    L = _lib.load()
    if isinstance(windows, np.ndarray) and windows.ndim == 2:
        n, wl = windows.shape
        arrs = [None] * n
        lengths = np.full(n, wl, dtype=np.uint32)
        starts = np.arange(n, dtype=np.uint64) * np.uint64(wl)
        flat = np.ascontiguousarray(windows, dtype=np.uint8).reshape(-1)
        if flat.size == 0:
            flat = np.zeros(1, np.uint8)
    else:
        arrs = [to_dna5(w) for w in windows]
        lengths = np.array([a.size for a in arrs], dtype=np.uint32)
        starts = np.zeros(len(arrs), dtype=np.uint64)
        if len(arrs) > 1:
            starts[1:] = np.cumsum(lengths[:-1], dtype=np.uint64)
        flat = np.concatenate(arrs) if arrs and lengths.sum() else np.zeros(1, np.uint8)
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    lens_c = lengths if lengths.size else np.zeros(1, np.uint32)
    n_bases = int(L.ac_image_bases(_ptr(lens_c, ctypes.c_uint32), len(arrs)))
    codes = np.zeros(n_bases // 16, dtype=np.uint32)
    nmask = np.zeros(n_bases // 32, dtype=np.uint32)
    out_start = np.zeros(max(len(arrs), 1), dtype=np.uint64)
    out_len = np.zeros(max(len(arrs), 1), dtype=np.uint32)
    st = L.ac_pack_windows(_ptr(flat, ctypes.c_uint8),
                           _ptr(starts if starts.size else np.zeros(1, np.uint64), ctypes.c_uint64),
                           _ptr(lens_c, ctypes.c_uint32), len(arrs),
                           _ptr(codes, ctypes.c_uint32), _ptr(nmask, ctypes.c_uint32),
                           _ptr(out_start, ctypes.c_uint64), _ptr(out_len, ctypes.c_uint32), n_bases)
    check(st)
    return PackedSample(codes, nmask, out_start[: len(arrs)], out_len[: len(arrs)], n_bases)


def hits_words(n_kmers: int, n_windows: int, max_errors: int = 2) -> int:
    """ac_window_hits_words: the u32 words of one segment's hit matrix, (E + 1) x n_windows x ceil(n_kmers / 32)."""
    return (int(max_errors) + 1) * int(n_windows) * ((int(n_kmers) + 31) // 32)


def unpack_hits(levels, n_kmers: int) -> np.ndarray:
    """A hit matrix's bits: `levels` is (E + 1, n_windows, words) uint32, bit c % 32 of word c // 32 =
    candidate c; returns bool (E + 1, n_windows, n_kmers).  Pure numpy."""
    lv = np.ascontiguousarray(levels, dtype="<u4")
    if lv.ndim != 3 or lv.shape[2] != (int(n_kmers) + 31) // 32:
        raise ValueError("hit matrix must be (levels, n_windows, ceil(n_kmers / 32))")
    bits = np.unpackbits(lv.view(np.uint8).reshape(lv.shape[0], lv.shape[1], lv.shape[2] * 4), axis=-1,
                         bitorder="little")
    return bits[:, :, : int(n_kmers)].astype(bool)


def distances_from_hits(hit) -> np.ndarray:
    """uint8 (n_windows, n_kmers) distances from nested levels (`hit`: bool (E + 1, n_windows, n_kmers),
    hit[e] = within e edits): the first level that holds the pair, E + 1 meaning "more than E".  Levels
    that do not nest (a pair at level e missing from level e + 1) raise ValueError."""
    hit = np.asarray(hit, dtype=bool)
    if hit.ndim != 3:
        raise ValueError("hit must be (levels, n_windows, n_kmers)")
    if (hit[:-1] & ~hit[1:]).any():
        raise ValueError("hit levels do not nest")
    return (hit.shape[0] - hit.sum(axis=0)).astype(np.uint8)


def positions_words(n_kmers: int, n_windows: int) -> int:
    """ac_window_positions_words: the u32 words of one segment's position matrix, 8 x n_windows x ceil(n_kmers / 32)."""
    return 8 * int(n_windows) * ((int(n_kmers) + 31) // 32)


def cooccurrence_words(n_kmers: int, levels: int = 1) -> int:
    """ac_hit_cooccurrence_words: the u32 words of a co-occurrence result, levels x n_kmers x n_kmers."""
    return int(levels) * int(n_kmers) * int(n_kmers)


def cross_cooccurrence_words(n_a: int, n_b: int, levels: int = 1) -> int:
    """ac_hit_cross_cooccurrence_words: the u32 words of a cross co-occurrence result, levels x n_a x n_b."""
    return int(levels) * int(n_a) * int(n_b)


def flank_words(n_kmers: int, depth: int) -> int:
    """ac_hit_flank_words: the u32 words of a flank profile, 2 sides x n_kmers x depth x 5 symbols."""
    return 2 * int(n_kmers) * int(depth) * 5


def flank_consensus(profile, min_windows: int = 1, min_share: float = 0.5) -> list:
    """The majority extension of every k-mer from its flank profile (uint32 (2, n_kmers, D, 5): side 0 = the
    bases after the occurrence's end, 1 = before its start, nearest first; A C G T N).  Returns one
    (left, right) pair of strings per k-mer, the left one in reading order (its last base is the one just
    before the occurrence).  A side is extended from the nearest column while the column's total (N
    included) is at least min_windows and its largest A/C/G/T count is more than min_share of the total; it
    stops at the first column that fails.  Pure numpy."""
    prof = np.asarray(profile)
    if prof.ndim != 4 or prof.shape[0] != 2 or prof.shape[3] != 5:
        raise ValueError("flank profile must be (2, n_kmers, depth, 5)")
    prof = prof.astype(np.int64)
    total = prof.sum(axis=3)
    best = prof[..., :4].argmax(axis=3)
    top = prof[..., :4].max(axis=3)
    ok = (total >= max(int(min_windows), 1)) & (top > float(min_share) * total)
    n = np.where(ok.all(axis=2), ok.shape[2], (~ok).argmax(axis=2))  # the columns before the first failing one
    out = []
    for c in range(prof.shape[1]):
        right = "".join("ACGT"[b] for b in best[0, c, : n[0, c]])
        left = "".join("ACGT"[b] for b in best[1, c, : n[1, c]])[::-1]
        out.append((left, right))
    return out


def edit_words(n_kmers: int, k: int) -> int:
    """ac_hit_edit_words: the u32 words of an edit profile, n_kmers x k x 12 operations."""
    return int(n_kmers) * int(k) * 12


def edit_consensus(profile, kmers, k: int, min_windows: int = 1, min_share: float = 0.5) -> list:
    """The corrected string of every k-mer from its edit profile (uint32 (n_kmers, k, 12): per base of the
    k-mer the windows by what the best occurrence holds there -- 0 match, 1..5 substituted by A C G T N,
    6 deleted, 7..11 followed by an inserted A C G T N).  Per k-mer n is the windows its first base was aligned
    in (operations 0..6); below min_windows the k-mer is returned as it is.  Otherwise every base is dropped
    where it was deleted in more than min_share of the n windows, else replaced by the A/C/G/T that
    substituted it in more than min_share of them, else kept; and after every base, kept or dropped, the
    A/C/G/T inserted after it in more than min_share of them is appended.  min_share in [0.5, 1): at most
    one base can hold a majority.  Pure numpy."""
    prof = np.asarray(profile)
    k = int(k)
    kmers = [int(v) for v in np.asarray(kmers).reshape(-1)]
    if prof.ndim != 3 or prof.shape != (len(kmers), k, 12):
        raise ValueError("edit profile must be (n_kmers, k, 12)")
    if not 0.5 <= float(min_share) < 1.0:
        raise ValueError("min_share must be in [0.5, 1)")
    prof = prof.astype(np.int64)
    out = []
    for c, v in enumerate(kmers):
        s = "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))
        n = int(prof[c, 0, :7].sum()) if k else 0
        if n < int(min_windows):
            out.append(s)
            continue
        need, t = float(min_share) * n, []
        for i in range(k):
            sub, ins = prof[c, i, 1:5], prof[c, i, 7:11]
            if not prof[c, i, 6] > need:
                t.append("ACGT"[int(sub.argmax())] if sub.max() > need else s[i])
            if ins.max() > need:
                t.append("ACGT"[int(ins.argmax())])
        out.append("".join(t))
    return out


def unpack_positions(planes, hit_E, n_kmers: int) -> np.ndarray:
    """A position matrix's values: `planes` is (8, n_windows, words) uint32, plane b holding bit b of
    pos - 1; `hit_E` is bool (n_windows, n_kmers), the pairs within the budget (level E of the hit
    matrix).  Returns int16 (n_windows, n_kmers): the exclusive end offset 1..L of the leftmost occurrence
    at the best distance, -1 where hit_E is False.  Pure numpy."""
    pl = np.ascontiguousarray(planes, dtype="<u4")
    if pl.ndim != 3 or pl.shape[0] != 8 or pl.shape[2] != (int(n_kmers) + 31) // 32:
        raise ValueError("position matrix must be (8, n_windows, ceil(n_kmers / 32))")
    hit_E = np.asarray(hit_E, dtype=bool)
    if hit_E.shape != (pl.shape[1], int(n_kmers)):
        raise ValueError("hit_E must be (n_windows, n_kmers)")
    bits = np.unpackbits(pl.view(np.uint8).reshape(8, pl.shape[1], pl.shape[2] * 4), axis=-1,
                         bitorder="little")[:, :, : int(n_kmers)]
    pos = np.zeros(hit_E.shape, dtype=np.int16)
    for b in range(8):
        pos |= bits[b].astype(np.int16) << b
    return np.where(hit_E, pos + 1, -1).astype(np.int16)


def unpack_starts(planes, hit_E, n_kmers: int) -> np.ndarray:
    """A start matrix's values (ac_hit_start_positions_device): the layout of a position matrix, plane b
    holding bit b of the start itself.  Returns int16 (n_windows, n_kmers): the 0-based inclusive start of
    the shortest occurrence ending at the pair's end position at the best distance, -1 where hit_E is
    False.  Pure numpy."""
    return np.where(np.asarray(hit_E, dtype=bool), unpack_positions(planes, hit_E, n_kmers) - 1, -1).astype(np.int16)


class WindowHits:
    """One part's counts and hit levels (ac_window_hits_samples): which windows hold each k-mer within
    0..E edits -- the reference's tcount[errors][read] (approx_counter.cpp:553-565) before it is summed.
    From window_hits(..., positions=True) also the match end positions (ac_window_positions_samples); from
    window_hits(..., spans=True) the match starts as well (ac_window_spans_samples)."""

    def __init__(self, counts, levels, n_kmers: int, planes=None, window_len: int = 0, counter=None, starts=None,
                 k: int = 0, flanks=None, edits=None):
        self.counts = counts
        self.levels = np.asarray(levels, dtype=np.uint32)  # (E + 1, n_windows, words)
        self.n_kmers = int(n_kmers)
        self.planes = None if planes is None else np.asarray(planes, dtype=np.uint32)  # (8, n_windows, words)
        self.starts = None if starts is None else np.asarray(starts, dtype=np.uint32)  # (8, n_windows, words)
        self.window_len = int(window_len)
        self.k = int(k)
        self.flanks = None if flanks is None else np.asarray(flanks, dtype=np.uint32)  # (2, n_kmers, D, 5)
        self.edits = None if edits is None else np.asarray(edits, dtype=np.uint32)  # (n_kmers, k, 12)
        self._counter = counter

    def flank_profile(self) -> np.ndarray:
        """uint32 (2, n_kmers, D, 5): per k-mer the windows (within E edits) by the base -- A C G T N -- at each
        of the D bases after the best occurrence's end (side 0) and before its start (side 1), nearest first;
        a base outside the window is not counted (ac_window_flanks_samples)."""
        if self.flanks is None:
            raise ValueError("no flank profile: ask window_hits(..., flanks=D)")
        return self.flanks

    def edit_profile(self) -> np.ndarray:
        """uint32 (n_kmers, k, 12): per k-mer and base the windows (within E edits) by what the best occurrence
        holds there -- 0 match, 1..5 substituted by A C G T N, 6 deleted, 7..11 followed by an inserted
        A C G T N (ac_window_edits_samples; edit_consensus(...) gives the corrected k-mers)."""
        if self.edits is None:
            raise ValueError("no edit profile: ask window_hits(..., edits=True)")
        return self.edits

    def start_positions(self) -> np.ndarray:
        """int16 (n_windows, n_kmers): where the best occurrence starts (0-based, inclusive: the shortest
        substring ending at end_positions() at the best distance), -1 where the window does not hold the
        k-mer within E edits."""
        if self.starts is None:
            raise ValueError("no spans: ask window_hits(..., spans=True)")
        return unpack_starts(self.starts, self.hit(self.max_errors), self.n_kmers)

    def span_lengths(self) -> np.ndarray:
        """int16 (n_windows, n_kmers): end - start, k - d .. k + d, -1 where there is no hit."""
        start = self.start_positions()
        return np.where(start >= 0, self.end_positions() - start, -1).astype(np.int16)

    def length_profile(self) -> np.ndarray:
        """uint32 (E + 1, n_kmers, 2 E + 1): the windows at distance exactly d whose occurrence has length
        k - E .. k + E (an insertion lengthens it, a deletion shortens it).  numpy."""
        if not self.k:
            raise ValueError("no k-mer length: this object was not made by window_hits(..., spans=True)")
        E, ln = self.max_errors, self.span_lengths()
        d = self.distances()
        prof = np.zeros((E + 1, self.n_kmers, 2 * E + 1), np.uint32)
        ws, cs = np.nonzero(ln >= 0)
        at = ln[ws, cs].astype(np.int64) - (self.k - E)
        ok = (at >= 0) & (at <= 2 * E)
        np.add.at(prof, (d[ws, cs][ok], cs[ok], at[ok]), 1)
        return prof

    def start_profile(self) -> np.ndarray:
        """uint32 (E + 1, n_kmers, L): the windows at distance exactly d whose best occurrence starts at base
        p, computed on the device (ac_hit_position_profile_device on the start matrix)."""
        if self.starts is None or self._counter is None:
            raise ValueError("no spans: ask window_hits(..., spans=True)")
        return self._profile(self.starts)

    def end_positions(self) -> np.ndarray:
        """int16 (n_windows, n_kmers): where the leftmost occurrence at the best distance ends (exclusive,
        1..L), -1 where the window does not hold the k-mer within E edits."""
        if self.planes is None:
            raise ValueError("no positions: ask window_hits(..., positions=True)")
        return unpack_positions(self.planes, self.hit(self.max_errors), self.n_kmers)

    def position_profile(self) -> np.ndarray:
        """uint32 (E + 1, n_kmers, L): the windows at distance exactly d whose best occurrence ends at base
        p + 1, computed on the device (ac_hit_position_profile_device)."""
        if self.planes is None or self._counter is None:
            raise ValueError("no positions: ask window_hits(..., positions=True)")
        return self._profile(self.planes)

    def _profile(self, planes) -> np.ndarray:
        import torch

        lv, nw, _ = self.levels.shape
        if not (self.n_kmers and nw):
            return np.zeros((lv, self.n_kmers, self.window_len), np.uint32)
        dev = torch.device("cuda")
        h = torch.from_numpy(self.levels.view(np.int32)).to(dev)
        p = torch.from_numpy(np.ascontiguousarray(planes).view(np.int32)).to(dev)
        out = self._counter.hit_position_profile(h, p, self.n_kmers, nw, lv, self.window_len)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)

    @property
    def max_errors(self) -> int:
        return int(self.levels.shape[0]) - 1

    def hit(self, e: int) -> np.ndarray:
        """bool (n_windows, n_kmers): window w holds k-mer c within e edits."""
        return unpack_hits(self.levels[e:e + 1], self.n_kmers)[0]

    def distances(self) -> np.ndarray:
        """uint8 (n_windows, n_kmers): min(d, E + 1)."""
        return distances_from_hits(unpack_hits(self.levels, self.n_kmers))

    def level_counts(self) -> np.ndarray:
        """uint64 (E + 1, n_kmers): the windows within e edits of every k-mer; their sum over e is .counts."""
        return unpack_hits(self.levels, self.n_kmers).sum(axis=1, dtype=np.uint64)

    def cooccurrence(self, e=None) -> np.ndarray:
        """uint32 (n_kmers, n_kmers): entry (a, b) = the windows that hold k-mers a and b both within e edits
        (default: the top level E); symmetric, its diagonal level_counts()[e].  Computed on the device
        (ac_hit_cooccurrence_device) when the counter that made this object is attached, else with numpy."""
        e = self.max_errors if e is None else int(e)
        if not 0 <= e <= self.max_errors:
            raise ValueError(f"level {e} is outside 0..{self.max_errors}")
        nw = int(self.levels.shape[1])
        if self._counter is None or not (self.n_kmers and nw):
            h = self.hit(e).astype(np.float32)  # (exact: every sum is an integer below 2^24)
            if nw >= 1 << 24:
                h = h.astype(np.float64)
            return (h.T @ h).astype(np.uint32)
        import torch

        dev = torch.device("cuda")
        plane = torch.from_numpy(np.ascontiguousarray(self.levels[e]).view(np.int32)).to(dev)
        out = self._counter.hit_cooccurrence(plane, self.n_kmers, nw, 1)
        torch.cuda.synchronize(dev)
        return out[0].cpu().numpy().view(np.uint32)

    def cross_cooccurrence(self, other, e=None, e_other=None) -> np.ndarray:
        """uint32 (self.n_kmers, other.n_kmers): entry (a, b) = the windows that hold this object's k-mer a
        within e edits and `other`'s k-mer b within e_other edits (defaults: each object's top level).  The
        two objects must be over the same windows, row w of both the same read (two parts over paired
        windows, or the same object twice: wh.cross_cooccurrence(wh, 0, wh.max_errors) pairs two levels).
        Computed on the device (ac_hit_cross_cooccurrence_device) when either object has its counter attached,
        else with numpy."""
        e = self.max_errors if e is None else int(e)
        e_other = other.max_errors if e_other is None else int(e_other)
        if not 0 <= e <= self.max_errors:
            raise ValueError(f"level {e} is outside 0..{self.max_errors}")
        if not 0 <= e_other <= other.max_errors:
            raise ValueError(f"level {e_other} of the other matrix is outside 0..{other.max_errors}")
        nw = int(self.levels.shape[1])
        if int(other.levels.shape[1]) != nw:
            raise ValueError(f"the two matrices hold {nw} and {int(other.levels.shape[1])} windows: not the same reads")
        counter = self._counter if self._counter is not None else other._counter
        if counter is None or not (self.n_kmers and other.n_kmers and nw):
            dt = np.float64 if nw >= 1 << 24 else np.float32  # (float32 is exact: every sum is an integer below 2^24)
            return (self.hit(e).astype(dt).T @ other.hit(e_other).astype(dt)).astype(np.uint32)
        import torch

        dev = torch.device("cuda")
        a = torch.from_numpy(np.ascontiguousarray(self.levels[e]).view(np.int32)).to(dev)
        b = torch.from_numpy(np.ascontiguousarray(other.levels[e_other]).view(np.int32)).to(dev)
        out = counter.hit_cross_cooccurrence(a, self.n_kmers, b, other.n_kmers, nw, 1)
        torch.cuda.synchronize(dev)
        return out[0].cpu().numpy().view(np.uint32)

    def window_counts(self) -> np.ndarray:
        """uint32 (E + 1, n_windows): how many of the k-mers every window holds within e edits."""
        lv, nw, _ = self.levels.shape
        if self._counter is None or not (self.n_kmers and nw):
            return unpack_hits(self.levels, self.n_kmers).sum(axis=2, dtype=np.uint32)
        import torch

        dev = torch.device("cuda")
        h = torch.from_numpy(np.ascontiguousarray(self.levels).view(np.int32)).to(dev)
        out = self._counter.hit_window_counts(h, self.n_kmers, nw, lv)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)


class _PinnedBlock:
    """One ac_host_alloc block, released when the last array viewing it goes (numpy keeps this
    object as the arrays' base)."""

    def __init__(self, nbytes: int):
        L = _lib.load()
        p = ctypes.c_void_p()
        check(L.ac_host_alloc(max(int(nbytes), 1), ctypes.byref(p)))
        self._L, self.ptr, self.nbytes = L, p.value, max(int(nbytes), 1)
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False),
                                    "version": 3}

    def __del__(self):
        if getattr(self, "ptr", None):
            self._L.ac_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


def pinned_empty(n: int, dtype) -> np.ndarray:
    """An uninitialised array of n elements in pinned, device-mapped host memory (ac_host_alloc)."""
    dt = np.dtype(dtype)
    return np.asarray(_PinnedBlock(n * dt.itemsize)).view(dt)[:n]


def pinned_copy(a) -> np.ndarray:
    """A copy of `a` in ac_host_alloc memory."""
    a = np.ascontiguousarray(a)
    out = pinned_empty(max(a.size, 1), a.dtype)[: a.size]
    out[...] = a.reshape(-1)
    return out.reshape(a.shape)


class Dna5Sample:
    """A sample as errorCount receives it: a StringSet<Dna5String>
    (approx_counter.cpp:38), i.e. Dna5 ordinal bytes concatenated, with each
    window's offset and length (ac_dna5_windows)."""

    def __init__(self, bases, offset, length):
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.offset = np.ascontiguousarray(offset, dtype=np.uint64)
        self.length = np.ascontiguousarray(length, dtype=np.uint32)
        if self.offset.shape != self.length.shape:
            raise ValueError("Dna5Sample: offset and length differ in size")
        # ac_dna5_windows carries no size for `bases`: the packer would read past the buffer
        if self.length.size and int((self.offset + self.length.astype(np.uint64)).max()) > self.bases.size:
            raise ValueError("Dna5Sample: a window reaches past the end of `bases`")
        if self.bases.size == 0:
            self.bases = np.zeros(1, np.uint8)

    @classmethod
    def from_windows(cls, windows) -> "Dna5Sample":
        """From a sequence of strings / Dna5 arrays, or a 2-D uint8 array of
        equal-length windows (one per row)."""
        if isinstance(windows, np.ndarray) and windows.ndim == 2:
            n, wl = windows.shape
            return cls(windows.reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(wl),
                       np.full(n, wl, dtype=np.uint32))
        arrs = [to_dna5(w) for w in windows]
        length = np.array([a.size for a in arrs], dtype=np.uint32)
        offset = np.zeros(len(arrs), dtype=np.uint64)
        if len(arrs) > 1:
            offset[1:] = np.cumsum(length[:-1], dtype=np.uint64)
        bases = np.concatenate(arrs) if arrs and length.sum() else np.zeros(1, np.uint8)
        return cls(bases, offset, length)

    def pinned(self) -> "Dna5Sample":
        """The same sample with its bytes and offsets in ac_host_alloc memory: ac_error_count_jobs
        then packs it on the device when its windows have one length of 1..256 bases."""
        return Dna5Sample(pinned_copy(self.bases), pinned_copy(self.offset), pinned_copy(self.length))

    def subset(self, lo: int, hi: int) -> "Dna5Sample":
        """Windows [lo, hi) (a shard), sharing the bases."""
        return Dna5Sample(self.bases, self.offset[lo:hi], self.length[lo:hi])

    @property
    def n_windows(self) -> int:
        return int(self.length.size)

    @property
    def total_bases(self) -> int:
        return int(self.length.sum(dtype=np.uint64))

    def as_struct(self) -> ACDna5Windows:
        one = lambda a, t: _ptr(a if a.size else np.zeros(1, a.dtype), t)  # noqa: E731
        return ACDna5Windows(_ptr(self.bases, ctypes.c_uint8), one(self.offset, ctypes.c_uint64),
                             one(self.length, ctypes.c_uint32), self.n_windows)


class Jobs:
    """A reusable ac_job array (both read ends of one run, or shards): the
    k-mer and count arrays are kept alive with it."""

    def __init__(self, parts):
        """`parts`: sequence of (kmers, Dna5Sample)."""
        self.kmers = [np.ascontiguousarray(np.asarray(km, dtype=np.uint64)) for km, _ in parts]
        self.samples = [smp for _, smp in parts]
        self.counts = [np.zeros(max(k.size, 1), dtype=np.uint64) for k in self.kmers]
        self.n_counts = sum(int(k.size) for k in self.kmers)
        self.array = (ACJob * len(parts))(*[
            ACJob(_ptr(km if km.size else np.zeros(1, np.uint64), ctypes.c_uint64), int(km.size), smp.as_struct(),
                  _ptr(c, ctypes.c_uint64))
            for km, smp, c in zip(self.kmers, self.samples, self.counts)])

    def results(self):
        return [c[: k.size] for c, k in zip(self.counts, self.kmers)]


class ApproxCounter:
    """One device context (ac_create / ac_destroy), or with n_gpus a context
    whose host-buffer counts are sharded over that many devices (ac_create_multi)."""

    def __init__(self, device: int = -1, n_gpus: int = 0, max_errors: int = 2):
        """max_errors: the edit budget E of the approximate counts (set_max_errors); 2 is the reference's."""
        L = _lib.load()
        self._L = L
        h = ctypes.c_void_p()
        if n_gpus:
            check(L.ac_create_multi(ctypes.byref(h), int(n_gpus)))
        else:
            check(L.ac_create(ctypes.byref(h), device))
        self._h = h
        if max_errors != 2:
            try:
                self.set_max_errors(max_errors)
            except Exception:
                self.close()
                raise

    def set_max_errors(self, max_errors: int) -> None:
        """ac_set_max_errors: every approximate count of this context from now on adds
        max(0, E + 1 - d) per window, E = max_errors in 0..3 (2: the reference's contract).  Another
        budget than 2 counts only where the bit-sliced kernel does -- k = 16 or 18..32, every job with
        equal windows of 1..256 bases -- and any other call then raises (AC_ERR_INVALID) instead of
        counting under another budget.  The exact count does not depend on it."""
        if not hasattr(self._L, "ac_set_max_errors"):
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "this build of the library has no ac_set_max_errors")
        if not 0 <= int(max_errors) <= 3:
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "max_errors must be 0..3")
        check(self._L.ac_set_max_errors(self._h, int(max_errors)), self._h)

    @property
    def max_errors(self) -> int:
        """ac_max_errors: the context's edit budget."""
        return int(self._L.ac_max_errors(self._h)) if hasattr(self._L, "ac_max_errors") else 2

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.ac_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def count(self, k: int, kmers, sample: PackedSample) -> np.ndarray:
        """ac_error_count: host arrays in, uint64 counts out (input order)."""
        kmers = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
        counts = np.zeros(max(kmers.size, 1), dtype=np.uint64)
        ws = sample.as_struct()
        st = self._L.ac_error_count(self._h, int(k),
                                    _ptr(kmers if kmers.size else np.zeros(1, np.uint64), ctypes.c_uint64),
                                    int(kmers.size), ctypes.byref(ws), _ptr(counts, ctypes.c_uint64))
        check(st, self._h)
        return counts[: kmers.size]

    def count_words(self, k: int, kmers, win_bits, win_nmask, win_word_offset, win_len) -> np.ndarray:
        """ac_count (SURVEY.md 8(b) layout): 2-bit words, N bitmap, per-window word offset
        (even) and uint16 length."""
        kmers = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
        bits = np.ascontiguousarray(win_bits, dtype=np.uint32)
        nm = np.ascontiguousarray(win_nmask, dtype=np.uint32)
        off = np.ascontiguousarray(win_word_offset, dtype=np.uint64)
        ln = np.ascontiguousarray(win_len, dtype=np.uint16)
        counts = np.zeros(max(kmers.size, 1), dtype=np.uint64)
        one = lambda a, t: _ptr(a if a.size else np.zeros(1, a.dtype), t)  # noqa: E731
        st = self._L.ac_count(self._h, int(k), one(kmers, ctypes.c_uint64), int(kmers.size), one(bits, ctypes.c_uint32),
                              one(nm, ctypes.c_uint32), one(off, ctypes.c_uint64), one(ln, ctypes.c_uint16),
                              int(ln.size), _ptr(counts, ctypes.c_uint64))
        check(st, self._h)
        return counts[: kmers.size]

    def count_jobs(self, k: int, jobs) -> list:
        """ac_error_count_jobs: the whole stage from Dna5 host buffers (pack, one DMA, one
        fused launch, counts back), up to 4 jobs.  `jobs` is a Jobs object or a sequence of
        (kmers, Dna5Sample / windows); returns the uint64 counts of every job."""
        if not isinstance(jobs, Jobs):
            jobs = Jobs([(km, w if isinstance(w, Dna5Sample) else Dna5Sample.from_windows(w)) for km, w in jobs])
        st = self._L.ac_error_count_jobs(self._h, int(k), jobs.array, len(jobs.array))
        check(st, self._h)
        return jobs.results()

    def submit_jobs(self, k: int, jobs: "Jobs", d_counts, stream=None, hits=None, positions=None) -> None:
        """ac_error_count_jobs_submit: pack + send + launch; uint32 counts (jobs concatenated)
        go to the device tensor `d_counts` on `stream` (asynchronous).
        hits: one device tensor per job (None for a job without work), of hits_words(...) int32 / uint32 each
        -- ac_window_hits_jobs_submit, the same launch also stores every window's hit levels there; positions:
        beside it one tensor of positions_words(...) per job (ac_window_positions_jobs_submit)."""
        ptr = ctypes.cast(ctypes.c_void_p(d_counts.data_ptr()), ctypes.POINTER(ctypes.c_uint32))
        if hits is None and positions is None:
            st = self._L.ac_error_count_jobs_submit(self._h, int(k), jobs.array, len(jobs.array), ptr,
                                                    ctypes.c_void_p(stream or 0))
            if st:
                check(st, self._h)
            return
        if not hasattr(self._L, "ac_window_hits_jobs_submit"):
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "this build of the library has no ac_window_hits_jobs_submit")
        if hits is None:
            raise ValueError("positions come with the hits: pass hits too")
        dev = lambda ts: (_lib.p32 * len(jobs.array))(*[  # noqa: E731
            ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else None), _lib.p32) for t in ts])
        if positions is None:
            st = self._L.ac_window_hits_jobs_submit(self._h, int(k), jobs.array, len(jobs.array), ptr, dev(hits),
                                                    ctypes.c_void_p(stream or 0))
        else:
            st = self._L.ac_window_positions_jobs_submit(self._h, int(k), jobs.array, len(jobs.array), ptr, dev(hits),
                                                         dev(positions), ctypes.c_void_p(stream or 0))
        if st:
            check(st, self._h)

    def window_hits_jobs(self, k: int, jobs, positions: bool = False) -> list:
        """ac_window_hits_jobs: count_jobs -- the whole stage from Dna5 host buffers, `jobs` a Jobs object or a
        sequence of (kmers, Dna5Sample / windows); pinned Dna5Samples are packed by the kernel -- whose one
        launch also writes every window's hit levels; returns one WindowHits per job, row w = the job's window
        w.  Only where the bit-sliced kernel counts (k = 16 or 18..32, every job with work holding equal
        windows of 1..256 bases, a single-device context), at the context's edit budget; anything else raises
        (AC_ERR_INVALID).  positions: ac_window_positions_jobs -- every WindowHits also holds the match end
        positions (.end_positions(), .position_profile()).  There is no `spans` here: match spans are not built
        for the jobs stage, whose image keeps N in inline records the span pass does not decode -- use
        window_hits(..., spans=True)."""
        if not hasattr(self._L, "ac_window_hits_jobs"):
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "this build of the library has no ac_window_hits_jobs")
        if not isinstance(jobs, Jobs):
            jobs = Jobs([(km, w if isinstance(w, Dna5Sample) else Dna5Sample.from_windows(w)) for km, w in jobs])
        E = self.max_errors
        shapes = [(int(km.size), smp.n_windows, int(smp.length[0]) if smp.n_windows else 0)
                  for km, smp in zip(jobs.kmers, jobs.samples)]
        # (all ones: the call writes every word, so one it missed would show as a row of hits, not pass as none)
        mats = [np.full(max(hits_words(nk, nw, E), 1), 0xFFFFFFFF, dtype=np.uint32) for nk, nw, _ in shapes]
        # (a job without work has no matrix: NULL)
        host = lambda ms: (_lib.p32 * len(ms))(*[  # noqa: E731
            _ptr(m, ctypes.c_uint32) if nk and nw else None for m, (nk, nw, _) in zip(ms, shapes)])
        hp = host(mats)
        if positions:
            planes = [np.full(max(positions_words(nk, nw), 1), 0xFFFFFFFF, dtype=np.uint32) for nk, nw, _ in shapes]
            pp = host(planes)
            check(self._L.ac_window_positions_jobs(self._h, int(k), jobs.array, len(jobs.array), hp, pp), self._h)
            return [WindowHits(c, m[: hits_words(nk, nw, E)].reshape(E + 1, nw, (nk + 31) // 32), nk,
                               p[: positions_words(nk, nw)].reshape(8, nw, (nk + 31) // 32), L, self)
                    for c, m, p, (nk, nw, L) in zip(jobs.results(), mats, planes, shapes)]
        check(self._L.ac_window_hits_jobs(self._h, int(k), jobs.array, len(jobs.array), hp), self._h)
        return [WindowHits(c, m[: hits_words(nk, nw, E)].reshape(E + 1, nw, (nk + 31) // 32), nk, counter=self)
                for c, m, (nk, nw, _) in zip(jobs.results(), mats, shapes)]

    def _sample_jobs(self, fn, k, parts):
        keep, arr = [], []
        for km, ws in parts:
            km = np.ascontiguousarray(np.asarray(km, dtype=np.uint64))
            c = np.zeros(max(km.size, 1), dtype=np.uint64)
            keep.append((km, c))
            arr.append(ACSampleJob(_ptr(km if km.size else np.zeros(1, np.uint64), ctypes.c_uint64), int(km.size), ws,
                                   _ptr(c, ctypes.c_uint64)))
        a = (ACSampleJob * len(arr))(*arr)
        check(fn(self._h, int(k), a, len(arr)), self._h)
        return [c[: km.size] for km, c in keep]

    def count_images(self, k: int, parts) -> list:
        """ac_error_count_images: host images [(kmers, PackedSample), ...] (up to 4 jobs) in one
        fused launch per device (sharded over the devices of an n_gpus context)."""
        return self._sample_jobs(self._L.ac_error_count_images, k, [(km, smp.as_struct()) for km, smp in parts])

    def upload_sample(self, sample: PackedSample, slot: int = 0) -> ACWindows:
        """ac_sample_upload_slot: the device copy of a host image (valid until the slot's next upload)."""
        dev = ACWindows()
        hw = sample.as_struct()
        check(self._L.ac_sample_upload_slot(self._h, int(slot), ctypes.byref(hw), ctypes.byref(dev)), self._h)
        return dev

    def count_samples(self, k: int, parts) -> list:
        """ac_error_count_samples: [(kmers, device sample from upload_sample), ...], one fused launch."""
        return self._sample_jobs(self._L.ac_error_count_samples, k, parts)

    def window_hits(self, k: int, parts, positions: bool = False, spans: bool = False, flanks: int = 0,
                    edits: bool = False) -> list:
        """ac_window_hits_samples: [(kmers, PackedSample), ...] (up to 4 parts, e.g. both read ends) are
        uploaded into the context's sample slots and counted in one fused launch that also writes every
        window's hit levels; returns one WindowHits per part.  Only where the bit-sliced kernel counts
        (k = 16 or 18..32, equal windows of 1..256 bases, a single-device context), at the context's
        edit budget; anything else raises (AC_ERR_INVALID).  positions: ac_window_positions_samples -- every
        WindowHits also holds the match end positions (.end_positions(), .position_profile()).  spans (implies
        positions): ac_window_spans_samples -- and the match starts (.start_positions(), .span_lengths(),
        .length_profile(), .start_profile()).  flanks = D in 1..32 (implies spans): ac_window_flanks_samples --
        and the flank profile of D bases (.flank_profile()).  edits (implies spans; with or without flanks):
        ac_window_edits_samples -- and the edit profile (.edit_profile())."""
        if not hasattr(self._L, "ac_window_hits_samples"):
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "this build of the library has no ac_window_hits_samples")
        if positions or spans or flanks or edits:
            return self._window_positions(k, parts, spans or bool(flanks) or bool(edits), int(flanks), bool(edits))
        E = self.max_errors
        keep, arr, mats = [], [], []
        for slot, (km, smp) in enumerate(parts):
            km = np.ascontiguousarray(np.asarray(km, dtype=np.uint64))
            c = np.zeros(max(km.size, 1), dtype=np.uint64)
            # (all ones: the call writes every word, so one it missed would show as a row of hits, not pass as none)
            m = np.full(max(hits_words(km.size, smp.n_windows, E), 1), 0xFFFFFFFF, dtype=np.uint32)
            keep.append((km, c, smp.n_windows))
            mats.append(m)
            arr.append(ACSampleJob(_ptr(km if km.size else np.zeros(1, np.uint64), ctypes.c_uint64), int(km.size),
                                   self.upload_sample(smp, slot), _ptr(c, ctypes.c_uint64)))
        a = (ACSampleJob * len(arr))(*arr)
        hp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in mats])
        check(self._L.ac_window_hits_samples(self._h, int(k), a, len(arr), hp), self._h)
        return [WindowHits(c[: km.size], m[: hits_words(km.size, nw, E)].reshape(E + 1, nw, (km.size + 31) // 32), km.size,
                           counter=self)
                for (km, c, nw), m in zip(keep, mats)]

    def _window_positions(self, k: int, parts, spans: bool = False, flanks: int = 0, edits: bool = False) -> list:
        name = "ac_window_edits_samples" if edits else "ac_window_flanks_samples" if flanks else "ac_window_spans_samples" if spans else "ac_window_positions_samples"
        if not hasattr(self._L, name):
            raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, f"this build of the library has no {name}")
        E = self.max_errors
        keep, arr, mats, planes, starts, profs, eds = [], [], [], [], [], [], []
        for slot, (km, smp) in enumerate(parts):
            km = np.ascontiguousarray(np.asarray(km, dtype=np.uint64))
            c = np.zeros(max(km.size, 1), dtype=np.uint64)
            mats.append(np.full(max(hits_words(km.size, smp.n_windows, E), 1), 0xFFFFFFFF, dtype=np.uint32))
            planes.append(np.full(max(positions_words(km.size, smp.n_windows), 1), 0xFFFFFFFF, dtype=np.uint32))
            starts.append(np.full(max(positions_words(km.size, smp.n_windows), 1), 0xFFFFFFFF, dtype=np.uint32))
            profs.append(np.full(max(flank_words(km.size, flanks), 1), 0xFFFFFFFF, dtype=np.uint32))
            eds.append(np.full(max(edit_words(km.size, k), 1) if edits else 1, 0xFFFFFFFF, dtype=np.uint32))
            keep.append((km, c, smp.n_windows, int(smp.length[0]) if smp.n_windows else 0))
            arr.append(ACSampleJob(_ptr(km if km.size else np.zeros(1, np.uint64), ctypes.c_uint64), int(km.size),
                                   self.upload_sample(smp, slot), _ptr(c, ctypes.c_uint64)))
        a = (ACSampleJob * len(arr))(*arr)
        hp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in mats])
        pp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in planes])
        if edits:
            sp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in starts])
            fp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in profs]) if flanks else None
            ep = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in eds])
            check(self._L.ac_window_edits_samples(self._h, int(k), a, len(arr), int(flanks), hp, pp, sp, fp, ep), self._h)
        elif flanks:
            sp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in starts])
            fp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in profs])
            check(self._L.ac_window_flanks_samples(self._h, int(k), a, len(arr), int(flanks), hp, pp, sp, fp), self._h)
        elif spans:
            sp = (_lib.p32 * len(arr))(*[_ptr(m, ctypes.c_uint32) for m in starts])
            check(self._L.ac_window_spans_samples(self._h, int(k), a, len(arr), hp, pp, sp), self._h)
        else:
            check(self._L.ac_window_positions_samples(self._h, int(k), a, len(arr), hp, pp), self._h)
        shape = lambda m, km, nw: m[: positions_words(km.size, nw)].reshape(8, nw, (km.size + 31) // 32)  # noqa: E731
        # (a job without windows has no work: the call leaves its profile alone, and it is all zeros)
        prof = lambda f, km, nw: (f[: flank_words(km.size, flanks)] if nw else  # noqa: E731
                                  np.zeros(flank_words(km.size, flanks), np.uint32)).reshape(2, km.size, flanks, 5)
        edit = lambda e, km, nw: (e[: edit_words(km.size, k)] if nw else  # noqa: E731
                                  np.zeros(edit_words(km.size, k), np.uint32)).reshape(km.size, int(k), 12)
        return [WindowHits(c[: km.size], m[: hits_words(km.size, nw, E)].reshape(E + 1, nw, (km.size + 31) // 32), km.size,
                           shape(p, km, nw), L, self, shape(t, km, nw) if spans else None, int(k),
                           prof(f, km, nw) if flanks else None, edit(e, km, nw) if edits else None)
                for (km, c, nw, L), m, p, t, f, e in zip(keep, mats, planes, starts, profs, eds)]

    def hit_start_positions(self, k: int, kmers, n_kmers: int, sample, window_len: int, hits, pos, levels: int,
                            out=None, stream=None):
        """ac_hit_start_positions_device: the span pass alone over resident tensors -- `kmers` the device
        k-mers (int64 / uint64 words), `sample` an ACWindows of device pointers (or a DeviceSegment) holding
        equal windows of window_len bases, `hits` a device hit matrix of `levels` planes, `pos` its position
        matrix.  Returns an int32 device tensor (8, n_windows, ceil(n_kmers / 32)), the start matrix (`out`,
        when given, is written instead; asynchronous)."""
        import torch

        ws = sample.as_struct() if hasattr(sample, "as_struct") else sample
        ws = ws.sample if isinstance(ws, ACSegment) else ws
        words = (int(n_kmers) + 31) // 32
        if out is None:
            out = torch.empty(max(positions_words(n_kmers, ws.n_windows), 1), dtype=torch.int32, device=hits.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)  # noqa: E731
        kp = ctypes.cast(ctypes.c_void_p(kmers.data_ptr() if kmers is not None else 0), ctypes.POINTER(ctypes.c_uint64))
        check(self._L.ac_hit_start_positions_device(self._h, int(k), kp, int(n_kmers), ctypes.byref(ws), int(window_len),
                                                    p(hits), p(pos), int(levels), p(out), ctypes.c_void_p(stream or 0)),
              self._h)
        return out[: positions_words(n_kmers, ws.n_windows)].view(8, int(ws.n_windows), words)

    def hit_flank_profile(self, sample, window_len: int, hit_plane, pos, start, n_kmers: int, n_windows: int, depth: int,
                          out=None, stream=None):
        """ac_hit_flank_profile_device: the flank pass alone over resident tensors -- `sample` an ACWindows of
        device pointers (or a DeviceSegment) holding n_windows equal windows of window_len bases, `hit_plane`
        one level plane of a device hit matrix (int32, n_windows x ceil(n_kmers / 32)), `pos` its position
        matrix, `start` its start matrix or None (the left half is then zeros).  Returns an int32 device
        tensor (2, n_kmers, depth, 5) (`out`, when given, is written instead; asynchronous)."""
        import torch

        ws = sample.as_struct() if hasattr(sample, "as_struct") else sample
        ws = ws.sample if isinstance(ws, ACSegment) else ws
        if int(n_windows) != int(ws.n_windows):
            ws = ACWindows.from_buffer_copy(ws)  # (the first n_windows windows of the image)
            ws.n_windows = int(n_windows)
        n = flank_words(n_kmers, depth)
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int32, device=pos.device if pos is not None else "cuda")
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_flank_profile_device(self._h, ctypes.byref(ws), int(window_len), p(hit_plane), p(pos), p(start),
                                                  int(n_kmers), int(depth), p(out), ctypes.c_void_p(stream or 0)), self._h)
        return out[:n].view(2, int(n_kmers), int(depth), 5)

    def hit_edit_profile(self, k: int, kmers, n_kmers: int, sample, window_len: int, hit_plane, pos, start, n_windows: int,
                         out=None, stream=None):
        """ac_hit_edit_profile_device: the edit pass alone over resident tensors -- `kmers` a device pointer to
        n_kmers k-mers (an int: a DeviceSegment's .kmers; or an int64 device tensor), `sample` an ACWindows of
        device pointers (or a DeviceSegment) holding n_windows equal windows of window_len bases, `hit_plane`
        one level plane of a device hit matrix (int32, n_windows x ceil(n_kmers / 32)), `pos` its position
        matrix, `start` its start matrix.  Returns an int32 device tensor (n_kmers, k, 12) (`out`, when given,
        is written instead; asynchronous)."""
        import torch

        ws = sample.as_struct() if hasattr(sample, "as_struct") else sample
        ws = ws.sample if isinstance(ws, ACSegment) else ws
        if int(n_windows) != int(ws.n_windows):
            ws = ACWindows.from_buffer_copy(ws)  # (the first n_windows windows of the image)
            ws.n_windows = int(n_windows)
        n = edit_words(n_kmers, k)
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int32, device=pos.device if pos is not None else "cuda")
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)  # noqa: E731
        kp = kmers.data_ptr() if hasattr(kmers, "data_ptr") else (kmers or 0)
        check(self._L.ac_hit_edit_profile_device(self._h, int(k), ctypes.cast(ctypes.c_void_p(kp), ctypes.POINTER(ctypes.c_uint64)),
                                                 int(n_kmers), ctypes.byref(ws), int(window_len), p(hit_plane), p(pos), p(start),
                                                 p(out), ctypes.c_void_p(stream or 0)), self._h)
        return out[:n].view(int(n_kmers), int(k), 12)

    def hit_position_profile(self, hits, pos, n_kmers: int, n_windows: int, levels: int, window_len: int, stream=None):
        """ac_hit_position_profile_device over a device hit matrix (`levels` planes) and its position
        matrix (8 planes), torch tensors: returns an int32 device tensor (levels, n_kmers, window_len), the
        windows at distance exactly d whose best occurrence ends at base p + 1 (asynchronous)."""
        import torch

        out = torch.empty((int(levels), max(int(n_kmers), 1), int(window_len)), dtype=torch.int32, device=hits.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_position_profile_device(self._h, p(hits), p(pos), int(n_kmers), int(n_windows), int(levels),
                                                     int(window_len), p(out), ctypes.c_void_p(stream or 0)), self._h)
        return out[:, : int(n_kmers)]

    def hit_level_counts(self, hits, n_kmers: int, n_windows: int, levels: int, stream=None):
        """ac_hit_level_counts_device over a device hit matrix (a torch tensor of `levels` planes): returns
        an int32 device tensor (levels, n_kmers), the windows within e edits of every k-mer (asynchronous)."""
        import torch

        out = torch.empty((int(levels), max(int(n_kmers), 1)), dtype=torch.int32, device=hits.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_level_counts_device(self._h, p(hits), int(n_kmers), int(n_windows), int(levels), p(out),
                                                 ctypes.c_void_p(stream or 0)), self._h)
        return out[:, : int(n_kmers)]

    def hit_cooccurrence(self, hits, n_kmers: int, n_windows: int, levels: int, stream=None):
        """ac_hit_cooccurrence_device over a device hit matrix (a torch tensor of `levels` planes; a view at
        plane e's offset with levels = 1 reduces that plane alone): returns an int32 device tensor
        (levels, n_kmers, n_kmers), entry (e, a, b) = the windows of plane e that hold k-mers a and b both
        (asynchronous)."""
        import torch

        n = int(n_kmers)
        out = torch.empty((int(levels), n, n), dtype=torch.int32, device=hits.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_cooccurrence_device(self._h, p(hits), n, int(n_windows), int(levels), p(out),
                                                 ctypes.c_void_p(stream or 0)), self._h)
        return out

    def hit_cross_cooccurrence(self, hits_a, n_a: int, hits_b, n_b: int, n_windows: int, levels: int, stream=None):
        """ac_hit_cross_cooccurrence_device over two device hit matrices of the same n_windows (torch tensors of
        `levels` planes each; views at two planes' offsets with levels = 1 pair those planes): returns an int32
        device tensor (levels, n_a, n_b), entry (e, a, b) = the windows of plane e that hold k-mer a of the
        first matrix and k-mer b of the second (asynchronous)."""
        import torch

        na, nb = int(n_a), int(n_b)
        out = torch.empty((int(levels), na, nb), dtype=torch.int32, device=hits_a.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_cross_cooccurrence_device(self._h, p(hits_a), na, p(hits_b), nb, int(n_windows), int(levels),
                                                       p(out), ctypes.c_void_p(stream or 0)), self._h)
        return out

    def hit_window_counts(self, hits, n_kmers: int, n_windows: int, levels: int, stream=None):
        """ac_hit_window_counts_device over a device hit matrix: returns an int32 device tensor
        (levels, n_windows), how many of the k-mers every window holds (asynchronous)."""
        import torch

        out = (torch.empty if int(n_kmers) else torch.zeros)((int(levels), int(n_windows)), dtype=torch.int32, device=hits.device)
        p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        check(self._L.ac_hit_window_counts_device(self._h, p(hits), int(n_kmers), int(n_windows), int(levels), p(out),
                                                  ctypes.c_void_p(stream or 0)), self._h)
        return out

    def cooccurrence_host(self, hits, n_kmers: int, n_windows: int, levels: int) -> np.ndarray:
        """ac_hit_cooccurrence: a host hit matrix (uint32, `levels` planes) in, uint32 (levels, n_kmers,
        n_kmers) out; synchronous (the command line's route)."""
        m = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1)
        n = int(n_kmers)
        if m.size < hits_words(n, n_windows, int(levels) - 1):
            raise ValueError("hit matrix smaller than (levels, n_windows, ceil(n_kmers / 32))")
        out = np.full(max(cooccurrence_words(n, levels), 1), 0xFFFFFFFF, dtype=np.uint32)
        check(self._L.ac_hit_cooccurrence(self._h, _ptr(m if m.size else np.zeros(1, np.uint32), ctypes.c_uint32), n,
                                          int(n_windows), int(levels), _ptr(out, ctypes.c_uint32)), self._h)
        return out[: cooccurrence_words(n, levels)].reshape(int(levels), n, n)

    def cross_cooccurrence_host(self, hits_a, n_a: int, hits_b, n_b: int, n_windows: int, levels: int) -> np.ndarray:
        """ac_hit_cross_cooccurrence: two host hit matrices (uint32, `levels` planes each, the same n_windows)
        in, uint32 (levels, n_a, n_b) out; synchronous (the command line's route)."""
        a = np.ascontiguousarray(hits_a, dtype=np.uint32).reshape(-1)
        b = np.ascontiguousarray(hits_b, dtype=np.uint32).reshape(-1)
        na, nb = int(n_a), int(n_b)
        if a.size < hits_words(na, n_windows, int(levels) - 1) or b.size < hits_words(nb, n_windows, int(levels) - 1):
            raise ValueError("hit matrix smaller than (levels, n_windows, ceil(n / 32))")
        words = cross_cooccurrence_words(na, nb, levels)
        out = np.full(max(words, 1), 0xFFFFFFFF, dtype=np.uint32)
        one = np.zeros(1, np.uint32)
        check(self._L.ac_hit_cross_cooccurrence(self._h, _ptr(a if a.size else one, ctypes.c_uint32), na,
                                                _ptr(b if b.size else one, ctypes.c_uint32), nb, int(n_windows),
                                                int(levels), _ptr(out, ctypes.c_uint32)), self._h)
        return out[:words].reshape(int(levels), na, nb)

    def exact_path(self) -> int:
        """ac_exact_path: 1 partitioned, 0 hash table, -1 no exact count yet."""
        return int(self._L.ac_exact_path(self._h))

    def stage_mode(self) -> int:
        """ac_stage_mode: the last jobs call's stage -- 2 early launch (the count kernel copies each
        job in as the host flags it), 0 copy kernel / copy engine ahead of the launch, -1 no call yet."""
        return int(self._L.ac_stage_mode(self._h))

    # ---- multi-process data parallelism: the count all-reduce over RCCL (ac_comm_*) ----
    def comm_unique_id(self) -> bytes:
        """ac_comm_unique_id: a fresh RCCL unique id (rank 0 sends it to every rank)."""
        buf = ctypes.create_string_buffer(self._L.ac_comm_id_bytes())
        check(self._L.ac_comm_unique_id(self._h, buf), self._h)
        return buf.raw

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes) -> None:
        """ac_comm_init: join the n_ranks-rank RCCL communicator as `rank`."""
        buf = ctypes.create_string_buffer(bytes(unique_id), self._L.ac_comm_id_bytes())
        check(self._L.ac_comm_init(self._h, int(n_ranks), int(rank), buf), self._h)

    def allreduce_counts(self, d_counts, stream=None) -> None:
        """ac_allreduce_counts: in-place uint32 sum of a device count tensor over the ranks."""
        check(self._L.ac_allreduce_counts(self._h, ctypes.c_void_p(d_counts.data_ptr()),
                                          ctypes.c_uint64(d_counts.numel()), ctypes.c_void_p(stream or 0)),
              self._h)

    def check(self, stream=None) -> None:
        """ac_check: raise if a device launch since the last check skipped a malformed window."""
        check(self._L.ac_check(self._h, ctypes.c_void_p(stream or 0)), self._h)

    def exact_count(self, k: int, sample: PackedSample, lc_threshold: float, forbidden=(), limit: int = 500,
                    solid: int = 0):
        """ac_exact_count: count_kmers (approx_counter.cpp:487-519) + get_most_frequent /
        get_solid_kmers on the GPU.  Returns ([(kmer, count), ...] in CompareCount order,
        n_distinct, had_n)."""
        fb = np.ascontiguousarray(np.asarray(list(forbidden) or [0], dtype=np.uint64))
        cap = max(1, int(limit) if not solid else 1024)
        ws = sample.as_struct()
        while True:
            km = np.zeros(cap, np.uint64)
            ct = np.zeros(cap, np.uint64)
            n_out, n_dist, had_n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            st = self._L.ac_exact_count(self._h, int(k), ctypes.byref(ws), float(lc_threshold),
                                        _ptr(fb, ctypes.c_uint64), len(forbidden), int(limit), int(solid),
                                        _ptr(km, ctypes.c_uint64), _ptr(ct, ctypes.c_uint64), cap,
                                        ctypes.byref(n_out), ctypes.byref(n_dist), ctypes.byref(had_n))
            if st == _lib.AC_ERR_INVALID and n_out.value > cap:
                cap = int(n_out.value)
                continue
            check(st, self._h)
            n = int(n_out.value)
            return [(int(a), int(b)) for a, b in zip(km[:n], ct[:n])], int(n_dist.value), int(had_n.value)

    @staticmethod
    def segment_array(segments):
        """The ac_segment array of DeviceSegment objects, built once and reusable with
        count_device (saves the per-call ctypes marshalling in launch loops)."""
        return (ACSegment * len(segments))(*[s.as_struct() for s in segments])

    def count_device(self, k: int, segments, stream=None, accumulate: bool = False, window_len=None, hits=None,
                     positions=None, spans=None) -> None:
        """ac_error_count_device over DeviceSegment objects, or an array from
        segment_array (asynchronous).  window_len (one per segment): the samples'
        windows all have that length and sit back to back at ceil32 strides
        (start / length are not read).  accumulate: AC_DEVICE_ACCUMULATE.
        hits (one device tensor per segment, hits_words(...) int32 / uint32 words each; None for a segment
        without work): ac_window_hits_device -- the same launch also writes the windows' hit levels
        (window_len required, no accumulate).  positions (with hits; one device tensor per segment,
        positions_words(...) words each): ac_window_positions_device -- and the match end positions.  spans (with
        positions; one device tensor per segment, positions_words(...) words each): the span pass
        (ac_hit_start_positions_device) is enqueued on the same stream after the launch, per segment with
        work, and fills the match starts."""
        if spans is not None and (hits is None or positions is None):
            raise ValueError("spans come with hits and positions")
        arr = segments if isinstance(segments, ctypes.Array) else self.segment_array(segments)
        wp = None
        if window_len is not None:
            wl = np.ascontiguousarray(window_len, dtype=np.uint32)
            if wl.size != len(arr):
                raise ValueError("one window_len per segment")
            wp = _ptr(wl, ctypes.c_uint32)
        if hits is not None:
            if accumulate:
                raise _lib.ApproxCounterError(_lib.AC_ERR_INVALID, "window hits: accumulate mode is refused")
            if len(hits) != len(arr):
                raise ValueError("one hits tensor per segment")
            hp = (_lib.p32 * len(arr))(*[ctypes.cast(ctypes.c_void_p(h.data_ptr() if h is not None else 0), _lib.p32)
                                         for h in hits])
            if positions is not None:
                if len(positions) != len(arr):
                    raise ValueError("one positions tensor per segment")
                pp = (_lib.p32 * len(arr))(*[ctypes.cast(ctypes.c_void_p(h.data_ptr() if h is not None else 0), _lib.p32)
                                             for h in positions])
                st = self._L.ac_window_positions_device(self._h, int(k), arr, len(arr), wp, hp, pp,
                                                        ctypes.c_void_p(stream or 0))
            else:
                st = self._L.ac_window_hits_device(self._h, int(k), arr, len(arr), wp, hp, ctypes.c_void_p(stream or 0))
        elif positions is not None:
            raise ValueError("positions come with hits")
        else:
            st = self._L.ac_error_count_device(self._h, int(k), arr, len(arr), wp, 1 if accumulate else 0,
                                               ctypes.c_void_p(stream or 0))
        if st:
            check(st, self._h)
        if spans is not None:
            if len(spans) != len(arr):
                raise ValueError("one spans tensor per segment")
            if window_len is None:
                raise ValueError("spans need window_len")
            for seg, L, h, p, t in zip(arr, wl, hits, positions, spans):
                if seg.n_kmers and seg.sample.n_windows:
                    st = self._L.ac_hit_start_positions_device(
                        self._h, int(k), seg.kmers, seg.n_kmers, ctypes.byref(seg.sample), int(L),
                        *[ctypes.cast(ctypes.c_void_p(x.data_ptr() if x is not None else 0), _lib.p32) for x in (h, p)],
                        self.max_errors + 1, ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32),
                        ctypes.c_void_p(stream or 0))
                    if st:
                        check(st, self._h)

    def last_launch(self):
        w, wpw, g = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self._L.ac_last_launch(self._h, ctypes.byref(w), ctypes.byref(wpw), ctypes.byref(g)), self._h)
        return {"waves": w.value, "windows_per_wave": wpw.value, "groups": g.value}


class DeviceSegment:
    """A segment whose arrays live in device memory (torch tensors on cuda)."""

    def __init__(self, kmers, codes, nmask, start, length, counts, n_bases: int):
        self.kmers, self.codes, self.nmask = kmers, codes, nmask
        self.start, self.length, self.counts = start, length, counts
        self.n_bases = int(n_bases)

    @classmethod
    def upload(cls, kmers, sample: PackedSample, device="cuda"):
        import torch

        def t(a):
            # uint64 / uint32 views through int64 / int32 tensors (same bytes)
            a = np.ascontiguousarray(a)
            view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype]
            return torch.from_numpy(a.view(view) if a.size else np.zeros(1, view)).to(device)

        km = np.asarray(kmers, dtype=np.uint64)
        counts = torch.zeros(max(km.size, 1), dtype=torch.int32, device=device)
        seg = cls(t(km), t(sample.codes), t(sample.nmask), t(sample.start), t(sample.length),
                  counts, sample.n_bases)
        seg.n_kmers = int(km.size)
        seg.n_windows = sample.n_windows
        return seg

    def as_struct(self) -> ACSegment:
        def p(tensor, typ):
            return ctypes.cast(ctypes.c_void_p(tensor.data_ptr()), ctypes.POINTER(typ))

        ws = ACWindows(p(self.codes, ctypes.c_uint32), p(self.nmask, ctypes.c_uint32),
                       p(self.start, ctypes.c_uint64), p(self.length, ctypes.c_uint32),
                       self.n_windows, self.n_bases)
        return ACSegment(p(self.kmers, ctypes.c_uint64), self.n_kmers, ws,
                         p(self.counts, ctypes.c_uint32))

    def counts_numpy(self) -> np.ndarray:
        return self.counts[: self.n_kmers].cpu().numpy().view(np.uint32).astype(np.uint64)


def plan_host_cpus(rank_cpulists, rank: int, allowed: str, core_of=None) -> list:
    """ac_plan_host_cpus: the host-pool CPUs of local rank `rank`, given every local
    rank's GPU cpulist (sysfs text such as "0-63,128-191"), the CPUs the process may
    use and optionally each CPU's physical core (index = CPU)."""
    L = _lib.load()
    arr = (ctypes.c_char_p * len(rank_cpulists))(*[s.encode() for s in rank_cpulists])
    core = None
    if core_of is not None:
        core = np.ascontiguousarray(np.asarray(core_of, dtype=np.int32))
    cap = 4096
    out = np.zeros(cap, np.int32)
    n = L.ac_plan_host_cpus(arr, len(rank_cpulists), int(rank), allowed.encode(),
                            _ptr(core, ctypes.c_int) if core is not None else None,
                            int(core.size) if core is not None else 0, _ptr(out, ctypes.c_int), cap)
    if n < 0:
        raise ValueError("ac_plan_host_cpus: bad arguments")
    return [int(c) for c in out[: min(n, cap)]]


def host_pool_cpus():
    """ac_host_pool_cpus: (participants, [CPUs]) of the host pool plan in force."""
    L = _lib.load()
    part = ctypes.c_int()
    out = np.zeros(4096, np.int32)
    n = L.ac_host_pool_cpus(ctypes.byref(part), _ptr(out, ctypes.c_int), out.size)
    return int(part.value), [int(c) for c in out[: min(n, out.size)]]


_default_counter = None


def _counter() -> ApproxCounter:
    global _default_counter
    if _default_counter is None:
        _default_counter = ApproxCounter()
    return _default_counter


def error_count(sequences, exact_count, nb_thread: int = 4, k: int = 16, v: int = 0, max_errors: int = 2) -> dict:
    """errorCount (approx_counter.cpp:531-601): {kmer: approximate count}.  max_errors (an extension:
    the reference counts at 2): the edit budget of this call, see ApproxCounter.set_max_errors."""
    del nb_thread, v  # OpenMP thread count / verbosity of the CPU reference
    kmers = [int(km) for km, _ in exact_count]
    if not kmers:
        return {}
    ctr = _counter()
    if ctr.max_errors != max_errors:
        ctr.set_max_errors(max_errors)
    # the sample as a StringSet<Dna5String>: packed, sent and counted by ac_error_count_jobs
    counts = ctr.count_jobs(k, [(np.array(kmers, dtype=np.uint64), Dna5Sample.from_windows(sequences))])[0]
    return {km: int(c) for km, c in zip(kmers, counts)}


def error_levels(sequences, exact_count, nb_thread: int = 4, k: int = 16, v: int = 0, max_errors: int = 2) -> dict:
    """errorCount's bitfields (approx_counter.cpp:553-565), which the reference sums away: {kmer: (n_0, .., n_E)},
    n_e = the sequences that hold the k-mer within e edits, E = max_errors.  sum(levels) is error_count's value.
    Through ApproxCounter.window_hits_jobs, so only where that runs: k = 16 or 18..32, sequences of one length
    of 1..256 bases."""
    del nb_thread, v  # OpenMP thread count / verbosity of the CPU reference
    kmers = [int(km) for km, _ in exact_count]
    if not kmers:
        return {}
    ctr = _counter()
    if ctr.max_errors != max_errors:
        ctr.set_max_errors(max_errors)
    wh = ctr.window_hits_jobs(k, [(np.array(kmers, dtype=np.uint64), Dna5Sample.from_windows(sequences))])[0]
    lv = wh.level_counts()
    return {km: tuple(int(x) for x in lv[:, i]) for i, km in enumerate(kmers)}
