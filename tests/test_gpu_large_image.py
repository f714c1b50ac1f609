"""GPU tests of window images up to the size bound the ABI accepts (AC_MAX_IMAGE_BASES = 2^34 - 4096 bases:
4 GiB of code words less 1 KiB), whose base indices pass 2^32 and whose code-byte offsets pass 2^31 -- the
sign bit of the 32-bit size every buffer descriptor of the count kernels is made with.  The shapes are large
because the edge is an address, not a length: nothing smaller reaches it.  The work is small the other way:
32 candidates (one candidate group), 64 where a second word column matters.

The images are built on the device (tests/large_cases.py; tests/test_large_cases.py shows on the CPU that
every case has the property relied on here).  Dense images hold dictionary texts, marker texts at every
boundary window; counts are compared with bincount(idx) @ per_text, hit / position / start matrices plane by
plane with the per-text rows of the CPU references expanded by idx, flank and edit profiles with the per-text
profiles summed through bincount(idx).  The sparse image holds a few dozen ragged
windows around the boundaries; counts are the oracle's.  Every launch asserts which count kernel ran.

Sizes ascend within the file, so the smallest failing size is the one reported.  The module's peak device
memory (torch.cuda.max_memory_allocated) is asserted below 32 GiB by the last test; a test skips only when
the device has less than that free."""
import gc

import numpy as np
import pytest

import approx_counter_amd as ac
from tests import large_cases as lc
from tests.test_gpu_bitslice import BITSLICE, WORD, kernel_of

pytestmark = pytest.mark.gpu
GIB = 1 << 30
PEAK_LIMIT = 32 * GIB
BS_ON = BITSLICE == 1
TOP = lc.TOP_BASES
SIZES = ((1 << 32) + (1 << 20), (1 << 33) + (1 << 20), TOP)


@pytest.fixture(scope="module")
def ctx():
    """One context for the module; the tensors of every test are freed as it ends."""
    import torch

    c = ac.ApproxCounter(0)
    torch.cuda.reset_peak_memory_stats()  # (the peak asserted by the last test is this module's)
    yield c
    c.close()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def room():
    import torch

    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < PEAK_LIMIT:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free, the large-image tests need {PEAK_LIMIT // GIB}")
    yield
    gc.collect()
    torch.cuda.empty_cache()


def device():
    import torch

    return torch.device("cuda")


def segment(km, codes, nmask, n_windows, n_bases, start=None, length=None):
    """A DeviceSegment over an image built on the device; equal windows carry no descriptors."""
    import torch

    dev = codes.device
    km = np.ascontiguousarray(km, dtype=np.uint64)
    start = torch.zeros(1, dtype=torch.int64, device=dev) if start is None else start
    length = torch.zeros(1, dtype=torch.int32, device=dev) if length is None else length
    seg = ac.DeviceSegment(torch.from_numpy(km.view(np.int64)).to(dev), codes, nmask, start, length,
                           torch.zeros(max(km.size, 1), dtype=torch.int32, device=dev), n_bases)
    seg.n_kmers, seg.n_windows = int(km.size), int(n_windows)
    return seg


def dense(k, n_kmers, L, n_bases, seed=3):
    """(segment, idx, per_text) of the dense image of n_bases over the (k, n_kmers, L) dictionary."""
    dev = device()
    km, texts, per, markers = lc.dense_dictionary(k, n_kmers, L)
    nw = lc.windows_in(n_bases, L)
    marks = lc.boundary_windows(nw, lc.slot(L))
    idx, _ = lc.dense_index(nw, len(texts), seed, marks, markers, dev)
    codes, nmask = lc.dense_image(*lc.text_tables(texts), idx, n_bases, dev)
    return segment(km, codes, nmask, nw, n_bases), idx, per


def same_counts(what, seg, want):
    got = seg.counts_numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], (want[bad[:8]] - got[bad[:8]]).astype(np.int64))


def count_and_accumulate(ctx, k, seg, L, want, kernel, what):
    """The counts of one launch, then of a second one in accumulate mode: want and twice want."""
    import torch

    wl = None if L is None else [L]
    ctx.count_device(k, [seg], window_len=wl)
    torch.cuda.synchronize()
    assert kernel_of(ctx) == kernel, what
    ctx.check()
    same_counts(what, seg, want)
    ctx.count_device(k, [seg], window_len=wl, accumulate=True)
    torch.cuda.synchronize()
    assert kernel_of(ctx) == kernel, what
    ctx.check()
    same_counts((what, "accumulate"), seg, 2 * want)


# ---- 1: dense, the bit-sliced count kernel ----

@pytest.mark.parametrize("n_bases,L,k", [(n, 100, k) for n in SIZES for k in (16, 22)] +
                         [(TOP, 200, 16), (TOP, 200, 22), (TOP, 256, 16)])
def test_dense_bit_sliced_count(ctx, n_bases, L, k):
    """32 candidates over equal windows of 100 bases (slots of 32 bytes) in images that cross base 2^32, base
    2^33 (code byte 2^31) and reach the bound (134,217,695 windows); at the bound also windows of 200 bases
    (slots of 56 bytes, 76,695,826 windows, the boundaries inside slots) and of 256 (slots of 64 bytes,
    67,108,847 windows).  Under AC_BITSLICE=0 the same launches are the word-parallel kernel's."""
    seg, idx, per = dense(k, 32, L, n_bases)
    count_and_accumulate(ctx, k, seg, L, lc.expected_counts(idx, per), BITSLICE, (n_bases, L, k))


# ---- 2: dense, hits, positions, spans, flank and edit profiles at the bound ----

def hits_launch(ctx, E):
    """The hits-and-positions launch at k = 16, 64 candidates, windows of 100 bases, the largest image, at edit
    budget E: (seg, idx, rows on the device, host rows, hits, positions), or None where AC_BITSLICE=0 refuses it
    (asserted)."""
    import torch

    k, nk, L = 16, 64, 100
    seg, idx, _ = dense(k, nk, L, TOP)
    nw = seg.n_windows
    rows = lc.text_rows(k, nk, L, E)
    dev = device()
    h = torch.full((ac.hits_words(nk, nw, E),), -1, dtype=torch.int32, device=dev)  # (all ones: every word is written)
    p = torch.full((ac.positions_words(nk, nw),), -1, dtype=torch.int32, device=dev)
    ctx.set_max_errors(E)
    try:
        if not BS_ON:
            with pytest.raises(ac.ApproxCounterError) as ei:
                ctx.count_device(k, [seg], window_len=[L], hits=[h], positions=[p])
            assert ei.value.status == 1 and "AC_BITSLICE" in str(ei.value)
            return None
        ctx.count_device(k, [seg], window_len=[L], hits=[h], positions=[p])
        torch.cuda.synchronize()
        assert kernel_of(ctx) == BITSLICE
        ctx.check()
    finally:
        ctx.set_max_errors(2)
    n = lc.text_counts(idx, rows["hit"].shape[1])
    levels = np.einsum("t,etc->ec", n, rows["hit"].astype(np.uint64))
    same_counts(("counts", E), seg, levels.sum(axis=0))
    drows = {name: lc.on(rows[name], dev) for name in ("hits", "pos", "start")}
    return seg, idx, drows, rows, n, levels, h.view(E + 1, nw, 2), p.view(8, nw, 2)


@pytest.mark.parametrize("E", [2, 3])
def test_dense_hits_and_positions(ctx, E):
    """The level planes (E + 1 x 134,217,695 x 2 words) and the eight position planes (8.59 GB: byte offsets past
    2^32, word offsets up to 528 short of 2^31) equal the per-text rows expanded by idx; the three reductions of
    those matrices equal the same rows reduced through bincount(idx)."""
    import torch

    got = hits_launch(ctx, E)
    if got is None:
        return
    seg, idx, drows, rows, n, levels, h, p = got
    nk, nw, L, S = 64, seg.n_windows, 100, 128
    for e in range(E + 1):
        assert (bad := lc.first_mismatch(h[e], drows["hits"][e], idx, S)) is None, f"level {e}: {bad}"
    for b in range(8):
        assert (bad := lc.first_mismatch(p[b], drows["pos"][b], idx, S)) is None, f"position plane {b}: {bad}"
    lv = ctx.hit_level_counts(h, nk, nw, E + 1)
    prof = ctx.hit_position_profile(h, p, nk, nw, E + 1, L)
    torch.cuda.synchronize()
    assert np.array_equal(lv.cpu().numpy().view(np.uint32), levels)
    assert np.array_equal(prof.cpu().numpy().view(np.uint32), np.einsum("t,tecp->ecp", n, rows["prof"]))
    del lv, prof
    wc = ctx.hit_window_counts(h, nk, nw, E + 1)
    torch.cuda.synchronize()
    per_text = lc.on(rows["hit"].sum(axis=2).astype(np.int32), device())  # (E + 1, n_texts)
    for e in range(E + 1):
        bad = lc.first_mismatch(wc[e].view(nw, 1), per_text[e].view(-1, 1), idx, S)
        assert bad is None, f"window counts, level {e}: {bad}"
    ctx.check()


def span_pass(ctx, got):
    """The span pass over hits_launch(ctx, 2)'s matrices; the eight start planes are compared with the per-text
    start rows expanded by idx before anything uses them."""
    import torch

    seg, idx, drows, rows, n, levels, h, p = got
    start = ctx.hit_start_positions(16, seg.kmers, 64, seg, 100, h, p, 3)
    torch.cuda.synchronize()
    ctx.check()
    for b in range(8):
        assert (bad := lc.first_mismatch(start[b], drows["start"][b], idx, 128)) is None, f"start plane {b}: {bad}"
    return start


def test_dense_spans(ctx):
    """The span pass over the same launch's matrices at E = 2: the eight start planes equal the per-text start
    rows expanded by idx."""
    got = hits_launch(ctx, 2)
    if got is None:
        return
    span_pass(ctx, got)


def test_dense_flank_profiles(ctx):
    """The flank pass over the same matrices and the span pass's starts (134,217,695 windows x 2 word columns: a
    window's text lies at up to base 2^34 - 4256, a plane word at up to 2^31 - 528 words into the sixteen position
    and start planes): the top plane at D = 8 and D = 32, once without starts (the left half zeros), once plane 0
    -- each equal to the per-text profiles summed through bincount(idx)."""
    import torch

    got = hits_launch(ctx, 2)
    if got is None:
        return
    seg, idx, drows, rows, n, levels, h, p = got
    start = span_pass(ctx, got)
    nk, nw, L, E = 64, seg.n_windows, 100, 2
    per = lc.text_profiles(16, nk, L, E)["flank"]
    for D, plane, with_start in ((8, E, True), (32, E, True), (8, E, False), (8, 0, True)):
        out = ctx.hit_flank_profile(seg, L, h[plane], p, start if with_start else None, nk, nw, D)
        torch.cuda.synchronize()
        ctx.check()
        prof = out.cpu().numpy().view(np.uint32)
        want = lc.image_profile(n, per[D, plane, with_start])
        assert want.any() and want.max() <= nw < 1 << 32
        bad = lc.first_cell(prof, want, ("side", "k-mer", "column", "symbol"))
        assert bad is None, f"flank profile, D = {D}, plane {plane}, {'with' if with_start else 'no'} starts: {bad}"
        assert with_start or not prof[1].any()
        del out
    ctx.check()


def test_dense_edit_profiles(ctx):
    """The edit pass over the same matrices and starts: the top plane and plane 0 equal the per-text profiles summed
    through bincount(idx), and for every k-mer and base the operations 0..6 (match, five substitutions, deletion)
    sum to the k-mer's pairs in the plane -- every pair of the dictionary meets the pass's conditions."""
    import torch

    got = hits_launch(ctx, 2)
    if got is None:
        return
    seg, idx, drows, rows, n, levels, h, p = got
    start = span_pass(ctx, got)
    nk, nw, L, E, k = 64, seg.n_windows, 100, 2, 16
    per = lc.text_profiles(k, nk, L, E)["edit"]
    for plane in (E, 0):
        out = ctx.hit_edit_profile(k, seg.kmers, nk, seg, L, h[plane], p, start, nw)
        torch.cuda.synchronize()
        ctx.check()
        prof = out.cpu().numpy().view(np.uint32)
        want = lc.image_profile(n, per[plane])
        assert want.any() and want.max() <= nw < 1 << 32
        bad = lc.first_cell(prof, want, ("k-mer", "base", "operation"))
        assert bad is None, f"edit profile, plane {plane}: {bad}"
        pairs = np.repeat(levels[plane][:, None], k, axis=1)
        bad = lc.first_cell(prof[:, :, :7].sum(axis=2, dtype=np.uint64), pairs, ("k-mer", "base"))
        assert bad is None, f"edit profile, plane {plane}: operations 0..6 against the k-mer's pairs: {bad}"
        del out
    ctx.check()


# ---- 3: dense, the word-parallel kernel ----

@pytest.mark.parametrize("k,L", [(10, 100), (16, 300)])
def test_dense_word_parallel_count(ctx, k, L):
    """k = 10 is no bit-sliced instantiation; windows of 300 bases (slots of 80 bytes, 53,687,078 windows) are
    longer than one 256-base fetch.  The largest image, 32 candidates."""
    seg, idx, per = dense(k, 32, L, TOP)
    count_and_accumulate(ctx, k, seg, L, lc.expected_counts(idx, per), WORD, (k, L))


# ---- 4: sparse, ragged windows ----

@pytest.mark.parametrize("k", [10, 16, 22, 32])
def test_sparse_ragged_windows(ctx, k):
    """A zero image of the largest size with ragged windows ending at, starting at and straddling base 2^32 and
    base 2^33 (one with a 256-base fetch seam on the boundary), at base 0 and up to the image's last base, some
    with N: the oracle's counts, ac_check clean, twice the counts in accumulate mode.  Then one more window,
    33 bases from the image's last 32: the device error word reports it and it is skipped."""
    import torch

    dev = device()
    km, regions, windows = lc.sparse_case(k)
    want = lc.sparse_expected(k)
    codes, nmask = lc.sparse_image(regions, TOP, dev)

    def seg_of(ws):
        start = torch.tensor([s for s, _ in ws], dtype=torch.int64, device=dev)
        length = torch.tensor([n for _, n in ws], dtype=torch.int32, device=dev)
        return segment(km, codes, nmask, len(ws), TOP, start, length)

    count_and_accumulate(ctx, k, seg_of(windows), None, want, WORD, ("sparse", k))
    bad = seg_of(windows[:7] + [(TOP - 32, 33)] + windows[7:])
    ctx.count_device(k, [bad])
    with pytest.raises(ac.ApproxCounterError) as ei:
        ctx.check()
    assert ei.value.status == 1 and "malformed" in str(ei.value)
    ctx.check()  # the word was cleared
    same_counts(("sparse, one window past the image", k), bad, want)


# ---- the bound itself ----

def test_images_between_the_bound_and_2_34_are_refused(ctx):
    """An image of 2^34 - 4096 bases or more is refused before any launch, by the count and by the hits entry
    points; the largest accepted one is what every test above counted."""
    import torch

    dev = device()
    km, texts, per, _ = lc.dense_dictionary(16, 32, 100)
    idx, _ = lc.dense_index(40, len(texts), 1, [], [0], dev)
    codes, nmask = lc.dense_image(*lc.text_tables(texts), idx, 48 * 128, dev)
    seg = segment(km, codes, nmask, 40, 48 * 128)
    h = torch.zeros(ac.hits_words(32, 40), dtype=torch.int32, device=dev)
    for n_bases in (lc.MAX_IMAGE_BASES, lc.MAX_IMAGE_BASES + 32, (1 << 34) - 1024, (1 << 34) - 32, 1 << 34):
        seg.n_bases = n_bases
        for kw in ({}, {"hits": [h]}) if BS_ON else ({},):
            with pytest.raises(ac.ApproxCounterError) as ei:
                ctx.count_device(16, [seg], window_len=[100], **kw)
            assert ei.value.status == 1 and "2^34 - 4096" in str(ei.value), n_bases
    seg.n_bases = TOP  # accepted (the 40 windows and what a lane loads past a slot lie inside the tensors, whatever the image claims)
    ctx.count_device(16, [seg], window_len=[100])
    torch.cuda.synchronize()
    ctx.check()
    same_counts("after the refusals", seg, lc.expected_counts(idx, per))


# ---- last: the module's peak ----

def test_peak_device_memory():
    import torch

    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory of the large-image tests: {peak / GIB:.2f} GiB", flush=True)
    assert peak < PEAK_LIMIT, peak
