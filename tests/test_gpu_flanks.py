"""GPU tests of the flank profiles (ac_hit_flank_profile_device, ac_window_flanks_samples; DESIGN.md §4e "Flank
profiles"): the flank pass (hit_flank.hip) after count_device(..., spans=), alone over hand-built planes, behind
window_hits(..., flanks=D) and behind the command line's --flanks.  Expected values:
tests/flank_cases.flank_profile_of -- the definition in plain numpy over the window strings and the matrices of
tests/span_cases.expected_spans.

Every device output is filled with 0xFFFFFFFF before the call and followed by guard words of the same value,
and is compared word for word: a word the pass did not define and a store past the result both show."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.flank_cases import flank_profile_of, matrices, pack_hits, pack_positions, pack_starts
from tests.hits_cases import FILL, GUARD
from tests.test_bs_nfa_k import LISTED_K
from tests.test_flanks_cpu import hostile_flank_planes
from tests.test_gpu_bitslice import BITSLICE, kernel_of
from tests.test_gpu_positions import refused, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1
CHUNK = 128    # windows of a chunk (hit_flank.hip FL_CHUNK): a strip is whole chunks
BLOCKS = 1024  # workgroups a launch aims at (FL_BLOCKS): at most BLOCKS / tiles strips, a tile one word column
NAMES = "(side, k-mer, column, symbol)"


@pytest.fixture(scope="module")
def ctxs():
    """One context per edit budget (the budget is sticky; the session's `counter` stays at 2)."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (0, 1, 2, 3)}
    yield made
    for c in made.values():
        c.close()


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def flank_pass(c, seg, L, plane, pos_m, start_m, n_kmers, n_windows, depth):
    """ac_hit_flank_profile_device over device tensors: the profile (2, n_kmers, depth, 5), guards asserted."""
    import torch

    n = ac.flank_words(n_kmers, depth)
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    c.hit_flank_profile(seg, L, plane, pos_m, start_m, n_kmers, n_windows, depth, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "a store past the profile"
    return got[:n].reshape(2, n_kmers, depth, 5)


def device_matrices(c, k, km, w, hit, pos, start):
    """The segment and its three device matrices.  Where the bit-sliced kernels count this k at the context's
    budget: from count_device(..., hits=, positions=, spans=), checked against the expected ones; anywhere
    else: the expected ones, uploaded."""
    import torch

    E = hit.shape[0] - 1
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
    want = pack_hits(hit), pack_positions(pos), pack_starts(start, hit[E])
    if not (BS_ON and k in LISTED_K and c.max_errors == E):
        return (seg,) + tuple(cuda(m).reshape(-1) for m in want)
    bufs = [torch.full((m.size,), -1, dtype=torch.int32, device="cuda") for m in want]
    c.count_device(k, [seg], window_len=[len(w[0])], hits=[bufs[0]], positions=[bufs[1]], spans=[bufs[2]])
    torch.cuda.synchronize()
    c.check()
    assert kernel_of(c) == 1
    for b, m, what in zip(bufs, want, ("levels", "positions", "starts")):
        same(b.cpu().numpy().view(np.uint32).reshape(m.shape), m, what, "(plane, window, word)")
    return (seg,) + tuple(bufs)


def one(c, k, n_kmers, n_windows, L, seed, depth=8):
    E = c.max_errors
    km, w, hit, pos, start, _ = matrices(seed, k, n_kmers, n_windows, L, E)
    seg, hb, pb, sb = device_matrices(c, k, km, w, hit, pos, start)
    top = hb[E * hit[0].shape[0] * ((n_kmers + 31) // 32):]  # the top level plane
    for D in depth if isinstance(depth, tuple) else (depth,):
        got = flank_pass(c, seg, L, top, pb, sb, n_kmers, len(w), D)
        same(got, flank_profile_of(w, hit[E], pos, start, D), (k, n_kmers, len(w), L, E, D), NAMES)
    return seg, hb, pb, sb, (km, w, hit, pos, start)


# ---- every k, every budget --------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_every_k_at_two_edits(ctxs, k):
    """40 k-mers x (30 + plants + 30) windows x 100 bases, D = 8, after the count launch and the span pass."""
    one(ctxs[2], k, 40, 30, 100, 13000 + k)


@pytest.mark.parametrize("k", [16, 22, 32])
@pytest.mark.parametrize("E", [0, 1, 3])
def test_other_budgets(ctxs, E, k):
    one(ctxs[E], k, 40, 30, 100, 13100 + 10 * k + E)


# ---- shapes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 31, 32, 33, 64, 65, 300])
def test_candidate_counts(ctxs, n_kmers):
    """A word's edges -- a tile is one word column -- and ten tiles."""
    one(ctxs[2], 16, n_kmers, 30, 100, 13300 + n_kmers)


def synthetic(seed, n_kmers, n_windows, L, density=0.03, p_n=0.05):
    """Hand-built planes over random windows (no alignment: the pass reads what the planes say): a hit at
    `density` of the pairs, its end anywhere in 1..L, its start anywhere below the end.  Returns the Dna5
    windows (n_windows, L) and hit, pos, start (n_windows, n_kmers)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, size=(n_windows, L)).astype(np.uint8)
    w[rng.random((n_windows, L)) < p_n] = 4
    hit = rng.random((n_windows, n_kmers)) < density
    hit[-1, :] = True  # (the last window, past the edge, has hits)
    pos = rng.integers(1, L + 1, size=hit.shape)
    start = (rng.random(hit.shape) * pos).astype(np.int64)
    return w, hit, np.where(hit, pos, -1), np.where(hit, start, -1)


def synthetic_pass(c, seed, n_kmers, n_windows, L, D):
    w, hit, pos, start = synthetic(seed, n_kmers, n_windows, L)
    seg = ac.DeviceSegment.upload(np.arange(n_kmers, dtype=np.uint64), ac.pack_windows(w))
    got = flank_pass(c, seg, L, cuda(pack_hits(hit[None])[0]), cuda(pack_positions(pos)), cuda(pack_starts(start, hit)),
                     n_kmers, n_windows, D)
    want = flank_profile_of(w, hit, pos, start, D)
    assert want.sum() > 100
    same(got, want, (n_kmers, n_windows, L, D), NAMES)


@pytest.mark.parametrize("n_windows", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges(counter, n_windows):
    """The pass alone over hand-built planes: one window, one short of a chunk of 128 windows, exactly one, one
    past it and over two (every strip one chunk here), at one and at three word columns."""
    for n_kmers in (20, 70):
        synthetic_pass(counter, 13400 + n_windows, n_kmers, n_windows, 60, 8)


@pytest.mark.parametrize("n_windows", [CHUNK * BLOCKS // 2 - 1, CHUNK * BLOCKS // 2, CHUNK * BLOCKS // 2 + 1])
def test_strip_edges(counter, n_windows):
    """Two tiles (40 k-mers) get at most 512 strips: 512 chunks of windows are 512 strips of one chunk, one
    window more makes every strip two chunks (257 strips, the last of one window)."""
    synthetic_pass(counter, 13500, 40, n_windows, 33, 16)


@pytest.mark.parametrize("k", [16, 32])
def test_window_lengths_and_depths(ctxs, k):
    """L = 1, k, 63, 65, 256 (a window shorter than the depth, one code word's worth and a base more, plane 7)
    at D = 1, 16 and 32."""
    for L in (1, k, 63, 65, 256):
        one(ctxs[2], k, 40, 12, L, 13600 + L, depth=(1, 16, 32))


# ---- the pass alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 17])
def test_pass_alone_at_k_no_count_kernel_has(counter, k):
    """Hand-built planes from the DP at k = 5 and 17, budgets 0..3: the pass runs at any k, on any context."""
    for E in (0, 1, 2, 3):
        for L in (k, 65, 256):
            km, w, hit, pos, start, _ = matrices(13700 + 10 * k + E, k, 40, 14, L, E)
            seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
            got = flank_pass(counter, seg, L, cuda(pack_hits(hit)[E]), cuda(pack_positions(pos)),
                             cuda(pack_starts(start, hit[E])), 40, len(w), 8)
            same(got, flank_profile_of(w, hit[E], pos, start, 8), f"k {k} E {E} L {L}", NAMES)


@pytest.mark.parametrize("k", [5, 17])
def test_hostile_planes_count_nothing(counter, k):
    """Hit bits where the position planes store 0 or a position past the window, starts at or past the end,
    stray bits past n_kmers in every plane: nothing counted for any, the real pairs' profile unchanged.  (The
    step's bounds on such planes are checked on the CPU, under the sanitizers, before this runs.)"""
    km, w, plane, planes, starts, hit, pos, start = hostile_flank_planes(k)
    want = flank_profile_of(w, hit[2], pos, start, 8)
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    same(flank_pass(counter, seg, len(w[0]), cuda(plane), cuda(planes), cuda(starts), 40, len(w), 8), want, "hostile", NAMES)
    stray = np.uint32((0xFFFFFFFF << (40 % 32)) & 0xFFFFFFFF)
    plane, planes, starts = plane.copy(), planes.copy(), starts.copy()
    plane[:, -1] |= stray
    planes[:, :, -1] |= stray
    starts[:, :, -1] |= stray
    same(flank_pass(counter, seg, len(w[0]), cuda(plane), cuda(planes), cuda(starts), 40, len(w), 8), want,
         "hostile, stray bits", NAMES)


def test_no_start_matrix_and_a_lower_plane(ctxs):
    """start = None: the right half as ever, the left half zeros.  Plane 0 of an E = 2 matrix: the exact
    occurrences alone, at the positions the matrices hold."""
    E, k, nk = 2, 16, 40
    seg, hb, pb, sb, (km, w, hit, pos, start) = one(ctxs[E], k, nk, 30, 100, 13800)
    plane_words = len(w) * 2
    got = flank_pass(ctxs[E], seg, 100, hb[E * plane_words:], pb, None, nk, len(w), 8)
    same(got, flank_profile_of(w, hit[E], pos, None, 8), "no start matrix", NAMES)
    assert got[0].any() and not got[1].any()
    got = flank_pass(ctxs[E], seg, 100, hb[:plane_words], pb, sb, nk, len(w), 8)
    want = flank_profile_of(w, hit[0], pos, start, 8)
    assert 0 < want.sum() < flank_profile_of(w, hit[E], pos, start, 8).sum()
    same(got, want, "plane 0", NAMES)


# ---- the samples route ------------------------------------------------------------------------------

def test_samples_route(ctxs):
    """ApproxCounter.window_hits(flanks=8): both ends fused, E = 2 and 3; the profile (filled with 0xFFFFFFFF
    before the call) word for word, beside the three matrices flanks= implies; and two jobs of which one has
    no windows."""
    for E in (2, 3):
        c = ctxs[E]
        a = matrices(13901, 16, 40, 30, 100, E)
        b = matrices(13902, 16, 70, 41, 101, E)
        imgs = [(x[0], ac.pack_windows(list(x[1]))) for x in (a, b)]
        if not BS_ON:
            refused(lambda: c.window_hits(16, imgs, flanks=8))
            continue
        got = c.window_hits(16, imgs, flanks=8)
        assert kernel_of(c) == 1
        for (km, w, hit, pos, start, counts), wh in zip((a, b), got):
            same(wh.levels, pack_hits(hit), "levels", "(level, window, word)")
            same(wh.planes, pack_positions(pos), "positions", "(plane, window, word)")
            same(wh.starts, pack_starts(start, hit[E]), "starts", "(plane, window, word)")
            np.testing.assert_array_equal(wh.counts, counts)
            prof = wh.flank_profile()
            assert prof.dtype == np.uint32
            same(prof, flank_profile_of(w, hit[E], pos, start, 8), "samples", NAMES)
            assert len(ac.flank_consensus(prof)) == len(km)
        # spans=True alone still gives no profile
        with pytest.raises(ValueError, match="flanks="):
            c.window_hits(16, imgs[:1], spans=True)[0].flank_profile()
        empty = (a[0][:5], ac.pack_windows([]))
        got = c.window_hits(16, [imgs[1], empty], flanks=3)
        same(got[0].flank_profile(), flank_profile_of(b[1], b[2][E], b[3], b[4], 3), "beside a job without windows", NAMES)
        assert got[1].flank_profile().shape == (2, 5, 3, 5) and not got[1].flank_profile().any() and not got[1].counts.any()
        c.check()


# ---- refusals ---------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Every refusal of ac_hit_flank_profile_device: AC_ERR_INVALID naming the constraint, nothing enqueued
    (the output keeps its fill), each followed by a correct call on the same context; then
    ac_window_flanks_samples' own."""
    import torch

    k, E, L, D = 17, 2, 60, 8
    km, w, hit, pos, start, _ = matrices(14000, k, 40, 12, L, E)
    nw = len(w)
    want = flank_profile_of(w, hit[E], pos, start, D)
    with ac.ApproxCounter(0) as c:
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
        hb, pb, sb = cuda(pack_hits(hit)[E]), cuda(pack_positions(pos)), cuda(pack_starts(start, hit[E]))
        out = torch.full((ac.flank_words(40, 32),), -1, dtype=torch.int32, device="cuda")

        def good():
            torch.cuda.synchronize()
            assert bool((out == -1).all()), "a refused call wrote"
            c.check()
            same(flank_pass(c, seg, L, hb, pb, sb, 40, nw, D), want, "after a refusal", NAMES)

        def call(sample=seg, wl=L, h=hb, p=pb, s=sb, n=nw, d=D, o=out):
            return lambda: c.hit_flank_profile(sample, wl, h, p, s, 40, n, d, out=o)

        short = seg.as_struct().sample
        short.n_bases = nw * 64 - 32  # (the windows at 64-base strides do not fit)
        no_codes, no_nmask = seg.as_struct().sample, seg.as_struct().sample
        no_codes.codes = None
        no_nmask.nmask = None
        for fn, word in ((call(d=0), "depth must be 1..32"), (call(d=33), "depth must be 1..32"),
                         (call(wl=0), "window_len must be 1..256"), (call(wl=257), "window_len must be 1..256"),
                         (call(sample=short), "do not fit n_bases"),
                         (call(h=None), "hit_plane or pos is NULL"), (call(p=None), "hit_plane or pos is NULL"),
                         (call(sample=no_codes), "codes or nmask is NULL"), (call(sample=no_nmask), "codes or nmask is NULL")):
            assert word in refused(fn, "flank profile"), word
            good()
        L_ = _lib.load()
        ws = seg.as_struct().sample
        p32 = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        st = L_.ac_hit_flank_profile_device(c.handle, ctypes.byref(ws), L, p32(hb), p32(pb), p32(sb), 40, D, None, None)
        assert st == _lib.AC_ERR_INVALID and b"the output is NULL" in L_.ac_last_error(c.handle)
        st = L_.ac_hit_flank_profile_device(c.handle, None, L, p32(hb), p32(pb), p32(sb), 40, D, p32(out), None)
        assert st == _lib.AC_ERR_INVALID and b"sample is NULL" in L_.ac_last_error(c.handle)
        assert L_.ac_hit_flank_profile_device(None, ctypes.byref(ws), L, p32(hb), p32(pb), p32(sb), 40, D, p32(out),
                                              None) == _lib.AC_ERR_INVALID
        good()
        # no k-mers: no work, nothing written.  No windows: zeros, NULL matrices are fine
        c.hit_flank_profile(seg, L, None, None, None, 0, nw, D, out=out)
        good()
        z = torch.full((ac.flank_words(40, D) + GUARD,), -1, dtype=torch.int32, device="cuda")
        c.hit_flank_profile(seg, L, None, None, None, 40, 0, D, out=z)
        torch.cuda.synchronize()
        z = z.cpu().numpy()
        assert not z[:-GUARD].any() and (z[-GUARD:] == -1).all()
        good()
        # the samples route: what ac_window_spans_samples refuses, a bad depth and a NULL profile
        if BS_ON:
            a = matrices(14001, 16, 40, 12, 100, 2)
            ragged = cases.planted_case(14002, 16, 40, 30, win_len=(90, 110))
            imgs = [(a[0], ac.pack_windows(list(a[1]))), (np.asarray(ragged[0], np.uint64), ac.pack_windows(ragged[1]))]
            assert "ragged" in refused(lambda: c.window_hits(16, imgs, flanks=8))
            assert "16 or 18..32" in refused(lambda: c.window_hits(17, [(km, ac.pack_windows(list(w)))], flanks=8))
            assert "depth must be 1..32" in refused(lambda: c.window_hits(16, imgs[:1], flanks=33), "flank profile")
            dev = c.upload_sample(imgs[0][1], 0)
            cnt = np.zeros(40, np.uint64)
            u64 = ctypes.POINTER(ctypes.c_uint64)
            job = (_lib.ACSampleJob * 1)(_lib.ACSampleJob(a[0].ctypes.data_as(u64), 40, dev, cnt.ctypes.data_as(u64)))
            n1 = len(a[1])
            hm = np.full(ac.hits_words(40, n1, 2), FILL, np.uint32)
            pm, sm = (np.full(ac.positions_words(40, n1), FILL, np.uint32) for _ in range(2))
            one32 = lambda x: (_lib.p32 * 1)(x.ctypes.data_as(_lib.p32) if x is not None else None)  # noqa: E731
            args = (one32(hm), one32(pm), one32(sm))
            assert L_.ac_window_flanks_samples(c.handle, 16, job, 1, 8, *args, one32(None)) == _lib.AC_ERR_INVALID
            assert b"flank_host[j] is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_flanks_samples(c.handle, 16, job, 1, 8, *args, None) == _lib.AC_ERR_INVALID
            assert b"flank_host is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_flanks_samples(c.handle, 16, job, 1, 0, *args, one32(hm)) == _lib.AC_ERR_INVALID
            assert b"depth must be 1..32" in L_.ac_last_error(c.handle)
            assert all((m == FILL).all() for m in (hm, pm, sm)), "a refused call wrote"
            wh = c.window_hits(16, imgs[:1], flanks=8)[0]
            same(wh.flank_profile(), flank_profile_of(a[1], a[2][2], a[3], a[4], 8), "after the refusals", NAMES)
        good()
    with ac.ApproxCounter(n_gpus=2) as multi:  # (an ac_create_multi context uses its first device)
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
        same(flank_pass(multi, seg, L, hb, pb, sb, 40, nw, D), want, "multi", NAMES)


# ---- the command line -------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


def test_cli_flanks(tmp_path):
    """The cfg1 FASTA with --seed 1 --flanks 8: the main files are byte for byte the golden ones; every .flanks
    line holds the main file's k-mer and 16 groups a,c,g,t,n -- the eight columns before the start from the
    farthest to the nearest, then the eight after the end from the nearest to the farthest -- equal to the
    profile derived from the sample --dump-sample writes with the same seed."""
    from tests.span_cases import expected_spans
    from tests.test_reader import decode, load_image

    D = 8
    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--flanks", str(D), "-o", "fl"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        main = open(tmp_path / f"fl_0.{end}").read()
        assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        assert not os.path.exists(tmp_path / f"fl_0.{end}.starts")  # (the flag alone writes its own file only)
        rows = [ln.split("\t") for ln in main.splitlines()]
        table = [ln.split("\t") for ln in open(tmp_path / f"fl_0.{end}.flanks").read().splitlines()]
        assert [x[0] for x in table] == [a for a, _ in rows] and all(len(x) == 2 * D + 1 for x in table)
        kmers = [cases.kmer_value(a) for a, _ in rows]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        assert len(kmers) == 100 and len(wins) == 1000
        hit, pos, start, _, _ = expected_spans(16, kmers, wins, 2)
        want = flank_profile_of(wins, hit[2], pos, start, D)
        got = np.array([[[int(v) for v in g.split(",")] for g in x[1:]] for x in table], np.uint32)  # (k-mer, 2 D, 5)
        np.testing.assert_array_equal(got[:, :D][:, ::-1], want[1])
        np.testing.assert_array_equal(got[:, D:], want[0])
        assert want[0].any() and want[1].any()
