"""GPU tests of the match spans (ac_hit_start_positions_device, ac_window_spans_samples; DESIGN.md §4e "Match
spans"): the span pass (hit_span.hip) behind count_device(..., spans=), alone over hand-built planes, behind
window_hits(..., spans=True) and behind the command line's --spans.  Expected values:
tests/span_cases.expected_spans -- the plain global DP of the reversed k-mer against the reversed text before
the expected end position (itself pinned to the oracle's distance), the least qualifying length.

Every device start buffer is filled with 0xFFFFFFFF before the call and followed by guard words of the same
value, and is compared word for word: a word the pass did not write, a stray bit past n_kmers or in a pair
without a hit, and a store past the matrix all show."""
import os
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.positions_cases import FILL, GUARD, profile_of
from tests.span_cases import (expected_spans, length_profile_of, pack_hits, pack_positions, pack_starts, plain_case,
                              spans_case)
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_bitslice import BITSLICE, kernel_of, n_windows_case
from tests.test_gpu_positions import refused, same
from tests.test_spans_cpu import hostile_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1
SLAB = 128  # hit words of a workgroup's slab (hit_span.hip SP_SLAB)


@pytest.fixture(scope="module")
def ctxs():
    """One context per edit budget (the budget is sticky; the session's `counter` stays at 2)."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (0, 1, 2, 3)}
    yield made
    for c in made.values():
        c.close()


def device_spans(c, k, parts, lens=None):
    """count_device(..., hits=, positions=, spans=) over resident images: parts = [(kmers, windows)], a part
    without windows is a dead segment (no matrices).  Returns [(counts, hit, position, start matrix)];
    asserts the guards."""
    import torch

    E = c.max_errors
    packed = [ac.pack_windows(w) for _, w in parts]
    lens = lens or [p.equal_window_len() or 100 for p in packed]
    segs = [ac.DeviceSegment.upload(km, p) for (km, _), p in zip(parts, packed)]
    hw = [ac.hits_words(s.n_kmers, s.n_windows, E) for s in segs]
    pw = [ac.positions_words(s.n_kmers, s.n_windows) for s in segs]
    full = lambda n: torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") if n else None  # noqa: E731
    hb, pb, sb = [full(n) for n in hw], [full(n) for n in pw], [full(n) for n in pw]
    call = lambda: c.count_device(k, segs, window_len=lens, hits=hb, positions=pb, spans=sb)  # noqa: E731
    if not BS_ON:
        refused(call)
        torch.cuda.synchronize()
        assert all(b is None or bool((b == -1).all()) for b in hb + pb + sb), "a refused call wrote"
        return None
    call()
    torch.cuda.synchronize()
    c.check()
    assert kernel_of(c) == 1
    out = []
    for s, h, p, t, nh, np_ in zip(segs, hb, pb, sb, hw, pw):
        words = (s.n_kmers + 31) // 32
        if h is None:
            zero = np.zeros((8, s.n_windows, words), np.uint32)
            out.append((s.counts_numpy(), np.zeros((E + 1, s.n_windows, words), np.uint32), zero, zero))
            continue
        h, p, t = (x.cpu().numpy().view(np.uint32) for x in (h, p, t))
        assert (h[nh:] == FILL).all() and (p[np_:] == FILL).all() and (t[np_:] == FILL).all(), "a store past a matrix"
        out.append((s.counts_numpy(), h[:nh].reshape(E + 1, s.n_windows, words).copy(),
                    p[:np_].reshape(8, s.n_windows, words).copy(), t[:np_].reshape(8, s.n_windows, words).copy()))
    return out


def check(got, hit, pos, start, counts, what):
    """The three matrices word for word, the counts, and the unpacked starts."""
    g_counts, g_m, g_p, g_s = got
    same(g_m, pack_hits(hit), f"{what} levels", "(level, window, word)")
    same(g_p, pack_positions(pos), f"{what} positions", "(plane, window, word)")
    same(g_s, pack_starts(start, hit[-1]), f"{what} starts", "(plane, window, word)")
    np.testing.assert_array_equal(g_counts, counts, err_msg=str(what))
    np.testing.assert_array_equal(ac.unpack_starts(g_s, hit[-1], hit.shape[2]), start, err_msg=str(what))


def one(c, k, n_kmers, n_windows, L, seed, p_n=0.01, need=()):
    km, w, hit, pos, start, counts, did = spans_case(seed, k, n_kmers, n_windows, L, c.max_errors, p_n=p_n)
    assert set(need) <= did, (need, did)
    got = device_spans(c, k, [(km, w)])
    if got:
        check(got[0], hit, pos, start, counts, (k, n_kmers, len(w), L, c.max_errors))


def pass_alone(c, k, km, w, m, planes, levels):
    """ac_hit_start_positions_device over given planes (no count launch): the start matrix, guards asserted."""
    import torch

    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    n = ac.positions_words(len(km), len(w))
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    hb = torch.from_numpy(np.ascontiguousarray(m).view(np.int32)).cuda()
    pb = torch.from_numpy(np.ascontiguousarray(planes).view(np.int32)).cuda()
    c.hit_start_positions(k, seg.kmers, len(km), seg, len(w[0]), hb, pb, levels, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "a store past the matrix"
    return got[:n].reshape(8, len(w), (len(km) + 31) // 32)


# ---- every k, every budget --------------------------------------------------------------------------

PLANTS2 = ("ins1", "ins2", "del1", "del2", "lead", "leadN", "clip", "s0", "s15", "s16", "s17", "s31", "s32", "s33",
           "sEnd", "len", "multi", "h")


@pytest.mark.parametrize("k", LISTED_K)
def test_every_k_at_two_edits(ctxs, k):
    """40 k-mers x (30 + plants) windows x 100 bases through count_device(..., spans=): inserted and missing
    bases, a substituted and an N first base, a clipped first base, starts at every word seam, every length
    k - 2 .. k + 2, pairs with more than one qualifying start, a tenth of the pairs hit."""
    one(ctxs[2], k, 40, 30, 100, 11000 + k, need=PLANTS2)


@pytest.mark.parametrize("k", [16, 22, 32])
@pytest.mark.parametrize("E", [0, 1, 3])
def test_other_budgets(ctxs, E, k):
    need = ("s0", "s33", "sEnd", "len", "h") + (("lead", "leadN", "clip", "multi", "ins1", "del1") if E else ())
    one(ctxs[E], k, 40, 30, 100, 11100 + 10 * k + E, need=need + (("ins3", "del3") if E == 3 else ()))


# ---- shapes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 31, 32, 33, 256, 257, 300])
def test_candidate_counts(ctxs, n_kmers):
    """A word's edges, and the word-column and candidate-group edges."""
    one(ctxs[2], 16, n_kmers, 30, 100, 11300 + n_kmers)
    if n_kmers in (1, 33, 257):
        one(ctxs[3], 22, n_kmers, 30, 100, 11350 + n_kmers)


@pytest.mark.parametrize("n_windows", [1, 7, 65])
def test_window_counts(ctxs, n_windows):
    for n_kmers in (300, 40):
        one(ctxs[2], 16, n_kmers, n_windows, 101, 11500 + n_windows)
    one(ctxs[3], 22, 40, n_windows, 101, 11600 + n_windows)


@pytest.mark.parametrize("k", [16, 32])
def test_window_lengths(ctxs, k):
    """k - 3, k, 63, 64, 65, 129, 255, 256: windows shorter than a k-mer, of one code word's worth and one
    base more, and plane 7 (starts at 128 and later)."""
    for L in (k - 3, k, 63, 64, 65, 129, 255, 256):
        need = ("s127", "s128", "s129", "sEnd") if L > 129 + k else ("sEnd",) if L >= k else ()
        for E in (2, 3):
            one(ctxs[E], k, 40, 12, L, 11400 + L, p_n=0.02, need=need)


@pytest.mark.parametrize("shape", [(20, SLAB - 1), (20, SLAB), (20, SLAB + 1), (20, 2 * SLAB + 1), (70, 43), (70, 86)])
def test_slab_edges(counter, shape):
    """The pass alone over hand-built planes (from the DP): one window short of a workgroup's slab of 128 hit
    words, exactly one, one past it and over two slabs at one word a window; and at three words a window a slab
    edge inside a window (43 windows = 129 words, 86 = 258)."""
    n_kmers, n_windows = shape
    k, E, L = 16, 2, 60
    km, texts = plain_case(11700 + n_kmers, k, n_kmers, 24, L, E)
    hit_t, pos_t, start_t, _, _ = expected_spans(k, km, texts, E)
    idx = np.random.default_rng(n_windows).integers(0, len(texts), size=n_windows)
    idx[-1] = int(np.argmax(hit_t[E].sum(axis=1)))  # (the last window, past the edge, has hits)
    hit, pos, start, w = hit_t[:, idx, :], pos_t[idx], start_t[idx], [texts[i] for i in idx]
    assert hit[E, -1].any() and hit[E].mean() > 0.03
    got = pass_alone(counter, k, km, w, pack_hits(hit), pack_positions(pos), E + 1)
    same(got, pack_starts(start, hit[E]), f"slab {shape}", "(plane, window, word)")


# ---- N ----------------------------------------------------------------------------------------------

def test_n_bitmap_words_on_the_device_route(ctxs):
    """Windows with 1..4, 5, 6, 7 and only N, N at the code-word and bitmap-word seams."""
    for counts_n, spots in (([1, 2, 3, 4], ()), ([0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99)), ([0, 0, 0, 100], ())):
        km, w = n_windows_case(len(counts_n) + len(spots), 37, 100, counts_n, spots)
        texts = ["".join("ACGTN"[int(x)] for x in row) for row in w]
        hit, pos, start, counts, _ = expected_spans(16, km, texts, 2)
        got = device_spans(ctxs[2], 16, [(km, w)])
        if got:
            check(got[0], hit, pos, start, counts, counts_n)


# ---- fused segments ---------------------------------------------------------------------------------

def test_four_fused_segments_with_a_dead_one(ctxs):
    for E, k in ((2, 16), (3, 22)):
        a = spans_case(11801, k, 300, 40, 150, E)
        b = spans_case(11802, k, 37, 30, 151, E)
        d = spans_case(11803, k, 65, 9, 33, E)
        got = device_spans(ctxs[E], k, [a[:2], (a[0][:5], []), b[:2], d[:2]])
        if not got:
            continue
        for g, wnt in zip(got, (a, None, b, d)):
            if wnt is None:
                assert not g[0].any()
            else:
                check(g, wnt[2], wnt[3], wnt[4], wnt[5], (E, k))


# ---- the pass alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 17])
def test_pass_alone_at_k_no_count_kernel_has(counter, k):
    """Hand-built planes from the DP at k = 5 and 17, levels 1..4: the pass runs at any k, on any context."""
    for E in (0, 1, 2, 3):
        for L in (k, 65, 256):
            km, w = plain_case(11900 + 10 * k + E, k, 40, 14, L, E)
            hit, pos, start, _, _ = expected_spans(k, km, w, E)
            got = pass_alone(counter, k, km, w, pack_hits(hit), pack_positions(pos), E + 1)
            same(got, pack_starts(start, hit[E]), f"k {k} E {E} L {L}", "(plane, window, word)")


@pytest.mark.parametrize("k", [5, 17])
def test_hostile_planes_give_no_bits(counter, k):
    """Hit bits where the position planes store 0, stored positions past the window, level bits without the
    top level's, stray bits past n_kmers in every plane: 0 bits for each, the real pairs' starts unchanged.
    (The step's bounds on such planes are checked on the CPU, under the sanitizers, before this runs.)"""
    km, w, m, planes, want = hostile_planes(k)
    same(pass_alone(counter, k, km, w, m, planes, 3), want, "hostile", "(plane, window, word)")
    top = np.uint32((0xFFFFFFFF << (40 % 32)) & 0xFFFFFFFF)
    m[:, :, -1] |= top
    planes[:, :, -1] |= top
    same(pass_alone(counter, k, km, w, m, planes, 3), want, "hostile, stray bits", "(plane, window, word)")


# ---- the samples route ------------------------------------------------------------------------------

def test_samples_route_and_profiles(ctxs):
    """ApproxCounter.window_hits(spans=True): both ends fused, E = 2 and 3; the three host matrices (filled
    with 0xFFFFFFFF before the call) bit for bit; .start_positions(), .span_lengths(), the numpy
    .length_profile() and the device-computed .start_profile() against numpy."""
    for E in (2, 3):
        a = spans_case(12001, 16, 40, 30, 100, E, p_n=0.0)
        b = spans_case(12002, 16, 70, 41, 101, E)
        c = ctxs[E]
        imgs = [(np.asarray(x[0], np.uint64), ac.pack_windows(x[1])) for x in (a, b)]
        if not BS_ON:
            refused(lambda: c.window_hits(16, imgs, spans=True))
            continue
        got = c.window_hits(16, imgs, spans=True)
        assert kernel_of(c) == 1
        for (km, w, hit, pos, start, counts, _), wh in zip((a, b), got):
            check((wh.counts, wh.levels, wh.planes, wh.starts), hit, pos, start, counts, "samples")
            np.testing.assert_array_equal(wh.end_positions(), pos)
            np.testing.assert_array_equal(wh.start_positions(), start)
            np.testing.assert_array_equal(wh.span_lengths(), np.where(hit[E], pos - start, -1))
            np.testing.assert_array_equal(wh.length_profile(), length_profile_of(hit, pos, start, 16))
            # (a start matrix stores the start itself where a position matrix stores pos - 1)
            np.testing.assert_array_equal(wh.start_profile(), profile_of(hit, start + 1, len(w[0])))
            np.testing.assert_array_equal(wh.start_profile().sum(axis=2), wh.length_profile().sum(axis=2))
        # positions=True alone still gives no spans; spans=True implied the positions
        plain = c.window_hits(16, imgs[:1], positions=True)[0]
        assert plain.starts is None
        with pytest.raises(ValueError):
            plain.start_positions()


# ---- refusals ---------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Every refusal of ac_hit_start_positions_device: AC_ERR_INVALID naming the constraint, nothing enqueued
    (the output keeps its fill), each followed by a correct call on the same context."""
    import torch

    k, E, L = 17, 2, 60
    km, w = plain_case(12100, k, 40, 12, L, E)
    hit, pos, start, _, _ = expected_spans(k, km, w, E)
    want = pack_starts(start, hit[E])
    with ac.ApproxCounter(0) as c:
        img = ac.pack_windows(w)
        seg = ac.DeviceSegment.upload(km, img)
        hb = torch.from_numpy(pack_hits(hit).view(np.int32)).cuda()
        pb = torch.from_numpy(pack_positions(pos).view(np.int32)).cuda()
        out = torch.full((ac.positions_words(40, 12),), -1, dtype=torch.int32, device="cuda")

        def good():
            torch.cuda.synchronize()
            assert bool((out == -1).all()), "a refused call wrote"
            same(pass_alone(c, k, km, w, pack_hits(hit), pack_positions(pos), E + 1), want, "after a refusal",
                 "(plane, window, word)")

        def call(kk=k, kmers=seg.kmers, sample=seg, wl=L, h=hb, p=pb, lv=E + 1, o=out):
            return lambda: c.hit_start_positions(kk, kmers, 40, sample, wl, h, p, lv, out=o)

        short = seg.as_struct().sample
        short.n_bases = 12 * 64 - 32  # (12 windows at 64-base strides do not fit)
        no_codes, no_nmask = seg.as_struct().sample, seg.as_struct().sample
        no_codes.codes = None
        no_nmask.nmask = None
        for fn, word in ((call(kk=1), "k must be 2..32"), (call(kk=33), "k must be 2..32"),
                         (call(lv=0), "levels must be 1..4"), (call(lv=5), "levels must be 1..4"),
                         (call(kk=3, lv=3), "levels must be below k"), (call(kk=4, lv=4), "levels must be below k"),
                         (call(wl=0), "window_len must be 1..256"), (call(wl=257), "window_len must be 1..256"),
                         (call(sample=short), "do not fit n_bases"),
                         (call(h=None), "hits or pos is NULL"), (call(p=None), "hits or pos is NULL"),
                         (call(sample=no_codes), "codes or nmask is NULL"), (call(sample=no_nmask), "codes or nmask is NULL"),
                         (call(kmers=None), "kmers is NULL")):
            assert word in refused(fn, "match spans"), word
            good()
        L_ = _lib.load()
        ws = seg.as_struct().sample
        import ctypes

        p32 = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        st = L_.ac_hit_start_positions_device(c.handle, k, seg.as_struct().kmers, 40, ctypes.byref(ws), L, p32(hb), p32(pb),
                                              E + 1, None, None)
        assert st == _lib.AC_ERR_INVALID and b"the output is NULL" in L_.ac_last_error(c.handle)
        st = L_.ac_hit_start_positions_device(c.handle, k, seg.as_struct().kmers, 40, None, L, p32(hb), p32(pb), E + 1,
                                              p32(out), None)
        assert st == _lib.AC_ERR_INVALID and b"sample is NULL" in L_.ac_last_error(c.handle)
        assert L_.ac_hit_start_positions_device(None, k, None, 40, None, L, None, None, 3, None, None) == _lib.AC_ERR_INVALID
        good()
        # no work: no k-mers, or no windows -- NULL matrices are fine, nothing is written
        c.hit_start_positions(k, None, 0, seg, L, None, None, E + 1, out=out)
        none = seg.as_struct().sample
        none.n_windows = 0
        c.hit_start_positions(k, seg.kmers, 40, none, L, None, None, E + 1, out=out)
        good()
        # the samples route: what ac_window_positions_samples refuses, and a NULL start matrix
        if BS_ON:
            km16, w16 = plain_case(12101, 16, 40, 12, 100, 2)
            ragged = cases.planted_case(12102, 16, 40, 30, win_len=(90, 110))
            imgs = [(np.asarray(x, np.uint64), ac.pack_windows(y)) for x, y in ((km16, w16), ragged)]
            assert "ragged" in refused(lambda: c.window_hits(16, imgs, spans=True))
            assert "16 or 18..32" in refused(lambda: c.window_hits(17, [(np.asarray(km, np.uint64), img)], spans=True))
            dev = c.upload_sample(imgs[0][1], 0)
            kk = np.asarray(km16, np.uint64)
            cnt = np.zeros(40, np.uint64)
            job = (_lib.ACSampleJob * 1)(_lib.ACSampleJob(kk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 40, dev,
                                                          cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
            hm = np.zeros(ac.hits_words(40, 12, 2), np.uint32)
            pm = np.zeros(ac.positions_words(40, 12), np.uint32)
            one32 = lambda a: (_lib.p32 * 1)(a.ctypes.data_as(_lib.p32) if a is not None else None)  # noqa: E731
            assert L_.ac_window_spans_samples(c.handle, 16, job, 1, one32(hm), one32(pm), one32(None)) == _lib.AC_ERR_INVALID
            assert b"start_host[j] is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_spans_samples(c.handle, 16, job, 1, one32(hm), one32(pm), None) == _lib.AC_ERR_INVALID
            wh = c.window_hits(16, imgs[:1], spans=True)[0]
            hit16, pos16, start16, counts16, _ = expected_spans(16, km16, w16, 2)
            check((wh.counts, wh.levels, wh.planes, wh.starts), hit16, pos16, start16, counts16, "after the refusals")
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:  # (an ac_create_multi context uses its first device)
        same(pass_alone(multi, k, km, w, pack_hits(hit), pack_positions(pos), E + 1), want, "multi", "(plane, window, word)")


# ---- the command line -------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


@pytest.mark.parametrize("E", [2, 3])
def test_cli_spans(tmp_path, E):
    """The cfg1 FASTA with --seed 1 --spans --positions --levels: the main files are byte for byte those of a
    run without the flags (at E = 2: the golden files); every .starts line holds the main file's k-mer and L
    integers, every .lengths line the k-mer and 2 E + 1, equal to what the DP derives from the sample
    --dump-sample writes with the same seed; both sum to the last column of the .levels line; and every
    per-distance count (the differences of consecutive .levels columns) is the DP's over the same sample."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1",
            "--max-errors", str(E)]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--spans", "--positions", "--levels", "-o", "sp"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["-o", "plain"]).returncode == 0
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        main = open(tmp_path / f"sp_0.{end}").read()
        assert main == open(tmp_path / f"plain_0.{end}").read()
        if E == 2:
            assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        assert not os.path.exists(tmp_path / f"plain_0.{end}.starts") and not os.path.exists(tmp_path / f"plain_0.{end}.lengths")
        rows = [ln.split("\t") for ln in main.splitlines()]
        table = lambda ext: [ln.split("\t") for ln in open(tmp_path / f"sp_0.{end}.{ext}").read().splitlines()]  # noqa: E731
        lv, ps, st, ln = table("levels"), table("positions"), table("starts"), table("lengths")
        kmers = [cases.kmer_value(a) for a, _ in rows]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        L = len(wins[0])
        assert len(kmers) == 100 and len(wins) == 1000 and all(len(x) == L for x in wins)
        names = [a for a, _ in rows]
        assert names == [x[0] for x in st] == [x[0] for x in ln] == [x[0] for x in ps]
        assert all(len(x) == L + 1 for x in st) and all(len(x) == 2 * E + 2 for x in ln)
        num = lambda t: np.array([[int(v) for v in x[1:]] for x in t], np.uint64)  # noqa: E731
        hit, pos, start, _, _ = expected_spans(16, kmers, wins, E)
        np.testing.assert_array_equal(num(st), profile_of(hit, start + 1, L).sum(axis=0))
        np.testing.assert_array_equal(num(ln), length_profile_of(hit, pos, start, 16).sum(axis=0))
        np.testing.assert_array_equal(num(ps), profile_of(hit, pos, L).sum(axis=0))
        np.testing.assert_array_equal(num(st).sum(axis=1), num(lv)[:, -1])
        np.testing.assert_array_equal(num(ln).sum(axis=1), num(lv)[:, -1])
        np.testing.assert_array_equal(np.diff(num(lv).astype(np.int64), axis=1, prepend=0),
                                      np.diff(hit.sum(axis=1).T.astype(np.int64), axis=1, prepend=0))
