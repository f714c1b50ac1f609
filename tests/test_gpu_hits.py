"""GPU tests of the hit levels (ac_window_hits_device / _samples, ac_hit_level_counts_device; DESIGN.md §4e
"Hit levels"): the hits-writing family of the bit-sliced count kernel (bsh_count.hip) and the level-count
kernel.  Expected values: tests/hits_cases.expected_hits, hit_e[w][c] = d(c, w) <= e from the oracle's DP
distance.  Every matrix is compared bit for bit; the counts of the same launch must equal the expected
counts and the ordinary call's.

Every device hits buffer is filled with 0xFFFFFFFF before the launch and followed by guard words of the
same value: a word the launch did not write, a stray bit past n_kmers and a store past the matrix all show.
The samples route's device matrices are the library's own; its host matrices are filled with 0xFFFFFFFF by
ApproxCounter.window_hits before the call (a word the copy back did not reach shows) and compared bit for
bit as well.

With AC_BITSLICE=0 in the environment no launch is bit-sliced, so every hits call must be refused
(AC_ERR_INVALID, nothing written) instead.

The jobs stage's inline N records do not reach these launches: the device route and the samples route
read a window's N bits from its N-bitmap words (or know the image to hold no N), so the N cases below are
bitmap words, has_n = 0, windows of 5 and more N, and an all-N window."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.hits_cases import FILL, GUARD, equal_case, expected_hits, hits_case, pack_hits
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_bitslice import BITSLICE, kernel_of, n_windows_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1


@pytest.fixture(scope="module")
def ctxs():
    """One context per edit budget (the budget is sticky; the session's `counter` stays at 2)."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (0, 1, 2, 3)}
    yield made
    for c in made.values():
        c.close()


def refused(fn, word="window hits"):
    with pytest.raises(_lib.ApproxCounterError) as e:
        fn()
    assert e.value.status == _lib.AC_ERR_INVALID, e.value
    assert word in str(e.value), e.value
    return str(e.value)


def device_hits(c, k, parts, lens=None, check_plain=True):
    """ac_window_hits_device over resident images: parts = [(kmers, windows)], a part without windows is a
    dead segment (no matrix).  Returns [(counts, matrix (E + 1, n_windows, words))]; asserts the guard
    words, and that an ordinary count launch of the same segments gives the same counts."""
    import torch

    E = c.max_errors
    packed = [ac.pack_windows(w) for _, w in parts]
    lens = lens or [p.equal_window_len() or 100 for p in packed]
    segs = [ac.DeviceSegment.upload(km, p) for (km, _), p in zip(parts, packed)]
    words = [ac.hits_words(s.n_kmers, s.n_windows, E) for s in segs]
    bufs = [torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") if n else None for n in words]
    call = lambda: c.count_device(k, segs, window_len=lens, hits=bufs)  # noqa: E731
    if not BS_ON:
        refused(call)
        torch.cuda.synchronize()
        for b in bufs:
            assert b is None or bool((b == -1).all()), "a refused call wrote"
        return None
    call()
    torch.cuda.synchronize()
    c.check()
    assert kernel_of(c) == 1
    out = []
    for s, b, n in zip(segs, bufs, words):
        counts = s.counts_numpy()
        if b is None:
            out.append((counts, np.zeros((E + 1, s.n_windows, (s.n_kmers + 31) // 32), np.uint32)))
            continue
        h = b.cpu().numpy().view(np.uint32)
        assert (h[n:] == FILL).all(), "a store past the matrix"
        out.append((counts, h[:n].reshape(E + 1, s.n_windows, (s.n_kmers + 31) // 32).copy()))
    if check_plain:
        for s in segs:
            s.counts.fill_(-1)
        c.count_device(k, segs, window_len=lens)
        torch.cuda.synchronize()
        c.check()
        for s, (counts, _) in zip(segs, out):
            np.testing.assert_array_equal(s.counts_numpy(), counts, err_msg="hits launch vs ordinary launch")
    return out


def popcounts(m, n_kmers):
    return ac.unpack_hits(m, n_kmers).sum(axis=(0, 1)).astype(np.uint64)


def check(got, hit, counts, what):
    """Matrix bit-exact (which also says: no unwritten word, no bit past n_kmers), counts, popcount sum."""
    g_counts, g_m = got
    want = pack_hits(hit)
    assert g_m.shape == want.shape, what
    bad = np.argwhere(g_m != want)
    assert not len(bad), f"{what}: {len(bad)} words differ, first (level, window, word) {bad[0]}: " \
                         f"{g_m[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"
    np.testing.assert_array_equal(g_counts, counts, err_msg=str(what))
    np.testing.assert_array_equal(popcounts(g_m, hit.shape[2]), g_counts, err_msg=str(what))


def one(c, k, n_kmers, n_windows, L, seed, p_n=0.01):
    km, w, hit, counts = hits_case(seed, k, n_kmers, n_windows, L, c.max_errors, p_n=p_n)
    got = device_hits(c, k, [(km, w)])
    if got:
        check(got[0], hit, counts, (k, n_kmers, n_windows, L))


# ---- every k, every budget --------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_every_k_at_two_edits(ctxs, k):
    """300 candidates (groups of 256 + 44: 8 and 2 lanes per window), 37 windows of 100 bases: a partial
    last row at 8 and 32 windows per row."""
    one(ctxs[2], k, 300, 37, 100, 7000 + k)


@pytest.mark.parametrize("k", [16, 22, 29, 32])
@pytest.mark.parametrize("E", [0, 1, 3])
def test_other_budgets(ctxs, E, k):
    """E = 0 / 1 write 1 / 2 planes from the three-row kernel, E = 3 four from the four-row one; 100
    candidates make it 4 lanes and 16 windows per row.  (hits_case asserts a pair at distance exactly 3.)"""
    one(ctxs[E], k, 300, 37, 100, 7100 + 10 * k + E)
    one(ctxs[E], k, 100, 37, 100, 7200 + 10 * k + E)


# ---- shapes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 31, 32, 33, 64, 65, 255, 256, 257, 289, 500])
def test_candidate_counts(ctxs, n_kmers):
    """1..32 candidates: two lanes per window, the second without a word; 33..64: both; 65, 255: partial last
    words at 4 and 8 lanes; 257: a second group of one candidate; 289, 500: two groups with different lanes
    per window."""
    for E, k in ((2, 16), (3, 22)):
        one(ctxs[E], k, n_kmers, 37, 100, 7300 + n_kmers)


@pytest.mark.parametrize("k", [16, 32])
def test_window_lengths(ctxs, k):
    for L in (1, k - 3, k, k + 2, 101, 255, 256):
        for E in (2, 3):
            one(ctxs[E], k, 70, 37, L, 7400 + L, p_n=0.02)


@pytest.mark.parametrize("n_windows", [1, 7, 8, 9, 63, 64, 65])
def test_window_counts(ctxs, n_windows):
    """Around a row of 8 (300 candidates) and of 32 (40 candidates: 63, 64, 65)."""
    for n_kmers in (300, 40):
        one(ctxs[2], 16, n_kmers, n_windows, 101, 7500 + n_windows)
    one(ctxs[3], 22, 40, n_windows, 101, 7600 + n_windows)


# ---- N ----------------------------------------------------------------------------------------------

def test_n_bitmap_words_on_the_device_route(ctxs):
    """Every window with 1..4 N, windows with 5..7 N, N at the first and last base, and an all-N window,
    whose rows of the matrix are zero."""
    for counts_n, spots in (([1, 2, 3, 4], ()), ([2], (0, 99)), ([0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99)),
                            ([0, 0, 0, 100], ())):
        km, w = n_windows_case(len(counts_n) + len(spots), 37, 100, counts_n, spots)
        hit, counts = expected_hits(16, km, w, 2)
        got = device_hits(ctxs[2], 16, [(km, w)])
        if got:
            check(got[0], hit, counts, counts_n)
            all_n = [i for i in range(37) if (w[i] == 4).all()]
            assert (100 in counts_n) == bool(all_n) and not got[0][1][:, all_n, :].any()


def samples_hits(c, k, parts):
    """ApproxCounter.window_hits (ac_sample_upload_slot + ac_window_hits_samples), against the expected
    levels and against ac_error_count_samples over the same uploads."""
    imgs = [(np.asarray(km, np.uint64), ac.pack_windows(w)) for km, w in parts]
    if not BS_ON:
        refused(lambda: c.window_hits(k, imgs))
        return
    got = c.window_hits(k, imgs)
    assert kernel_of(c) == 1
    plain = c.count_samples(k, [(km, c.upload_sample(img, i)) for i, (km, img) in enumerate(imgs)])
    for (km, w), wh, p in zip(parts, got, plain):
        hit, counts = expected_hits(k, km, w, c.max_errors)
        assert wh.levels.shape == (c.max_errors + 1, len(w), (len(km) + 31) // 32)
        check((wh.counts, wh.levels), hit, counts, "samples")
        np.testing.assert_array_equal(p, wh.counts)
        np.testing.assert_array_equal(wh.level_counts().sum(axis=0), wh.counts)
        np.testing.assert_array_equal(wh.distances(), np.minimum(ac.distances_from_hits(hit), c.max_errors + 1))


def test_samples_route(ctxs):
    """The CLI's route, both ends fused: an image without any N (has_n = 0: the N bitmap is not read) beside
    one with N in most windows, windows of 5 and more N and an all-N window among them; E = 2 and 3."""
    km_a, w_a = equal_case(7701, 70, 37, 100, p_n=0.0)
    km_c, w_c = equal_case(7703, 300, 37, 100, p_n=0.0, k=22)
    assert not any("N" in x for x in w_a + w_c)
    km_b, w_b = n_windows_case(7702, 41, 101, [0, 1, 5, 0, 6, 101, 7], (0, 15, 16, 31, 32, 100))
    for E in (2, 3):
        samples_hits(ctxs[E], 16, [(km_a, w_a), (km_b, w_b)])
    samples_hits(ctxs[3], 22, [(km_c, w_c)])


# ---- fused segments, items of several rows ------------------------------------------------------------

def fused_parts(k, E):
    a = hits_case(7801, k, 300, 90, 150, E)
    b = hits_case(7802, k, 37, 70, 151, E)
    d = hits_case(7803, k, 65, 9, 33, E)
    dead = (a[0][:5], [])
    return [a[:2], dead, b[:2], d[:2]], [a[2:], None, b[2:], d[2:]]


def test_four_fused_segments_with_a_dead_one(ctxs):
    """Different n_kmers, lengths and window counts, each segment its own matrix; the dead segment (no
    windows) has no matrix and its counts are zeroed."""
    for E, k in ((2, 16), (3, 22)):
        parts, want = fused_parts(k, E)
        got = device_hits(ctxs[E], k, parts)
        if not got:
            continue
        for g, wnt in zip(got, want):
            if wnt is None:
                assert not g[0].any()
            else:
                check(g, wnt[0], wnt[1], (E, k))


def child_multi_row_items():
    """1 % of the waves that fit (AC_BS_WAVES_PCT=1): every wave claims items of several rows and rows of
    several items, so each wave stores many rows' words; 3000 windows drawn from 61 distinct texts."""
    for E, k in ((2, 16), (3, 22)):
        km, texts, hit_t, _ = hits_case(7900 + k, k, 300, 61, 100, E)
        idx = np.random.default_rng(k).integers(0, len(texts), size=3000)
        hit, w = hit_t[:, idx, :], [texts[i] for i in idx]
        with ac.ApproxCounter(0, max_errors=E) as c:
            got = device_hits(c, k, [(km, w)], check_plain=False)
            if not got:
                continue
            print(f"K {k} E {E}: {c.last_launch()}", flush=True)
            assert int(c.last_launch()["windows_per_wave"]) > 1
            check(got[0], hit, hit.sum(axis=(0, 1)).astype(np.uint64), (E, k))


def run_child(call, **env):
    code = f"from tests.test_gpu_hits import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_items_of_several_rows():
    print(run_child("child_multi_row_items()", AC_BS_WAVES_PCT="1"))


# ---- the level-count kernel -----------------------------------------------------------------------------

def test_level_counts_of_the_gpus_own_matrices(ctxs):
    """ac_hit_level_counts_device over the matrix a hits launch just wrote: equal to numpy's column sums of
    the expected levels, and summing to the launch's counts."""
    import torch

    for E, k, n_kmers, n_windows in ((2, 16, 300, 90), (3, 22, 33, 37), (0, 32, 1, 9)):
        c = ctxs[E]
        km, w, hit, counts = hits_case(8000 + k, k, n_kmers, n_windows, 100, E)
        if not BS_ON:
            device_hits(c, k, [(km, w)])
            continue
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        buf = torch.full((ac.hits_words(n_kmers, n_windows, E) + GUARD,), -1, dtype=torch.int32, device="cuda")
        c.count_device(k, [seg], window_len=[100], hits=[buf])
        lc = c.hit_level_counts(buf, n_kmers, n_windows, E + 1)
        torch.cuda.synchronize()
        c.check()
        lc = lc.cpu().numpy().astype(np.uint64)
        np.testing.assert_array_equal(lc, hit.sum(axis=1))
        np.testing.assert_array_equal(lc.sum(axis=0), seg.counts_numpy())
        np.testing.assert_array_equal(lc.sum(axis=0), counts)


@pytest.mark.parametrize("n_windows", [1, 31, 32, 255, 256, 257, 1100])
def test_level_counts_at_the_flush_threshold(counter, n_windows):
    """Hand-built matrices (no count launch: this kernel runs whatever AC_BITSLICE says): an all-ones plane --
    every counter reaches n_windows, through the planes' flush at 31 words and with one wave and several --
    and random planes; 70, 1000 and 2100 candidates: 3 word columns (16 windows per wave read, a partial last
    word), 32 (two windows per read) and 66 (two column tiles)."""
    import torch

    rng = np.random.default_rng(n_windows)
    for n_kmers in (70, 1000, 2100):
        hit = np.stack([np.ones((n_windows, n_kmers), bool), rng.random((n_windows, n_kmers)) < 0.5,
                        rng.random((n_windows, n_kmers)) < 0.03])
        m = pack_hits(hit)
        # (bits past n_kmers set in the last word: the kernel must not count them into a neighbour)
        if n_kmers % 32:
            m[:, :, -1] |= np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
        d = torch.from_numpy(m.view(np.int32)).cuda()
        lc = counter.hit_level_counts(d, n_kmers, n_windows, 3)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(lc.cpu().numpy(), hit.sum(axis=1))


# ---- refusals -----------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Each case of the header's list: AC_ERR_INVALID naming the constraint, nothing enqueued (the buffers
    keep their fill, the device error word stays clean), and the context counts correctly afterwards."""
    import torch

    k = 22
    eq = equal_case(8101, 40, 30, 100, k=k)
    ragged = cases.planted_case(8102, k, 40, 30, win_len=(90, 110))
    long = equal_case(8103, 40, 9, 300, k=k)

    def dev(c, kk, parts, lens):
        segs = [ac.DeviceSegment.upload(km, ac.pack_windows(w)) for km, w in parts]
        bufs = [torch.full((max(ac.hits_words(s.n_kmers, s.n_windows, 3), 1),), -1, dtype=torch.int32, device="cuda")
                for s in segs]
        return segs, bufs, (lambda: c.count_device(kk, segs, window_len=lens, hits=bufs))

    with ac.ApproxCounter(0) as c:
        every = []
        segs, bufs, call = dev(c, k, [ragged], None)
        assert "ragged" in refused(call) or not BS_ON
        every += bufs
        for kk in (15, 17):
            km, w = equal_case(8104 + kk, 40, 30, 100, k=kk)
            segs, bufs, call = dev(c, kk, [(km, w)], [100])
            assert "16 or 18..32" in refused(call)
            every += bufs
        segs, bufs, call = dev(c, k, [long], [300])
        assert "1..256" in refused(call)
        every += bufs
        # a NULL matrix for a live segment; accumulate mode; count vectors that alias
        segs, bufs, _ = dev(c, k, [eq, eq], [100, 100])
        refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=[bufs[0], None]))
        refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=bufs, accumulate=True))
        segs[1].counts = segs[0].counts
        if BS_ON:
            assert "overlap" in refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=bufs))
        every += bufs
        # the samples route: an equal job beside a ragged one, and a ragged one alone
        imgs = [(np.asarray(km, np.uint64), ac.pack_windows(w)) for km, w in (eq, ragged)]
        assert "ragged" in refused(lambda: c.window_hits(k, imgs)) or not BS_ON
        assert "ragged" in refused(lambda: c.window_hits(k, imgs[1:])) or not BS_ON
        torch.cuda.synchronize()
        assert all(bool((b == -1).all()) for b in every), "a refused call wrote"
        c.check()
        # the context still counts, and -- bit-sliced -- still writes hits
        for part in (ragged, eq, long):
            np.testing.assert_array_equal(c.count_jobs(k, [part])[0], oracle.count_myers(k, *part))
        got = device_hits(c, k, [eq])
        if got:
            check(got[0], *expected_hits(k, eq[0], eq[1], 2), "after the refusals")
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:
        segs, bufs, call = dev(multi, k, [eq], [100])
        assert "single-device" in refused(call)
        assert "single-device" in refused(lambda: multi.window_hits(k, [(np.asarray(eq[0], np.uint64), ac.pack_windows(eq[1]))]))
        np.testing.assert_array_equal(multi.count_jobs(k, [eq])[0], oracle.count_myers(k, *eq))


def child_bitslice_off():
    """AC_BITSLICE=0: every hits call is refused with the message that names the switch, and the ordinary
    count still runs (on the word-parallel kernel)."""
    import torch

    km, w = equal_case(8201, 40, 30, 100, k=22)
    img = ac.pack_windows(w)
    with ac.ApproxCounter(0) as c:
        seg = ac.DeviceSegment.upload(km, img)
        buf = torch.full((ac.hits_words(40, 30, 2),), -1, dtype=torch.int32, device="cuda")
        assert "AC_BITSLICE" in refused(lambda: c.count_device(22, [seg], window_len=[100], hits=[buf]))
        assert "AC_BITSLICE" in refused(lambda: c.window_hits(22, [(np.asarray(km, np.uint64), img)]))
        torch.cuda.synchronize()
        assert bool((buf == -1).all())
        c.count_device(22, [seg], window_len=[100])
        torch.cuda.synchronize()
        c.check()
        assert kernel_of(c) == 0
        assert np.array_equal(seg.counts_numpy(), oracle.count_myers(22, km, w))


def test_bitslice_off_refuses_every_hits_call():
    run_child("child_bitslice_off()", AC_BITSLICE="0")


# ---- the command line -----------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


@pytest.mark.parametrize("E", [2, 3])
def test_cli_levels(tmp_path, E):
    """The cfg1 FASTA (its sampled ends are equal windows) with --seed 1 --levels: the main files are byte for
    byte those of a run without the flag (at E = 2: the golden files), and every .levels line holds the main
    file's k-mer, sums to its count and equals the levels expected_hits derives from the sample --dump-sample
    writes with the same seed."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1",
            "--max-errors", str(E)]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--levels", "-o", "lv"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["-o", "plain"]).returncode == 0
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        main = open(tmp_path / f"lv_0.{end}").read()
        assert main == open(tmp_path / f"plain_0.{end}").read()
        if E == 2:
            assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        assert not os.path.exists(tmp_path / f"plain_0.{end}.levels")
        rows = [ln.split("\t") for ln in main.splitlines()]
        lv = [ln.split("\t") for ln in open(tmp_path / f"lv_0.{end}.levels").read().splitlines()]
        assert [a for a, _ in rows] == [x[0] for x in lv] and all(len(x) == E + 2 for x in lv)
        got = np.array([[int(v) for v in x[1:]] for x in lv], np.uint64)
        np.testing.assert_array_equal(got.sum(axis=1), np.array([int(b) for _, b in rows], np.uint64))
        kmers = [cases.kmer_value(a) for a, _ in rows]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        assert len(kmers) == 100 and len(wins) == 1000
        hit, _ = expected_hits(16, kmers, wins, E)
        np.testing.assert_array_equal(got, hit.sum(axis=1).T)
