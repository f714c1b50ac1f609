"""GPU tests of the match end positions (ac_window_positions_device / _samples,
ac_hit_position_profile_device; DESIGN.md §4e "Match end positions"): the hits-and-positions family of the
bit-sliced count kernel (bsp_count.hip) and the position-profile kernel.  Expected values:
tests/positions_cases.expected_positions -- a Sellers DP's whole last row, its minimum pinned to the
oracle's distance.  The counts, the hit levels and the positions of one launch are all compared, the two
matrices bit for bit.

Every device hits and position buffer is filled with 0xFFFFFFFF before the launch and followed by guard
words of the same value: a word the launch did not write, a stray bit past n_kmers or in a pair without a
hit, and a store past a matrix all show."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.positions_cases import (FILL, GUARD, expected_positions, pack_hits, pack_positions, positions_case,
                                   profile_of)
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_bitslice import BITSLICE, equal_case, kernel_of, n_windows_case

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


def refused(fn, word="window"):
    with pytest.raises(_lib.ApproxCounterError) as e:
        fn()
    assert e.value.status == _lib.AC_ERR_INVALID, e.value
    assert word in str(e.value), e.value
    return str(e.value)


def device_positions(c, k, parts, lens=None):
    """ac_window_positions_device over resident images: parts = [(kmers, windows)], a part without windows
    is a dead segment (no matrices).  Returns [(counts, hit matrix, position matrix)]; asserts the guards."""
    import torch

    E = c.max_errors
    packed = [ac.pack_windows(w) for _, w in parts]
    lens = lens or [p.equal_window_len() or 100 for p in packed]
    segs = [ac.DeviceSegment.upload(km, p) for (km, _), p in zip(parts, packed)]
    hw = [ac.hits_words(s.n_kmers, s.n_windows, E) for s in segs]
    pw = [ac.positions_words(s.n_kmers, s.n_windows) for s in segs]
    full = lambda n: torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") if n else None  # noqa: E731
    hb, pb = [full(n) for n in hw], [full(n) for n in pw]
    call = lambda: c.count_device(k, segs, window_len=lens, hits=hb, positions=pb)  # noqa: E731
    if not BS_ON:
        refused(call)
        torch.cuda.synchronize()
        assert all(b is None or bool((b == -1).all()) for b in hb + pb), "a refused call wrote"
        return None
    call()
    torch.cuda.synchronize()
    c.check()
    assert kernel_of(c) == 1
    out = []
    for s, h, p, nh, np_ in zip(segs, hb, pb, hw, pw):
        words = (s.n_kmers + 31) // 32
        if h is None:
            out.append((s.counts_numpy(), np.zeros((E + 1, s.n_windows, words), np.uint32),
                        np.zeros((8, s.n_windows, words), np.uint32)))
            continue
        h, p = h.cpu().numpy().view(np.uint32), p.cpu().numpy().view(np.uint32)
        assert (h[nh:] == FILL).all() and (p[np_:] == FILL).all(), "a store past a matrix"
        out.append((s.counts_numpy(), h[:nh].reshape(E + 1, s.n_windows, words).copy(),
                    p[:np_].reshape(8, s.n_windows, words).copy()))
    return out


def same(got, want, what, names):
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} words differ, first {names} {bad[0]}: " \
                         f"{got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def check(got, hit, pos, counts, what):
    """Both matrices bit-exact (no unwritten word, no bit past n_kmers, no position bit without a hit), the
    counts, and the unpacked positions."""
    g_counts, g_m, g_p = got
    same(g_m, pack_hits(hit), f"{what} levels", "(level, window, word)")
    same(g_p, pack_positions(pos), f"{what} positions", "(plane, window, word)")
    np.testing.assert_array_equal(g_counts, counts, err_msg=str(what))
    np.testing.assert_array_equal(ac.unpack_positions(g_p, hit[-1], hit.shape[2]), pos, err_msg=str(what))


def one(c, k, n_kmers, n_windows, L, seed, p_n=0.01, need=()):
    km, w, hit, pos, counts, did = positions_case(seed, k, n_kmers, n_windows, L, c.max_errors, p_n=p_n)
    assert set(need) <= did, (need, did)
    got = device_positions(c, k, [(km, w)])
    if got:
        check(got[0], hit, pos, counts, (k, n_kmers, n_windows, L, c.max_errors))


# ---- every k, every budget --------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_every_k_at_two_edits(ctxs, k):
    """40 k-mers x 30 windows x 100 bases: an overwritten position, two occurrences at the best distance,
    an end at the last base with the k-mer's last base missing, ends at the code-word seams, and a tenth
    of the pairs hit (positions_case asserts each)."""
    one(ctxs[2], k, 40, 30, 100, 9000 + k, need=("a", "b", "c", "e32", "h"))


@pytest.mark.parametrize("k", [16, 22, 29, 32])
@pytest.mark.parametrize("E", [0, 1, 3])
def test_other_budgets(ctxs, E, k):
    """E = 0 / 1: the three-row kernel, the levels above E must not move the position; E = 3: four rows,
    with a pair at distance exactly 3."""
    one(ctxs[E], k, 40, 30, 100, 9100 + 10 * k + E, need=("b", "h") + (("a", "c") if E else ()) + (("g",) if E == 3 else ()))


# ---- shapes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 31, 33, 255, 257, 500])
def test_candidate_counts(ctxs, n_kmers):
    """Block and group edges and 2..8 lanes per window."""
    for E, k in ((2, 16), (3, 22)):
        one(ctxs[E], k, n_kmers, 30, 100, 9300 + n_kmers)


@pytest.mark.parametrize("k", [16, 32])
def test_window_lengths(ctxs, k):
    """1, k - 3, k, 63, 64, 65, 129, 255, 256: a last block of 1..4 bases, and plane 7 (ends at 128, 129, L)."""
    for L in (1, k - 3, k, 63, 64, 65, 129, 255, 256):
        need = ("f128", "f129", f"f{L}") if L > 129 else ("d",) if L % 4 and L >= k else ()
        for E in (2, 3):
            one(ctxs[E], k, 40, 30, L, 9400 + L, p_n=0.02, need=need)


@pytest.mark.parametrize("n_windows", [1, 7, 9, 65])
def test_window_counts(ctxs, n_windows):
    """Rows that are not full, at 8 (300 candidates) and 32 (40) windows per row."""
    for n_kmers in (300, 40):
        one(ctxs[2], 16, n_kmers, n_windows, 101, 9500 + n_windows)
    one(ctxs[3], 22, 40, n_windows, 101, 9600 + n_windows)


# ---- N ----------------------------------------------------------------------------------------------

def test_n_bitmap_words_on_the_device_route(ctxs):
    for counts_n, spots in (([1, 2, 3, 4], ()), ([2], (0, 99)), ([0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99)),
                            ([0, 0, 0, 100], ())):
        km, w = n_windows_case(len(counts_n) + len(spots), 37, 100, counts_n, spots)
        texts = ["".join("ACGTN"[int(x)] for x in row) for row in w] if not isinstance(w[0], str) else w
        hit, pos, counts = expected_positions(16, km, texts, 2)
        got = device_positions(ctxs[2], 16, [(km, w)])
        if got:
            check(got[0], hit, pos, counts, counts_n)


# ---- the samples route ----------------------------------------------------------------------------------

def test_samples_route(ctxs):
    """ApproxCounter.window_hits(positions=True): both ends fused, E = 2 and 3; the host matrices (filled
    with 0xFFFFFFFF before the call) bit for bit, .end_positions() and the device-computed
    .position_profile()."""
    a = positions_case(9701, 16, 40, 30, 100, 2, p_n=0.0)
    b = positions_case(9702, 16, 70, 41, 101, 2)
    for E in (2, 3):
        c = ctxs[E]
        imgs = [(np.asarray(km, np.uint64), ac.pack_windows(w)) for km, w in (a[:2], b[:2])]
        if not BS_ON:
            refused(lambda: c.window_hits(16, imgs, positions=True))
            continue
        got = c.window_hits(16, imgs, positions=True)
        assert kernel_of(c) == 1
        for (km, w), wh in zip((a[:2], b[:2]), got):
            hit, pos, counts = expected_positions(16, km, w, E)
            check((wh.counts, wh.levels, wh.planes), hit, pos, counts, "samples")
            np.testing.assert_array_equal(wh.end_positions(), pos)
            np.testing.assert_array_equal(wh.position_profile(), profile_of(hit, pos, len(w[0])))


# ---- fused segments, items of several rows ------------------------------------------------------------

def test_four_fused_segments_with_a_dead_one(ctxs):
    for E, k in ((2, 16), (3, 22)):
        a = positions_case(9801, k, 300, 90, 150, E)
        b = positions_case(9802, k, 37, 70, 151, E)
        d = positions_case(9803, k, 65, 9, 33, E)
        got = device_positions(ctxs[E], k, [a[:2], (a[0][:5], []), b[:2], d[:2]])
        if not got:
            continue
        for g, wnt in zip(got, (a, None, b, d)):
            if wnt is None:
                assert not g[0].any()
            else:
                check(g, wnt[2], wnt[3], wnt[4], (E, k))


def child_multi_row_items():
    """1 % of the waves that fit (AC_BS_WAVES_PCT=1): every wave stores many rows' words; 3000 windows drawn
    from 61 distinct texts."""
    for E, k in ((2, 16), (3, 22)):
        km, texts, hit_t, pos_t, _, _ = positions_case(9900 + k, k, 300, 61, 100, E)
        idx = np.random.default_rng(k).integers(0, len(texts), size=3000)
        hit, pos, w = hit_t[:, idx, :], pos_t[idx], [texts[i] for i in idx]
        with ac.ApproxCounter(0, max_errors=E) as c:
            got = device_positions(c, k, [(km, w)])
            if not got:
                continue
            print(f"K {k} E {E}: {c.last_launch()}", flush=True)
            assert int(c.last_launch()["windows_per_wave"]) > 1
            check(got[0], hit, pos, hit.sum(axis=(0, 1)).astype(np.uint64), (E, k))


def run_child(call, **env):
    code = f"from tests.test_gpu_positions import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_items_of_several_rows():
    print(run_child("child_multi_row_items()", AC_BS_WAVES_PCT="1"))


# ---- the position-profile kernel ----------------------------------------------------------------------

def test_profile_of_the_gpus_own_matrices(ctxs):
    """ac_hit_position_profile_device over the matrices a launch just wrote: numpy's profile of the expected
    values, and its sum over the positions is the difference of consecutive hit_level_counts."""
    import torch

    for E, k, n_kmers, n_windows in ((2, 16, 300, 90), (3, 22, 33, 37), (0, 32, 1, 9)):
        c = ctxs[E]
        km, w, hit, pos, counts, _ = positions_case(10000 + k, k, n_kmers, n_windows, 100, E)
        if not BS_ON:
            device_positions(c, k, [(km, w)])
            continue
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        hb = torch.full((ac.hits_words(n_kmers, n_windows, E) + GUARD,), -1, dtype=torch.int32, device="cuda")
        pb = torch.full((ac.positions_words(n_kmers, n_windows) + GUARD,), -1, dtype=torch.int32, device="cuda")
        c.count_device(k, [seg], window_len=[100], hits=[hb], positions=[pb])
        prof = c.hit_position_profile(hb, pb, n_kmers, n_windows, E + 1, 100)
        lc = c.hit_level_counts(hb, n_kmers, n_windows, E + 1)
        torch.cuda.synchronize()
        c.check()
        prof, lc = prof.cpu().numpy().view(np.uint32), lc.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(prof, profile_of(hit, pos, 100))
        np.testing.assert_array_equal(prof.sum(axis=2), np.diff(lc, axis=0, prepend=0))


@pytest.mark.parametrize("n_windows", [1, 255, 4096, 4097, 9000])
def test_profile_of_hand_built_planes(counter, n_windows):
    """Random nested levels and positions (no count launch), bits past n_kmers set in every plane's last
    word; window counts at a workgroup's slab of 4096 windows, one past it and over two slabs; 70 and 1000
    candidates; window_len 256, and 100 with longer positions in the planes (dropped)."""
    import torch

    rng = np.random.default_rng(n_windows)
    for n_kmers, levels, L, Lmax in ((70, 4, 256, 256), (1000, 3, 100, 100), (33, 2, 100, 130)):
        d = rng.integers(0, levels + 3, size=(n_windows, n_kmers))
        hit = np.stack([d <= e for e in range(levels)])
        pos = np.where(hit[-1], rng.integers(1, Lmax + 1, size=d.shape), -1)
        m, planes = pack_hits(hit), pack_positions(pos)
        if n_kmers % 32:
            top = np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
            m[:, :, -1] |= top
            planes[:, :, -1] |= top
        prof = counter.hit_position_profile(torch.from_numpy(m.view(np.int32)).cuda(),
                                            torch.from_numpy(planes.view(np.int32)).cuda(), n_kmers, n_windows, levels, L)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(prof.cpu().numpy().view(np.uint32), profile_of(hit & (pos <= L), pos, L))


# ---- refusals -----------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Each case of hits_refusal and the NULL position matrix: AC_ERR_INVALID naming the constraint, nothing
    enqueued (the buffers keep their fill, the error word stays clean); the context counts afterwards and a
    following positions call is correct."""
    import torch

    k = 22
    eq = positions_case(10101, k, 40, 30, 100, 2)
    ragged = cases.planted_case(10102, k, 40, 30, win_len=(90, 110))
    long = equal_case(10103, 40, 9, 300, k=k)

    def dev(c, kk, parts, lens):
        segs = [ac.DeviceSegment.upload(km, ac.pack_windows(w)) for km, w in parts]
        hb = [torch.full((max(ac.hits_words(s.n_kmers, s.n_windows, 3), 1),), -1, dtype=torch.int32, device="cuda") for s in segs]
        pb = [torch.full((max(ac.positions_words(s.n_kmers, s.n_windows), 1),), -1, dtype=torch.int32, device="cuda")
              for s in segs]
        return segs, hb, pb, (lambda: c.count_device(kk, segs, window_len=lens, hits=hb, positions=pb))

    with ac.ApproxCounter(0) as c:
        every = []
        segs, hb, pb, call = dev(c, k, [ragged], None)
        assert "ragged" in refused(call) or not BS_ON
        every += hb + pb
        for kk in (15, 17):
            km, w = equal_case(10104 + kk, 40, 30, 100, k=kk)
            segs, hb, pb, call = dev(c, kk, [(km, w)], [100])
            assert "16 or 18..32" in refused(call)
            every += hb + pb
        segs, hb, pb, call = dev(c, k, [long], [300])
        assert "1..256" in refused(call)
        every += hb + pb
        segs, hb, pb, _ = dev(c, k, [eq[:2], eq[:2]], [100, 100])
        if BS_ON:
            assert "pos[i] is NULL" in refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=hb,
                                                                      positions=[pb[0], None]))
        refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=[hb[0], None], positions=pb))
        refused(lambda: c.count_device(k, segs, window_len=[100, 100], hits=hb, positions=pb, accumulate=True))
        every += hb + pb
        imgs = [(np.asarray(km, np.uint64), ac.pack_windows(w)) for km, w in (eq[:2], ragged)]
        assert "ragged" in refused(lambda: c.window_hits(k, imgs, positions=True)) or not BS_ON
        torch.cuda.synchronize()
        assert all(bool((b == -1).all()) for b in every), "a refused call wrote"
        c.check()
        for part in (ragged, eq[:2], long):
            np.testing.assert_array_equal(c.count_jobs(k, [part])[0], oracle.count_myers(k, *part))
        got = device_positions(c, k, [eq[:2]])
        if got:
            check(got[0], eq[2], eq[3], eq[4], "after the refusals")
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:
        segs, hb, pb, call = dev(multi, k, [eq[:2]], [100])
        assert "single-device" in refused(call)
        np.testing.assert_array_equal(multi.count_jobs(k, [eq[:2]])[0], oracle.count_myers(k, *eq[:2]))


def child_bitslice_off():
    """AC_BITSLICE=0: every positions call is refused with the message that names the switch."""
    import torch

    km, w = equal_case(10201, 40, 30, 100, k=22)
    img = ac.pack_windows(w)
    with ac.ApproxCounter(0) as c:
        seg = ac.DeviceSegment.upload(km, img)
        hb = torch.full((ac.hits_words(40, 30, 2),), -1, dtype=torch.int32, device="cuda")
        pb = torch.full((ac.positions_words(40, 30),), -1, dtype=torch.int32, device="cuda")
        assert "AC_BITSLICE" in refused(lambda: c.count_device(22, [seg], window_len=[100], hits=[hb], positions=[pb]))
        assert "AC_BITSLICE" in refused(lambda: c.window_hits(22, [(np.asarray(km, np.uint64), img)], positions=True))
        torch.cuda.synchronize()
        assert bool((hb == -1).all()) and bool((pb == -1).all())
        c.count_device(22, [seg], window_len=[100])
        torch.cuda.synchronize()
        c.check()
        assert kernel_of(c) == 0
        assert np.array_equal(seg.counts_numpy(), oracle.count_myers(22, km, w))


def test_bitslice_off_refuses_every_positions_call():
    run_child("child_bitslice_off()", AC_BITSLICE="0")


# ---- the command line -----------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


@pytest.mark.parametrize("E", [2, 3])
def test_cli_positions(tmp_path, E):
    """The cfg1 FASTA with --seed 1 --positions --levels: the main files are byte for byte those of a run
    without the flags (at E = 2: the golden files); every .positions line holds the main file's k-mer and L
    integers equal to the profile (folded over the distances) that the DP derives from the sample
    --dump-sample writes with the same seed, and sums to the last column of its .levels line."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1",
            "--max-errors", str(E)]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--positions", "--levels", "-o", "ps"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["-o", "plain"]).returncode == 0
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        main = open(tmp_path / f"ps_0.{end}").read()
        assert main == open(tmp_path / f"plain_0.{end}").read()
        if E == 2:
            assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        assert not os.path.exists(tmp_path / f"plain_0.{end}.positions")
        rows = [ln.split("\t") for ln in main.splitlines()]
        lv = [ln.split("\t") for ln in open(tmp_path / f"ps_0.{end}.levels").read().splitlines()]
        ps = [ln.split("\t") for ln in open(tmp_path / f"ps_0.{end}.positions").read().splitlines()]
        kmers = [cases.kmer_value(a) for a, _ in rows]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        L = len(wins[0])
        assert len(kmers) == 100 and len(wins) == 1000 and all(len(x) == L for x in wins)
        assert [a for a, _ in rows] == [x[0] for x in ps] and all(len(x) == L + 1 for x in ps)
        got = np.array([[int(v) for v in x[1:]] for x in ps], np.uint64)
        np.testing.assert_array_equal(got.sum(axis=1), np.array([int(x[-1]) for x in lv], np.uint64))
        hit, pos, _ = expected_positions(16, kmers, wins, E)
        np.testing.assert_array_equal(got, profile_of(hit, pos, L).sum(axis=0))
