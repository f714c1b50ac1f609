"""GPU tests of the co-occurrence (ac_hit_cooccurrence_device, ac_hit_cooccurrence, ac_hit_window_counts_device;
DESIGN.md §4e "Co-occurrence"): hit_cooc.hip's transposition, product and window-count kernels.  Expected
values: numpy's product H^t H of the unpacked plane (in float32, which is exact below 2^24, so that BLAS does
it) and its row sums; every comparison is exact.

Every output buffer is filled with 0xFFFFFFFF before the call and followed by guard words of the same value:
a word the call did not define and a store past the end both show.

Which path a shape takes (hit_cooc.h co_splits, pinned by tests/test_cooc_cpu.py::test_launch_rule): the
transposed planes are cut into slabs of 1024 windows.  Up to 2048 windows (one or two slabs) a workgroup takes
its tile pair's whole window axis and stores every word once: the unsplit path -- every shape below with
n_windows <= 2048, so all of the n_kmers list at 257 and 1100 windows.  From 2049 windows on the window axis is
split over workgroups that add into the zeroed output -- 2049 (two workgroups: two slabs and one), 5000 (three)
and 70001 windows (35) at 70 and 300 candidates -- unless the launch has 4096 workgroups without it: at three
planes that is 1366 tile pairs, 52 tiles of 64, so 3264 candidates x 2049 windows split and 3265 do not.  2048 /
2049 windows and 3264 / 3265 candidates straddle the two thresholds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.positions_cases import FILL, GUARD
from tests.hits_cases import expected_hits, hits_case, pack_hits
from tests.test_gpu_bitslice import BITSLICE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1


def p32(t):
    return ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)


def gram(hit):
    assert hit.shape[1] < 1 << 24
    h = hit.astype(np.float32)
    return np.stack([p.T @ p for p in h]).astype(np.uint32)


def filled(n):
    import torch

    return torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")


def take(buf, n, shape, what):
    """The first n words of a filled buffer, after the guard check."""
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n:] == FILL).all(), f"{what}: a store past the end"
    return h[:n].reshape(shape).copy()


def device_cooc(c, d_hits, n_kmers, n_windows, levels):
    """ac_hit_cooccurrence_device into a filled, guarded buffer: uint32 (levels, n, n)."""
    import torch

    n = levels * n_kmers * n_kmers
    out = filled(n)
    _lib.check(c._L.ac_hit_cooccurrence_device(c.handle, p32(d_hits), n_kmers, n_windows, levels, p32(out), None), c.handle)
    torch.cuda.synchronize()
    return take(out, n, (levels, n_kmers, n_kmers), "cooc")


def device_window_counts(c, d_hits, n_kmers, n_windows, levels):
    import torch

    n = levels * n_windows
    out = filled(n)
    _lib.check(c._L.ac_hit_window_counts_device(c.handle, p32(d_hits), n_kmers, n_windows, levels, p32(out), None), c.handle)
    torch.cuda.synchronize()
    return take(out, n, (levels, n_windows), "window counts")


def hand_built(n_kmers, n_windows, seed=0):
    """(hit bool (3, n_windows, n_kmers), matrix with stray bits): plane 0 all ones, 1 of density 0.5, 2 of 0.03."""
    rng = np.random.default_rng(1000 * n_kmers + n_windows + seed)
    hit = np.stack([np.ones((n_windows, n_kmers), bool), rng.random((n_windows, n_kmers)) < 0.5,
                    rng.random((n_windows, n_kmers)) < 0.03])
    m = pack_hits(hit)
    if n_kmers % 32:
        m[:, :, -1] |= np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
    return hit, m


def check_hand_built(c, n_kmers, n_windows):
    import torch

    hit, m = hand_built(n_kmers, n_windows)
    d = torch.from_numpy(m.view(np.int32)).cuda().reshape(-1)
    got = device_cooc(c, d, n_kmers, n_windows, 3)
    want = gram(hit)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} entries differ, first (plane, a, b) {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert (got[0] == n_windows).all()
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    lc = c.hit_level_counts(d, n_kmers, n_windows, 3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.diagonal(got, axis1=1, axis2=2), lc.cpu().numpy().view(np.uint32))
    wc = device_window_counts(c, d, n_kmers, n_windows, 3)
    np.testing.assert_array_equal(wc, hit.sum(axis=2))
    c.check()
    return got, d


# ---- hand-built matrices (no count launch: these run whatever AC_BITSLICE says) ---------------------------

@pytest.mark.parametrize("n_windows", [257, 1100])
@pytest.mark.parametrize("n_kmers", [1, 31, 32, 33, 63, 64, 65, 70, 127, 129, 300, 1000, 2100])
def test_candidate_counts(counter, n_kmers, n_windows):
    """One word and a partial one, one product tile of 64 and a partial second, 33 tiles (2100); 1100 windows
    are two slabs.  All unsplit."""
    check_hand_built(counter, n_kmers, n_windows)


@pytest.mark.parametrize("n_kmers", [70, 300])
@pytest.mark.parametrize("n_windows", [1, 31, 32, 33, 63, 64, 65, 255, 1100, 2048, 2049, 5000, 70001])
def test_window_counts(counter, n_windows, n_kmers):
    """Around a word of 32 windows and the transposition's 64; 2048 | 2049: the last unsplit shape and the
    first split one; 5000 and 70001 split in 3 and 35."""
    check_hand_built(counter, n_kmers, n_windows)


@pytest.mark.parametrize("n_kmers", [3264, 3265])
def test_the_tile_pair_threshold(counter, n_kmers):
    """Three planes of 2049 windows: 51 tiles are 3978 workgroups unsplit, so the window axis is split; 52
    tiles are 4134, so it is not."""
    check_hand_built(counter, n_kmers, 2049)


def test_the_single_plane_idiom(counter):
    """A view at plane 2's offset with levels = 1 equals plane 2 of the full call (split and unsplit)."""
    for n_kmers, n_windows in ((300, 257), (70, 5000)):
        got, d = check_hand_built(counter, n_kmers, n_windows)
        words = (n_kmers + 31) // 32
        one = device_cooc(counter, d[2 * n_windows * words:], n_kmers, n_windows, 1)
        np.testing.assert_array_equal(one[0], got[2])
        wc = device_window_counts(counter, d[2 * n_windows * words:], n_kmers, n_windows, 1)
        np.testing.assert_array_equal(wc[0], hand_built(n_kmers, n_windows)[0][2].sum(axis=1))


# ---- the GPU's own matrices ---------------------------------------------------------------------------------

@pytest.mark.skipif(not BS_ON, reason="AC_BITSLICE=0: no hits launch to take a matrix from")
@pytest.mark.parametrize("E,k,n_kmers,n_windows", [(2, 16, 300, 90), (3, 22, 33, 37), (0, 32, 1, 9)])
def test_cooccurrence_of_a_hits_launch(E, k, n_kmers, n_windows):
    """A hits launch on the bit-sliced route, then the co-occurrence of its buffer: the numpy product of the
    expected levels, its diagonal summing over the levels to the launch's counts."""
    import torch

    km, w, hit, counts = hits_case(8000 + k, k, n_kmers, n_windows, 100, E)
    with ac.ApproxCounter(0, max_errors=E) as c:
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        buf = filled(ac.hits_words(n_kmers, n_windows, E))
        c.count_device(k, [seg], window_len=[100], hits=[buf])
        got = device_cooc(c, buf, n_kmers, n_windows, E + 1)
        c.check()
        np.testing.assert_array_equal(got, gram(hit))
        diag = np.diagonal(got, axis1=1, axis2=2).astype(np.uint64)
        np.testing.assert_array_equal(diag.sum(axis=0), seg.counts_numpy())
        np.testing.assert_array_equal(diag.sum(axis=0), counts)
        np.testing.assert_array_equal(device_window_counts(c, buf, n_kmers, n_windows, E + 1), hit.sum(axis=2))
        np.testing.assert_array_equal(c.hit_cooccurrence(buf, n_kmers, n_windows, E + 1).cpu().numpy().view(np.uint32), got)
        torch.cuda.synchronize()


def test_window_hits_objects_reduce_on_the_device():
    """WindowHits.cooccurrence() / .window_counts() of a hits call's result (the counter attached) equal the
    numpy path of the same matrix."""
    if not BS_ON:
        pytest.skip("AC_BITSLICE=0: no hits launch to take a matrix from")
    km, w, hit, _ = hits_case(8301, 16, 70, 41, 100, 2)
    with ac.ApproxCounter(0) as c:
        wh = c.window_hits(16, [(np.asarray(km, np.uint64), ac.pack_windows(w))])[0]
        assert wh._counter is c
        want = gram(hit)
        np.testing.assert_array_equal(wh.cooccurrence(), want[2])
        np.testing.assert_array_equal(wh.cooccurrence(0), want[0])
        np.testing.assert_array_equal(wh.window_counts(), hit.sum(axis=2))


# ---- the host-buffer call -------------------------------------------------------------------------------------

def test_host_buffers_and_scratch_growth():
    """ac_hit_cooccurrence on 130 x 257 equals the device call; a larger matrix (1000 x 1100) on the same
    context, which grows both scratch blocks, is correct; so is the small one again; n_windows = 0 is zeros."""
    import torch

    with ac.ApproxCounter(0) as c:
        for n_kmers, n_windows in ((130, 257), (1000, 1100), (130, 257)):
            hit, m = hand_built(n_kmers, n_windows)
            got = c.cooccurrence_host(m, n_kmers, n_windows, 3)
            np.testing.assert_array_equal(got, gram(hit))
            d = torch.from_numpy(m.view(np.int32)).cuda()
            np.testing.assert_array_equal(got, device_cooc(c, d, n_kmers, n_windows, 3))
        zeros = c.cooccurrence_host(np.zeros(0, np.uint32), 130, 0, 3)
        assert zeros.shape == (3, 130, 130) and not zeros.any()
        assert not device_cooc(c, None, 130, 0, 3).any()
        c.check()


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """levels 0 and 5, a NULL output and a NULL matrix: AC_ERR_INVALID naming the constraint, nothing enqueued (the
    buffers keep their fill, the device error word stays clean), and a following call is correct; a two-device
    context computes on its first device."""
    import torch

    n_kmers, n_windows = 70, 300
    hit, m = hand_built(n_kmers, n_windows)
    want = gram(hit)

    def refused(c, status, word):
        assert status == _lib.AC_ERR_INVALID
        msg = c._L.ac_last_error(c.handle).decode()
        assert word in msg, msg

    with ac.ApproxCounter(0) as c:
        L, h = c._L, c.handle
        d = torch.from_numpy(m.view(np.int32)).cuda()
        out, wc = filled(3 * n_kmers * n_kmers), filled(3 * n_windows)
        for lv in (0, 5):
            refused(c, L.ac_hit_cooccurrence_device(h, p32(d), n_kmers, n_windows, lv, p32(out), None), "levels must be 1..4")
            refused(c, L.ac_hit_window_counts_device(h, p32(d), n_kmers, n_windows, lv, p32(wc), None), "levels must be 1..4")
            refused(c, L.ac_hit_cooccurrence(h, m.ctypes.data_as(_lib.p32), n_kmers, n_windows, lv,
                                             np.zeros(1, np.uint32).ctypes.data_as(_lib.p32)), "levels must be 1..4")
        refused(c, L.ac_hit_cooccurrence_device(h, p32(d), n_kmers, n_windows, 3, None, None), "output is NULL")
        refused(c, L.ac_hit_window_counts_device(h, p32(d), n_kmers, n_windows, 3, None, None), "output is NULL")
        refused(c, L.ac_hit_cooccurrence_device(h, None, n_kmers, n_windows, 3, p32(out), None), "hits is NULL")
        refused(c, L.ac_hit_window_counts_device(h, None, n_kmers, n_windows, 3, p32(wc), None), "hits is NULL")
        refused(c, L.ac_hit_cooccurrence(h, None, n_kmers, n_windows, 3, m.ctypes.data_as(_lib.p32)), "hits is NULL")
        torch.cuda.synchronize()
        assert bool((out == -1).all()) and bool((wc == -1).all()), "a refused call wrote"
        c.check()
        np.testing.assert_array_equal(device_cooc(c, d, n_kmers, n_windows, 3), want)
        np.testing.assert_array_equal(device_window_counts(c, d, n_kmers, n_windows, 3), hit.sum(axis=2))
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:
        d = torch.from_numpy(m.view(np.int32)).cuda()
        np.testing.assert_array_equal(device_cooc(multi, d, n_kmers, n_windows, 3), want)
        np.testing.assert_array_equal(multi.cooccurrence_host(m, n_kmers, n_windows, 3), want)


# ---- the command line -------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


def test_cli_cooccurrence(tmp_path):
    """The cfg1 FASTA with --seed 1 --cooccurrence --levels: the main files are byte for byte the golden ones;
    every .cooc line holds the main file's k-mer and n integers; the matrix is symmetric, its diagonal the last
    column of the .levels file, and it equals the product of the hits expected_hits derives from the sample
    --dump-sample writes with the same seed."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--cooccurrence", "--levels", "-o", "co"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        main = open(tmp_path / f"co_0.{end}").read()
        assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        rows = [ln.split("\t") for ln in main.splitlines()]
        co = [ln.split("\t") for ln in open(tmp_path / f"co_0.{end}.cooc").read().splitlines()]
        lv = [ln.split("\t") for ln in open(tmp_path / f"co_0.{end}.levels").read().splitlines()]
        n = len(rows)
        assert [a for a, _ in rows] == [x[0] for x in co] and all(len(x) == n + 1 for x in co)
        got = np.array([[int(v) for v in x[1:]] for x in co], np.uint32)
        np.testing.assert_array_equal(got, got.T)
        np.testing.assert_array_equal(np.diag(got), np.array([int(x[-1]) for x in lv], np.uint32))
        kmers = [cases.kmer_value(a) for a, _ in rows]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        assert n == 100 and len(wins) == 1000
        hit, _ = expected_hits(16, kmers, wins, 2)
        np.testing.assert_array_equal(got, gram(hit[2:3])[0])
