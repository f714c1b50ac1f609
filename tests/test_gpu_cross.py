"""GPU tests of the cross co-occurrence (ac_hit_cross_cooccurrence_device, ac_hit_cross_cooccurrence; DESIGN.md
§4e "Cross co-occurrence"): hit_cooc.hip's transposition of two matrices and hit_cross.hip's product kernel.
Expected values: numpy's product H_a^t H_b of the unpacked planes (in float32, which is exact below 2^24, so
that BLAS does it); every comparison is exact.

Every output buffer is filled with 0xFFFFFFFF before the call and followed by guard words of the same value: a
word the call did not define and a store past the end both show.  Input matrices have their stray bits set.

Which path a shape takes (hit_cross.h cx_splits, pinned by tests/test_cross_cpu.py::test_launch_rule): up to
2048 windows (one or two slabs of 1024) a workgroup takes its tile's whole window axis and stores every word
once.  From 2049 windows on the window axis is split over workgroups that add into the zeroed output -- 2049
(two workgroups a tile) and 5000 (three) -- unless the launch has 4096 workgroups without it: at four planes
32 x 31 tiles (2048 x 1984 candidates) are 3968, split, and 32 x 32 (2048 x 1985) are 4096, not."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.hits_cases import budget_case, expected_hits, pack_hits
from tests.positions_cases import FILL, GUARD
from tests.test_gpu_bitslice import BITSLICE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1
needs_hits = pytest.mark.skipif(not BS_ON, reason="AC_BITSLICE=0: no hits launch to take a matrix from")


def p32(t):
    return ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)


def cross(hit_a, hit_b):
    """uint32 (levels, n_a, n_b) of two bool (levels, n_windows, n)."""
    assert hit_a.shape[:2] == hit_b.shape[:2] and hit_a.shape[1] < 1 << 24
    return np.stack([a.T @ b for a, b in zip(hit_a.astype(np.float32), hit_b.astype(np.float32))]).astype(np.uint32)


def filled(n):
    import torch

    return torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")


def take(buf, n, shape, what):
    """The first n words of a filled buffer, after the guard check."""
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n:] == FILL).all(), f"{what}: a store past the end"
    return h[:n].reshape(shape).copy()


def device_cross(c, d_a, n_a, d_b, n_b, n_windows, levels):
    """ac_hit_cross_cooccurrence_device into a filled, guarded buffer: uint32 (levels, n_a, n_b)."""
    import torch

    n = levels * n_a * n_b
    out = filled(n)
    _lib.check(c._L.ac_hit_cross_cooccurrence_device(c.handle, p32(d_a), n_a, p32(d_b), n_b, n_windows, levels, p32(out),
                                                     None), c.handle)
    torch.cuda.synchronize()
    return take(out, n, (levels, n_a, n_b), "cross")


def device_cooc(c, d_hits, n_kmers, n_windows, levels):
    import torch

    n = levels * n_kmers * n_kmers
    out = filled(n)
    _lib.check(c._L.ac_hit_cooccurrence_device(c.handle, p32(d_hits), n_kmers, n_windows, levels, p32(out), None), c.handle)
    torch.cuda.synchronize()
    return take(out, n, (levels, n_kmers, n_kmers), "cooc")


DENSITY = (None, 0.5, 0.03, 0.2)  # plane 0 is all ones


def hand_built(n, n_windows, seed=0, levels=3):
    """(hit bool (levels, n_windows, n), matrix with stray bits): plane 0 all ones, 1 of density 0.5, 2 of 0.03
    (a fourth of 0.2)."""
    rng = np.random.default_rng(1000 * n + n_windows + 7919 * seed)
    hit = np.stack([np.ones((n_windows, n), bool) if p is None else rng.random((n_windows, n), dtype=np.float32) < p
                    for p in DENSITY[:levels]])
    m = pack_hits(hit)
    if n % 32:
        m[:, :, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return hit, m


def to_device(m):
    import torch

    return torch.from_numpy(m.view(np.int32)).cuda().reshape(-1)


def exact(got, want):
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} entries differ, first (plane, a, b) {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def check_hand_built(c, n_a, n_b, n_windows, levels=3):
    (ha, ma), (hb, mb) = hand_built(n_a, n_windows, 1, levels), hand_built(n_b, n_windows, 2, levels)
    da, db = to_device(ma), to_device(mb)
    got = device_cross(c, da, n_a, db, n_b, n_windows, levels)
    exact(got, cross(ha, hb))
    assert (got[0] == n_windows).all()
    c.check()
    return got, (ha, da), (hb, db)


# ---- hand-built matrices (no count launch: these run whatever AC_BITSLICE says) ---------------------------

SIDES = [1, 31, 32, 33, 64, 65, 129]


@pytest.mark.parametrize("n_a,n_b", [(n, 70) for n in SIDES] + [(70, n) for n in SIDES] + [(1, 300), (300, 1), (1, 1)])
def test_candidate_counts(counter, n_a, n_b):
    """Each side at one word and a partial one, one tile of 64 and a partial second (129: a third) against 70,
    and the lopsided shapes, at 257 windows.  All unsplit."""
    check_hand_built(counter, n_a, n_b, 257)


@pytest.mark.parametrize("n_windows", [1, 31, 32, 33, 64, 65, 1024, 1025, 2048, 2049, 5000])
def test_window_axis(counter, n_windows):
    """70 x 130 around a word of 32 windows, the transposition's 64 and a slab of 1024; 2048 | 2049: the last
    unsplit shape and the first split one; 5000: three workgroups a tile."""
    check_hand_built(counter, 70, 130, n_windows)


@pytest.mark.parametrize("n_b", [1984, 1985])
def test_the_workgroup_threshold(counter, n_b):
    """Four planes of 2049 windows, 2048 x n_b: 32 x 31 tiles are 3968 workgroups unsplit, so the window axis is
    split; 32 x 32 are 4096, so it is not."""
    check_hand_built(counter, 2048, n_b, 2049, levels=4)


def test_identities(counter):
    """cross(A, A) is the Gram call's result; cross(A, B) is cross(B, A) transposed; against B's all-ones plane
    every column is A's level counts.  One unsplit and one split shape."""
    import torch

    for n_a, n_b, n_windows in ((130, 70, 257), (70, 130, 2049)):
        got, (ha, da), (hb, db) = check_hand_built(counter, n_a, n_b, n_windows)
        np.testing.assert_array_equal(device_cross(counter, da, n_a, da, n_a, n_windows, 3), device_cooc(counter, da, n_a, n_windows, 3))
        np.testing.assert_array_equal(device_cross(counter, db, n_b, da, n_a, n_windows, 3), got.transpose(0, 2, 1))
        lc = counter.hit_level_counts(da, n_a, n_windows, 3)
        torch.cuda.synchronize()
        lc = lc.cpu().numpy().view(np.uint32)
        wa = (n_a + 31) // 32
        for e in range(3):
            ones = device_cross(counter, da[e * n_windows * wa:], n_a, db, n_b, n_windows, 1)[0]  # (B's plane 0)
            np.testing.assert_array_equal(ones, np.repeat(lc[e][:, None], n_b, axis=1))
        np.testing.assert_array_equal(counter.hit_cross_cooccurrence(da, n_a, db, n_b, n_windows, 3).cpu().numpy().view(np.uint32), got)
    counter.check()


def test_the_single_plane_idiom(counter):
    """Plane 2 of A against plane 0 of B, and A against itself at planes (0, 2), passed as the planes' offsets
    with levels = 1: numpy's product of those planes (unsplit and split)."""
    for n_a, n_b, n_windows in ((130, 70, 257), (70, 130, 5000)):
        (ha, ma), (hb, mb) = hand_built(n_a, n_windows, 1), hand_built(n_b, n_windows, 2)
        da, db = to_device(ma), to_device(mb)
        wa, wb = (n_a + 31) // 32, (n_b + 31) // 32
        got = device_cross(counter, da[2 * n_windows * wa:], n_a, db, n_b, n_windows, 1)
        exact(got, cross(ha[2:3], hb[0:1]))
        # (B's plane 0 is all ones: also two planes that both vary)
        got = device_cross(counter, da[1 * n_windows * wa:], n_a, db[2 * n_windows * wb:], n_b, n_windows, 1)
        exact(got, cross(ha[1:2], hb[2:3]))
        got = device_cross(counter, da, n_a, da[2 * n_windows * wa:], n_a, n_windows, 1)
        exact(got, cross(ha[0:1], ha[2:3]))
    counter.check()


# ---- the GPU's own matrices ---------------------------------------------------------------------------------

def paired_parts(seed, k, n_a, n_b, n_reads):
    """Two parts over paired windows: k-mer sets of n_a and n_b, window lists of the same n_reads reads -- their
    first 100 and last 101 bases, row w of both read w."""
    km_a, w_a = budget_case(seed, k, n_a, n_reads, 100, p_n=0.01)
    km_b, w_b = budget_case(seed + 1, k, n_b, n_reads, 101, p_n=0.01)
    return (km_a, w_a), (km_b, w_b)


def check_objects(r, k, E, a, b):
    ha, _ = expected_hits(k, a[0], a[1], E)
    hb, _ = expected_hits(k, b[0], b[1], E)
    assert ha[E].any() and hb[E].any()
    exact(r[0].cross_cooccurrence(r[1])[None], cross(ha[E:], hb[E:]))
    exact(r[0].cross_cooccurrence(r[1], 0, E)[None], cross(ha[0:1], hb[E:]))
    exact(r[1].cross_cooccurrence(r[0], 0, E)[None], cross(hb[0:1], ha[E:]))
    exact(r[0].cross_cooccurrence(r[0], 0, E)[None], cross(ha[0:1], ha[E:]))


@needs_hits
@pytest.mark.parametrize("E,k,n_a,n_b,n_reads", [(2, 16, 70, 33, 41), (3, 22, 33, 9, 37)])
def test_window_hits_objects_cross_on_the_device(E, k, n_a, n_b, n_reads):
    """One window_hits call with two parts over paired windows: r[0].cross_cooccurrence(r[1]) is numpy's product
    of the two parts' expected top levels, (0, E) of the bottom and top ones; the counter is attached, so the
    device path ran."""
    a, b = paired_parts(8400 + k, k, n_a, n_b, n_reads)
    with ac.ApproxCounter(0, max_errors=E) as c:
        r = c.window_hits(k, [(np.asarray(a[0], np.uint64), ac.pack_windows(a[1])),
                              (np.asarray(b[0], np.uint64), ac.pack_windows(b[1]))])
        assert r[0]._counter is c and r[1]._counter is c
        check_objects(r, k, E, a, b)
        c.check()


@needs_hits
def test_window_hits_jobs_objects_cross_on_the_device():
    """The same through window_hits_jobs (the jobs stage's Dna5 buffers)."""
    a, b = paired_parts(8416, 16, 70, 33, 41)
    with ac.ApproxCounter(0) as c:
        r = c.window_hits_jobs(16, [(np.asarray(a[0], np.uint64), a[1]), (np.asarray(b[0], np.uint64), b[1])])
        assert r[0]._counter is c and r[1]._counter is c
        check_objects(r, 16, 2, a, b)
        c.check()


# ---- the host-buffer call -------------------------------------------------------------------------------------

def test_host_buffers_and_scratch_growth():
    """ac_hit_cross_cooccurrence on 130 x 70 x 257 equals numpy and the device call; a larger shape (1000 x 600 x
    1100) on the same context, which grows both scratch blocks, is exact; so is the small one again, and a Gram
    call between them, which shares the scratch; n_windows = 0 is zeros; n_a = 0 leaves the buffer alone."""
    import torch

    with ac.ApproxCounter(0) as c:
        for n_a, n_b, n_windows in ((130, 70, 257), (1000, 600, 1100), (130, 70, 257)):
            (ha, ma), (hb, mb) = hand_built(n_a, n_windows, 1), hand_built(n_b, n_windows, 2)
            got = c.cross_cooccurrence_host(ma, n_a, mb, n_b, n_windows, 3)
            exact(got, cross(ha, hb))
            da, db = to_device(ma), to_device(mb)
            np.testing.assert_array_equal(got, device_cross(c, da, n_a, db, n_b, n_windows, 3))
            exact(device_cooc(c, db, n_b, n_windows, 3), cross(hb, hb))
            np.testing.assert_array_equal(got, device_cross(c, da, n_a, db, n_b, n_windows, 3))
        empty = np.zeros(0, np.uint32)
        zeros = c.cross_cooccurrence_host(empty, 130, empty, 70, 0, 3)
        assert zeros.shape == (3, 130, 70) and not zeros.any()
        assert not device_cross(c, None, 130, None, 70, 0, 3).any()
        out = filled(64)
        _lib.check(c._L.ac_hit_cross_cooccurrence_device(c.handle, p32(da), 0, p32(db), n_b, n_windows, 3, p32(out), None), c.handle)
        _lib.check(c._L.ac_hit_cross_cooccurrence_device(c.handle, p32(da), n_a, p32(db), 0, n_windows, 3, p32(out), None), c.handle)
        torch.cuda.synchronize()
        assert bool((out == -1).all()), "a call without work wrote"
        assert c.cross_cooccurrence_host(empty, 0, mb, n_b, n_windows, 3).shape == (3, 0, n_b)
        c.check()


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """levels 0 and 5, a NULL output and a NULL matrix on either side: AC_ERR_INVALID naming the constraint,
    nothing enqueued (the buffer keeps its fill, the device error word stays clean), and a following call is exact;
    a two-device context computes on its first device."""
    import torch

    n_a, n_b, n_windows = 70, 40, 300
    (ha, ma), (hb, mb) = hand_built(n_a, n_windows, 1), hand_built(n_b, n_windows, 2)
    want = cross(ha, hb)
    host = lambda m: m.ctypes.data_as(_lib.p32)  # noqa: E731

    def refused(c, status, word):
        assert status == _lib.AC_ERR_INVALID
        msg = c._L.ac_last_error(c.handle).decode()
        assert word in msg, msg

    with ac.ApproxCounter(0) as c:
        L, h = c._L, c.handle
        da, db = to_device(ma), to_device(mb)
        out = filled(3 * n_a * n_b)
        h_out = np.full(3 * n_a * n_b, FILL, np.uint32)
        for lv in (0, 5):
            refused(c, L.ac_hit_cross_cooccurrence_device(h, p32(da), n_a, p32(db), n_b, n_windows, lv, p32(out), None), "levels must be 1..4")
            refused(c, L.ac_hit_cross_cooccurrence(h, host(ma), n_a, host(mb), n_b, n_windows, lv, host(h_out)), "levels must be 1..4")
            refused(c, L.ac_testing_hit_cross_stages(h, p32(da), n_a, p32(db), n_b, n_windows, lv, p32(out), 3, None), "levels must be 1..4")
        refused(c, L.ac_hit_cross_cooccurrence_device(h, p32(da), n_a, p32(db), n_b, n_windows, 3, None, None), "output is NULL")
        refused(c, L.ac_hit_cross_cooccurrence(h, host(ma), n_a, host(mb), n_b, n_windows, 3, None), "output is NULL")
        refused(c, L.ac_hit_cross_cooccurrence_device(h, None, n_a, p32(db), n_b, n_windows, 3, p32(out), None), "hits_a is NULL")
        refused(c, L.ac_hit_cross_cooccurrence_device(h, p32(da), n_a, None, n_b, n_windows, 3, p32(out), None), "hits_b is NULL")
        refused(c, L.ac_hit_cross_cooccurrence(h, None, n_a, host(mb), n_b, n_windows, 3, host(h_out)), "hits_a is NULL")
        refused(c, L.ac_hit_cross_cooccurrence(h, host(ma), n_a, None, n_b, n_windows, 3, host(h_out)), "hits_b is NULL")
        refused(c, L.ac_testing_hit_cross_stages(h, p32(da), n_a, p32(db), n_b, n_windows, 3, p32(out), 0, None), "stages must be 1..3")
        assert L.ac_hit_cross_cooccurrence_device(None, p32(da), n_a, p32(db), n_b, n_windows, 3, p32(out), None) == _lib.AC_ERR_INVALID
        assert b"ctx is NULL" in L.ac_last_error(None)
        torch.cuda.synchronize()
        assert bool((out == -1).all()) and (h_out == FILL).all(), "a refused call wrote"
        c.check()
        exact(device_cross(c, da, n_a, db, n_b, n_windows, 3), want)
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:
        da, db = to_device(ma), to_device(mb)
        exact(device_cross(multi, da, n_a, db, n_b, n_windows, 3), want)
        exact(multi.cross_cooccurrence_host(ma, n_a, mb, n_b, n_windows, 3), want)


# ---- the command line -------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


def test_cli_cross_cooccurrence(tmp_path):
    """The cfg1 FASTA with --seed 1 --paired-sample --cross-cooccurrence --levels (-sn covers every read, so the
    paired sample is the same set of reads): the main files are byte for byte the golden ones; cx_0.cross holds
    one line per .start k-mer in its order, the k-mer and one integer per .end k-mer; its matrix is the product
    of the hits expected_hits derives from the two images --dump-sample --paired-sample writes with the same seed,
    in the files' k-mer orders."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1",
            "--paired-sample"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--cross-cooccurrence", "--levels", "-o", "cx"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    kmers, hit = {}, {}
    for end in ("start", "end"):
        main = open(tmp_path / f"cx_0.{end}").read()
        assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
        kmers[end] = [ln.split("\t")[0] for ln in main.splitlines()]
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        assert len(kmers[end]) == 100 and len(wins) == 1000
        hit[end], _ = expected_hits(16, [cases.kmer_value(a) for a in kmers[end]], wins, 2)
    cx = [ln.split("\t") for ln in open(tmp_path / "cx_0.cross").read().splitlines()]
    assert [x[0] for x in cx] == kmers["start"] and all(len(x) == 1 + len(kmers["end"]) for x in cx)
    got = np.array([[int(v) for v in x[1:]] for x in cx], np.uint32)
    exact(got[None], cross(hit["start"][2:3], hit["end"][2:3]))
    assert got.any()
