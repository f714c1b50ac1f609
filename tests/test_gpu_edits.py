"""GPU tests of the edit profiles (ac_hit_edit_profile_device, ac_window_edits_samples; DESIGN.md §4e "Edit
profiles"): the edit pass (hit_edit.hip) after count_device(..., spans=), alone over hand-built planes, behind
window_hits(..., edits=True) with and without flanks=, and behind the command line's --edits.  Expected values:
tests/edit_cases.edit_profile_of -- the definition as a plain full-table DP with its traceback over the window
strings and the matrices of tests/span_cases.expected_spans.

Every device output is filled with 0xFFFFFFFF before the call and followed by guard words of the same value,
and is compared word for word: a word the pass did not define and a store past the result both show.  Every
plane given to the pass holds ends and starts inside the window; hostile planes are for the sanitised host tool
(tests/test_edits_cpu.py)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.edit_cases import edit_matrices, edit_profile_of, pack_hits, pack_positions, pack_starts
from tests.flank_cases import flank_profile_of
from tests.hits_cases import FILL, GUARD
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_bitslice import BITSLICE, kernel_of
from tests.test_gpu_positions import refused, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1
CHUNK = 128    # windows of a chunk (hit_edit.hip EP_CHUNK): a strip is whole chunks
BLOCKS = 1024  # workgroups a launch aims at (EP_BLOCKS): at most BLOCKS / word columns strips
NAMES = "(k-mer, base, operation)"


@pytest.fixture(scope="module")
def ctxs():
    """One context per edit budget used here (the budget is sticky; the session's `counter` stays at 2)."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (2, 3)}
    yield made
    for c in made.values():
        c.close()


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def edit_pass(c, k, seg, L, plane, pos_m, start_m, n_kmers, n_windows, out=None):
    """ac_hit_edit_profile_device over device tensors: the profile (n_kmers, k, 12), guards asserted."""
    import torch

    n = ac.edit_words(n_kmers, k)
    if out is None:
        out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    c.hit_edit_profile(k, seg.kmers, n_kmers, seg, L, plane, pos_m, start_m, n_windows, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "a store past the profile"
    return got[:n].reshape(n_kmers, k, 12)


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


def trimmed(case, n_kmers, n_windows):
    """The first n_kmers k-mers and n_windows windows of an edit_matrices case."""
    km, w, hit, pos, start, _ = case
    assert len(km) >= n_kmers and len(w) >= n_windows
    return km[:n_kmers], w[:n_windows], hit[:, :n_windows, :n_kmers], pos[:n_windows, :n_kmers], start[:n_windows, :n_kmers]


def every_route(c, k, km, w, hit, pos, start, what):
    """The pass after the real count launch and span pass (count_device with the planes, then
    hit_edit_profile), and window_hits(edits=True) without and with flanks=8: all equal to the definition."""
    E, L, nk = c.max_errors, len(w[0]), len(km)
    assert hit.shape[0] == E + 1
    want = edit_profile_of(k, km, w, hit[E], pos, start)
    assert want[:, :, 0].any() and (E == 0 or want[:, :, 1:].any())
    seg, hb, pb, sb = device_matrices(c, k, km, w, hit, pos, start)
    top = hb[E * len(w) * ((nk + 31) // 32):]  # the top level plane
    same(edit_pass(c, k, seg, L, top, pb, sb, nk, len(w)), want, (what, "the pass"), NAMES)
    img = [(km, ac.pack_windows(list(w)))]
    if not BS_ON:
        refused(lambda: c.window_hits(k, img, edits=True))
        return seg, hb, pb, sb
    for D in (0, 8):
        wh = c.window_hits(k, img, flanks=D, edits=True)[0]
        assert kernel_of(c) == 1
        same(wh.levels, pack_hits(hit), "levels", "(level, window, word)")
        same(wh.planes, pack_positions(pos), "positions", "(plane, window, word)")
        same(wh.starts, pack_starts(start, hit[E]), "starts", "(plane, window, word)")
        prof = wh.edit_profile()
        assert prof.dtype == np.uint32
        same(prof, want, (what, "samples", D), NAMES)
        if D:
            same(wh.flank_profile(), flank_profile_of(w, hit[E], pos, start, D), (what, "flanks beside edits"),
                 "(side, k-mer, column, symbol)")
        else:
            with pytest.raises(ValueError, match="flanks="):
                wh.flank_profile()
    return seg, hb, pb, sb


# ---- every route, after the launch ------------------------------------------------------------------

@pytest.mark.parametrize("k,E", [(16, 2), (22, 2), (32, 2), (32, 3)])
def test_every_route(ctxs, k, E):
    """40 k-mers x (30 + plants + 30 + 6 with an N in the occurrence) windows x 100 bases.  k = 32 at E = 3: texts
    of 33..35 bases, past the first 32-base run of codes."""
    km, w, hit, pos, start, _ = edit_matrices(15000 + 10 * k + E, k, 40, 30, 100, E)
    if (k, E) == (32, 3):
        assert ((pos - start)[hit[E]] > 32).any()
    every_route(ctxs[E], k, km, w, hit, pos, start, (k, E))


@pytest.mark.parametrize("n_kmers,L,n_windows", [(33, 33, 129), (40, 100, 257), (40, 256, 129), (33, 100, 257)])
def test_shapes(ctxs, n_kmers, L, n_windows):
    """A partial last word column (33 and 40 k-mers), windows of 33, 100 and 256 bases, and one window past one
    and two chunks of 128."""
    case = edit_matrices(15100 + L, 16, 40, (n_windows + 1) // 2, L, 2)
    km, w, hit, pos, start = trimmed(case, n_kmers, n_windows)
    every_route(ctxs[2], 16, km, w, hit, pos, start, (n_kmers, L, n_windows))


def test_spans_alone_gives_no_profile(ctxs):
    km, w, *_ = edit_matrices(15000 + 10 * 16 + 2, 16, 40, 30, 100, 2)
    if not BS_ON:
        refused(lambda: ctxs[2].window_hits(16, [(km, ac.pack_windows(list(w)))], edits=True))
        return
    with pytest.raises(ValueError, match="edits="):
        ctxs[2].window_hits(16, [(km, ac.pack_windows(list(w)))], spans=True)[0].edit_profile()
    empty = (km[:5], ac.pack_windows([]))
    got = ctxs[2].window_hits(16, [(km, ac.pack_windows(list(w))), empty], edits=True)
    assert got[1].edit_profile().shape == (5, 16, 12) and not got[1].edit_profile().any() and not got[1].counts.any()
    assert got[0].edit_profile().any()
    ctxs[2].check()


# ---- the pass alone ---------------------------------------------------------------------------------

def planted_planes(seed, k, n_kmers, n_windows, L, every=1):
    """Hand-built planes: random windows (2 % N) and random k-mers; every `every`-th window (and the last)
    holds one k-mer with up to 3 edits, one of them an N at times, and the pair's bit, end and start say where:
    at base 0, ending at base L, across a 16-base code word's seam, across a 32-base bitmap word's seam, or
    anywhere.  Ends and starts are inside the window.  Returns (kmers, windows, hit, pos, start)."""
    rng = random.Random(seed)
    km = np.array(rng.sample(range(1 << min(2 * k, 62)), n_kmers), np.uint64)
    w = [cases.rand_seq(rng, L, 0.02) for _ in range(n_windows)]
    hit = np.zeros((n_windows, n_kmers), bool)
    pos, start = np.full(hit.shape, -1), np.full(hit.shape, -1)
    at_windows = sorted(set(range(0, n_windows, every)) | {n_windows - 1})
    for n, wi in enumerate(at_windows):
        c = rng.randrange(n_kmers)
        t = cases.mutate(rng, cases.kmer_string(int(km[c]), k), rng.randint(0, 2))
        if n % 5 == 0 and len(t) > 2:
            x = rng.randrange(1, len(t) - 1)
            t = t[:x] + "N" + t[x + (n % 2):]  # (substituted or inserted)
        else:
            t = cases.mutate(rng, t, rng.randint(0, 1))
        t = t[:L]
        m = len(t)
        mode = n % 5
        s = (0 if mode == 0 else L - m if mode == 1 else 16 * rng.randint(1, max((L - m) // 16, 1)) - m // 2 if mode == 2
             else 32 * rng.randint(1, max((L - m) // 32, 1)) - m // 2 if mode == 3 else rng.randint(0, L - m))
        s = min(max(s, 0), L - m)
        w[wi] = w[wi][:s] + t + w[wi][s + m:]
        hit[wi, c], pos[wi, c], start[wi, c] = True, s + m, s
    return km, w, hit, pos, start


def planted_pass(c, seed, k, n_kmers, n_windows, L, every=1, least=100):
    km, w, hit, pos, start = planted_planes(seed, k, n_kmers, n_windows, L, every)
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    got = edit_pass(c, k, seg, L, cuda(pack_hits(hit[None])[0]), cuda(pack_positions(pos)), cuda(pack_starts(start, hit)),
                    n_kmers, n_windows)
    want = edit_profile_of(k, km, w, hit, pos, start)
    assert want[:, :, 0].sum() > least and (n_windows < 8 or want[:, :, 1:].any())
    same(got, want, (k, n_kmers, n_windows, L), NAMES)
    return hit, pos, start


@pytest.mark.parametrize("k,L", [(16, 100), (32, 70), (5, 33), (17, 256)])
def test_pass_alone_at_the_edges_and_seams(counter, k, L):
    """Occurrences that start at base 0, end at base L and lie across the 16-base and 32-base word seams, at a k
    no count kernel has as well: the pass runs at any k, on any context."""
    hit, pos, start = planted_pass(counter, 15200 + k, k, 40, 200, L)
    p, s = pos[hit], start[hit]
    assert (s == 0).any() and (p == L).any()
    assert ((s // 16 < (p - 1) // 16) & (s % 16 > 0)).any() and ((s // 32 < (p - 1) // 32) & (s % 32 > 0)).any()


@pytest.mark.parametrize("n_windows", [1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges(counter, n_windows):
    """One window, exactly a chunk, one past it and one past two (every strip one chunk here: the strips' edges
    fall inside the window range), at one and at three word columns."""
    for n_kmers in (20, 70):
        planted_pass(counter, 15300 + n_windows, 16, n_kmers, n_windows, 60, least=min(n_windows, 100))


def test_strips_of_two_chunks(counter):
    """Two word columns get at most 512 strips: 512 chunks and one window more make every strip two chunks (257
    strips, the last of one window); a hit in every 16th window and in the last."""
    planted_pass(counter, 15400, 16, 40, CHUNK * BLOCKS // 2 + 1, 33, every=16)


def test_lower_plane_no_windows_no_kmers_and_twice(ctxs):
    """Plane 0 of an E = 2 matrix: the exact occurrences alone.  n_windows = 0 writes zeros; n_kmers = 0 touches
    nothing.  Two calls into one buffer on one context give the same: the launch zeroes the output."""
    import torch

    c, E, k, nk = ctxs[2], 2, 16, 40
    km, w, hit, pos, start, _ = edit_matrices(15000 + 10 * k + E, k, nk, 30, 100, E)
    seg, hb, pb, sb = device_matrices(c, k, km, w, hit, pos, start)
    plane_words = len(w) * 2
    got = edit_pass(c, k, seg, 100, hb[:plane_words], pb, sb, nk, len(w))
    want0 = edit_profile_of(k, km, w, hit[0], pos, start)
    assert want0[:, :, 0].any() and not want0[:, :, 1:].any()
    same(got, want0, "plane 0", NAMES)
    want = edit_profile_of(k, km, w, hit[E], pos, start)
    out = torch.full((ac.edit_words(nk, k) + GUARD,), -1, dtype=torch.int32, device="cuda")
    for n in range(2):
        same(edit_pass(c, k, seg, 100, hb[E * plane_words:], pb, sb, nk, len(w), out=out), want, f"call {n}", NAMES)
    # the first 31 windows of the image, through n_windows: planes of that shape
    sub = slice(0, 31)
    got = edit_pass(c, k, seg, 100, cuda(pack_hits(hit[:, sub])[E]), cuda(pack_positions(pos[sub])),
                    cuda(pack_starts(start[sub], hit[E][sub])), nk, 31)
    same(got, edit_profile_of(k, km, w[:31], hit[E][sub], pos[sub], start[sub]), "31 windows", NAMES)
    z = torch.full((ac.edit_words(nk, k) + GUARD,), -1, dtype=torch.int32, device="cuda")
    c.hit_edit_profile(k, seg.kmers, nk, seg, 100, None, None, None, 0, out=z)
    torch.cuda.synchronize()
    z = z.cpu().numpy()
    assert not z[:-GUARD].any() and (z[-GUARD:] == -1).all()
    z = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    c.hit_edit_profile(k, None, 0, seg, 100, None, None, None, len(w), out=z)
    torch.cuda.synchronize()
    assert bool((z == -1).all())
    c.check()


# ---- refusals ---------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Every refusal of ac_hit_edit_profile_device: AC_ERR_INVALID naming the constraint, nothing enqueued (the
    output keeps its fill), each followed by a correct call on the same context; then ac_window_edits_samples'
    own."""
    import torch

    k, E, L = 17, 2, 60
    km, w, hit, pos, start, _ = edit_matrices(16000, k, 40, 12, L, E)
    nw = len(w)
    want = edit_profile_of(k, km, w, hit[E], pos, start)
    with ac.ApproxCounter(0) as c:
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
        hb, pb, sb = cuda(pack_hits(hit)[E]), cuda(pack_positions(pos)), cuda(pack_starts(start, hit[E]))
        out = torch.full((ac.edit_words(40, 32),), -1, dtype=torch.int32, device="cuda")

        def good():
            torch.cuda.synchronize()
            assert bool((out == -1).all()), "a refused call wrote"
            c.check()
            same(edit_pass(c, k, seg, L, hb, pb, sb, 40, nw), want, "after a refusal", NAMES)

        def call(kk=k, km_=seg.kmers, sample=seg, wl=L, h=hb, p=pb, s=sb, n=nw, o=out):
            return lambda: c.hit_edit_profile(kk, km_, 40, sample, wl, h, p, s, n, out=o)

        short = seg.as_struct().sample
        short.n_bases = nw * 64 - 32  # (the windows at 64-base strides do not fit)
        no_codes, no_nmask = seg.as_struct().sample, seg.as_struct().sample
        no_codes.codes = None
        no_nmask.nmask = None
        for fn, word in ((call(kk=1), "k must be 2..32"), (call(kk=33), "k must be 2..32"),
                         (call(wl=0), "window_len must be 1..256"), (call(wl=257), "window_len must be 1..256"),
                         (call(sample=short), "do not fit n_bases"),
                         (call(km_=None), "kmers is NULL"),
                         (call(h=None), "hit_plane, pos or start is NULL"), (call(p=None), "hit_plane, pos or start is NULL"),
                         (call(s=None), "hit_plane, pos or start is NULL"),
                         (call(sample=no_codes), "codes or nmask is NULL"), (call(sample=no_nmask), "codes or nmask is NULL")):
            assert word in refused(fn, "edit profile"), word
            good()
        L_ = _lib.load()
        ws = seg.as_struct().sample
        p32 = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
        kp = ctypes.cast(ctypes.c_void_p(seg.kmers.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
        st = L_.ac_hit_edit_profile_device(c.handle, k, kp, 40, ctypes.byref(ws), L, p32(hb), p32(pb), p32(sb), None, None)
        assert st == _lib.AC_ERR_INVALID and b"the output is NULL" in L_.ac_last_error(c.handle)
        st = L_.ac_hit_edit_profile_device(c.handle, k, kp, 40, None, L, p32(hb), p32(pb), p32(sb), p32(out), None)
        assert st == _lib.AC_ERR_INVALID and b"sample is NULL" in L_.ac_last_error(c.handle)
        assert L_.ac_hit_edit_profile_device(None, k, kp, 40, ctypes.byref(ws), L, p32(hb), p32(pb), p32(sb), p32(out),
                                             None) == _lib.AC_ERR_INVALID
        good()
        # the samples route: what ac_window_flanks_samples refuses (but a depth of 0), and a NULL profile
        if BS_ON:
            a = edit_matrices(16001, 16, 40, 12, 100, 2)
            ragged = cases.planted_case(16002, 16, 40, 30, win_len=(90, 110))
            imgs = [(a[0], ac.pack_windows(list(a[1]))), (np.asarray(ragged[0], np.uint64), ac.pack_windows(ragged[1]))]
            assert "ragged" in refused(lambda: c.window_hits(16, imgs, edits=True))
            assert "16 or 18..32" in refused(lambda: c.window_hits(17, [(km, ac.pack_windows(list(w)))], edits=True))
            assert "depth must be" in refused(lambda: c.window_hits(16, imgs[:1], flanks=33, edits=True), "flank profile")
            dev = c.upload_sample(imgs[0][1], 0)
            cnt = np.zeros(40, np.uint64)
            u64 = ctypes.POINTER(ctypes.c_uint64)
            job = (_lib.ACSampleJob * 1)(_lib.ACSampleJob(a[0].ctypes.data_as(u64), 40, dev, cnt.ctypes.data_as(u64)))
            n1 = len(a[1])
            hm = np.full(ac.hits_words(40, n1, 2), FILL, np.uint32)
            pm, sm = (np.full(ac.positions_words(40, n1), FILL, np.uint32) for _ in range(2))
            em = np.full(ac.edit_words(40, 16), FILL, np.uint32)
            one32 = lambda x: (_lib.p32 * 1)(x.ctypes.data_as(_lib.p32) if x is not None else None)  # noqa: E731
            args = (one32(hm), one32(pm), one32(sm))
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 0, *args, None, one32(None)) == _lib.AC_ERR_INVALID
            assert b"edit_host[j] is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 0, *args, None, None) == _lib.AC_ERR_INVALID
            assert b"edit_host is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 8, *args, None, one32(em)) == _lib.AC_ERR_INVALID
            assert b"flank_host is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 8, *args, one32(None), one32(em)) == _lib.AC_ERR_INVALID
            assert b"flank_host[j] is NULL" in L_.ac_last_error(c.handle)
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 33, *args, one32(hm), one32(em)) == _lib.AC_ERR_INVALID
            assert b"depth must be" in L_.ac_last_error(c.handle)
            assert all((m == FILL).all() for m in (hm, pm, sm, em)), "a refused call wrote"
            # a depth of 0 with no flank buffer: the edits alone
            assert L_.ac_window_edits_samples(c.handle, 16, job, 1, 0, *args, None, one32(em)) == _lib.AC_OK
            same(em.reshape(40, 16, 12), edit_profile_of(16, a[0], a[1], a[2][2], a[3], a[4]), "after the refusals", NAMES)
        good()
    with ac.ApproxCounter(n_gpus=2) as multi:  # (an ac_create_multi context uses its first device)
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(list(w)))
        same(edit_pass(multi, k, seg, L, hb, pb, sb, 40, nw), want, "multi", NAMES)


# ---- the command line -------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")


def test_cli_edits(tmp_path):
    """The cfg1 FASTA with --seed 1 --levels --positions --spans --flanks 8, without and with --edits: the other
    output files are byte for byte the same (the main files the golden ones); every .edits line holds the main
    file's k-mer and 16 groups of 12 counts, equal to the profile derived from the sample --dump-sample writes
    with the same seed and to the Python route's over that sample."""
    from tests.span_cases import expected_spans
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1"]
    others = ["--levels", "--positions", "--spans", "--flanks", "8"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(others + ["--edits", "-o", "ed"])
    if not BS_ON:
        assert r.returncode == 1 and "window hits need" in r.stderr and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(others + ["-o", "no"]).returncode == 0
    assert run(["--edits", "-o", "alone", "-v", "0"]).returncode == 0
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    with ac.ApproxCounter(0) as c:
        for end in ("start", "end"):
            main = open(tmp_path / f"ed_0.{end}").read()
            assert main == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
            for ext in ("", ".levels", ".positions", ".starts", ".lengths", ".flanks"):
                assert open(tmp_path / f"ed_0.{end}{ext}", "rb").read() == open(tmp_path / f"no_0.{end}{ext}", "rb").read(), ext
            assert not os.path.exists(tmp_path / f"no_0.{end}.edits")
            assert not os.path.exists(tmp_path / f"alone_0.{end}.flanks")  # (the flag alone writes its own file only)
            text = open(tmp_path / f"ed_0.{end}.edits").read()
            assert text == open(tmp_path / f"alone_0.{end}.edits").read()
            rows = [ln.split("\t") for ln in main.splitlines()]
            table = [ln.split("\t") for ln in text.splitlines()]
            assert [x[0] for x in table] == [a for a, _ in rows] and all(len(x) == 16 + 1 for x in table)
            kmers = [cases.kmer_value(a) for a, _ in rows]
            wins = decode(load_image(tmp_path / f"smp_0.{end}"))
            assert len(kmers) == 100 and len(wins) == 1000
            got = np.array([[[int(v) for v in g.split(",")] for g in x[1:]] for x in table], np.uint32)  # (k-mer, 16, 12)
            wh = c.window_hits(16, [(np.array(kmers, np.uint64), ac.pack_windows(wins))], edits=True)[0]
            np.testing.assert_array_equal(got, wh.edit_profile())
            hit, pos, start, _, _ = expected_spans(16, kmers, wins, 2)
            want = edit_profile_of(16, kmers, wins, hit[2], pos, start)
            np.testing.assert_array_equal(got, want)
            assert want[:, :, 0].any() and want[:, :, 1:].any()
