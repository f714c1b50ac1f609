"""GPU tests of mixed call sequences on one context (DESIGN.md §4e "Call sequences"): the walk of
tests/sequence_cases.py -- every launch kind directly after every launch kind, with side operations, refusals,
empty calls, budget changes and slot re-uploads between them -- run segment by segment on one context, and again
with a fresh context per segment.  A bug that needs a long history fails only the shared-context tests; a plain bug
fails both.

Every result is compared bit for bit with the expected values sequence_cases caches per shape.  Every device output
is filled with 0xFFFFFFFF and followed by GUARD words of it first.  After every launch the test asserts which kernel
ran, the stage mode where the kind fixes it, and the candidate groups tests/test_sequence_cases.py predicted: guards
that the walk reached what it set out to reach.  After every refusal: AC_ERR_INVALID, a message that names the
constraint, the filled buffers untouched, and a clean check().

The span, flank and edit passes are in the walk three ways: the `profiles` kind (window_hits(spans= / flanks= /
edits=), whose per-job matrices and profiles the context carves out of grow-only blocks), every other `pos` visit
(count_device(..., spans=)), and side operations that run each pass alone over the matrices the last hits launch
left, with start positions from the CPU reference.

With AC_BITSLICE=0 in the environment no launch is bit-sliced: the hits kinds and every launch at a budget other
than 2 are then refusals themselves, and the rest of the walk still runs."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import sequence_cases as sc
from tests.hits_cases import FILL, GUARD, pack_hits
from tests.positions_cases import pack_positions, profile_of
from tests.test_gpu_bitslice import AC_TESTING_DEVICE_PACK, BITSLICE, hooks, kernel_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")
BS_ON = BITSLICE == 1
AC_TESTING_TWO_PARTS = 16
EARLY = os.environ.get("AC_STAGE_EARLY", "1") != "0"  # (the child of the DMA route runs with 0)


def p32(t):
    return ctypes.cast(ctypes.c_void_p(t.data_ptr() if t is not None else 0), _lib.p32)


def filled(n):
    import torch

    return torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")


def take(buf, n, shape, what):
    """The first n words of a filled buffer, after the guard check."""
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n:] == FILL).all(), f"{what}: a store past the end"
    return h[:n].reshape(shape).copy()


def untouched(bufs):
    import torch

    torch.cuda.synchronize()
    return all(b is None or bool((b == -1).all()) for b in bufs)


def to_device(m):
    import torch

    return torch.from_numpy(np.ascontiguousarray(m).view(np.int32)).cuda().reshape(-1)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} values differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def refused(c, fn, word, bufs=()):
    """A refusal: AC_ERR_INVALID naming the constraint, the filled buffers untouched, check() clean."""
    before = (kernel_of(c), c.last_launch(), c.max_errors)
    with pytest.raises(_lib.ApproxCounterError) as e:
        fn()
    assert e.value.status == _lib.AC_ERR_INVALID, e.value
    assert word in str(e.value), e.value
    assert untouched(bufs), f"a refused call wrote ({word})"
    c.check()
    assert (kernel_of(c), c.last_launch(), c.max_errors) == before


def raw_refused(c, status, word, bufs=()):
    assert status == _lib.AC_ERR_INVALID, status
    msg = c._L.ac_last_error(c.handle).decode()
    assert word in msg, msg
    assert untouched(bufs), f"a refused call wrote ({word})"
    c.check()


def device_segment(shape, j):
    km, w = sc.case(shape, j)
    return ac.DeviceSegment.upload(km, ac.pack_windows(w))


def host_buffers(c, k, km, smp, D):
    """The host matrices and profiles of one job of ac_window_*_samples, each filled and GUARD words longer."""
    nk, nw = len(km), smp.n_windows
    sizes = {"hits": ac.hits_words(nk, nw, c.max_errors), "pos": ac.positions_words(nk, nw),
             "start": ac.positions_words(nk, nw), "flank": ac.flank_words(nk, D), "edit": ac.edit_words(nk, k)}
    return {name: np.full(n + GUARD, FILL, np.uint32) for name, n in sizes.items()}


def raw_window_profiles(c, k, parts, packed, D, edits):
    """upload_sample into slot j, then the entry point window_hits(spans= / flanks= / edits=) calls, over host
    buffers of 0xFFFFFFFF with GUARD words more: (status, [counts per job], [host_buffers per job])."""
    u64 = ctypes.POINTER(ctypes.c_uint64)
    kms, counts, bufs, jobs = [], [], [], []
    for slot, ((km, _), smp) in enumerate(zip(parts, packed)):
        km = np.ascontiguousarray(km, np.uint64)
        kms.append(km if km.size else np.zeros(1, np.uint64))
        counts.append(np.full(km.size + 1, 0xFFFFFFFFFFFFFFFF, np.uint64))
        bufs.append(host_buffers(c, k, km, smp, D))
        jobs.append(_lib.ACSampleJob(kms[-1].ctypes.data_as(u64), km.size, c.upload_sample(smp, slot),
                                     counts[-1].ctypes.data_as(u64)))
    arr = (_lib.ACSampleJob * len(jobs))(*jobs)
    ptrs = lambda name: (_lib.p32 * len(jobs))(*[b[name].ctypes.data_as(_lib.p32) for b in bufs])  # noqa: E731
    mats = (ptrs("hits"), ptrs("pos"), ptrs("start"))
    if edits:
        st = c._L.ac_window_edits_samples(c.handle, k, arr, len(jobs), D, *mats, ptrs("flank") if D else None, ptrs("edit"))
    elif D:
        st = c._L.ac_window_flanks_samples(c.handle, k, arr, len(jobs), D, *mats, ptrs("flank"))
    else:
        st = c._L.ac_window_spans_samples(c.handle, k, arr, len(jobs), *mats)
    return st, counts, bufs


class Run:
    """One context's walk: the context, and what the side operations read -- the hit matrices the last hits or
    positions launch left (before any: HIT_SHAPES[0] at E = 2, uploaded from the host), the k-mers and window
    image of that job on the device, and the sample last uploaded into slot 0."""

    def __init__(self, c, two_parts=False):
        self.c, self.two_parts, self.jobs_calls = c, two_parts, 0
        hit, pos, _ = sc.expected_matrices(sc.HIT_SHAPES[0], 0, 2)
        self.mat = (sc.HIT_SHAPES[0], 0, 2, to_device(pack_hits(hit)), to_device(pack_positions(pos)))
        self.seg = device_segment(sc.HIT_SHAPES[0], 0)
        self.uploaded = (sc.SAMPLE_STATES[0], 0)

    # ---- launches ----

    def parts(self, v):
        return [sc.case(v.shape, j) for j in range(len(v.shape.jobs))]

    def keep(self, v, d_hits, d_pos):
        """The first live job's matrices are what the reductions read next (positions the launch did not write
        come from the expected ones), with its k-mers and windows on the device for the span, flank and edit
        passes."""
        j = next(i for i, x in enumerate(v.shape.jobs) if sc.live(x))
        pos = d_pos[j] if d_pos is not None else to_device(pack_positions(sc.expected_matrices(v.shape, j, v.E)[1]))
        self.mat = (v.shape, j, v.E, d_hits[j], pos)
        self.seg = device_segment(v.shape, j)

    def reached(self, v, kernel, mode=None, groups=True):
        c = self.c
        assert kernel_of(c) == kernel, (v, kernel_of(c))
        if mode is not None:
            assert c.stage_mode() == mode, (v, c.stage_mode(), mode)
        if groups:
            want = sc.launch_groups(v.kind, v.shape, early=EARLY, bs_on=BS_ON)[1]
            assert c.last_launch()["groups"] == want, (v, c.last_launch(), want)

    def compare_matrices(self, v, j, counts, levels, planes):
        hit, pos, want = sc.expected_matrices(v.shape, j, v.E)
        same(levels, pack_hits(hit), (v.kind, v.n, j, "hit words"))
        if planes is not None:
            same(planes, pack_positions(pos), (v.kind, v.n, j, "position words"))
        same(counts, want, (v.kind, v.n, j, "counts"))

    def hooks_for(self, v):
        flags = AC_TESTING_DEVICE_PACK if v.kind == "dp_jobs" else 0
        if self.two_parts and self.jobs_calls % 2:
            flags |= AC_TESTING_TWO_PARTS
        self.jobs_calls += 1
        return flags

    def refused_launch(self, v, fn, bufs=()):
        """AC_BITSLICE=0: a hits kind names the switch; another launch at a budget other than 2 names the budget."""
        hits = v.kind in sc.HIT_KINDS or v.with_hits
        refused(self.c, fn, "AC_BITSLICE" if hits else "max_errors", bufs)

    def launch(self, v):
        getattr(self, "launch_" + ("device" if v.kind in ("wm", "bs", "hits", "pos") else v.kind))(v)

    def launch_device(self, v):
        """wm, bs, hits, pos: count() or count_device over resident images."""
        import torch

        c, k, parts = self.c, v.shape.k, self.parts(v)
        if v.kind == "wm" and len(parts) == 1 and v.nth % 2 == 0:
            got = c.count(k, parts[0][0], ac.pack_windows(parts[0][1]))
            self.reached(v, 0)
            same(got, sc.expected_counts(v.shape, 0, v.E), (v.kind, v.n, "count()"))
            return
        packed = [ac.pack_windows(w) for _, w in parts]
        segs = [ac.DeviceSegment.upload(km, p) for (km, _), p in zip(parts, packed)]
        for s in segs:
            s.counts = filled(s.n_kmers)
        lens = None if v.kind == "wm" else [p.equal_window_len() or 100 for p in packed]
        E = v.E
        words = (lambda s: (s.n_kmers + 31) // 32)
        hb = pb = None
        if v.kind in ("hits", "pos"):
            hb = [filled(ac.hits_words(s.n_kmers, s.n_windows, E)) if sc.live(j) else None
                  for s, j in zip(segs, v.shape.jobs)]
        if v.kind == "pos":
            pb = [filled(ac.positions_words(s.n_kmers, s.n_windows)) if sc.live(j) else None
                  for s, j in zip(segs, v.shape.jobs)]
        sb = None
        if sc.pos_spans(v):  # (a dead segment's tensor must stay as it is: the span pass skips it)
            sb = [filled(ac.positions_words(s.n_kmers, s.n_windows) if sc.live(j) else 8) for s, j in zip(segs, v.shape.jobs)]
        call = lambda: c.count_device(k, segs, window_len=lens, hits=hb, positions=pb, spans=sb)  # noqa: E731
        if v.kind != "wm" and not BS_ON and (hb is not None or E != 2):
            return self.refused_launch(v, call, [s.counts for s in segs] + (hb or []) + (pb or []) + (sb or []))
        call()
        torch.cuda.synchronize()
        c.check()
        self.reached(v, 0 if v.kind == "wm" else BITSLICE)
        for j, (s, job) in enumerate(zip(segs, v.shape.jobs)):
            if not s.n_kmers:
                assert untouched([s.counts])
                continue
            counts = take(s.counts, s.n_kmers, (s.n_kmers,), "counts").astype(np.uint64)
            if hb is None or not sc.live(job):
                same(counts, sc.expected_counts(v.shape, j, E), (v.kind, v.n, j))
                continue
            nh = ac.hits_words(s.n_kmers, s.n_windows, E)
            levels = take(hb[j], nh, (E + 1, s.n_windows, words(s)), "hits")
            planes = None
            if pb is not None:
                planes = take(pb[j], ac.positions_words(s.n_kmers, s.n_windows), (8, s.n_windows, words(s)), "positions")
            self.compare_matrices(v, j, counts, levels, planes)
            if sb is not None:
                starts = take(sb[j], ac.positions_words(s.n_kmers, s.n_windows), (8, s.n_windows, words(s)), "starts")
                same(starts, sc.packed_starts(v.shape, j, E), (v.kind, v.n, j, "start words"))
        if sb is not None:
            assert untouched([t for t, job in zip(sb, v.shape.jobs) if not sc.live(job)]), "a dead segment's starts"
        if hb is not None:
            self.keep(v, hb, pb)

    def launch_samples(self, v):
        c, k, parts = self.c, v.shape.k, self.parts(v)
        packed = [ac.pack_windows(w) for _, w in parts]
        dev = [c.upload_sample(p, slot) for slot, p in enumerate(packed)]
        self.uploaded = (v.shape, 0)
        bs = sc.is_bs(v.kind, v.shape, BS_ON)
        call = lambda: c.count_samples(k, [(km, d) for (km, _), d in zip(parts, dev)])  # noqa: E731
        if v.E != 2 and not bs:
            return self.refused_launch(v, call)
        got = call()
        self.reached(v, 1 if bs else 0)
        for j in range(len(parts)):
            same(got[j], sc.expected_counts(v.shape, j, v.E), (v.kind, v.n, j))
        if not v.wh:
            return
        positions = v.nth % 2 == 1
        wh_call = lambda: c.window_hits(k, list(zip([km for km, _ in parts], packed)), positions=positions)  # noqa: E731
        if not BS_ON:
            return refused(c, wh_call, "AC_BITSLICE")
        wh = wh_call()
        self.reached(v, 1)
        for j, job in enumerate(v.shape.jobs):
            if sc.live(job):
                self.compare_matrices(v, j, wh[j].counts, wh[j].levels, wh[j].planes)
            else:
                assert not wh[j].counts.any()
        j = next(i for i, x in enumerate(v.shape.jobs) if sc.live(x))
        self.keep(v, {j: to_device(wh[j].levels)}, {j: to_device(wh[j].planes)} if positions else None)

    def compare_profiles(self, v, j, D, edits, starts, flanks, edit_prof):
        """The start planes, and the flank and edit profiles the variant asked for, of live job j."""
        nk = v.shape.jobs[j][0]
        same(starts, sc.packed_starts(v.shape, j, v.E), (v.kind, v.n, j, "start words"))
        if D:
            same(np.asarray(flanks).reshape(2, nk, D, 5), sc.expected_flanks(v.shape, j, v.E, D),
                 (v.kind, v.n, j, f"flank profile, D = {D}: (side, k-mer, column, symbol)"))
        if edits:
            same(np.asarray(edit_prof).reshape(nk, v.shape.k, 12), sc.expected_edits(v.shape, j, v.E),
                 (v.kind, v.n, j, "edit profile: (k-mer, base, operation)"))

    def launch_profiles(self, v):
        """window_hits(spans= / flanks= / edits=): the parts are uploaded into the slots, counted in one launch,
        and the span, flank and edit passes follow per job on the context's stream.  A shape with a dead job goes
        through upload_sample and the entry point itself, over filled host buffers: a job without work leaves
        them as they are."""
        c, k, parts = self.c, v.shape.k, self.parts(v)
        packed = [ac.pack_windows(w) for _, w in parts]
        spans, D, edits = sc.profile_args(v)
        self.uploaded = (v.shape, 0)
        first = next(i for i, x in enumerate(v.shape.jobs) if sc.live(x))
        if all(sc.live(x) for x in v.shape.jobs):
            call = lambda: c.window_hits(k, [(km, p) for (km, _), p in zip(parts, packed)], spans=spans, flanks=D,  # noqa: E731
                                         edits=edits)
            if not BS_ON:
                return self.refused_launch(v, call)
            wh = call()
            self.reached(v, 1)
            for j in range(len(parts)):
                self.compare_matrices(v, j, wh[j].counts, wh[j].levels, wh[j].planes)
                assert (wh[j].flanks is None) == (not D) and (wh[j].edits is None) == (not edits)
                self.compare_profiles(v, j, D, edits, wh[j].starts, wh[j].flanks, wh[j].edits)
            self.keep(v, {first: to_device(wh[first].levels)}, {first: to_device(wh[first].planes)})
            return
        before = (kernel_of(c), c.last_launch(), c.max_errors)
        st, counts, bufs = raw_window_profiles(c, k, parts, packed, D, edits)
        if not BS_ON:
            assert st == _lib.AC_ERR_INVALID and "AC_BITSLICE" in c._L.ac_last_error(c.handle).decode(), st
            assert all((a == FILL).all() for b in bufs for a in b.values()), "a refused call wrote"
            c.check()
            assert (kernel_of(c), c.last_launch(), c.max_errors) == before
            return
        _lib.check(st, c.handle)
        self.reached(v, 1)
        used = {"hits", "pos", "start"} | ({"flank"} if D else set()) | ({"edit"} if edits else set())
        for j, (job, b) in enumerate(zip(v.shape.jobs, bufs)):
            nk, nw = job[:2]
            assert counts[j][nk] == 0xFFFFFFFFFFFFFFFF, "a count past the job's k-mers"
            if not sc.live(job):  # no work: zero counts, every host buffer as it was
                assert not counts[j][:nk].any() and all((a == FILL).all() for a in b.values()), (v.n, j)
                continue
            words = (nk + 31) // 32
            shapes = {"hits": (v.E + 1, nw, words), "pos": (8, nw, words), "start": (8, nw, words),
                      "flank": (2, nk, D, 5), "edit": (nk, k, 12)}
            got = {}
            for name, a in b.items():
                n = int(np.prod(shapes[name]))
                assert (a[n if name in used else 0:] == FILL).all(), (v.n, j, name, "a store past the end, or into a buffer not asked for")
                got[name] = a[:n].reshape(shapes[name])
            self.compare_matrices(v, j, counts[j][:nk], got["hits"], got["pos"])
            self.compare_profiles(v, j, D, edits, got["start"], got["flank"], got["edit"])
        self.keep(v, {first: to_device(bufs[first]["hits"][:-GUARD])}, {first: to_device(bufs[first]["pos"][:-GUARD])})

    def jobs_of(self, v, pinned=False):
        out = []
        for km, w in self.parts(v):
            s = ac.Dna5Sample.from_windows(w)
            out.append((km, s.pinned() if pinned else s))
        return ac.Jobs(out)

    def launch_count_jobs(self, v, kernel, mode):
        c, jobs = self.c, self.jobs_of(v, pinned=v.kind == "dp_jobs")
        flags = self.hooks_for(v)
        bs = sc.is_bs(v.kind, v.shape, BS_ON)
        with hooks(flags):
            if v.E != 2 and not bs:
                return self.refused_launch(v, lambda: c.count_jobs(v.shape.k, jobs))
            got = [x.copy() for x in c.count_jobs(v.shape.k, jobs)]
        self.reached(v, kernel if bs or kernel == 0 else 0, mode if EARLY else 0,
                     groups=not (flags & AC_TESTING_TWO_PARTS))
        for j in range(len(got)):
            same(got[j], sc.expected_counts(v.shape, j, v.E), (v.kind, v.n, j))

    def launch_wm_jobs(self, v):
        self.launch_count_jobs(v, 0, 2)

    def launch_bs_jobs(self, v):
        self.launch_count_jobs(v, 1, 2)

    def launch_dp_jobs(self, v):
        self.launch_count_jobs(v, 1, 3)

    def launch_window_hits_jobs(self, v, positions):
        c, jobs = self.c, self.jobs_of(v)
        flags = self.hooks_for(v)
        with hooks(flags):
            call = lambda: c.window_hits_jobs(v.shape.k, jobs, positions=positions)  # noqa: E731
            if not BS_ON:
                return self.refused_launch(v, call)
            wh = call()
        self.reached(v, 1, 2 if EARLY else 0, groups=not (flags & AC_TESTING_TWO_PARTS))
        for j, job in enumerate(v.shape.jobs):
            if sc.live(job):
                self.compare_matrices(v, j, wh[j].counts, wh[j].levels, wh[j].planes if positions else None)
            else:
                assert not wh[j].counts.any() and wh[j].levels.size == 0
        j = next(i for i, x in enumerate(v.shape.jobs) if sc.live(x))
        self.keep(v, {j: to_device(wh[j].levels)}, {j: to_device(wh[j].planes)} if positions else None)

    def launch_hits_jobs(self, v):
        self.launch_window_hits_jobs(v, False)

    def launch_pos_jobs(self, v):
        self.launch_window_hits_jobs(v, True)

    def launch_submit(self, v):
        """submit_jobs into a filled device tensor -- with hits= (and, every other time, positions=) or without
        -- then synchronize, check(), compare."""
        import torch

        c, k, E, jobs = self.c, v.shape.k, v.E, self.jobs_of(v)
        shapes = [(job[0], job[1]) for job in v.shape.jobs]
        out = filled(jobs.n_counts)
        dh = dp = None
        positions = v.with_hits and v.nth % 4 == 3
        if v.with_hits:
            dh = [filled(ac.hits_words(nk, nw, E)) if nk and nw else None for nk, nw in shapes]
        if positions:
            dp = [filled(ac.positions_words(nk, nw)) if nk and nw else None for nk, nw in shapes]
        st = torch.cuda.current_stream()
        flags = self.hooks_for(v)
        with hooks(flags):
            call = lambda: c.submit_jobs(k, jobs, out, stream=st.cuda_stream, hits=dh, positions=dp)  # noqa: E731
            if not BS_ON and (v.with_hits or E != 2):
                return self.refused_launch(v, call, [out] + (dh or []) + (dp or []))
            call()
            st.synchronize()
            torch.cuda.synchronize()
            c.check()
        self.reached(v, BITSLICE, groups=BS_ON and not (flags & AC_TESTING_TWO_PARTS))
        counts, at = take(out, jobs.n_counts, (jobs.n_counts,), "submit counts").astype(np.uint64), 0
        for j, (nk, nw) in enumerate(shapes):
            mine = counts[at:at + nk]
            at += nk
            if not (nk and nw):
                assert not mine.any()
            elif not v.with_hits:
                same(mine, sc.expected_counts(v.shape, j, E), (v.kind, v.n, j))
            else:
                words = (nk + 31) // 32
                levels = take(dh[j], ac.hits_words(nk, nw, E), (E + 1, nw, words), "submit hits")
                planes = take(dp[j], ac.positions_words(nk, nw), (8, nw, words), "submit positions") if positions else None
                self.compare_matrices(v, j, mine, levels, planes)
        if v.with_hits:
            self.keep(v, dh, dp)

    # ---- side operations ----

    def side(self, name, i):
        getattr(self, "side_" + name)(i)

    def matrix(self):
        shape, j, E, d_hits, d_pos = self.mat
        hit, pos, _ = sc.expected_matrices(shape, j, E)
        nk, nw, L = shape.jobs[j][:3]
        return hit, pos, nk, nw, L, E + 1, d_hits, d_pos

    def reduce(self, fn, args, n, shape, what):
        import torch

        out = filled(n)
        _lib.check(fn(self.c.handle, *args, p32(out), None), self.c.handle)
        torch.cuda.synchronize()
        self.c.check()
        return take(out, n, shape, what)

    def side_exact(self, shape, j):
        got = self.c.exact_count(shape.k, ac.pack_windows(sc.case(shape, j)[1]),
                                 float(sc_threshold(shape.k)), (), 50)
        assert got == sc.expected_exact(shape, j), ("exact count", shape)

    def side_exact_packed(self, i):
        shape = (sc.BS_SHAPES[0], sc.WM_SHAPES[1], sc.WM_JOBS_SHAPES[0])[i % 3]
        self.side_exact(shape, 0)

    def side_exact_uploaded(self, i):
        self.side_exact(*self.uploaded)

    def side_level_counts(self, i):
        hit, _, nk, nw, _, lv, d_hits, _ = self.matrix()
        got = self.reduce(self.c._L.ac_hit_level_counts_device, (p32(d_hits), nk, nw, lv), lv * nk, (lv, nk), "level counts")
        same(got, hit.sum(axis=1), "level counts")

    def side_position_profile(self, i):
        hit, pos, nk, nw, L, lv, d_hits, d_pos = self.matrix()
        got = self.reduce(self.c._L.ac_hit_position_profile_device, (p32(d_hits), p32(d_pos), nk, nw, lv, L),
                          lv * nk * L, (lv, nk, L), "position profile")
        same(got, profile_of(hit, pos, L), "position profile")

    def side_window_counts(self, i):
        hit, _, nk, nw, _, lv, d_hits, _ = self.matrix()
        got = self.reduce(self.c._L.ac_hit_window_counts_device, (p32(d_hits), nk, nw, lv), lv * nw, (lv, nw), "window counts")
        same(got, hit.sum(axis=2), "window counts")

    def side_cooc(self, i):
        hit, _, nk, nw, _, lv, d_hits, _ = self.matrix()
        got = self.reduce(self.c._L.ac_hit_cooccurrence_device, (p32(d_hits), nk, nw, lv), lv * nk * nk, (lv, nk, nk), "cooc")
        same(got, sc.product(hit, hit), "co-occurrence")

    def side_cross(self, i):
        """The matrix's bottom plane against its top one."""
        hit, _, nk, nw, _, lv, d_hits, _ = self.matrix()
        top = d_hits[(lv - 1) * nw * ((nk + 31) // 32):]
        got = self.reduce(self.c._L.ac_hit_cross_cooccurrence_device, (p32(d_hits), nk, p32(top), nk, nw, 1), nk * nk,
                          (1, nk, nk), "cross")
        same(got, sc.product(hit[:1], hit[-1:]), "cross co-occurrence")

    def profile_inputs(self):
        """The matrix's job for the span, flank and edit passes: (shape, j, E, n_kmers, n_windows, L, hits, pos,
        plane(e) -> level plane e, the expected start matrix uploaded).  The starts come from the CPU reference,
        so that a wrong span pass cannot hide a wrong flank or edit pass."""
        shape, j, E, d_hits, d_pos = self.mat
        nk, nw, L = shape.jobs[j][:3]
        size = nw * ((nk + 31) // 32)
        return (shape, j, E, nk, nw, L, d_hits, d_pos, lambda e: d_hits[e * size:(e + 1) * size],
                to_device(sc.packed_starts(shape, j, E)))

    def device_pass(self, fn, n, shape, what):
        """One pass into a filled, guarded output: synchronize, check(), the guard, the result."""
        import torch

        out = filled(n)
        fn(out)
        torch.cuda.synchronize()
        self.c.check()
        return take(out, n, shape, what)

    def side_spans_device(self, i):
        shape, j, E, nk, nw, L, d_hits, d_pos, _, _ = self.profile_inputs()
        got = self.device_pass(lambda out: self.c.hit_start_positions(shape.k, self.seg.kmers, nk, self.seg, L, d_hits, d_pos,
                                                                      E + 1, out=out),
                               ac.positions_words(nk, nw), (8, nw, (nk + 31) // 32), "starts")
        same(got, sc.packed_starts(shape, j, E), "span pass: start words")

    def side_flanks_device(self, i):
        """With the start matrix and with start = None (the left half zeros), over the top plane and plane 0."""
        shape, j, E, nk, nw, L, _, d_pos, plane, d_start = self.profile_inputs()
        with_start, top, D = sc.flanks_side(i)
        got = self.device_pass(lambda out: self.c.hit_flank_profile(self.seg, L, plane(E if top else 0), d_pos,
                                                                    d_start if with_start else None, nk, nw, D, out=out),
                               ac.flank_words(nk, D), (2, nk, D, 5), "flank profile")
        same(got, sc.expected_flanks(shape, j, E, D, None if top else 0, with_start),
             f"flank pass, D = {D}, {'top plane' if top else 'plane 0'}, {'with' if with_start else 'no'} starts: "
             "(side, k-mer, column, symbol)")
        assert with_start or not got[1].any()

    def side_edits_device(self, i):
        shape, j, E, nk, nw, L, _, d_pos, plane, d_start = self.profile_inputs()
        top = sc.edits_side(i)
        got = self.device_pass(lambda out: self.c.hit_edit_profile(shape.k, self.seg.kmers, nk, self.seg, L,
                                                                   plane(E if top else 0), d_pos, d_start, nw, out=out),
                               ac.edit_words(nk, shape.k), (nk, shape.k, 12), "edit profile")
        same(got, sc.expected_edits(shape, j, E, None if top else 0),
             f"edit pass, {'top plane' if top else 'plane 0'}: (k-mer, base, operation)")

    def side_refuse_profiles(self, i):
        """One refusal of each of the three passes, the cases in turn (those tests/test_gpu_spans.py,
        test_gpu_flanks.py and test_gpu_edits.py pin)."""
        c = self.c
        shape, j, E, nk, nw, L, d_hits, d_pos, plane, d_start = self.profile_inputs()
        k, seg, top = shape.k, self.seg, plane(E)
        out = filled(max(ac.positions_words(nk, nw), ac.flank_words(nk, 32), ac.edit_words(nk, 32)))
        span = lambda kk=k, wl=L, lv=E + 1, p=d_pos: (  # noqa: E731
            lambda: c.hit_start_positions(kk, seg.kmers, nk, seg, wl, d_hits, p, lv, out=out))
        flank = lambda wl=L, d=8, h=top: lambda: c.hit_flank_profile(seg, wl, h, d_pos, d_start, nk, nw, d, out=out)  # noqa: E731
        edit = lambda kk=k, wl=L, s=d_start: (  # noqa: E731
            lambda: c.hit_edit_profile(kk, seg.kmers, nk, seg, wl, top, d_pos, s, nw, out=out))
        for fn, word in (((span(lv=5), "levels must be 1..4"), (span(kk=33), "k must be 2..32"), (span(p=None), "hits or pos is NULL"))[i % 3],
                         ((flank(d=33), "depth must be 1..32"), (flank(wl=257), "window_len must be 1..256"),
                          (flank(h=None), "hit_plane or pos is NULL"))[i % 3],
                         ((edit(wl=0), "window_len must be 1..256"), (edit(kk=33), "k must be 2..32"),
                          (edit(s=None), "hit_plane, pos or start is NULL"))[i % 3]):
            refused(c, fn, word, [out])

    def side_cooc_host(self, i):
        nk, nw = sc.COOC_HOST[i % 3]
        hit, m = sc.random_hits(nk, nw, 3, 1)
        same(self.c.cooccurrence_host(m, nk, nw, 3), sc.product(hit, hit), "host co-occurrence")
        self.c.check()

    def side_cross_host(self, i):
        na, nb, nw = sc.CROSS_HOST[i % 3]
        (ha, ma), (hb, mb) = sc.random_hits(na, nw, 3, 2), sc.random_hits(nb, nw, 3, 3)
        same(self.c.cross_cooccurrence_host(ma, na, mb, nb, nw, 3), sc.product(ha, hb), "host cross co-occurrence")
        self.c.check()

    def side_reupload(self, i):
        """Other samples into both slots, which a launch has just read: ragged with N into slot 0, a small one
        into slot 1.  The notes about the slots' images must go with them."""
        shape = sc.SAMPLE_STATES[2] if i % 2 == 0 else sc.SAMPLE_STATES[3]
        self.c.upload_sample(ac.pack_windows(sc.case(shape, 0)[1]), 0)
        self.c.upload_sample(ac.pack_windows(sc.case(sc.SAMPLE_STATES[3], 1)[1]), 1)
        self.uploaded = (shape, 0)
        self.c.check()

    def side_empty(self, i):
        """K-mers but no windows: nothing is launched, the counts come back zero over the fill, and the context's
        last launch stays what it was."""
        import torch

        c = self.c
        if not BS_ON and c.max_errors != 2:
            return  # (AC_BITSLICE=0: at such a budget every call is a refusal, the empty one too)
        before = kernel_of(c)
        km = sc.case(sc.BS_SHAPES[3], 3)[0]
        assert len(km) == 5
        if i % 2 == 0:
            seg = ac.DeviceSegment.upload(km, ac.pack_windows([]))
            seg.counts = filled(len(km))
            c.count_device(16, [seg], window_len=[100])
            torch.cuda.synchronize()
            got = take(seg.counts, len(km), (len(km),), "empty call")
        else:
            got = c.count_jobs(16, [(km, [])])[0]
        c.check()
        assert not np.asarray(got).any() and kernel_of(c) == before

    def ragged_segment(self):
        km, w = sc.case(sc.WM_SHAPES[2], 2)
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        seg.counts = filled(seg.n_kmers)
        return seg

    def side_refuse_ragged_hits(self, i):
        seg = self.ragged_segment()
        hb = filled(ac.hits_words(seg.n_kmers, seg.n_windows, 3))
        refused(self.c, lambda: self.c.count_device(16, [seg], hits=[hb]), "ragged", [seg.counts, hb])

    def side_refuse_pos_without_hits(self, i):
        c = self.c
        km, w = sc.case(sc.HIT_SHAPES[0], 0)
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        seg.counts = filled(seg.n_kmers)
        pb = filled(ac.positions_words(seg.n_kmers, seg.n_windows))
        arr = c.segment_array([seg])
        wl = np.array([100], np.uint32)
        pp = (_lib.p32 * 1)(p32(pb))
        st = c._L.ac_window_positions_device(c.handle, 16, arr, 1, wl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None,
                                             pp, None)
        raw_refused(c, st, "hits is NULL", [seg.counts, pb])

    def side_refuse_budget_k(self, i):
        """A budget other than 2 at k = 17, which the bit-sliced kernel lacks: through count_jobs and count_device."""
        c = self.c
        assert c.max_errors != 2
        km, w = sc.case(sc.WM_SHAPES[1], 0)
        if i % 2 == 0:
            refused(c, lambda: c.count_jobs(17, [(km, w)]), "16 or 18..32")
        else:
            seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
            seg.counts = filled(seg.n_kmers)
            refused(c, lambda: c.count_device(17, [seg]), "16 or 18..32", [seg.counts])

    def side_refuse_levels5(self, i):
        c, L = self.c, self.c._L
        _, _, nk, nw, wl, lv, d_hits, d_pos = self.matrix()
        out = filled(5 * max(nk * nk, nk * wl, nw))
        h, o = p32(d_hits), p32(out)
        for st in (L.ac_hit_level_counts_device(c.handle, h, nk, nw, 5, o, None),
                   L.ac_hit_window_counts_device(c.handle, h, nk, nw, 5, o, None),
                   L.ac_hit_cooccurrence_device(c.handle, h, nk, nw, 5, o, None),
                   L.ac_hit_cross_cooccurrence_device(c.handle, h, nk, h, nk, nw, 5, o, None),
                   L.ac_hit_position_profile_device(c.handle, h, p32(d_pos), nk, nw, 5, wl, o, None)):
            raw_refused(c, st, "levels must be 1..4", [out])

    # ---- a segment ----

    def segment(self, ops):
        for op in ops:
            if op[0] == "set_max_errors":
                self.c.set_max_errors(op[1])
                assert self.c.max_errors == op[1]
            elif op[0] == "side":
                self.side(op[1], op[2])
            else:
                assert self.c.max_errors == op[1].E
                self.launch(op[1])


def sc_threshold(k):
    from oracle import host_ref

    return host_ref.adjust_threshold(1.0, 16, k)


# ---- the walk on one context, and segment by segment on fresh ones -----------------------------------------------

@pytest.fixture(scope="module")
def shared():
    """One context for the whole walk: it starts at max_errors = 2, and only the walk's set_max_errors operations
    change it."""
    with ac.ApproxCounter(0) as c:
        assert c.max_errors == 2
        yield Run(c)


@pytest.mark.parametrize("s", range(len(sc.SEGMENTS)))
def test_walk_on_one_context(shared, s):
    t = time.perf_counter()
    shared.segment(sc.SEGMENTS[s])
    print(f"segment {s}: {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("s", range(len(sc.SEGMENTS)))
def test_segment_on_a_fresh_context(s):
    with ac.ApproxCounter(0) as c:
        Run(c).segment(sc.SEGMENTS[s])


# ---- the DMA route: a child process with AC_STAGE_EARLY=0 ----------------------------------------------------------

def child_dma_route():
    """The first two segments on one context without the early launch (ac_stage_mode 0: the copy engine moves the
    jobs, the plain kernels count them), every other jobs call cut into two parts (AC_TESTING_TWO_PARTS)."""
    import torch

    assert not EARLY
    with ac.ApproxCounter(0) as c:
        r = Run(c, two_parts=True)
        for seg in sc.SEGMENTS[:2]:
            r.segment(seg)
        torch.cuda.synchronize()
        c.check()
        assert r.jobs_calls >= 8


def test_dma_route_first_two_segments():
    code = "from tests.test_gpu_call_sequence import *\nchild_dma_route()\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, AC_STAGE_EARLY="0"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])


# ---- the command line: everything on at once, three runs on one context ---------------------------------------------

def test_cli_every_extension_three_runs(tmp_path):
    """adaptFinder on the cfg1 FASTA with --seed 1 -mr 3 --paired-sample --levels --positions --spans --flanks 8
    --edits --cooccurrence --cross-cooccurrence --max-errors 3: three runs of upload, exact count, positions
    launch, span, flank and edit passes, co-occurrence and cross on one context.  Every file of runs 1 and 2 is byte for byte run 0's, and run 0's main files are those of
    the same command without the extension flags."""
    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1",
            "-mr", "3", "--paired-sample", "--max-errors", "3"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["--levels", "--positions", "--spans", "--flanks", "8", "--edits", "--cooccurrence", "--cross-cooccurrence",
             "-o", "all"])
    if not BS_ON:
        assert r.returncode == 1 and "AC_BITSLICE" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    plain = run(["-o", "plain"])
    assert plain.returncode == 0, plain.stderr
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("all_0."))
    assert {"all_0.start", "all_0.end", "all_0.cross"} <= set(names), names
    for ext in (".levels", ".positions", ".cooc", ".starts", ".lengths", ".flanks", ".edits"):
        assert {f"all_0.start{ext}", f"all_0.end{ext}"} <= set(names), names
    for name in names:
        first = (tmp_path / name).read_bytes()
        assert first, name
        for run_id in (1, 2):
            assert (tmp_path / name.replace("all_0.", f"all_{run_id}.")).read_bytes() == first, (name, run_id)
    for end in ("start", "end"):
        assert (tmp_path / f"all_0.{end}").read_bytes() == (tmp_path / f"plain_0.{end}").read_bytes(), end
