"""GPU tests of the routes by which a launch reaches the bit-sliced count kernel (bs_count.inc; DESIGN.md
§4e, "routes tested"), and of its work items of more than one row.  Every case goes through the C ABI,
is compared bit-exactly with the CPU oracle -- directly, or for large samples through a dictionary
(tests/cases.py dictionary_case: the sample's counts are a sum of its texts' oracle count vectors) --
and asserts which count kernel the launch ran (ac_testing_last_count_kernel).

Work items: an item is chunk = min(8, rows per wave / 64) rows (count_launch.cpp).  AC_BS_WAVES_PCT
(read once per process: child processes) shrinks a launch to 1 % of the waves that fit, so that ~21k
rows of 20-base windows are items of 8 rows; ac_last_launch says what the launch planned, and the
chunk derived from it guards that the shape reached the path (it is no correctness check)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from tests import cases
from tests.test_gpu_bitslice import (AC_TESTING_ALL_AHEAD, BITSLICE, WORD, device_count, equal_case, hooks,
                                     kernel_of, n_windows_case)
from tests.test_gpu_bs_claims import fitting_waves

pytestmark = pytest.mark.gpu
K = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what a launch planned is asserted for the bit-sliced kernel at its own share of the waves
GEOMETRY = bool(BITSLICE) and "AC_BS_WAVES_PCT" not in os.environ


def bs_rows(n_kmers, n_windows):
    """Rows (work items of chunk 1) of a segment: per group of 256 candidates, rows of 64 / LW windows."""
    rows = 0
    for g0 in range(0, n_kmers, 256):
        blocks = -(-min(256, n_kmers - g0) // 32)
        lw = 2
        while lw < blocks:
            lw *= 2
        rows += -(-n_windows // (64 // lw))
    return rows


def chunk_of(items, waves):
    return max(1, min(8, -(-items // waves) // 64))


def rows_for(W, chunk):
    """Rows of 13 + 64 x chunk per wave and one more (so the launch's items are `chunk` rows), not a
    multiple of chunk (the last item is partial)."""
    rows = W * (64 * chunk + 13) + 1
    while chunk > 1 and rows % chunk == 0:
        rows += 1
    return rows


def windows_for(W, chunk, n_kmers, first, ok):
    """The first window count from `first` on at which ok(n) holds and the launch's items are `chunk` rows."""
    for n in range(first, first + 4096):
        if ok(n) and chunk_of(bs_rows(n_kmers, n), W) == chunk:
            return n
    raise AssertionError("no window count with these properties")


class Reach:
    """Compares counts, and what the launch ran and planned with what the case set out to reach."""

    def __init__(self, counter, geometry):
        self.c, self.geometry = counter, geometry

    def same(self, what, got, want, kernel=BITSLICE):
        assert kernel_of(self.c) == kernel, what
        bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
        assert bad.size == 0, (what, bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])

    def planned(self, what, W, chunk):
        geo = self.c.last_launch()
        got = max(1, min(8, int(geo["windows_per_wave"]) // 64))
        print(f"reached {what}: waves {geo['waves']} rows/wave {geo['windows_per_wave']} chunk {got}", flush=True)
        if self.geometry:
            assert geo["waves"] == W and got == chunk, (what, geo, W, chunk)


def run_child(call, **env):
    code = f"from tests.test_gpu_bs_routes import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


# ---- 1, 2: work items of more than one row (children with AC_BS_WAVES_PCT) ----

def child_items_one_percent(fit, geometry):
    """1 % of the waves that fit.  Resident (ac_error_count_device): one group at chunk 1, 2, 3 and 8 with
    a partial last item and a partial last row (at 8, waves of ~525 rows flush their counters inside
    items many times); two groups with rows of 8 and of 32 windows; two fused segments.  Staged
    (ac_error_count_jobs, a heap sample): windows of 100 bases with inline N records, overflowed ones
    too, so the whole-segment wait happens inside an item."""
    W = max(4, fit // 100 // 4 * 4)
    with ac.ApproxCounter(0) as c:
        r = Reach(c, geometry)
        if geometry:
            assert fitting_waves(c) == W, (fitting_waves(c), W)
        km, texts, per = cases.dictionary_case(4, 40, 20, n_per_text=cases.SHORT_N)
        for chunk in (1, 2, 3, 8):
            rows = rows_for(W, chunk)
            w, want = cases.dictionary_sample(texts, per, 32 * rows - 5, chunk)
            assert bs_rows(40, len(w)) == rows and chunk_of(rows, W) == chunk
            r.same(("one group", chunk), device_count(c, K, [(km, w)])[0], want)
            r.planned(f"resident, one group, chunk {chunk}", W, chunk)

        km, texts, per = cases.dictionary_case(1, 300, 24, n_per_text=cases.SHORT_N)
        n = windows_for(W, 2, 300, (W * 141 + 1) * 32 // 5,
                        lambda n: n % 8 and -(-n // 8) % 2 and -(-n // 32) % 2)
        w, want = cases.dictionary_sample(texts, per, n, 5)
        r.same("two groups", device_count(c, K, [(km, w)])[0], want)
        r.planned("resident, two groups, chunk 2", W, 2)

        a = cases.dictionary_case(2, 129, 100)
        b = cases.dictionary_case(1, 40, 33, n_per_text=cases.SHORT_N)
        na = next(n for n in range((W * 141 + 1) * 320 // 41, 1 << 30)
                  if chunk_of(bs_rows(129, n) + bs_rows(40, n // 10), W) == 2 and n % 8 and (n // 10) % 32)
        wa, want_a = cases.dictionary_sample(a[1], a[2], na, 6)
        wb, want_b = cases.dictionary_sample(b[1], b[2], na // 10, 7)
        got = device_count(c, K, [(a[0], wa), (b[0], wb)])
        r.same("fused, first", got[0], want_a)
        r.same("fused, second", got[1], want_b)
        r.planned("resident, two fused segments, chunk 2", W, 2)

        km, texts, per = cases.dictionary_case(1, 40, 100)
        assert ((texts == 4).sum(axis=1) >= 5).any()  # records that overflow
        for chunk in (2, 8):
            w, want = cases.dictionary_sample(texts, per, 32 * rows_for(W, chunk) - 5, 10 + chunk)
            smp = ac.Dna5Sample.from_windows(w)
            for flags in (0, AC_TESTING_ALL_AHEAD):
                with hooks(flags):
                    got = c.count_jobs(K, [(km, smp)])[0]
                assert c.stage_mode() == 2, c.stage_mode()
                r.same(("staged", chunk, flags), got, want)
                r.planned(f"staged, hooks {flags}, chunk {chunk}", W, chunk)


def child_items_ten_percent(fit, geometry):
    """10 % of the waves that fit: more sub-queues than at 1 %, so the steal probe has more siblings; 300
    candidates (two groups) at chunk 2, resident and staged."""
    W = max(4, fit // 10 // 4 * 4)
    with ac.ApproxCounter(0) as c:
        r = Reach(c, geometry)
        km, texts, per = cases.dictionary_case(1, 300, 20, n_per_text=cases.SHORT_N)
        n = windows_for(W, 2, 300, (W * 141 + 1) * 32 // 5,
                        lambda n: n % 8 and -(-n // 8) % 2 and -(-n // 32) % 2)
        w, want = cases.dictionary_sample(texts, per, n, 8)
        r.same("resident", device_count(c, K, [(km, w)])[0], want)
        r.planned("10 %, resident, chunk 2", W, 2)
        got = c.count_jobs(K, [(km, ac.Dna5Sample.from_windows(w))])[0]
        assert c.stage_mode() == 2, c.stage_mode()
        r.same("staged", got, want)
        r.planned("10 %, staged, chunk 2", W, 2)


def test_multi_row_items_resident_and_staged(counter):
    out = run_child(f"child_items_one_percent({fitting_waves(counter)}, {GEOMETRY})", AC_BS_WAVES_PCT="1")
    print(out)
    if GEOMETRY:
        for what in ("resident, one group, chunk 2", "resident, one group, chunk 3", "resident, one group, chunk 8",
                     "staged, hooks 0, chunk 8", "staged, hooks 2, chunk 8"):
            assert re.search(f"reached {what}: .* chunk {what[-1]}\n", out), what


def test_multi_row_items_more_sub_queues(counter):
    print(run_child(f"child_items_ten_percent({fitting_waves(counter)}, {GEOMETRY})", AC_BS_WAVES_PCT="10"))


# ---- 3: the DMA path (a child with AC_STAGE_EARLY=0): the plain instantiation with inline N records ----

def more_kmers(w, n, seed):
    """n k-mers cut from rows of the 2-D Dna5 array w (an N base replaced at random)."""
    rng = np.random.default_rng(seed)
    km = []
    for _ in range(n):
        row = w[int(rng.integers(len(w)))]
        s0 = int(rng.integers(0, w.shape[1] - K + 1))
        v = 0
        for b in row[s0:s0 + K]:
            v = (v << 2) | (int(b) if b < 4 else int(rng.integers(4)))
        km.append(v)
    return np.array(km, np.uint64)


def submit_counts(c, jobs):
    """ac_error_count_jobs_submit into a device tensor pre-filled with garbage, then ac_check."""
    import torch

    out = torch.full((jobs.n_counts,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    c.submit_jobs(K, jobs, out, stream=st.cuda_stream)
    c.check(stream=st.cuda_stream)
    return out.cpu().numpy().view(np.uint32).astype(np.uint64)


def child_dma_path():
    """ac_error_count_jobs and _submit without the early launch (ac_stage_mode 0): the copy engine moves
    the jobs and bs_count_kernel<16, false> reads inline N records.  One part (direct oracle): records,
    overflowed records, and windows of 128 bases (no room for a record: bitmap words).  Two parts
    (>= 2^17 windows: part 0 runs with half the waves) and four (>= 2^19), synchronous and as a submit
    whose parts add into one device vector."""
    with ac.ApproxCounter(0) as c:
        r = Reach(c, False)
        km60, w1 = n_windows_case(5, 900, 100, [0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99))
        km1 = np.concatenate([km60, more_kmers(w1, 240, 6)])
        km2, w2 = equal_case(31, 37, 500, 128, p_n=0.02)
        want = [oracle.count_myers(K, km1, w1, 16), oracle.count_myers(K, km2, w2, 16)]
        assert want[0].any() and want[1].any()
        jobs = ac.Jobs([(km1, ac.Dna5Sample.from_windows(w1)), (km2, ac.Dna5Sample.from_windows(w2))])
        got = c.count_jobs(K, jobs)
        assert c.stage_mode() == 0, c.stage_mode()
        r.same("one part, records", got[0], want[0])
        r.same("one part, bitmap", got[1], want[1])
        r.same("one part, submit", submit_counts(c, jobs), np.concatenate(want))
        assert c.stage_mode() == 0
        print("reached one part, stage mode 0", flush=True)

        a = cases.dictionary_case(4, 40, 20, n_per_text=cases.SHORT_N)
        b = cases.dictionary_case(1, 300, 101)
        d = cases.dictionary_case(18, 40, 16, n_per_text=cases.SHORT_N)
        for parts, shapes in ((2, [(a, (1 << 17) + 777), (b, 5000)]), (4, [(d, (1 << 19) + 5)])):
            smp = [cases.dictionary_sample(x[1], x[2], n, parts + i) for i, (x, n) in enumerate(shapes)]
            jobs = ac.Jobs([(x[0], ac.Dna5Sample.from_windows(w)) for (x, _), (w, _) in zip(shapes, smp)])
            want = [e for _, e in smp]
            got = c.count_jobs(K, jobs)
            assert c.stage_mode() == 0, c.stage_mode()
            for j in range(len(want)):
                r.same((parts, "parts, job", j), got[j], want[j])
            r.same((parts, "parts, submit"), submit_counts(c, jobs), np.concatenate(want))
            assert c.stage_mode() == 0
            print(f"reached {parts} parts ({sum(n for _, n in shapes)} windows), stage mode 0", flush=True)


def test_dma_path_records_and_parts():
    out = run_child("child_dma_path()", AC_STAGE_EARLY="0")
    print(out)
    assert "reached 2 parts" in out and "reached 4 parts" in out


# ---- 4: the CLI's route: ac_sample_upload_slot + ac_error_count_samples ----

@pytest.mark.parametrize("p_n", [0.0, 0.01])
def test_samples_route_equal_ends(counter, p_n):
    """Both ends truly equal windows (100 and 101 bases, as the CLI's start and end samples), 500 and 37
    candidates: N-free (the upload notes no_n: the kernel reads no N words) and with 1 % N (no records:
    the bitmap words are fetched with the text)."""
    a = equal_case(41, 500, 150, 100, p_n=p_n)
    b = equal_case(42, 37, 90, 101, p_n=p_n)
    assert any("N" in x for x in a[1] + b[1]) == (p_n > 0)
    da = counter.upload_sample(ac.pack_windows(a[1]), 0)
    db = counter.upload_sample(ac.pack_windows(b[1]), 1)
    got = counter.count_samples(K, [(a[0], da), (b[0], db)])
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got[0], oracle.count_myers(K, *a)) and np.array_equal(got[1], oracle.count_myers(K, *b))


def test_samples_route_one_ragged_end(counter):
    """One equal and one ragged end: the launch as a whole stays on the word-parallel kernel."""
    a = equal_case(43, 500, 150, 100)
    b = cases.planted_case(44, K, 37, 90, win_len=(90, 110), p_n=0.01)
    da = counter.upload_sample(ac.pack_windows(a[1]), 0)
    db = counter.upload_sample(ac.pack_windows(b[1]), 1)
    got = counter.count_samples(K, [(a[0], da), (b[0], db)])
    assert kernel_of(counter) == WORD
    assert np.array_equal(got[0], oracle.count_myers(K, *a)) and np.array_equal(got[1], oracle.count_myers(K, *b))


# ---- 5: fused launches of four segments ----

@pytest.fixture(scope="module")
def four_segments():
    """Four equal-window segments that differ in lanes per window (8, 2, 2, 8), slot size (32, 8, 64, 32
    bytes) and share of the launch's windows, with their oracle counts."""
    parts = [equal_case(51, 500, 150, 100), equal_case(52, 33, 1500, 16), equal_case(53, 1, 40, 256),
             equal_case(54, 129, 9, 128)]
    want = [oracle.count_myers(K, km, w, 16) for km, w in parts]
    assert all(x.any() for x in want)
    return parts, want


def test_four_fused_segments_resident(counter, four_segments):
    parts, want = four_segments
    got = device_count(counter, K, parts)
    assert kernel_of(counter) == BITSLICE
    assert all(np.array_equal(g, e) for g, e in zip(got, want))
    got = device_count(counter, K, parts, accumulate=True)  # twice into zeroed counts
    assert kernel_of(counter) == BITSLICE
    assert all(np.array_equal(g, 2 * e) for g, e in zip(got, want))


def test_four_fused_segments_as_jobs(counter, four_segments):
    """The same four through ac_error_count_jobs: records (16 and 100 bases) and bitmap words (128, 256)
    in one launch."""
    parts, want = four_segments
    got = counter.count_jobs(K, parts)
    assert kernel_of(counter) == BITSLICE
    assert all(np.array_equal(g, e) for g, e in zip(got, want))


def test_dead_segments_beside_live_ones(counter, four_segments):
    """[live, candidates without windows, windows without candidates, live]: the launch is bit-sliced, and
    the counts of the candidates without windows come back zero over garbage."""
    import torch

    parts, want = four_segments
    no_windows = (parts[1][0], [])
    no_kmers = (np.zeros(0, np.uint64), parts[1][1])
    four = [parts[0], no_windows, no_kmers, parts[3]]
    segs = [ac.DeviceSegment.upload(km, ac.pack_windows(w)) for km, w in four]
    for s in segs:
        s.counts.fill_(12345)
    counter.count_device(K, segs, window_len=[100, 16, 16, 128])
    torch.cuda.synchronize()
    counter.check()
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(segs[0].counts_numpy(), want[0]) and np.array_equal(segs[3].counts_numpy(), want[3])
    assert not segs[1].counts_numpy().any()


def test_window_shards_alias_one_count_vector(counter):
    """Four window shards of one candidate set whose segments share one count vector, pre-filled with
    garbage, in one launch that does not accumulate: the launch zeroes the vector once and every group
    adds; the result equals the whole sample's."""
    import torch

    km, w = equal_case(55, 500, 1000, 100)
    segs = [ac.DeviceSegment.upload(km, ac.pack_windows(w[lo:lo + 250])) for lo in range(0, 1000, 250)]
    shared = torch.full((500,), 12345, dtype=torch.int32, device="cuda")
    for s in segs:
        s.counts = shared
    counter.count_device(K, segs, window_len=[100] * 4)
    torch.cuda.synchronize()
    counter.check()
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(segs[0].counts_numpy(), oracle.count_myers(K, km, w, 16))


# ---- 6: windows shorter than 14 bases ----

@pytest.mark.parametrize("L", [1, 3, 4, 5, 8, 12, 13, 14])
def test_short_windows(counter, L):
    """Windows of one or two 4-base blocks issue and read the next item's claim in the same block.  40
    candidates, 3 x 32 windows per wave that fits (every wave claims several items), each window the
    first L bases of a candidate or of a candidate with one base changed: no window of 13 bases or
    fewer holds an occurrence at 2 edits (the oracle says so, asserted); at 14 -- the control -- the
    unchanged prefixes do.  Staged and resident."""
    rng = np.random.default_rng(L)
    km = np.array(cases.planted_case(60 + L, K, 40, 0)[0], np.uint64)
    texts = []
    for i in range(61):
        t = ac.to_dna5(cases.kmer_string(int(km[i % 40]), K))[:L].copy()
        if i >= 40:
            t[int(rng.integers(L))] ^= 1
        texts.append(t)
    texts = np.stack(texts)
    per = np.stack([oracle.count_myers(K, km, t[None, :]) for t in texts]).astype(np.uint64)
    idx = rng.integers(0, 61, size=3 * fitting_waves(counter) * 32)
    want = np.bincount(idx, minlength=61).astype(np.uint64) @ per
    assert want.any() == (L >= 14)
    w = texts[idx]
    got = counter.count_jobs(K, [(km, ac.Dna5Sample.from_windows(w))])[0]
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got, want)
    got = device_count(counter, K, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got, want)


# ---- 7: ac_create_multi contexts (the DMA path, one unit per shard) ----

@pytest.mark.parametrize("n_gpus", [2, 3])
def test_multi_device_contexts_equal_windows(counter, n_gpus):
    """Two equal-window jobs -- 100 bases with records and overflowed records, 128 bases with bitmap
    words -- sharded over the contexts of ac_create_multi (all on the one GPU): equal to one context
    and to the oracle; with 5 and 2 windows some shard gets one window and some shard none."""
    for n1, n2 in ((90, 70), (5, 2)):
        km1, w1 = n_windows_case(70 + n1, n1, 100, [0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99))
        km2, w2 = n_windows_case(80 + n2, n2, 128, [2, 0, 3])
        jobs = [(km1, ac.Dna5Sample.from_windows(w1)), (km2, ac.Dna5Sample.from_windows(w2))]
        want = [oracle.count_myers(K, km1, w1), oracle.count_myers(K, km2, w2)]
        assert want[0].any() and want[1].any()
        one = counter.count_jobs(K, jobs)
        assert kernel_of(counter) == BITSLICE
        with ac.ApproxCounter(n_gpus=n_gpus) as multi:
            got = multi.count_jobs(K, jobs)
            assert kernel_of(multi) == BITSLICE and multi.stage_mode() == 0
        for j in range(2):
            assert np.array_equal(got[j], want[j]) and np.array_equal(one[j], want[j]), (n1, n2, j)
