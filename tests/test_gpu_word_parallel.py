"""GPU parity of the word-parallel count kernel (wm2_count_kernel<P, STAGED, EQ>: wm_count.hip,
wm_window_loop.inc, count_frame.inc, wm_tid_blocks.inc) on the equal-window launches it still serves:
k = 2..15 and 17, windows longer than one 256-base fetch at any k, and every k under AC_BITSLICE=0.
One k per pack factor P (WP_K = 8, 10, 15, 17 for P = 4, 3, 2, 1), the staged instantiation (the early
launch of ac_error_count_jobs, inline N records) and the plain one (ac_error_count_device on a resident
image; with records, the DMA path of a child process under AC_STAGE_EARLY=0).

Every count is compared bit for bit with the CPU oracle -- directly, or for large samples through a
dictionary (tests/cases.py) -- and every launch asserts ac_testing_last_count_kernel == 0, so that a
later change of the routing cannot move these cases to another kernel unnoticed.  No in-process case
depends on AC_BITSLICE.  The cases come from tests/word_cases.py; tests/test_word_cases.py shows on the
CPU that each has the property its test here relies on."""
import os
import subprocess
import sys

import pytest

import approx_counter_amd as ac
import oracle
from tests import cases
from tests import word_cases as wc
from tests.test_gpu_bitslice import AC_TESTING_ALL_AHEAD, AC_TESTING_DEVICE_PACK, device_count, hooks, kernel_of
from tests.test_gpu_bs_routes import Reach, chunk_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD = 0  # ac_testing_last_count_kernel: the word-parallel kernel


def same(counter, what, got, want):
    Reach(counter, True).same(what, got, want, kernel=WORD)


def staged_counts(counter, k, km, w, mode=2):
    """ac_error_count_jobs on a heap sample: the staged instantiation (early launch, stage mode 2)."""
    got = counter.count_jobs(k, [(km, w if isinstance(w, ac.Dna5Sample) else ac.Dna5Sample.from_windows(w))])[0]
    assert counter.stage_mode() == mode, counter.stage_mode()
    counter.check()
    return got


def staged_and_plain(counter, k, km, w, want, what):
    same(counter, (what, "staged"), staged_counts(counter, k, km, w), want)
    same(counter, (what, "plain"), device_count(counter, k, [(km, w)])[0], want)


def run_child(call, **env):
    code = f"from tests.test_gpu_word_parallel import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def record_calls(c, k, L, flags=0, mode=2, reps=2):
    """The record jobs (word_cases.record_jobs: four) in one call, `reps` times (both staging slots)."""
    jobs = wc.record_jobs(k, L)
    call = ac.Jobs([(km, ac.Dna5Sample.from_windows(w)) for km, w, _ in jobs])
    for rep in range(reps):
        with hooks(flags):
            got = c.count_jobs(k, call)
        assert c.stage_mode() == mode, c.stage_mode()
        c.check()
        for j, (_, _, want) in enumerate(jobs):
            same(c, ("records", k, L, "job", j, "call", rep), got[j], want)


# ---- 1: every EQ instantiation, staged and plain ----

@pytest.mark.parametrize("k", wc.WP_K)
def test_every_instantiation_staged_and_plain(counter, k):
    """300 candidates (more than one group at every P but 2 and 4, a partial last lane word) over 37
    windows of 100 bases: <P, staged, eq> with inline N records, <P, plain, eq> with N-bitmap words."""
    km, w, want = wc.basic_case(k)
    staged_and_plain(counter, k, km, w, want, ("basic", k))


def child_plain_with_records():
    """AC_STAGE_EARLY=0: ac_error_count_jobs sends the jobs with the copy engine (stage mode 0) and the
    plain instantiation reads the inline N records -- the basic case and the record jobs of 100 bases
    (records at capacity, overflowed records with and without other N-holders) at every P."""
    with ac.ApproxCounter(0) as c:
        for k in wc.WP_K:
            km, w, want = wc.basic_case(k)
            same(c, ("dma, basic", k), staged_counts(c, k, km, w, mode=0), want)
            record_calls(c, k, 100, mode=0, reps=1)
            print(f"reached plain with records, k {k}: stage mode {c.stage_mode()} kernel {kernel_of(c)}", flush=True)


def test_plain_instantiation_with_records():
    out = run_child("child_plain_with_records()", AC_STAGE_EARLY="0")
    print(out)
    for k in wc.WP_K:
        assert f"reached plain with records, k {k}: stage mode 0 kernel 0\n" in out


# ---- 2: window lengths ----

@pytest.mark.parametrize("k,L", [(k, L) for k in wc.EDGE_K for L in wc.lengths_for(k)])
def test_window_lengths(counter, k, L):
    """Lengths below and at the shortest occurrence (k - 3: no count at all; k - 2: the whole window is one
    at 2 edits), around the 16-base chunks, the first 32-base block (whose hit accumulation k = 15 and
    17 skip over bases 0..11: the first window's occurrence ends at base k - 3), an odd chunk count,
    every record capacity (nrec.h: 4, 4, 0, 0, 3, 2, 1 at 100, 101, 127, 128, 129, 150, 151) and the
    second fetch segment (257 and up; no record)."""
    km, w, want = wc.length_case(k, L)
    staged_and_plain(counter, k, km, w, want, ("length", k, L))


@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("L", wc.LONG_L)
def test_long_windows_at_the_bit_sliced_ks(counter, k, L):
    """Equal windows longer than one 256-base fetch go to the word-parallel kernel at k = 16 and 22 too."""
    km, w, want = wc.length_case(k, L)
    staged_and_plain(counter, k, km, w, want, ("long", k, L))


# ---- 3: inline N records ----

@pytest.mark.parametrize("k", wc.WP_K)
@pytest.mark.parametrize("L", wc.RECORD_L)
def test_inline_n_records(counter, k, L):
    """The three jobs of test_gpu_jobs.py::test_inline_n_records at this kernel's k: records that hold
    0..cap N, records at capacity, overflowed records (the bitmap fetch inside the window loop, after
    the gated wait for the whole segment), a job whose only N-holders overflow, an N-free job; N on the
    N-mask words' edges (0, 15, 16, 31, 32, 63).  A fourth job's records hold one or two N at every one of
    the spots 0, 15, 16, 31, 32, 63, 64, L - 1: each N-mask word and both position widths (7 and 8 bits)."""
    record_calls(counter, k, L)


@pytest.mark.parametrize("k", wc.EDGE_K)
def test_inline_n_records_all_sent_ahead(counter, k):
    """The same jobs with every job sent ahead of the launch (AC_TESTING_ALL_AHEAD): resident input to
    the staged instantiation, no wait."""
    record_calls(counter, k, 100, flags=AC_TESTING_ALL_AHEAD)


# ---- 4: candidate-group and window-count edges ----

@pytest.mark.parametrize("k,n_kmers", [(k, n) for k in wc.WP_K for n in wc.CAND_COUNTS[k]])
def test_candidate_counts_at_the_group_edges(counter, k, n_kmers):
    """One candidate, a partial first lane word, one below / at / above the staged group size (for P = 1
    the plain one too) and one above twice it; the first and the last candidate expect hits."""
    km, w, want = wc.group_case(k, n_kmers)
    staged_and_plain(counter, k, km, w, want, ("candidates", k, n_kmers))
    assert counter.last_launch()["groups"] == wc.groups_of(k, n_kmers, False)


def test_tagged_early_launch_group_words(counter):
    """700 candidates at k = 17 through a synchronous ac_error_count_jobs call: the host polls one tagged
    error word per candidate group, 6 groups of 128 for the staged P = 1 kernel (11 plain ones).  Then
    the other staging slot, the words of the call before still in it."""
    km, w, want = wc.group_case(17, 700, 90)
    same(counter, "700 candidates", staged_counts(counter, 17, km, w), want)
    assert counter.last_launch()["groups"] == 6
    same(counter, "700 candidates, 50 windows", staged_counts(counter, 17, km, w[:50]),
         oracle.count_myers(17, km, w[:50]))


@pytest.mark.parametrize("k", wc.WP_K)
@pytest.mark.parametrize("n_windows", wc.WINDOW_COUNTS)
def test_window_counts(counter, k, n_windows):
    km, w, want = wc.group_case(k, 300, n_windows, 101)
    staged_and_plain(counter, k, km, w, want, ("windows", k, n_windows))


# ---- 5: work items of more than one window ----

def resident_waves(counter, k, staged):
    """The waves of a launch of this instantiation with fewer items than fit: all that are resident."""
    km, w, want = wc.basic_case(k)
    got = staged_counts(counter, k, km, w) if staged else device_count(counter, k, [(km, w)])[0]
    same(counter, ("small launch", k), got, want)
    geo = counter.last_launch()
    assert geo["groups"] * len(w) < geo["waves"] and geo["waves"] % 4 == 0, geo
    return int(geo["waves"])


@pytest.mark.parametrize("k,n_kmers", [(17, 640), (15, 1300)])
@pytest.mark.parametrize("chunk", [1, 2, 3, 8])
def test_multi_window_items_resident(counter, k, n_kmers, chunk):
    """Items of 1, 2, 3 and 8 windows of 20 bases on a resident image: 13 + 64 x chunk items per resident
    wave, so every wave goes on from its static item to claimed and stolen ones; the window count is no
    multiple of chunk (a partial last item per group).  At chunk 8 a P <= 2 wave counts ~600 windows."""
    W = resident_waves(counter, k, False)
    km, texts, per = wc.item_dictionary(k, n_kmers, 20)
    groups = wc.groups_of(k, n_kmers, False)
    n = wc.item_windows(W, chunk, groups)
    w, want = cases.dictionary_sample(texts, per, n, chunk)
    r = Reach(counter, True)
    r.same(("resident", k, chunk), device_count(counter, k, [(km, w)])[0], want, kernel=WORD)
    r.planned(f"resident, k {k}, {groups} groups x {n} windows, chunk {chunk}", W, chunk)


@pytest.mark.parametrize("k,n_kmers", [(17, 1300), (10, 2600)])
@pytest.mark.parametrize("chunk", [2, 8])
def test_multi_window_items_staged(counter, k, n_kmers, chunk):
    """Items of 2 and 8 windows of 100 bases through the early launch: records, and records that overflow,
    so the wait for the whole segment happens inside an item."""
    W = resident_waves(counter, k, True)
    km, texts, per = wc.item_dictionary(k, n_kmers, 100)
    assert ((texts == 4).sum(axis=1) > wc.nrec_cap(100)).any()  # records that overflow
    groups = wc.groups_of(k, n_kmers, True)
    n = wc.item_windows(W, chunk, groups)
    w, want = cases.dictionary_sample(texts, per, n, 10 + chunk)
    r = Reach(counter, True)
    r.same(("staged", k, chunk), staged_counts(counter, k, km, ac.Dna5Sample.from_windows(w)), want, kernel=WORD)
    r.planned(f"staged, k {k}, {groups} groups x {n} windows, chunk {chunk}", W, chunk)


def test_multi_window_items_two_fused_segments(counter):
    """Two segments of different candidate counts (640 and 40), window lengths (20 and 33) and window counts
    (10 : 1) in one launch at chunk 2, neither count a multiple of 2."""
    k = 17
    W = resident_waves(counter, k, False)
    a, b = wc.item_dictionary(k, 640, 20), wc.item_dictionary(k, 40, 33)
    ga, gb = wc.groups_of(k, 640, False), wc.groups_of(k, 40, False)
    na, nb = wc.fused_windows(W, 2, ga, gb)
    wa, want_a = cases.dictionary_sample(a[1], a[2], na, 6)
    wb, want_b = cases.dictionary_sample(b[1], b[2], nb, 7)
    assert chunk_of(ga * na + gb * nb, W) == 2
    got = device_count(counter, k, [(a[0], wa), (b[0], wb)])
    r = Reach(counter, True)
    r.same("fused, first", got[0], want_a, kernel=WORD)
    r.same("fused, second", got[1], want_b, kernel=WORD)
    r.planned(f"resident, two fused segments of {na} and {nb} windows, chunk 2", W, 2)


# ---- 6: device packing ----

def packed_counts(counter, k, km, sample):
    """ac_error_count_jobs on a pinned sample that the copier workgroups pack (stage mode 3)."""
    with hooks(AC_TESTING_DEVICE_PACK):
        got = counter.count_jobs(k, ac.Jobs([(km, sample.pinned())]))[0]
        mode = counter.stage_mode()
    print(f"stage mode {mode}", flush=True)
    assert mode == 3, mode
    counter.check()
    return got


@pytest.mark.parametrize("k", wc.PACK_K)
@pytest.mark.parametrize("L", wc.PACK_L)
def test_device_pack_slot_shapes(counter, k, L):
    """1,500 windows with 2 % N packed on the device: slots with a record (33, 100, 101, 151) and without
    (128, 256), the records written by the copier workgroups and read by this kernel."""
    km, w, want = wc.pack_case(k, L)
    same(counter, ("device pack", k, L), packed_counts(counter, k, km, ac.Dna5Sample.from_windows(w)), want)


@pytest.mark.parametrize("k", wc.PACK_K)
def test_device_pack_record_overflow_and_n_runs(counter, k):
    """6 % N, an all-N window, a run of 40 N, N at both ends, N bytes of 4, 5, 77 and 255."""
    km, w, sample, want = wc.pack_overflow_case(k)
    same(counter, ("device pack, overflow", k), packed_counts(counter, k, km, sample), want)


@pytest.mark.parametrize("k", [15, 17])
@pytest.mark.parametrize("n_windows,L", wc.TAIL_SHAPES)
def test_device_pack_block_tail(counter, k, n_windows, L):
    """Blocks of 151, 202, 450 and (the control) 100 bytes whose last bytes end an occurrence."""
    km, w = wc.tail_case(k, n_windows, L)
    want = oracle.count_myers(k, km, w)
    assert list(want) == [3 * n_windows, 0]
    same(counter, ("device pack, tail", k, n_windows, L), packed_counts(counter, k, km, ac.Dna5Sample.from_windows(w)),
         want)


# ---- 7: the word-parallel kernel at the bit-sliced kernel's k values (a child with AC_BITSLICE=0) ----

def child_bitslice_off():
    """AC_BITSLICE=0 keeps every launch on the word-parallel kernel: k = 16 and 22 (the benchmark's two)
    on the basic case, staged and plain, the record jobs of 100 and 151 bases, and a device-packed call."""
    with ac.ApproxCounter(0) as c:
        for k, L in ((16, 100), (22, 151)):
            km, w, want = wc.basic_case(k)
            staged_and_plain(c, k, km, w, want, ("bitslice off, basic", k))
            record_calls(c, k, L)
            km, w, want = wc.pack_case(k, L)
            same(c, ("bitslice off, device pack", k), packed_counts(c, k, km, ac.Dna5Sample.from_windows(w)), want)
            print(f"reached bitslice off, k {k}: kernel {kernel_of(c)}", flush=True)


def test_word_parallel_kernel_with_bitslice_off():
    out = run_child("child_bitslice_off()", AC_BITSLICE="0")
    print(out)
    assert "reached bitslice off, k 16: kernel 0\n" in out and "reached bitslice off, k 22: kernel 0\n" in out
    assert out.count("stage mode 3\n") == 2
