"""GPU parity of the bit-sliced count kernel (bs_count.inc) for the pattern lengths above
16 in AC_BS_K_LIST: every case goes through the C ABI, is compared bit-exactly with the CPU oracle
(oracle.count_myers; large samples through a dictionary, tests/cases.py) and asserts with
ac_testing_last_count_kernel which count kernel the launch ran -- the bit-sliced one, or the
word-parallel one when the run sets AC_BITSLICE=0.

Every list of cases is written over the k in AC_BS_K_LIST (tests/test_bs_nfa_k.py LISTED_K): a k taken
off the list takes its cases with it.  The geometry these shapes aim at: a candidate group is 256
candidates whatever k is (the word-parallel kernel's groups are 64 or 128 for k >= 17); a group of n
candidates takes max(2, next_pow2(ceil(n / 32))) lanes per window; a window's slot is ceil32(L) bases,
with an inline N record where the slot has 10 bits or more to spare, else N-bitmap words."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from tests import cases
from tests.test_bs_nfa_k import LISTED_K, all_t_case, shared_prefix_case
from tests.test_gpu_bitslice import (AC_TESTING_ALL_AHEAD, AC_TESTING_DEVICE_PACK, BITSLICE, WORD, device_count,
                                     equal_case, hooks, kernel_of)
from tests.test_gpu_bs_routes import Reach, bs_rows, chunk_of, rows_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_K = [k for k in LISTED_K if k > 16]
EDGE_K = [k for k in (22, 32) if k in LISTED_K]
K22 = [k for k in (22,) if k in LISTED_K]
GEOMETRY = bool(BITSLICE) and "AC_BS_WAVES_PCT" not in os.environ


def both_routes(counter, k, km, w, what=None):
    """The case through ac_error_count_jobs (the staged instantiation) and through ac_error_count_device
    with window_len (the plain one), against the oracle."""
    want = oracle.count_myers(k, km, w)
    got = counter.count_jobs(k, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE, what
    assert np.array_equal(got, want), what
    got = device_count(counter, k, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE, what
    assert np.array_equal(got, want), what
    return want


@pytest.mark.parametrize("k", NEW_K)
def test_every_listed_k_staged_and_plain(counter, k):
    """300 candidates (groups of 256 and 44: 8 and 2 lanes per window), 37 windows of 100 bases (a
    partial last row at both row sizes), 1 % N."""
    km, w = equal_case(1000 + k, 300, 37, 100, k=k)
    assert both_routes(counter, k, km, w).any()


def edge_lengths(k):
    return sorted({k - 2, k - 1, k, k + 1, 31, 32, 33, 150, 151, 255, 256})


@pytest.mark.parametrize("k,L", [(k, L) for k in EDGE_K for L in edge_lengths(k)])
def test_window_lengths(counter, k, L):
    """Lengths around k, the 32-base slot steps and the 256-base limit at 2 % N: inline N records (and
    overflowed ones) where the slot has room, N-bitmap words elsewhere and on the resident image."""
    km, w = equal_case(2000 + 300 * k + L, 100, 70, L, p_n=0.02, k=k)
    both_routes(counter, k, km, w)


@pytest.mark.parametrize("k,n_kmers", [(k, n) for k in EDGE_K for n in (1, 32, 33, 65, 129, 256, 257, 513)])
def test_candidate_counts(counter, k, n_kmers):
    """Candidate counts at the lanes-per-window steps and around the group size of 256 (257 and 513: a
    last group of one candidate)."""
    km, w = equal_case(3000 + 600 * k + n_kmers, n_kmers, 37, 100, k=k)
    both_routes(counter, k, km, w)


@pytest.mark.parametrize("k,n_windows", [(k, n) for k in EDGE_K for n in (1, 7, 8, 9, 31, 33)])
def test_window_counts(counter, k, n_windows):
    """One window, and counts below / at / above a row of 8 (300 candidates) and of 32 (40 candidates)."""
    for n_kmers in (300, 40):
        km, w = equal_case(4000 + 40 * k + n_windows, n_kmers, n_windows, 101, k=k)
        both_routes(counter, k, km, w, n_kmers)


def padded(wins, L, fill):
    return [(w + fill * L)[:L] for w in wins]


@pytest.mark.parametrize("k", EDGE_K)
def test_candidates_sharing_their_first_16_bases(counter, k):
    """Candidates that differ only past the table build's first pass of 16 positions (at 16, at k - 1)."""
    km, wins = shared_prefix_case(k)
    w = padded(wins, k + 24, "A")
    want = both_routes(counter, k, np.array(km, np.uint64), w)
    assert len(set(want.tolist())) > 1


@pytest.mark.parametrize("k", EDGE_K)
def test_the_all_t_kmer_and_a_first_base_t(counter, k):
    """The all-T k-mer -- at k = 32 all 64 bits of the k-mer word -- and a k-mer whose first base is T."""
    km, wins = all_t_case(k)
    w = padded(wins, 64, "C")
    want = both_routes(counter, k, np.array(km, np.uint64), w)
    assert want[0] > 0 and want[2] > 0


def fitting_waves(counter, k):
    """The waves of a bit-sliced launch of one row: every workgroup that fits for this k."""
    text = "ACGTACGTTGCAAGCTGATTACAGGCATTCAG"[:k]
    km = np.array([cases.kmer_value(text)] * 3, np.uint64)
    got = device_count(counter, k, [(km, [text])])[0]
    assert list(got) == [3] * 3
    return text, km, int(counter.last_launch()["waves"])


@pytest.mark.parametrize("k", EDGE_K)
def test_counter_flush_threshold_on_the_device(counter, k):
    """12 rows per launched wave on average, every window adding 3 to every candidate: some wave counts
    past the 10 rows its bit planes hold and has to flush at the threshold.  On a resident image."""
    import torch

    text, km, waves = fitting_waves(counter, k)
    assert kernel_of(counter) == BITSLICE
    w = np.tile(ac.to_dna5(text), (12 * waves * 32, 1))
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    counter.count_device(k, [seg], window_len=[k])
    torch.cuda.synchronize()
    counter.check()
    assert kernel_of(counter) == BITSLICE
    if GEOMETRY:  # above 1.25 rounds every workgroup that fits is launched, at any residency
        assert counter.last_launch()["waves"] == waves
    assert list(seg.counts_numpy()) == [3 * len(w)] * 3


# ---- k = 22: the routes ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", K22)
def test_two_fused_ends_through_every_entry(counter, k):
    """Both read ends in one launch (150 and 151 bases, 500 and 37 candidates): ac_error_count_device,
    ac_error_count_jobs with a heap sample and with a pinned one packed on the device,
    ac_error_count_samples."""
    a = equal_case(5021, 500, 150, 150, k=k)
    b = equal_case(5022, 37, 90, 151, k=k)
    want = [oracle.count_myers(k, *a), oracle.count_myers(k, *b)]
    assert want[0].any() and want[1].any()

    def same(got):
        assert kernel_of(counter) == BITSLICE
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    same(device_count(counter, k, [a, b]))
    same(counter.count_jobs(k, [a, b]))
    with hooks(AC_TESTING_DEVICE_PACK):
        got = counter.count_jobs(k, ac.Jobs([(km, ac.Dna5Sample.from_windows(w).pinned()) for km, w in (a, b)]))
        assert counter.stage_mode() == 3
    same(got)
    da = counter.upload_sample(ac.pack_windows(a[1]), 0)
    db = counter.upload_sample(ac.pack_windows(b[1]), 1)
    same(counter.count_samples(k, [(a[0], da), (b[0], db)]))


@pytest.mark.parametrize("k", K22)
def test_ragged_windows_keep_the_word_parallel_kernel(counter, k):
    km, w = cases.planted_case(5077, k, 120, 60, win_len=(90, 110), p_n=0.01)
    got = counter.count_jobs(k, [(km, w)])[0]
    assert kernel_of(counter) == WORD
    assert np.array_equal(got, oracle.count_myers(k, km, w))
    # one equal and one ragged job: the launch as a whole stays on the word-parallel kernel, its groups 128
    a = equal_case(5078, 300, 50, 100, k=k)
    got = counter.count_jobs(k, [a, (km, w)])
    assert kernel_of(counter) == WORD
    assert np.array_equal(got[0], oracle.count_myers(k, *a)) and np.array_equal(got[1], oracle.count_myers(k, km, w))


@pytest.mark.parametrize("k", K22)
def test_tagged_early_launch_group_words(counter, k):
    """700 candidates through a synchronous ac_error_count_jobs call (an early launch with tagged
    completion: the host polls one error word per candidate group): 3 groups of 256 for the bit-sliced
    launch, where the word-parallel kernel's 128-candidate groups are 6.  The plan and the launch must
    count the same groups, or the host waits for words that never come or misses some."""
    km, w = equal_case(5700, 700, 90, 100, k=k)
    got = counter.count_jobs(k, [(km, ac.Dna5Sample.from_windows(w))])[0]
    assert counter.stage_mode() == 2, counter.stage_mode()
    assert kernel_of(counter) == BITSLICE
    if BITSLICE:
        assert counter.last_launch()["groups"] == 3
    counter.check()
    assert np.array_equal(got, oracle.count_myers(k, km, w))
    # and again (the other staging slot, the group words of the call before still in it)
    got = counter.count_jobs(k, [(km, ac.Dna5Sample.from_windows(w[:50]))])[0]
    counter.check()
    assert np.array_equal(got, oracle.count_myers(k, km, w[:50]))


@pytest.mark.parametrize("k", K22)
def test_cfg5_shape_cut_down(counter, k):
    """The benchmark's k = 22 configuration cut to 1,000 candidates x 2 ends x 1,000 windows of 150 and
    151 bases."""
    a = equal_case(5501, 1000, 1000, 150, k=k)
    b = equal_case(5502, 1000, 1000, 151, k=k)
    got = counter.count_jobs(k, [a, b])
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got[0], oracle.count_myers(k, *a, 16)) and np.array_equal(got[1], oracle.count_myers(k, *b, 16))


# ---- k = 22 in child processes (settings read once per process) -----------------------------------

def run_child(call, **env):
    code = f"from tests.test_gpu_bitslice_k import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def child_items_one_percent(k, fit, geometry):
    """1 % of the waves that fit: work items of 1, 2 and 8 rows with a partial last item and a partial
    last row on a resident image, of 2 rows staged (windows with inline N records)."""
    W = max(4, fit // 100 // 4 * 4)
    with ac.ApproxCounter(0) as c:
        r = Reach(c, geometry)
        km, texts, per = cases.dictionary_case(2, 40, 30, n_per_text=cases.SHORT_N, k=k)
        for chunk in (1, 2, 8):
            rows = rows_for(W, chunk)
            w, want = cases.dictionary_sample(texts, per, 32 * rows - 5, chunk)
            assert bs_rows(40, len(w)) == rows and chunk_of(rows, W) == chunk
            r.same(("one group", chunk), device_count(c, k, [(km, w)])[0], want)
            r.planned(f"resident, one group, chunk {chunk}", W, chunk)
        km, texts, per = cases.dictionary_case(3, 40, 100, k=k)
        w, want = cases.dictionary_sample(texts, per, 32 * rows_for(W, 2) - 5, 12)
        got = c.count_jobs(k, [(km, ac.Dna5Sample.from_windows(w))])[0]
        assert c.stage_mode() == 2, c.stage_mode()
        r.same("staged", got, want)
        r.planned("staged, chunk 2", W, 2)


@pytest.mark.parametrize("k", K22)
def test_multi_row_items(counter, k):
    fit = fitting_waves(counter, k)[2]
    out = run_child(f"child_items_one_percent({k}, {fit}, {GEOMETRY})", AC_BS_WAVES_PCT="1")
    print(out)
    if GEOMETRY:
        assert "reached resident, one group, chunk 8" in out and "reached staged, chunk 2" in out


def child_dma_path(k):
    """ac_error_count_jobs without the early launch (ac_stage_mode 0): the copy engine moves the jobs and
    the plain instantiation reads inline N records.  One part: records, overflowed records (100 bases)
    and bitmap words (128 bases), 300 and 37 candidates; two parts (>= 2^17 windows: part 0 runs with
    half the waves of its kernel)."""
    with ac.ApproxCounter(0) as c:
        r = Reach(c, False)
        a = cases.dictionary_case(3, 300, 100, k=k)
        assert ((a[1] == 4).sum(axis=1) >= 5).any()  # records that overflow
        wa, want_a = cases.dictionary_sample(a[1], a[2], 900, 1)
        km2, w2 = equal_case(5031, 37, 500, 128, p_n=0.02, k=k)
        got = c.count_jobs(k, ac.Jobs([(a[0], ac.Dna5Sample.from_windows(wa)), (km2, ac.Dna5Sample.from_windows(w2))]))
        assert c.stage_mode() == 0, c.stage_mode()
        r.same("one part, records", got[0], want_a)
        r.same("one part, bitmap", got[1], oracle.count_myers(k, km2, w2, 16))
        print("reached one part, stage mode 0", flush=True)
        d = cases.dictionary_case(2, 40, 30, n_per_text=cases.SHORT_N, k=k)
        w, want = cases.dictionary_sample(d[1], d[2], (1 << 17) + 777, 3)
        got = c.count_jobs(k, ac.Jobs([(d[0], ac.Dna5Sample.from_windows(w))]))
        assert c.stage_mode() == 0, c.stage_mode()
        r.same("two parts", got[0], want)
        print("reached 2 parts, stage mode 0", flush=True)


@pytest.mark.parametrize("k", K22)
def test_dma_path(k):
    out = run_child(f"child_dma_path({k})", AC_STAGE_EARLY="0")
    print(out)
    assert "reached one part" in out and "reached 2 parts" in out
