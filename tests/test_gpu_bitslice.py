"""GPU parity of the bit-sliced count kernel (approx_counter_amd/csrc/bs_count.inc):
k = 16, equal windows of at most 256 bases.  Every case goes through the C ABI, is compared
bit-exactly with the CPU oracle (oracle.count_myers), and asserts with the test-only query
ac_testing_last_count_kernel which count kernel the launch ran.

The kernel's geometry, for the shapes below: a candidate group is 256 candidates; a group of n
candidates takes LW = max(2, next_pow2(ceil(n / 32))) <= 8 lanes per window, and a wave counts a row
of 64 / LW consecutive windows; a wave's bit-plane counters hold VC_WINDOWS = 10 rows between
flushes (bs_nfa.h)."""
import os

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases

pytestmark = pytest.mark.gpu
K = 16
# the kernel a qualifying launch must report: the bit-sliced one, unless the run keeps every launch on
# the word-parallel kernel (AC_BITSLICE=0: a run done by hand, which no default run makes -- the default
# run's tests of that kernel's equal-window code are tests/test_gpu_word_parallel.py)
WORD, BITSLICE = 0, (0 if os.environ.get("AC_BITSLICE", "1") == "0" else 1)
AC_TESTING_ALL_AHEAD, AC_TESTING_DEVICE_PACK = 2, 8


def kernel_of(counter):
    return int(_lib.load().ac_testing_last_count_kernel(counter.handle))


class hooks:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.prev = _lib.load().ac_testing_stage_hooks(self.flags)

    def __exit__(self, *exc):
        _lib.load().ac_testing_stage_hooks(self.prev)


def equal_case(seed, n_kmers, n_windows, L, p_n=0.01, k=K):
    km, w = cases.planted_case(seed, k, n_kmers, n_windows, win_len=(L, L), p_n=p_n)
    return km, [(x + "A" * L)[:L] for x in w]  # truly equal (a planted occurrence may grow a window)


def device_count(counter, k, parts, accumulate=False):
    """ac_error_count_device with window_len over resident images (no inline N records: the windows' N
    bits are their N-bitmap words); returns the segments, counts in device memory."""
    import torch

    packed = [ac.pack_windows(w) for _, w in parts]
    lens = [p.equal_window_len() for p in packed]
    segs = [ac.DeviceSegment.upload(km, p) for (km, _), p in zip(parts, packed)]
    for _ in range(2 if accumulate else 1):
        counter.count_device(k, segs, window_len=lens, accumulate=accumulate)
    torch.cuda.synchronize()
    counter.check()
    return [s.counts_numpy() for s in segs]


@pytest.mark.parametrize("n_kmers", [1, 31, 32, 33, 64, 65, 128, 129, 500, 512, 513, 2047, 2048, 2049])
def test_candidate_counts_at_every_lane_edge(counter, n_kmers):
    """Candidate counts around every lanes-per-window step (32 | 64: 2 lanes, 65..128: 4, 129..256: 8) and
    around the group size (256: 500, 512, 513 are 2-3 groups, 2047..2049 are 8-9, the last group of
    513 and 2049 holding one candidate); 37 windows leave a partial last row at every row size."""
    km, w = equal_case(n_kmers, n_kmers, 37, 100)
    got = counter.count_jobs(K, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got, oracle.count_myers(K, km, w))


@pytest.mark.parametrize("n_windows", [1, 7, 8, 9, 31, 33, 65])
def test_window_counts_with_partial_rows(counter, n_windows):
    """One window, and counts one below / at / above a row of 8 (300 candidates: 8 lanes per window and
    4 for the second group's 44) and of 32 (40 candidates: 2 lanes)."""
    for n_kmers in (300, 40):
        km, w = equal_case(50 + n_windows, n_kmers, n_windows, 101)
        got = counter.count_jobs(K, [(km, w)])[0]
        assert kernel_of(counter) == BITSLICE
        assert np.array_equal(got, oracle.count_myers(K, km, w)), n_kmers


@pytest.mark.parametrize("L", [14, 15, 16, 17, 31, 32, 33, 100, 101, 127, 128, 129, 255, 256])
def test_window_lengths(counter, L):
    """Lengths at the 16-base chunk, 128-base and 256-base slot boundaries, 2 % N: through the jobs
    stage (inline N records where the slot has room: 14..17, 100, 101; the N bitmap elsewhere) and
    through ac_error_count_device on a resident image (N bitmap words for every window)."""
    km, w = equal_case(300 + L, 100, 70, L, p_n=0.02)
    want = oracle.count_myers(K, km, w)
    got = counter.count_jobs(K, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got, want)
    got_dev = device_count(counter, K, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE
    assert np.array_equal(got_dev, want)


def n_windows_case(seed, n, L, counts, spots=()):
    """n equal windows of L random bases as a 2-D Dna5 array; window i holds counts[i % len(counts)] N
    bases, the first at `spots`, the rest at random places; and 60 k-mers cut from the windows."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    for i in range(n):
        c = min(L, counts[i % len(counts)])
        pos = [p for p in spots if p < L][:c]
        free = np.setdiff1d(np.arange(L), pos)
        pos += list(rng.choice(free, size=c - len(pos), replace=False))
        w[i, pos] = 4
    km = []
    for _ in range(60):
        row = w[int(rng.integers(n))]
        s0 = int(rng.integers(0, L - K + 1))
        v = 0
        for b in row[s0:s0 + K]:
            v = (v << 2) | (int(b) if b < 4 else int(rng.integers(4)))
        km.append(v)
    return np.array(km, np.uint64), w


@pytest.mark.parametrize("name,counts,spots", [
    ("no_n", [0], ()),
    ("n_in_every_window", [1, 2, 3, 4], ()),
    ("n_at_first_and_last_base", [2], (0, 99)),
    ("all_n_window_among_clean", [0, 0, 0, 100], ()),
    ("records_overflow", [0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99)),
])
def test_n_cases_staged_and_resident(counter, name, counts, spots):
    """N nowhere, in every window, at base 0 and at the last base, an all-N window, and records that
    overflow (5+ N in a 100-base window: those windows read their N-bitmap words) -- staged (the early
    launch counts windows as they arrive and waits for the whole segment on an overflowed record) and,
    with every job sent ahead of the launch (AC_TESTING_ALL_AHEAD), on resident input."""
    km, w = n_windows_case(len(name), 90, 100, counts, spots)
    want = oracle.count_myers(K, km, w, 16)
    for flags in (0, AC_TESTING_ALL_AHEAD):
        with hooks(flags):
            got = counter.count_jobs(K, [(km, ac.Dna5Sample.from_windows(w))])[0]
        assert kernel_of(counter) == BITSLICE
        assert np.array_equal(got, want), flags


def test_shifted_and_duplicate_candidates(counter):
    """Candidates that are one-base shifts of each other (neighbouring bits of a lane word must not
    leak into each other) and duplicates (equal columns of the ~Eq table)."""
    rng = np.random.default_rng(3)
    text = "".join("ACGT"[i] for i in rng.integers(0, 4, size=80))
    shifts = [cases.kmer_value(text[i:i + K]) for i in range(40)]
    km = np.array(shifts + shifts[:10] + [shifts[0]] * 5, np.uint64)
    w = [(text[i:] + text)[:100] for i in range(0, 60, 3)] + ["A" * 100, text[:50] * 2]
    got = counter.count_jobs(K, [(km, w)])[0]
    assert kernel_of(counter) == BITSLICE
    want = oracle.count_myers(K, km, w)
    assert want.sum() > 0
    assert np.array_equal(got, want)


def test_two_fused_ends_through_every_entry(counter):
    """Both read ends in one launch, with different candidate counts (500 and 37: 8 and 2 lanes per
    window) and lengths (100 / 101): ac_error_count_device with window_len, plain and accumulating
    (AC_DEVICE_ACCUMULATE, twice: double the counts); ac_error_count_jobs with a heap sample; with a
    pinned sample packed on the device (AC_TESTING_DEVICE_PACK); ac_error_count_jobs_submit."""
    import torch

    a = equal_case(21, 500, 150, 100)
    b = equal_case(22, 37, 90, 101)
    want = [oracle.count_myers(K, *a), oracle.count_myers(K, *b)]

    def same(got, times=1):
        assert kernel_of(counter) == BITSLICE
        assert np.array_equal(got[0], times * want[0]) and np.array_equal(got[1], times * want[1])

    same(device_count(counter, K, [a, b]))
    same(device_count(counter, K, [a, b], accumulate=True), 2)
    same(counter.count_jobs(K, [a, b]))
    with hooks(AC_TESTING_DEVICE_PACK):
        got = counter.count_jobs(K, ac.Jobs([(km, ac.Dna5Sample.from_windows(w).pinned()) for km, w in (a, b)]))
        assert counter.stage_mode() == 3
    same(got)
    jobs = ac.Jobs([(km, ac.Dna5Sample.from_windows(w)) for km, w in (a, b)])
    out = torch.full((jobs.n_counts,), 7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(2):  # both staging slots
        counter.submit_jobs(K, jobs, out, stream=st.cuda_stream)
    counter.check(stream=st.cuda_stream)
    flat = out.cpu().numpy().view(np.uint32).astype(np.uint64)
    same([flat[:500], flat[500:]])


def _all_hit(counter, rows_per_wave, L, text):
    """3 equal candidates (2 lanes per window: rows of 32 windows) that hit every window at all three
    levels, over rows_per_wave x (launched waves) rows: (candidates, 2-D Dna5 windows)."""
    km = np.array([cases.kmer_value("ACGTACGTTGCAAGCT")] * 3, np.uint64)
    counter.count_jobs(K, [(km, [text])])
    assert kernel_of(counter) == BITSLICE
    waves = counter.last_launch()["waves"]
    return km, np.tile(ac.to_dna5(text), (rows_per_wave * waves * 32, 1))


def test_waves_claim_several_items(counter):
    """More rows than launched waves: 2 x (launched waves) x 64 windows of 20 bases are 4 rows per
    wave on average, so waves go on from their static first item to claimed (and stolen) ones.  This
    shape does not have to reach the counters' flush threshold (10 rows in one wave); the next one does."""
    km, w = _all_hit(counter, 4, 20, "ACGTACGTTGCAAGCTACGT")
    got = counter.count_jobs(K, [(km, ac.Dna5Sample.from_windows(w))])[0]
    assert kernel_of(counter) == BITSLICE
    assert len(w) // 32 == 4 * counter.last_launch()["waves"]
    assert list(got) == [3 * len(w)] * 3


def test_counter_flush_threshold_on_the_device(counter):
    """12 rows per launched wave on average: whatever the claims' order, some wave counts 12 rows or
    more, past the 10 its bit planes hold, and every window adds 3 to every candidate -- without the
    flush at the threshold its planes would wrap and the total come out short.  On a resident image
    (ac_error_count_device: the windows' N bits come from the bitmap)."""
    import torch

    km, w = _all_hit(counter, 12, 16, "ACGTACGTTGCAAGCT")
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    counter.count_device(K, [seg], window_len=[16])
    torch.cuda.synchronize()
    counter.check()
    assert kernel_of(counter) == BITSLICE
    assert len(w) // 32 == 12 * counter.last_launch()["waves"]
    assert list(seg.counts_numpy()) == [3 * len(w)] * 3


@pytest.mark.parametrize("k", [15, 17])
def test_other_k_keeps_the_word_parallel_kernel(counter, k):
    km, w = equal_case(400 + k, 120, 60, 100, k=k)
    got = counter.count_jobs(k, [(km, w)])[0]
    assert kernel_of(counter) == WORD
    assert np.array_equal(got, oracle.count_myers(k, km, w))


def test_ragged_windows_keep_the_word_parallel_kernel(counter):
    km, w = cases.planted_case(77, K, 120, 60, win_len=(90, 110), p_n=0.01)
    got = counter.count_jobs(K, [(km, w)])[0]
    assert kernel_of(counter) == WORD
    assert np.array_equal(got, oracle.count_myers(K, km, w))
    # one equal and one ragged job in a launch: the launch as a whole stays on the word-parallel kernel
    a = equal_case(78, 100, 50, 100)
    got = counter.count_jobs(K, [a, (km, w)])
    assert kernel_of(counter) == WORD
    assert np.array_equal(got[0], oracle.count_myers(K, *a)) and np.array_equal(got[1], oracle.count_myers(K, km, w))
