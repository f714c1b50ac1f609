"""GPU tests of the edit budget (ac_set_max_errors; DESIGN.md §4e "Edit budget"): M1(E) for E = 0, 1, 3
on every route to the bit-sliced count kernel.  Every case goes through the C ABI, is bit-exact against
count_e (tests/test_budget_cpu.py: the oracle's DP distances, cap E + 1) and asserts that the launch ran
the bit-sliced kernel (ac_testing_last_count_kernel).  With AC_BITSLICE=0 in the environment no launch
is bit-sliced, so the same calls must fail with AC_ERR_INVALID instead: nothing counts at another budget
than the one asked for.

Every E = 3 case holds a window at distance exactly 3 from a candidate wherever its windows are long
enough for one (k - 3 bases), so that its expected counts differ from the E = 2 counts: asserted on the
CPU before the GPU is asked.

Contexts: the budget is sticky, so these tests use contexts of their own and leave the session's
`counter` at the default."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.test_bs_nfa_k import LISTED_K
from tests.test_budget_cpu import count_e
from tests.test_gpu_bitslice import AC_TESTING_DEVICE_PACK, BITSLICE, device_count, equal_case, hooks, kernel_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
CFG1 = os.path.join(ROOT, "tests", "golden", "cfg1")
BS_ON = BITSLICE == 1


@pytest.fixture(scope="module")
def c3():
    with ac.ApproxCounter(0, max_errors=3) as c:
        assert c.max_errors == 3
        yield c


@pytest.fixture(scope="module")
def ce():
    """A context whose budget the E = 0 / 1 tests set."""
    with ac.ApproxCounter(0) as c:
        assert c.max_errors == 2
        yield c


def refused(fn):
    with pytest.raises(_lib.ApproxCounterError) as e:
        fn()
    assert e.value.status == _lib.AC_ERR_INVALID, e.value
    assert "max_errors" in str(e.value)
    return str(e.value)


def budget_case(seed, k, n_kmers, n_windows, L, p_n=0.01):
    """equal_case with, where L >= k - 3, the first windows replaced by candidates at exactly 3 edits:
    candidate 0 with 3 bases deleted (L = k - 3 exactly), or with 3 spaced bases substituted, then random
    bases up to L."""
    km, w = equal_case(seed, n_kmers, n_windows, L, p_n=p_n, k=k)
    if L >= k - 3:
        rng = np.random.default_rng(seed)
        s = cases.kmer_string(km[0], k)
        if L < k:
            cut = sorted(rng.choice(k, size=k - L, replace=False).tolist())
            t = "".join(c for i, c in enumerate(s) if i not in cut)
        else:
            t = list(s)
            for p in (1, k // 2, k - 2):
                t[p] = "ACGT"[("ACGT".index(t[p]) + 1 + int(rng.integers(3))) % 4]
            t = "".join(t) + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L - k))
        w[0] = t
        if n_windows > 2:
            w[n_windows - 1] = t[::-1][:L] if L < k else t[k:] + t[:k]  # (and at the window's end)
    return km, w


def expect(E, k, km, w, differs=True):
    want = count_e(E, k, km, w)
    if E != 2 and differs:
        assert (want != oracle.count_myers(k, km, w)).any(), "no window at a distance that tells the budgets apart"
    return want


def both_routes(c, k, km, w, want, what):
    """count_jobs (the staged instantiation) and count_device with window_len (the plain one)."""
    if not BS_ON:
        refused(lambda: c.count_jobs(k, [(km, w)]))
        refused(lambda: device_count(c, k, [(km, w)]))
        return
    got = c.count_jobs(k, [(km, w)])[0]
    assert kernel_of(c) == 1, what
    np.testing.assert_array_equal(got, want, err_msg=f"{what} staged")
    got = device_count(c, k, [(km, w)])[0]
    assert kernel_of(c) == 1, what
    np.testing.assert_array_equal(got, want, err_msg=f"{what} plain")


def staged_route(c, k, km, w, want, what):
    if not BS_ON:
        refused(lambda: c.count_jobs(k, [(km, w)]))
        return
    got = c.count_jobs(k, [(km, w)])[0]
    assert kernel_of(c) == 1 and c.stage_mode() == 2, what
    np.testing.assert_array_equal(got, want, err_msg=str(what))


# ---- E = 3 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_e3_every_k(c3, k):
    """300 candidates (groups of 256 + 44), 37 windows of 100 bases, 1 % N."""
    km, w = budget_case(1000 + k, k, 300, 37, 100)
    both_routes(c3, k, km, w, expect(3, k, km, w), f"K {k}")


@pytest.mark.parametrize("k", [16, 22, 32])
def test_e3_window_lengths(c3, k):
    """70 windows, 2 % N, at lengths around k (k - 4: no occurrence within 3 edits fits, every count is 0),
    at the 16-base chunk boundary, and 100, 101, 255, 256: inline N records, overflowed records and
    bitmap words all occur across them."""
    for L in sorted({k - 4, k - 3, k, k + 3, 14, 15, 16, 17, 100, 101, 255, 256}):
        km, w = budget_case(2000 + 300 * k + L, k, 100, 70, L, p_n=0.02)
        want = expect(3, k, km, w, differs=L >= k - 3)
        assert want.any() == (L >= k - 3)
        both_routes(c3, k, km, w, want, f"K {k} L {L}")


@pytest.mark.parametrize("k", [16, 32])
def test_e3_candidate_counts(c3, k):
    for n in (1, 33, 256, 257):
        km, w = budget_case(3000 + k + n, k, n, 37, 100)
        staged_route(c3, k, km, w, expect(3, k, km, w), (k, n))


@pytest.mark.parametrize("k", [16, 32])
def test_e3_window_counts(c3, k):
    """One window, and counts below / at / above a row of 8 (300 candidates: 8 lanes per window)."""
    for n in (1, 7, 8, 9):
        km, w = budget_case(4000 + k + n, k, 300, n, 101)
        staged_route(c3, k, km, w, expect(3, k, km, w), (k, n))


def child_flush_threshold():
    """1 % of the waves that fit (AC_BS_WAVES_PCT=1): 24k windows in rows of 32 leave every wave tens of
    rows, so its plane counters flush (every 7 rows at E = 3) many times.  The all-T k-mer on all-T
    windows counts 4 per window; the other candidates (a block of 32 and a partial one) whatever the
    one distinct window gives them."""
    n = 32 * 750 + 5
    with ac.ApproxCounter(0, max_errors=3) as c:
        for k in (16, 32):
            km = [cases.kmer_value("T" * k)] * 2 + cases.planted_case(k, k, 38, 0)[0] + [cases.kmer_value("T" * k)]
            km[5] = cases.kmer_value("T" * (k - 2) + "GT")
            win = "T" * 40
            want = count_e(3, k, km, [win]) * np.uint64(n)
            assert want[0] == 4 * n and want[-1] == 4 * n and want[5] == 3 * n
            w = np.full((n, 40), 3, np.uint8)
            job = [(np.array(km, np.uint64), ac.Dna5Sample.from_windows(w))]
            if not BS_ON:
                refused(lambda: c.count_jobs(k, job))
                continue
            got = c.count_jobs(k, job)[0]
            assert kernel_of(c) == 1 and c.stage_mode() == 2
            rows_per_wave = int(c.last_launch()["windows_per_wave"])
            print(f"K {k}: rows per wave {rows_per_wave}", flush=True)
            assert rows_per_wave > 7
            assert np.array_equal(got, want), (k, got[:8], want[:8])


def run_child(call, **env):
    code = f"from tests.test_gpu_budget import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_e3_flush_threshold():
    print(run_child("child_flush_threshold()", AC_BS_WAVES_PCT="1"))


# ---- E = 0 and 1 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 22, 32])
@pytest.mark.parametrize("E", [0, 1])
def test_e0_e1(ce, E, k):
    ce.set_max_errors(E)
    assert ce.max_errors == E
    km, w = budget_case(5000 + k, k, 300, 37, 100)
    both_routes(ce, k, km, w, expect(E, k, km, w), f"E {E} K {k}")
    for L in (k - 1, k, 100, 256):
        km, w = budget_case(5100 + 300 * k + L, k, 100, 70, L, p_n=0.02)
        # (exact and 1-edit occurrences: the planted windows hold them; k - 1 bases hold no exact one)
        want = expect(E, k, km, w)
        assert want.any() == (E == 1 or L >= k)
        both_routes(ce, k, km, w, want, f"E {E} K {k} L {L}")


# ---- the other entry points, E = 3, K = 22 ---------------------------------------------------------

K22 = 22


@pytest.fixture(scope="module")
def two_ends():
    a = budget_case(6001, K22, 300, 90, 150)
    b = budget_case(6002, K22, 37, 70, 151)
    return [a, b], [expect(3, K22, *a), expect(3, K22, *b)]


def test_e3_device_packed_jobs(c3, two_ends):
    """Two fused ends in pinned memory, packed by the kernel's copier workgroups (stage mode 3)."""
    parts, want = two_ends
    jobs = ac.Jobs([(km, ac.Dna5Sample.from_windows(w).pinned()) for km, w in parts])
    with hooks(AC_TESTING_DEVICE_PACK):
        if not BS_ON:
            refused(lambda: c3.count_jobs(K22, jobs))
            return
        got = c3.count_jobs(K22, jobs)
    assert kernel_of(c3) == 1 and c3.stage_mode() == 3
    for g, e in zip(got, want):
        np.testing.assert_array_equal(g, e)


def test_e3_uploaded_samples(c3, two_ends):
    """The CLI's route: ac_sample_upload_slot + ac_error_count_samples."""
    parts, want = two_ends
    dev = [c3.upload_sample(ac.pack_windows(w), i) for i, (_, w) in enumerate(parts)]
    call = lambda: c3.count_samples(K22, [(km, d) for (km, _), d in zip(parts, dev)])  # noqa: E731
    if not BS_ON:
        refused(call)
        return
    got = call()
    assert kernel_of(c3) == 1
    for g, e in zip(got, want):
        np.testing.assert_array_equal(g, e)


def child_dma_path():
    parts = [budget_case(6001, K22, 300, 90, 150), budget_case(6002, K22, 37, 70, 151)]
    want = [count_e(3, K22, *p) for p in parts]
    with ac.ApproxCounter(0, max_errors=3) as c:
        if not BS_ON:
            refused(lambda: c.count_jobs(K22, parts))
            return
        got = c.count_jobs(K22, parts)
        assert c.stage_mode() == 0 and kernel_of(c) == 1
        assert all(np.array_equal(g, e) for g, e in zip(got, want))


def test_e3_dma_path():
    run_child("child_dma_path()", AC_STAGE_EARLY="0")


def test_e3_multi_device_context():
    """ac_create_multi: the budget reaches every shard; with 5 and 2 windows some shard counts one window
    and some shard none."""
    for n1, n2 in ((90, 70), (5, 2)):
        a = budget_case(6100 + n1, K22, 60, n1, 150)
        b = budget_case(6200 + n2, K22, 40, n2, 151)
        want = [expect(3, K22, *a), expect(3, K22, *b)]
        with ac.ApproxCounter(n_gpus=2, max_errors=3) as multi:
            assert multi.max_errors == 3
            if not BS_ON:
                refused(lambda: multi.count_jobs(K22, [a, b]))
                continue
            got = multi.count_jobs(K22, [a, b])
            assert kernel_of(multi) == 1 and multi.stage_mode() == 0
        for g, e in zip(got, want):
            np.testing.assert_array_equal(g, e)


# ---- the setting itself -----------------------------------------------------------------------------

def test_setter_range_and_default():
    with ac.ApproxCounter(0) as c:
        assert c.max_errors == 2
        L = _lib.load()
        assert L.ac_set_max_errors(c.handle, 4) == _lib.AC_ERR_INVALID and c.max_errors == 2
        assert b"0..3" in L.ac_last_error(c.handle)
        with pytest.raises(_lib.ApproxCounterError):
            c.set_max_errors(7)
        for e in (0, 1, 3, 2):
            c.set_max_errors(e)
            assert c.max_errors == e


def test_sticky(two_ends):
    """One context: E = 3, then 2, then 3 again."""
    parts, want3 = two_ends
    with ac.ApproxCounter(0) as c:
        c.set_max_errors(3)
        first = c.count_jobs(K22, parts) if BS_ON else refused(lambda: c.count_jobs(K22, parts))
        c.set_max_errors(2)
        two = c.count_jobs(K22, parts)
        c.set_max_errors(3)
        if not BS_ON:  # (refused again, and the E = 2 call between the refusals counted)
            refused(lambda: c.count_jobs(K22, parts))
            for j, (km, w) in enumerate(parts):
                np.testing.assert_array_equal(two[j], oracle.count_myers(K22, km, w))
            return
        again = c.count_jobs(K22, parts)
        again2 = c.count_jobs(K22, parts)  # (and without a set in between)
    for j, (km, w) in enumerate(parts):
        np.testing.assert_array_equal(two[j], oracle.count_myers(K22, km, w))
        np.testing.assert_array_equal(first[j], want3[j])
        np.testing.assert_array_equal(again[j], first[j])
        np.testing.assert_array_equal(again2[j], first[j])


def test_exact_count_ignores_the_budget(c3, counter):
    _, w = equal_case(71, 10, 200, 100)
    img = ac.pack_windows(w)
    assert c3.exact_count(16, img, 1.0, limit=50) == counter.exact_count(16, img, 1.0, limit=50)


def test_refusals_leave_the_context_usable():
    """E = 3 with a ragged job, an equal job beside a ragged one, k = 17, k = 15, windows of 300 bases, and
    packed images with window descriptors: each raises AC_ERR_INVALID naming the constraint, nothing was
    launched (the device error word stays clean), and an E = 2 call on the same context is bit-exact."""
    eq = equal_case(81, 40, 30, 100, k=K22)
    ragged = cases.planted_case(82, K22, 40, 30, win_len=(90, 110))
    with ac.ApproxCounter(0, max_errors=3) as c:
        assert "ragged" in refused(lambda: c.count_jobs(K22, [ragged]))
        assert "ragged" in refused(lambda: c.count_jobs(K22, [eq, ragged]))
        for k in (17, 15):
            km, w = equal_case(83 + k, 40, 30, 100, k=k)
            assert "16 or 18..32" in refused(lambda: c.count_jobs(k, [(km, w)]))
            assert "16 or 18..32" in refused(lambda: device_count(c, k, [(km, w)]))
        long = equal_case(84, 40, 9, 300, k=K22)
        assert "1..256" in refused(lambda: c.count_jobs(K22, [long]))
        assert "1..256" in refused(lambda: device_count(c, K22, [long]))
        refused(lambda: c.count(K22, eq[0], ac.pack_windows(eq[1])))  # (descriptors: never a bit-sliced launch)
        seg = ac.DeviceSegment.upload(ragged[0], ac.pack_windows(ragged[1]))
        refused(lambda: c.count_device(K22, [seg]))
        c.check()
        c.set_max_errors(2)
        for part in (ragged, eq, long):
            np.testing.assert_array_equal(c.count_jobs(K22, [part])[0], oracle.count_myers(K22, *part))
        c.check()


# ---- the command line -------------------------------------------------------------------------------

def test_cli_counts_at_three_edits(tmp_path):
    """The cfg1 FASTA with --seed 1 --max-errors 3 -k 16: the k-mers and counts of both output files equal
    count_e(3, ...) over the sample --dump-sample writes with the same seed; without the flag the same
    command reproduces the golden files."""
    from tests.test_reader import decode, load_image

    base = [CLI, os.path.join(CFG1, "reads.fa"), "-k", "16", "-sn", "1000", "-sl", "100", "-lim", "100", "--seed", "1"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)  # noqa: E731
    r = run(["-o", "plain"])
    assert r.returncode == 0, r.stderr
    for end in ("start", "end"):
        assert open(tmp_path / f"plain_0.{end}").read() == open(os.path.join(CFG1, f"out.txt_0.{end}")).read()
    r = run(["--max-errors", "3", "-o", "three"])
    if not BS_ON:
        assert r.returncode == 1 and "max_errors" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert run(["--dump-sample", "smp", "-v", "0"]).returncode == 0
    for end in ("start", "end"):
        rows = [ln.split("\t") for ln in open(tmp_path / f"three_0.{end}").read().splitlines()]
        kmers = [cases.kmer_value(a) for a, _ in rows]
        got = np.array([int(b) for _, b in rows], np.uint64)
        wins = decode(load_image(tmp_path / f"smp_0.{end}"))
        assert len(kmers) == 100 and len(wins) == 1000
        want = count_e(3, 16, kmers, wins)
        np.testing.assert_array_equal(got, want)
        assert (want != oracle.count_myers(16, kmers, wins)).any()
        assert list(got) == sorted(got, reverse=True)
