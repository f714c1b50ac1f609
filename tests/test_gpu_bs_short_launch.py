"""GPU tests of the bit-sliced count kernel's per-wave fixed work, which a short launch does not amortise
(bs_count.inc): the ~Eq table built from parked k-mers (bs::neq_mask) and the flush by plane
merge.  Every case goes through the C ABI, is compared bit for bit with the CPU oracle and asserts which
count kernel the launch ran (ac_testing_last_count_kernel).  The cases are built in
tests/short_launch_cases.py; tests/test_short_launch_cases.py shows what they hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from tests import short_launch_cases as slc
from tests.hits_cases import hits_case
from tests.test_bs_nfa_k import LISTED_K
from tests.test_budget_cpu import count_e
from tests.test_gpu_bitslice import BITSLICE, device_count, equal_case, kernel_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1


def same(c, what, got, want, kernel=BITSLICE):
    assert kernel_of(c) == kernel, what
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, (what, bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])


def launched_waves(c, k):
    """The waves of a launch of less than one round of the k kernel, at the process's share of the waves."""
    km, w = equal_case(k, 3, 2, 100, k=k)
    device_count(c, k, [(km, w)])
    return int(c.last_launch()["waves"])


def run_child(call, **env):
    code = f"from tests.test_gpu_bs_short_launch import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


# ---- the table ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_table_of_single_base_variants(counter, k):
    """The all-A k-mer and its 3 k single-base variants, each planted once, among 1 .. 500 candidates: one,
    two and four building waves, a partial last block, blocks that LW rounds up to, a second group -- staged
    (ac_error_count_jobs) and, at 257 and 500, resident."""
    for n in slc.TABLE_COUNTS:
        km, w = slc.table_case(k, n)
        want = oracle.count_myers(k, km, w)
        same(counter, (k, n, "jobs"), counter.count_jobs(k, [(km, w)])[0], want)
        if n >= 257:
            same(counter, (k, n, "device"), device_count(counter, k, [(km, w)])[0], want)


# ---- the flush ------------------------------------------------------------------------------------

def child_flush_threshold():
    """1 % of the waves that fit: 30 rows per wave, each of 32 windows that all hold candidate 0 exactly, so
    a wave flushes at its threshold -- 10 rows (7 at E = 3) -- with the same count, the largest five planes
    hold, in each of the 32 lanes that are merged.  E = 2, 3 and 0; staged and resident."""
    with ac.ApproxCounter(0) as c:
        W = launched_waves(c, 16)
    for E in (2, 3, 0):
        if E != 2 and not BS_ON:
            continue
        km, w, (n0, n1) = slc.threshold_case(32 * 30 * W - 5)
        per = [count_e(E, 16, km, [t]) for t in slc.THRESHOLD_TEXTS]
        want = per[0] * np.uint64(n0) + per[1] * np.uint64(n1)
        with ac.ApproxCounter(0, max_errors=E) as c:
            same(c, (E, "jobs"), c.count_jobs(16, [(km, ac.Dna5Sample.from_windows(w))])[0], want)
            rows = int(c.last_launch()["windows_per_wave"])
            print(f"E {E}: rows per wave {rows}", flush=True)
            assert rows > (7 if E == 3 else 10) or not BS_ON
            same(c, (E, "device"), device_count(c, 16, [(km, w)])[0], want)


def test_flush_at_the_threshold_in_every_merged_lane():
    print(run_child("child_flush_threshold()", AC_BS_WAVES_PCT="1"))


@pytest.mark.parametrize("n_kmers", [32, 33, 64, 65, 128, 129, 256])
def test_flush_lane_edges_and_partial_rows(counter, n_kmers):
    """Candidate counts at each lanes-per-window edge; 1, wpr - 1, wpr + 1 and 3 wpr + 5 windows: lanes
    without a window are merged as zeros, and a lane extracts candidates whose windows sat in other lanes."""
    wpr = slc.lanes_per_window(n_kmers)[1]
    for n_windows in (1, wpr - 1, wpr + 1, 3 * wpr + 5):
        km, w = equal_case(7000 + n_kmers + n_windows, n_kmers, n_windows, 100)
        want = oracle.count_myers(16, km, w)
        same(counter, (n_kmers, n_windows, "jobs"), counter.count_jobs(16, [(km, w)])[0], want)
        same(counter, (n_kmers, n_windows, "device"), device_count(counter, 16, [(km, w)])[0], want)


@pytest.mark.parametrize("E", [0, 3])
def test_flush_other_budgets(E):
    if not BS_ON:
        return  # (another budget than 2 needs the bit-sliced kernel: tests/test_gpu_budget.py has the refusals)
    with ac.ApproxCounter(0, max_errors=E) as c:
        for k, n_kmers, n_windows in ((16, 129, 3 * 8 + 5), (22, 65, 17), (32, 300, 9)):
            km, w = equal_case(7100 + n_kmers + E, n_kmers, n_windows, 100, k=k)
            want = count_e(E, k, km, w)
            same(c, (E, k, "jobs"), c.count_jobs(k, [(km, w)])[0], want, 1)
            same(c, (E, k, "device"), device_count(c, k, [(km, w)])[0], want, 1)


def test_flush_of_a_hits_launch(counter):
    """The hits-writing family runs the same flush: matrix and counts of 129 candidates over 3 rows and 5."""
    from tests.test_gpu_hits import check, device_hits

    km, w, hit, counts = hits_case(7200, 16, 129, 3 * 8 + 5, 100, 2)
    got = device_hits(counter, 16, [(km, w)])
    if got:
        check(got[0], hit, counts, "hits")
