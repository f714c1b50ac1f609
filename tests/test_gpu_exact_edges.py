"""The exact count (exact_count.hip, capi_exact.cpp) at the edges its machinery has: every partition
geometry, the bucket-overflow fallback and the limits of the per-bucket table, the count bins, the
wrapped all-T key, N flags at every window position and the low-complexity cut at equality -- on the
partitioned path and, where both exist, on the hash-table path.  Bit-exact against oracle/host_ref.py.
The samples come from tests/exact_cases.py; tests/test_exact_cases.py shows on the CPU that each one
has the property its test here relies on."""
import os
import subprocess
import sys

import pytest

import approx_counter_amd as ac
from oracle import host_ref
from tests import exact_cases as xc
from tests.test_gpu_exact import check

pytestmark = pytest.mark.gpu

PARTITIONED, HASH_TABLE = 1, 0


_COUNTED = {}


def check_sample(counter, sample, windows, k, thr, forbidden=frozenset(), limit=500, solid=0):
    """tests/test_gpu_exact.py::check for a sample packed by the caller (a padded or placed image);
    `windows` is one of tests/exact_cases.py's cached lists, so its count_kmers is taken once per
    threshold and forbidden set and only ranked anew for each limit."""
    key = (id(windows), k, float(thr), frozenset(forbidden))
    if key not in _COUNTED:
        _COUNTED[key] = (windows, *host_ref.count_kmers(windows, k, thr, forbidden))
    _, counted, exp_n = _COUNTED[key]
    exp = host_ref.get_solid_kmers(counted, solid, k) if solid else host_ref.get_most_frequent(counted, limit, k)
    got, n_dist, had_n = counter.exact_count(k, sample, thr, forbidden, limit, solid)
    assert got == exp
    assert (n_dist, had_n) == (len(counted), exp_n)
    return got, n_dist


def check_dense(counter, sample, ref, k, thr, limit=500, solid=0):
    """The same comparison against a vectorised reference (host_ref.count_kmers_dense's kept k-mers,
    counts and N-skips), ranked by host_ref.rank_dense."""
    uk, cnt, ref_n = ref
    got, n_dist, had_n = counter.exact_count(k, sample, thr, (), limit, solid)
    assert got == host_ref.rank_dense(uk, cnt, limit, solid, k)
    assert (n_dist, had_n) == (int(uk.size), ref_n)
    return got


# ---- C: geometry -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("nb_log2", xc.DENSE_NB)
def test_dense_geometry(counter, nb_log2, k):
    """2^nb_log2 buckets for nb_log2 = 7..12: 1, 2, 4, .., 32 buckets per super-bucket, on a skewed
    sample (planted adapter k-mers: one super-bucket of many level-2 chunks, many of few).  At
    nb_log2 = 10 the level-1 column scan crosses its slab boundary: 129 chunks for k = 16 (two slabs
    of EXACT_SCAN_SLAB = 128 rows, the second of one row), 257 for k = 22 (three slabs)."""
    w = xc.dense_windows(nb_log2)
    smp = ac.pack_windows(w)
    assert xc.nb_log2_for(smp.n_bases) == nb_log2
    if nb_log2 == 10:
        assert -(-max(32, smp.n_bases) // (8192 if k == 16 else 4096)) == (129 if k == 16 else 257)
    got = check_dense(counter, smp, xc.dense_reference(nb_log2, k), k, xc.lc_threshold(k), limit=300)
    assert counter.exact_path() == PARTITIONED
    assert got[0][1] > w.shape[0] // 8  # planted adapter k-mers lead the list


@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("nb_log2", xc.SPARSE_NB)
def test_sparse_geometry(counter, nb_log2, k):
    """2,000 ragged windows at the first slots, the middle and the very last slots of an image sized
    for 2^14 and 2^15 buckets (and 2^9 again): nearly every bucket, level-1 chunk and super-bucket
    is empty.  limit = 10^6 lists every kept k-mer (the count kernel again, emit_only).  Then 7 windows
    alone at the image's end, where many super-buckets are empty too."""
    smp = xc.sparse_sample(nb_log2)
    assert xc.nb_log2_for(smp.n_bases) == nb_log2
    ref = xc.sparse_reference(k)
    for limit in (200, 10**6):
        check_dense(counter, smp, ref, k, xc.lc_threshold(k), limit=limit)
        assert counter.exact_path() == PARTITIONED
    # a handful of windows at the image's end: fewer keys than super-buckets
    tail = xc.sparse_tail_sample(nb_log2)
    assert xc.nb_log2_for(tail.n_bases) == nb_log2
    for thr in (xc.lc_threshold(k), 100.0):
        check_sample(counter, tail, xc.sparse_tail_windows(), k, thr, limit=10**6)
        check_sample(counter, tail, xc.sparse_tail_windows(), k, thr, limit=5)
        assert counter.exact_path() == PARTITIONED


def test_rotation_on_one_context(counter):
    """Calls of different geometry, key width and list size back to back on one context: the grown,
    reused device blocks carry no state from one call to the next."""
    big = ac.pack_windows(xc.dense_windows(12))
    small = xc.sparse_sample(9)
    tiny = ["ACGTTGCAAGGCTTAACCGGTTAACGT" * 3, "T" * 40, "ACGTNACGT" * 5]
    for k in (16, 22, 16):
        check_dense(counter, big, xc.dense_reference(12, k), k, xc.lc_threshold(k), limit=300)
        assert counter.exact_path() == PARTITIONED
        check_dense(counter, small, xc.sparse_reference(k), k, xc.lc_threshold(k), limit=10**6)
        check_dense(counter, small, xc.sparse_reference(k), k, xc.lc_threshold(k), limit=50)
        assert counter.exact_path() == PARTITIONED
        check(counter, tiny, k, 100.0, limit=10**6)
        check(counter, tiny, k, 100.0, limit=50)


# ---- D: overflow fallback and table limits -----------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("name", list(xc.OVERFLOW_CASES))
def test_bucket_table_limits(counter, name, k):
    """One bucket of 2^7 filled with crafted keys (threshold 100.0: nothing filtered).  4,096 keys of
    4,096 home slots fill the LDS table exactly; 64 keys of one home slot probe up to index 63: both
    stay partitioned.  4,097 keys, or 65 of one home slot, overflow: the host recounts on the hash
    table from clean state (the N-skips of the random windows would show a count taken twice).  A
    plain call straight after is partitioned again."""
    wins, _, _, _, path = xc.overflow_case(name, k)
    smp = xc.overflow_sample(wins)
    assert xc.nb_log2_for(smp.n_bases) == xc.OVERFLOW_NB
    check_sample(counter, smp, wins, k, 100.0, limit=10**6)
    assert counter.exact_path() == path
    check_sample(counter, smp, wins, k, 100.0, limit=40)
    assert counter.exact_path() == path
    check_sample(counter, smp, wins, k, 100.0, solid=2)
    assert counter.exact_path() == path
    # recovery: a normal sample of the same geometry on the same context
    plain = xc.filler_windows(k, 300, seed=k)
    check_sample(counter, xc.overflow_sample(plain), plain, k, 100.0, limit=10**6)
    assert counter.exact_path() == PARTITIONED


# ---- E and F: run on the session's context (partitioned) and in a child with AC_EXACT_HASH=1 ------------------

def run_count_bins(counter, path):
    """Counts on both sides of the per-bucket histogram's edge (32 | 33) and of the last bin
    (4094 | 4095), ties inside it: the limit's cut inside the last bin, at the phist edge, everything
    listed; solid thresholds below, at and above every edge; the distinct count every time."""
    for k in (16, 22):
        smp = ac.pack_windows(xc.count_bins_case(k)[0])
        ref = xc.count_bins_reference(k)
        for limit in xc.BIN_LIMITS:
            check_dense(counter, smp, ref, k, xc.lc_threshold(k), limit=limit)
            assert counter.exact_path() == path
        for solid in xc.BIN_SOLIDS:
            check_dense(counter, smp, ref, k, xc.lc_threshold(k), solid=solid)
            assert counter.exact_path() == path


def run_all_t(counter, path):
    """The all-T k-mer whose stored key wraps (k = 16 compact, k = 32 wide) at counts 1, 2, 33 and
    4,096: forbidden, it vanishes and the distinct count drops by one; with only other k-mers
    forbidden it stays; at threshold 1.0 it is dropped as low-complexity."""
    for k in xc.ALL_T_KS:
        t = xc.all_t(k)
        for count in xc.ALL_T_COUNTS:
            wins, others = xc.all_t_case(k, count)
            smp = ac.pack_windows(wins)
            for limit in (10**6, 3):
                base, n_base = check_sample(counter, smp, wins, k, 100.0, limit=limit)
                gone, n_gone = check_sample(counter, smp, wins, k, 100.0, {t}, limit=limit)
                kept, n_kept = check_sample(counter, smp, wins, k, 100.0, set(others[:3]), limit=limit)
                low, _ = check_sample(counter, smp, wins, k, 1.0, limit=limit)
                assert counter.exact_path() == path
                if limit > 3 or count > 1:
                    assert (t, count) in base and (t, count) in kept
                assert t not in dict(gone) and t not in dict(low)
                assert (n_gone, n_kept) == (n_base - 1, n_base - 3)
            for solid in (1, count, count + 1):
                check_sample(counter, smp, wins, k, 100.0, solid=solid)
                check_sample(counter, smp, wins, k, 100.0, {t, others[0]}, solid=solid)


def run_n_positions(counter, path):
    """A single N at each position of a window (and at both ends), k on both key widths."""
    for k in xc.N_POSITION_KS:
        check(counter, xc.n_position_case(k), k, 100.0, limit=10**6)
        assert counter.exact_path() == path


def run_score_equality(counter, path):
    """The low-complexity cut at thresholds that some k-mers score exactly, and the float32 on either
    side: the kept set is the reference's at every one."""
    for k in xc.SCORE_KS:
        w, thresholds, _ = xc.score_case(k)
        smp = ac.pack_windows(w)
        for thr in thresholds:
            check_dense(counter, smp, host_ref.count_kmers_dense(w, k, thr), k, float(thr), limit=10**6)
            assert counter.exact_path() == path


def test_count_bins(counter):
    run_count_bins(counter, PARTITIONED)


def test_all_t_key(counter):
    run_all_t(counter, PARTITIONED)


def test_n_at_every_position(counter):
    run_n_positions(counter, PARTITIONED)


def test_score_equality(counter):
    run_score_equality(counter, PARTITIONED)


def _on_hash_table(fn):
    """fn of this module in one fresh child process with AC_EXACT_HASH=1 (the hash-table path:
    exact_scan_kernel and the table gather)."""
    code = (
        "import approx_counter_amd as ac\n"
        "from tests import test_gpu_exact_edges as t\n"
        "c = ac.ApproxCounter(0)\n"
        f"t.{fn}(c, t.HASH_TABLE)\n"
        "c.close()\n"
        "print('OK')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AC_EXACT_HASH="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_count_bins_on_hash_table():
    _on_hash_table("run_count_bins")


@pytest.mark.parametrize("fn", ["run_all_t", "run_n_positions", "run_score_equality"])
def test_keys_and_filters_on_hash_table(fn):
    _on_hash_table(fn)
