"""GPU tests of the hit levels and match end positions from the jobs stage (ac_window_hits_jobs,
ac_window_positions_jobs and their _submit forms; DESIGN.md §4e "Hits from the jobs stage"): Dna5 windows in,
counts, hit matrices and position matrices out of one call, on every route a single-device jobs call takes --
the early launch and device packing (the staged hits kernels, bshs_count.hip / bsps_count.hip), the DMA path in
one part and in two (the plain hits kernels, here on images with inline N records).

Expected values: tests/hits_cases.expected_hits and tests/positions_cases.expected_positions, from the oracle's
DP distance.  Every matrix is compared bit for bit; the counts of the same call must equal the expected
counts, the matrix's popcounts and a plain count_jobs.  Host matrices are filled with 0xFFFFFFFF by
ApproxCounter.window_hits_jobs before the call; device matrices are filled with it and followed by GUARD words
of it: a word the call did not write, a stray bit past n_kmers and a store past the matrix all show."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.hits_cases import FILL, GUARD, equal_case, expected_hits, pack_hits
from tests.positions_cases import expected_positions, pack_positions, positions_case, profile_of
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_bitslice import AC_TESTING_DEVICE_PACK, BITSLICE, hooks, kernel_of, n_windows_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_ON = BITSLICE == 1
AC_TESTING_TWO_PARTS = 16
EARLY = os.environ.get("AC_STAGE_EARLY", "1") != "0"  # (the children of the DMA routes run with 0)


@pytest.fixture(scope="module")
def ctxs():
    """One context per edit budget (the budget is sticky; the session's `counter` stays at 2)."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (0, 1, 2, 3)}
    yield made
    for c in made.values():
        c.close()


def refused(fn, word="window"):
    with pytest.raises(_lib.ApproxCounterError) as e:
        fn()
    assert e.value.status == _lib.AC_ERR_INVALID, e.value
    assert word in str(e.value), e.value
    return str(e.value)


@functools.lru_cache(maxsize=None)
def case(seed, k, n_kmers, n_windows, L, E, p_n=0.01):
    """(kmers, windows, hit, pos, counts): positions_case, built once per shape and shared."""
    km, w, hit, pos, counts, _ = positions_case(seed, k, n_kmers, n_windows, L, E, p_n=p_n)
    return np.asarray(km, np.uint64), w, hit, pos, counts


def expect(k, km, w, E):
    hit, pos, counts = expected_positions(k, km, w, E)
    return hit, pos, counts


def sample_of(w, pinned=False, shuffle=None):
    """The job's Dna5Sample; shuffle (a seed): the windows lie in memory in a random order, window i still
    being w[i]."""
    s = ac.Dna5Sample.from_windows(w)
    if shuffle is not None and s.n_windows:
        L = int(s.length[0])
        perm = np.random.default_rng(shuffle).permutation(s.n_windows)
        bases = np.empty_like(s.bases)
        for i, p in enumerate(perm):
            bases[p * L:(p + 1) * L] = s.bases[i * L:(i + 1) * L]
        s = ac.Dna5Sample(bases, perm.astype(np.uint64) * np.uint64(L), s.length)
    return s.pinned() if pinned else s


def compare(what, k, km, w, E, counts, levels, planes, plain, want=None):
    """One job's results against the expected values, bit for bit."""
    hit, pos, want_counts = want if want is not None else expect(k, km, w, E)
    words = (len(km) + 31) // 32
    assert levels.shape == (E + 1, len(w), words), what
    m = pack_hits(hit)
    bad = np.argwhere(levels != m)
    assert not len(bad), f"{what}: {len(bad)} hit words differ, first (level, window, word) {bad[0]}: " \
                         f"{levels[tuple(bad[0])]:#x} != {m[tuple(bad[0])]:#x}"
    if planes is not None:
        p = pack_positions(pos)
        bad = np.argwhere(planes != p)
        assert not len(bad), f"{what}: {len(bad)} position words differ, first (plane, window, word) {bad[0]}: " \
                             f"{planes[tuple(bad[0])]:#x} != {p[tuple(bad[0])]:#x}"
    np.testing.assert_array_equal(counts, want_counts, err_msg=str(what))
    np.testing.assert_array_equal(ac.unpack_hits(levels, len(km)).sum(axis=(0, 1)).astype(np.uint64), counts, err_msg=str(what))
    np.testing.assert_array_equal(plain, counts, err_msg=f"{what}: the plain count_jobs")


def run(c, k, parts, positions=False, pinned=False, shuffle=None, mode=None, wants=None):
    """window_hits_jobs over parts = [(kmers, windows)], hits and (asked) positions, each job compared; then the
    plain count_jobs of the same Jobs.  mode: the ac_stage_mode the call must report."""
    jobs = ac.Jobs([(np.asarray(km, np.uint64), sample_of(w, pinned, shuffle)) for km, w in parts])
    if not BS_ON:
        refused(lambda: c.window_hits_jobs(k, jobs, positions=positions), "AC_BITSLICE")
        return None
    got = c.window_hits_jobs(k, jobs, positions=positions)
    if any(len(km) and len(w) for km, w in parts):
        assert kernel_of(c) == 1
        if mode is not None:
            assert c.stage_mode() == mode, (c.stage_mode(), mode)
    counts = [wh.counts.copy() for wh in got]
    plain = [x.copy() for x in c.count_jobs(k, jobs)]
    for j, ((km, w), wh) in enumerate(zip(parts, got)):
        if len(km) and len(w):
            compare((k, j, len(km), len(w)), k, km, w, c.max_errors, counts[j], wh.levels, wh.planes if positions else None,
                    plain[j], wants[j] if wants else None)
        else:
            assert not counts[j].any() and not plain[j].any() and wh.levels.size == 0
    return got


def one(c, k, n_kmers, n_windows, L, seed, p_n=0.01, **kw):
    km, w, hit, pos, counts = case(seed, k, n_kmers, n_windows, L, c.max_errors, p_n)
    for positions in (False, True):
        run(c, k, [(km, w)], positions=positions, wants=[(hit, pos, counts)], **kw)


# ---- lanes and rows, window lengths -------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers,n_windows", [(40, 37), (300, 70), (1, 1), (33, 65)])
def test_lanes_and_rows(ctxs, n_kmers, n_windows):
    """40 x 37: a partial second candidate block, two lanes per window, a second row of 5 windows; 300 x 70: two
    candidate groups, 256 + 44, the second one's lanes past its last block without a word; 1 x 1; 33 x 65."""
    one(ctxs[2], 16, n_kmers, n_windows, 100, 9000 + n_kmers)


@pytest.mark.parametrize("L", [1, 3, 13, 100, 101, 255, 256])
def test_window_lengths(ctxs, L):
    """One or two 4-base blocks, the filling N, a full slot, and slots whose last code word has no room for a
    record (13 has, 255 and 256 have not)."""
    one(ctxs[2], 16, 40, 20, L, 9100 + L, p_n=0.02)


# ---- the sources of a window's N bits -------------------------------------------------------------------

@pytest.mark.parametrize("name,counts_n,spots", [
    ("records", [1], ()),
    ("records_at_capacity_and_overflowed", [0, 4, 5, 1, 4, 5], ()),
    ("first_last_and_word_edges", [0, 2, 4, 6, 8], (0, 99, 31, 32, 63, 64, 95, 96)),
    ("all_n_window", [0, 0, 0, 100], ()),
])
def test_n_sources(ctxs, name, counts_n, spots):
    """100-base windows hold records of up to 4 positions (nrec.h): every window with 1 N; windows with 4 and
    with 5 (overflowed: the staged kernel reads their bitmap words after the whole-segment wait); N on the first
    and last base and both sides of each 32-base edge; an all-N window, whose rows are zero.  Beside each, in the
    same call, a job without any N."""
    km, w = n_windows_case(9200 + len(name), 37, 100, counts_n, spots)
    km_c, w_c = equal_case(9250, 40, 20, 100, p_n=0.0)
    assert not any("N" in x for x in w_c)
    for E in (2, 3):
        got = run(ctxs[E], 16, [(km, w), (km_c, w_c)], positions=True)
        if got and "all_n" in name:
            all_n = [i for i in range(37) if (w[i] == 4).all()]
            assert all_n and not got[0].levels[:, all_n, :].any() and not got[0].planes[:, all_n, :].any()


# ---- jobs -----------------------------------------------------------------------------------------------

def test_four_jobs_in_both_orders(ctxs):
    """100-base start windows, 101-base end windows, a job with k-mers and no windows (NULL matrices), a job with
    windows and no k-mers; then the first two in the other order."""
    a = case(9301, 16, 40, 37, 100, 2)
    b = case(9302, 16, 70, 41, 101, 2)
    dead, none = (a[0][:5], []), (np.zeros(0, np.uint64), a[1])
    for first, second in ((a, b), (b, a)):
        for positions in (False, True):
            run(ctxs[2], 16, [first[:2], second[:2], dead, none], positions=positions,
                wants=[first[2:], second[2:], None, None])


# ---- every k, every budget --------------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_every_k_at_two_edits(ctxs, k):
    one(ctxs[2], k, 40, 37, 100, 9400 + k)


@pytest.mark.parametrize("k", [16, 22, 29, 32])
@pytest.mark.parametrize("E", [0, 1, 3])
def test_other_budgets(ctxs, E, k):
    one(ctxs[E], k, 40, 37, 100, 9500 + 10 * k + E)


# ---- routes ---------------------------------------------------------------------------------------------

def test_early_launch(ctxs):
    """Mode 2: the staged hits kernels stage their own input."""
    for E, k in ((2, 16), (3, 22)):
        one(ctxs[E], k, 40, 37, 100, 9600 + k, mode=2 if EARLY else 0)


def test_device_packing(ctxs):
    """Mode 3: pinned Dna5Samples packed by the staged hits kernels' copier workgroups, the windows lying in
    memory in a shuffled order -- row w is still the job's window w."""
    with hooks(AC_TESTING_DEVICE_PACK):
        for E, k in ((2, 16), (3, 22)):
            one(ctxs[E], k, 40, 37, 100, 9600 + k, pinned=True, shuffle=k, mode=3 if EARLY else 0)
            one(ctxs[E], k, 300, 70, 101, 9650 + k, pinned=True, shuffle=k, mode=3 if EARLY else 0)


def submit(c, k, parts, positions):
    """The _submit forms: device matrices of the caller's, guarded; then check()."""
    import torch

    E = c.max_errors
    jobs = ac.Jobs([(np.asarray(km, np.uint64), sample_of(w)) for km, w in parts])
    nh = [ac.hits_words(len(km), len(w), E) for km, w in parts]
    npos = [ac.positions_words(len(km), len(w)) for km, w in parts]
    mk = lambda n: torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") if n else None  # noqa: E731
    dh, dp = [mk(n) for n in nh], [mk(n) for n in npos]
    out = torch.full((jobs.n_counts,), 7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    call = lambda: c.submit_jobs(k, jobs, out, stream=st.cuda_stream, hits=dh, positions=dp if positions else None)  # noqa: E731
    if not BS_ON:
        refused(call, "AC_BITSLICE")
        return
    for _ in range(2):  # both staging slots
        call()
        st.synchronize()
        c.check()
        assert kernel_of(c) == 1
    plain = [x.copy() for x in c.count_jobs(k, jobs)]
    counts, at = out.cpu().numpy().astype(np.uint64), 0
    for j, (km, w) in enumerate(parts):
        mine = counts[at:at + len(km)]
        at += len(km)
        if not (len(km) and len(w)):
            assert not mine.any()
            continue
        words = (len(km) + 31) // 32
        h = dh[j].cpu().numpy().view(np.uint32)
        assert (h[nh[j]:] == FILL).all(), "a store past the hit matrix"
        planes = None
        if positions:
            p = dp[j].cpu().numpy().view(np.uint32)
            assert (p[npos[j]:] == FILL).all(), "a store past the position matrix"
            planes = p[:npos[j]].reshape(8, len(w), words)
        compare(("submit", j), k, km, w, E, mine, h[:nh[j]].reshape(E + 1, len(w), words), planes, plain[j])


def test_submit_forms(ctxs):
    a = case(9301, 16, 40, 37, 100, 2)
    b = case(9302, 16, 70, 41, 101, 2)
    for positions in (False, True):
        submit(ctxs[2], 16, [a[:2], b[:2], (a[0][:5], [])], positions)
    a3 = case(9701, 22, 40, 37, 100, 3)
    submit(ctxs[3], 22, [a3[:2]], True)


def child_dma(two_parts):
    """AC_STAGE_EARLY=0: the DMA path -- the plain hits kernels on images with inline N records; with
    AC_TESTING_TWO_PARTS two parts, each writing its own rows: 37 and 70 windows at two lanes per window (32 per
    row) cut at 19 and 35, inside a row."""
    import torch

    assert not EARLY
    for E, k in ((2, 16), (3, 22)):
        with ac.ApproxCounter(0, max_errors=E) as c, hooks(AC_TESTING_TWO_PARTS if two_parts else 0):
            one(c, k, 40, 37, 100, 9600 + k, mode=0)
            one(c, k, 40, 70, 101, 9800 + k, mode=0)
            km, w = n_windows_case(9850, 37, 100, [0, 4, 5, 1, 4, 5], (0, 99))
            a = case(9301, 16, 40, 37, 100, 2)
            run(c, 16, [(km, w), a[:2]], positions=True, mode=0)
            if E == 2:
                submit(c, 16, [a[:2], (km, w)], True)
            torch.cuda.synchronize()
            c.check()


def child_multi_row_items():
    """1 % of the waves that fit (AC_BS_WAVES_PCT=1): every wave claims several items, so each wave stores many
    rows' words; 1,500 windows drawn from 61 distinct texts."""
    for E, k in ((2, 16), (3, 22)):
        km, texts, hit_t, pos_t, _ = case(9900 + k, k, 40, 61, 100, E)
        idx = np.random.default_rng(k).integers(0, len(texts), size=1500)
        hit, pos, w = hit_t[:, idx, :], pos_t[idx, :], [texts[i] for i in idx]
        with ac.ApproxCounter(0, max_errors=E) as c:
            got = run(c, k, [(km, w)], positions=True, mode=2 if EARLY else 0,
                      wants=[(hit, pos, hit.sum(axis=(0, 1)).astype(np.uint64))])
            if got:
                print(f"K {k} E {E}: {c.last_launch()}", flush=True)
                assert int(c.last_launch()["windows_per_wave"]) > 1


def child_bitslice_off():
    """AC_BITSLICE=0: every call is refused with the message that names the switch, nothing is written, and the
    ordinary count still runs (on the word-parallel kernel)."""
    import torch

    km, w = equal_case(9951, 40, 30, 100, k=22)
    with ac.ApproxCounter(0) as c:
        for positions in (False, True):
            assert "AC_BITSLICE" in refused(lambda: c.window_hits_jobs(22, [(km, w)], positions=positions))
        jobs = ac.Jobs([(np.asarray(km, np.uint64), sample_of(w))])
        buf = torch.full((ac.hits_words(40, 30, 2),), -1, dtype=torch.int32, device="cuda")
        out = torch.full((40,), 7, dtype=torch.int32, device="cuda")
        assert "AC_BITSLICE" in refused(lambda: c.submit_jobs(22, jobs, out, hits=[buf]))
        torch.cuda.synchronize()
        assert bool((buf == -1).all()) and bool((out == 7).all())
        assert np.array_equal(c.count_jobs(22, [(km, w)])[0], oracle.count_myers(22, km, w))
        assert kernel_of(c) == 0


def run_child(call, **env):
    code = f"from tests.test_gpu_jobs_hits import *\n{call}\nprint('OK')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_dma_path_in_one_part():
    run_child("child_dma(False)", AC_STAGE_EARLY="0")


def test_dma_path_in_two_parts():
    run_child("child_dma(True)", AC_STAGE_EARLY="0")


def test_items_of_several_rows_early():
    print(run_child("child_multi_row_items()", AC_BS_WAVES_PCT="1"))


def test_items_of_several_rows_dma():
    print(run_child("child_multi_row_items()", AC_BS_WAVES_PCT="1", AC_STAGE_EARLY="0"))


def test_bitslice_off_refuses_every_call():
    run_child("child_bitslice_off()", AC_BITSLICE="0")


# ---- the routes agree -------------------------------------------------------------------------------------

def test_jobs_route_equals_samples_route(ctxs):
    """window_hits_jobs equals window_hits (host pack_windows, upload, ac_window_positions_samples) on the same
    windows, word for word; position_profile() and level_counts() equal numpy's."""
    c = ctxs[2]
    km, w, hit, pos, counts = case(9001, 16, 40, 37, 100, 2)
    if not BS_ON:
        refused(lambda: c.window_hits_jobs(16, [(km, w)], positions=True), "AC_BITSLICE")
        return
    a = c.window_hits_jobs(16, [(km, w)], positions=True)[0]
    b = c.window_hits(16, [(km, ac.pack_windows(w))], positions=True)[0]
    np.testing.assert_array_equal(a.levels, b.levels)
    np.testing.assert_array_equal(a.planes, b.planes)
    np.testing.assert_array_equal(a.counts, b.counts)
    np.testing.assert_array_equal(a.level_counts(), hit.sum(axis=1))
    np.testing.assert_array_equal(a.position_profile(), profile_of(hit, pos, 100))
    np.testing.assert_array_equal(a.end_positions(), pos)
    np.testing.assert_array_equal(a.distances(), np.minimum(ac.distances_from_hits(hit), 3))


# ---- refusals ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    """Each case of the header's list: AC_ERR_INVALID naming the constraint, nothing written, and the context
    counts correctly afterwards."""
    import torch

    k = 22
    eq = equal_case(9961, 40, 30, 100, k=k)
    ragged = cases.planted_case(9962, k, 40, 30, win_len=(90, 110))
    long = equal_case(9963, 40, 9, 300, k=k)
    L = _lib.load()

    def dev_call(c, kk, parts):
        jobs = ac.Jobs([(np.asarray(km, np.uint64), sample_of(w)) for km, w in parts])
        bufs = [torch.full((max(ac.hits_words(len(km), len(w), 3), 1),), -1, dtype=torch.int32, device="cuda")
                for km, w in parts]
        out = torch.full((max(jobs.n_counts, 1),), 7, dtype=torch.int32, device="cuda")
        return bufs + [out], (lambda: c.submit_jobs(kk, jobs, out, hits=bufs))

    with ac.ApproxCounter(0) as c:
        every = []
        for parts, word in (([ragged], "ragged"), ([eq, ragged], "ragged"), ([long], "1..256")):
            for positions in (False, True):
                assert word in refused(lambda: c.window_hits_jobs(k, parts, positions=positions)) or not BS_ON
            bufs, call = dev_call(c, k, parts)
            assert word in refused(call) or not BS_ON
            every.append(bufs)
        for kk in (15, 17):
            km, w = equal_case(9964 + kk, 40, 30, 100, k=kk)
            assert "16 or 18..32" in refused(lambda: c.window_hits_jobs(kk, [(km, w)]))
            bufs, call = dev_call(c, kk, [(km, w)])
            assert "16 or 18..32" in refused(call)
            every.append(bufs)
        # a NULL matrix for a job with work: the host forms (raw), the submit form
        jobs = ac.Jobs([(np.asarray(eq[0], np.uint64), sample_of(eq[1]))] * 2)
        m = np.full(ac.hits_words(40, 30, 2), FILL, np.uint32)
        hp = (_lib.p32 * 2)(m.ctypes.data_as(_lib.p32), None)
        assert L.ac_window_hits_jobs(c.handle, k, jobs.array, 2, hp) == _lib.AC_ERR_INVALID
        assert b"NULL" in L.ac_last_error(c.handle) or not BS_ON
        assert L.ac_window_positions_jobs(c.handle, k, jobs.array, 2, hp, hp) == _lib.AC_ERR_INVALID
        assert b"NULL" in L.ac_last_error(c.handle) or not BS_ON
        assert (m == FILL).all()
        bufs, _ = dev_call(c, k, [eq, eq])
        assert "NULL" in refused(lambda: c.submit_jobs(k, jobs, bufs[2], hits=[bufs[0], None])) or not BS_ON
        assert "NULL" in refused(lambda: c.submit_jobs(k, jobs, bufs[2], hits=bufs[:2], positions=[bufs[0], None])) or not BS_ON
        every.append(bufs)
        torch.cuda.synchronize()
        for bufs in every:
            assert all(bool((b == -1).all()) for b in bufs[:-1]) and bool((bufs[-1] == 7).all()), "a refused call wrote"
        c.check()
        for part in (ragged, eq, long):
            np.testing.assert_array_equal(c.count_jobs(k, [part])[0], oracle.count_myers(k, *part))
        run(c, k, [eq], positions=True)
        c.check()
    with ac.ApproxCounter(n_gpus=2) as multi:
        for positions in (False, True):
            assert "single-device" in refused(lambda: multi.window_hits_jobs(k, [eq], positions=positions))
        np.testing.assert_array_equal(multi.count_jobs(k, [eq])[0], oracle.count_myers(k, *eq))


# ---- error_levels -------------------------------------------------------------------------------------------

def test_error_levels_cfg1():
    """error_levels on the config-1 fixture: each k-mer's levels sum to error_count's value and equal the oracle's
    per-level counts."""
    import json

    from oracle import host_ref

    d = os.path.join(ROOT, "tests", "golden", "cfg1")
    params = json.load(open(os.path.join(d, "params.json")))
    _, seqs = host_ref.read_fasta(os.path.join(d, "reads.fa"))
    k = params["k"]
    for end, bottom in (("start", False), ("end", True)):
        wins = host_ref.sample_all(seqs, params["sl"], bottom)
        exact = [(cases.kmer_value(ln.split("\t")[0]), int(ln.split("\t")[1]))
                 for ln in open(os.path.join(d, "exact_0." + end)).read().splitlines()]
        if not BS_ON:
            refused(lambda: ac.error_levels(wins, exact, 4, k, 0), "AC_BITSLICE")
            continue
        lv = ac.error_levels(wins, exact, 4, k, 0)
        res = ac.error_count(wins, exact, 4, k, 0)
        kmers = [km for km, _ in exact]
        hit, _ = expected_hits(k, kmers, wins, 2)
        want = hit.sum(axis=1)
        assert list(lv) == kmers
        for i, km in enumerate(kmers):
            assert len(lv[km]) == 3 and sum(lv[km]) == res[km], km
            assert lv[km] == tuple(int(x) for x in want[:, i]), km
