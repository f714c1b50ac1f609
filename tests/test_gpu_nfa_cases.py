"""GPU parity of the count kernels on designed contents (tests/nfa_cases.py; DESIGN.md §4e "Which file covers
which kernel"): pairs at distance exactly E + 1, low-complexity and periodic candidates against near-periodic
text, and the overlapping k-mers of one adapter side by side in a lane word -- where the other GPU files draw
random candidates and random text.  Through the code that has no host build: the word-parallel kernel's
generated blocks (every pack factor and width, the pipeline's drain at a window's last bases, the 256-base
fetch seam, skip_first), the bit-sliced bodies (the LDS ~Eq table, the 4-base blocks and the filled-up last
one), the N paths, and the hits and positions stores.

Every comparison is bit-exact against the plain DP (tests.test_budget_cpu.distances / counts_from,
tests.positions_cases.expected_positions, oracle.count_dp); tests/test_nfa_cases.py shows on the CPU that each
case has the property relied on here and that a kernel wrong at d = E + 1 or at a tie would fail.  Every launch
asserts which kernel ran (ac_testing_last_count_kernel: 1 bit-sliced, 0 word-parallel); every hits and positions
buffer is pre-filled and guarded (tests.test_gpu_positions.device_positions / check).  With AC_BITSLICE=0 the
same calls expect the word-parallel kernel's counts at E = 2 and a refusal of every other budget, of hits and of
positions.  The budget is sticky: the other budgets have contexts of their own, the session's `counter` stays
at 2.

If a test here fails the kernel is wrong, not the DP: read the kernel against the failing pair (the builders name
k-mer, window, placement and edit kinds) and keep a reduction of the input as a named case in nfa_cases.py."""
import numpy as np
import pytest

import approx_counter_amd as ac
from tests import nfa_cases as nc
from tests.positions_cases import expected_positions, pack_hits, pack_positions
from tests.test_bs_nfa_k import LISTED_K
from tests.test_budget_cpu import counts_from
from tests.test_gpu_bitslice import BITSLICE, device_count, kernel_of
from tests.test_gpu_budget import refused as budget_refused
from tests.test_gpu_positions import check, device_positions
from tests.test_gpu_positions import refused as hits_refused

pytestmark = pytest.mark.gpu
BS_ON = BITSLICE == 1
WORD = 0
# the shapes run here; tests/test_nfa_cases.py shows each one's property on the CPU
RAGGED_K = (5, 8, 9, 10, 11, 15, 16, 17, 22, 32)  # every pack factor and width of the word-parallel kernel
EQ_WORD_K = (8, 10, 15, 17)
SEAM_K = (10, 16, 22)
BUDGET_K = (16, 22, 29, 32)  # the k that also run E = 0, 1 and 3
WHOLE_K = (16, 32)
BLOCK_K = (16, 22, 32)
N_K = (10, 16, 22)
TIE_SHAPES = ((16, 41), (22, 100), (32, 67))
SMALL_K = (2, 3, 4)


@pytest.fixture(scope="module")
def ctxs(counter):
    """One context per edit budget other than 2, and one at 2 for the hits and positions calls."""
    made = {E: ac.ApproxCounter(0, max_errors=E) for E in (0, 1, 2, 3)}
    yield made
    for c in made.values():
        c.close()
    assert counter.max_errors == 2


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert not len(bad), f"{what}: {len(bad)} counts differ, first k-mer {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def ragged(counter, k, km, w, want, what):
    """ac_error_count on a packed image with window descriptors: the word-parallel kernel's ragged code."""
    got = counter.count(k, km, ac.pack_windows(w))
    assert kernel_of(counter) == WORD, what
    same(got, want, what)


def staged_and_plain(c, k, parts, want, what, kernel):
    """count_jobs (the staged instantiation) and count_device with window_len (the plain one) over equal-window
    parts [(kmers, windows)], at the context's budget; at another budget than 2 without the bit-sliced kernel
    both are refused."""
    if kernel != 1 and c.max_errors != 2:
        budget_refused(lambda: c.count_jobs(k, parts))
        budget_refused(lambda: device_count(c, k, parts))
        return
    for route, got in (("staged", lambda: c.count_jobs(k, parts)), ("plain", lambda: device_count(c, k, parts))):
        got = got()
        assert kernel_of(c) == kernel, (what, route)
        for j, (g, wnt) in enumerate(zip(got, want)):
            same(g, wnt, (what, route, "part", j))


# ---- 1, 2: the word-parallel kernel, ragged ------------------------------------------------------------

@pytest.mark.parametrize("k", RAGGED_K)
def test_word_parallel_ragged(counter, k):
    """near_miss_case(k): every P and W instantiation; ragged windows keep k = 16, 22 and 32 on this kernel."""
    km, w, d = nc.near_miss_case(k)
    ragged(counter, k, km, w, counts_from(d, 2), ("near miss", k))


@pytest.mark.parametrize("k", SMALL_K)
def test_word_parallel_exhaustive(counter, k):
    """All 4^k candidates against every text of 0..k + 3 bases and every text of k + 1 with an N."""
    km, w, want = nc.exhaustive_small(k)
    ragged(counter, k, km, w, want, ("exhaustive", k))


# ---- 3, 4: the word-parallel kernel, equal windows and the fetch seams -----------------------------------

@pytest.mark.parametrize("side", ["start", "end"])
@pytest.mark.parametrize("k", EQ_WORD_K)
def test_word_parallel_equal_windows(counter, k, side):
    """The near-miss windows padded to k + 9 bases, the occurrence at the window's first or last base."""
    km, w, d = nc.equalised_case(k, side)
    staged_and_plain(counter, k, [(km, w)], [counts_from(d, 2)], ("equalised", k, side), WORD)


@pytest.mark.parametrize("k", SEAM_K)
def test_word_parallel_seams(counter, k):
    """Occurrences that end at base 254..258 and 510, 512, 513 of 300 and 520 bases and at the last base of 257."""
    km, w, want = nc.seam_case(k)
    ragged(counter, k, km, w, want, ("seams", k))


# ---- 5: the bit-sliced count ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", LISTED_K)
def test_bit_sliced_at_two_edits(counter, k):
    for side in ("start", "end"):
        km, w, d = nc.equalised_case(k, side)
        staged_and_plain(counter, k, [(km, w)], [counts_from(d, 2)], ("equalised", k, side), BITSLICE)


@pytest.mark.parametrize("E", [0, 1, 3])
@pytest.mark.parametrize("k", BUDGET_K)
def test_bit_sliced_other_budgets(ctxs, k, E):
    """d = E + 1 is not a hit, d = E is: at least 100 pairs of each in every case."""
    for side in ("start", "end"):
        km, w, d = nc.equalised_case(k, side)
        staged_and_plain(ctxs[E], k, [(km, w)], [counts_from(d, E)], ("equalised", k, side, E), BITSLICE)


# ---- 6, 7: whole windows and block ends ------------------------------------------------------------------

@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("k", WHOLE_K)
def test_bit_sliced_whole_windows(counter, ctxs, k, E):
    """The window is the occurrence: nine equal-window parts of k - 4..k + 4 bases, three to a call.  Below k
    bases only deletions can hit; at k - 4 nothing may, not even at E = 3."""
    c = counter if E == 2 else ctxs[E]
    km, groups = nc.whole_window_case(k)
    for call in (groups[0:3], groups[3:6], groups[6:9]):
        want = [counts_from(d, E) for _, _, d in call]
        staged_and_plain(c, k, [(km, w) for _, w, _ in call], want, ("whole", k, E, call[0][0]), BITSLICE)
    assert not counts_from(groups[0][2], E).any()


@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("k", BLOCK_K)
def test_bit_sliced_block_ends(counter, ctxs, k, E):
    """Four consecutive window lengths in one call: every fill of the last 4-base block; the occurrence ends at
    base L, L - 1, L - 2 and L - 3, and starts at base 0."""
    c = counter if E == 2 else ctxs[E]
    km, parts = nc.block_end_case(k)
    want = [counts_from(d, E) for _, _, d in parts]
    staged_and_plain(c, k, [(km, w) for _, w, _ in parts], want, ("block ends", k, E), BITSLICE)


# ---- 8: N near a near-miss ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", N_K)
def test_n_near_a_near_miss(counter, k):
    """An N at the edited base, before and after the occurrence, and 5 and 6 N in a 100-base window: at k = 16
    and 22 inline records and overflowed ones (count_jobs) and bitmap words (count_device); at k = 10 the
    word-parallel kernel's ragged route."""
    km, w, d, _ = nc.n_case(k)
    want = counts_from(d, 2)
    if k in LISTED_K:
        staged_and_plain(counter, k, [(km, w)], [want], ("N", k), BITSLICE)
    else:
        ragged(counter, k, km, w, want, ("N", k))


# ---- 9, 10: hit levels, end positions, co-occurrence -------------------------------------------------------

@pytest.mark.parametrize("E", [0, 1, 2, 3])
@pytest.mark.parametrize("k,L", TIE_SHAPES)
def test_levels_and_positions_at_ties(ctxs, k, L, E):
    """tie_case: hundreds of pairs at their least distance at more than one end (the first wins) and with a worse
    earlier end within E (overwritten): both matrices, the counts and the unpacked positions."""
    case = nc.tie_case(k, L)
    hit, pos, counts = nc.expected(case, E)
    got = device_positions(ctxs[E], k, [(case[0], case[1])])
    assert (got is not None) == BS_ON  # (refused, and asserted so by the helper, without the bit-sliced kernel)
    if BS_ON:
        check(got[0], hit, pos, counts, ("ties", k, L, E))


def test_levels_and_positions_from_the_jobs_stage(ctxs):
    """tie_case(16, 41) at E = 2 through window_hits_jobs(positions=True): the device route's words."""
    k, L = TIE_SHAPES[0]
    case = nc.tie_case(k, L)
    km, w = case[0], case[1]
    if not BS_ON:
        hits_refused(lambda: ctxs[2].window_hits_jobs(k, [(km, w)], positions=True), "AC_BITSLICE")
        return
    hit, pos, counts = nc.expected(case, 2)
    e_hit, e_pos, e_counts = expected_positions(k, km, w, 2)  # (and the helper at E = 2 itself)
    assert (e_hit == hit).all() and (e_pos == pos).all() and (e_counts == counts).all()
    wh = ctxs[2].window_hits_jobs(k, [(km, w)], positions=True)[0]
    assert kernel_of(ctxs[2]) == 1
    dev = device_positions(ctxs[2], k, [(km, w)])[0]
    np.testing.assert_array_equal(wh.levels, dev[1])
    np.testing.assert_array_equal(wh.planes, dev[2])
    np.testing.assert_array_equal(wh.counts, dev[0])
    np.testing.assert_array_equal(wh.levels, pack_hits(hit))
    np.testing.assert_array_equal(wh.planes, pack_positions(pos))
    np.testing.assert_array_equal(wh.end_positions(), pos)


def test_cooccurrence_of_related_candidates(ctxs):
    """The E = 2 hits of tie_case(16, 41): .cooccurrence() is the numpy product of the expected top plane, whose
    block of the adapter's tiles has no zero."""
    k, L = TIE_SHAPES[0]
    case = nc.tie_case(k, L)
    km, w = case[0], case[1]
    if not BS_ON:
        hits_refused(lambda: ctxs[2].window_hits_jobs(k, [(km, w)]), "AC_BITSLICE")
        return
    hit, _, counts = nc.expected(case, 2)
    wh = ctxs[2].window_hits_jobs(k, [(km, w)])[0]
    assert kernel_of(ctxs[2]) == 1
    np.testing.assert_array_equal(wh.counts, counts)
    h = hit[2].astype(np.float32)  # (exact below 2^24)
    want = (h.T @ h).astype(np.uint32)
    _, at = nc.candidates(k)
    assert (want[at:at + 13, at:at + 13] > 0).all()
    got = wh.cooccurrence()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.diagonal(got), hit[2].sum(axis=0))
