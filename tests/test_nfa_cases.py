"""The designed cases of tests/nfa_cases.py on the CPU: each builder has the property its GPU test
(tests/test_gpu_nfa_cases.py) relies on -- the builders assert them; the figures are printed (`pytest -s`) and
written down in DESIGN.md §4e -- the builders are deterministic, and every GPU test would fail on a subtly
wrong kernel: the two mutations of the expected side (a pair at d = E + 1 counted as a hit; the last end at the
least distance instead of the first) change the expected values of every case a GPU test uses -- but for
exhaustive_small(2), where no pair is further than 2 edits and nothing sits at d = E + 1.

The cases also run through the stand-alone host programs of the arithmetic headers, built as
tests/test_budget_cpu.py and tests/test_positions_cpu.py build them (g++, address and undefined-behaviour
sanitizers, a child process): tools/bs_nfa_r_check.cpp `count kernel|rows E` on near_miss_case at every listed
k and E = 0..3, tools/bs_pos_check.cpp `pos E` on tie_case at k = 16, 22, 32 and E = 0..3.  They are the pin
that bs_nfa_r.h and bs_pos.h are not what a failure of the GPU file is about."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
from tests import cases
from tests import nfa_cases as nc
from tests.positions_cases import pack_hits
from tests.test_bs_nfa_k import LISTED_K
from tests.test_gpu_nfa_cases import BLOCK_K, EQ_WORD_K, N_K, SEAM_K, SMALL_K, TIE_SHAPES, WHOLE_K
from tests.test_budget_cpu import CSRC, ROOT, SANITIZE, counts_from, distances, run_count
from tests.test_positions_cpu import run_pos

NEAR_K = sorted(set(LISTED_K) | {5, 8, 9, 10, 11, 15, 17})


def as_hit(d, E):
    """The first mutation: d = E + 1 counts as a hit at level E."""
    return np.where(d == E + 1, E, d)


# ---- the edits ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 16, 32])
def test_neighbourhood_is_what_it_says(k):
    s = nc.randoms_of(k)[0]
    one = nc.single_edits(s)
    assert len(one) == 3 * k + k + 4 * (k + 1)
    for kind, p, t in one:
        assert len(t) == k + {"sub": 0, "del": -1, "ins": 1}[kind]
        if kind != "del":
            assert t[:p] == s[:p] and t[p + 1:] == s[p + (kind == "sub"):]
    for n in (2, 3, 4)[:k - 3]:
        for where in nc.PLACEMENTS:
            pos = nc.placement(k, n, where)
            assert len(set(pos)) == n and all(0 <= p < k for p in pos)
        assert nc.placement(k, n, "head") == list(range(n)) and nc.placement(k, n, "tail") == list(range(k - n, k))
        assert nc.placement(k, n, "spread")[0] == 1 and nc.placement(k, n, "spread")[-1] == k - 2
    many = nc.multi_edits(s, 4)
    assert len(many) == 5 * sum(3 ** n for n in (2, 3, 4) if n <= k - 2)
    nb = nc.neighbourhood(s, 4)
    assert len(set(nb)) == len(nb) and {len(t) for t in nb} == set(range(k - min(4, k - 2), k + min(4, k - 2) + 1))
    # within n_max edits of s, and each distance 1..4 is there (the window is the whole string's neighbourhood)
    d = distances(k, [cases.kmer_value(s)], nb, 5)[0]
    assert d.max() <= 4 and set(d.tolist()) >= set(range(1, min(4, k - 2) + 1))


@pytest.mark.parametrize("k", NEAR_K)
def test_candidates(k):
    lc = nc.low_complexity(k)
    assert len(set(lc)) == len(lc) and all(len(s) == k and set(s) <= set("ACGT") for s in lc)
    assert {c * k for c in "ACGT"} <= set(lc) and (len(lc) >= 45 or k < 9)
    for p, unit in nc.UNITS.items():
        assert all(nc.periodic(unit, ph, k) in lc for ph in range(p))
    km, at = nc.candidates(k)
    tl = nc.tiles(nc.adapter_of(k), k)
    assert len(tl) == 13 and all(a[1:] == b[:-1] for a, b in zip(tl, tl[1:]))
    assert km[at:at + 13] == tl == km[at + 32:at + 45] and len(km) == len(lc) + 6 + 26 <= 80
    assert set(lc) | set(nc.randoms_of(k)) <= set(km)


# ---- the near-miss case --------------------------------------------------------------------------------

@pytest.mark.parametrize("k", NEAR_K)
def test_near_miss_case(k):
    """At least 200 pairs at each exact distance 0..4, every budget's count apart from the one below for half of
    the k-mers, the DP at E = 2 equal to oracle.count_myers (asserted by the builder); ragged; deterministic."""
    km, w, d = nc.near_miss_case(k)
    pop = nc.populations(d)
    print(f"near_miss_case k {k}: {len(km)} k-mers x {len(w)} windows, pairs at d = 0..4 {pop}")
    assert min(pop) >= 200 and len(km) <= 80 and len(w) <= 5000
    assert len({len(x) for x in w}) > 9 and len(set(w)) == len(w) and all(set(x) <= set("ACGT") for x in w)
    assert nc.near_miss_inputs(k) == (km, w) == nc.near_miss_inputs(k)
    for E in range(4):
        assert (counts_from(as_hit(d, E), E) != counts_from(d, E)).any()


@pytest.mark.parametrize("k", sorted(set(LISTED_K) | set(EQ_WORD_K)))
def test_equalised_case(k):
    """Padded to k + 9 bases at either side the d = E + 1 population still holds 100 pairs for every E."""
    _, w0, _ = nc.near_miss_case(k)
    for side in ("start", "end"):
        km, w, d = nc.equalised_case(k, side)
        print(f"equalised_case k {k} {side}: pairs at d = 0..4 {nc.populations(d)}")
        assert len(w) == len(w0) and all(len(x) == k + 9 for x in w)
        short = [(a, b) for a, b in zip(w0, w) if len(a) <= k + 9]
        assert all(b.startswith(a) if side == "start" else b.endswith(a) for a, b in short)
        assert nc.equalised(w0, k + 9, side) == w
        for E in range(4):
            assert int((d == E + 1).sum()) >= 100
            assert (counts_from(as_hit(d, E), E) != counts_from(d, E)).any()


@pytest.mark.parametrize("k", WHOLE_K)
def test_whole_window_case(k):
    """Nine equal-window parts, k - 4..k + 4 bases; nothing within 3 edits at k - 4, deletions only below k; sent
    three parts to a call, every call holds pairs at d = E + 1 for E = 2 and 3."""
    km, groups = nc.whole_window_case(k)
    assert [L for L, _, _ in groups] == list(range(k - 4, k + 5))
    for L, w, d in groups:
        assert all(len(x) == L for x in w) and d.shape == (len(km), len(w)) and d.min() >= max(k - L, 0)
    for call in (groups[0:3], groups[3:6], groups[6:9]):
        d = np.concatenate([g[2] for g in call], axis=1)
        for E in (2, 3):
            assert (counts_from(as_hit(d, E), E) != counts_from(d, E)).any()


# ---- ties ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,L", TIE_SHAPES)
def test_tie_case(k, L):
    """At least 500 pairs within 3 edits at their minimum at more than one end, at least 100 with a worse earlier
    end within E (asserted by the builder); both mutations change the expected values at every budget."""
    case = nc.tie_case(k, L)
    km, w, hit3, pos3, tied, over = case
    print(f"tie_case ({k}, {L}): {len(w)} windows, tied pairs at E = 0..3 {tied}, overwritten {over}")
    assert tied[3] >= 500 and over[3] >= 100 and len(w) <= 800 and all(len(x) == L for x in w)
    assert nc.tie_inputs(k, L) == (km, w)
    e = nc.tie_rows(k, L)
    d = e.min(axis=2)
    for E in range(4):
        hit, pos, counts = nc.expected(case, E)
        assert hit.shape == (E + 1, len(w), len(km)) and ((pos > 0) == hit[E]).all()
        np.testing.assert_array_equal(counts, counts_from(np.minimum(d, 5).T, E))
        assert ((d == E + 1) & ~hit[E]).any()  # counted as a hit, level E's matrix and the counts change
        last = nc.last_end_positions(e, E)
        assert ((last > 0) == (pos > 0)).all() and (last >= pos).all()
        assert int((last != pos).sum()) == tied[E] > 0


def test_tie_case_cooccurrence_block_is_dense():
    """The tiles' block of the E = 2 co-occurrence of tie_case(16, 41) has no zero: neighbouring tiles share
    windows, which random candidates never do."""
    case = nc.tie_case(16, 41)
    _, at = nc.candidates(16)
    h = nc.expected(case, 2)[0][2].astype(np.float32)
    co = (h.T @ h).astype(np.uint32)
    assert (co[at:at + 13, at:at + 13] > 0).all() and (co[at:at + 13, at + 32:at + 45] > 0).all()
    rnd = [i for i, s in enumerate(nc.candidates(16)[0]) if s in nc.randoms_of(16)[1:]]
    assert not co[np.ix_(rnd, rnd)][~np.eye(len(rnd), dtype=bool)].all()
    assert pack_hits(nc.expected(case, 2)[0]).shape == (3, len(case[1]), 3)


# ---- seams, block ends, N, exhaustive --------------------------------------------------------------------

@pytest.mark.parametrize("k", sorted(set(SEAM_K) | {32}))
def test_seam_case(k):
    km, w, want = nc.seam_case(k)
    t = nc.occurrences(k)[0]
    ends = [e for _, es in nc.SEAM_ENDS for e in es]
    assert ends == [254, 255, 256, 257, 258, 510, 512, 513, 257]
    assert [x[e - len(t):e] for x, e in zip(w, ends)] == [t] * 9 and len(w[-1]) == 257
    assert {len(x) for x in w} == {300, 520, 257} and len(w) == 9 * len(nc.occurrences(k))
    assert want.shape == (len(km),)
    d = distances(k, km, w, 4)
    np.testing.assert_array_equal(counts_from(d, 2), want)
    assert (counts_from(as_hit(d, 2), 2) != want).any()
    assert nc.seam_inputs(k) == w


@pytest.mark.parametrize("k", BLOCK_K)
def test_block_end_case(k):
    km, parts = nc.block_end_case(k)
    lens = [L for L, _, _ in parts]
    assert lens == nc.block_end_lengths(k) and sorted(L % 4 for L in lens) == [0, 1, 2, 3] and lens[0] % 4 == 1
    assert lens[0] >= k + 21
    occ = nc.occurrences(k)
    for L, w, d in parts:
        t = occ[0]
        assert [x[L - b - len(t):L - b] for b, x in enumerate(w[:4])] == [t] * 4 and w[4].startswith(t)
        assert len(w) == 5 * len(occ) and all(len(x) == L for x in w)
        print(f"block_end_case k {k} L {L}: pairs at d = 0..4 {nc.populations(d)}")
        for E in (2, 3):
            assert (counts_from(as_hit(d, E), E) != counts_from(d, E)).any()
    assert nc.block_end_inputs(k) == [p[:2] for p in parts]


@pytest.mark.parametrize("k", sorted(set(N_K) | {32}))
def test_n_case(k):
    """The N matter: the counts differ from those of the same windows without them (asserted by the builder at
    every budget); N at the edited base, before and after the occurrence; windows of 5 and 6 N."""
    km, w, d, d_clean = nc.n_case(k)
    assert all(len(x) == 100 for x in w) and sorted({x.count("N") for x in w}) == [1, 5, 6]
    assert (d >= d_clean).all() and (d > d_clean).any()
    print(f"n_case k {k}: {len(w)} windows, pairs at d = 0..4 {nc.populations(d)}, without the N {nc.populations(d_clean)}")
    assert (counts_from(as_hit(d, 2), 2) != counts_from(d, 2)).any()
    assert nc.n_inputs(k)[0] == w


@pytest.mark.parametrize("k", SMALL_K)
def test_exhaustive_small(k):
    km, w, want = nc.exhaustive_small(k)
    assert len(km) == 4 ** k and len(w) == sum(4 ** n for n in range(k + 4)) + (k + 1) * 4 ** k
    assert w[0] == "" and len(set(w)) == len(w)
    np.testing.assert_array_equal(want, oracle.count_myers(k, km, w))
    # the first mutation on the case itself (k = 4: on every 37th window -- it only ever adds to a count, so what
    # it adds there it adds to the whole case's counts).  At k = 2 no pair is further than 2 edits: nothing sits
    # at d = 3 and this mutation changes nothing; there the case holds every distance 0..2 instead.
    sub = w if k < 4 else w[::37]
    d = distances(k, km, sub, 4)
    true = counts_from(d, 2)
    np.testing.assert_array_equal(true, oracle.count_dp(k, km, sub))
    added = counts_from(as_hit(d, 2), 2) - true
    assert added.any() == (k > 2) and set(d.ravel().tolist()) >= set(range(min(3, k) + 1)) and d.max() <= k


# ---- the host harnesses ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    """Both programs, compiled side by side: {name: executable}."""
    where = tmp_path_factory.mktemp("nfa_cases")
    names = ("bs_nfa_r_check", "bs_pos_check")
    jobs = [subprocess.Popen(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", n + ".cpp"), "-o", str(where / n)])
            for n in names]
    assert [j.wait(timeout=600) for j in jobs] == [0, 0]
    return {n: str(where / n) for n in names}


@pytest.fixture(scope="module")
def count_tool(tools):
    return tools["bs_nfa_r_check"]


@pytest.fixture(scope="module")
def pos_tool(tools):
    return tools["bs_pos_check"]


def in_children(tmp_path, runs, fn):
    """fn(directory of its own, *run) for every run, the child processes side by side (4 at a time)."""
    def one(run):
        d = tmp_path / "_".join(str(x) for x in run)
        d.mkdir()
        return fn(d, *run)

    with ThreadPoolExecutor(4) as pool:
        return dict(zip(runs, pool.map(one, runs)))


@pytest.mark.parametrize("k", LISTED_K)
def test_host_nfa_counts_the_near_miss_case(count_tool, tmp_path, k):
    """bs_nfa_r.h, both forms, E = 0..3, on near_miss_case(k): the DP's counts."""
    km, w, d = nc.near_miss_case(k)
    runs = [(form, E) for E in range(4) for form in ("kernel", "rows")]
    got = in_children(tmp_path, runs, lambda dr, form, E: run_count(count_tool, dr, form, E, k, km, w)[0])
    for form, E in runs:
        np.testing.assert_array_equal(got[form, E], counts_from(d, E), err_msg=f"K {k} E {E} {form}")


@pytest.mark.parametrize("k,L", TIE_SHAPES)
def test_host_nfa_positions_of_the_tie_case(pos_tool, tmp_path, k, L):
    """bs_pos.h, E = 0..3, on tie_case: every pair's distance level and position are the Sellers DP's."""
    case = nc.tie_case(k, L)
    got = in_children(tmp_path, [(E,) for E in range(4)], lambda dr, E: run_pos(pos_tool, dr, E, k, case[0], case[1]))
    for E in range(4):
        hit, pos, _ = nc.expected(case, E)
        d_got, p_got = got[E,]
        np.testing.assert_array_equal(d_got, np.where(hit[E], hit.shape[0] - hit.sum(axis=0), -1), err_msg=f"levels {k} {E}")
        np.testing.assert_array_equal(p_got, np.where(pos > 0, pos, 0), err_msg=f"positions {k} {E}")
