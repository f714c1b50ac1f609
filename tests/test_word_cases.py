"""CPU checks of tests/word_cases.py: for every designed case of tests/test_gpu_word_parallel.py the
property its GPU test relies on, asserted on the oracle and on Python restatements of the kernel's
constants alone -- so that no GPU test there can pass vacuously."""
import numpy as np
import pytest

import oracle
from tests import cases
from tests import word_cases as wc
from tests.test_gpu_bs_routes import chunk_of


def test_geometry_restated():
    """P and the candidate group sizes of wm_count.h (cands_per_wave: 64 plain and 128 staged for P = 1,
    256 for P = 2, 192 for P = 3, 256 for P = 4), one k of WP_K per P."""
    assert [wc.pack_factor(k) for k in wc.WP_K] == [4, 3, 2, 1]
    assert [wc.pack_factor(k) for k in (2, 9, 11, 16, 22, 32)] == [4, 3, 2, 2, 1, 1]
    assert [(wc.group_size(k, False), wc.group_size(k, True)) for k in wc.WP_K] == \
        [(256, 256), (192, 192), (256, 256), (64, 128)]
    for k, counts in wc.CAND_COUNTS.items():
        g = wc.group_size(k, True)
        assert {1, 33, g - 1, g, g + 1, 2 * g + 1} <= set(counts), k
        assert k != 17 or wc.group_size(k, False) + 1 in counts
    assert wc.groups_of(17, 700, True) == 6


def test_nrec_arithmetic_matches_the_header():
    lines, claims = wc.nrec_header_claims()
    assert len(lines) == 3 and len(claims) == 9
    fn = {"bits": wc.nrec_bits, "cap": wc.nrec_cap}
    for name, L, v in claims:
        assert fn[name](L) == v, (name, L, v)
    # record capacities at the lengths of the window-length tests
    assert [wc.nrec_cap(L) for L in (100, 101, 127, 128, 129, 150, 151)] == [4, 4, 0, 0, 3, 2, 1]
    assert [wc.nrec_cap(L) for L in (16, 40, 255, 256, 257, 300)] == [4, 4, 0, 0, 0, 0]


@pytest.mark.parametrize("k", wc.WP_K + (16, 22))
def test_basic_case(k):
    km, w, want = wc.basic_case(k)
    assert len(km) == 300 and len(w) == 37 and all(len(x) == 100 for x in w)
    assert any("N" in x for x in w) and np.count_nonzero(want) > 10


@pytest.mark.parametrize("k", wc.EDGE_K)
def test_length_cases(k):
    """Counts are nonzero exactly from L = k - 2 on (a shorter window holds no occurrence at 2 edits), and
    from there the start-planted window alone adds to candidate 0: at L = k - 2 it is the whole window,
    so the hit ends at base k - 3, inside the bases whose hit accumulation skip_first skips."""
    lengths = wc.lengths_for(k)
    assert {k - 3, k - 2, k, k + 2, 16, 32, 64, 128, 256, 257, 513} <= set(lengths)
    for L in lengths:
        km, w, want = wc.length_case(k, L)
        assert len(w) == 70 and all(len(x) == L for x in w)
        assert bool(want.any()) == (L >= k - 2), L
        occ = wc.short_occurrence(km[0], k)
        assert len(occ) == k - 2 and oracle.distance(int(km[0]), k, occ) == 2
        if L >= k - 2:
            assert w[0].startswith(occ) and w[-1].endswith(occ)
            assert oracle.count_myers(k, km[:1], [w[0]])[0] >= 1
            assert oracle.count_myers(k, km[:1], [w[0][:k - 2]])[0] == 1  # ... through the hit that ends at base k - 3
            assert oracle.count_myers(k, km[:1], [w[-1][L - (k - 2):]])[0] == 1
        if L >= 40:
            assert any("N" in x for x in w)
    for kk in (16, 22):
        for L in wc.LONG_L:
            assert wc.length_case(kk, L)[2].any()


@pytest.mark.parametrize("L", wc.RECORD_L)
def test_record_jobs(L):
    """Per L: some window holds exactly as many N as its record does and some window more (L = 128: no
    record, so any N), with N on the mask words' edges; the overflow job's N-holders all overflow; the
    third job is N-free; every job's k-mers hit.  In the first job the records that hold their window's
    N hold the first spots only; the fourth job's records hold every spot."""
    cap = wc.nrec_cap(L)
    assert cap == {100: 4, 101: 4, 150: 2, 151: 1, 128: 0, 16: 4, 40: 4}[L]
    for k in wc.WP_K:
        (km, ws, want), (km2, over, want2), (km3, clean, want3), (km4, edges, want4) = wc.record_jobs(k, L)
        n = (ws > 3).sum(axis=1)
        assert (n == cap).any() and (n > cap).any() and (n == 0).any()
        for p in [p for p in wc.record_spots(L) if p < L][:6]:  # (a window of 6 N takes the first six spots)
            assert (ws[:, p] > 3).any(), p
        held = n[(n > 0) & (n <= cap)]
        assert cap == 0 or held.size > 100  # records that hold their window's N
        n2 = (over > 3).sum(axis=1)
        assert set(n2) == {0, 7} and 7 > cap
        assert not (clean > 3).any()
        assert len(km) == 300 and len(km2) == 120 and len(km3) == 64
        assert np.count_nonzero(want) > 150 and np.count_nonzero(want2) > 50 and want3.any()
        # the fourth job: every spot is held by a record of one position, and (where two fit) of two
        n4 = (edges > 3).sum(axis=1)
        assert set(n4) == {0, 1, 2} and len(km4) == 100 and np.count_nonzero(want4) > 50
        for p in wc.edge_spots(L):
            for c in (1, 2):
                assert ((edges[:, p] > 3) & (n4 == c)).any(), (p, c)
        assert wc.edge_spots(L)[-1] == L - 1 and (L < 100 or {16, 31, 32, 63, 64} <= set(wc.edge_spots(L)))


@pytest.mark.parametrize("k", wc.WP_K)
def test_group_cases(k):
    for n in wc.CAND_COUNTS[k]:
        km, w, want = wc.group_case(k, n)
        assert len(km) == n and len(w) == 37
        assert want[0] >= 3 and want[-1] >= 3  # the first and the last lane in use
    km, w, want = wc.group_case(17, 700, 90)
    assert want[0] >= 3 and want[-1] >= 3 and wc.groups_of(17, 700, True) == 6
    for n in wc.WINDOW_COUNTS:
        km, w, want = wc.group_case(k, 300, n, 101)
        assert len(w) == n and want[0] >= 3 and want[-1] >= 3


# resident wave counts a launch may have (the GPU tests read theirs from the launch)
WAVES = (1024, 4096, 8192)


def test_item_window_counts():
    for W in WAVES:
        for groups in (1, 3, 6, 10, 11, 14):
            for chunk in (1, 2, 3, 8):
                n = wc.item_windows(W, chunk, groups)
                assert chunk_of(groups * n, W) == chunk and (chunk == 1 or n % chunk)
                assert groups * n >= W * (64 * chunk + 13)  # 13 items per wave above the least: claims and steals
        na, nb = wc.fused_windows(W, 2, 10, 1)
        assert chunk_of(10 * na + nb, W) == 2 and na % 2 and nb % 2 and na != nb


@pytest.mark.parametrize("k,n_kmers,L", list(wc.DICT_SEEDS))
def test_item_dictionaries(k, n_kmers, L):
    """The dictionaries of the multi-window-item tests: the builder's own assertions hold at the chosen
    seed (3/4 of the texts count, half have a vector of their own), the samples' too (every block of 32
    candidates expects a hit) at every chunk's sample size, and a materialised sample's counts equal
    the oracle's."""
    km, texts, per = wc.item_dictionary(k, n_kmers, L)
    assert texts.shape == (wc.DICT_SEEDS[(k, n_kmers, L)][1], L) and per.shape == (len(texts), n_kmers)
    if L == 100:
        assert ((texts == 4).sum(axis=1) > wc.nrec_cap(L)).any()  # records that overflow
    w, want = cases.dictionary_sample(texts, per, 3001, 3)
    assert np.array_equal(want, oracle.count_myers(k, km, w, 16))
    for staged in (False, True):
        groups = wc.groups_of(k, n_kmers, staged)
        for W in WAVES:
            for chunk in (1, 2, 3, 8):
                n = wc.item_windows(W, chunk, groups)
                cases.dictionary_sample(texts, per, n, chunk)
                cases.dictionary_sample(texts, per, n, 10 + chunk)


@pytest.mark.parametrize("k", wc.PACK_K)
def test_pack_cases(k):
    for L in wc.PACK_L:
        km, w, want = wc.pack_case(k, L)
        assert len(w) == 1500 and all(len(x) == L for x in w) and np.count_nonzero(want) > 100
        n = np.array([x.count("N") for x in w])
        assert (n > (wc.nrec_cap(L) if L >= 100 else 0)).any() and (n == 0).any()
    km, w, smp, want = wc.pack_overflow_case(k)
    assert w[5] == "N" * 100 and "N" * 40 in w[6] and w[7][0] == w[7][-1] == "N"
    assert {4, 5, 77, 255} <= set(np.unique(smp.bases)) and np.count_nonzero(want) > 100
    assert (np.array([x.count("N") for x in w]) > 4).sum() > 200  # overflowed records
    for nw, L in wc.TAIL_SHAPES:
        if k >= 15:
            tk, tw = wc.tail_case(k, nw, L)
            assert list(oracle.count_myers(k, tk, tw)) == [3 * nw, 0]
