"""CPU checks of tests/exact_cases.py: the mirrors of the partition's hash and geometry, and for every
designed sample of tests/test_gpu_exact_edges.py the condition its GPU test relies on, asserted on
the reference alone -- so that no GPU test there can pass vacuously."""
import random

import numpy as np
import pytest

import approx_counter_amd as ac
from oracle import host_ref
from tests import cases
from tests import exact_cases as xc


def test_hash_inverse_round_trip():
    rng = random.Random(1)
    for x in [0, 1, xc.M32] + [rng.randrange(1 << 32) for _ in range(10**4)]:
        assert xc.inv_part_hash32(xc.part_hash32(x)) == x
        assert xc.part_hash32(xc.inv_part_hash32(x)) == x


def test_hash_mirror_known_values():
    """The mixer by hand for one word (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
    x ^= x >> 16), and the 64-bit fold."""
    x = 0x12345678
    y = x ^ (x >> 16)
    y = (y * 0x7FEB352D) % (1 << 32)
    y ^= y >> 15
    y = (y * 0x846CA68B) % (1 << 32)
    y ^= y >> 16
    assert xc.part_hash32(x) == y
    assert xc.part_hash32(0) == 0
    key = (0xABCDEF01 << 32) | x
    assert xc.part_hash64(key) == xc.part_hash32(x ^ xc.part_hash32((0xABCDEF01 + 0x9E3779B9) % (1 << 32)))
    assert xc.part_hash(x, 16) == xc.part_hash32(x) and xc.part_hash(key, 32) == xc.part_hash64(key)


@pytest.mark.parametrize("k", [16, 17, 22, 32])
@pytest.mark.parametrize("nb_log2", [7, 12, 16])
def test_crafted_keys_land_where_asked(k, nb_log2):
    bucket = (1 << nb_log2) - 3
    slots = [0, 1, 2047, 4095]
    keys = xc.crafted_keys(k, nb_log2, bucket, slots, 5)
    assert len(keys) == 20 and len(set(keys)) == 20
    for i, v in enumerate(keys):
        assert 0 <= v < (1 << (2 * k)) and v != xc.all_t(k)
        assert xc.bucket_of(v, k, nb_log2) == bucket
        assert xc.home_slot(v, k) == slots[i // 5]


def test_geometry_rule():
    assert xc.nb_log2_for(0) == xc.nb_log2_for(32) == xc.nb_log2_for(2048 << 6) == 6
    for nb in range(7, 17):
        assert xc.nb_log2_for(xc.min_bases_for(nb)) == nb
        assert xc.nb_log2_for(xc.min_bases_for(nb) - 32) == nb - 1
    assert xc.nb_log2_for(1 << 40) == 16
    # buckets per super-bucket over the sweep: 2, 4, .., 32 (dense), 128 (sparse)
    assert [1 << (nb - xc.s_log2_for(nb)) for nb in range(6, 17)] == [1, 1, 2, 4, 8, 16, 32, 64, 128, 128, 128]
    for nb in xc.DENSE_NB:
        n_bases = xc.dense_windows_n(nb) * 128
        assert xc.nb_log2_for(n_bases) == nb
        assert n_bases - (1 << (10 + nb)) <= 2048  # just above 2^(10 + nb_log2)
    # nb_log2 = 10: 129 level-1 chunks of 8,192 32-bit keys, 257 of 4,096 64-bit keys
    n_bases = xc.dense_windows_n(10) * 128
    assert (-(-n_bases // 8192), -(-n_bases // 4096)) == (129, 257)


def _base(smp, i):
    if (int(smp.nmask[i // 32]) >> (i % 32)) & 1:
        return "N"
    return "ACGT"[(int(smp.codes[i // 16]) >> (2 * (i % 16))) & 3]


def test_placed_and_padded_keep_the_windows():
    rng = random.Random(3)
    groups = [[cases.rand_seq(rng, rng.randint(0, 90), p_n=0.05) for _ in range(7)] for _ in range(3)]
    parts = [ac.pack_windows(g) for g in groups]
    n_bases = 4096
    smp = xc.placed([(parts[0], 0), (parts[1], 2048), (parts[2], n_bases - parts[2].n_bases)], n_bases)
    assert smp.n_bases == n_bases and smp.codes.size == n_bases // 16 and smp.nmask.size == n_bases // 32
    wins = [w for g in groups for w in g]
    assert smp.n_windows == len(wins)
    covered = np.zeros(n_bases, bool)
    for w, st, ln in zip(wins, smp.start, smp.length):
        assert int(st) % 32 == 0 and int(ln) == len(w)
        assert "".join(_base(smp, int(st) + i) for i in range(len(w))) == w
        covered[int(st): int(st) + len(w)] = True
    assert int(smp.start[-1]) + 32 > n_bases - 32 * 4  # the last window sits in the image's last slots
    # nothing but the windows' bases is set: the padding holds no code and no N flag
    every = np.arange(n_bases)
    stray = ((smp.codes[every // 16] >> (2 * (every % 16)).astype(np.uint32)) & 3) | \
        ((smp.nmask[every // 32] >> (every % 32).astype(np.uint32)) & 1)
    assert not stray[~covered].any()
    p0 = parts[0]
    one = xc.padded(p0, 1024)
    assert np.array_equal(one.codes[: p0.codes.size], p0.codes) and not one.codes[p0.codes.size:].any()
    assert np.array_equal(one.nmask[: p0.nmask.size], p0.nmask) and not one.nmask[p0.nmask.size:].any()
    assert np.array_equal(one.start, p0.start) and np.array_equal(one.length, p0.length)
    assert one.n_bases == 1024 and one.n_bases % 32 == 0


@pytest.mark.parametrize("k", [16, 22])
def test_ragged_reference_is_count_kmers(k):
    a, b, c = xc.sparse_windows()
    wins = a[:25] + b[:10] + c[-25:]  # the hand-made low-complexity, empty and short windows included
    thr = np.float32(xc.lc_threshold(k))
    counter, had_n = host_ref.count_kmers(wins, k, thr)
    uk, cnt, had = xc.ragged_reference(wins, k, thr)
    assert dict(zip(uk.tolist(), cnt.tolist())) == counter and had == had_n and had_n > 0
    top = host_ref.get_most_frequent(counter, 30, k)
    assert host_ref.rank_dense(uk, cnt, 30, 0, k) == top


def test_sparse_samples_choose_their_geometry():
    groups = xc.sparse_windows()
    assert sum(len(g) for g in groups) == 2000
    for nb in xc.SPARSE_NB:
        smp = xc.sparse_sample(nb)
        assert xc.nb_log2_for(smp.n_bases) == nb and smp.n_windows == 2000
        assert int(smp.start[0]) == 0
        last = int(np.max(smp.start + smp.length.astype(np.uint64)))
        assert smp.n_bases - 32 < last <= smp.n_bases  # the last window ends in the image's last slot
        tail = xc.sparse_tail_sample(nb)
        assert xc.nb_log2_for(tail.n_bases) == nb and tail.n_windows == 7
        assert int(tail.start[0]) >= tail.n_bases - 7 * 64  # all of it in the last slots
    for k in (16, 22):
        counter, _ = host_ref.count_kmers(xc.sparse_tail_windows(), k, 100.0)
        supers = {xc.part_hash(v, k) >> (32 - 7) for v in counter}
        assert 5 < len(counter) and len(supers) < 100 and xc.all_t(k) in counter  # empty super-buckets
        assert len(host_ref.count_kmers(xc.sparse_tail_windows(), k, xc.lc_threshold(k))[0]) < len(counter)
    for k in (16, 22):
        uk, cnt, had = xc.sparse_reference(k)
        assert uk.size > 200 and had > 0 and int(cnt.max()) > 1  # limit = 200 cuts, limit = 10^6 lists all


def _simulate_table(keys, k):
    """The per-bucket table filled one key after another (linear probing from the home slot, at most
    COUNT_PROBES probes): (largest probe index used, keys left without a slot)."""
    table, worst, lost = {}, 0, 0
    for v in keys:
        h = xc.home_slot(v, k)
        for probe in range(xc.COUNT_PROBES):
            s = (h + probe) % xc.BUCKET_SLOTS
            if s not in table:
                table[s] = v
                worst = max(worst, probe)
                break
        else:
            lost += 1
    return worst, lost


@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("name", list(xc.OVERFLOW_CASES))
def test_overflow_cases(name, k):
    """Crafted families at threshold 100.0: the bucket holds exactly the crafted keys, nothing is
    filtered, and the table's outcome does not depend on the order of the inserts: with distinct home
    slots every key claims its own at probe 0; 4,097 keys cannot fit 4,096 slots; n keys of one home
    slot h can only take slots h .. h + 63, which holds 64 of them (the last claimer at probe index
    63) and not 65."""
    wins, keys, copies, bucket, path = xc.overflow_case(name, k)
    assert len(set(keys)) == len(keys)
    assert all(xc.bucket_of(v, k, xc.OVERFLOW_NB) == bucket for v in keys)
    smp = xc.overflow_sample(wins)
    assert xc.nb_log2_for(smp.n_bases) == xc.OVERFLOW_NB and xc.s_log2_for(xc.OVERFLOW_NB) == 7
    counter, had_n = host_ref.count_kmers(wins, k, 100.0)
    in_bucket = {v: c for v, c in counter.items() if xc.bucket_of(v, k, xc.OVERFLOW_NB) == bucket}
    assert in_bucket == dict(zip(keys, copies))
    assert len(counter) > len(keys) + 1000 and had_n > 0  # other buckets are not empty; N-skips to count
    slots = [xc.home_slot(v, k) for v in keys]
    worst, lost = _simulate_table(keys, k)
    worst_r, lost_r = _simulate_table(keys[::-1], k)
    if name == "full_table":
        assert sorted(slots) == list(range(xc.BUCKET_SLOTS)) and (worst, lost) == (0, 0)
    elif name == "pigeonhole":
        assert len(keys) == xc.BUCKET_SLOTS + 1 and lost >= 1 and lost_r >= 1
    elif name == "probe_limit":
        assert len(keys) == 64 and len(set(slots)) == 1 and (worst, lost) == (63, 0) == (worst_r, lost_r)
    else:
        assert len(keys) == 65 and len(set(slots)) == 1 and lost == 1 == lost_r
    assert path == (0 if lost else 1)


@pytest.mark.parametrize("k", [16, 22])
def test_count_bins_case(k):
    w, keys, copies = xc.count_bins_case(k)
    assert w.shape == (sum(copies) + xc.BIN_N_WINDOWS, k)
    uk, cnt, had = xc.count_bins_reference(k)
    assert dict(zip(uk.tolist(), cnt.tolist())) == dict(zip(keys, copies))  # nothing filtered
    assert uk.size == 40 and had == xc.BIN_N_WINDOWS
    counts = sorted(cnt.tolist())
    # both sides of every bin edge are present: phist (32 | 33), the last bin (4094 | 4095), and ties in it
    for c in (1, 2, 32, 33, 4094, 4095, 4096, 5000, 70000):
        assert c in counts
    assert counts.count(5000) == 2 and counts.count(4095) == 2
    assert xc.BIN_LIMITS[5] == sum(c >= 33 for c in counts) == 9
    for lim in xc.BIN_LIMITS:
        assert len(host_ref.rank_dense(uk, cnt, lim, 0, k)) == min(lim, 40)
    sizes = [len(host_ref.rank_dense(uk, cnt, 0, s, k)) for s in xc.BIN_SOLIDS]
    assert sizes == [40, 14, 11, 9, 6, 4, 3, 1, 0]
    # the small reference agrees with the loop restatement (the dense one is used at 10^5 windows)
    first = host_ref.get_most_frequent(dict(zip(uk.tolist(), cnt.tolist())), 40, k)
    assert host_ref.rank_dense(uk, cnt, 10**6, 0, k) == first


@pytest.mark.parametrize("count", xc.ALL_T_COUNTS)
@pytest.mark.parametrize("k", xc.ALL_T_KS)
def test_all_t_case(k, count):
    wins, others = xc.all_t_case(k, count)
    t = xc.all_t(k)
    counter, _ = host_ref.count_kmers(wins, k, 100.0)
    assert counter[t] == count and len(counter) == len(others) + 1  # nothing filtered at 100.0
    without, _ = host_ref.count_kmers(wins, k, 100.0, {t, others[0]})
    assert t not in without and len(without) == len(counter) - 2
    kept, _ = host_ref.count_kmers(wins, k, 100.0, set(others[:3]))
    assert kept[t] == count and len(kept) == len(counter) - 3
    low, _ = host_ref.count_kmers(wins, k, 1.0)
    assert t not in low and len(low) > 0


@pytest.mark.parametrize("k", xc.N_POSITION_KS)
def test_n_position_case(k):
    wins = xc.n_position_case(k)
    assert len(wins) == 82 and all(len(w) == 80 for w in wins)
    assert all(w.count("N") == 1 and w[p] == "N" for p, w in enumerate(wins[:80]))
    _, had_n = host_ref.count_kmers(wins, k, 100.0)
    npos = 80 - k + 1
    covering = [min(p, npos - 1) - max(0, p - k + 1) + 1 for p in range(80)]  # k-mer positions over base p
    assert had_n == sum(covering) + 2 * (covering[0] + covering[79])


@pytest.mark.parametrize("k", xc.SCORE_KS)
def test_score_case(k):
    """At each threshold the reference keeps some k-mers and drops others (except where no set of
    k-mers can: k = 3 and k = 4 attain two and three sums, so a threshold at or below their lowest
    score drops everything and one above their highest keeps everything); the k-mers that score equal
    to a picked sum exist and change sides between that threshold and the float32 above it; and the
    vectorised score used as the reference equals getComplexity's on every k-mer of the set."""
    w, thresholds, picked = xc.score_case(k)
    assert len(thresholds) == 3 * len(picked) and len(set(picked)) == len(picked) == (2 if k == 3 else 3)
    keys = np.array([cases.kmer_value(s) for s in xc.strings(w)], np.uint64)
    uniq = np.unique(keys)
    scores = host_ref.complexity_dense(uniq, k)
    assert [float(s) for s in scores] == [float(host_ref.get_complexity(int(v), k)) for v in uniq]
    sums = np.array([xc.dimer_sum(int(v), k) for v in uniq])
    for i, s in enumerate(picked):
        below, at, above = thresholds[3 * i: 3 * i + 3]
        assert below < at < above and at == np.float32(s) / np.float32(2 * (k - 2))
        equal = sums == s
        assert equal.any() and (scores[equal] == at).all()
        for thr in (below, at, above):
            dropped = scores >= thr
            assert np.array_equal(dropped, sums >= s if thr <= at else sums > s)
            if sums.min() < s < sums.max():
                assert dropped.any() and not dropped.all()
            uk, _, _ = host_ref.count_kmers_dense(w, k, thr)
            assert np.array_equal(uk, uniq[~dropped])
        assert (scores[equal] >= at).all() and not (scores[equal] >= above).any()
    if k >= 8:
        assert all(sums.min() < s < sums.max() for s in picked)
