"""The cases of tests/test_gpu_bs_short_launch.py have the properties they are there for (no GPU)."""
import pytest

import oracle
from tests import cases
from tests import short_launch_cases as slc
from tests.test_bs_nfa_k import LISTED_K
from tests.test_budget_cpu import count_e


@pytest.mark.parametrize("k", LISTED_K)
def test_table_case_covers_every_position_and_base(k):
    """At 129 candidates and more (3 k + 1 <= 97) every (position, base) of the table belongs to some
    candidate, each non-A one among the variants to exactly one; every window holds its variant exactly and
    the variants one base apart at one edit, so a wrong table bit changes a count."""
    assert 3 * k + 1 <= 129
    for n in slc.TABLE_COUNTS:
        km, wins = slc.table_case(k, n)
        assert len(km) == n and len(set(km.tolist())) == n
        assert len(wins) == min(n, 3 * k + 1) and {len(w) for w in wins} == {k + 10}
        v = [cases.kmer_string(int(x), k) for x in km[:3 * k + 1]]
        if n >= 3 * k + 1:
            for i in range(k):
                for c in "CGT":
                    assert sum(1 for s in v if s[i] == c) == 1
                assert sum(1 for s in v if s[i] == "A") == 3 * k + 1 - 3
    km, wins = slc.table_case(k, 129)
    want = oracle.count_myers(k, km, wins)
    assert (want[:3 * k + 1] >= 3 + 2 * 3).all()  # its own window at 0 edits, three other variants' at <= 1, ...
    assert len(set(want.tolist())) > 1


@pytest.mark.parametrize("E", [0, 1, 2, 3])
def test_threshold_case_fills_every_lane(E):
    km, w, (n0, n1) = slc.threshold_case(32 * 50)
    assert len(km) == 32 and slc.lanes_per_window(len(km)) == (2, 32)
    assert n0 and n1 and n0 + n1 == len(w) and w.shape[1] == 20
    per = [count_e(E, 16, km, [t]) for t in slc.THRESHOLD_TEXTS]
    assert per[0][0] == E + 1 and per[1][0] == E + 1  # every window, every level
    if E >= 1:
        assert (per[0][1:16] == E).all()  # (one base changed)
    assert per[1][24] == E + 1 and per[0][24] < E + 1  # the two texts differ, so rows do


def test_lanes_per_window():
    assert [slc.lanes_per_window(n) for n in (1, 64, 65, 128, 129, 256)] == [(2, 32), (2, 32), (4, 16), (4, 16), (8, 8),
                                                                            (8, 8)]
