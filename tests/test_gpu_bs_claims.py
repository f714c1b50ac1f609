"""GPU tests of how the bit-sliced count kernel (bs_count.inc) hands out its work:
every row item is claimed from the sub-queues, the first one too, and a launch of more than one and at
most 1.25 rounds of row items takes 3 of every 4 workgroups that fit (count_launch.cpp).  Every case
goes through the C ABI and is compared with exact totals; what the launch planned is read with
ac_last_launch.  The shapes of test_gpu_bitslice.py: 3 equal candidates (2 lanes per window: rows of
32 windows) that hit every window at all three levels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from tests import cases

pytestmark = pytest.mark.gpu
K = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITSLICE = os.environ.get("AC_BITSLICE", "1") != "0"
TEXT = "ACGTACGTTGCAAGCTACGT"
KM = np.array([cases.kmer_value(TEXT[:K])] * 3, np.uint64)


def count_rows(counter, rows):
    """`rows` rows of 32 windows on a resident image: (counts, the launch's waves, its items per wave)."""
    import torch

    w = np.tile(ac.to_dna5(TEXT), (rows * 32, 1))
    seg = ac.DeviceSegment.upload(KM, ac.pack_windows(w))
    counter.count_device(K, [seg], window_len=[len(TEXT)])
    torch.cuda.synchronize()
    counter.check()
    geo = counter.last_launch()
    return seg.counts_numpy(), int(geo["waves"]), int(geo["windows_per_wave"]), len(w)


def fitting_waves(counter):
    """The waves of a launch of less than one round of the same kernel (a resident image): all that fit."""
    return count_rows(counter, 1)[1]


@pytest.mark.parametrize("num,den,extra,share", [(1, 2, 0, 4), (1, 1, 0, 4), (1, 1, 1, 3), (9, 8, 0, 3), (5, 4, 0, 3),
                                                 (5, 4, 1, 4), (2, 1, 0, 4), (7, 2, 0, 4)])
def test_rounds_and_launched_waves(counter, num, den, extra, share):
    """num / den rounds of rows (of the waves that fit) + extra rows: up to one round and above 1.25,
    every workgroup that fits is launched; between them (one row above one round, 1.25 rounds exactly)
    3 of 4.  Exact totals at every size: each row is claimed once, whichever wave takes it."""
    fit = fitting_waves(counter)
    assert fit >= 64 and fit % 16 == 0
    rows = fit * num // den + extra
    got, waves, per_wave, n = count_rows(counter, rows)
    assert list(got) == [3 * n] * 3
    if BITSLICE and "AC_BS_WAVES_PCT" not in os.environ:
        assert waves == fit * share // 4
        assert per_wave == -(-rows // waves)


@pytest.mark.parametrize("num,den", [(9, 8), (9, 4)])
def test_rows_that_differ(counter, num, den):
    """Rows that are not alike, so a row counted twice in place of another shows: every window holds one
    of two texts, chosen at random (30 % the second), each an exact occurrence of one candidate and no
    hit of the other at any level (checked with the oracle on the two texts).  Row r also differs from
    row r + 1 in how many of its 32 windows hold the second text in all but a few cases."""
    alt = "TTGACCATGCAGTCAAGGTC"
    km = np.array([cases.kmer_value(TEXT[:K]), cases.kmer_value(alt[:K])], np.uint64)
    one = oracle.count_myers(K, km, [TEXT, alt])
    assert list(oracle.count_myers(K, km, [TEXT])) == [3, 0] and list(one) == [3, 3]
    import torch

    rows = fitting_waves(counter) * num // den + 1
    pick = np.random.default_rng(num).random(rows * 32) < 0.3
    w = np.where(pick[:, None], ac.to_dna5(alt)[None, :], ac.to_dna5(TEXT)[None, :]).astype(np.uint8)
    seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
    counter.count_device(K, [seg], window_len=[len(TEXT)])
    torch.cuda.synchronize()
    counter.check()
    assert list(seg.counts_numpy()) == [3 * int((~pick).sum()), 3 * int(pick.sum())]


def test_fewer_rows_than_sub_queues(counter):
    """1, 2, 5 and 33 rows: most sub-queues hold no item, and the waves that find theirs empty steal or stop."""
    for rows in (1, 2, 5, 33):
        got, _, _, n = count_rows(counter, rows)
        assert list(got) == [3 * n] * 3, rows


def test_forced_share_by_environment():
    """AC_BS_WAVES_PCT (read once per process: a child) sets the share for every bit-sliced launch: 50 %
    of the waves at 3.5 rounds, exact totals."""
    code = ("import approx_counter_amd as ac\nfrom tests.test_gpu_bs_claims import fitting_waves, count_rows\n"
            "with ac.ApproxCounter(0) as c:\n    half = fitting_waves(c)\n    got, waves, _, n = count_rows(c, 7 * half)\n"
            "    assert waves == half and list(got) == [3 * n] * 3, (waves, half)\nprint('OK', half)")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AC_BS_WAVES_PCT="50", PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
