"""Device packing of a pinned block whose byte count is no multiple of 4: the copier
workgroups read the Dna5 bytes in dwords through a range-checked buffer descriptor, and a dword that
holds the block's last bytes but reaches past them must still be read -- or the sample's last window
loses up to 3 bases and an occurrence that ends there is missed."""
import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases

pytestmark = pytest.mark.gpu
AC_TESTING_DEVICE_PACK = 8


@pytest.mark.parametrize("k", [16, 22])
@pytest.mark.parametrize("n_windows,L", [(1, 151), (2, 101), (3, 150), (1, 100)])
def test_an_occurrence_at_the_blocks_last_bytes(counter, k, n_windows, L):
    """Blocks of 151, 202, 450 and (the control) 100 bytes; every window ends with the k-mer."""
    kmer = "ACGTACGTTGCAAGCTGATTACAGGCATTCAG"[:k]
    km = np.array([cases.kmer_value(kmer), cases.kmer_value("T" * k)], np.uint64)
    wins = [("C" * L)[:L - k] + kmer for _ in range(n_windows)]
    prev = _lib.load().ac_testing_stage_hooks(AC_TESTING_DEVICE_PACK)
    try:
        got = counter.count_jobs(k, ac.Jobs([(km, ac.Dna5Sample.from_windows(wins).pinned())]))[0]
        assert counter.stage_mode() == 3
    finally:
        _lib.load().ac_testing_stage_hooks(prev)
    want = oracle.count_myers(k, km, wins)
    assert list(want) == [3 * n_windows, 0]
    assert np.array_equal(got, want)
