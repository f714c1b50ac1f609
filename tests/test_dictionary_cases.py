"""CPU test of the dictionary samples (tests/cases.py dictionary_case / dictionary_sample) that the GPU
tests of large launches (tests/test_gpu_bs_routes.py) take their expected counts from: the counts of
a sample computed from its texts' count vectors equal the oracle's on the materialised sample."""
import numpy as np
import pytest

import oracle
from tests import cases

K = 16
# (candidates, L, seed, N bases per text); the seeds are ones at which the helper's own assertions hold
SHAPES = [(40, 20, 4, cases.SHORT_N), (300, 24, 1, cases.SHORT_N), (300, 100, 1, cases.N_PER_TEXT)]


@pytest.mark.parametrize("n_kmers,L,seed,n_per_text", SHAPES)
def test_dictionary_counts_equal_the_oracle(n_kmers, L, seed, n_per_text):
    km, texts, per_text = cases.dictionary_case(seed, n_kmers, L, n_per_text=n_per_text)
    assert texts.shape == (61, L) and texts.dtype == np.uint8 and texts.max() <= 4
    assert per_text.shape == (61, n_kmers) and per_text.dtype == np.uint64
    assert len({t.tobytes() for t in texts}) == 61
    w, want = cases.dictionary_sample(texts, per_text, 5000, 3)
    assert w.shape == (5000, L) and want.dtype == np.uint64
    assert np.array_equal(want, oracle.count_myers(K, km, w))


@pytest.mark.parametrize("n_kmers,L,seed,n_per_text", SHAPES)
def test_dictionary_n_bases(n_kmers, L, seed, n_per_text):
    """Text t holds n_per_text[t % len] N bases."""
    km, texts, per_text = cases.dictionary_case(seed, n_kmers, L, n_per_text=n_per_text)
    n = (texts == 4).sum(axis=1)
    assert list(n) == [n_per_text[t % 9] for t in range(61)]
    assert L < 100 or (n >= 5).any()  # (overflows an inline N record at L = 100)


def test_dictionary_asserts_texts_that_tell_nothing():
    """The helper's own assertions: texts of mostly N have zero count vectors (the 3/4 rule, and with
    it the rule that half the texts have a vector of their own); a sample that leaves a block of 32
    candidates without a hit is refused."""
    with pytest.raises(AssertionError, match="nonzero count vector"):
        cases.dictionary_case(1, 40, 20, n_per_text=(0, 12, 12))
    km, texts, per_text = cases.dictionary_case(4, 40, 20, n_per_text=cases.SHORT_N)
    dead = per_text.copy()
    dead[:, 32:] = 0
    with pytest.raises(AssertionError, match="expect no hit"):
        cases.dictionary_sample(texts, dead, 1000, 1)
    with pytest.raises(AssertionError, match="count vector of their own"):  # one candidate: 0..3 per text
        cases.dictionary_case(3, 1, 100, n_per_text=(0,))
