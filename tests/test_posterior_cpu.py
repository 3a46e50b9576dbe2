"""The host side of the posterior summary (pyratbay_amd/posterior.py), no GPU: the NumPy statement
of the weighted-quantile kernel against np.percentile of the real expansion, bit for bit, and the
deduplication of a chain as the reference does it (tools/retrieval_tools.py:440-442)."""
import numpy as np
import pytest

from pyratbay_amd import posterior as post

Q_ALL = post.QUANTILES + [0.0, 1.0, 0.25]


def expansion(counts):
    """An inverse index that repeats sample i counts[i] times, shuffled like a chain."""
    inverse = np.repeat(np.arange(len(counts)), counts)
    return np.random.default_rng(len(inverse)).permutation(inverse)


@pytest.mark.parametrize('kind', ['levels', 'normal'])
def test_host_statement_equals_percentile(kind):
    """200 random cases per kind, n = 1 ... 40, three columns each: values from five levels of
    mixed sign (ties) or from a normal distribution, counts 0 ... 5 with at least one non-zero,
    the reference's five quantiles and 0, 1, 0.25."""
    rng = np.random.default_rng({'levels': 1, 'normal': 2}[kind])
    levels = np.array([-2.5, -1e-3, 0.0, 0.7, 3.25e4])
    for case in range(200):
        n = int(rng.integers(1, 41))
        if kind == 'levels':
            values = levels[rng.integers(0, 5, (n, 3))]
        else:
            values = rng.normal(0.0, 10.0**rng.uniform(-3, 3), (n, 3))
        counts = rng.integers(0, 6, n)
        if not counts.any():
            counts[rng.integers(0, n)] = 1 + case % 5
        want = np.percentile(values[expansion(counts)], 100 * np.array(Q_ALL), axis=0)
        got = post.weighted_quantiles_host(values, counts, Q_ALL)
        assert got.shape == (len(Q_ALL), 3)
        assert np.array_equal(got, want), (kind, case, n)


def test_single_element_cases():
    """N = 1 (one sample visited once, beside samples that do not exist) and n = 1 with a count
    of 7: every quantile is that element."""
    values = np.array([[3.5, -1.0], [7.25, 2.0], [-4.0, 9.0]])
    got = post.weighted_quantiles_host(values, [0, 1, 0], Q_ALL)
    assert np.array_equal(got, np.tile(values[1], (len(Q_ALL), 1)))
    assert np.array_equal(got, np.percentile(values[[1]], 100 * np.array(Q_ALL), axis=0))
    one = post.weighted_quantiles_host(np.array([1.75]), [7], Q_ALL)
    assert one.shape == (len(Q_ALL),) and np.all(one == 1.75)
    assert np.array_equal(one, np.percentile(np.full(7, 1.75), 100 * np.array(Q_ALL)))


def test_large_counts_need_no_expansion():
    """Counts near 1e10 each (N past 2^31): the ranks stay exact integers, and scaling every
    count of a small case by the same factor moves no quantile by more than one sample."""
    rng = np.random.default_rng(3)
    values = rng.normal(size=(9, 2))
    counts = 10**10 + rng.integers(0, 1000, 9)
    lo, hi, gamma = post.quantile_ranks(counts.sum(), Q_ALL)
    assert lo.dtype == np.int64 and lo.max() == counts.sum() - 1 > 2**31
    assert np.all((hi - lo >= 0) & (hi - lo <= 1)) and np.all((gamma >= 0) & (gamma < 1))
    got = post.weighted_quantiles_host(values, counts, [0.0, 0.5, 1.0])
    assert np.array_equal(got[0], values.min(axis=0)) and np.array_equal(got[2], values.max(axis=0))
    assert np.array_equal(got[1], np.median(values, axis=0))      # (9 samples of near-equal weight)


def test_unique_samples():
    """A small chain with repeated first-column values whose later columns differ: the reference
    deduplicates on the first column only."""
    chain = np.array([[0.3, 1.0], [0.1, 2.0], [0.3, 9.0], [0.2, 4.0], [0.1, 5.0], [0.3, 6.0]])
    u_index, counts, inverse = post.unique_samples(chain)
    u, want_index, want_inverse = np.unique(chain[:, 0], return_index=True, return_inverse=True)
    assert np.array_equal(u_index, want_index) and np.array_equal(inverse, want_inverse)
    assert np.array_equal(counts, np.bincount(want_inverse)) and list(counts) == [2, 1, 3]
    assert np.array_equal(chain[u_index][inverse][:, 0], chain[:, 0])
    assert list(u_index) == [1, 3, 0]                     # (the first visit of each value)
    with pytest.raises(ValueError):
        post.unique_samples(np.zeros(4))


def test_argument_checks():
    with pytest.raises(ValueError):
        post.quantile_ranks(5, [0.5, 1.5])
    with pytest.raises(ValueError):
        post.quantile_ranks(0, [0.5])
    with pytest.raises(ValueError, match='every count is zero'):
        post.weighted_quantiles_host(np.ones((3, 2)), [0, 0, 0], [0.5])
    with pytest.raises(ValueError):
        post.weighted_quantiles_host(np.ones((3, 2)), [1, 1], [0.5])
