"""The prior transform on the host (Retrieval.prior_transform_host) against the exact inverse CDF
of the two-sided Gaussian prior (tests/golden/prior_transform.npz, made by
make_golden_prior_transform.py with mpmath at 50 digits), and what follows from the mathematics
alone: reflection for a symmetric prior, monotonicity across the split, the end values.  No GPU.

The bound is test_gpu_retrieval's TRANSFORM_UNITS = 8 units of eps (|prior| + s (1 + |z|)), in
both branches.  Until the upper branch passed the tail mass itself to the inverse normal CDF
(prior - up ndtri(x) instead of prior + up ndtri(1 - x)), test_host_against_the_exact_inverse_cdf
failed above prior from three sigma upward: 15 units at an upper-tail mass of 1e-3 of
(0.25, 3.0, 0.3), 114 at 1e-4, 4.7e7 at 1e-10, 4.9e12 at u = 1 - 1e-16, 1.8e9 at 1e-14 of
(-1400, 0.2, 2.0); below prior its worst was 1.2 units then as now."""
import importlib.util
import os

import numpy as np
import pytest

import prior_transform_cases as pc
from prior_transform_cases import TRANSFORM_UNITS

EPS = pc.EPS


@pytest.fixture(scope='module')
def ret():
    return pc.golden_retrieval()


def test_golden_regenerates():
    """The committed fixture is what its maker writes (where mpmath imports)."""
    pytest.importorskip('mpmath')
    path = os.path.join(os.path.dirname(pc.GOLDEN), 'make_golden_prior_transform.py')
    spec = importlib.util.spec_from_file_location('make_golden_prior_transform', path)
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fresh, g = maker.build(), pc.golden()
    assert os.path.getsize(pc.GOLDEN) < 200 * 1000
    assert set(fresh) == set(g)
    for name, a in fresh.items():
        a = np.asarray(a)
        assert a.dtype == g[name].dtype and a.shape == g[name].shape, name
        same = a == g[name] if a.dtype.kind == 'U' else \
            a.view(np.uint8) == g[name].view(np.uint8)
        assert np.all(same), name


def test_golden_is_what_its_docstring_says():
    """The cube's shape and range, and the identities that need no solver: the split point maps
    to prior, a symmetric prior at u = 1/2 too, and theta is monotone in u in every column."""
    g = pc.golden()
    u, theta, z, branch = g['u'], g['theta'], g['z'], g['branch']
    prior, lo, up = g['params'].T
    assert u.shape == (1000, 7) and np.all((u > 0) & (u < 1)) and np.all(np.isfinite(theta))
    assert u.min() <= 1e-300 and u.max() == 1.0 - 2.0**-53
    assert z.min() < -37.0 and z.max() > 8.2
    assert np.all((z <= 0) == (branch == 0) | (z == 0)) and np.all((theta >= prior) | (branch == 0))
    names = list(g['group_names'])
    assert [int(np.sum(g['group'] == k)) for k in range(len(names))] == \
        [6, 3, 15, 300, 2, 106, 60, 60, 60, 388]
    half = np.flatnonzero(np.all(u == 0.5, axis=1))[0]
    assert theta[half, 0] == prior[0] and z[half, 0] == 0.0
    # (fl(lo / (lo + up)) is within half an ulp of the split: theta is within a unit of prior)
    split = np.flatnonzero(g['group'] == names.index('split'))[0]
    assert np.all(np.abs(theta[split] - prior) <= EPS * (np.abs(prior) + np.maximum(lo, up)))
    for c in range(7):
        order = np.argsort(u[:, c], kind='stable')
        exact = np.longdouble(theta[order, c]) + np.longdouble(g['resid'][order, c])
        assert np.all(np.diff(theta[order, c]) >= 0) and np.all(np.diff(exact) >= 0), c
    # every upper-tail mass of the rule is there: q = 1e-k is Q(z) of its row, to the rounding of
    # u = 1 - q M at 1 (half an ulp of 1 against a mass of q M)
    from scipy.special import ndtr
    rows = np.flatnonzero(g['group'] == names.index('upper'))
    for k, r in enumerate(rows, start=1):
        q, mass = 10.0**-k, 2 * up / (lo + up)
        ok = u[r] < 1.0 - 2.0**-53
        assert np.all(np.abs(ndtr(-z[r, ok]) / q - 1.0) <= 1e-12 + EPS / (q * mass[ok])), k
    rows = np.flatnonzero(g['group'] == names.index('lower'))
    np.testing.assert_allclose(ndtr(z[rows[2]]), 1e-3, rtol=1e-12)
    np.testing.assert_allclose(ndtr(z[rows[299]]), 1e-300, rtol=1e-12)


def test_host_against_the_exact_inverse_cdf(ret):
    """prior_transform_host within TRANSFORM_UNITS of the exact value, below and above prior."""
    g = pc.golden()
    got = ret.prior_transform_host(g['u'])
    ratio = pc.units(got)
    below, above = pc.worst_by_branch(ratio, 'prior_transform_host against the exact inverse CDF')
    # the rows of the upper tail one by one, for the record
    names = list(g['group_names'])
    for r in np.flatnonzero(g['group'] == names.index('upper')):
        print('upper-tail mass 1e-%02d: units per column %s' % (
            r - np.flatnonzero(g['group'] == names.index('upper'))[0] + 1,
            ' '.join(f'{v:9.3g}' for v in ratio[r])))
    assert below <= TRANSFORM_UNITS, 'below prior'
    assert above <= TRANSFORM_UNITS, 'above prior'
    assert np.all(ratio <= TRANSFORM_UNITS)


def test_the_side_of_the_split_is_decided_exactly():
    """below_split(u, lo, up) is u (lo + up) < lo in rational arithmetic: at the fixture's split
    rows, 40 ulps to either side of fl(lo / (lo + up)) for the fixture's columns and for 200
    random widths over six decades, at the ends, and for NaN.  (fl(lo / (lo + up)) itself is on
    the wrong side for some of them, which is why the statement does not compare with it.)"""
    from fractions import Fraction
    from pyratbay_amd.retrieval import below_split
    rng = np.random.default_rng(11)
    g = pc.golden()
    lo = np.concatenate([g['params'][:, 1], 10.0**rng.uniform(-3, 3, 200)])
    up = np.concatenate([g['params'][:, 2], 10.0**rng.uniform(-3, 3, 200)])
    split = lo / (lo + up)
    chain, v, w = [split], split, split
    for _ in range(40):
        v, w = np.nextafter(v, 0.0), np.nextafter(w, 1.0)
        chain += [v, w]
    u = np.array(chain + [np.full(len(lo), x) for x in (0.0, 5e-324, 1e-300, 0.5, 1 - 2.0**-53,
                                                         1.0)])
    got = below_split(u, lo, up)
    want = np.array([[Fraction(x) * (Fraction(a) + Fraction(b)) < Fraction(a)
                      for x, a, b in zip(row, lo, up)] for row in u])
    assert np.array_equal(got, want)
    naive = u < split
    print(f'u < fl(lo / (lo + up)) is on the wrong side for {int(np.sum(naive != want))} of '
          f'{want.size} elements')
    assert np.any(naive != want)
    assert not np.any(below_split(np.full(len(lo), np.nan), lo, up))
    # the fixture's own branch is this decision
    assert np.array_equal(below_split(g['u'], *g['params'][:, 1:].T), g['branch'] == 0)


def test_mirror_for_a_symmetric_prior():
    """lo == up and the exact pairs (2^-k, 1 - 2^-k): the two results reflect about prior, within
    the sum of their two bounds (z from the lower statement's own argument, ndtri(2^-k))."""
    from scipy.special import ndtri
    prior = np.array([3.0, -1400.0, 0.0, 1.0e6, 1.0e-3])
    s = np.array([0.5, 2.0, 1.0e-3, 1.0e-6, 0.05])
    sym = pc.retrieval(prior, s, s)
    k = np.arange(1, 54)
    low, high = 2.0**-k, 1.0 - 2.0**-k
    assert np.all(1.0 - high == low)
    a = sym.prior_transform_host(np.tile(low[:, None], (1, 5)))
    b = sym.prior_transform_host(np.tile(high[:, None], (1, 5)))
    z = np.abs(ndtri(low))[:, None]
    bound = TRANSFORM_UNITS * EPS * (np.abs(prior) + s * (1.0 + z))
    assert np.all(a <= prior) and np.all(b >= prior) and np.all(np.isfinite(a + b))
    assert np.all(np.abs((prior - a) - (b - prior)) <= 2.0 * bound)
    assert np.array_equal(a[0], prior) and np.array_equal(b[0], prior)       # u = 1/2
    assert a[-1, 2] < -8.2e-3 and b[-1, 2] > 8.2e-3                          # 2^-53: 8.2 sigma


def test_monotone_in_u(ret):
    """Every column is non-decreasing in sorted u: the fixture's u, and 64 neighbours of the split
    point on either side, ulp by ulp, so that the change of branch is inside the run."""
    g = pc.golden()
    prior, lo, up = g['params'].T
    split = lo / (lo + up)
    chain = [split]
    for way in (0.0, 1.0):
        v = split
        for _ in range(64):
            v = np.nextafter(v, way)
            chain.append(v)
    u = np.sort(np.concatenate([g['u'], np.array(chain)]), axis=0)
    theta = ret.prior_transform_host(u)
    assert np.all(np.isfinite(theta))
    steps = np.diff(theta, axis=0)
    for c in range(7):
        worst = int(np.argmin(steps[:, c]))
        assert steps[worst, c] >= 0, (c, u[worst:worst + 2, c], theta[worst:worst + 2, c])
    # and it is not flat: from 37 sigma below to 7 sigma above (u = 1 - 2^-53 is an upper-tail mass
    # of 2^-53 (lo + up) / (2 up): 7.4 sigma where up is a thousandth of lo)
    assert np.all(theta[0] < prior - 37 * lo) and np.all(theta[-1] > prior + 7 * up)


def test_end_values(ret):
    """u = 0 gives -inf, u = 1 gives +inf, NaN gives NaN, in whichever column; inside_host is
    False for such a walker."""
    for bad, want in ((0.0, -np.inf), (1.0, np.inf), (np.nan, np.nan)):
        for c in range(7):
            cube = np.full((2, 7), 0.25)
            cube[1, c] = bad
            theta = ret.prior_transform_host(cube)
            assert np.array_equal(theta[1, c:c + 1], [want], equal_nan=True), (bad, c)
            assert np.all(np.isfinite(theta[0])) and np.all(np.isfinite(np.delete(theta[1], c)))
            assert list(ret.inside_host(theta)) == [True, False]
            assert ret.log_prior_host(theta)[1] == -np.inf


def test_prior_widths_refused_at_construction():
    """A free parameter whose priorlow or priorup is negative or not finite, or with exactly one
    of the two zero (a half-open prior), is refused by name; fixed parameters are not looked at;
    a uniform parameter with an infinite bound is still refused by the transform only."""
    prior, lo, up = np.zeros(4), np.array([0.5, 0.0, 1.0, 2.0]), np.array([0.5, 0.0, 3.0, 2.0])
    pc.retrieval(prior, lo, up, pmin=np.full(4, -9.0), pmax=np.full(4, 9.0))
    width = r"retrieval_params: free parameters \['{}'\] have a negative or non-finite priorlow or priorup"
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        for side, name in ((lo, 'a0'), (up, 'a2')):
            a = side.copy()
            a[int(name[1])] = bad
            with pytest.raises(ValueError, match=width.format(name)):
                pc.retrieval(prior, *((a, up) if side is lo else (lo, a)))
    half = r"retrieval_params: free parameters \[{}\] have exactly one of priorlow and priorup equal to zero"
    with pytest.raises(ValueError, match=half.format("'a1'")):
        pc.retrieval(prior, np.array([0.5, 1.0, 1.0, 2.0]), up)
    with pytest.raises(ValueError, match=half.format("'a0', 'a3'")):
        pc.retrieval(prior, lo, np.array([0.0, 0.0, 3.0, 0.0]))
    # a line that is not free may hold anything
    from pyratbay_amd import retrieval as pr
    ok = pc.retrieval(prior, lo, up, pmin=np.full(4, -9.0), pmax=np.full(4, 9.0))
    cols = [ok.pnames, ok.params, ok.pmin, ok.pmax, np.array([1.0, 1.0, 0.0, 1.0]), ok.prior,
            np.array([0.5, 0.0, 0.0, 2.0]), np.array([0.5, 0.0, -3.0, 2.0])]
    fixed = pr.Retrieval(ok.model, ok.atmosphere, ok.bands, ok.observation, cols)
    assert fixed.nfree == 3
    # the existing refusal: a uniform parameter with an infinite bound, by the transform only
    open_ = pc.retrieval(prior, lo, up)
    assert open_.inside_host(np.zeros((1, 4)))[0]
    with pytest.raises(ValueError, match=r"prior_transform: uniform parameters \['a1'\] have an "
                                         'infinite bound'):
        open_.prior_transform_host(np.full((1, 4), 0.5))
