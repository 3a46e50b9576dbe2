"""The prior transform at the kernel boundary (csrc/pb_retrieval.hip: pb_prior_transform), driven
through the C ABI on dirty memory, against the exact inverse CDF of the two-sided Gaussian prior
(tests/golden/prior_transform.npz: mpmath at 50 digits, prior_transform_cases.py).

Every launch: `theta` is NaN before the call and sits between two guard blocks of 3 NaN that must
still be NaN afterwards; the six inputs are uploaded from copies and must read back unchanged; one
synchronize before the result is read.  Every Gaussian element is compared with the fixture's
theta + resid (the exact value to about 32 digits) in units of eps (|prior| + s (1 + |z|)), s and z
of the exact solution, against test_gpu_retrieval's TRANSFORM_UNITS = 8; every uniform element
must have the bits of pmin + u (pmax - pmin).  Each check prints its worst ratio below and above
prior and where, then asserts.

Which test launches which situation:

  one element; 255, 256, 257 elements (one block and one        test_shapes (nfree = 1)
    element more); the i >= total guard
  nfree = 128 (divides the block), 65 (does not), several       test_shapes (2 x 128, 3 x 128,
    blocks, i % nfree across block seams                          5 x 65, 1000 x 7)
  uniform parameters beside Gaussian ones, the seven columns    test_shapes (nfree = 65, 128)
    under a permutation
  the whole fixture, 28 blocks; the same rows in pieces of 1,    test_shapes[1000-7],
    37 and 256 walkers: equal bits                                 test_pieces_have_the_bits...
  two launches: equal bits                                       test_shapes
  the split point and the ulp on either side of it, with         test_shapes (rows 6 - 8 of the
    lo = 1000 up and up = 1000 lo                                  fixture)
  u = 0, 1, NaN -> -inf, +inf, NaN; pb_retrieval_map then says   test_end_values
    inside == 0 and log-prior -inf
  nwalkers = 0, nfree = 0, each pointer NULL                     test_noops_and_refusals
"""
import numpy as np
import pytest

import prior_transform_cases as pc
from prior_transform_cases import TRANSFORM_UNITS
from test_gpu_hires_boundary import Dirty, bits, ptr, stream, upload

pytestmark = pytest.mark.gpu

TRANSFORM = 'pb_prior_transform'
INPUTS = ('cube', 'pmin', 'pmax', 'prior', 'priorlow', 'priorup')


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def transform(eng, cube_h, cols_h, into=None, **over):
    """pb_prior_transform on host arrays -> host theta[nw, nfree] (with the Dirty `into` given:
    of that buffer).  cols_h: (pmin, pmax, prior, priorlow, priorup); over: arguments replaced by
    name (a pointer by None, a count by another)."""
    import torch
    from pyratbay_amd import _capi
    nw, nfree = cube_h.shape
    kept = dict(zip(INPUTS, [np.array(a, np.float64) for a in (cube_h, *cols_h)]))
    device = {name: upload(eng, a) for name, a in kept.items()}
    out = Dirty(nw, nfree) if into is None else into
    a = dict(theta=out.ptr, nfree=nfree, nwalkers=nw, **{n: ptr(t) for n, t in device.items()})
    assert set(over) <= set(a)
    a.update(over)
    try:
        rc = _capi.call(TRANSFORM, a['theta'], a['cube'], a['pmin'], a['pmax'], a['prior'],
                        a['priorlow'], a['priorup'], a['nfree'], a['nwalkers'], stream())
    finally:
        torch.cuda.synchronize()
    assert rc == _capi.PB_OK and out.guards_intact()
    for name, t in device.items():
        assert np.array_equal(bits(t.cpu().numpy()), bits(kept[name])), name
    return out.body.cpu().numpy()


def check(got, cube, source, cols, rows, what):
    """Uniform parameters: the bits of the two operations; Gaussian parameters: within
    TRANSFORM_UNITS of the exact value, below and above prior.  -> the two worst ratios."""
    pmin, pmax = cols[:2]
    gauss = source >= 0
    assert got.shape == cube.shape and not np.any(np.isnan(got)), what
    if np.any(~gauss):
        flat = pmin[~gauss] + cube[:, ~gauss] * (pmax[~gauss] - pmin[~gauss])
        assert np.array_equal(bits(got[:, ~gauss]), bits(flat)), what
    assert np.all(np.isfinite(got[:, gauss])), what
    ratio = pc.units(got[:, gauss], cols=source[gauss], rows=rows)
    worst = pc.worst_by_branch(ratio, what, cols=source[gauss], rows=rows)
    assert max(worst) <= TRANSFORM_UNITS, (what, worst)
    return worst


def first_rows(nw):
    """Where in the fixture a launch of nw walkers starts: the whole cube from row 0; a launch of
    a few walkers once at each of: the existing test's rows, the split rows, upper-tail masses
    1e-3, 1e-10 and 1e-15, lower-tail masses 1e-1, 1e-150 and 1e-300, the ends, the ladder."""
    return (0,) if nw >= 255 else (0, 4, 6, 11, 18, 23, 24, 173, 323, 324, 400, 612, 998)


SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (2, 128), (3, 128), (5, 65), (1000, 7)]


@pytest.mark.parametrize('nw,nfree', SHAPES)
def test_shapes(eng, nw, nfree):
    source = pc.layout(nfree)
    cols = pc.columns(source)
    assert (nfree <= 7) == bool(np.all(source >= 0)) and len(source) == nfree
    if nfree > 7:
        assert set(source[source >= 0]) == set(range(7)) and np.sum(source < 0) >= nfree // 5
    for first in first_rows(nw):
        cube, rows = pc.cube_for(nw, source, first)
        got = transform(eng, cube, cols)
        check(got, cube, source, cols, rows, f'{nw} x {nfree} from row {first}')
        assert np.array_equal(bits(transform(eng, cube, cols)), bits(got))


def test_pieces_have_the_bits_of_the_whole(eng):
    """The fixture's 1000 x 7 in one launch (28 blocks) and the same rows launched in pieces of
    1, 37 and 256 walkers, in turn, until the cube is covered: the same bits, whichever block,
    lane and i % nfree an element went through."""
    source = pc.layout(7)
    cols = pc.columns(source)
    assert np.array_equal(source, np.arange(7))
    cube, rows = pc.cube_for(1000, source)
    assert np.array_equal(bits(cube), bits(pc.golden()['u']))
    whole = transform(eng, cube, cols)
    check(whole, cube, source, cols, rows, 'the fixture in one launch')
    start, sizes, count = 0, (1, 37, 256), 0
    while start < 1000:
        n = min(sizes[count % 3], 1000 - start)
        piece = transform(eng, np.ascontiguousarray(cube[start:start + n]), cols)
        assert np.array_equal(bits(piece), bits(whole[start:start + n])), (start, n)
        start, count = start + n, count + 1
    assert count == 12                       # (three rounds of 1 + 37 + 256, then 1, 37 and 80)


def test_end_values(eng):
    """u = 0, 1 and NaN in each column in turn give -inf, +inf and NaN there and finite values
    elsewhere; pb_retrieval_map then reports inside == 0 and a log-prior of -inf for that walker,
    and inside == 1 with the host's log-prior for the walker without such a value."""
    from test_gpu_retrieval import run_map
    ret = pc.golden_retrieval()
    source = pc.layout(7)
    cols = pc.columns(source)
    ends = ((0.0, -np.inf), (1.0, np.inf), (np.nan, np.nan))
    cube = np.full((1 + 3 * 7, 7), 0.25)
    want = np.zeros(cube.shape)
    for k, (bad, value) in enumerate(ends):
        for c in range(7):
            cube[1 + 7 * k + c, c], want[1 + 7 * k + c, c] = bad, value
    theta = transform(eng, cube, cols)
    special = want != 0
    assert np.array_equal(theta[special], want[special], equal_nan=True)
    assert np.all(np.isfinite(theta[~special]))
    assert np.array_equal(bits(np.where(special, 0.0, theta)),
                          bits(np.where(special, 0.0, np.tile(theta[0], (22, 1)))))
    _, log_prior, inside = run_map(eng, ret, theta)
    assert list(inside) == [1] + [0] * 21
    assert np.all(log_prior[1:] == -np.inf) and np.isfinite(log_prior[0])
    assert np.array_equal(ret.inside_host(theta), inside.astype(bool))
    host = ret.log_prior_host(theta)
    assert np.all(host[1:] == -np.inf) and abs(log_prior[0] - host[0]) <= 9 * pc.EPS * abs(host[0])


def test_noops_and_refusals(eng):
    """nwalkers = 0 returns PB_OK and writes nothing (with every pointer NULL too); nfree = 0, a
    negative count and each of the seven pointers NULL raise PbError with the entry point's own
    message; `theta` keeps its NaN through all of it; then the same arguments, unmodified, run."""
    from pyratbay_amd import _capi
    source = pc.layout(65)
    cols = pc.columns(source)
    cube, rows = pc.cube_for(5, source, 6)
    out = Dirty(5, 65)
    transform(eng, cube, cols, into=out, nwalkers=0)
    transform(eng, cube, cols, into=out, nwalkers=0, theta=None, **{n: None for n in INPUTS})
    assert out.untouched()
    for bad in (dict(nfree=0), dict(nfree=-1), dict(nwalkers=-1), dict(nfree=0, nwalkers=0)):
        with pytest.raises(_capi.PbError, match=rf'\): {TRANSFORM}: bad shape'):
            transform(eng, cube, cols, into=out, **bad)
        assert out.untouched(), bad
    for name in ('theta',) + INPUTS:
        with pytest.raises(_capi.PbError, match=rf'\): {TRANSFORM}: null pointer'):
            transform(eng, cube, cols, into=out, **{name: None})
        assert out.untouched(), name
    got = transform(eng, cube, cols, into=out)
    check(got, cube, source, cols, rows, 'after the refusals')
