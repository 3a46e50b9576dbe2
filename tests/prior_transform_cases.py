"""What test_prior_transform_cpu.py and test_gpu_prior_transform_boundary.py share: the exact
fixture tests/golden/prior_transform.npz (make_golden_prior_transform.py: the inverse CDF of the
two-sided Gaussian prior at 50 digits), a Retrieval on stand-in objects over given prior columns,
the error of a transform in the project's units, and the wide column layouts of the GPU shapes.

Units: one unit is eps (|prior| + s (1 + |z|)) with s and z of the EXACT solution (the fixture's
branch and z): the rounding of prior, of s z and of their sum.  The error is taken against
theta + resid, the exact value to about 32 digits, not against the rounded double."""
import os
import types

import numpy as np

from test_gpu_retrieval import TRANSFORM_UNITS                      # noqa: F401  (the bound)

EPS = np.finfo(float).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prior_transform.npz')
BRANCHES = ('below prior', 'above prior')

_LOADED = {}


def golden():
    """The fixture's arrays, loaded once and left unchanged (read-only)."""
    if not _LOADED:
        with np.load(GOLDEN) as f:
            for k in f.files:
                _LOADED[k] = f[k]
                _LOADED[k].flags.writeable = False
    return _LOADED


def retrieval(prior, lo, up, pmin=None, pmax=None):
    """A Retrieval whose free parameters are the given columns, on stand-in objects (Retrieval
    reads only attributes).  pmin / pmax default to -inf / +inf."""
    from pyratbay_amd import retrieval as pr
    prior, lo, up = (np.asarray(a, np.float64) for a in (prior, lo, up))
    n = len(prior)
    names = [f'a{k}' for k in range(n)]
    atm = types.SimpleNamespace(free=names, npar=n, base_params=None,
                                par_scalar={'rplanet': -1, 'log_refpressure': -1, 'mplanet': -1})
    obs = types.SimpleNamespace(offset_models=[], err_models=[], noff=0, nerr=0,
                                err_defaults=np.zeros(0), nbands=1)
    model = types.SimpleNamespace(rt_path='emission', continuum=None, irradiation=None)
    bands = types.SimpleNamespace(star_grid=None, nbands=1)
    pmin = np.full(n, -np.inf) if pmin is None else np.asarray(pmin, np.float64)
    pmax = np.full(n, np.inf) if pmax is None else np.asarray(pmax, np.float64)
    finite = np.isfinite(pmin) & np.isfinite(pmax)
    value = np.where(finite, 0.5 * (np.where(finite, pmin, 0.0) + np.where(finite, pmax, 0.0)),
                     prior)
    return pr.Retrieval(model, atm, bands, obs,
                        (names, value, pmin, pmax, np.ones(n), prior, lo, up))


def golden_retrieval():
    prior, lo, up = golden()['params'].T
    return retrieval(prior, lo, up)


def units(got, cols=None, rows=None):
    """|got - exact| in units of eps (|prior| + s (1 + |z|)) for got[len(rows), len(cols)], the
    transform of the fixture's u[rows][:, cols] (default: all) under the fixture's columns."""
    g = golden()
    cols = np.arange(g['u'].shape[1]) if cols is None else np.asarray(cols)
    rows = np.arange(g['u'].shape[0]) if rows is None else np.asarray(rows)
    pick = np.ix_(rows, cols)
    prior, lo, up = g['params'][cols].T
    s = np.where(g['branch'][pick] == 0, lo, up)
    unit = EPS * (np.abs(prior) + s * (1.0 + np.abs(g['z'][pick])))
    LD = np.longdouble
    with np.errstate(all='ignore'):
        err = np.abs((LD(got) - LD(g['theta'][pick])) - LD(g['resid'][pick]))
        ratio = np.asarray(err / LD(unit), np.float64)
    return np.where(np.isnan(ratio), np.inf, ratio)              # (a NaN result is no result)


def worst_by_branch(ratio, what, cols=None, rows=None):
    """Prints the worst ratio of either branch and where (u, column parameters, z); -> the two
    worst ratios."""
    g = golden()
    cols = np.arange(g['u'].shape[1]) if cols is None else np.asarray(cols)
    rows = np.arange(g['u'].shape[0]) if rows is None else np.asarray(rows)
    branch = g['branch'][np.ix_(rows, cols)]
    worst = []
    for b, name in enumerate(BRANCHES):
        if not np.any(branch == b):
            worst.append(0.0)
            print(f'{what}, {name}: no element')
            continue
        masked = np.where(branch == b, ratio, -1.0)
        i, j = np.unravel_index(np.argmax(masked), masked.shape)
        r, c = rows[i], cols[j]
        worst.append(float(masked[i, j]))
        print(f'{what}, {name}: worst {masked[i, j]:.3f} units at u = {g["u"][r, c]!r} '
              f'(1 - u = {1.0 - g["u"][r, c]:.3e}), (prior, lo, up) = '
              f'{tuple(float(v) for v in g["params"][c])}, z = {g["z"][r, c]:.3f}, row {r} '
              f'({g["group_names"][g["group"][r]]})')
    return worst


# the wide layouts of the GPU shapes: which fixture column (or -1: uniform) free parameter f reads
PERMUTATION = (4, 1, 6, 0, 3, 5, 2)
FEW = (2, 4, 5, 1, 3, 6, 0)
UNIFORM_EVERY = 5


def layout(nfree):
    """source[nfree]: nfree == 7: the fixture's columns as they are.  Fewer: the first nfree of
    FEW (an asymmetric column first).  Beyond: every fifth parameter (f % 5 == 2) is uniform
    (-1), the others walk the seven columns cyclically under PERMUTATION."""
    if nfree == 7:
        return np.arange(7)
    if nfree < 7:
        return np.array(FEW[:nfree])
    source, k = [], 0
    for f in range(nfree):
        if f % UNIFORM_EVERY == 2:
            source.append(-1)
        else:
            source.append(PERMUTATION[k % 7])
            k += 1
    return np.array(source)


def columns(source):
    """(pmin, pmax, prior, lo, up)[nfree] of a layout; the uniform parameters get distinct finite
    bounds, and prior = lo = up = 0."""
    g = golden()
    source = np.asarray(source)
    gauss = source >= 0
    par = g['params'][np.where(gauss, source, 0)]
    prior, lo, up = (np.where(gauss, par[:, k], 0.0) for k in range(3))
    f = np.arange(len(source), dtype=np.float64)
    pmin = np.where(gauss, -np.inf, -2.0 - 0.37 * f)
    pmax = np.where(gauss, np.inf, 7.0 + 1.3 * f)
    return pmin, pmax, prior, lo, up


def cube_for(nw, source, first=0):
    """u[nw, nfree] and the fixture rows behind it: walker w reads row (first + w) % 1000 of the
    fixture in the column its parameter names; a uniform parameter reads column f % 7."""
    g = golden()
    source = np.asarray(source)
    rows = (first + np.arange(nw)) % g['u'].shape[0]
    read = np.where(source >= 0, source, np.arange(len(source)) % g['u'].shape[1])
    return np.ascontiguousarray(g['u'][np.ix_(rows, read)]), rows
