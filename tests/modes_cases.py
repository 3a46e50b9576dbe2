"""Cases the CPU and GPU tests of the mode decomposition share (pyratbay_amd/modes.py,
csrc/pb_modes.hip): a two-mode target whose evidence and local evidences are known in closed form,
with its committed bounds, next to nested_cases' Gaussian; hand-made rows for link_host and
points for assign_host."""
import functools
import types

import numpy as np

import nested_cases as nc

# -------------------------------------------------------------------------------------------------
# the two-mode target: 3 parameters, a uniform prior over the box +-10 (sigma = 1), and
#   L = w exp(-|theta - 5|^2 / 2) + (1 - w) s^-3 exp(-|theta + 5|^2 / (2 s^2))
# so that the integral of L is (2 pi)^1.5 and the modes carry w and 1 - w of it
# -------------------------------------------------------------------------------------------------
NFREE = 3
LN_Z = float(np.log((2.0 * np.pi)**1.5 / 20.0**3))
FORMS = {'equal': (0.5, 1.0), 'wide': (0.25, 2.0)}
NLIVE, BATCH, NSTEPS, DLOGZ, MAX_ITER = nc.NLIVE, nc.BATCH, nc.NSTEPS, nc.DLOGZ, nc.MAX_ITER
SEEDS = nc.SEEDS


def local_ln_z(form):
    """(ln Z of the mode at +5, ln Z of the mode at -5)."""
    w, _ = FORMS[form]
    return LN_Z + float(np.log(w)), LN_Z + float(np.log(1.0 - w))


# The worst values of run_host + modes_host over seeds 0 - 19 at nested_cases' settings
# (profiles/modes.md has the table), per form: |ln Z_m - closed form| over both modes, and the
# posterior mass assigned to the mode across theta_0 = 0.  The committed bound on the local
# evidences is twice the worst value, nested_cases' rule and for its reason: 20 seeds sample the
# tail thinly.  Conditions, not measurements: the bound may not exceed 0.5, the misassigned mass
# is at most 1e-2, and the mean of each local evidence over the 20 seeds lies within
# 3 std / sqrt(20) of its closed form.
WORST_LOCAL = {'equal': 0.18671, 'wide': 0.19101}
WORST_MASS = {'equal': 6.404e-07, 'wide': 5.625e-03}
BOUND_LOCAL = {form: 2 * worst for form, worst in WORST_LOCAL.items()}
BOUND_MASS = 1e-2


def prior_transform_host(cube):
    return 20.0 * np.asarray(cube) - 10.0


def log_like_host(theta, form):
    w, s = FORMS[form]
    theta = np.asarray(theta)
    r1 = np.sum((theta - 5.0)**2, axis=1)
    r2 = np.sum((theta + 5.0)**2, axis=1)
    return np.logaddexp(np.log(w) - 0.5 * r1,
                        (np.log(1.0 - w) - 3.0 * np.log(s)) - r2 / (2.0 * s * s))


def target_torch(form):
    """(log_like, prior_transform): the same operations as torch callables on device tensors."""
    import torch
    w, s = FORMS[form]

    def prior_transform(cube):
        return 20.0 * cube - 10.0

    def log_like(theta):
        r1 = torch.sum((theta - 5.0)**2, dim=1)
        r2 = torch.sum((theta + 5.0)**2, dim=1)
        return torch.logaddexp(float(np.log(w)) - 0.5 * r1,
                               float(np.log(1.0 - w) - 3.0 * np.log(s)) - r2 / (2.0 * s * s))
    return log_like, prior_transform


@functools.lru_cache(maxsize=None)
def run_host(form, seed):
    """run_host on the target at nested_cases' settings, and what modes_host makes of it
    (computed once per session; do not modify the result) -> a namespace of st, fin, cube,
    theta and md."""
    from pyratbay_amd import modes, nested
    st = nested.run_host(functools.partial(log_like_host, form=form), prior_transform_host,
                         NLIVE, BATCH, NSTEPS, MAX_ITER, seed=seed, nfree=NFREE, dlogz=DLOGZ)
    fin = nested.finish_host(st.dead_logl, st.dead_logw, st.live_logl, st.ln_x)
    cube = np.concatenate((st.dead_u, st.live_u))
    md = modes.modes_host(cube, fin, seed)
    return types.SimpleNamespace(st=st, fin=fin, cube=cube, theta=prior_transform_host(cube),
                                 md=md)


def weighted_median(x, weight):
    order = np.argsort(x, kind='stable')
    cdf = np.cumsum(weight[order])
    return x[order][np.searchsorted(cdf, 0.5 * cdf[-1])]


def mode_figures(form, theta, logw, ln_z, md):
    """Of one decomposition into two modes: (err[2], mass) -- ln Z_m minus its closed form for the
    mode at +5 and the mode at -5, told apart by the sign of the weighted median of theta_0, and
    the posterior mass of the points that lie across theta_0 = 0 from their mode's centre."""
    p = np.exp(logw - ln_z)
    truth = local_ln_z(form)
    err, mass = [np.nan, np.nan], 0.0
    for c in range(md.nmodes):
        member = md.mode == c
        sign = np.sign(weighted_median(theta[member, 0], p[member]))
        err[0 if sign > 0 else 1] = md.ln_z[c] - truth[0 if sign > 0 else 1]
        mass += float(np.sum(p[member & (np.sign(theta[:, 0]) != sign)]))
    return np.array(err), mass


# -------------------------------------------------------------------------------------------------
# hand-made rows for link_host
# -------------------------------------------------------------------------------------------------
LINK_NS = (2, 3, 9, 64, 65, 300)
LINK_NFREES = (1, 3, 16, 128)
KINDS = ('default', 'blobs', 'chain', 'equal', 'small', 'many', 'repeated', 'lattice')


def _blobs(rng, sizes, centres, half, nfree):
    return np.concatenate([c + rng.uniform(-half, half, (m, nfree))
                           for m, c in zip(sizes, centres)])


def link_case(kind, n, nfree):
    """(R[n, nfree], keywords of link_host, the number of modes to expect or None), or None where
    the kind has no case of n rows.  Every row lies inside the unit cube.
      default   two blobs under the default keywords (n <= knn: k = n - 1 and one component);
      blobs     two blobs of 2/3 and 1/3 of the rows;
      chain     two blobs joined by a chain of single points: single linkage merges them;
      equal     components of equal size (lines of evenly spaced rows), the rows shuffled: ties go to the lower row index;
      small     a component below the default min_mode: its rows are loose;
      many      nine components under max_modes = 3;
      repeated  every other row repeats the one before it: d2 = 0, and at knn = 1 ell2 = 0 when
                n is even;
      lattice   rows on a lattice of spacing 1/64 or 1/512 with a gap of three spacings: every d2
                is exact and several equal ell2."""
    rng = np.random.default_rng(1000 * n + nfree + 17 * KINDS.index(kind))
    lo, hi = np.full(nfree, 0.25), np.full(nfree, 0.75)
    small = n // 3
    if kind == 'default':
        return _blobs(rng, (n - small, small), (lo, hi), 0.05, nfree), {}, \
            (1 if n <= 11 else None)
    if kind == 'blobs':
        return _blobs(rng, (n - small, small), (lo, hi), 0.05, nfree), \
            dict(knn=3, min_mode=2), (1 if n <= 4 else None)
    if kind == 'chain':
        if n < 9:
            return None
        m = 3 if n == 9 else 7
        a = (n - m) // 2
        chain = np.array([lo + 0.5 * (t + 1.0) / (m + 1.0) for t in range(m)])
        R = np.concatenate((_blobs(rng, (a, n - m - a), (lo, hi), 0.05, nfree), chain))
        return R, dict(knn=3, min_mode=2), 1
    if kind == 'equal':
        parts = {9: 3, 64: 4, 65: 5, 300: 3}.get(n)
        if parts is None:
            return None
        # (a line of evenly spaced rows per component, so that none of them splits)
        R = np.concatenate([np.full((n // parts, nfree), 0.1 + 0.2 * c) for c in range(parts)])
        R[:, 0] += 0.0005 * (np.arange(n) % (n // parts))
        return R[rng.permutation(n)], dict(knn=2, min_mode=2), parts
    if kind == 'small':
        if n < 9:
            return None
        return _blobs(rng, (n - 3, 3), (lo, hi), 0.05, nfree), dict(knn=2), 1
    if kind == 'many':
        if n < 64:
            return None
        sizes = [n // 9 + (1 if c < n % 9 else 0) for c in range(9)]
        centres = [np.full(nfree, 0.1 + 0.1 * c) for c in range(9)]
        R = _blobs(rng, sizes, centres, 0.01, nfree)
        return R[rng.permutation(n)], dict(knn=2, min_mode=2, max_modes=3), 3
    if kind == 'repeated':
        R = _blobs(rng, (n - small, small), (lo, hi), 0.05, nfree)
        R[1::2] = R[0:2 * (n // 2):2]
        return R, dict(knn=1, min_mode=1, max_modes=4096), None
    if kind == 'lattice':
        if n < 9:
            return None
        # the first n - n // 2 sites of a lattice four wide (a line where nfree = 1), a gap of
        # three spacings, the others
        width = 1 if nfree == 1 else 4
        site = np.arange(n)
        x = site // width + np.where(site >= n - n // 2, 3, 0)
        scale = 512.0 if n >= 64 else 64.0
        R = np.full((n, nfree), 0.5)
        R[:, 0] = (x + 1.0) / scale
        if nfree > 1:
            R[:, 1] = (site % width + 1.0) / scale
        return R, dict(knn=2, min_mode=2), None
    raise ValueError(kind)


def link_cases():
    """[(name, R, keywords, expected nmodes or None)]: every kind at every n of LINK_NS and nfree
    of LINK_NFREES that has one, and two blobs of 4096 rows of 3 parameters."""
    out = []
    for kind in KINDS:
        for n in LINK_NS:
            for nfree in LINK_NFREES:
                case = link_case(kind, n, nfree)
                if case is not None:
                    out.append((f'{kind}-{n}-{nfree}',) + case)
    rng = np.random.default_rng(4096)
    R = _blobs(rng, (2731, 1365), (np.full(3, 0.25), np.full(3, 0.75)), 0.05, 3)
    out.append(('default-4096-3', R, {}, 2))
    return out


# -------------------------------------------------------------------------------------------------
# hand-made points for assign_host
# -------------------------------------------------------------------------------------------------
ASSIGN_NS = (1, 63, 64, 65, 1000)


def assign_case(N, nfree, variant):
    """(P[N, nfree], R[n, nfree], labels[n]).  R: a lattice of 65 (or, for 128 parameters, 300)
    rows in two components.
      'modes'  the labels link_host gives; P[0] is the midpoint of the last row of the first
               component and the first row of the second, where every d2 is exact: equidistant
               from rows of two modes, and the lower row wins;
      'loose'  all rows loose but the largest component."""
    from pyratbay_amd import modes
    n = 300 if nfree == 128 else 65
    R, kw, _ = link_case('lattice', n, nfree)
    labels, nmodes, _ = modes.link_host(R, **kw)
    assert nmodes == 2
    rng = np.random.default_rng(N + 7 * nfree)
    P = rng.uniform(0.0, 1.0, (N, nfree))
    # (near the lattice, so that the nearest row varies from point to point)
    span = min(nfree, 2)
    P[:, :span] = rng.uniform(0.0, 1.0, (N, span)) * (1.1 * R[:, :span].max(axis=0))
    first = np.where(labels == labels[0])[0]
    other = np.where(labels != labels[0])[0]
    P[0] = 0.5 * (R[first[-1]] + R[other[0]])
    if variant == 'loose':
        labels = np.where(labels == 0, 0, -1).astype(np.int32)
    return P, R, labels
