#!/usr/bin/env python3
"""Fixture prior_transform.npz: the exact inverse CDF of the two-sided Gaussian prior, for the
prior transform of a nested sampler (Retrieval.prior_transform_host, pb_prior_transform).

    python tests/golden/make_golden_prior_transform.py

Needs mpmath and NumPy only and reads nothing else.  Every input -- u, prior, lo, up -- is taken as
the exact double it is.  The density is exp(-0.5 ((p - prior) / s)^2) with s = lo below prior and
s = up above it; its mass below prior is lo / (lo + up), so its CDF is

    F(theta) = 2 lo / (lo + up) * Phi((theta - prior) / lo)             theta <  prior   (branch 0)
    F(theta) = 1 - 2 up / (lo + up) * Phi(-(theta - prior) / up)        theta >= prior   (branch 1)

For each element the branch is decided exactly (u (lo + up) < lo), the tail mass t of the standard
normal is formed exactly (t = u (lo + up) / (2 lo), or (1 - u) (lo + up) / (2 up)), and x >= 0 with
log Q(x) = log t, Q(x) = erfc(x / sqrt 2) / 2, is found by Newton's method on the LOGARITHM of the
tail at DPS digits: log Q is concave and decreasing, so the iteration converges from any start,
and 1e-300 is no harder than 0.3.  z = -x below prior and +x above it; theta = prior + s z.
Self-check, on the unrounded theta, with the tail evaluated anew at DPS + 20 digits:
|F(theta) - u| <= 1e-30 u, and the same relative to the tail mass itself.

Stored: params[7, 3] = (prior, lo, up) of the seven columns; u[1000, 7]; theta = theta rounded to
double; resid = theta - float(theta), rounded to double (so that theta + resid carries the exact
value to about 32 digits); z (double) and branch (0 below prior, 1 above); group[1000], the index
into group_names of the rule that made the row.

The rows (612 by rule, and a ladder that fills the cube to 1000 rows):
  existing   1e-300, 1e-16, 0.02275, 0.5, 0.97725, 1 - 1e-16 in every column
  split      fl(lo / (lo + up)) of each column and its two neighbours
  upper      upper-tail masses q = 1e-1 ... 1e-15 of each column: u = fl(1 - q 2 up / (lo + up)),
             not above 1 - 2^-53
  lower      lower-tail masses q = 1e-1 ... 1e-300 of each column: u = fl(q 2 lo / (lo + up))
  ends       2^-53 and 1 - 2^-53
  pairs      2^-k and 1 - 2^-k, k = 1 ... 53
  log_low    60 draws 10^-U(0, 300) per column;  log_high  60 draws 1 - 10^-U(0, 15.9)
  uniform    60 draws U(0, 1) per column
  ladder     388 rows: z from -37.5 to +8.25 in equal steps, u = fl(F(prior + s z)) (not below
             1e-300, not above 1 - 2^-53): both branches at an even spacing in z
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'prior_transform.npz')

DPS = 50
PARAMS = np.array([(3.0, 0.5, 0.5), (-1400.0, 0.2, 2.0), (0.25, 3.0, 0.3), (1.0e-3, 0.5, 0.05),
                   (0.0, 1.0, 1.0e-3), (0.0, 1.0e-3, 1.0), (1.0e6, 1.0e-6, 2.0e-6)])
NROWS = 1000
GROUPS = ('existing', 'split', 'upper', 'lower', 'ends', 'pairs', 'log_low', 'log_high',
          'uniform', 'ladder')
# (1e-300 is the smallest u of the rules above.  Below it u (lo + up), which the transform forms
# before it divides by lo, is subnormal for the narrowest column: no longer a rounding question.)
U_MIN, U_MAX = 1.0e-300, 1.0 - 2.0**-53
SEED = 20953


def cube():
    """(u[NROWS, 7], group[NROWS]): the rows of the module docstring, every u in (0, 1)."""
    import mpmath as mp
    prior, lo, up = PARAMS.T
    ncol = len(PARAMS)
    rows, group = [], []

    def add(name, block):
        block = np.atleast_2d(np.asarray(block, np.float64))
        assert block.shape[1] == ncol
        rows.append(block)
        group.extend([GROUPS.index(name)] * len(block))

    add('existing', [np.full(ncol, u) for u in (1e-300, 1e-16, 0.02275, 0.5, 0.97725, 1 - 1e-16)])
    split = lo / (lo + up)
    add('split', [split, np.nextafter(split, 0.0), np.nextafter(split, 1.0)])
    add('upper', [np.minimum(1.0 - 10.0**-k * (2.0 * up / (lo + up)), U_MAX)
                  for k in range(1, 16)])
    add('lower', [float(f'1e-{k}') * (2.0 * lo / (lo + up)) for k in range(1, 301)])
    add('ends', [np.full(ncol, 2.0**-53), np.full(ncol, 1.0 - 2.0**-53)])
    add('pairs', [np.full(ncol, v) for k in range(1, 54) for v in (2.0**-k, 1.0 - 2.0**-k)])
    rng = np.random.default_rng(SEED)
    add('log_low', 10.0**-rng.uniform(0.0, 300.0, (60, ncol)))
    add('log_high', np.minimum(1.0 - 10.0**-rng.uniform(0.0, 15.9, (60, ncol)), U_MAX))
    add('uniform', rng.uniform(0.0, 1.0, (60, ncol)))
    nladder = NROWS - sum(len(b) for b in rows)
    with mp.workdps(DPS):
        ladder = np.empty((nladder, ncol))
        for j, z in enumerate(np.linspace(-37.5, 8.25, nladder)):
            for c in range(ncol):
                s = lo[c] if z < 0 else up[c]
                ladder[j, c] = float(cdf(mp.mpf(prior[c]) + mp.mpf(s) * mp.mpf(z), *PARAMS[c]))
    add('ladder', np.clip(ladder, U_MIN, U_MAX))
    u = np.concatenate(rows)
    assert u.shape == (NROWS, ncol) and np.all((u > 0.0) & (u < 1.0))
    return u, np.array(group, np.int8)


def tail(x):
    """Q(x) = 1 - Phi(x), at the working precision, in the far tail too."""
    import mpmath as mp
    return mp.erfc(x / mp.sqrt(2)) / 2


def cdf(theta, prior, lo, up):
    """F(theta) of the module docstring for mpf theta and double prior, lo, up."""
    import mpmath as mp
    prior, lo, up = mp.mpf(prior), mp.mpf(lo), mp.mpf(up)
    if theta < prior:
        return 2 * lo / (lo + up) * tail((prior - theta) / lo)
    return 1 - 2 * up / (lo + up) * tail((theta - prior) / up)


def start(t):
    """A double x with Q(x) ~ t to about 1e-12, 0 < t <= 0.5: Newton on log Q in doubles from the
    leading asymptote (from the right of the root the iterates fall monotonically)."""
    if t >= 0.5:
        return 0.0
    target = math.log(t)
    x = math.sqrt(-2.0 * target) + 1.0
    for _ in range(200):
        q = 0.5 * math.erfc(x / math.sqrt(2.0))
        if q <= 0.0:                                   # (beyond the doubles: step back in)
            x -= 0.25
            continue
        slope = -math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) / q
        dx = (math.log(q) - target) / slope
        x = max(x - dx, 0.0)
        if abs(dx) <= 1e-13 * max(x, 1.0):
            break
    return x


def solve(u, prior, lo, up):
    """(theta as mpf, z as mpf, branch) with F(theta) = u for the exact doubles u, prior, lo, up;
    call under mp.workdps(DPS)."""
    import mpmath as mp
    u, prior, lo, up = mp.mpf(u), mp.mpf(prior), mp.mpf(lo), mp.mpf(up)
    branch = 0 if u * (lo + up) < lo else 1
    t = u * (lo + up) / (2 * lo) if branch == 0 else (1 - u) * (lo + up) / (2 * up)
    assert 0 < t <= mp.mpf(1) / 2
    target = mp.log(t)
    x = mp.mpf(start(float(t)))
    # (quadratic convergence: a step of 1e-22 leaves an error near 1e-44, and check() verifies it)
    small = mp.mpf('1e-22')
    for _ in range(60):
        q = tail(x)
        slope = -mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi) / q
        dx = (mp.log(q) - target) / slope
        x -= dx
        if abs(dx) <= small * max(abs(x), 1):
            break
    else:
        raise RuntimeError(f'no convergence at u = {u}, (prior, lo, up) = ({prior}, {lo}, {up})')
    if x < 0:                                          # (t = 1/2 to the last digit: the split)
        x = mp.mpf(0)
    z = -x if branch == 0 else x
    return prior + (lo if branch == 0 else up) * z, z, branch


def check(theta, u, prior, lo, up, branch):
    """|F(theta) - u| <= 1e-30 u, and relative to the tail mass on either side, with F evaluated
    anew at DPS + 20 digits."""
    import mpmath as mp
    with mp.workdps(DPS + 20):
        u = mp.mpf(u)
        f = cdf(theta, prior, lo, up)
        assert (theta < mp.mpf(prior)) == (branch == 0) or theta == mp.mpf(prior)
        assert abs(f - u) <= mp.mpf('1e-30') * u, (u, prior, lo, up)
        assert abs(f - u) <= mp.mpf('1e-30') * min(u, 1 - u), (u, prior, lo, up)


def build():
    """The arrays of the fixture, as a dict."""
    import mpmath as mp
    u, group = cube()
    theta, resid, z = np.empty_like(u), np.empty_like(u), np.empty_like(u)
    branch = np.empty(u.shape, np.int8)
    with mp.workdps(DPS):
        for c, (prior, lo, up) in enumerate(PARAMS):
            for r in range(len(u)):
                th, zz, branch[r, c] = solve(u[r, c], prior, lo, up)
                check(th, u[r, c], prior, lo, up, branch[r, c])
                theta[r, c] = float(th)
                resid[r, c] = float(th - mp.mpf(theta[r, c]))
                z[r, c] = float(zz)
    assert np.all(np.isfinite(theta)) and np.all(np.abs(resid) <= 0.5 * np.spacing(np.abs(theta)))
    return dict(params=PARAMS, u=u, theta=theta, resid=resid, z=z, branch=branch, group=group,
                group_names=np.array(GROUPS))


def main():
    store = build()
    np.savez_compressed(OUT, **store)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes, z from {store["z"].min():.2f} to '
          f'{store["z"].max():.2f}, {int(store["branch"].sum())} of {store["branch"].size} '
          'elements above prior')


if __name__ == '__main__':
    main()
