#!/usr/bin/env python3
"""Fixture two_stream_exact.npz: two-stream fluxes (pyrat/spectrum.py:454-522; Heng et al. 2014
Eqs. B5-B6) at 50 digits, for the statements of csrc/pb_two_stream.h and the four kernels that
share them.

    python tests/golden/make_golden_two_stream_exact.py

Needs mpmath, NumPy and the oracle's library (for check (b) only); reads nothing else.
tests/two_stream_exact_cases.py holds what this file and the tests state identically: shapes,
classes of columns, the depth recurrence, the float64 statements, the bound.

Inputs, per shape (L, W) and walker: intervals[L - 1] (cm, the first one a power of two), temp[L]
in [300, 3000] K with the maximum at or above 1500 K -- walker 0 rises monotonically with depth,
walker 1 has inversions (temperatures() below) -- and ec[L, W] > 0, solved row by row from a
target optical depth per interval (ec[i + 1] = 2 target / h[i] - ec[i]; a target that would make
the next row non-positive becomes 1.05 ... 2 times that limit).  The columns cycle over four
classes of targets:

    thin        ascending draws of 10**U(-16, -8)
    thin_thick  10**(linspace(-16, 2, L - 1) + U(-0.3, 0.3))
    old         10**U(-3, 0.7), what every earlier two-stream test drew
    special     as old, but the first interval is exactly 1, 0.999999, 1.000001, 80, 40, 4, 1e-3,
                1e3, 1e-16 or 2^-30 (cycled): exp1's branch point, the steps of its continued
                fraction's length, exp(-dtau0) underflowing, dtau0 below 2^-53

Per shape: wn[W] in [1100, 7000] cm-1 (h c wn / (k T) >= 0.5 everywhere), f_int[W], flux_top[W]
and the trapezoid weights tw[W] of wn.

Truth.  depth and dtau0 come from cases.depth_of (the kernels' float64 recurrence); the float64
dtau0, temp, wn, f_int, flux_top and tw are taken as exact, the constants of pb_common.h as the
doubles they are, and at 50 digits: the Planck function, trans = (1 - dtau0) exp(-dtau0) +
dtau0^2 E1(dtau0) with mpmath.e1, both sweeps for rtop = 0 and, for the (17, 257) shape, for
rtop = 3 (the irradiation is then lost, as in the reference), and q_up[i], q_down[i] =
sum_j tw[j] flux[i][j].  Stored rounded to float64.  exp1_x, exp1_y: mpmath.e1 at 3000 points
log-uniform in [1e-16, 630] and at the special arguments.

Before writing, the checks (their maxima are printed and kept in profiles/two_stream.md):
  (a) the float64 NumPy statement with expm1 (cases.two_stream) stays below a quarter of bound on
      every element and of boundQ on every sum;
  (b) the reference's statement (oracle.two_stream) exceeds bound more than 1e3 times on at least
      one element of every thin and thin_thick column and stays inside it on every old column."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import two_stream_exact_cases as tc  # noqa: E402

OUT = os.path.join(HERE, 'two_stream_exact.npz')
DPS = 50
SEED = 20959
NEXP1 = 3000


def trapezoid_weights(wn):
    """t[W] with sum(t * y) = np.trapezoid(y, wn) in exact arithmetic (radeq.trapezoid_weights)."""
    t = np.zeros(len(wn))
    gaps = np.diff(wn)
    t[0], t[-1] = gaps[0] / 2.0, gaps[-1] / 2.0
    t[1:-1] = (wn[2:] - wn[:-2]) / 2.0
    return t


def solve_ec(rng, h, W):
    """ec[L, W] of one walker from the per-interval targets of the module docstring."""
    n = len(h)
    cls = tc.column_class(W)
    target = np.empty((n, W))
    for j in range(W):
        name = tc.CLASSES[cls[j]]
        if name == 'thin':
            t = 10.0**np.sort(rng.uniform(-16.0, -8.0, n))
        elif name == 'thin_thick':
            t = 10.0**(np.linspace(-16.0, 2.0, n) + rng.uniform(-0.3, 0.3, n))
        else:
            t = 10.0**rng.uniform(-3.0, 0.7, n)
        if name == 'special':
            t[0] = tc.FIRST[(j // len(tc.CLASSES)) % len(tc.FIRST)]
        target[:, j] = t
    ec = np.empty((n + 1, W))
    ec[0] = target[0] / h[0]
    for i in range(n):
        # ec[i + 1] = 2 target / h[i] - ec[i] > 0  <=>  target > 0.5 h[i] ec[i]
        floor = 0.5 * h[i] * ec[i] * (1 + 1e-6)
        bad = target[i] <= floor
        if i == 0:
            assert not bad.any()                 # (ec[1] = ec[0]: half the target each)
        target[i, bad] = floor[bad] * rng.uniform(1.05, 2.0, bad.sum())
        ec[i + 1] = 2 * target[i] / h[i] - ec[i]
    assert np.all(ec > 0)
    return ec


def temperatures(rng, L, walker):
    """temp[L] in [300, 3000] K, the hottest layer drawn from [1500, 3000] K.  Neighbouring layers
    differ by at most min(0.01 L, 0.2) in ln T: the bound grows with L while the reference's form
    loses pi |dB| 2^-53 / dtau0 per interval whatever L is, so a profile of two or three layers
    with steps of a factor of two would put the OLD class outside the bound too (check (b):
    test_gpu_two_stream_batch.py draws the two layers of L = 2 within 5e-4 for the same reason).
    Walker 0 rises monotonically with depth, by at most a factor of 5 in all; walker 1 takes steps
    of either sign (for L = 2: colder below)."""
    step = min(0.01 * L, 0.2)
    if walker == 0:
        step = min(step, np.log(5.0) / (L - 1))
        steps = rng.uniform(0.1 * step, step, L - 1)
    else:
        steps = rng.uniform(-step, step, L - 1)
        if L == 2:
            steps = -np.abs(steps)
    ln_t = np.concatenate([[0.0], np.cumsum(steps)])
    temp = np.maximum(rng.uniform(1500.0, 3000.0) * np.exp(ln_t - ln_t.max()), 300.0)
    if walker == 0:
        assert np.all(np.diff(temp) > 0)
    else:
        assert np.any(np.diff(temp) < 0)
    return temp


def inputs(rng, L, W):
    """The shape's shared rows and its walkers' (ec, intervals, temp)."""
    wn = np.sort(rng.uniform(1100.0, 7000.0, W))
    wn[0], wn[-1] = 1100.0, 7000.0
    shared = dict(wn=wn, f_int=10.0**rng.uniform(0, 2, W), flux_top=10.0**rng.uniform(2, 4, W),
                  tw=trapezoid_weights(wn))
    walkers = []
    for walker in range(tc.NWALKERS):
        h = 2.0e6 * (1 + 0.03 * np.arange(L - 1)) * rng.uniform(0.9, 1.1, L - 1)
        h[0] = 2.0**np.round(np.log2(h[0]))
        temp = temperatures(rng, L, walker)
        assert temp.max() >= 1500.0 and temp.min() >= 300.0 and temp.max() <= 3000.0
        ec = solve_ec(rng, h, W)
        _, dtau0 = tc.depth_of(ec, h)
        assert np.all(dtau0 > 0)
        special = np.flatnonzero(tc.column_class(W) == tc.CLASSES.index('special'))
        first = [tc.FIRST[(j // len(tc.CLASSES)) % len(tc.FIRST)] for j in special]
        assert np.array_equal(dtau0[0, special], first)
        walkers.append((ec, h, temp))
    assert np.all(tc.planck_x(wn, np.array([3000.0])) >= 0.5)
    return shared, walkers


def exact(dtau0, wn, temp, f_int, flux_tops, tw):
    """{rtop-key: (down, up, q_down, q_up)} at DPS digits, rounded to float64, for every top
    boundary of flux_tops (a dict key -> row or None)."""
    import mpmath as mp
    n, W = dtau0.shape
    L = n + 1
    out = {}
    with mp.workdps(DPS):
        h, c, k = mp.mpf(tc.K_H), mp.mpf(tc.K_LS), mp.mpf(tc.K_KB)
        third = mp.mpf(1) / 3
        B = [[None] * W for _ in range(L)]
        for j in range(W):
            w = mp.mpf(float(wn[j]))
            factor = 2 * h * c * c * w**3
            for i in range(L):
                B[i][j] = factor / mp.expm1(h * c * w / (k * mp.mpf(float(temp[i]))))
        trans = [[None] * W for _ in range(n)]
        slope = [[None] * W for _ in range(n)]           # pi Bp (2/3 (1 - e^-d) - d (1 - trans/3))
        for i in range(n):
            for j in range(W):
                d = mp.mpf(float(dtau0[i, j]))
                t = (1 - d) * mp.exp(-d) + d * d * mp.e1(d)
                trans[i][j] = t
                slope[i][j] = mp.pi * (B[i + 1][j] - B[i][j]) / d * \
                    (-2 * third * mp.expm1(-d) - d * (1 - t * third))
        twm = [mp.mpf(float(v)) for v in tw]
        for name, top in flux_tops.items():
            down = [[mp.mpf(0)] * W for _ in range(L)]
            up = [[mp.mpf(0)] * W for _ in range(L)]
            for j in range(W):
                if top is not None:
                    down[0][j] = mp.mpf(float(top[j]))
                for i in range(n):
                    down[i + 1][j] = trans[i][j] * down[i][j] + \
                        mp.pi * B[i][j] * (1 - trans[i][j]) - slope[i][j]
                up[L - 1][j] = down[L - 1][j] + mp.mpf(float(f_int[j]))
                for i in reversed(range(n)):
                    up[i][j] = trans[i][j] * up[i + 1][j] + \
                        mp.pi * B[i + 1][j] * (1 - trans[i][j]) + slope[i][j]
            q_down = [mp.fsum(twm[j] * down[i][j] for j in range(W)) for i in range(L)]
            q_up = [mp.fsum(twm[j] * up[i][j] for j in range(W)) for i in range(L)]

            def f64(rows):
                return np.array([[float(v) for v in row] for row in rows])
            out[name] = (f64(down), f64(up), np.array([float(v) for v in q_down]),
                         np.array([float(v) for v in q_up]))
    return out


def exp1_table(rng):
    import mpmath as mp
    x = np.concatenate([10.0**rng.uniform(-16.0, np.log10(630.0), NEXP1), tc.FIRST])
    with mp.workdps(DPS):
        y = np.array([float(mp.e1(mp.mpf(float(v)))) for v in x])
    return x, y


def checks(store, orc):
    """Checks (a) and (b) of the module docstring on the arrays about to be written; returns the
    printed maxima."""
    worst_a = worst_aq = 0.0
    least_thin, worst_old = np.inf, 0.0
    for L, W, walker, rtop in tc.cases():
        ec, h, temp = tc.walker_inputs(store, L, W, walker)
        wn, f_int, top, tw = tc.shared_inputs(store, L, W)
        down, up, q_down, q_up = tc.truth(store, L, W, walker, rtop)
        depth, dtau0 = tc.depth_of(ec, h)
        bnd = tc.bound(wn, temp, down, up)
        got = tc.two_stream(dtau0, tc.planck(wn, temp), f_int, top if rtop == 0 else None)
        cls = tc.column_class(W)
        for flux, want, q_want in ((got[0], down, q_down), (got[1], up, q_up)):
            a = tc.worst_over_bound(flux, want, bnd).max()
            aq = np.max(np.abs(flux @ tw - q_want) / tc.bound_q(tw, bnd, want))
            assert a < 0.25 and aq < 0.25, (L, W, walker, rtop, a, aq)
            worst_a, worst_aq = max(worst_a, a), max(worst_aq, aq)
        ref = orc.two_stream(depth, wn, temp, f_int, top, rtop)
        over = np.maximum(tc.worst_over_bound(ref[0], down, bnd),
                          tc.worst_over_bound(ref[1], up, bnd))
        thin = (cls == tc.CLASSES.index('thin')) | (cls == tc.CLASSES.index('thin_thick'))
        old = cls == tc.CLASSES.index('old')
        assert np.all(over[thin] > 1e3), (L, W, walker, rtop, over[thin].min())
        assert np.all(over[old] <= 1.0), (L, W, walker, rtop, over[old].max())
        least_thin, worst_old = min(least_thin, over[thin].min()), max(worst_old, over[old].max())
    return worst_a, worst_aq, least_thin, worst_old


def build():
    rng = np.random.default_rng(SEED)
    store = {}
    for L, W in tc.SHAPES:
        shared, walkers = inputs(rng, L, W)
        for name, v in shared.items():
            store[tc.key(L, W) + name] = v
        for walker, (ec, h, temp) in enumerate(walkers):
            k = tc.key(L, W, walker)
            store[k + 'ec'], store[k + 'intervals'], store[k + 'temp'] = ec, h, temp
            tops = {'': shared['flux_top']}
            if (L, W) == tc.RTOP_SHAPE:
                tops[f'rtop{tc.RTOP}_'] = None
            _, dtau0 = tc.depth_of(ec, h)
            res = exact(dtau0, shared['wn'], temp, shared['f_int'], tops, shared['tw'])
            for name, arrays in res.items():
                for what, v in zip(('down', 'up', 'q_down', 'q_up'), arrays):
                    store[k + name + what] = v
    store['exp1_x'], store['exp1_y'] = exp1_table(rng)
    return store


def main():
    from oracle import oracle as orc
    orc.lib()
    store = build()
    worst_a, worst_aq, least_thin, worst_old = checks(store, orc)
    print(f'(a) corrected float64 statement: worst error / bound = {worst_a:.3f}, '
          f'worst sum error / boundQ = {worst_aq:.3f}')
    print(f'(b) reference statement: least worst-element error / bound over the thin and '
          f'thin_thick columns = {least_thin:.3g}, largest over the old columns = {worst_old:.3f}')
    rel = tc.exp1_units(tc.exp1(store['exp1_x']), store['exp1_y'])
    print(f'exp1 (E1XB, float64) against mpmath.e1: worst relative error = {rel.max():.2f} units '
          'of 2^-53')
    np.savez_compressed(OUT, **store)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
