"""The record kernel's sample index of a line on a layer's grid, idwn = (int)((wavn - own0) / dwnstep),
formed without the division (trunc_quot_inv, csrc/pb_ext_args.h): q = (wavn - own0) * RN(1 / dwnstep),
t = (int)q, and t stands when q is farther than 2^-19 from every integer; else the division decides.
This file restates those operations in NumPy float64 and holds them against the true division --
the reference is int((wavn - own0) / dwnstep), never the restatement -- on the inputs where a wrong
last bit would flip the integer (lines on the samples of the layer's grid, and 1 and 2 ulp beside
them) and on 1e6 random lines per grid.  No GPU needed.

Why 2^-19: q carries two roundings and RN(x / d) one, so for |x / d| < 2^31 the two are less than
2^31 (2^-52 + 2^-53 + 2^-106) < 2^-19 apart; farther than that from every integer they lie strictly
between the same two consecutive integers."""
import numpy as np
import pytest

TOL = 0.5 - 2.0**-19

# every oversampling factor the project's grids use: the divisors of the oversampling factors of
# the benchmark configurations, the tests and the reference's default rule (synth.HCN)
OSAMPS = (6, 12, 24, 48, 60, 120, 720, 2160, 2520)


def divisors_in_use():
    from pyratbay_amd import synth
    out = set()
    for o in OSAMPS:
        out.update(int(d) for d in synth.divisors(o))
    return sorted(out)


def restated(x, d):
    """trunc_quot_inv(x, d, 1 / d) -> (result, lanes that took the product form)"""
    x = np.asarray(x, np.float64)
    inv = np.float64(1.0) / np.float64(d)
    q = x * inv
    with np.errstate(invalid='ignore'):
        t = np.trunc(np.clip(q, -2.0**31, 2.0**31 - 1))           # (int)q saturates
        f = np.abs(q - t)
        fast = np.abs(f - 0.5) < TOL                               # False for NaN
    slow = np.trunc(x / np.float64(d))
    return np.where(fast, t, slow).astype(np.int64), fast


def true_index(x, d):
    return np.trunc(np.asarray(x, np.float64) / np.float64(d)).astype(np.int64)


def ulp_moves(v):
    v = np.asarray(v, np.float64)
    out = [v]
    up, down = v, v
    for _ in range(2):
        up = np.nextafter(up, np.inf)
        down = np.nextafter(down, -np.inf)
        out += [up, down]
    return np.concatenate(out)


def grid_points(own0, dwnstep, onwn):
    n = {0, 1, onwn - 1}
    k = 1
    while k < onwn:
        n.update((k - 1, k, k + 1))
        k *= 2
    n = np.array(sorted(i for i in n if 0 <= i < onwn), np.float64)
    return ulp_moves(own0 + n * dwnstep)


@pytest.mark.parametrize('own0', [4000.0, 0.1])
@pytest.mark.parametrize('ownstep', [2.8e-4, 0.005, 1 / 3e3])
def test_index_equals_true_division(ownstep, own0):
    onwn_fine = 100_000 * 24                       # a fine grid as long as the largest benchmark's
    rng = np.random.default_rng(int(ownstep * 1e7) + int(own0))
    total = fast_total = 0
    for ofactor in divisors_in_use():
        dwnstep = np.float64(ownstep) * np.float64(ofactor)     # k_layer_state: ownstep * ofactor
        onwn = 1 + (onwn_fine - 1) // ofactor
        wavn = grid_points(np.float64(own0), dwnstep, onwn)
        x = wavn - np.float64(own0)
        got, fast = restated(x, dwnstep)
        assert np.array_equal(got, true_index(x, dwnstep)), (ofactor, 'grid points')
        # where the product form stands, it stands on its own: the same integer as the division
        assert np.array_equal(np.trunc(x * (1.0 / dwnstep))[fast].astype(np.int64),
                              true_index(x, dwnstep)[fast])
        total += len(x)
        fast_total += int(fast.sum())
    # random lines: one grid per ownstep / own0 pair is the issue's 1e6; the factor 1 grid is the
    # longest (largest quotients, coarsest ulp)
    for ofactor in (1, divisors_in_use()[-1]):
        dwnstep = np.float64(ownstep) * np.float64(ofactor)
        wavn = np.float64(own0) + rng.uniform(0.0, onwn_fine * ownstep, 1_000_000)
        x = wavn - np.float64(own0)
        got, fast = restated(x, dwnstep)
        assert np.array_equal(got, true_index(x, dwnstep)), (ofactor, 'random lines')
        # the division is the exception: a random line is within 2^-19 of a sample 4e-6 of the time
        assert fast.mean() > 0.999, fast.mean()


def test_special_values_take_the_division():
    d = np.float64(0.005)
    with np.errstate(all='ignore'):
        x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0**31 * 0.005, 2.0**40, -3.2 * 0.005,
                      -3.0 * 0.005, 2.0**-1070])
        got, fast = restated(x, d)
        assert not fast[[0, 1, 2, 3, 4, 6, 9]].any()
        finite = np.isfinite(x)
        assert np.array_equal(got[finite], true_index(x[finite], d))
    assert got[7] == -3                       # truncation toward zero, like the cast


def test_tolerance_covers_the_error_bound():
    """2^31 (2^-52 + 2^-53 + 2^-106) < 2^-19, in exact rational arithmetic."""
    from fractions import Fraction as F
    assert F(2)**31 * (F(2)**-52 + F(2)**-53 + F(2)**-106) < F(2)**-19
    assert TOL == 0.5 - 2.0**-19
