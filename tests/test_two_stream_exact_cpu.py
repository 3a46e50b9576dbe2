"""The fixture tests/golden/two_stream_exact.npz (two-stream fluxes at 50 digits:
golden/make_golden_two_stream_exact.py) checked from its stored arrays, so that no regenerated
fixture slips past the generator's own checks; the oracle's exp1 against mpmath.e1; and the depth
recurrence of two_stream_exact_cases against the oracle's running sums.

(a) the float64 NumPy statement of the interval formulas with expm1 -- what the kernels compute
    since pb_two_stream.h forms the sweeps' bracket from it -- stays below a quarter of the bound
    on every element, and of boundQ on every bolometric sum;
(b) the reference's statement, which the oracle keeps (it is the parity yardstick), exceeds the
    bound more than 1e3 times somewhere in every thin and thin_thick column and stays inside it on
    every column of the old class: the fixture tells the two forms apart, and only on inputs that
    no earlier two-stream test drew.

The bound and the classes: two_stream_exact_cases.py."""
import numpy as np
import pytest

import two_stream_exact_cases as tc


@pytest.fixture(scope='module')
def exact(golden):
    return golden('two_stream_exact')


def test_fixture_holds_the_issue_cases(exact):
    """Shapes, walkers, positive ec and dtau0, the special first intervals exactly, temperatures
    and wavenumbers in range, one walker monotonic and one with an inversion."""
    for L, W in tc.SHAPES:
        wn, f_int, top, tw = tc.shared_inputs(exact, L, W)
        assert wn.shape == f_int.shape == top.shape == tw.shape == (W,)
        assert wn.min() >= 1100.0 and wn.max() <= 7000.0 and np.all(np.diff(wn) > 0)
        special = np.flatnonzero(tc.column_class(W) == tc.CLASSES.index('special'))
        first = [tc.FIRST[(j // len(tc.CLASSES)) % len(tc.FIRST)] for j in special]
        for walker in range(tc.NWALKERS):
            ec, h, temp = tc.walker_inputs(exact, L, W, walker)
            assert ec.shape == (L, W) and h.shape == (L - 1,) and temp.shape == (L,)
            assert np.all(ec > 0) and np.all(h > 0)
            assert np.log2(h[0]) == np.round(np.log2(h[0]))
            assert temp.min() >= 300.0 and 1500.0 <= temp.max() <= 3000.0
            assert np.all(tc.planck_x(wn, temp) >= 0.5)
            assert np.all(np.diff(temp) > 0) if walker == 0 else np.any(np.diff(temp) < 0)
            _, dtau0 = tc.depth_of(ec, h)
            assert np.all(dtau0 > 0)
            assert np.array_equal(dtau0[0, special], first)
            thin = tc.column_class(W) == tc.CLASSES.index('thin')
            assert dtau0[:, thin].max() < 1e-6
    assert len(tc.cases()) == len(tc.SHAPES) * tc.NWALKERS + tc.NWALKERS


@pytest.mark.parametrize('L,W,walker,rtop', tc.cases())
def test_corrected_statement_is_inside_a_quarter_of_the_bound(exact, L, W, walker, rtop):
    ec, h, temp = tc.walker_inputs(exact, L, W, walker)
    wn, f_int, top, tw = tc.shared_inputs(exact, L, W)
    down, up, q_down, q_up = tc.truth(exact, L, W, walker, rtop)
    _, dtau0 = tc.depth_of(ec, h)
    bnd = tc.bound(wn, temp, down, up)
    got = tc.two_stream(dtau0, tc.planck(wn, temp), f_int, top if rtop == 0 else None)
    for name, flux, want, q_want in (('down', got[0], down, q_down), ('up', got[1], up, q_up)):
        worst = tc.worst_over_bound(flux, want, bnd).max()
        worst_q = np.max(np.abs(flux @ tw - q_want) / tc.bound_q(tw, bnd, want))
        print(f'L={L} W={W} walker {walker} rtop={rtop} {name}: error / bound = {worst:.3f}, '
              f'sum error / boundQ = {worst_q:.3f}')
        assert worst < 0.25 and worst_q < 0.25


@pytest.mark.parametrize('L,W,walker,rtop', tc.cases())
def test_reference_statement_fails_where_layers_are_thin(exact, orc, L, W, walker, rtop):
    ec, h, temp = tc.walker_inputs(exact, L, W, walker)
    wn, f_int, top, _ = tc.shared_inputs(exact, L, W)
    down, up, _, _ = tc.truth(exact, L, W, walker, rtop)
    depth, _ = tc.depth_of(ec, h)
    bnd = tc.bound(wn, temp, down, up)
    ref = orc.two_stream(depth, wn, temp, f_int, top, rtop)
    over = np.maximum(tc.worst_over_bound(ref[0], down, bnd),
                      tc.worst_over_bound(ref[1], up, bnd))
    cls = tc.column_class(W)
    thin = (cls == tc.CLASSES.index('thin')) | (cls == tc.CLASSES.index('thin_thick'))
    old = cls == tc.CLASSES.index('old')
    print(f'L={L} W={W} walker {walker} rtop={rtop}: reference statement, worst error / bound per '
          f'column: thin and thin_thick {over[thin].min():.3g} ... {over[thin].max():.3g}, '
          f'old at most {over[old].max():.3f}')
    assert np.all(over[thin] > 1e3)
    assert np.all(over[old] <= 1.0)


def test_oracle_exp1_against_mpmath(exact, orc):
    """The E1XB routine as the oracle (and exp1_real on the device) states it, against mpmath.e1
    at 50 digits: at most 64 units of 2^-53, the next power of two above four times the 9.6
    measured -- so the worst must stay below 16.  exp1(0) = inf and exp1(< 0) = NaN stay."""
    x, want = exact['exp1_x'], exact['exp1_y']
    assert len(x) >= 3000 and x.min() < 2e-16 and x.max() == 1e3
    assert set(tc.FIRST) <= set(x.tolist())
    units = tc.exp1_units(orc.exp1(x), want)
    worst = int(np.argmax(units))
    print(f'orc.exp1 against mpmath.e1: worst {units[worst]:.2f} units of 2^-53 at x = {x[worst]!r}')
    assert np.all(units <= 64.0)
    assert units[worst] < 16.0
    units_np = tc.exp1_units(tc.exp1(x), want)
    print(f'two_stream_exact_cases.exp1: worst {units_np.max():.2f} units of 2^-53')
    assert units_np.max() < 16.0
    assert np.isinf(orc.exp1(np.array([0.0]))[0]) and np.isnan(orc.exp1(np.array([-0.5]))[0])


def test_depth_has_the_bits_of_the_oracle(exact, orc):
    """depth_of is plane_parallel_optical_depth(maxdepth = inf) for every walker."""
    for L, W in tc.SHAPES:
        for walker in range(tc.NWALKERS):
            ec, h, _ = tc.walker_inputs(exact, L, W, walker)
            want = np.zeros((L, W))
            stop = np.zeros(W, np.int32)
            orc.plane_parallel_optical_depth(want, stop, np.ascontiguousarray(ec), h, np.inf, 0, L)
            depth, dtau0 = tc.depth_of(ec, h)
            assert np.array_equal(depth, want)
            assert np.array_equal(dtau0, np.diff(want, axis=0))
