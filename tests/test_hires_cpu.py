"""Host side of the high-resolution data path (pyratbay_amd/hires.py) against fixture G21 =
the taps the reference's ps.inst_convolution hands to scipy.signal.convolve
(tests/golden/make_golden_hires.py).  No GPU."""
import math

import numpy as np
import pytest


def cases(g):
    for c in range(int(g['ncases'])):
        r_inst, r_samp = g[f'c{c}_resolution']
        yield c, float(r_inst), (None if np.isnan(r_samp) else float(r_samp))


def test_inst_kernel_scipy_form(golden):
    """With SciPy: the same calls of the same library as the reference -- bit-equal when the
    SciPy version is the fixture's, else within 1e-15 of the largest tap."""
    scipy = pytest.importorskip('scipy')
    from pyratbay_amd import hires
    g = golden('g21_hires')
    for c, r_inst, r_samp in cases(g):
        want = g[f'c{c}_taps']
        got = hires.inst_kernel(r_inst, wn=g[f'c{c}_wn'], sampling_res=r_samp)
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.max(np.abs(got - want)) / np.max(want)
        print(f'case {c}: T = {len(got)}, SciPy form max |diff| / max tap = {err:.2e}')
        if scipy.__version__ == str(g['scipy_version']):
            assert np.array_equal(got, want)
        assert err <= 1e-15


def test_inst_kernel_without_scipy(golden):
    """The SciPy-free form (Gaussian window + not-a-knot spline restated): within 1e-14 of the
    largest tap (measured: below 4.5e-16; the bound leaves 20x)."""
    from pyratbay_amd import hires
    g = golden('g21_hires')
    for c, r_inst, r_samp in cases(g):
        want = g[f'c{c}_taps']
        got = hires.inst_kernel(r_inst, wn=g[f'c{c}_wn'], sampling_res=r_samp, use_scipy=False)
        assert got.shape == want.shape
        err = np.max(np.abs(got - want)) / np.max(want)
        print(f'case {c}: T = {len(got)}, SciPy-free form max |diff| / max tap = {err:.2e}')
        assert err <= 1e-14


@pytest.mark.parametrize('use_scipy', [True, False])
def test_inst_kernel_shape_and_norm(golden, use_scipy):
    """T as the reference derives it (odd: 2 n_rv0 + 1), taps summing to 1 within an ulp of 1.
    The sum meant is the taps' own (math.fsum: exact, rounded once); a running sum of T terms
    adds up to T / 2 ulp of its own (printed: 3 ulp on the reference's taps at T = 59)."""
    from pyratbay_amd import hires
    g = golden('g21_hires')
    sizes = []
    for c, r_inst, r_samp in cases(g):
        taps = hires.inst_kernel(r_inst, wn=g[f'c{c}_wn'], sampling_res=r_samp,
                                 use_scipy=use_scipy)
        sizes.append(len(taps))
        assert len(taps) % 2 == 1 and len(taps) == len(g[f'c{c}_taps'])
        total = math.fsum(taps)
        print(f'case {c}: T = {len(taps)}, fsum - 1 = {total - 1:.2e}, '
              f'running sum - 1 = {sum(taps) - 1:.2e}')
        assert abs(total - 1.0) <= np.spacing(1.0)
    assert min(sizes) == 17 and max(sizes) == 179


def test_inst_kernel_needs_a_sampling():
    from pyratbay_amd import hires
    with pytest.raises(ValueError, match='sampling'):
        hires.inst_kernel(25000.0)


def test_doppler_factor_is_rv_shift(golden):
    """The grid nodes stored in G21's data sets are wn * doppler_factor(rv), bit for bit."""
    from pyratbay_amd import hires
    g = golden('g21_hires')
    for c, _, _ in cases(g):
        wn = g[f'c{c}_wn']
        for r, rv in enumerate(g['rv']):
            shifted = wn * hires.doppler_factor(rv)
            on_node = np.sum(np.isin(g[f'c{c}_rv{r}_data_wn'], shifted))
            assert on_node == int(g[f'c{c}_rv{r}_on_node']) >= 16


def test_hires_data_host_checks(golden):
    """HiresData's constructor checks the host arrays before it touches the device."""
    from pyratbay_amd import engine, hires
    g = golden('g21_hires')
    wn = g['c0_wn']
    inside = np.linspace(wn[10], wn[-10], 50)
    with pytest.raises(ValueError, match='ascending'):
        engine.HiresData(wn[::-1], inside, 25000.0, sampling_res=123300.0)
    with pytest.raises(ValueError, match='data_wn'):
        engine.HiresData(wn, np.zeros(0), 25000.0, sampling_res=123300.0)
    with pytest.raises(ValueError, match='rv_max'):
        engine.HiresData(wn, inside, 25000.0, sampling_res=123300.0, rv_max=-1.0)
    # a point on the last node is inside the grid at rest, outside it for rv > 0
    edge = np.append(inside, wn[-1])
    hires.check_data_in_grid(wn, edge, 0.0)
    with pytest.raises(ValueError, match='shifted by up to'):
        engine.HiresData(wn, edge, 25000.0, sampling_res=123300.0, rv_max=5.0)
    with pytest.raises(ValueError, match='shifted by up to'):
        engine.HiresData(wn, np.append(inside, wn[0] * (1 + 1e-6)), 25000.0,
                         sampling_res=123300.0, rv_max=5.0)
    # an instrument profile wider than one tile + its halo is refused, not truncated
    coarse = 4000.0 + 1e-4 * np.arange(5000)
    with pytest.raises(ValueError, match=f'at most {hires.MAX_TAPS}'):
        engine.HiresData(coarse, coarse[100:200], 2000.0, rv_max=0.1)
