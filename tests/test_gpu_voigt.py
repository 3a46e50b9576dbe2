"""Voigt table built by the HIP kernel against the golden table of the compiled
reference and against the oracle: small grids, the full-size grids of the benchmark
configurations and a grid of cells placed on the regime switches.  Needs an MI355X.

Tolerance: rtol 2e-12.  The reference accumulates the Region-I series in x87 long
double; the kernel is binary64 (<= 4e-15), device sin/cos/exp add a few
ulp that the cancellation in Region I amplifies."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 2e-12


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.mark.parametrize('osamp', [1, 7, 12])
def test_g1_voigt_golden(eng, golden, osamp):
    g = golden('g1_voigt')
    vt = eng.VoigtTable.build(g['lorentz'], g['doppler'], g['size_in'], float(g['dwn']), osamp)
    assert np.array_equal(vt.size, g['size_out'])
    assert np.array_equal(vt.index, g['index_out'])
    assert vt.nprofile == int(g['used'])
    flat = vt.flat()
    q0, qn, st = int(g['quick_start']), int(g['quick_n']), int(g['quick_stride'])
    err = np.max(np.abs(flat[:q0] / g['profile_head'] - 1))
    print(f'osamp={osamp}: max rel err vs reference table = {err:.2e}')
    np.testing.assert_allclose(flat[:q0], g['profile_head'], rtol=RTOL)
    np.testing.assert_allclose(flat[q0:q0 + qn:st], g['quick_sub'], rtol=RTOL)
    np.testing.assert_allclose(flat[q0:q0 + qn].sum(), g['quick_sum'], rtol=1e-11)


def test_from_flat_round_trip(eng, golden, orc):
    """reference-layout table -> phase-major -> reference layout is the identity."""
    c = cases.extinction_inputs()
    size = c['size'].copy()
    index = np.zeros_like(size)
    profile = np.zeros(np.sum(2 * size + 1))
    orc.voigt_grid(profile, size, index, c['lorentz'], c['doppler'], c['own'][1] - c['own'][0])
    for osamp in (12, 5):
        vt = eng.VoigtTable.from_flat(profile, size, index, c['lorentz'], c['doppler'], osamp)
        assert np.array_equal(vt.size, size) and np.array_equal(vt.index, index)
        back = vt.flat()
        assert np.array_equal(back, profile[:vt.nprofile])


def test_realistic_grid_vs_oracle(eng, orc):
    """A width grid as voigt.py builds it (log-spaced, dlratio skipping)."""
    from pyratbay_amd import synth
    case = synth.lbl_case(2001, 10, 10, wnosamp=60, nlor=16, ndop=8, extent=60.0, cutoff=12.0)
    vg, g = case['voigt'], case['grid']
    size = vg['size'].copy()
    index = np.zeros_like(size)
    profile = np.zeros(np.sum(2 * size + 1))
    orc.voigt_grid(profile, size, index, vg['lorentz'], vg['doppler'], g['ownstep'])
    vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'], 60)
    assert np.array_equal(vt.size, size) and np.array_equal(vt.index, index)
    np.testing.assert_allclose(vt.flat(), profile[:vt.nprofile], rtol=RTOL)


def test_bad_arguments(eng):
    from pyratbay_amd._capi import PbError
    with pytest.raises(PbError):
        eng.VoigtTable.build([1e-3], [1e-2, 2e-2], [[0, 5]], 1e-3, 4)   # size 0 in column 0
    with pytest.raises(PbError):
        eng.VoigtTable.build([1e-3], [1e-2], [[-3]], 1e-3, 4)


# ---------------------------------------------------------------------------
# full-size tables and the regime switches against the oracle's own table
# ---------------------------------------------------------------------------
# Bound of the tests below.  Measured on an MI355X, worst relative error against the oracle
# (quick / two-point mean / Simpson): c2 5.8e-14 / 3.4e-14 / 4.1e-14, c3 5.8e-14 / 3.6e-14 /
# 4.9e-14, c4 6.6e-14 / 3.5e-14 / 4.3e-14, c2-res 6.6e-14 / 2.8e-14 / 3.9e-14; the boundary
# grid 4.1e-15 / 1.1e-14 / 8.6e-15 at every osamp.  (The oracle agrees with the compiled
# reference to 4.1e-15 at c2 / c3 size: test_oracle_voigt_full.py.)
TABLE_RTOL = 1e-13


def table_rows(vt, flat):
    """got_row of cases.compare_voigt_tables for a table the GPU built."""
    return lambda m, start, n: (flat[start:start + n], vt.size[m], vt.index[m])


@pytest.mark.parametrize('name', ['c2', 'c3', 'c4', 'c2-res'])
def test_full_size_table_vs_oracle(eng, orc, name):
    """The width grid of each benchmark configuration (100 x 50 cells, extent 300, cutoff 25,
    1.3-2.4e8 samples), built as the product builds it (LBLSpectrum: keep_flat 2 in `resolution`
    mode), against the oracle one Lorentz row at a time: identical size, index and zero
    pattern, every sample within TABLE_RTOL; each grid holds cells of all three regimes."""
    case = cases.full_width_grid(name)
    vg, g = case['voigt'], case['grid']
    regimes = cases.voigt_regimes(vg['doppler'], vg['size'], g['ownstep'])
    keep_flat = 2 if g.get('resolution') else False
    vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                              g['wnosamp'], keep_flat)
    flat = vt.flat()
    vt.close()
    want = cases.oracle_voigt_rows(orc, vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'])
    worst, count, total = cases.compare_voigt_tables(table_rows(vt, flat), want, regimes,
                                                     TABLE_RTOL)
    assert total == vt.nprofile == flat.size
    assert all(count.values()), count
    print(f'{name}: osamp {g["wnosamp"]}, {total} samples, cells {count}; worst rel err vs '
          'oracle ' + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))


def test_from_flat_round_trip_full_size(eng, orc):
    """The oracle's C2 table -> phase-major at osamp 180 -> reference layout: the same bits."""
    case = cases.full_width_grid('c2')
    vg, g = case['voigt'], case['grid']
    profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
    vt = eng.VoigtTable.from_flat(profile, size, index, vg['lorentz'], vg['doppler'],
                                  g['wnosamp'])
    assert np.array_equal(vt.size, size) and np.array_equal(vt.index, index)
    assert vt.nprofile == profile.size
    assert np.array_equal(vt.flat().view(np.int64), profile.view(np.int64))


@pytest.mark.parametrize('osamp', [1, 7, 180, 2520])
def test_regime_boundaries_vs_oracle(eng, orc, osamp):
    """Cells exactly on the switches of voigtn (cases.voigt_boundary_case): QUICK from 100 001
    samples on, the 3-sample minimum, step / fine at 1, 2, 3 and just below, over in the
    thousands, y on either side of 1.8 and 5, a row of aliases; cells shorter than osamp."""
    c = cases.voigt_boundary_case()
    size, dop, dwn = c['size'], c['doppler'], c['dwn']

    def plan(m, n):
        return cases.voigt_plan(size[m, n], dwn, dop[n])
    # the cells are where they were meant to be
    assert 2 * size[1, 0] + 1 == 99999 and plan(1, 0)[0] == 'simpson'
    assert 2 * size[1, 8] + 1 == 99999 and plan(1, 8)[0] == 'mean'
    assert 2 * size[1, 2] + 1 == 100001 and plan(1, 2)[0] == 'quick'
    assert size[0, 0] == 1 and size[1, 3] == 1
    want_over = {(1, 'at'): ('simpson', 2), (1, 'below'): ('mean', 1),
                 (2, 'at'): ('simpson', 4), (2, 'below'): ('simpson', 2),
                 (3, 'at'): ('simpson', 4), (3, 'below'): ('simpson', 4)}
    step = 2.0 * (dwn * 40) / 80
    for n, (k, where) in c['ratio_cols'].items():
        ratio = step / (dop[n] / 49)
        assert (ratio == k) if where == 'at' else (ratio < k and ratio > k * (1 - 1e-15))
        assert size[0, n] == 40 and plan(0, n) == want_over[(k, where)], (n, k, where)
    assert plan(0, 7)[1] > 1000
    y = c['y'][2:6, 0]
    assert y[0] < 1.8 < y[1] and y[2] < 5.0 < y[3]
    assert np.all(np.abs(y / [1.8, 1.8, 5.0, 5.0] - 1) <= 1.01e-12)
    assert size[-1, 0] > 0 and np.all(size[-1, 1:] == 0)
    assert osamp == 1 or np.any(2 * size[size > 0] + 1 < osamp)

    regimes = cases.voigt_regimes(dop, size, dwn)
    vt = eng.VoigtTable.build(c['lorentz'], dop, size, dwn, osamp)
    flat = vt.flat()
    want = cases.oracle_voigt_rows(orc, c['lorentz'], dop, size, dwn)
    worst, count, total = cases.compare_voigt_tables(table_rows(vt, flat), want, regimes,
                                                     TABLE_RTOL)
    assert total == vt.nprofile
    assert all(count.values()), count
    print(f'boundaries osamp={osamp}: worst rel err vs oracle '
          + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
