"""The host forms of radiative equilibrium with the equilibrium chemistry of every iteration:
ChemNetwork.equilibrium_host from a carried iterate (the host form of pb_radeq_equilibrium) on the
warm-start grid of radeq_chemistry_cases.py, and the host chain against fixture G31
(tests/golden/make_golden_radeq_chemistry.py).

Bounds.  Warm against cold: 2e-12 relative on every species with a cold VMR >= 1e-250, ten times
the 2.0e-13 measured on the grid (profiles/radeq_chemistry.md); two converged solutions of one
convex problem.  Iterations of a warm solve with |dT| <= 50 K: at most 8 (measured 2-6) and never
more than the cold solve.  Every check prints its figure before it asserts."""
import numpy as np
import pytest

import chemistry_cases as cc
import radeq_chemistry_cases as rq

WARM_BOUND = 2e-12


@pytest.fixture(scope='module')
def ch():
    from pyratbay_amd import chemistry
    return chemistry


@pytest.fixture(scope='module')
def net():
    return rq.network()


@pytest.fixture(scope='module')
def grid(net):
    """The grid's solutions, computed once: the starts, the cold solves and the warm ones."""
    p, t_start, t_solve, dt = rq.warm_grid()
    start = net.equilibrium_host(t_start, p, cc.B, start='cold')
    cold = net.equilibrium_host(t_solve, p, cc.B, start='cold')
    warm = net.equilibrium_host(t_solve, p, cc.B, start=start[3])
    assert np.all(start[2] > 0) and np.all(cold[2] > 0)
    return dict(p=p, t_start=t_start, t_solve=t_solve, dt=dt, start=start[3], cold=cold, warm=warm)


def deviation(vmr, cold):
    seen = cold >= 1e-250
    return np.where(seen, np.abs(vmr / np.where(seen, cold, 1.0) - 1.0), 0.0)


def test_grid_is_the_stated_one(grid):
    assert len(grid['p']) == 2 * 384
    assert grid['t_start'].min() >= 300.0 and grid['t_solve'].max() <= 6000.0
    assert set(np.abs(grid['dt'])) == {1.0, 10.0, 50.0, 300.0, 1500.0}


def test_warm_equals_cold(grid):
    dev = deviation(grid['warm'][0], grid['cold'][0])
    i = np.unravel_index(np.argmax(dev), dev.shape)
    print(f'warm against cold: {dev.max():.2e} (bound {WARM_BOUND:.0e}) at p = '
          f'{grid["p"][i[0]]:g} bar, {grid["t_start"][i[0]]:g} -> {grid["t_solve"][i[0]]:g} K, '
          f'{cc.SPECIES[i[1]]}')
    assert np.all(grid['warm'][2] > 0)
    assert dev.max() <= WARM_BOUND


def test_no_cell_falls_back_and_the_counts(net, ch, grid):
    """The warm Newton iteration itself converges in every cell (equilibrium_host would hide a
    fallback behind the cold solve); its counts against the cold solve's."""
    g, lnp = net.gibbs_at(grid['t_solve']), np.log(grid['p'])
    _, its, ok, _, _ = net._newton(g, lnp, cc.B, ch.TOLERANCE, grid['start'], ch.TOL_ALL)
    assert ok.all(), f'{np.sum(~ok)} cells did not converge from the carried iterate'
    assert np.array_equal(its, grid['warm'][1])
    cold = grid['cold'][1]
    for size in (1.0, 10.0, 50.0, 300.0, 1500.0):
        pick = np.abs(grid['dt']) == size
        print(f'|dT| = {size:6g} K: warm {its[pick].min()}-{its[pick].max()} (mean '
              f'{its[pick].mean():.2f}), cold {cold[pick].min()}-{cold[pick].max()}')
    small = np.abs(grid['dt']) <= 50.0
    assert its[small].max() <= 8
    assert np.all(its[small] <= cold[small])


def test_the_weighted_test_alone_passes_wrong_trace_species(net, grid):
    """tol_all = inf leaves CEA's test, weighed by n_i: some cells then 'converge' in one
    iteration with species far off -- the reason for TOL_ALL."""
    loose = net.equilibrium_host(grid['t_solve'], grid['p'], cc.B, start=grid['start'],
                                 tol_all=np.inf)
    dev = deviation(loose[0], grid['cold'][0])
    print(f'tol_all = inf: warm against cold {dev.max():.2e}, fewest iterations {loose[1].min()}')
    assert loose[1].min() == 1
    assert dev.max() > 1e-3


@pytest.mark.parametrize('tol_all', [1e-6, 1e-11])
def test_other_values_of_tol_all_give_the_same(net, grid, tol_all):
    other = net.equilibrium_host(grid['t_solve'], grid['p'], cc.B, start=grid['start'],
                                 tol_all=tol_all)
    dev = deviation(other[0], grid['cold'][0])
    print(f'tol_all = {tol_all:g}: warm against cold {dev.max():.2e}')
    assert np.all(other[2] > 0) and dev.max() <= WARM_BOUND


def test_start_cold_has_the_bits_of_the_plain_call(net, grid):
    plain = net.equilibrium_host(grid['t_solve'][:40], grid['p'][:40], cc.B)
    for a, b in zip(plain, (v[:40] for v in grid['cold'][:3])):
        assert np.array_equal(a, b)


def test_a_start_that_is_not_finite_gives_the_cold_bits(net, grid):
    n = 24
    ln_ni, ln_n = grid['start'][0][:n].copy(), grid['start'][1][:n].copy()
    ln_ni[3, 5], ln_ni[7, 0], ln_n[11] = np.nan, np.inf, np.nan
    ln_ni[15] = 700.0                                  # finite, and nothing converges from it
    got = net.equilibrium_host(grid['t_solve'][:n], grid['p'][:n], cc.B, start=(ln_ni, ln_n))
    for k in (3, 7, 11, 15):
        assert np.array_equal(got[0][k], grid['cold'][0][k]), k
        assert got[1][k] == grid['cold'][1][k] and got[2][k] == grid['cold'][2][k]
        assert np.array_equal(got[3][0][k], grid['cold'][3][0][k])
        assert got[3][1][k] == grid['cold'][3][1][k]
    others = np.setdiff1d(np.arange(n), [3, 7, 11, 15])
    assert np.array_equal(got[0][others], grid['warm'][0][:n][others])


def test_a_failed_cell_keeps_its_start(net):
    """A temperature outside the Gibbs table: the status, zeros in vmr, the start unchanged."""
    p, t = np.array([1.0, 1.0]), np.array([1000.0, 7000.0])
    first = net.equilibrium_host([1000.0, 1100.0], p, cc.B, start='cold')
    got = net.equilibrium_host(t, p, cc.B, start=first[3])
    from pyratbay_amd import chemistry
    assert got[2][0] > 0 and got[2][1] == chemistry.STATUS_TEMPERATURE
    assert np.all(got[0][1] == 0.0)
    assert np.array_equal(got[3][0][1], first[3][0][1]) and got[3][1][1] == first[3][1][1]
    with pytest.raises(ValueError, match="'cold' or"):
        net.equilibrium_host(t, p, cc.B, start='warm')
    with pytest.raises(ValueError, match='start must have shapes'):
        net.equilibrium_host(t, p, cc.B, start=(first[3][0][:1], first[3][1]))


def test_the_binding_has_the_new_entry_and_fields():
    from pyratbay_amd import _capi
    assert _capi.struct('pb_radeq')._fields_[-1][0] == 'temps_only'
    names = [f[0] for f in _capi.struct('pb_radeq_chem')._fields_]
    assert names == ['ln_ni_d', 'ln_n_d', 'vmr_d', 'mm_d', 'mol_mass_d', 'status_d',
                     'failures_d', 'tol_all']
    assert 'pb_radeq_equilibrium' in _capi.exported_names()


# ------------------------------------------------------------------------------ the trajectories
@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def bound(name):
    return max(10.0 * float(rq.fixture()[f'{name}_sens']), 1e-12)


@pytest.mark.parametrize('name', rq.CASES)
def test_host_trajectory_reproduces_the_fixture(orc, name):
    c, fx = rq.case(name), rq.fixture()
    assert fx[f'{name}_temps'].shape == (c['nw'], rq.NITER + 1, c['L'])
    assert fx[f'{name}_vmr_hist'].shape == (c['nw'], rq.NITER, c['L'], len(rq.SPECIES))
    for w in range(c['nw']):
        run = rq.run_host(orc, c, w, rq.NITER)
        terr = np.max(np.abs(run['temps'] - fx[f'{name}_temps'][w]) / fx[f'{name}_temps'][w])
        verr = deviation(run['vmr'], fx[f'{name}_vmr_hist'][w]).max()
        print(f'case {name} profile {w}: temperatures {terr:.2e} (bound {bound(name):.2e}), VMRs '
              f'{verr:.2e} (bound 1e-9)')
        assert terr <= bound(name)
        # (a VMR follows its temperature: d ln x / d ln T reaches 1e2 for the trace species)
        assert verr <= 1e-9
        assert np.array_equal(run['sign'], fx[f'{name}_sign'][w])
        assert np.array_equal(run['wobble'], fx[f'{name}_wobble'][w])
        assert np.array_equal(run['convective'], fx[f'{name}_convective'][w])
        assert not run['failures'].any()
        assert np.all(np.abs(run['chem_iterations'] - fx[f'{name}_chem_iterations'][w]) <= 1)


def test_fixture_covers_what_it_is_for():
    fx = rq.fixture()
    for name in rq.CASES:
        assert float(fx[f'{name}_sens']) <= 1e-8
    assert fx['r_convective'].any()
    ch4, co = (fx['r_vmr_hist'][0][:, :, rq.SPECIES.index(s)] for s in ('CH4', 'CO'))
    assert np.any(ch4[0] > co[0]) and np.any(ch4[0] < co[0])
    assert np.any((ch4[0] > co[0]) != (ch4[-1] > co[-1]))
    q = rq.case('q')
    assert list(q['metal']) == [-0.5, 0.0, 1.0] and list(q['c_o']) == [0.3, 0.55, 1.1]
    assert not np.array_equal(fx['r_restart_temps'], fx['r_temps'][0])


def test_cold_start_trajectory_stays_within_the_bound(orc):
    """chemistry_start='cold' on the host: the same trajectory within the fixture's bound, with
    more solver iterations in every layer."""
    c, fx = rq.case('p'), rq.fixture()
    run = rq.run_host(orc, c, 0, rq.NITER, start='cold')
    terr = np.max(np.abs(run['temps'] - fx['p_temps'][0]) / fx['p_temps'][0])
    print(f'cold start: temperatures {terr:.2e} (bound {bound("p"):.2e}); iterations '
          f'{run["chem_iterations"].min()}-{run["chem_iterations"].max()} against '
          f'{fx["p_chem_iterations"].min()}-{fx["p_chem_iterations"].max()}')
    assert terr <= bound('p')
    assert np.all(run['chem_iterations'] >= fx['p_chem_iterations'][0])
    assert run['chem_iterations'].sum() > fx['p_chem_iterations'].sum()
