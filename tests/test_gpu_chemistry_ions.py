"""Equilibrium chemistry with ions and electrons on the device: the charged instantiations of
pb_equilibrium_vmr and pb_radeq_equilibrium (csrc/pb_chemistry.hip) at their boundary against
ChemNetwork.equilibrium_host and against the solver-independent conditions (element ratios, mass
action on [stoich | charges], charge neutrality, the Saha closed form), then H- opacity with
equilibrium chemistry through WalkerAtmosphere, eval_params, Retrieval and RadiativeEquilibrium.
Every output buffer is pre-filled with NaN (statuses with a sentinel).

Bounds, those of test_gpu_chemistry.py and test_gpu_radeq_chemistry.py: device against host VMRs
1e-9 relative wherever the host VMR is >= 1e-250, the host's status sign, iteration counts within
2; optimality and neutrality 1e-11; closed form 1e-12; a warm launch against the host's cold solve
2e-12; the mean mass against sum x_i m_i 1e-14.  Every check prints its figure before it asserts;
the figures measured on an MI355X are in profiles/chemistry_ions.md.

(The grid's 28 cells are 7 temperatures x 4 pressures and the kernel takes one pressure per layer,
so they are nw = 7 walkers of L = 4 layers; every other launch here has nw <= 4, L <= 7.)"""
import numpy as np
import pytest

import chemistry_cases as cc
import ion_cases as ic
from test_gpu_chemistry import SENTINEL, compare_with_host, run_kernel

pytestmark = pytest.mark.gpu
WARM_BOUND = 2e-12
GRID_TEMPS = np.repeat(np.array(cc.GRID_T)[:, None], 4, axis=1)          # [7, 4]
GRID_PRESS = np.array(cc.GRID_P)


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def ch():
    from pyratbay_amd import chemistry
    return chemistry


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


@pytest.fixture(scope='module')
def net(ch):
    return ic.network(ch)


@pytest.fixture(scope='module')
def grid_host(net):
    """The host's solution of the 28 cells, once."""
    return [net.equilibrium_host(GRID_TEMPS[w], GRID_PRESS, ic.B) for w in range(7)]


@pytest.fixture(scope='module')
def grid_device(eng, ch, net):
    return run_kernel(eng, ch, net, GRID_TEMPS, GRID_PRESS, guard=64)


def host(t):
    return t.cpu().numpy()


def optimality(net, vmr, temps, pressure, b):
    """(element ratios, mass action, neutrality), the worst over the cells of vmr[nw, L, S]."""
    nw, L, _ = vmr.shape
    mass = max(ic.mass_action_residual(net, vmr[w, l], temps[w, l], pressure[l])
               for w in range(nw) for l in range(L))
    return ic.element_error(net, vmr, b).max(), mass, ic.neutrality(net, vmr).max()


# ------------------------------------------------------------------------------ kernel boundary
def test_device_vs_host_on_the_grid(net, grid_host, grid_device):
    vmr, status = grid_device
    assert np.all(status > 0), status
    for w in range(7):
        want_vmr, _, want_status = grid_host[w]
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'{cc.GRID_T[w]:g} K')
    print('iterations, device (T down, p across):\n', status, '\nhost:\n',
          np.array([h[2] for h in grid_host]))
    assert np.all(vmr[..., net.charges != 0] > 0)


def test_device_optimality_without_the_host(net, grid_device):
    vmr, _ = grid_device
    elem, mass, neutral = optimality(net, vmr, GRID_TEMPS, GRID_PRESS, ic.B)
    print(f'device, 14 species: element ratios {elem:.2e}, mass action {mass:.2e}, neutrality '
          f'{neutral:.2e} (bounds 1e-11)')
    assert elem <= 1e-11 and mass <= 1e-11 and neutral <= 1e-11


def test_saha_on_the_smallest_instantiation(eng, ch):
    """S = 3, E = 1 with charges: 61 idle lanes, the 3 x 3 system."""
    saha = ic.saha_network(ch)
    temps, pressure = np.array([[3000.0, 6000.0, 6000.0, 1000.0]]), np.array([1e-4, 1e-6, 1.0, 1.0])
    vmr, status = run_kernel(eng, ch, saha, temps, pressure, guard=16)
    assert np.all(status > 0), status
    for l in range(4):
        want = ic.saha_closed_form(temps[0, l], pressure[l])
        dev = max(abs(vmr[0, l, 1] / want - 1.0), abs(vmr[0, l, 2] / want - 1.0))
        print(f'x_H+ = x_e at {temps[0, l]} K, {pressure[l]} bar: {vmr[0, l, 1]:.16e} vs '
              f'{want:.16e}, rel {dev:.2e} (bound 1e-12), {status[0, l]} iterations')
        assert dev <= 1e-12
        assert abs(vmr[0, l, 0] / (1.0 - 2.0 * want) - 1.0) <= 1e-12


def test_largest_charged_instantiation(eng, ch):
    """S = 32, E = 7 and the charge balance: the 9 x 9 system of the neutral E = 8, at 4 cells."""
    big, b = ic.padded_network(ch)
    assert (big.nspecies, big.nelements) == (32, 7) and big.charged
    temps = np.array([[600.0, 3000.0], [6000.0, 1000.0]])
    pressure = np.array([100.0, 1e-4])
    vmr, status = run_kernel(eng, ch, big, temps, pressure, guard=64)
    assert np.all(status > 0), status
    elem, mass, neutral = optimality(big, vmr, temps, pressure, b)
    print(f'device, 32 species: element ratios {elem:.2e}, mass action {mass:.2e}, neutrality '
          f'{neutral:.2e} (bounds 1e-11), iterations {status.tolist()}')
    assert elem <= 1e-11 and mass <= 1e-11 and neutral <= 1e-11
    for w in range(2):
        want_vmr, _, want_status = big.equilibrium_host(temps[w], pressure, b)
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'S = 32, walker {w}')


@pytest.mark.parametrize('enthalpy', [1.536e6, 9e6, 4e7])
def test_ions_that_underflow(eng, ch, enthalpy):
    """The cations at 1.5, 9 and 40 MJ/mol, 300 K and 1000 K at 1 bar: at 9 MJ/mol (300 K) and at
    40 MJ/mol every ion underflows, the charge row is dropped and the status is still positive."""
    network = ic.network(ch, enthalpy)
    temps, pressure = np.array([[300.0], [1000.0]]), np.array([1.0])
    vmr, status = run_kernel(eng, ch, network, temps, pressure, guard=16)
    print(f'h = {enthalpy:g}: status {status.ravel()}, ions\n', vmr[:, 0, 9:])
    assert np.all(np.isfinite(vmr)) and np.all(status > 0)
    for w in range(2):
        want_vmr, _, want_status = network.equilibrium_host(temps[w], pressure, ic.B)
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'{temps[w, 0]:g} K')
        assert np.array_equal(vmr[w] == 0, want_vmr == 0)
    assert ic.neutrality(network, vmr).max() <= 1e-11


def test_zero_charges_are_the_neutral_launch(eng, ch):
    plain = cc.network(ch)
    zeros = ch.ChemNetwork(cc.SPECIES, cc.ELEMENTS, cc.STOICH, cc.TABLE_T, cc.gibbs(cc.TABLE_T),
                           cc.BASE_DEX, charges=np.zeros(16, int))
    temps = np.array([[300.0, 1000.0, 2500.0, 6000.0], [4000.0, 600.0, 1500.0, 300.0]])
    want = run_kernel(eng, ch, plain, temps, GRID_PRESS)
    got = run_kernel(eng, ch, zeros, temps, GRID_PRESS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(want[1] > 0)


# ------------------------------------------------------------------------ pb_radeq_equilibrium
def test_carried_equilibrium_with_ions(eng, ch, net):
    """warm = 0: the bits of pb_equilibrium_vmr.  warm = 1 from T -+ 25 K: the host's cold solve
    within the carried bound, no failure, fewer iterations than the cold launch; the mean mass
    is sum x_i m_i with the electrons' mass in it."""
    import torch
    pressure = np.array([1e-8, 1e-4, 1e-2, 1.0, 100.0])
    temps = np.array([[600.0, 1000.0, 1500.0, 2500.0, 4000.0],
                      [6000.0, 3000.0, 2000.0, 800.0, 350.0]])
    shift = np.where(np.arange(10).reshape(2, 5) % 2 == 0, 25.0, -25.0)
    ce = ch.CarriedEquilibrium(net, 2, eng.dev(pressure), ic.MASS)
    ce.status.fill_(SENTINEL)

    def solve(t, warm):
        ce.solve(eng.dev(np.ascontiguousarray(t)), warm)
        torch.cuda.synchronize()
        return {k: host(getattr(ce, k)).copy() for k in ('vmr', 'mm', 'status', 'failures',
                                                         'ln_ni', 'ln_n')}
    cold = solve(temps, False)
    want_vmr, want_status = ch.equilibrium_vmr(net, eng.dev(temps), eng.dev(pressure))
    torch.cuda.synchronize()
    assert np.all(cold['status'] > 0), cold['status']
    assert np.array_equal(cold['status'], host(want_status))
    assert np.array_equal(cold['vmr'], host(want_vmr))
    assert np.all(np.isfinite(cold['ln_ni'])) and np.all(np.isfinite(cold['ln_n']))

    warm = solve(temps + shift, True)
    assert np.all(warm['status'] > 0) and not warm['failures'].any()
    worst = 0.0
    for w in range(2):
        v = net.equilibrium_host(temps[w] + shift[w], pressure, ic.B)[0]
        seen = v >= 1e-250
        worst = max(worst, np.max(np.abs(warm['vmr'][w][seen] / v[seen] - 1.0)))
    neutral = ic.neutrality(net, warm['vmr']).max()
    print(f'warm launch against the host cold solve: {worst:.2e} (bound {WARM_BOUND:.0e}), '
          f'neutrality {neutral:.2e}; iterations warm {warm["status"].tolist()}, cold '
          f'{cold["status"].tolist()}')
    assert worst <= WARM_BOUND and neutral <= 1e-11
    assert np.all(warm['status'] < cold['status'])
    for run in (cold, warm):
        mm = np.sum(run['vmr'] * ic.MASS, axis=-1)
        err = np.max(np.abs(run['mm'] / mm - 1.0))
        print(f'mean mass against sum x_i m_i: {err:.2e} (bound 1e-14)')
        assert err <= 1e-14
    # the electrons count: at 6000 K and 1e-8 bar they are 4 % of the particles
    ie = net.species.index('e-')
    assert cold['vmr'][1, 0, ie] > 0.01
    without = np.sum(np.delete(cold['vmr'][1, 0] * ic.MASS, ie))
    assert abs(cold['mm'][1, 0] / without - 1.0) > 1e-6


# ------------------------------------------------------------------------------------ end to end
BLOCK = """
    T_iso       2500.0  1500.0  3200.0   50.0
    [M/H]          0.0    -2.0     2.0    0.3    0.0    0.5
"""


def test_hminus_with_equilibrium_chemistry_end_to_end(eng, pa, ch, golden):
    """An isothermal atmosphere on the 16 species + ions network with [M/H] free, and a continuum
    with H- (Rayleigh, CIA, H-) on the table of test_gpu_chemistry's retrieval test (L = 12, 1000
    samples, transit): eval_params and Retrieval.log_posterior against eval_bands fed with
    evaluate_host's profiles, with that test's bounds -- the two sides' VMRs may differ by 1e-9,
    a band depth then by ten times that, the likelihood by sum |d - m| / s^2 * 1e-8 m.  And the
    H- term is in: without the electrons' column the spectrum is another."""
    import torch
    import test_gpu_batch_continuum as base
    network, mass, _ = ic.sixteen_with_ions(ch)
    s = base.setup(golden('g7_continuum'), 4, seed=77, hminus=True, clouds=False)
    wn, pressure, cont = s['wn'], s['pressure'], s['cont']
    assert cont.species == ['H2', 'He', 'H', 'e-'] and cont.hminus
    atm = pa.WalkerAtmosphere(pressure, network.species, mass, None, None,
                              pa.Isothermal(pressure), [pa.MetalEquil()], mplanet=1.2e30,
                              rplanet=7.5e9, refpressure=0.1, base_params=[2500.0, 0.0],
                              chemistry=network)
    atm.bind(['H2O', 'CO', 'CH4'], cont)
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, atm.base_radius, 8.8e10,
                              rt_path='transit', column_order=None, continuum=cont)
    _, pb = base.make_bands(eng, wn)
    theta = np.array([[2500.0, 0.0], [2900.0, 0.8], [2100.0, -0.6], [2700.0, 0.3]])
    flux = host(model.eval_params(atm, eng.dev(theta), pb))
    assert np.all(np.isfinite(flux)) and np.all(flux > 0)

    profs = [atm.evaluate_host(p) for p in theta]
    assert all(p.reject == 0 for p in profs)
    cdens = np.stack([p.continuum_density for p in profs])
    assert np.all(cdens[..., 3] > 0)

    def bands(continuum_density):
        return model.eval_bands(eng.dev(np.stack([p.temps for p in profs])),
                                eng.dev(np.stack([p.dens for p in profs])), pb,
                                radius=eng.dev(np.stack([p.radius for p in profs])),
                                continuum_density=eng.dev(continuum_density))
    host_flux_d = bands(cdens)
    host_flux = host(host_flux_d)
    dev = np.max(np.abs(flux / host_flux - 1.0))
    print(f'eval_params against eval_bands on the host profiles: {dev:.2e} (bound 1e-8)')
    assert dev <= 1e-8
    no_electrons = cdens.copy()
    no_electrons[..., 3] = 0.0
    change = np.abs(host(bands(no_electrons)) / host_flux - 1.0)
    print('band depths without the electrons, relative change per walker:\n', change)
    assert np.all(change.max(axis=1) > 0.0)

    data = flux[0] * (1 + np.random.default_rng(11).normal(0, 0.02, 3))
    uncert = 0.03 * flux[0]
    obs = eng.Observation(data, uncert)
    ret = eng.Retrieval(model, atm, pb, obs, BLOCK)
    assert ret.destination == [('params', 0), ('params', 1)]
    assert np.all(ret.inside_host(theta))
    post = ret.log_posterior(eng.dev(theta))
    torch.cuda.synchronize()
    post = host(post)
    want = host(obs.loglike(host_flux_d)) + ret.log_prior_host(theta)
    bound = np.finfo(float).eps * np.abs(want) + \
        np.sum(np.abs(data - host_flux) / uncert**2 * 1e-8 * host_flux, axis=1)
    print('log-posterior device', post, 'host profiles', want, 'difference', post - want,
          'bound', bound)
    assert np.all(np.isfinite(post)) and np.all(post > -1e6)
    assert np.all(np.abs(post - want) <= bound)
    assert len(set(np.round(post, 6))) == 4


def test_radiative_equilibrium_with_ions_and_hminus(eng, ch):
    """RadiativeEquilibrium(chemistry=ion network) with an H- continuum, two iterations of case
    (p) of radeq_chemistry_cases.py from 2500 K: no chemistry failure, the VMRs it leaves are the
    host's equilibrium at its last temperatures (the bound of test_gpu_radeq_chemistry's
    trajectories), neutral, and the mean mass counts the electrons.  (The host loop of
    radeq_chemistry_cases.py is written for the 16-species network and a continuum without H-,
    so the temperatures have no host trajectory here.)"""
    import radeq_chemistry_cases as rq
    from pyratbay_amd import continuum as ct, radeq
    network, mass, b = ic.sixteen_with_ions(ch)
    c = rq.case('p')
    cont = ct.Continuum(c['wn'], c['pressure'], [ct.Hydrogen_Ion(c['wn'])])
    assert cont.species == ['H', 'e-']
    model = eng.TableSpectrum(c['etable'], c['ttable'], c['wn'], c['radius'], 1.0,
                              rt_path='emission_two_stream', continuum=cont, timestamps=False,
                              tint=float(c['tint'][0]))
    re = radeq.RadiativeEquilibrium(model, c['pressure'], None, mass, tint=float(c['tint'][0]),
                                    tmin=c['tmin'], tmax=c['tmax'],
                                    table_species=rq.TABLE_SPECIES, chemistry=network,
                                    metallicity=0.0, radius_model=None)
    temps = host(re.run(np.full(c['L'], 2500.0), 2, diagnostics=True))
    assert temps.shape == (1, 3, c['L']) and np.all(np.isfinite(temps))
    assert not host(re.chem_failures).any()
    assert np.all(host(re.history['chem_iterations']) > 0)
    assert np.any(temps[0, 2] != temps[0, 0])
    vmr = host(re.vmr)[0]
    want = network.equilibrium_host(temps[0, -1], c['pressure'], b)[0]
    seen = want >= 1e-250
    dev = np.max(np.abs(vmr[seen] / want[seen] - 1.0))
    neutral = ic.neutrality(network, vmr).max()
    merr = np.max(np.abs(host(re.mean_mass)[0] / (vmr @ mass) - 1.0))
    print(f'.vmr against the host at the last row {dev:.2e} (bound {WARM_BOUND:.0e}), neutrality '
          f'{neutral:.2e}, mean mass {merr:.2e}; solver iterations '
          f'{host(re.history["chem_iterations"])[0].tolist()}')
    assert dev <= WARM_BOUND and neutral <= 1e-11 and merr <= 1e-14
    assert np.all(vmr[:, network.species.index('e-')] > 0)
