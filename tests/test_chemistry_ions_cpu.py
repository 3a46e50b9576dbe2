"""Equilibrium chemistry with ions and electrons on the host (ChemNetwork(charges=...)): the Saha
closed form, the 28-point grid against the optimality conditions with the charge balance among
them, iteration counts that do not grow with the ionisation energy, ions that underflow, the
unchanged neutral network, the carried start, what is refused, and the continuum densities of a
WalkerAtmosphere on such a network.

Bounds.  Element ratios, mass action (on net.balance) and neutrality |sum q x| / sum |q| x: 1e-11
on the grid, the bounds of test_chemistry_cpu.py (measured here: 3.1e-14, 1.7e-13, 2.1e-14); a
solver whose convergence test does not see trace ions leaves the neutrality at 1.0.  Closed form:
1e-12 (measured 2.9e-14).  Warm against cold: test_radeq_chemistry_cpu's 2e-12 on every species
with a cold VMR >= 1e-250.  Every check prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import chemistry_cases as cc
import ion_cases as ic

WARM_BOUND = 2e-12
TEMPS = np.array([t for t, _ in cc.GRID])
PRESS = np.array([p for _, p in cc.GRID])
ENTHALPIES = (1.536e6, 9e6, 4e7)
COLD_T, COLD_P = np.array([300.0, 1000.0]), np.array([1.0, 1.0])


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
def grid_solution(net):
    """The 28 grid points solved once (with the iterate), shared and left unchanged."""
    vmr, iterations, status, iterate = net.equilibrium_host(TEMPS, PRESS, ic.B, start='cold')
    for a in (vmr, iterations, status) + iterate:
        a.setflags(write=False)
    return vmr, iterations, status, iterate


# -------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize('temp,pressure', [(3000.0, 1e-4), (6000.0, 1e-6), (6000.0, 1.0),
                                           (1000.0, 1.0)])
def test_saha_closed_form(ch, temp, pressure):
    saha = ic.saha_network(ch)
    assert (saha.nspecies, saha.nelements) == (3, 1)
    vmr, _, status = saha.equilibrium_host([temp], [pressure], np.array([1.0]))
    want = ic.saha_closed_form(temp, pressure)
    dev = max(abs(vmr[0, 1] / want - 1.0), abs(vmr[0, 2] / want - 1.0))
    print(f'x_H+ = x_e at {temp} K, {pressure} bar: {vmr[0, 1]:.16e}, {vmr[0, 2]:.16e} vs '
          f'{want:.16e}, rel {dev:.2e} (bound 1e-12)')
    assert status[0] > 0 and want > 0.0
    assert dev <= 1e-12
    assert abs(vmr[0, 0] / (1.0 - 2.0 * want) - 1.0) <= 1e-12


# ----------------------------------------------------------------------------------- the grid
def test_grid_converges_everywhere(ch, grid_solution):
    vmr, iterations, status, _ = grid_solution
    print('iterations per (T, p):\n', iterations.reshape(len(cc.GRID_T), len(cc.GRID_P)))
    assert len(TEMPS) == 28
    assert np.all(status > 0) and np.array_equal(status, iterations)
    assert iterations.max() < ch.MAX_ITERATIONS
    assert np.all(np.isfinite(vmr)) and np.all(np.abs(vmr.sum(axis=1) - 1.0) < 1e-14)


def test_grid_element_ratios_and_mass_action(net, grid_solution):
    vmr = grid_solution[0]
    err = ic.element_error(net, vmr, ic.B)
    res = [ic.mass_action_residual(net, vmr[i], TEMPS[i], PRESS[i]) for i in range(28)]
    print(f'element ratios vs b: max rel {err.max():.2e}; mass action on [stoich | charges]: max '
          f'{max(res):.2e} (bounds 1e-11); min VMR {vmr.min():.2e}')
    assert err.max() <= 1e-11
    assert max(res) <= 1e-11


def test_grid_is_neutral_in_every_cell(net, grid_solution):
    """What an implementation without the ions' own convergence rule misses: the weighted test
    passes with no neutrality at all (1.0) at 300-1000 K and >= 1 bar."""
    vmr = grid_solution[0]
    neutrality = ic.neutrality(net, vmr)
    print('neutrality per (T, p):\n', neutrality.reshape(len(cc.GRID_T), len(cc.GRID_P)),
          f'\nmax {neutrality.max():.2e} (bound 1e-11)')
    assert np.all(vmr[:, net.charges != 0] > 0)          # no ion underflows on this grid
    assert neutrality.max() <= 1e-11


def test_cells_are_independent(net, grid_solution):
    vmr, iterations = grid_solution[:2]
    for i in (0, 10, 27):
        v, it, _ = net.equilibrium_host(TEMPS[i:i + 1], PRESS[i:i + 1], ic.B)
        assert np.array_equal(v[0], vmr[i]) and it[0] == iterations[i]


# ------------------------------------------------------------------- the ionisation energy
def test_iterations_do_not_grow_with_the_ionisation_energy(ch):
    """The cations' enthalpy at 1.5, 9 and 40 MJ/mol, at 300 K and 1000 K: from the cold start
    alone the count would grow like dG / (2 R T) (hundreds to thousands).  At 9 MJ/mol and 300 K
    and at 40 MJ/mol every cation underflows; the anions H- and e- do with them."""
    sub = ic.neutral_subnetwork(ch)
    sub_vmr, sub_iterations, sub_status = sub.equilibrium_host(COLD_T, COLD_P, ic.B)
    assert np.all(sub_status > 0)
    neutral = ic.CHARGES == 0
    for h in ENTHALPIES:
        net = ic.network(ch, h)
        vmr, iterations, status = net.equilibrium_host(COLD_T, COLD_P, ic.B)
        g, lnp = net.gibbs_at(COLD_T), np.log(COLD_P)
        first = net._iterate(net.stoich[neutral].astype(float), ic.B, g[:, neutral], lnp,
                             ch.TOLERANCE, np.full((2, 9), np.log(0.1 / 9)),
                             np.full(2, np.log(0.1)))[2]
        print(f'h = {h:g} J/mol: iterations {iterations} (neutral step {first}), ions\n',
              vmr[:, ~neutral])
        assert np.all(status > 0) and np.array_equal(status, iterations)
        assert np.array_equal(first, sub_iterations)
        assert np.all((iterations > first) & (iterations < ch.MAX_ITERATIONS))
        assert np.all(iterations - first <= 3)
        assert np.all(np.isfinite(vmr)) and np.all(vmr >= 0)
        dev = np.max(np.abs(vmr[:, neutral] / sub_vmr - 1.0))
        print(f'  neutral species against the neutral sub-network: {dev:.2e} (bound 1e-12)')
        assert dev <= 1e-12
        assert ic.neutrality(net, vmr).max() <= 1e-11
        underflow = vmr[:, ic.CATIONS].max(axis=1) == 0.0
        assert list(underflow) == {1.536e6: [False, False], 9e6: [True, False],
                                   4e7: [True, True]}[h]
        assert np.all(vmr[underflow][:, ~neutral] == 0.0)


# ------------------------------------------------------------------ the neutral network stays
def test_zero_or_absent_charges_are_the_neutral_network(ch):
    plain = cc.network(ch)
    want = plain.equilibrium_host(cc_temps(), cc_press(), cc.B)
    args = (cc.SPECIES, cc.ELEMENTS, cc.STOICH, cc.TABLE_T, cc.gibbs(cc.TABLE_T), cc.BASE_DEX)
    for charges in (None, np.zeros(16, int)):
        net = ch.ChemNetwork(*args, charges=charges)
        assert not net.charged and net.balance.shape == (16, 6)
        assert np.array_equal(net.balance[:, :5], cc.STOICH) and not net.balance[:, 5].any()
        got = net.equilibrium_host(cc_temps(), cc_press(), cc.B)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    assert plain.charges is None
    # and the refusals of a network without charges hold with zeros
    with pytest.raises(ValueError, match='ions and electrons'):
        ch.ChemNetwork(cc.SPECIES[:-1] + ['H+'], *args[1:], charges=np.zeros(16, int))


def cc_temps():
    return np.array([t for t, _ in cc.GRID])


def cc_press():
    return np.array([p for _, p in cc.GRID])


def test_inert_trace_ions_leave_the_neutral_species(ch):
    """The 16 species with H+, H- and e- added, about 1e-16 of the gas at 1000 K and 1 bar: the
    neutral VMRs are those of the 16-species network to 1e-12 (they are diluted by the ions'
    1e-16, and solved from another cold start)."""
    trace = ic.sixteen_with_trace_ions(ch)
    v, _, s = trace.equilibrium_host([1000.0], [1.0], cc.B)
    plain, _, t = cc.network(ch).equilibrium_host([1000.0], [1.0], cc.B)
    dev = np.max(np.abs(v[0, :16] / plain[0] - 1.0))
    print(f'ions {v[0, 16:]}, neutrality {ic.neutrality(trace, v)[0]:.2e}; neutral species '
          f'with and without them: {dev:.2e} (bound 1e-12)')
    assert s[0] > 0 and t[0] > 0
    assert np.all(v[0, 16:] > 0) and 1e-17 < v[0, 16:].max() < 1e-15
    assert ic.neutrality(trace, v)[0] <= 1e-11
    assert dev <= 1e-12


# ------------------------------------------------------------------------------ carried start
def test_carried_start(ch, net, grid_solution):
    """From the solution at T, solved at T +- 25 K: the cold solve's VMRs, neutral, in few
    iterations; a NaN in the iterate and the cell has the cold result's bits."""
    _, _, _, iterate = grid_solution
    for shift in (25.0, -25.0):
        temps = TEMPS + np.where(TEMPS + shift > 6500.0, -shift, shift)
        cold = net.equilibrium_host(temps, PRESS, ic.B, start='cold')
        warm = net.equilibrium_host(temps, PRESS, ic.B, start=iterate)
        assert np.all(cold[2] > 0) and np.all(warm[2] > 0)
        seen = cold[0] >= 1e-250
        dev = np.max(np.abs(warm[0][seen] / cold[0][seen] - 1.0))
        neutrality = ic.neutrality(net, warm[0]).max()
        print(f'dT = {shift:+g} K: warm against cold {dev:.2e} (bound {WARM_BOUND:.0e}), '
              f'neutrality {neutrality:.2e}, iterations warm {warm[1].min()}-{warm[1].max()}, '
              f'cold {cold[1].min()}-{cold[1].max()}')
        assert dev <= WARM_BOUND and neutrality <= 1e-11
        assert np.all(warm[1] <= cold[1])
        # the warm Newton iteration itself converged: no cell fell back to the cold solve
        ok = net._newton(net.gibbs_at(temps), np.log(PRESS), ic.B, ch.TOLERANCE, iterate,
                         ch.TOL_ALL)[2]
        assert ok.all()
    ln_ni, ln_n = iterate[0].copy(), iterate[1].copy()
    ln_ni[3, 11], ln_n[9] = np.nan, np.nan
    got = net.equilibrium_host(temps, PRESS, ic.B, start=(ln_ni, ln_n))
    for k in (3, 9):
        assert np.array_equal(got[0][k], cold[0][k]) and got[2][k] == cold[2][k]
        assert np.array_equal(got[3][0][k], cold[3][0][k]) and got[3][1][k] == cold[3][1][k]
    others = np.setdiff1d(np.arange(28), [3, 9])
    assert np.array_equal(got[0][others], warm[0][others])


def test_each_step_has_its_own_cap(ch, net):
    """MAX_ITERATIONS caps the neutral step and the full system each: with room for the first
    alone the cell converges with a status above the cap; without, STATUS_NOT_CONVERGED, zeros."""
    full = net.equilibrium_host([1000.0], [1.0], ic.B)[1][0]
    first = ic.neutral_subnetwork(ch).equilibrium_host([1000.0], [1.0], ic.B)[1][0]
    assert first < full <= 2 * first
    saved = ch.MAX_ITERATIONS
    try:
        ch.MAX_ITERATIONS = 2
        vmr, iterations, status = net.equilibrium_host([1000.0], [1.0], ic.B)
        assert status[0] == ch.STATUS_NOT_CONVERGED and iterations[0] == 2 and np.all(vmr == 0)
        ch.MAX_ITERATIONS = first
        vmr, iterations, status = net.equilibrium_host([1000.0], [1.0], ic.B)
        assert status[0] == full and iterations[0] == full and np.all(vmr > 0)
    finally:
        ch.MAX_ITERATIONS = saved


# ----------------------------------------------------------------------------------- refusals
def test_network_refusals_with_charges(ch):
    T = cc.TABLE_T
    g = cc.gibbs(T, ic.H_FORM.astype(float), ic.S_ENT)

    def make(species=ic.SPECIES, elements=ic.ELEMENTS, stoich=ic.STOICH, table=g,
             dex=ic.BASE_DEX, charges=ic.CHARGES):
        return ch.ChemNetwork(species, elements, stoich, T, table, dex, charges=charges)
    net = make()
    assert net.charged and net.charges.dtype == np.int32 and net.balance.shape == (14, 6)
    assert np.array_equal(net.balance[:, :5], net.stoich)
    assert np.array_equal(net.balance[:, 5], ic.CHARGES) and net.stoich.shape == (14, 5)
    # without charges= the names are refused as before, and the charge never enters stoich
    with pytest.raises(ValueError, match='ions and electrons'):
        make(charges=None)
    stoich = ic.STOICH.copy()
    stoich[11, 0] = -1
    with pytest.raises(ValueError, match='non-negative integers'):
        make(stoich=stoich)
    with pytest.raises(ValueError, match='ions and electrons'):
        make(elements=ic.ELEMENTS[:-1] + ['e-'])
    with pytest.raises(ValueError, match='charges must hold 14 integers'):
        make(charges=ic.CHARGES[:-1])
    with pytest.raises(ValueError, match='charges must hold 14 integers'):
        make(charges=ic.CHARGES + 0.5)
    # a species must hold an element or a charge
    charges = ic.CHARGES.copy()
    charges[11] = 0
    with pytest.raises(ValueError, match="species 'e-' holds no element and no charge"):
        make(charges=charges)
    # charged species of both signs
    with pytest.raises(ValueError, match='both signs'):
        make(charges=np.abs(ic.CHARGES))
    # every element in a neutral species: K only as K+ ...
    keep = [i for i in range(14) if ic.SPECIES[i] != 'K']
    with pytest.raises(ValueError, match="element 'K' is in no neutral species"):
        make(species=[ic.SPECIES[i] for i in keep], stoich=ic.STOICH[keep], table=g[:, keep],
             charges=ic.CHARGES[keep])
    # ... the neutral sub-network of rank E: H and O neutral only as H2O and H4O2
    with pytest.raises(ValueError, match='neutral species has rank 1 < 2'):
        ch.ChemNetwork(['H2O', 'H4O2', 'H+', 'e-'], ['H', 'O'], [[2, 1], [4, 2], [1, 0], [0, 0]],
                       T, g[:, :4], [12.0, 8.5], charges=[0, 0, 1, -1])
    # ... [stoich | charges] of rank E + 1: every H carries +1, every O -2, H2O is the one neutral
    with pytest.raises(ValueError, match=r'\[stoich \| charges\] has rank 2 < 2 elements \+ 1'):
        ch.ChemNetwork(['H2O', 'H+', 'O--'], ['H', 'O'], [[2, 1], [1, 0], [0, 1]], T, g[:, :3],
                       [12.0, 8.5], charges=[0, 1, -2])
    # the charge balance takes one of the eight rows
    names = ['H'] + list('ABCDFGI')
    with pytest.raises(ValueError, match='8 elements with charges'):
        ch.ChemNetwork(names + ['H+', 'e-'], names, np.vstack([np.eye(8, dtype=int),
                       [[1] + [0] * 7, [0] * 8]]), T, np.zeros((len(T), 10)), np.full(8, 12.0),
                       charges=[0] * 8 + [1, -1])
    seven = names[:7]
    ch.ChemNetwork(seven + ['H+', 'e-'], seven, np.vstack([np.eye(7, dtype=int),
                   [[1] + [0] * 6, [0] * 7]]), T, np.zeros((len(T), 9)), np.full(7, 12.0),
                   charges=[0] * 7 + [1, -1])


def test_hybrid_on_a_charged_species_is_refused(ch, pa, net, grid_solution):
    with pytest.raises(ValueError, match="hybrid model on 'e-'"):
        net.hybrid_host(grid_solution[0], 'e-', -8.0)
    with pytest.raises(ValueError, match="hybrid model on 'Na\\+'"):
        net.model_struct(4, 2, hybrids=[(net.species.index('Na+'), 1)])
    net.model_struct(4, 2, hybrids=[(net.species.index('Na'), 1)])
    # the cap of a neutral species goes over the elements only
    k = net.species.index('H2O')
    cap = np.minimum((grid_solution[0] @ net.stoich[:, 0]) / 2.0, grid_solution[0] @ net.stoich[:, 2])
    assert np.allclose(net.hybrid_host(grid_solution[0], 'H2O', -1.0), cap, rtol=1e-15, atol=0)
    assert k == 3
    pressure = np.logspace(-6, 1, 5)
    kw = dict(mplanet=1.5e30, rplanet=7.0e9, refpressure=0.1,
              base_radius=np.linspace(8e9, 7e9, 5), chemistry=net)
    pa.WalkerAtmosphere(pressure, ic.SPECIES, ic.MASS, None, None, pa.Isothermal(pressure),
                        [pa.MetalEquil(), pa.IsoVMR('Na', pressure)], **kw)
    with pytest.raises(ValueError, match="hybrid model on 'H-'"):
        pa.WalkerAtmosphere(pressure, ic.SPECIES, ic.MASS, None, None, pa.Isothermal(pressure),
                            [pa.MetalEquil(), pa.IsoVMR('H-', pressure)], **kw)
    with pytest.raises(ValueError, match="species must be the network's"):
        pa.WalkerAtmosphere(pressure, ic.SPECIES[::-1], ic.MASS, None, None,
                            pa.Isothermal(pressure), [pa.MetalEquil()], **kw)


def test_struct_check_with_charges(ch, net):
    """pb_chem_model's new last field, and pb_equilibrium_vmr's check of it before any HIP call
    (nwalkers = 0; the pointers are never dereferenced)."""
    from pyratbay_amd import _capi
    lib = _capi.lib()
    name, ctype = ch.ChemModelStruct._fields_[-1]
    assert name == 'charge_d' and ctype is C.c_void_p

    def filled(network):
        st = network.model_struct(4, 3, par_metal=0)
        for field, kind in ch.ChemModelStruct._fields_:
            if kind is C.c_void_p:
                setattr(st, field, 4096)
        return st
    st = filled(net)
    assert (st.nelements, st.nspecies) == (5, 14)
    assert lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None) == 0
    big = cc.padded_network(ch, 32)
    assert big.nelements == 8
    st = filled(big)
    assert lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None) == -1
    assert '8 elements with charges' in lib.pb_last_error().decode(), lib.pb_last_error()
    st.charge_d = None
    assert lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None) == 0
    st = filled(big)
    st.nelements = 9
    assert lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None) == -1
    assert '1-8 elements, not 9' in lib.pb_last_error().decode()
    seven = filled(ic.padded_network(ch)[0])
    assert (seven.nelements, seven.nspecies) == (7, 32)
    assert lib.pb_equilibrium_vmr(C.byref(seven), 4096, 4096, 0, 4096, 4096, None) == 0


# --------------------------------------------------------------------------- through the class
def test_walker_atmosphere_gives_the_continuum_its_electrons(pa, ch, net):
    """evaluate_host on the ion network, bound to a continuum with H- (species H and e-, found by
    name): its two density columns are vmr x the ideal-gas density of the layer."""
    from pyratbay_amd import continuum as ct
    pressure = np.logspace(-6, 1, 5)

    class Cont:
        species, alkali_species = ['H', 'e-'], []
    atm = pa.WalkerAtmosphere(pressure, ic.SPECIES, ic.MASS, None, None, pa.Isothermal(pressure),
                              [pa.MetalEquil()], rmodel='hydro_m', mplanet=1.5e30,
                              rplanet=7.0e9, refpressure=0.1, base_params=[2500.0, 0.0],
                              chemistry=net)
    atm.bind(['H2O'], Cont())
    for params in ([2500.0, 0.0], [3200.0, 0.5]):
        prof = atm.evaluate_host(params)
        assert prof.reject == 0 and prof.continuum_density.shape == (5, 2)
        b = net.element_abundances_host(params[1])
        vmr, _, status = net.equilibrium_host(np.full(5, params[0]), pressure, b)
        assert np.all(status > 0)
        dens = pa.ideal_gas_density(vmr, pressure, np.full(5, params[0]))
        for col, name in enumerate(('H', 'e-')):
            assert np.array_equal(prof.continuum_density[:, col],
                                  dens[:, ic.SPECIES.index(name)]), name
        assert np.all(prof.continuum_density > 0)
        mm = vmr @ ic.MASS
        assert np.max(np.abs(prof.mm / mm - 1.0)) <= 1e-15
    # more metals, more electrons (Na and K give them at this temperature)
    rich = atm.evaluate_host([2500.0, 1.0])
    poor = atm.evaluate_host([2500.0, 0.0])
    assert np.all(rich.continuum_density[:, 1] > poor.continuum_density[:, 1])
