"""Equilibrium chemistry on the host: the abundance rule, the solver against solver-independent
optimality conditions and closed forms, its status paths, the hybrid cap, and what
WalkerAtmosphere(chemistry=net) takes and refuses.

Bounds: the element ratios and the mass-action residual to 1e-11 on the 28-point grid, 40-300 times
what the NumPy solver leaves there (2.9e-14 and 2.6e-13): the margin is for exp and log of other
bits; a solver that stops early or balances the wrong element misses by many orders.  Closed forms
to 1e-12.  Every check prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import chemistry_cases as cc


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
    return cc.network(ch)


@pytest.fixture(scope='module')
def grid_solution(net):
    """The 28 grid points solved once, shared and left unchanged."""
    temps = np.array([t for t, _ in cc.GRID])
    press = np.array([p for _, p in cc.GRID])
    vmr, iterations, status = net.equilibrium_host(temps, press, cc.B)
    for a in (vmr, iterations, status):
        a.setflags(write=False)
    return temps, press, vmr, iterations, status


# ------------------------------------------------------------------------------ abundance rule
def test_abundance_rule_steps_and_order(net):
    H, He, Cc, N, O = (net.elements.index(e) for e in ('H', 'He', 'C', 'N', 'O'))
    base = net.base_dex
    # 1 and 5: base_dex alone, relative to H
    b = net.element_abundances_host()
    assert np.allclose(b, cc.B, rtol=1e-14) and b[H] == 1.0
    # 2: every element but H and He
    b = net.element_abundances_host(metallicity=1.0)
    assert b[H] == 1.0 and b[He] == 10.0**(base[He] - base[H])
    for j in (Cc, N, O):
        assert b[j] == 10.0**((base[j] + 1.0) - base[H])
    # 3: [X/H] overrides the metallicity for X
    b = net.element_abundances_host(metallicity=1.0, e_scale={'C': -0.5})
    assert b[Cc] == 10.0**((base[Cc] - 0.5) - base[H])
    assert b[O] == 10.0**((base[O] + 1.0) - base[H])
    # 4: X/Y after both: carbon ends at dex[O] + log10(0.6), O carries the metallicity
    b = net.element_abundances_host(metallicity=1.0, e_scale={'C': -0.5}, e_ratio={'C/O': 0.6})
    dex_o = base[O] + 1.0
    assert b[O] == 10.0**(dex_o - base[H])
    assert b[Cc] == 10.0**((dex_o + np.log10(0.6)) - base[H])
    assert abs(b[Cc] / b[O] - 0.6) < 1e-15
    # the reference's key for a ratio, and model order: N/C reads the carbon C/O has just set
    b = net.element_abundances_host(e_ratio={'C_O': 0.6, 'N/C': 2.0})
    assert abs(b[N] / b[Cc] - 2.0) < 1e-15 and abs(b[Cc] / b[O] - 0.6) < 1e-15
    b = net.element_abundances_host(e_ratio={'N/C': 2.0, 'C/O': 0.6})
    assert abs(b[N] / 10.0**(base[Cc] - base[H]) - 2.0) < 1e-15
    # a ratio <= 0 rejects the walker
    for bad in (0.0, -0.3, float('nan')):
        assert net.element_abundances_host(e_ratio={'C/O': bad}) is None
    with pytest.raises(ValueError, match="'Na' is not in the network"):
        net.element_abundances_host(e_scale={'Na': 0.1})


# --------------------------------------------------------------------------------- optimality
def test_grid_converges_everywhere(ch, grid_solution):
    temps, press, vmr, iterations, status = grid_solution
    print('iterations per (T, p):\n', iterations.reshape(len(cc.GRID_T), len(cc.GRID_P)))
    assert len(temps) == 28
    assert np.all(status > 0) and np.array_equal(status, iterations)
    assert iterations.max() < ch.MAX_ITERATIONS
    assert np.all(vmr > 0) and np.all(np.abs(vmr.sum(axis=1) - 1.0) < 1e-14)


def test_grid_element_ratios(net, grid_solution):
    _, _, vmr, _, _ = grid_solution
    err = cc.element_error(net, vmr, cc.B)
    print(f'element ratios vs b: max rel {err.max():.2e} (bound 1e-11)')
    assert err.max() <= 1e-11


def test_grid_mass_action(net, grid_solution):
    temps, press, vmr, _, _ = grid_solution
    res = [cc.mass_action_residual(net, vmr[i], temps[i], press[i]) for i in range(len(temps))]
    print(f'mass-action residual: max {max(res):.2e} (bound 1e-11); min VMR {vmr.min():.2e}')
    assert max(res) <= 1e-11


def test_cells_are_independent(net, grid_solution):
    """A cell depends on nothing but its own inputs: solved alone it has the same bits."""
    temps, press, vmr, iterations, _ = grid_solution
    for i in (0, 13, 27):
        v, it, _ = net.equilibrium_host(temps[i:i + 1], press[i:i + 1], cc.B)
        assert np.array_equal(v[0], vmr[i]) and it[0] == iterations[i]


# -------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize('temp,pressure', [(2000.0, 1e-3), (4000.0, 1.0)])
def test_hydrogen_dissociation(ch, temp, pressure):
    hyd = cc.hydrogen_network(ch)
    vmr, _, status = hyd.equilibrium_host([temp], [pressure], np.array([1.0]))
    want = cc.hydrogen_closed_form(temp, pressure)
    dev = abs(vmr[0, 1] / want - 1.0)
    print(f'x_H at {temp} K, {pressure} bar: {vmr[0, 1]:.16e} vs {want:.16e}, rel {dev:.2e}')
    assert status[0] > 0 and dev <= 1e-12
    assert abs(vmr[0, 0] / (1.0 - want) - 1.0) <= 1e-12


def test_one_species_network(ch):
    one = ch.ChemNetwork(['H2'], ['H'], [[2]], cc.TABLE_T, cc.gibbs(cc.TABLE_T)[:, :1], [12.0])
    vmr, _, status = one.equilibrium_host([1000.0, 300.0], [1.0, 1e-6], np.array([1.0]))
    assert np.all(status > 0) and np.array_equal(vmr, np.ones((2, 1)))


def test_inert_helium_changes_no_ratio(ch):
    with_he, without = cc.hydrogen_network(ch, True), cc.hydrogen_network(ch)
    for temp, pressure in ((2000.0, 1e-3), (4000.0, 1.0)):
        # He dilutes: the same partial pressure of hydrogen species means the same H : H2
        v, _, s = with_he.equilibrium_host([temp], [pressure], np.array([1.0, 0.085]))
        assert s[0] > 0
        p_hydrogen = pressure * (v[0, 0] + v[0, 1])
        u, _, _ = without.equilibrium_host([temp], [p_hydrogen], np.array([1.0]))
        dev = abs((v[0, 1] / v[0, 0]) / (u[0, 1] / u[0, 0]) - 1.0)
        print(f'H : H2 with and without He at {temp} K: rel {dev:.2e}')
        assert dev <= 1e-12
        # and the He : H element ratio is b's
        assert abs(v[0, 2] / (2.0 * v[0, 0] + v[0, 1]) / 0.085 - 1.0) <= 1e-12


# -------------------------------------------------------------------------------- status paths
def test_status_paths(ch, net):
    temps = np.array([1000.0, 100.0, 7000.0, 0.0, -5.0, float('nan'), float('inf')])
    vmr, iterations, status = net.equilibrium_host(temps, np.full(7, 1.0), cc.B)
    assert status[0] > 0 and status[0] == iterations[0]
    assert list(status[1:]) == [ch.STATUS_TEMPERATURE, ch.STATUS_TEMPERATURE, ch.STATUS_REJECTED,
                                ch.STATUS_REJECTED, ch.STATUS_REJECTED, ch.STATUS_TEMPERATURE]
    assert np.all(vmr[1:] == 0) and np.all(iterations[1:] == 0)
    # a bad ratio: every cell of the walker, but for those rejected before
    vmr, _, status = net.equilibrium_host(temps[[0, 3]], [1.0, 1.0], None)
    assert list(status) == [ch.STATUS_RATIO, ch.STATUS_REJECTED] and np.all(vmr == 0)
    # not converged: the same cell with room for two iterations only
    saved = ch.MAX_ITERATIONS
    try:
        ch.MAX_ITERATIONS = 2
        vmr, iterations, status = net.equilibrium_host([1000.0], [1.0], cc.B)
    finally:
        ch.MAX_ITERATIONS = saved
    assert status[0] == ch.STATUS_NOT_CONVERGED and iterations[0] == 2 and np.all(vmr == 0)


def test_network_refusals(ch):
    T, g = cc.TABLE_T, cc.gibbs(cc.TABLE_T)

    def make(species=cc.SPECIES, elements=cc.ELEMENTS, stoich=cc.STOICH, temps=T, table=g,
             dex=cc.BASE_DEX):
        return ch.ChemNetwork(species, elements, stoich, temps, table, dex)
    make()
    with pytest.raises(ValueError, match='rank 1 < 2'):      # H and O only ever come as 2 : 1
        ch.ChemNetwork(['H2O', 'H4O2'], ['H', 'O'], [[2, 1], [4, 2]], T, g[:, :2], [12.0, 8.5])
    with pytest.raises(ValueError, match="no 'H' among"):
        ch.ChemNetwork(['CO', 'O'], ['C', 'O'], [[1, 1], [0, 1]], T, g[:, :2], [8.0, 8.5])
    with pytest.raises(ValueError, match='rank 2 < 3'):
        ch.ChemNetwork(['H2', 'CO', 'H'], ['H', 'C', 'O'], [[2, 0, 0], [0, 1, 1], [1, 0, 0]], T,
                       g[:, :3], [12.0, 8.0, 8.5])
    stoich = cc.STOICH.copy()
    stoich[:, 1] = 0
    with pytest.raises(ValueError, match="element 'He' is in no species"):
        make(stoich=np.where(np.arange(16)[:, None] == 2, [[1, 0, 0, 0, 0]], stoich))
    stoich = cc.STOICH.copy()
    stoich[15] = 0
    with pytest.raises(ValueError, match="species 'O2' holds no element"):
        make(stoich=stoich)
    with pytest.raises(ValueError, match='ions and electrons'):
        make(species=cc.SPECIES[:-1] + ['H+'])
    with pytest.raises(ValueError, match='ions and electrons'):
        make(elements=cc.ELEMENTS[:-1] + ['e-'])
    stoich = cc.STOICH.copy()
    stoich[1, 0] = -1
    with pytest.raises(ValueError, match='non-negative integers'):
        make(stoich=stoich)
    bad = g.copy()
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match='must be finite'):
        make(table=bad)
    with pytest.raises(ValueError, match='ascending'):
        make(temps=T[::-1])
    too_many = cc.padded_network(ch, 32)
    with pytest.raises(ValueError, match='1 ... 32 distinct names'):
        cc.padded_network(ch, 33)
    assert too_many.nspecies == 32 and too_many.nelements == 8
    with pytest.raises(ValueError, match='1 ... 8 distinct names'):
        ch.ChemNetwork(['H'] + list('ABCDEFGI'), ['H'] + list('ABCDEFGI'), np.eye(9, dtype=int),
                       T, np.zeros((len(T), 9)), np.full(9, 12.0))


# -------------------------------------------------------------------------------------- hybrid
def test_hybrid_cap(net, grid_solution):
    temps, press, vmr, _, _ = grid_solution
    k = net.species.index('H2O')
    a = net.stoich.astype(float)
    # the cap, layer by layer: H2O cannot hold more O than the mixture has, nor more H than half
    cap = np.minimum((vmr @ a[:, 0]) / 2.0, vmr @ a[:, 4])
    assert np.all(cap < 1e-3) and np.all(cap > 1e-4)
    below = net.hybrid_host(vmr, 'H2O', -6.0)
    assert np.array_equal(below, np.full(len(temps), 10.0**-6.0))
    above = net.hybrid_host(vmr, 'H2O', -1.0)
    assert np.allclose(above, cap, rtol=1e-15, atol=0) and np.all(above < 0.1)
    assert k == 3


def test_hybrid_through_the_class(pa, ch, net):
    atm, base = cc.chem_atmosphere(pa, net)
    ih2o = atm.species.index('H2O')
    free = cc.chem_atmosphere(pa, net, hybrid=False)[0]
    equil = free._chain(base[:3])['vmr']
    low = atm._chain(np.append(base[:3], -7.0))
    assert low['reject'] == 0
    assert np.array_equal(low['vmr'][:, ih2o], np.full(atm.nlayers, 10.0**-7.0))
    others = [i for i in range(atm.nspecies) if i != ih2o]
    assert np.array_equal(low['vmr'][:, others], equil[:, others])      # nothing renormalised
    high = atm._chain(np.append(base[:3], -1.0))
    assert high['reject'] == 0                   # the reference's out-of-bounds flag is inert
    assert np.array_equal(high['vmr'][:, ih2o], net.hybrid_host(equil, 'H2O', -1.0))
    assert np.array_equal(high['vmr'][:, others], equil[:, others])


# ------------------------------------------------------------------------------ through the class
def test_walker_atmosphere_takes_equilibrium_models(pa, ch, net):
    """(On the parent commit a MetalEquil in vmr_models is a ValueError.)"""
    atm, base = cc.chem_atmosphere(pa, net)
    assert atm.free == ['T_iso', '[M/H]', 'C/O', 'log_H2O']
    models = atm.vmr_models
    assert [m.name for m in models] == ['metal_equil', 'ratio_equil', 'log_H2O']
    assert [m.type for m in models] == ['equil', 'equil', 'free']
    scale = pa.ScaleEquil('[C/H]')
    assert (scale.name, scale.pnames, scale.element, scale.type) == \
        ('scale_equil', ['[C/H]'], 'C', 'equil')
    assert models[1].elements == ['C', 'O'] and models[1].element_ratio == 'C_O'
    atm.bind(['H2O', 'CO', 'CH4'])
    prof = atm.evaluate_host(base)
    assert prof.reject == 0 and prof.dens.shape == (atm.nlayers, 3)
    assert np.all(prof.dens > 0) and np.all(np.diff(prof.radius) < 0)
    # metallicity moves the mean molecular mass; C/O <= 0 and a temperature outside the table
    # reject under the chemistry bit alone
    rich = atm.evaluate_host(base + [0, 1.0, 0, 0])
    assert rich.reject == 0 and np.all(rich.mm > prof.mm)
    for change in ([0, 0, -1.0, 0], [5500.0, 0, 0, 0]):
        r = atm.evaluate_host(base + change)
        assert r.reject == pa.REJECT_CHEMISTRY, r.reject
        assert np.all(r.temps == 0) and np.array_equal(r.radius, atm.base_radius)
    assert atm.evaluate_host(base * [0, 1, 1, 1]).reject == pa.REJECT_TEMP
    assert pa.REJECT_CHEMISTRY in pa.REJECT_NAMES and pa.REJECT_CHEMISTRY != pa.REJECT_ISOTOPE


def test_walker_atmosphere_refusals(pa, ch, net):
    L = 5
    pressure = np.logspace(-6, 1, L)
    kw = dict(mplanet=1.5e30, rplanet=7.0e9, refpressure=0.1,
              base_radius=np.linspace(8e9, 7e9, L), chemistry=net)
    tmodel = pa.Isothermal(pressure)
    pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel, [pa.MetalEquil()], **kw)
    with pytest.raises(ValueError, match='base_vmr and bulk are not taken'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, ['H2'], tmodel,
                            [pa.MetalEquil()], **kw)
    with pytest.raises(ValueError, match='base_vmr and bulk are not taken'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, np.full((L, 16), 1 / 16), None, tmodel,
                            [pa.MetalEquil()], **kw)
    with pytest.raises(ValueError, match='hard-wired to IsoVMR'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                            [pa.ScaleVMR('H2O', pressure, np.full(L, 1e-4))], **kw)
    with pytest.raises(ValueError, match='hard-wired to IsoVMR'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                            [pa.SlantVMR('H2O', pressure)], **kw)
    with pytest.raises(ValueError, match="species must be the network's"):
        pa.WalkerAtmosphere(pressure, cc.SPECIES[::-1], cc.MASS, None, None, tmodel,
                            [pa.MetalEquil()], **kw)
    with pytest.raises(ValueError, match="element 'Na' is not in the network"):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                            [pa.ScaleEquil('[Na/H]')], **kw)
    with pytest.raises(ValueError, match='named twice'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                            [pa.MetalEquil(), pa.MetalEquil()], **kw)
    # without a network the equilibrium models stay refused
    kw.pop('chemistry')
    with pytest.raises(ValueError, match='not supported'):
        pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, np.full((L, 16), 1 / 16), ['H2'],
                            tmodel, [pa.MetalEquil()], **kw)


def test_struct_mirror_and_check_before_hip(pa, ch, net):
    """ChemModelStruct mirrors pb_chem_model and AtmModelStruct's new field sits in what was
    padding; pb_equilibrium_vmr checks its struct before any HIP call (GPU or not: the pointers
    below are never dereferenced)."""
    from pyratbay_amd import _capi
    lib = _capi.lib()
    for name in ('pb_equilibrium_vmr', 'pb_walker_temperature', 'pb_walker_atmosphere_chem'):
        assert name in _capi.exported_names()
    assert C.sizeof(pa.AtmModelStruct) == 456 and pa.AtmModelStruct.base_vmr_stride.offset == 348

    def filled(**columns):
        st = net.model_struct(4, 3, **columns)
        for name, ctype in ch.ChemModelStruct._fields_:
            if ctype is C.c_void_p:
                setattr(st, name, 4096)
        return st

    def check(st, text):
        rc = lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None)
        assert rc == -1, (text, rc)
        assert text in lib.pb_last_error().decode(), lib.pb_last_error()
    st = filled(par_metal=0, scales=[(2, 1)], ratios=[(2, 4, 2)], hybrids=[(3, 1)])
    assert lib.pb_equilibrium_vmr(C.byref(st), 4096, 4096, 0, 4096, 4096, None) == 0
    st.nspecies = 65
    check(st, '1-64 species, not 65')
    st = filled()
    st.nelements = 9
    check(st, '1-8 elements, not 9')
    st = filled(par_metal=3)
    check(st, '[M/H] in column 3 of 3')
    st = filled(ratios=[(2, 5, 0)])
    check(st, 'X/Y 0: elements 2 and 5 of 5')
    st = filled(hybrids=[(3, 0), (16, 1)])
    check(st, 'hybrid model 1: species 16 of 16')
    st = filled()
    st.tolerance = 0.0
    check(st, 'tolerance 0')
    st = filled()
    st.pressure_d = None
    check(st, 'null model array')


def test_refusal_messages_are_stable(pa, ch, net):
    """The chemistry twin of test_atmosphere_cpu's table: one bad constructor argument per row
    and the whole message, compared with == (a parameter named twice is met before a species
    taken twice; the model count before either).  The messages are those of the commit before
    atmosphere.py was split."""
    L = 5
    p = np.logspace(-6, 1, L)
    only = ('with chemistry, only MetalEquil, ScaleEquil, RatioEquil and (hybrid) IsoVMR models '
            "are taken; the reference's hybrid is hard-wired to IsoVMR")
    not_taken = ('chemistry: base_vmr and bulk are not taken (pass None): the equilibrium gives '
                 'every VMR, and the reference balances no bulk in equilibrium')
    good = dict(pressure=p, species=cc.SPECIES, mol_mass=cc.MASS, base_vmr=None, bulk=None,
                tmodel=pa.Isothermal(p), vmr_models=[pa.MetalEquil(), pa.IsoVMR('H2O', p)],
                mplanet=1.5e30, rplanet=7.0e9, refpressure=0.1,
                base_radius=np.linspace(8e9, 7e9, L), chemistry=net)
    pa.WalkerAtmosphere(**good)
    rows = [
        (dict(species=cc.SPECIES[::-1]),
         f"chemistry: species must be the network's {cc.SPECIES}, got {cc.SPECIES[::-1]}"),
        (dict(base_vmr=np.full((L, 16), 1 / 16)), not_taken),
        (dict(bulk=['H2']), not_taken),
        (dict(qcap=0.9), 'chemistry: qcap is not taken (there are no bulk species)'),
        (dict(vmr_models=[pa.ScaleVMR('H2O', p, np.full(L, 1e-4))]),
         'VMR model scale_H2O: ' + only),
        (dict(vmr_models=[pa.SlantVMR('H2O', p)]), 'VMR model slant_H2O: ' + only),
        (dict(vmr_models=[pa.ScaleEquil('[H/H]')]),
         'ScaleEquil: [H/H] is no parameter (abundances are relative to hydrogen)'),
        (dict(vmr_models=[pa.ScaleEquil('[Na/H]')]),
         "element 'Na' is not in the network (['H', 'He', 'C', 'N', 'O'])"),
        (dict(vmr_models=[pa.RatioEquil('C/Na')]),
         "element 'Na' is not in the network (['H', 'He', 'C', 'N', 'O'])"),
        (dict(vmr_models=[pa.MetalEquil(), pa.MetalEquil()]),
         "VMR models: a parameter is named twice (['[M/H]', '[M/H]'])"),
        (dict(vmr_models=[pa.IsoVMR('H2O', p), pa.MetalEquil(), pa.IsoVMR('H2O', p)]),
         "VMR models: a parameter is named twice (['log_H2O', '[M/H]', 'log_H2O'])"),
        (dict(vmr_models=[pa.MetalEquil(), pa.IsoVMR('H2O', 2 * p)]),
         'VMR model log_H2O is defined on another pressure grid'),
        (dict(vmr_models=[pa.MetalEquil(), pa.IsoVMR('TiO', p)]),
         f'VMR model log_TiO: species TiO is not in the atmosphere ({cc.SPECIES})'),
        (dict(vmr_models=[pa.MetalEquil()] * 17), 'at most 16 VMR models, got 17'),
        (dict(free=['T_iso', '[M/H]', 'log_H2O', 'rplanet', 'log_refpressure']),
         "free: 'rplanet' and 'log_refpressure' cannot both be free (the reference maps one or "
         'the other, pyrat_obj.py:269-272)'),
        (dict(base_radius=None),
         'give base_radius[L], or base_params (the parameter vector of the base model, whose '
         'radius it then is)'),
        (dict(base_radius=None, base_params=[7000.0, 0.0, -3.5]),
         'base_params give a rejected model: equilibrium chemistry: not converged, a '
         'temperature outside the Gibbs table, or an element ratio <= 0'),
        # without the network the arguments are those of free VMRs, whose first check this misses
        (dict(chemistry=None), 'base_vmr must have shape (5, 16), got (1,)'),
    ]
    for change, message in rows:
        with pytest.raises(ValueError) as err:
            pa.WalkerAtmosphere(**dict(good, **change))
        assert str(err.value) == message, list(change)
