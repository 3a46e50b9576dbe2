"""Atmospheres from retrieval parameters, host side (pyratbay_amd/atmosphere.py): the host forms
against fixture G22 (the reference's own functions, tests/golden/make_golden_atmosphere.py), the
constructor's / bind's / evaluate's validation, evaluate_host against the chained host forms, and
pb_walker_atmosphere's struct check before any HIP call.  No GPU.

Measured deviations of the host forms against G22 (every case, each function fed the RECORDED
results of the steps before it): Isothermal, Madhu, the VMR models + vmr_scale, qcapcheck,
ideal_gas_density, mean_weight, hydro_m and hydro_g 0 (the same bits); Guillot 8.9e-16 (the
reference's C extension is built with -ffast-math and has its own E2) -> tolerance 1e-14."""
import ctypes as C

import numpy as np
import pytest

import atm_cases as ac

GUILLOT_RTOL = 1e-14
G = ac.g22()
CASES = list(enumerate(G['case_list']))
IDS = [f'c{i}-{c["group"]}' for i, c in CASES]


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


def test_fixture_covers_the_cases():
    groups = [c['group'] for _, c in CASES]
    assert groups.count('isothermal') == 2 and groups.count('guillot') == 6
    assert groups.count('madhu') == 5 and groups.count('vmr') >= 6 and groups.count('radius') == 9
    assert {c['grid'] for _, c in CASES} >= {'p2', 'p11', 'p65', 'p81'}
    for name, n in (('p2', 2), ('p11', 11), ('p65', 65), ('p81', 81)):
        assert np.array_equal(G[f'grid_{name}'], np.logspace(-8, 2, n))
    assert sum(c['stops_after'] == 'temp' for _, c in CASES) == 1
    assert sum(c.get('qcap_flag', False) for _, c in CASES) == 1
    assert sum(c.get('divergent', False) for _, c in CASES) == 1
    assert {len(c['bulk']) for _, c in CASES if c['group'] == 'vmr'} == {1, 2}
    assert {len(c['vmr_models']) for _, c in CASES if c['group'] == 'vmr'} == {1, 2, 3}


def test_constants(pa):
    assert np.array_equal(G['constants'], [pa.K_BOLTZ, pa.G_GRAV, pa.N_AVOGADRO, pa.BAR])


@pytest.mark.parametrize('i,case', CASES, ids=IDS)
def test_host_forms_vs_g22(pa, i, case):
    species = [str(s) for s in G['species']]
    pressure, base_vmr = G[f'grid_{case["grid"]}'], G[f'base_vmr_{case["grid"]}']
    tmodel, vmr_models = ac.models(case, pressure, base_vmr, species)
    temp = tmodel(np.array(case['tpars']))
    want_temp = G[f'c{i}_temp']
    dev = ac.max_rel(temp, want_temp)
    print(f'case {i} {case["tmodel"]}: temperature max rel {dev:.2e}')
    assert dev <= (GUILLOT_RTOL if case['tmodel'] == 'guillot' else 0.0)
    if case['stops_after'] == 'temp':
        assert np.all(temp == 0.0)
        return
    pars, k = [], 0
    for m in vmr_models:
        pars.append(case['vmr_pars'][k:k + m.npars])
        k += m.npars
    vmr = pa.vmr_scale(base_vmr, species, vmr_models, pars, case['bulk'])
    assert np.array_equal(vmr, G[f'c{i}_vmr'])
    ibulk = [species.index(b) for b in case['bulk']]
    assert pa.qcapcheck(vmr, case['qcap'], ibulk) == case['qcap_flag']
    # each later step from the RECORDED results of the steps before it
    assert np.array_equal(pa.ideal_gas_density(vmr, pressure, want_temp), G[f'c{i}_dens'])
    mm = pa.mean_weight(vmr, mass=G['mass'])
    assert np.array_equal(mm, G[f'c{i}_mm'])
    if case['rmodel'] == 'hydro_m':
        radius = pa.hydro_m(pressure, want_temp, mm, case['mplanet'], case['refpressure'],
                            case['rplanet'])
    else:
        radius = pa.hydro_g(pressure, want_temp, mm, case['gplanet'], case['refpressure'],
                            case['rplanet'])
    assert np.array_equal(radius, G[f'c{i}_radius'])
    assert bool(np.any(np.isinf(radius))) == case['divergent']


def test_expn2(pa):
    """E2 at its branch points: E2(0) = 1, the cutoff, the series at x = 1 (E2(1) =
    0.148495506775922...) and the continued fraction one ulp above it.  Bound of the continued
    fraction: about 60 Lentz steps at x = 1, each a product rounded to half an ulp, 60 * 1.1e-16
    = 7e-15 -> 1e-14; with SciPy at hand also against scipy.special.expn over 1e-12 ... 88."""
    assert pa.expn2(0.0)[0] == 1.0
    assert pa.expn2(88.03)[0] == 0.0 and pa.expn2(88.02)[0] > 0.0
    below, above = pa.expn2(1.0)[0], pa.expn2(np.nextafter(1.0, 2.0))[0]
    assert abs(below - 0.14849550677592205) < 2e-16 and abs(above / below - 1) < 1e-14
    special = pytest.importorskip('scipy.special')
    x = 10.0**np.random.default_rng(0).uniform(-12, np.log10(88.0), 3000)
    assert np.max(np.abs(pa.expn2(x) / special.expn(2, x) - 1)) < 1e-14


def test_gaussian_filter_matches_scipy(pa):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(3)
    for n, sigma in ((11, 0.33), (11, 3.3), (5, 9.0), (81, 2.64), (2, 0.033)):
        raw = rng.uniform(500.0, 2500.0, n)
        got = pa.correlate_nearest(raw, pa.gaussian_weights(sigma))
        assert np.array_equal(got, ndimage.gaussian_filter1d(raw, sigma=sigma, mode='nearest'))


def test_evaluate_host_is_the_chain(pa):
    for i in (2, 9, 17, 25):
        case = G['case_list'][i]
        atm, params = ac.walker_atmosphere(case)
        got = atm.evaluate_host(params)
        species = atm.species
        itab = [species.index(s) for s in ac.TABLE_SPECIES]
        temp = atm.tmodel(params[:atm.tmodel.npars])
        pars = [params[o:o + m.npars] for o, m in zip(atm.vmr_par, atm.vmr_models)]
        vmr = pa.vmr_scale(atm.base_vmr, species, atm.vmr_models, pars, case['bulk'])
        mm = pa.mean_weight(vmr, mass=atm.mol_mass)
        hydro = pa.hydro_m if case['rmodel'] == 'hydro_m' else pa.hydro_g
        radius = hydro(atm.pressure, temp, mm,
                       case['mplanet'] if case['rmodel'] == 'hydro_m' else case['gplanet'],
                       case['refpressure'], case['rplanet'])
        assert got.reject == 0
        assert np.array_equal(got.temps, temp) and np.array_equal(got.mm, mm)
        assert np.array_equal(got.dens, pa.ideal_gas_density(vmr, atm.pressure, temp)[:, itab])
        assert np.array_equal(got.radius, radius)
        assert got.continuum_density is None and got.alkali_density is None


def test_evaluate_host_free_scalars_and_rejects(pa):
    case = G['case_list'][20]
    atm, params = ac.walker_atmosphere(case, free_scalars=('rplanet', 'mplanet'))
    fixed, fixed_params = ac.walker_atmosphere(case)
    assert atm.free[-2:] == ['rplanet', 'mplanet'] and atm.npar == fixed.npar + 2
    a, b = atm.evaluate_host(params), fixed.evaluate_host(fixed_params)
    assert np.array_equal(a.radius, b.radius) and a.reject == b.reject == 0
    logp, logp_params = ac.walker_atmosphere(case, free_scalars=('log_refpressure',))
    # (10**log10(p0) is p0 to an ulp or two; the radius moves by less than that relative step)
    assert ac.max_rel(logp.evaluate_host(logp_params).radius, b.radius) < 1e-13
    # every reject reason: its bit, temps = 0, zero densities, the base radius
    out = logp_params.copy()
    out[-1] = 2.5                                            # 10^2.5 bar: below the grid's bottom
    cold = fixed_params.copy()
    cold[4] = cold[5] = 0.0                                  # T_irr = T_int = 0
    for model, p, bit in ((logp, out, pa.REJECT_REFPRESSURE), (fixed, cold, pa.REJECT_TEMP)):
        r = model.evaluate_host(p)
        assert r.reject & bit
        assert np.all(r.temps == 0) and np.all(r.dens == 0) and np.all(r.mm == 0)
        assert np.array_equal(r.radius, model.base_radius)
    for i, bit in ((10, pa.REJECT_MADHU | pa.REJECT_TEMP), (19, pa.REJECT_QCAP),
                   (28, pa.REJECT_DIVERGENT)):
        model, p = ac.walker_atmosphere(G['case_list'][i])
        r = model.evaluate_host(p)
        assert r.reject == bit, (i, r.reject)
        assert np.all(r.temps == 0) and np.all(r.dens == 0)
        assert np.array_equal(r.radius, model.base_radius)


def test_constructor_validation(pa):
    case = G['case_list'][17]                     # slant + scale + iso
    atm, params = ac.walker_atmosphere(case)
    names = atm.free
    with pytest.raises(ValueError, match='cannot both be free'):
        ac.walker_atmosphere(case, free=names + ['rplanet', 'log_refpressure'])
    with pytest.raises(ValueError, match="'tstar' is not one of"):
        ac.walker_atmosphere(case, free=names + ['tstar'])
    with pytest.raises(ValueError, match='must begin with'):
        ac.walker_atmosphere(case, free=names[1:])
    with pytest.raises(ValueError, match='listed twice'):
        ac.walker_atmosphere(case, free=names + ['mplanet', 'mplanet'])
    with pytest.raises(ValueError, match='hydro_m needs mplanet'):
        ac.walker_atmosphere(case, mplanet=None)
    with pytest.raises(ValueError, match='strictly decreasing'):
        ac.walker_atmosphere(case, base_radius=np.ones(11))
    pressure, species = atm.pressure, atm.species

    equil = type('MetalEquil', (), dict(name='metal_equil', type='equil', species='H2O',
                                        pressure=pressure, npars=1, pnames=['[M/H]']))
    with pytest.raises(ValueError, match='equilibrium-chemistry'):
        pa.WalkerAtmosphere(pressure, species, atm.mol_mass, atm.base_vmr, ['H2'],
                            pa.Isothermal(pressure), [equil()], mplanet=1e30, rplanet=7e9,
                            refpressure=0.1, base_radius=atm.base_radius)
    with pytest.raises(ValueError, match='bulk species or has a model already'):
        pa.WalkerAtmosphere(pressure, species, atm.mol_mass, atm.base_vmr, ['H2'],
                            pa.Isothermal(pressure),
                            [pa.IsoVMR('CO', pressure), pa.IsoVMR('CO', pressure)], mplanet=1e30,
                            rplanet=7e9, refpressure=0.1, base_radius=atm.base_radius)
    with pytest.raises(ValueError, match='gravity = None or a scalar'):
        pa.WalkerAtmosphere(pressure, species, atm.mol_mass, atm.base_vmr, ['H2'],
                            pa.Guillot(pressure, np.full(11, 1000.0)), [], mplanet=1e30,
                            rplanet=7e9, refpressure=0.1, base_radius=atm.base_radius)
    # base_radius defaults to the radius of the model at base_params
    made = pa.WalkerAtmosphere(pressure, species, atm.mol_mass, atm.base_vmr, case['bulk'],
                               atm.tmodel, atm.vmr_models, mplanet=case['mplanet'],
                               rplanet=case['rplanet'], refpressure=case['refpressure'],
                               base_params=params)
    assert np.array_equal(made.base_radius, atm.bind(ac.TABLE_SPECIES).evaluate_host(params).radius)
    with pytest.raises(ValueError, match='base_radius'):
        pa.WalkerAtmosphere(pressure, species, atm.mol_mass, atm.base_vmr, case['bulk'],
                            atm.tmodel, atm.vmr_models, mplanet=case['mplanet'],
                            rplanet=case['rplanet'], refpressure=case['refpressure'])


def test_bind_and_evaluate_validation(pa):
    import torch
    atm, params = ac.walker_atmosphere(G['case_list'][14])
    with pytest.raises(ValueError, match='table species TiO is not in the atmosphere'):
        atm.bind(['H2O', 'TiO'])

    class Cont:
        species, alkali_species = ['H2', 'He'], ['Na']
    with pytest.raises(ValueError, match='alkali species Na is not in the atmosphere'):
        atm.bind(['H2O'], Cont())
    Cont.alkali_species = []
    atm.bind(['H2O', 'CO'], Cont())
    st = atm.model_struct()
    assert (st.ntab, st.ncont, st.nalk) == (2, 2, 0)
    host = atm.evaluate_host(params)
    assert host.dens.shape == (11, 2) and host.continuum_density.shape == (11, 2)
    # shape and dtype are refused before any HIP call (this machine may have no GPU at all)
    for bad in (torch.zeros(3, atm.npar + 1, dtype=torch.float64),
                torch.zeros(3, atm.npar, dtype=torch.float32),
                torch.zeros(atm.npar, dtype=torch.float64), params):
        with pytest.raises(ValueError, match='params must be a float64 tensor of shape'):
            atm.evaluate(bad)
    fresh, _ = ac.walker_atmosphere(G['case_list'][14])
    fresh._table_species = None
    with pytest.raises(ValueError, match='bind'):
        fresh.evaluate(torch.zeros(1, fresh.npar, dtype=torch.float64))


def test_struct_mirror_and_check_before_hip(pa):
    """AtmModelStruct mirrors pb_atm_model, and pb_walker_atmosphere checks it before any HIP
    call: with a bad field the call fails with PB_ERR_ARG and a message that names it, GPU or
    not (the pointers below are never dereferenced)."""
    from pyratbay_amd import _capi
    assert 'pb_walker_atmosphere' in _capi.exported_names()
    lib = _capi.lib()
    atm, _ = ac.walker_atmosphere(G['case_list'][17])
    # 4-byte counts, 8-byte doubles and pointers, natural alignment (pbhip.h's declaration)
    assert C.sizeof(pa.AtmModelStruct) == 456
    assert (pa.AtmModelStruct.mplanet.offset, pa.AtmModelStruct.base_radius_d.offset,
            pa.AtmModelStruct.alk_map_d.offset) == (352, 408, 448)

    def filled():
        st = atm.model_struct()
        for name, ctype in pa.AtmModelStruct._fields_:
            if ctype is C.c_void_p:
                setattr(st, name, 4096)
        return st

    def check(st, text):
        rc = lib.pb_walker_atmosphere(C.byref(st), 4096, 0, *([4096] * 7), None)
        assert rc == -1, (text, rc)
        assert text in lib.pb_last_error().decode(), lib.pb_last_error()
    st = filled()
    assert lib.pb_walker_atmosphere(C.byref(st), 4096, 0, *([4096] * 7), None) == 0   # no walkers
    st.nlayers = 1025
    check(st, '2-1024 layers, not 1025')
    st = filled()
    st.vmr_par[2] = st.npar
    check(st, 'VMR model 2: parameters')
    st = filled()
    st.par_rplanet, st.par_log_refpressure = 0, 1
    check(st, 'cannot both be free')
    st = filled()
    st.vmr_species[1] = st.bulk_species[0]
    check(st, 'is a bulk species or has a model already')
    st = filled()
    st.tab_map_d = None
    check(st, 'bind first')
    st = filled()
    st.mplanet = 0.0
    check(st, 'mplanet 0')
    with pytest.raises(_capi.PbError, match='null model struct'):
        _capi.call('pb_walker_atmosphere', None, None, 0, *([None] * 8))


@pytest.mark.parametrize('i,scalars', [(20, ('rplanet', 'mplanet')), (24, ('rplanet',))])
def test_bad_free_scalars_are_rejected_on_the_host(pa, i, scalars):
    """hydro_m and hydro_g: a free rplanet or mplanet that is NaN, zero, negative or infinite
    gives a radius that is no geometry; the walker has the divergent bit and the base radius."""
    atm, good = ac.walker_atmosphere(G['case_list'][i], free_scalars=scalars)
    assert atm.evaluate_host(good).reject == 0
    for k in range(atm.npar - len(scalars), atm.npar):
        for bad in (float('nan'), 0.0, -good[k], float('inf')):
            p = good.copy()
            p[k] = bad
            r = atm.evaluate_host(p)
            assert r.reject == pa.REJECT_DIVERGENT, (atm.free[k], bad, r.reject)
            assert np.all(r.temps == 0) and np.array_equal(r.radius, atm.base_radius)


def test_guillot_gravity_must_be_positive(pa):
    atm, _ = ac.walker_atmosphere(G['case_list'][14])
    for gravity in (0.0, -980.0, float('nan')):
        with pytest.raises(ValueError, match='gravity must be positive'):
            pa.WalkerAtmosphere(atm.pressure, atm.species, atm.mol_mass, atm.base_vmr, ['H2'],
                                pa.Guillot(atm.pressure, gravity), [], mplanet=1e30, rplanet=7e9,
                                refpressure=0.1, base_radius=atm.base_radius)


def test_refusal_messages_are_stable(pa):
    """One bad constructor argument per row and the whole message its caller gets, compared with
    == : the checks sit in WalkerAtmosphere and in the object that forms its VMRs, and which of
    two checks a bad argument meets first decides the message (a shorter pressure grid meets
    base_vmr's shape before the T model's grid).  The messages are those of the commit before
    atmosphere.py was split."""
    atm, _ = ac.walker_atmosphere(G['case_list'][17])
    p = atm.pressure
    species = "['H2', 'He', 'H2O', 'CH4', 'CO', 'CO2']"
    good = dict(pressure=p, species=atm.species, mol_mass=atm.mol_mass, base_vmr=atm.base_vmr,
                bulk=['H2'], tmodel=pa.Isothermal(p), vmr_models=[pa.IsoVMR('CO', p)],
                mplanet=1e30, rplanet=7e9, refpressure=0.1, base_radius=atm.base_radius)
    pa.WalkerAtmosphere(**good)
    rows = [
        (dict(pressure=p[:-1]), 'base_vmr must have shape (10, 6), got (11, 6)'),
        (dict(pressure=2 * p), 'tmodel is defined on another pressure grid'),
        (dict(species=atm.species[:-1]), 'mol_mass must have shape (5,), got (6,)'),
        (dict(base_vmr=atm.base_vmr[:-1]), 'base_vmr must have shape (11, 6), got (10, 6)'),
        (dict(bulk=['H2', 'Ar']), f'bulk species Ar is not in the atmosphere ({species})'),
        (dict(bulk=[]), 'bulk: 1 ... 4 distinct species, got []'),
        (dict(tmodel=pa.Isothermal(2 * p)), 'tmodel is defined on another pressure grid'),
        (dict(vmr_models=[pa.IsoVMR('H2', p)]),
         'VMR model log_H2: species H2 is a bulk species or has a model already'),
        (dict(vmr_models=[pa.IsoVMR('CO', p), pa.SlantVMR('CO', p)]),
         'VMR model slant_CO: species CO is a bulk species or has a model already'),
        (dict(vmr_models=[pa.IsoVMR('TiO', p)]),
         f'VMR model log_TiO: species TiO is not in the atmosphere ({species})'),
        (dict(vmr_models=[pa.IsoVMR('CO', 2 * p)]),
         'VMR model log_CO is defined on another pressure grid'),
        (dict(vmr_models=[pa.MetalEquil()]),
         'VMR model metal_equil: equilibrium-chemistry and hybrid models are not supported '
         'without chemistry=ChemNetwork(...), only IsoVMR, ScaleVMR and SlantVMR'),
        (dict(vmr_models=[pa.IsoVMR('CO', p)] * 17), 'at most 16 VMR models, got 17'),
        (dict(free=['T_iso', 'log_CO', 'rplanet', 'log_refpressure']),
         "free: 'rplanet' and 'log_refpressure' cannot both be free (the reference maps one or "
         'the other, pyrat_obj.py:269-272)'),
        (dict(free=['T_iso', 'log_CO', 'tstar']),
         "free: 'tstar' is not one of ('rplanet', 'log_refpressure', 'mplanet')"),
        (dict(free=['log_CO', 'T_iso']),
         "free must begin with the models' parameters ['T_iso', 'log_CO'], got "
         "['log_CO', 'T_iso']"),
        (dict(rmodel='hydro_g'), 'hydro_g needs gplanet (cm s-2)'),
        (dict(mplanet=None), 'hydro_m needs mplanet (g), as a constant or a free parameter'),
        (dict(rplanet=None), 'rplanet (cm) is needed, as a constant or a free parameter'),
        (dict(refpressure=None),
         'refpressure (bar) is needed, as a constant or a free parameter'),
        (dict(base_radius=None),
         'give base_radius[L], or base_params (the parameter vector of the base model, whose '
         'radius it then is)'),
        (dict(base_radius=None, base_params=[-5.0, -3.0]),
         'base_params give a rejected model: temperature <= 0 or not finite, divergent hydro_m '
         'profile, or a radius <= 0 or not finite'),
        (dict(base_radius=atm.base_radius[::-1]),
         'base_radius must be 11 finite, strictly decreasing radii'),
    ]
    for change, message in rows:
        with pytest.raises(ValueError) as err:
            pa.WalkerAtmosphere(**dict(good, **change))
        assert str(err.value) == message, list(change)
