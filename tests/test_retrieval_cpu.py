"""The retrieval front end on the host (pyratbay_amd/retrieval.py): parsing and name resolution
against fixture G28 (tests/golden/make_golden_retrieval.py: the reference's own retrieval_params
block, index maps, the state eval() leaves in its objects and Loglike's full vector), the prior and
prior-transform statements on hand-computed cases, and every refusal with its message.  No GPU:
the model and the bands are stand-ins with the attributes Retrieval reads."""
import types

import numpy as np
import pytest

from pyratbay_amd import atmosphere as pa
from pyratbay_amd import continuum as ct
from pyratbay_amd import observation as po
from pyratbay_amd import retrieval as pr
from pyratbay_amd import table as ptab

L = 8
PRESSURE = np.logspace(-5, 1, L)
WN = np.linspace(5900.0, 9000.0, 40)


def atmosphere(scalars, **kw):
    tmodel = pa.Guillot(PRESSURE, 2200.0)
    vmr_models = [pa.IsoVMR('H2O', PRESSURE)]
    free = list(tmodel.pnames) + ['log_H2O'] + list(scalars)
    vmr = np.tile([0.85, 0.1496, 4e-4], (L, 1))
    kw.setdefault('base_radius', np.linspace(7.5e9, 7.0e9, L))
    for name, value in (('mplanet', 1.2e30), ('rplanet', 7.1e9), ('refpressure', 0.1)):
        if name.replace('ref', 'log_ref') not in scalars:
            kw.setdefault(name, value)
    return pa.WalkerAtmosphere(PRESSURE, ['H2', 'He', 'H2O'], [2.01588, 4.002602, 18.01528], vmr,
                               ['H2', 'He'], tmodel, vmr_models, free=free, **kw)


def continuum(*extra):
    return ct.Continuum(WN, PRESSURE, [ct.Deck(PRESSURE, WN), ct.Lecavelier(PRESSURE, wn=WN),
                                       *extra])


def stand_ins(rt_path='emission', cont=None, grid=True, irradiation=None):
    model = types.SimpleNamespace(rt_path=rt_path, continuum=cont, irradiation=irradiation)
    bands = types.SimpleNamespace(nbands=2, star_grid=object() if grid else None)
    return model, bands


def observation(offsets=(), errs=()):
    return po.Observation(np.ones(2), np.ones(2), ['nrs1', 'nrs2'], list(offsets), list(errs))


@pytest.fixture(scope='module')
def g28(golden):
    return golden('g28_retrieval')


def g28_retrieval(g, tag, lines=None, **kw):
    block = str(g[f'{tag}_block'])
    if lines is not None:
        block = '\n'.join([ln for ln in block.splitlines() if ln.strip()][:lines])
    scalars = ['rplanet', 'mplanet'] if tag == 'eclipse' else ['log_refpressure', 'mplanet']
    model, bands = stand_ins('emission' if tag == 'eclipse' else 'transit', continuum(),
                             grid=tag == 'eclipse')
    return pr.Retrieval(model, atmosphere(scalars), bands, observation(), block,
                        runits=str(g[f'{tag}_runits']), mass_units=str(g[f'{tag}_mass_units']),
                        **kw)


# -------------------------------------------------------------------------------------------------
# parsing and resolution against the reference
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['eclipse', 'transmission'])
def test_parse_against_g28(g28, tag):
    g = g28
    p = pr.parse_retrieval_params(str(g[f'{tag}_block']))
    assert p.pnames == [str(n) for n in g[f'{tag}_pnames']]
    for name in ('params', 'pmin', 'pmax', 'pstep', 'prior', 'priorlow', 'priorup'):
        assert np.array_equal(getattr(p, name), g[f'{tag}_{name}']), name
    # the block has every field count, a fixed and a shared line
    counts = {len(ln.split()) for ln in str(g[f'{tag}_block']).splitlines() if ln.strip()}
    assert counts == {2, 5, 7, 8}
    assert np.any(p.pstep < 0) and np.any(p.pstep == 0)
    # the eight columns as arrays: the same object
    q = pr.parse_retrieval_params(dict(zip(pr.COLUMNS, p)))
    assert q.pnames == p.pnames and all(np.array_equal(a, b) for a, b in zip(q[1:], p[1:]))
    q = pr.parse_retrieval_params(tuple(p))
    assert q.pnames == p.pnames


def mass_gravity(m, r, G):
    """The fixed point the reference's MassGravity descriptor leaves after `atm.mplanet = m`."""
    grav = G * m / r**2
    while True:
        again = grav * r**2 / G
        if again == m:
            return m
        m = again
        if G * m / r**2 == grav:
            return m
        grav = G * m / r**2


def check_rows(g, tag, ret, nlines):
    """Every value split_host gives against what the reference's eval() left in its objects."""
    theta = g[f'{tag}_theta']
    full = g[f'{tag}_row_full'][:, :nlines]
    keep = [k for k, i in enumerate(np.where(g[f'{tag}_pstep'] > 0)[0]) if i < nlines]
    theta = theta[:, keep]
    assert np.array_equal(ret.expand_host(theta), full)
    assert np.all(ret.inside_host(theta))
    out = ret.split_host(theta)
    atm = ret.atmosphere
    params = out['params']
    ntemp = atm.tmodel.npars
    assert np.array_equal(params[:, :ntemp], g[f'{tag}_row_tpars'])
    assert np.array_equal(params[:, ntemp:ntemp + 1], g[f'{tag}_row_vmr_pars'])
    # M_planet: the value eval() ASSIGNS (pyrat_obj.py:275), bit for bit; what it LEAVES in
    # atm.mplanet went through the reference's MassGravity descriptor (pyrat/atmosphere.py:20-48:
    # gplanet = G m / r**2, then mplanet = gplanet r**2 / G, until neither changes), which moves
    # 1 of these 6 masses by an ulp: the same rule applied to the mapped value gives those bits
    mass = params[:, atm.par_scalar['mplanet']]
    assert np.array_equal(mass, g[f'{tag}_row_mplanet_assigned'])
    left = [mass_gravity(m, r, float(g['G'])) for m, r in zip(mass, g[f'{tag}_row_rplanet'])]
    assert np.array_equal(left, g[f'{tag}_row_mplanet'])
    if tag == 'eclipse':
        assert np.array_equal(params[:, atm.par_scalar['rplanet']], g[f'{tag}_row_rplanet'])
        assert np.all(g[f'{tag}_row_rplanet'] > 3e9)                 # (cgs)
    else:
        assert np.array_equal(10.0**params[:, atm.par_scalar['log_refpressure']],
                              g[f'{tag}_row_refpressure'])
    assert np.all(g[f'{tag}_row_mplanet'] > 1e29)
    for j in range(int(g[f'{tag}_nopacity'])):
        name = str(g[f'{tag}_opacity{j}_name'])
        want = g[f'{tag}_row_opacity{j}_pars']
        if name == 'deck':
            assert np.array_equal(out['deck_logp'], want[:, 0])
        elif name == 'lecavelier':
            assert np.array_equal(out['continuum_pars'], want)
        else:
            assert want.shape[1] == 0, name
    assert np.array_equal(out['f_patchy'], g[f'{tag}_row_fpatchy'])
    if nlines == len(g[f'{tag}_pnames']):
        assert np.array_equal(out['tstar'], g[f'{tag}_row_tstar'])
        assert np.array_equal(out['f_dilution'], g[f'{tag}_row_f_dilution'])


def check_maps(g, tag, ret, nlines):
    def index(a):
        return [] if a is None else [int(i) for i in np.ravel(a)]
    for name in ('irad', 'ipress', 'imass', 'ipatchy', 'irv', 'itemp', 'imol'):
        assert index(getattr(ret, name)) == index(g[f'{tag}_{name}']), name
    for name in ('itstar', 'idilut'):
        want = [i for i in index(g[f'{tag}_{name}']) if i < nlines]
        assert index(getattr(ret, name)) == want, name
    assert ret.map_pars['temp'] == index(g[f'{tag}_map_temp'])
    assert [list(m) for m in ret.map_pars['mol']] == g[f'{tag}_map_mol'].tolist()
    assert ret.model_pnames == [str(n) for n in g[f'{tag}_temp_pnames']] + \
        [str(n) for n in g[f'{tag}_mol_pnames']]
    for j in range(int(g[f'{tag}_nopacity'])):
        name = str(g[f'{tag}_opacity{j}_name'])
        assert ret.iopacity.get(name, []) == index(g[f'{tag}_iopacity{j}']), name
        assert ret.map_pars['opacity'].get(name, []) == index(g[f'{tag}_map_opacity{j}']), name


def test_resolve_against_g28_eclipse(g28):
    ret = g28_retrieval(g28, 'eclipse')
    assert ret.pnames == [str(n) for n in g28['eclipse_pnames']]
    assert ret.nfree == g28['eclipse_theta'].shape[1]
    assert ret.dest_names == ['params', 'continuum_pars', 'deck_logp', 'f_patchy', 'tstar',
                              'f_dilution']
    assert pr.RUNITS['rjup'] == float(g28['rjup']) and pr.MASS_UNITS['mjup'] == float(g28['mjup'])
    check_maps(g28, 'eclipse', ret, 15)
    check_rows(g28, 'eclipse', ret, 15)
    # T_irr is column 4 of the atmosphere's params, R_planet its 'rplanet' column times rjup
    i = ret.pnames.index('T_irr')
    assert ret.destination[i] == ('params', 4)
    i = ret.pnames.index('R_planet')
    assert ret.map_factor[i] == 7.1492e9 and ret.map_dest[i] == 0


def test_resolve_against_g28_transmission(g28):
    """The reference takes T_eff and f_dilution in any geometry; the batched loop has neither in
    transit geometry: the whole block is refused with eval_bands' message, its first 13 lines
    (everything but those two) resolve to the reference's state."""
    with pytest.raises(ValueError, match='not to transit geometry'):
        g28_retrieval(g28, 'transmission')
    ret = g28_retrieval(g28, 'transmission', lines=13)
    assert ret.pnames == [str(n) for n in g28['transmission_pnames']][:13]
    check_maps(g28, 'transmission', ret, 13)
    check_rows(g28, 'transmission', ret, 13)


# -------------------------------------------------------------------------------------------------
# constants of the map, fixed, shared
# -------------------------------------------------------------------------------------------------
BLOCK = """
    T_irr      1400.0   100.0  3000.0   50.0  1500.0  100.0  200.0
    log_H2O      -3.5   -10.0    -1.0    0.3
    R_planet      1.0     0.5     2.0    0.05    1.1    0.2
    log_k_ray     0.5    -5.0     5.0   -2
    offset_nrs2  10.0  -100.0   100.0    5.0
    T_eff      5500.0
"""


def small(block=BLOCK, base=True, fixed=None, cont='default', **kw):
    base_params = np.array([-1.5, -0.8, 0.2, 0.4, 1400.0, 150.0, -3.4, 7.5e9]) if base else None
    atm = atmosphere(['rplanet'], base_params=base_params)
    model, bands = stand_ins(cont=continuum() if cont == 'default' else cont, **kw)
    obs = observation(['offset_nrs1', 'offset_nrs2'], ['err_scale_nrs1'])
    return pr.Retrieval(model, atm, bands, obs, block, fixed=fixed)


def test_constants_fixed_and_shared():
    ret = small(fixed={'alpha': 0.25, 'offset_nrs1': -3.0})
    assert ret.nfree == 4 and list(ret.ifree) == [0, 1, 2, 4]
    assert ret.dest_names == ['params', 'continuum_pars', 'tstar', 'offsets']
    theta = np.array([[1450.0, -3.0, 1.2, 7.0], [1300.0, -4.0, 0.9, -2.0]])
    full = ret.expand_host(theta)
    assert np.array_equal(full[:, 3], theta[:, 1])                   # shared with log_H2O
    assert np.array_equal(full[:, 5], [5500.0, 5500.0])              # fixed at value
    out = ret.split_host(theta)
    base = ret.atmosphere.base_params
    want = np.tile(base, (2, 1))
    want[:, 4], want[:, 6], want[:, 7] = theta[:, 0], theta[:, 1], theta[:, 2] * 7.1492e9
    want[:, 3] = 0.25                                                # fixed=
    assert np.array_equal(out['params'], want)
    # log_k_ray follows log_H2O; alpha_ray is the model's current value
    assert np.array_equal(out['continuum_pars'], np.stack([theta[:, 1], [-4.0, -4.0]], axis=1))
    assert np.array_equal(out['tstar'], [5500.0, 5500.0])
    assert np.array_equal(out['offsets'], np.stack([[-3.0, -3.0], theta[:, 3]], axis=1))
    assert 'err_pars' not in out                                     # (no line names one)
    # a walker outside the bounds is mapped from the block's values
    theta[1, 1] = np.nan
    assert list(ret.inside_host(theta)) == [True, False]
    sub = ret.split_host(theta)
    assert sub['params'][1, 4] == 1400.0 and sub['params'][1, 7] == 1.0 * 7.1492e9
    assert np.array_equal(sub['params'][0], want[0])
    assert np.isnan(ret.split_host(theta, substitute=False)['params'][1, 6])
    lp = ret.log_prior_host(theta)
    assert np.isfinite(lp[0]) and lp[1] == -np.inf


# -------------------------------------------------------------------------------------------------
# priors and the prior transform, by hand
# -------------------------------------------------------------------------------------------------
def test_log_prior_by_hand():
    ret = small()
    #            T_irr: 1500 -100 +200; log_H2O, offset: uniform; R_planet: 1.1 +-0.2
    at_prior = np.array([[1500.0, -3.0, 1.1, 0.0]])
    assert ret.log_prior_host(at_prior)[0] == 0.0
    below = np.array([[1400.0, -3.0, 1.1, 0.0]])                     # one sigma below (lo = 100)
    above = np.array([[1700.0, -3.0, 1.1, 0.0]])                     # one sigma above (up = 200)
    assert ret.log_prior_host(below)[0] == -0.5 and ret.log_prior_host(above)[0] == -0.5
    two = np.array([[1300.0, -9.0, 1.1, 50.0]])                      # two sigma below: -2
    assert ret.log_prior_host(two)[0] == -2.0
    both = np.array([[1700.0, -3.0, 1.1 + 0.2 * 3, 0.0]])            # + three sigma in R_planet
    np.testing.assert_allclose(ret.log_prior_host(both)[0], -0.5 - 4.5, rtol=1e-14)
    # the ends of the bounds are inside, one ulp beyond is not
    ends = np.array([[100.0, -10.0, 0.5, -100.0], [3000.0, -1.0, 2.0, 100.0]])
    assert np.all(ret.inside_host(ends))
    for k in range(4):
        for row, way in ((0, -np.inf), (1, np.inf)):
            out = ends.copy()
            out[row, k] = np.nextafter(out[row, k], way)
            assert list(ret.inside_host(out)) == [row != 0, row != 1]
    for bad in (np.nan, np.inf, -np.inf):
        out = ends.copy()
        out[0, 3] = bad
        assert list(ret.inside_host(out)) == [False, True]


def test_prior_transform_by_hand():
    from scipy.special import ndtri
    ret = small()
    lo, up = 100.0, 200.0
    split = lo / (lo + up)
    u = np.array([[split, 0.0, 0.5, 1.0],
                  [0.5 * split, 1.0, 0.5, 0.0],
                  [np.nextafter(split, 0.0), 0.25, 0.5, 0.5]])
    got = ret.prior_transform_host(u)
    assert got[0, 0] == 1500.0                                       # the split point maps to prior
    assert np.array_equal(got[:, 2], [1.1, 1.1, 1.1])                # symmetric prior at u = 0.5
    # uniform parameters: the ends and the statement
    assert np.array_equal(got[:, 1], [-10.0, -1.0, -10.0 + 0.25 * 9.0])
    assert np.array_equal(got[:, 3], [100.0, -100.0, 0.0])
    # below the split: prior + lo ndtri(0.5 u (lo + up) / lo): a quarter of the mass below prior
    assert got[1, 0] == 1500.0 + lo * ndtri(0.5 * (0.5 * split) * (lo + up) / lo)
    np.testing.assert_allclose(got[1, 0], 1500.0 + lo * ndtri(0.25), rtol=1e-15)
    assert 1500.0 - 1e-10 < got[2, 0] <= 1500.0
    # one sigma on either side: the CDF of the two-sided density
    cdf_lo = split * 2 * 0.15865525393145707
    cdf_up = split + (1 - split) * (2 * 0.8413447460685429 - 1)
    got = ret.prior_transform_host(np.array([[cdf_lo, 0.5, 0.5, 0.5], [cdf_up, 0.5, 0.5, 0.5]]))
    np.testing.assert_allclose(got[:, 0], [1400.0, 1700.0], rtol=1e-13)
    # not truncated: inside catches what falls out
    far = ret.prior_transform_host(np.array([[1e-300, 0.5, 0.5, 0.5]]))
    assert far[0, 0] < 100.0 and not ret.inside_host(far)[0]
    # a uniform parameter with an infinite bound: refused by the transform only
    open_ = small(BLOCK.replace('log_H2O      -3.5   -10.0', 'log_H2O      -3.5   -inf'))
    assert open_.inside_host(np.array([[1500.0, -50.0, 1.1, 0.0]]))[0]
    with pytest.raises(ValueError, match=r"prior_transform: uniform parameters \['log_H2O'\]"):
        open_.prior_transform_host(u)


# -------------------------------------------------------------------------------------------------
# refusals
# -------------------------------------------------------------------------------------------------
def test_parse_refusals():
    for bad in ('T_irr', 'T_irr 1 2', 'T_irr 1 2 3', 'T_irr 1 2 3 4 5', 'T_irr 1 2 3 4 5 6 7 8'):
        with pytest.raises(ValueError, match='Invalid number of fields for retrieval_params '
                                             f"entry\n'{bad}'"):
            pr.parse_retrieval_params('log_H2O -3 -10 -1 0.3\n' + bad)
    with pytest.raises(ValueError, match=r"Repeated parameter names: \['T_irr'\]"):
        pr.parse_retrieval_params('T_irr 1\nlog_H2O 2\nT_irr 3')
    with pytest.raises(ValueError, match='eight columns'):
        pr.parse_retrieval_params((['a'], [1.0]))
    with pytest.raises(ValueError, match='every column must have 1 entries'):
        pr.parse_retrieval_params((['a'], [1.0, 2.0]) + ([0.0],) * 6)


def test_resolution_refusals():
    with pytest.raises(ValueError, match="Invalid retrieval parameter 'log_CO'. Possible values "
                                         r"are:\n\['log_p_ref', 'R_planet', .*'T_int', 'log_H2O', "
                                         r"'log_k_ray', 'alpha_ray', 'log_p_cl', 'offset_nrs1', "
                                         r"'offset_nrs2', 'err_scale_nrs1'\]"):
        small(BLOCK + 'log_CO -3 -10 -1 0.3')
    with pytest.raises(ValueError, match='no free parameters'):
        small('T_irr 1400\nT_eff 5500')
    # shared: out of range, and shared with a shared parameter (DEVIATION)
    with pytest.raises(ValueError, match='shared with parameter 8: there are 6'):
        small(BLOCK.replace('   -2\n', '   -9\n'))
    with pytest.raises(ValueError, match="'offset_nrs2' is shared with 'log_k_ray', which is "
                                         'shared itself'):
        small(BLOCK.replace('100.0    5.0', '100.0    -4'))
    # two continuum models of one kind
    two = ct.Continuum(WN, PRESSURE,
                       [ct.Lecavelier(PRESSURE, wn=WN), ct.Lecavelier(PRESSURE, wn=WN)])
    with pytest.raises(ValueError, match="'log_k_ray': 2 continuum models of one kind claim it"):
        small(cont=two)
    # destinations the objects cannot take
    with pytest.raises(ValueError, match="'M_planet': the atmosphere has no free 'mplanet'"):
        small(BLOCK + 'M_planet 0.6 0.1 2 0.1')
    with pytest.raises(ValueError, match="'log_p_ref': the atmosphere has no free"):
        small(BLOCK + 'log_p_ref -1 -3 1 0.1')
    with pytest.raises(ValueError, match='need a stellar SED grid on the bands'):
        small(grid=False)
    assert small(grid=False, irradiation=(object(), 1.0)).dest_names[2] == 'tstar'
    no_star = BLOCK.replace('T_eff      5500.0', '')
    with pytest.raises(ValueError, match=r'stellar SED grid \(set_eclipse_grid\): tstar\[nw\] is '
                                         'needed'):
        small(no_star)
    with pytest.raises(ValueError, match=r'irradiation \(irradiation=\): tstar\[nw\] is needed'):
        small(no_star, grid=False, irradiation=(object(), 1.0))
    assert small(no_star, grid=False).dest_names == ['params', 'continuum_pars', 'offsets']
    with pytest.raises(ValueError, match='rv .a radial-velocity shift. needs a HiresData'):
        small(BLOCK + 'rv_shift 0 -10 10 1')
    # high-resolution data: rv_shift goes to rv, T_eff is refused
    from pyratbay_amd.bands import HiresData
    atm = atmosphere(['rplanet'], base_params=np.array([-1.5, -0.8, 0.2, 0.4, 1400.0, 150.0,
                                                        -3.4, 7.5e9]))
    model, _ = stand_ins(cont=continuum())
    hires = object.__new__(HiresData)
    ret = pr.Retrieval(model, atm, hires, observation(), 'T_irr 1400 0 3000 50\nrv_shift 1 -9 9 1')
    assert ret.dest_names == ['params', 'rv'] and ret.irv == [1]
    assert np.array_equal(ret.split_host(np.array([[1500.0, -2.5]]))['rv'], [-2.5])
    with pytest.raises(ValueError, match='tstar / rplanet with a HiresData are not supported'):
        pr.Retrieval(model, atm, hires, observation(), 'T_irr 1400 0 3000 50\nT_eff 5000')
    with pytest.raises(ValueError, match='deck_logp needs a Deck'):
        small(BLOCK.replace('log_k_ray     0.5    -5.0     5.0   -2', 'log_p_cl 0 -5 2 0.1'),
              cont=None)
    with pytest.raises(ValueError, match="Invalid retrieval parameter 'log_k_ray'"):
        small(cont=None)
    with pytest.raises(ValueError, match=r'deck_logp: clouds are not supported.*two-stream'):
        small(BLOCK + 'log_p_cl 0 -5 2 0.1', rt_path='two_stream')
    with pytest.raises(ValueError, match=r'f_patchy: clouds are not supported.*two-stream'):
        small(BLOCK + 'f_patchy 0.5 0 1 0.1', rt_path='two_stream')
    with pytest.raises(ValueError, match='not to transit geometry'):
        small(rt_path='transit')
    with pytest.raises(ValueError, match="'f_dilution' belongs to emission"):
        small(no_star + 'f_dilution 0.9 0 1 0.05', rt_path='transit', grid=False)
    # a column nobody names and the objects hold no value for
    with pytest.raises(ValueError, match=r"'log_kappa'' \(params, column 0\) is named neither"):
        small(base=False)
    # fixed: unknown names, names of the block, two names for one value
    with pytest.raises(ValueError, match="Invalid retrieval parameter 'nope'"):
        small(fixed={'nope': 1.0})
    with pytest.raises(ValueError, match="fixed: 'T_irr' is a line of retrieval_params"):
        small(fixed={'T_irr': 1.0})
    with pytest.raises(ValueError, match="runits 'parsec'"):
        pr.Retrieval(None, None, None, None, BLOCK, runits='parsec')
    assert ptab.MSG_STAR_TRANSIT.startswith('eval_bands: tstar / rplanet')
