"""The host statements of pyratbay_amd/observation.py against fixture G25 (the reference's own
Data.offset_data / Data.scale_errors, Loglike.__call__ on the arrays they give, and
interp1d(sed_temps, starflux, axis=0): tests/golden/make_golden_observation.py), the constructor
errors in the reference's wording, the argument checks of the two C entries (they run before any
HIP call) and the refusals of eval_bands that are decided before anything touches the device.
None of it needs a GPU."""
import types

import numpy as np
import pytest

import observation_cases as oc
from pyratbay_amd import observation


@pytest.fixture(scope='module')
def g25(golden):
    return golden('g25_observation')


def test_fixture_layout(g25):
    """What the issue asks of G25: 11 bands over three instruments, offsets on two, one scale and
    one quadrature model in ppm, 7 rows of which one is all defaults, one rejected and one a
    perfect fit; 5 SED nodes on 700 samples, 6 bands, tstar at the first, an inner and the last
    node and three values between nodes."""
    assert len(g25['band_names']) == 11 and len(set(g25['band_names'])) == 3
    assert len(g25['offset_models']) == 2 and str(g25['units']) == 'ppm'
    assert [str(m)[:9] for m in g25['err_models']] == ['err_scale', 'err_quad_']
    assert g25['offsets'].shape == (7, 2) and g25['err_pars'].shape == (7, 2)
    assert np.all(g25['offsets'][2] == 0) and list(g25['err_pars'][2]) == [0.0, -100.0]
    assert g25['loglike'][4] == -1.0e98 and np.isinf(g25['models'][4]).any()
    assert np.array_equal(g25['models'][5], g25['offset_data'][5])
    assert g25['star_fluxes'].shape == (5, 700) and int(g25['star_nbands']) == 6
    nodes = np.isin(g25['star_tstar'], g25['star_sed_temps'])
    assert nodes.sum() == 3 and len(nodes) == 6
    assert {float(g25['star_sed_temps'][0]), float(g25['star_sed_temps'][-1])} <= \
        set(g25['star_tstar'][nodes])


def test_offsets_and_error_scaling_equal_the_reference(g25):
    """offset_data_host / scale_errors_host: the reference's values bit for bit (the same NumPy
    expressions on the same NumPy scalars, 10.0**val included)."""
    obs = oc.observation_of(g25, observation)
    assert obs.unit == float(g25['unit_value'])
    assert list(obs.err_mode_host) == [observation.SCALE, observation.QUADRATURE]
    for r in range(len(g25['offsets'])):
        np.testing.assert_array_equal(obs.offset_data_host(g25['offsets'][r]),
                                      g25['offset_data'][r])
        np.testing.assert_array_equal(obs.scale_errors_host(g25['err_pars'][r]),
                                      g25['scaled_uncert'][r])
    # None: the data and uncertainties as given
    np.testing.assert_array_equal(obs.offset_data_host(), g25['data'])
    np.testing.assert_array_equal(obs.scale_errors_host(), g25['uncert'])
    np.testing.assert_array_equal(obs.scale_errors_host(obs.err_defaults), g25['uncert'])


def test_loglike_host_against_the_reference(g25):
    obs = oc.observation_of(g25, observation)
    got = obs.loglike_host(g25['models'], g25['offsets'], g25['err_pars'])
    print(got, g25['loglike'])
    np.testing.assert_allclose(got, g25['loglike'], rtol=1e-13)
    assert got[4] == -1.0e98
    # the defaults row, by leaving the parameters out
    assert obs.loglike_host(g25['models'][2]) == got[2]
    # without models: tools/retrieval_tools.py:98-104 on the plain arrays
    plain = observation.Observation(g25['data'], g25['uncert'])
    m = g25['models'][0]
    want = -0.5 * np.sum(((g25['data'] - m) / g25['uncert'])**2.0) \
        - 0.5 * np.sum(np.log(2.0 * np.pi * g25['uncert']**2.0))
    assert plain.loglike_host(m) == want


def test_groups(g25):
    obs = oc.observation_of(g25, observation)
    names = [str(n) for n in g25['band_names']]
    assert list(obs.offset_group_host) == [1 if 'miri' in n else 0 if 'nrs2' in n else -1
                                           for n in names]
    assert list(obs.err_group_host) == [0 if 'nrs1' in n else 1 if 'miri' in n else -1
                                        for n in names]


def test_constructor_errors():
    data, uncert = np.ones(4), np.ones(4)
    names = ['nirspec_nrs1', 'nirspec_nrs2', 'miri_lrs', 'miri_lrs']
    with pytest.raises(ValueError, match='Multiple instrumental offsets apply to a same data '
                                         'point'):
        observation.Observation(data, uncert, names, ['offset_nirspec', 'offset_nrs1'])
    with pytest.raises(ValueError, match='Multiple uncertainty scaling apply to a same data '
                                         'point'):
        observation.Observation(data, uncert, names, (), ['err_scale_miri', 'err_quad_lrs'])
    with pytest.raises(ValueError, match="Invalid instrumental offset parameter 'offset_wfc3'. "
                                         "There is no instrument matching the name 'wfc3'"):
        observation.Observation(data, uncert, names, ['offset_wfc3'])
    with pytest.raises(ValueError, match="Invalid retrieval parameter 'err_quad_wfc3'. "
                                         "There is no instrument matching the name 'wfc3'"):
        observation.Observation(data, uncert, names, (), ['err_quad_wfc3'])
    with pytest.raises(ValueError, match="Invalid error scaling parameter 'err_fudging_miri'"):
        observation.Observation(data, uncert, names, (), ['err_fudging_miri'])
    with pytest.raises(ValueError, match='units'):
        observation.Observation(data, uncert, names, units='permille')
    with pytest.raises(ValueError, match='band_names'):
        observation.Observation(data, uncert, None, ['offset_miri'])
    # a string is one model; underscores of the instrument are blanks, as in the reference
    obs = observation.Observation(data, uncert, ['a b', 'c', 'c', 'c'], 'offset_a_b')
    assert list(obs.offset_group_host) == [0, -1, -1, -1]
    assert observation.parse_error_param('err_quad_NIRSpec_PRISM') == \
        ('NIRSpec PRISM', observation.QUADRATURE)


def test_units():
    assert observation.UNITS == {'none': 1.0, 'percent': 0.01, 'ppt': 0.001, 'ppm': 1e-6}


# -----------------------------------------------------------------------------------------------
# StellarGrid.flux_host (its constructor needs a device for the resident copy: the statement is
# reached through an instance made without it)
# -----------------------------------------------------------------------------------------------
def host_grid(wn, sed_temps, fluxes):
    grid = object.__new__(observation.StellarGrid)
    grid.wn_host, grid.sed_temps_host, grid.fluxes_host = wn, sed_temps, fluxes
    grid.nt, grid.nwave = fluxes.shape
    return grid


def test_flux_host_equals_interp1d(g25):
    grid = host_grid(g25['star_wn'], g25['star_sed_temps'], g25['star_fluxes'])
    for w, t in enumerate(g25['star_tstar']):
        np.testing.assert_array_equal(grid.flux_host(t), g25['star_starflux'][w])
    np.testing.assert_array_equal(grid.flux_host(g25['star_tstar']), g25['star_starflux'])
    # and today's SciPy on a seeded case (2 nodes: the clip at both ends)
    import scipy.interpolate as si
    c = oc.star_case(2, 5)
    grid = host_grid(c['wn'], c['sed_temps'], c['fluxes'])
    np.testing.assert_array_equal(grid.flux_host(c['tstar']),
                                  si.interp1d(c['sed_temps'], c['fluxes'], axis=0)(c['tstar']))
    for bad in (c['sed_temps'][0] - 1.0, c['sed_temps'][-1] + 1.0, np.nan):
        with pytest.raises(ValueError, match='outside'):
            grid.flux_host(bad)


def test_stellar_grid_validates_before_the_device():
    wn = np.linspace(1.0, 2.0, 5)
    for temps, fluxes, match in (([5000.0], np.ones((1, 5)), 'at least 2'),
                                 ([4000.0, 5000.0], np.ones((2, 4)), 'shape'),
                                 ([5000.0, 4000.0], np.ones((2, 5)), 'ascending'),
                                 ([4000.0, 4000.0], np.ones((2, 5)), 'ascending'),
                                 ([4000.0, np.nan], np.ones((2, 5)), 'ascending')):
        with pytest.raises(ValueError, match=match):
            observation.StellarGrid(wn, temps, fluxes)


# -----------------------------------------------------------------------------------------------
# the C entries: argument checks come before any HIP call
# -----------------------------------------------------------------------------------------------
def test_entry_argument_checks():
    import ctypes as C
    from pyratbay_amd import _capi
    one = C.c_void_p(8)                         # (never dereferenced: the checks fail first)

    def star(nt=2, nbands=1, nw=1, bandflux=one):
        return _capi.call('pb_star_band_scale_batch', bandflux, one, one, one, 1.0, None, 1.0,
                          None, one, one, one, one, one, None, nt, nbands, 10, nw, None)
    assert star(nw=0) == 0 and star(nbands=0) == 0           # nothing launched
    with pytest.raises(_capi.PbError, match='at least 2 temperatures'):
        star(nt=1)
    with pytest.raises(_capi.PbError, match='null pointer'):
        star(bandflux=None)
    with pytest.raises(_capi.PbError, match='bad sizes'):
        star(nw=-1)

    def ll(noff=0, nerr=0, nw=1, nb=1, out=one):
        return _capi.call('pb_loglike_obs', out, one, one, one, None, None, 1.0, noff, None, None,
                          None, 1.0, nerr, nw, nb, None)
    assert ll(nw=0) == 0
    with pytest.raises(_capi.PbError, match='bad shape'):
        ll(nb=0)
    with pytest.raises(_capi.PbError, match='null pointer'):
        ll(out=None)
    with pytest.raises(_capi.PbError, match='offsets'):
        ll(noff=1)
    with pytest.raises(_capi.PbError, match='error models'):
        ll(nerr=1)


# -----------------------------------------------------------------------------------------------
# eval_bands' refusals that are decided before anything touches the device
# -----------------------------------------------------------------------------------------------
def bare_model(rt_path):
    from pyratbay_amd.table import TableSpectrum
    model = object.__new__(TableSpectrum)
    model.rt_path, model.continuum = rt_path, None
    model.nlayers, model.nwave, model.tmin, model.tmax = 4, 10, 300.0, 3000.0
    return model


def batch_call(model, bands, **kw):
    import torch
    temps = torch.zeros((3, 4), dtype=torch.float64)
    dens = torch.zeros((3, 4, 1), dtype=torch.float64)
    args = dict.fromkeys(('radius', 'f_dilution', 'continuum_density', 'continuum_pars', 'rv',
                          'deck_logp', 'f_patchy', 'alkali_density', 'spectra_out'))
    return model._batch_call(temps, dens, bands, **args, **kw)


@pytest.mark.parametrize('rt_path', ['emission', 'two_stream'])
def test_eval_bands_refusals(rt_path):
    import torch
    from pyratbay_amd.bands import HiresData
    tstar = torch.full((3,), 5000.0, dtype=torch.float64)
    rplanet = torch.full((3,), 7.0e9, dtype=torch.float64)
    plain = types.SimpleNamespace(nbands=2, star_grid=None)
    with_grid = types.SimpleNamespace(nbands=2, star_grid=object(), grid_rplanet=7.0e9)
    grid_no_radius = types.SimpleNamespace(nbands=2, star_grid=object(), grid_rplanet=None)
    model = bare_model(rt_path)
    with pytest.raises(ValueError, match='need a stellar SED grid'):
        batch_call(model, plain, tstar=tstar)
    with pytest.raises(ValueError, match='need a stellar SED grid'):
        batch_call(model, plain, rplanet=rplanet)
    with pytest.raises(ValueError, match=r'tstar\[nw\] is needed'):
        batch_call(model, with_grid)
    with pytest.raises(ValueError, match='rplanet needs tstar'):
        batch_call(model, with_grid, rplanet=rplanet)
    with pytest.raises(ValueError, match='HiresData'):
        batch_call(model, object.__new__(HiresData), tstar=tstar)
    with pytest.raises(ValueError, match='HiresData'):
        batch_call(model, object.__new__(HiresData), rplanet=rplanet)
    for kw in (dict(tstar=tstar), dict(rplanet=rplanet), dict(tstar=tstar, rplanet=rplanet)):
        with pytest.raises(ValueError, match='transit geometry'):
            batch_call(bare_model('transit'), with_grid, **kw)
    # host tensors, wrong shapes and dtypes: _check_walker_tensor's refusal
    with pytest.raises(ValueError, match='eval_bands: tstar must be a float64 device tensor'):
        batch_call(model, with_grid, tstar=tstar)
    with pytest.raises(ValueError, match='eval_bands: tstar must be'):
        batch_call(model, with_grid, tstar=np.full(3, 5000.0))
    with pytest.raises(ValueError, match='a planet radius is needed'):
        batch_call(model, grid_no_radius, tstar=tstar)


def test_free_rplanet_column():
    """eval_params' rule: the atmosphere's free 'rplanet' is the rplanet of the eclipse factor
    when the bands carry a grid; the caller's own is then refused; otherwise kw is untouched."""
    import torch
    from pyratbay_amd.table import free_rplanet
    params = torch.arange(12, dtype=torch.float64).view(4, 3)
    atm = types.SimpleNamespace(par_scalar={'rplanet': 2, 'log_refpressure': -1, 'mplanet': -1})
    fixed = types.SimpleNamespace(par_scalar={'rplanet': -1, 'log_refpressure': -1, 'mplanet': 0})
    grid = types.SimpleNamespace(star_grid=object())
    plain = types.SimpleNamespace(star_grid=None)
    kw = {'chunk': 2}
    got = free_rplanet(atm, params, grid, kw, 'eval_params')
    assert torch.equal(got['rplanet'], params[:, 2]) and got['rplanet'].is_contiguous()
    assert got['chunk'] == 2 and 'rplanet' not in kw
    assert free_rplanet(atm, params, plain, kw, 'eval_params') is kw
    assert free_rplanet(fixed, params, grid, kw, 'eval_params') is kw
    with pytest.raises(ValueError, match="rplanet comes from the atmosphere's free 'rplanet'"):
        free_rplanet(atm, params, grid, {'rplanet': params[:, 0]}, 'eval_params')


def test_engine_exports():
    import pyratbay_amd.engine as engine
    assert engine.Observation is observation.Observation
    assert engine.StellarGrid is observation.StellarGrid
    assert hasattr(engine.TableSpectrum, 'eval_loglike')
    assert hasattr(engine.PassBands, 'set_eclipse_grid')
