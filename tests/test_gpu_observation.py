"""The exit of the batched loop towards the sampler on the device (csrc/pb_observation.hip,
pyratbay_amd/observation.py): pb_loglike_obs against its host statement and fixture G25;
pb_star_band_scale_batch against the route it replaces -- set_eclipse(rplanet, rstar,
star_bandflux(grid.flux_host(t))) + integrate_batch, one walker at a time -- BIT FOR BIT, against
the host statement with a planet radius per walker and against G25's reference values; eval_bands
with tstar / rplanet / f_dilution end to end, on poisoned memory too; eval_loglike; the launch
script of the new forms; the refusals."""
import numpy as np
import pytest

import cases
import observation_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def g25(golden):
    return golden('g25_observation')


def host(t):
    return t.cpu().numpy()


# -----------------------------------------------------------------------------------------------
# pb_loglike_obs
# -----------------------------------------------------------------------------------------------
def loglike_bound(obs, models, offsets, err_pars):
    """1e-13 (test_loglike_reference_fixture's factor) x the magnitude of the summed terms,
    0.5 sum r^2 + 0.5 sum |log(2 pi u^2)|, from the host statement: the two sums can cancel, and
    the device's pow is an ulp off libm's."""
    out = np.zeros(len(models))
    for w, m in enumerate(models):
        d = obs.offset_data_host(None if offsets is None else offsets[w])
        u = obs.scale_errors_host(obs.err_defaults if err_pars is None else err_pars[w])
        r = (d - m) / u
        out[w] = 1e-13 * (0.5 * np.sum(r**2) + 0.5 * np.sum(np.abs(np.log(2 * np.pi * u**2))))
    return out


def device_loglike(eng, obs, models, offsets, err_pars):
    return host(obs.loglike(eng.dev(models), None if offsets is None else eng.dev(offsets),
                            None if err_pars is None else eng.dev(err_pars)))


@pytest.mark.parametrize('nw', [1, 5])
@pytest.mark.parametrize('nb', [1, 63, 64, 65, 130])
def test_loglike_obs_against_the_host_statement(eng, nb, nw):
    """noff and nerr in 0 ... 3 (error models of alternating mode: both modes from nerr = 2 on)
    at the lane stride's edges."""
    for noff in range(4):
        for nerr in range(4):
            obs = oc.random_observation(eng, nb, noff, nerr, seed=100 * nb + 10 * noff + nerr)
            models, offsets, err_pars = oc.random_pars(obs, nw, seed=nb + nw)
            got = device_loglike(eng, obs, models, offsets, err_pars)
            want = obs.loglike_host(models, offsets, err_pars)
            bound = loglike_bound(obs, models, offsets, err_pars)
            err = np.abs(got - want)
            print(f'nb {nb} nw {nw} noff {obs.noff} nerr {obs.nerr}: max err / bound = '
                  f'{np.max(err / bound):.3g}')
            assert np.all(err <= bound), (noff, nerr, err, bound)
            if obs.noff == 0 and obs.nerr == 0:
                plain = eng.loglike(eng.dev(models), eng.dev(obs.data_host),
                                    eng.dev(obs.uncert_host))
                assert np.array_equal(got, host(plain))
            # None with models present: the defaults
            got0 = device_loglike(eng, obs, models, None, None)
            want0 = obs.loglike_host(models)
            assert np.all(np.abs(got0 - want0) <= loglike_bound(obs, models, None, None))


def test_loglike_obs_against_g25(eng, g25):
    obs = oc.observation_of(g25, eng)
    got = device_loglike(eng, obs, g25['models'], g25['offsets'], g25['err_pars'])
    bound = loglike_bound(obs, g25['models'], g25['offsets'], g25['err_pars'])
    print(got, g25['loglike'], bound)
    keep = np.arange(len(got)) != 4
    assert np.all(np.abs(got - g25['loglike'])[keep] <= bound[keep])
    assert got[4] == -1.0e98
    # the all-defaults row with its parameters left out
    got2 = device_loglike(eng, obs, g25['models'][2:3], None, None)
    assert abs(got2[0] - g25['loglike'][2]) <= bound[2]
    # one walker as a vector
    one = host(obs.loglike(eng.dev(g25['models'][0]), eng.dev(g25['offsets'][:1]),
                           eng.dev(g25['err_pars'][:1])))
    assert one.shape == (1,) and one[0] == got[0]


def test_loglike_obs_rejects(eng):
    """inf and NaN rows (a model value, an offset, an error parameter) give exactly -1e98; the
    other walkers keep their bits."""
    obs = oc.random_observation(eng, 65, 2, 2, seed=3)
    models, offsets, err_pars = oc.random_pars(obs, 6, seed=4)
    clean = device_loglike(eng, obs, models, offsets, err_pars)
    models[0, 64] = np.inf
    models[1, 3] = np.nan
    offsets[2, 1] = np.nan
    err_pars[3, 0] = np.inf
    got = device_loglike(eng, obs, models, offsets, err_pars)
    assert np.all(got[:4] == -1.0e98), got
    assert np.array_equal(got[4:], clean[4:]) and np.all(np.isfinite(clean))
    with pytest.raises(ValueError, match='offsets must be a float64 device tensor'):
        obs.loglike(eng.dev(models), eng.dev(offsets[:, :1]))
    with pytest.raises(ValueError, match='bandflux must be'):
        obs.loglike(eng.dev(models[:, :10]))
    with pytest.raises(ValueError, match='without such models'):
        eng.Observation(np.ones(65), np.ones(65)).loglike(eng.dev(models), eng.dev(offsets))


# -----------------------------------------------------------------------------------------------
# pb_star_band_scale_batch
# -----------------------------------------------------------------------------------------------
def frozen_route(eng, wn, bands, grid, planet_d, tstar, rplanet, rstar, f_dilution=None):
    """Today's route, one walker at a time: the host-interpolated stellar flux, its band fluxes,
    set_eclipse and integrate_batch -> [nw, nbands] (host).  rplanet: a scalar or [nw]."""
    out = []
    for w, t in enumerate(tstar):
        pb = eng.PassBands(wn, bands)
        rp = rplanet if np.ndim(rplanet) == 0 else rplanet[w]
        pb.set_eclipse(rp, rstar, pb.star_bandflux(grid.flux_host(t)))
        fd = None if f_dilution is None else eng.dev(f_dilution[w:w + 1])
        out.append(host(pb.integrate_batch(planet_d[w:w + 1], f_dilution=fd))[0])
    return np.array(out)


def host_statement(eng, wn, bands, grid, planet_d, tstar, rplanets, rstar, f_dilution):
    """k_band_scale's order with the factor of pyrat_obj.py:664-665 formed on the host: the band
    integrals are the device's (planet and star), the products NumPy's."""
    pb = eng.PassBands(wn, bands)
    v = host(pb.integrate_batch(planet_d))
    for w, t in enumerate(tstar):
        star = pb.star_bandflux(grid.flux_host(t))
        if f_dilution is not None:
            v[w] *= f_dilution[w]
        rprs = rplanets[w] / rstar
        v[w] *= rprs**2.0 / star
    return v


@pytest.mark.parametrize('nw', [1, 5])
@pytest.mark.parametrize('nt', [2, 3, 5])
def test_star_band_scale_bits_of_the_frozen_route(eng, nt, nw):
    """Bands of 2, 3, 255, 256, 257 and 600 samples on W = 700: the same IEEE operations in the
    same order as the route through host-interpolated flux, so the same bits; then a planet radius
    per walker against the host statement at 4e-16 (the one product that goes through libm's pow
    on the host), with and without dilution factors."""
    c = oc.star_case(nt, nw)
    grid = eng.StellarGrid(c['wn'], c['sed_temps'], c['fluxes'])
    planet_d = eng.dev(c['planet'])
    pb = eng.PassBands(c['wn'], c['bands']).set_eclipse_grid(c['rstar'], grid, c['rplanet'])
    tstar_d = eng.dev(c['tstar'])
    got = host(pb.integrate_batch(planet_d, tstar=tstar_d))
    want = frozen_route(eng, c['wn'], c['bands'], grid, planet_d, c['tstar'], c['rplanet'],
                        c['rstar'])
    assert np.all(np.isfinite(want)) and np.all(want > 0)
    assert np.array_equal(got, want)
    fd = eng.dev(c['f_dilution'])
    got = host(pb.integrate_batch(planet_d, f_dilution=fd, tstar=tstar_d))
    want = frozen_route(eng, c['wn'], c['bands'], grid, planet_d, c['tstar'], c['rplanet'],
                        c['rstar'], c['f_dilution'])
    assert np.array_equal(got, want)
    # a planet radius per walker
    for dil in (None, c['f_dilution']):
        got = host(pb.integrate_batch(planet_d, f_dilution=None if dil is None else fd,
                                      tstar=tstar_d, rplanet=eng.dev(c['rplanets'])))
        want = host_statement(eng, c['wn'], c['bands'], grid, planet_d, c['tstar'],
                              c['rplanets'], c['rstar'], dil)
        print(f'nt {nt} nw {nw}: rplanet[nw], max rel diff = {np.max(np.abs(got / want - 1)):.3g}')
        np.testing.assert_allclose(got, want, rtol=4e-16, atol=0)
    # without a planet radius anywhere
    bare = eng.PassBands(c['wn'], c['bands']).set_eclipse_grid(c['rstar'], grid)
    with pytest.raises(ValueError, match='planet radius'):
        bare.integrate_batch(planet_d, tstar=tstar_d)


def test_star_band_scale_against_g25(eng, g25):
    """Every tstar of G25 (all in range): the bits of the frozen route; the reference's
    band(starflux) and bandflux * rprs**2 / bandflux_star at 1e-13 (test_observables.py's
    tolerance for the reference's band integrals), for both radii."""
    wn, bands = g25['star_wn'], oc.star_bands(g25)
    grid = eng.StellarGrid(wn, g25['star_sed_temps'], g25['star_fluxes'])
    tstar, rstar = g25['star_tstar'], float(g25['star_rstar'])
    nw = len(tstar)
    plain = eng.PassBands(wn, bands)
    for w in range(nw):
        np.testing.assert_allclose(plain.star_bandflux(grid.flux_host(tstar[w])),
                                   g25['star_bandflux_star'][w], rtol=1e-13)
    # spectra whose band fluxes are the fixture's given planet band fluxes: constants
    # (a normalised band of a constant is the constant within rounding)
    for j, rp in enumerate(g25['star_rplanet']):
        pb = eng.PassBands(wn, bands).set_eclipse_grid(rstar, grid, rp)
        out = np.zeros((nw, len(bands)))
        for b in range(len(bands)):
            spectra = eng.dev(np.repeat(g25['star_planet_bandflux'][:, b:b + 1], len(wn), axis=1))
            got = host(pb.integrate_batch(spectra, tstar=eng.dev(tstar)))
            want = frozen_route(eng, wn, bands, grid, spectra, tstar, rp, rstar)
            assert np.array_equal(got, want)
            out[:, b] = got[:, b]
        print(f'rplanet {j}: max rel diff = '
              f'{np.max(np.abs(out / g25["star_eclipse_bandflux"][j] - 1)):.3g}')
        np.testing.assert_allclose(out, g25['star_eclipse_bandflux'][j], rtol=1e-13)


def test_star_band_scale_rejects(eng):
    """tstar below the grid, above it and NaN: +inf in every band; the other walkers of the batch
    keep their bits."""
    c = oc.star_case(3, 5)
    grid = eng.StellarGrid(c['wn'], c['sed_temps'], c['fluxes'])
    pb = eng.PassBands(c['wn'], c['bands']).set_eclipse_grid(c['rstar'], grid, c['rplanet'])
    planet_d = eng.dev(c['planet'])
    clean = host(pb.integrate_batch(planet_d, tstar=eng.dev(c['tstar'])))
    tstar = c['tstar'].copy()
    tstar[1] = np.nextafter(c['sed_temps'][0], 0.0)
    tstar[2] = np.nextafter(c['sed_temps'][-1], np.inf)
    tstar[3] = np.nan
    got = host(pb.integrate_batch(planet_d, tstar=eng.dev(tstar)))
    assert np.all(np.isposinf(got[1:4])), got
    assert np.array_equal(got[[0, 4]], clean[[0, 4]]) and np.all(np.isfinite(clean))
    with pytest.raises(ValueError, match='not on the wavenumbers'):
        eng.PassBands(c['wn'] + 1.0, c['bands']).set_eclipse_grid(c['rstar'], grid)


# -----------------------------------------------------------------------------------------------
# end to end: eval_bands with tstar, rplanet, f_dilution
# -----------------------------------------------------------------------------------------------
L, ITOP, W, NW = 17, 0, 256, 5


@pytest.fixture
def poison(monkeypatch):
    """poison(): from then to the end of the test torch.empty and torch.empty_like return
    poisoned memory (a call, so that a test can form its unpoisoned reference first)."""
    import torch
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.numel() == 0:
            return t
        if t.is_floating_point():
            t.fill_(float('nan'))
        elif t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
            t.fill_(torch.iinfo(t.dtype).min // 2)
        return t

    def empty(*args, **kw):
        return fill(real_empty(*args, **kw))

    def empty_like(*args, **kw):
        return fill(real_empty_like(*args, **kw))

    def start():
        monkeypatch.setattr(torch, 'empty', empty)
        monkeypatch.setattr(torch, 'empty_like', empty_like)
    return start


_E2E = {}


def e2e_case(eng):
    """cases.limited_table_model(17, 0, 256, opacity=100.0), its first 5 walkers, with a stellar
    grid of 4 nodes on its wavenumbers (built once, never changed)."""
    if not _E2E:
        m = cases.limited_table_model(L, ITOP, W, opacity=100.0)
        rng = np.random.default_rng(2500)
        sed_temps = np.array([4000.0, 4500.0, 5200.0, 6100.0])
        x = np.linspace(0.0, 1.0, W)
        fluxes = 2.0e5 * (sed_temps[:, None] / 5000.0)**3 * (1 + 0.2 * np.sin(7 * x)[None, :])
        m.update(sed_temps=sed_temps, fluxes=fluxes,
                 tstar=np.array([4000.0, 4321.0, 5200.0, 5999.5, 6100.0]),
                 rplanets=7.1e9 * rng.uniform(0.8, 1.3, NW),
                 f_dilution=rng.uniform(0.5, 1.0, NW),
                 et=eng.dev(m['etable']), td=eng.dev(m['temps'][:NW]),
                 dd=eng.dev(m['dens'][:NW]))
        m['grid'] = eng.StellarGrid(m['wn'], sed_temps, fluxes)
        _E2E.update(m)
    return _E2E


def e2e_model(eng, m, rt_path='emission'):
    return eng.TableSpectrum(m['et'], m['ttable'], m['wn'], m['radius0'], m['rstar'], itop=ITOP,
                             rt_path=rt_path, column_order=None)


def e2e_frozen(eng, m):
    """Per walker, the existing call with that walker's frozen factor."""
    model = e2e_model(eng, m)
    rows = []
    for w in range(NW):
        pb = eng.PassBands(m['wn'], m['bands'])
        pb.set_eclipse(m['rplanets'][w], m['rstar'],
                       pb.star_bandflux(m['grid'].flux_host(m['tstar'][w])))
        rows.append(model.eval_bands(m['td'][w:w + 1], m['dd'][w:w + 1], pb,
                                     f_dilution=eng.dev(m['f_dilution'][w:w + 1]))[0].clone())
    import torch
    return torch.stack(rows)


def e2e_call(eng, m, model=None):
    pb = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'])
    model = model or e2e_model(eng, m)
    return model.eval_bands(m['td'], m['dd'], pb, tstar=eng.dev(m['tstar']),
                            rplanet=eng.dev(m['rplanets']), f_dilution=eng.dev(m['f_dilution']),
                            chunk=2)


def test_eval_bands_with_tstar_rplanet_dilution(eng):
    """nw = 5 in chunks of 2, 2 and 1.  With a planet radius per walker the factor is t * t on
    the device and rprs**2.0 on the frozen route's host: the same bits wherever libm's pow(x, 2)
    is x * x rounded once -- asserted first, so that a failure names its cause."""
    import torch
    m = e2e_case(eng)
    for rp in m['rplanets']:
        t = rp / m['rstar']
        assert t**2.0 == t * t
    want = e2e_frozen(eng, m)
    got = e2e_call(eng, m)
    assert bool(torch.isfinite(want).all()) and bool((want > 0).all())
    assert torch.equal(got, want)
    # a rejected stellar temperature inside eval_bands: that walker alone
    pb = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'])
    tstar = m['tstar'].copy()
    tstar[2] = 9000.0
    bad = e2e_model(eng, m).eval_bands(m['td'], m['dd'], pb, tstar=eng.dev(tstar),
                                       rplanet=eng.dev(m['rplanets']),
                                       f_dilution=eng.dev(m['f_dilution']), chunk=2)
    assert bool(torch.isposinf(bad[2]).all())
    keep = [0, 1, 3, 4]
    assert torch.equal(bad[keep], want[keep])


def test_eval_bands_with_tstar_on_poisoned_memory(eng, poison):
    import torch
    m = e2e_case(eng)
    want = e2e_call(eng, m).clone()
    poison()
    assert bool(torch.isnan(torch.empty(3, dtype=torch.float64, device='cuda')).all())
    got = e2e_call(eng, m)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_eval_bands_two_stream_with_tstar(eng):
    """The same exit in two-stream geometry: the call with a grid against the frozen factor."""
    import torch
    m = e2e_case(eng)
    model = e2e_model(eng, m, 'two_stream')
    pb = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'], 7.1e9)
    got = model.eval_bands(m['td'], m['dd'], pb, tstar=eng.dev(m['tstar']), chunk=3)
    for w in range(NW):
        one = eng.PassBands(m['wn'], m['bands'])
        one.set_eclipse(7.1e9, m['rstar'], one.star_bandflux(m['grid'].flux_host(m['tstar'][w])))
        want = model.eval_bands(m['td'][w:w + 1], m['dd'][w:w + 1], one)
        assert torch.equal(got[w], want[0]), w


# -----------------------------------------------------------------------------------------------
# eval_loglike and the free rplanet of eval_params
# -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def params_case(eng, golden):
    """test_gpu_atmosphere's spectrum case (L = 12, W = 1000, 'rplanet' free, walkers 1 and
    nw - 2 rejected by the atmosphere) in emission geometry, with a stellar grid and an
    Observation with 2 offset and 2 error models on its 3 bands."""
    import test_gpu_atmosphere as atm_setup
    import test_gpu_batch_continuum as base
    from pyratbay_amd import atmosphere as pa
    nw = 5
    s = atm_setup.spectrum_case(eng, pa, golden('g7_continuum'), nw, 77, False, False)
    wn = s['wn']
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, s['base_radius'], 8.8e10,
                              rt_path='emission', column_order=None)
    bands, _ = base.make_bands(eng, wn)
    sed_temps = np.array([4000.0, 5000.0, 6500.0])
    x = np.linspace(0.0, 1.0, len(wn))
    fluxes = 2.0e5 * (sed_temps[:, None] / 5000.0)**3 * (1 + 0.2 * np.sin(7 * x)[None, :])
    grid = eng.StellarGrid(wn, sed_temps, fluxes)
    rng = np.random.default_rng(7)
    tstar = rng.uniform(4000.0, 6500.0, nw)
    params = eng.dev(s['params'])
    pb = eng.PassBands(wn, bands).set_eclipse_grid(8.8e10, grid)
    flux = host(model.eval_params(s['atm'], params, pb, tstar=eng.dev(tstar), chunk=2))
    data = flux[0] * (1 + rng.normal(0, 0.02, 3))
    obs = eng.Observation(data, 0.03 * flux[0], ['nrs1', 'nrs2', 'miri'],
                          ['offset_nrs1', 'offset_miri'], ['err_scale_nrs2', 'err_quad_miri'],
                          units='ppm')
    offsets = rng.uniform(-1.0, 1.0, (nw, 2)) * np.max(flux[0]) * 1e4
    err_pars = np.stack([rng.uniform(-0.3, 0.5, nw),
                         np.log10(np.max(flux[0]) * 1e6 * rng.uniform(0.01, 0.05, nw))], axis=1)
    return dict(s=s, model=model, bands=bands, grid=grid, pb=pb, tstar=tstar, params=params,
                flux=flux, obs=obs, offsets=offsets, err_pars=err_pars, nw=nw)


def test_eval_params_takes_the_free_rplanet(eng, params_case):
    """'rplanet' is free in the atmosphere and the bands carry a grid: eval_params passes that
    column as rplanet; the same call through eval_bands with the column given; passing rplanet
    as well is refused."""
    import torch
    c = params_case
    atm, params, model = c['s']['atm'], c['params'], c['model']
    col = atm.par_scalar['rplanet']
    assert col >= 0
    prof = atm.evaluate(params)
    tstar_d = eng.dev(c['tstar'])
    want = model.eval_bands(prof.temps, prof.dens, c['pb'], radius=prof.radius, tstar=tstar_d,
                            rplanet=params[:, col].contiguous(), chunk=2)
    assert torch.equal(torch.as_tensor(c['flux']), want.cpu())
    assert [w for w in range(c['nw']) if np.isposinf(c['flux'][w]).all()] == c['s']['rejected']
    assert np.all(np.isfinite(np.delete(c['flux'], c['s']['rejected'], axis=0)))
    with pytest.raises(ValueError, match="comes from the atmosphere's free 'rplanet'"):
        model.eval_params(atm, params, c['pb'], tstar=tstar_d, rplanet=params[:, col].contiguous())
    # bands without a grid: nothing is added, today's call
    plain = eng.PassBands(c['s']['wn'], c['bands'])
    assert torch.equal(model.eval_params(atm, params, plain, chunk=2),
                       model.eval_bands(prof.temps, prof.dens, plain, radius=prof.radius, chunk=2))


def test_eval_loglike(eng, params_case):
    """eval_loglike = observation.loglike(eval_params(...)), bit for bit; against the host
    statement on the band fluxes within the kernel's bound; rejected walkers: -1e98."""
    import torch
    c = params_case
    atm, params, model, obs = c['s']['atm'], c['params'], c['model'], c['obs']
    kw = dict(tstar=eng.dev(c['tstar']), chunk=2)
    off_d, err_d = eng.dev(c['offsets']), eng.dev(c['err_pars'])
    got = model.eval_loglike(atm, params, c['pb'], obs, offsets=off_d, err_pars=err_d, **kw)
    want = obs.loglike(model.eval_params(atm, params, c['pb'], **kw), off_d, err_d)
    assert torch.equal(got, want)
    got = host(got)
    rejected = c['s']['rejected']
    assert np.all(got[rejected] == -1.0e98)
    live = [w for w in range(c['nw']) if w not in rejected]
    ref = obs.loglike_host(c['flux'][live], c['offsets'][live], c['err_pars'][live])
    bound = loglike_bound(obs, c['flux'][live], c['offsets'][live], c['err_pars'][live])
    assert np.all(np.isfinite(ref)) and np.all(ref > -1e90)
    assert np.all(np.abs(got[live] - ref) <= bound), (got[live], ref, bound)
    # the defaults
    got0 = host(model.eval_loglike(atm, params, c['pb'], obs, **kw))
    ref0 = obs.loglike_host(c['flux'][live])
    assert np.all(np.abs(got0[live] - ref0) <= loglike_bound(obs, c['flux'][live], None, None))
    with pytest.raises(ValueError, match='data points'):
        model.eval_loglike(atm, params, c['pb'], eng.Observation(np.ones(2), np.ones(2)), **kw)


# -----------------------------------------------------------------------------------------------
# the launch script
# -----------------------------------------------------------------------------------------------
class Recorder:
    """The library handle with every call of a pb_* entry noted in `log`."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)              # (AttributeError: an entry the build lacks)
        if not name.startswith('pb_') or name == 'pb_last_error' or \
                name.endswith(('_work_doubles', '_supported')):
            return fn

        def noted(*args):
            self._log.append(name)
            return fn(*args)
        return noted


def recorded(monkeypatch, run):
    """run() before and after the proxy is installed -> (the entries the second run called, the
    first run's result, the second's)."""
    from pyratbay_amd import _capi
    before = run().clone()
    log = []
    monkeypatch.setattr(_capi, '_lib', Recorder(_capi.lib(), log))
    after = run().clone()
    monkeypatch.undo()
    return log, before, after


CHUNK = ['pb_interp_ec_batch', 'pb_emission_flux_batch', 'pb_band_integrate_batch']


def test_launch_script_of_an_eclipse_call(eng, monkeypatch):
    """Two chunks (3 + 2 walkers).  Frozen factor (set_eclipse), no tstar: the bands still end in
    pb_band_integrate_batch, pb_band_scale; with a grid and tstar: pb_band_integrate_batch,
    pb_star_band_scale_batch."""
    import torch
    m = e2e_case(eng)
    model = e2e_model(eng, m)
    frozen = eng.PassBands(m['wn'], m['bands'])
    frozen.set_eclipse(7.1e9, m['rstar'], frozen.star_bandflux(m['grid'].flux_host(5000.0)))
    log, before, after = recorded(
        monkeypatch, lambda: model.eval_bands(m['td'], m['dd'], frozen, chunk=3, streams=1))
    assert torch.equal(before, after)
    assert log == 2 * (CHUNK + ['pb_band_scale']) + ['pb_reject_walkers'], log
    pb = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'], 7.1e9)
    tstar = eng.dev(m['tstar'])
    log, before, after = recorded(
        monkeypatch, lambda: model.eval_bands(m['td'], m['dd'], pb, tstar=tstar, chunk=3,
                                              streams=1))
    assert torch.equal(before, after)
    assert log == 2 * (CHUNK + ['pb_star_band_scale_batch']) + ['pb_reject_walkers'], log


def test_launch_script_of_eval_loglike(eng, params_case, monkeypatch):
    """eval_loglike = eval_params' entries + exactly one pb_loglike_obs, and nothing is read back:
    no tensor leaves the device between the first launch and the result (Tensor.cpu / .item /
    .tolist / .numpy / __bool__ would)."""
    import torch
    c = params_case
    atm, params, model, obs = c['s']['atm'], c['params'], c['model'], c['obs']
    kw = dict(tstar=eng.dev(c['tstar']), chunk=3, streams=1)
    off_d, err_d = eng.dev(c['offsets']), eng.dev(c['err_pars'])
    log_p, _, _ = recorded(monkeypatch, lambda: model.eval_params(atm, params, c['pb'], **kw))
    assert log_p[-3:] == ['pb_band_integrate_batch', 'pb_star_band_scale_batch',
                          'pb_reject_walkers'], log_p
    reads = []

    def spy(name):
        real = getattr(torch.Tensor, name)

        def wrapped(self, *a, **k):
            if self.is_cuda:
                reads.append(name)
            return real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
        spy(name)
    log_l, before, after = recorded(
        monkeypatch, lambda: model.eval_loglike(atm, params, c['pb'], obs, offsets=off_d,
                                                err_pars=err_d, **kw))
    assert reads == [], reads
    assert log_l == log_p + ['pb_loglike_obs'], log_l
    assert torch.equal(before, after)


# -----------------------------------------------------------------------------------------------
# the refusals, on the device
# -----------------------------------------------------------------------------------------------
def test_refusals(eng):
    m = e2e_case(eng)
    model = e2e_model(eng, m)
    plain = eng.PassBands(m['wn'], m['bands'])
    with_grid = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'], 7.1e9)
    no_radius = eng.PassBands(m['wn'], m['bands']).set_eclipse_grid(m['rstar'], m['grid'])
    tstar, rplanet = eng.dev(m['tstar']), eng.dev(m['rplanets'])
    td, dd = m['td'], m['dd']
    transit = e2e_model(eng, m, 'transit')
    hires = eng.HiresData(m['wn'], m['wn'][60:200] + 0.013, 25000.0, rv_max=10.0)
    log = []
    from pyratbay_amd import _capi
    real = _capi._lib
    _capi._lib = Recorder(_capi.lib(), log)
    try:
        with pytest.raises(ValueError, match='need a stellar SED grid'):
            model.eval_bands(td, dd, plain, tstar=tstar)
        with pytest.raises(ValueError, match=r'tstar\[nw\] is needed'):
            model.eval_bands(td, dd, with_grid)
        with pytest.raises(ValueError, match='rplanet needs tstar'):
            model.eval_bands(td, dd, with_grid, rplanet=rplanet)
        with pytest.raises(ValueError, match='a planet radius is needed'):
            model.eval_bands(td, dd, no_radius, tstar=tstar)
        for kw in (dict(tstar=tstar), dict(rplanet=rplanet)):
            with pytest.raises(ValueError, match='HiresData'):
                model.eval_bands(td, dd, hires, **kw)
            with pytest.raises(ValueError, match='transit geometry'):
                transit.eval_bands(td, dd, with_grid, **kw)
        for bad in (tstar[:3], tstar.float(), m['tstar']):
            with pytest.raises(ValueError, match='eval_bands: tstar must be a float64 device'):
                model.eval_bands(td, dd, with_grid, tstar=bad)
        with pytest.raises(ValueError, match='eval_bands: rplanet must be a float64 device'):
            model.eval_bands(td, dd, with_grid, tstar=tstar, rplanet=rplanet[:2])
    finally:
        _capi._lib = real
    assert log == [], log                   # refused before any launch
