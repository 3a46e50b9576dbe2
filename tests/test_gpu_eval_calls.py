"""The launch script of a chunk of TableSpectrum.eval_bands: which entries of the C ABI one call
reaches, in which order, per form of the batch -- grid order, depth order, depth order with layer
limits and their gated repair (both geometries), two-stream, with a Continuum, with a cloud deck
and patchy clouds, shared and per-walker radius, PassBands and HiresData with rv.

A thin proxy stands in for the loaded library handle (_capi._lib): attribute access goes through
to the real functions, every CALL of an entry is noted by name (_capi.call and the direct
lib().pb_*_work_doubles look-ups both pass through it; the *_work_doubles / *_supported queries
launch nothing and are left out).  Every case is one eval_bands call of two chunks (chunk = half
the walkers, rounded up) on the caller's stream.  The expected sequences below were recorded by
running this file at commit 2d309e3, before eval_bands was split into validate / plan / run; a
second assertion per case: the band fluxes have the bits of the same call made before the proxy
was installed."""
import numpy as np
import pytest

import cases
import test_gpu_batch_clouds as clouds_setup
import test_gpu_batch_continuum as continuum_setup
import test_gpu_batch_two_stream as two_stream_setup

pytestmark = pytest.mark.gpu

L, ITOP, W = 17, 0, 256             # the smallest shape with two row tiles (test_gpu_batch_memory)
OPACITY = {'emission': 100.0, 'transit': 1.0}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


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


# ---------------------------------------------------------------------------------------------
# the cases: name -> a function(eng) that returns run()
# ---------------------------------------------------------------------------------------------
def limited_case(eng, rt_path, order, radius=False, hires=False, dilution=False):
    """cases.limited_table_model(17, 0, 256); order: None (grid), 'ordered' (depth order, no
    limits) or 'limited' (tile_margin = 0: limits and the gated repair)."""
    m = cases.limited_table_model(L, ITOP, W, opacity=OPACITY[rt_path])
    model = eng.TableSpectrum(eng.dev(m['etable']), m['ttable'], m['wn'], m['radius0'],
                              m['rstar'], itop=ITOP, rt_path=rt_path,
                              column_order=None if order is None else 'auto')
    model.tile_margin = 0 if order == 'limited' else -1
    td, dd = eng.dev(m['temps']), eng.dev(m['dens'])
    kw = dict(chunk=-(-m['nw'] // 2), streams=1)
    if radius:
        kw['radius'] = eng.dev(m['radius'])
    if dilution:
        kw['f_dilution'] = eng.dev(np.linspace(0.5, 1.0, m['nw']))
    if hires:
        bands = eng.HiresData(m['wn'], m['wn'][60:200] + 0.013, 25000.0, rv_max=10.0)
        kw['rv'] = eng.dev(np.linspace(-8.0, 8.0, m['nw']))
    else:
        bands = eng.PassBands(m['wn'], m['bands'])

    def run():
        out = model.eval_bands(td, dd, bands, **kw)
        assert (model.column_order is not None) == (order is not None)
        assert (model.tile_limit is not None) == (order == 'limited')
        return out
    return run


def two_stream_case(eng, hires=False):
    c = two_stream_setup.case()
    model = two_stream_setup.make_model(eng)
    td, dd, rd = two_stream_setup.device_walkers(eng)
    kw = dict(radius=rd, chunk=-(-two_stream_setup.NW // 2), streams=1)
    if hires:
        bands = two_stream_setup.hires_data(eng)
        kw['rv'] = eng.dev(c['rv'])
    else:
        bands = eng.PassBands(c['wn'], c['bands'])
    return lambda: model.eval_bands(td, dd, bands, **kw)


def continuum_case(eng, golden, rt_path):
    nw = 6
    s = continuum_setup.setup(golden('g7_continuum'), nw, L=20, seed=77)
    radius0 = np.linspace(8.0e9, 7.0e9, 20)
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], radius0, 8.8e10,
                              rt_path=rt_path, continuum=s['cont'], column_order=None)
    _, pb = continuum_setup.make_bands(eng, s['wn'])
    td, dd = eng.dev(s['temps']), eng.dev(s['dens'])
    kw = dict(continuum_density=eng.dev(s['cdens']), continuum_pars=eng.dev(s['pars']),
              chunk=nw // 2, streams=1)
    return lambda: model.eval_bands(td, dd, pb, **kw)


def clouds_case(eng, golden, geom, radius):
    """A deck and f_patchy per walker, the haze and the gray cloud as cloud-type models."""
    nw = 6
    s = clouds_setup.build_case(golden('g11_patchy'), nw, 11, geom)
    cont = clouds_setup.continuum_of(s, True, True)
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0],
                              clouds_setup.RSTAR, rt_path=geom, continuum=cont, column_order=None)
    _, pb = clouds_setup.make_bands(eng, s['wn'])
    td, dd = eng.dev(s['temps']), eng.dev(s['dens'])
    kw = dict(chunk=nw // 2, streams=1, continuum_density=eng.dev(s['cdens']),
              continuum_pars=eng.dev(s['pars']), deck_logp=eng.dev(s['logp']),
              f_patchy=eng.dev(s['fpatchy']))
    if radius:
        kw['radius'] = eng.dev(s['radius'])
    return lambda: model.eval_bands(td, dd, pb, **kw)


CASES = {
    'transit_grid_shared_radius': lambda eng, golden: limited_case(eng, 'transit', None),
    'transit_grid_radius_per_walker': lambda eng, golden: limited_case(eng, 'transit', None,
                                                                       radius=True),
    'transit_grid_hires_rv': lambda eng, golden: limited_case(eng, 'transit', None, hires=True),
    'emission_grid': lambda eng, golden: limited_case(eng, 'emission', None),
    'emission_grid_dilution_radius': lambda eng, golden: limited_case(
        eng, 'emission', None, radius=True, dilution=True),
    'transit_ordered': lambda eng, golden: limited_case(eng, 'transit', 'ordered'),
    'emission_ordered': lambda eng, golden: limited_case(eng, 'emission', 'ordered'),
    'transit_limited': lambda eng, golden: limited_case(eng, 'transit', 'limited'),
    'transit_limited_radius_per_walker': lambda eng, golden: limited_case(
        eng, 'transit', 'limited', radius=True),
    'emission_limited': lambda eng, golden: limited_case(eng, 'emission', 'limited'),
    'emission_limited_hires_rv_dilution': lambda eng, golden: limited_case(
        eng, 'emission', 'limited', hires=True, dilution=True),
    'two_stream': lambda eng, golden: two_stream_case(eng),
    'two_stream_hires_rv': lambda eng, golden: two_stream_case(eng, hires=True),
    'transit_continuum': lambda eng, golden: continuum_case(eng, golden, 'transit'),
    'emission_continuum': lambda eng, golden: continuum_case(eng, golden, 'emission'),
    'transit_clouds_shared_radius': lambda eng, golden: clouds_case(eng, golden, 'transit', False),
    'transit_clouds_radius_per_walker': lambda eng, golden: clouds_case(eng, golden, 'transit',
                                                                        True),
    'emission_clouds': lambda eng, golden: clouds_case(eng, golden, 'emission', True),
}

# what one chunk calls, by case (recorded at 2d309e3); an eval_bands call of two chunks is
# [pb_transit_path, if the radius is shared in transit geometry] + 2 x chunk + [pb_reject_walkers]
PATH, REJECT = 'pb_transit_path', 'pb_reject_walkers'
BANDS, HIRES = 'pb_band_integrate_batch', 'pb_hires_observe_batch'
LIMITED_TRANSIT = 2 * ['pb_interp_ec_batch_limited', 'pb_transit_spectrum_limited']
LIMITED_EMISSION = 2 * ['pb_interp_ec_batch_limited', 'pb_emission_flux_limited']
CLOUDS = ['pb_interp_ec_batch_cont', 'pb_deck_state_batch', 'pb_cloud_plan']
CHUNK = {
    'transit_grid_shared_radius': ['pb_interp_ec_batch', 'pb_transit_spectrum_batch', BANDS],
    'transit_grid_radius_per_walker': ['pb_interp_ec_batch', PATH, 'pb_transit_spectrum_batch',
                                       BANDS],
    'transit_grid_hires_rv': ['pb_interp_ec_batch', 'pb_transit_spectrum_batch', HIRES],
    'emission_grid': ['pb_interp_ec_batch', 'pb_emission_flux_batch', BANDS],
    'emission_grid_dilution_radius': ['pb_interp_ec_batch', 'pb_emission_flux_batch', BANDS,
                                      'pb_band_scale'],
    'transit_ordered': ['pb_interp_ec_batch', 'pb_transit_spectrum_ordered', BANDS],
    'emission_ordered': ['pb_interp_ec_batch', 'pb_emission_flux_ordered', BANDS],
    'transit_limited': LIMITED_TRANSIT + [BANDS],
    'transit_limited_radius_per_walker': ['pb_interp_ec_batch_limited', PATH,
                                          'pb_transit_spectrum_limited',
                                          'pb_interp_ec_batch_limited',
                                          'pb_transit_spectrum_limited', BANDS],
    'emission_limited': LIMITED_EMISSION + [BANDS],
    'emission_limited_hires_rv_dilution': LIMITED_EMISSION + [HIRES],
    'two_stream': ['pb_interp_ec_batch', 'pb_two_stream_batch', BANDS],
    'two_stream_hires_rv': ['pb_interp_ec_batch', 'pb_two_stream_batch', HIRES],
    'transit_continuum': ['pb_interp_ec_batch_cont', 'pb_transit_spectrum_batch', BANDS],
    'emission_continuum': ['pb_interp_ec_batch_cont', 'pb_emission_flux_batch', BANDS],
    'transit_clouds_shared_radius': CLOUDS + ['pb_cloudy_transit_batch', BANDS],
    'transit_clouds_radius_per_walker': CLOUDS + [PATH, 'pb_cloudy_transit_batch', BANDS],
    'emission_clouds': CLOUDS + ['pb_cloudy_emission_batch', BANDS],
}
SHARED_PATH = ('transit_grid_shared_radius', 'transit_grid_hires_rv', 'transit_ordered',
               'transit_limited', 'transit_continuum', 'transit_clouds_shared_radius')


def expected(name):
    head = [PATH] if name in SHARED_PATH else []
    return head + 2 * list(CHUNK[name]) + [REJECT]


@pytest.mark.parametrize('name', list(CASES))
def test_launch_script(eng, golden, monkeypatch, name):
    import torch
    run = CASES[name](eng, golden)
    log, before, after = recorded(monkeypatch, run)
    print(f'{name}: {log}')
    assert bool(torch.isfinite(before).all())
    assert torch.equal(after, before)
    assert log == expected(name), name
