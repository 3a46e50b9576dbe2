"""The posterior summary on the device (pyratbay_amd/posterior.py, TableSpectrum.posterior_summary)
and the `spectra_out` keyword of TableSpectrum.eval_bands it rests on, on the tiny models of the
other batch tests: five unique samples with counts [3, 1, 4, 1, 2] in chunks of 2 (2 + 2 + 1: the
seams of the transposed stores), in transit, emission and two-stream geometry and with a
Continuum, a cloud deck and patchy clouds.

Tolerances of spectra_out against the one-walker eval(): those test_gpu_batch.py and
test_gpu_batch_two_stream.py hold the band fluxes of the same two paths to -- 1e-13 (transit),
1e-14 (emission), equal bits (two-stream).  Everything about the quantiles is for equal values."""
import numpy as np
import pytest

import cases
import test_gpu_atmosphere as tatm
import test_gpu_batch_continuum as tcont
import test_gpu_batch_two_stream as tts
from pyratbay_amd import posterior as post

pytestmark = pytest.mark.gpu

COUNTS = np.array([3, 1, 4, 1, 2])
CHUNK = 2
EVAL_RTOL = {'transit': 1e-13, 'emission': 1e-14}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


@pytest.fixture(scope='module')
def g7(golden):
    return golden('g7_continuum')


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------ eval_bands(spectra_out)
@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_spectra_out_in_grid_order_on_every_branch(eng, rt_path):
    """limited_table_model(33, 2, 700), 9 walkers in chunks of 4 with their own radius profiles:
    grid order (the plain batch kernels), column_order='auto' with tile_margin = 0 (the ordered
    kernels under layer limits, walkers 3 and 5 run past them: the gated repair) and a given
    permutation (the ordered kernels).  spectra_out has the same bits under all three, is the
    spectrum eval() returns, integrates to the band fluxes the call returned, and leaves those
    band fluxes as they are without it."""
    import torch
    m = cases.limited_table_model(33, 2, 700, opacity=1.0 if rt_path == 'transit' else 0.02)
    nw, W = m['nw'], m['nwave']
    pb = eng.PassBands(m['wn'], m['bands'])
    td, dd, rd = eng.dev(m['temps']), eng.dev(m['dens']), eng.dev(m['radius'])
    spectra, flux = {}, {}
    for name, order in (('grid', None), ('auto', 'auto'),
                        ('given', np.random.default_rng(2).permutation(W))):
        model = eng.TableSpectrum(m['etable'], m['ttable'], m['wn'], m['radius0'], m['rstar'],
                                  itop=m['itop'], rt_path=rt_path, column_order=order)
        model.tile_margin = 0
        plain = model.eval_bands(td, dd, pb, radius=rd, chunk=4).clone()
        out = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
        flux[name] = model.eval_bands(td, dd, pb, radius=rd, chunk=4, spectra_out=out).clone()
        assert torch.equal(flux[name], plain), name
        assert (model.column_order is None) == (name == 'grid')
        if name == 'auto' and rt_path == 'transit':
            assert model.tile_limit is not None
        assert bool(torch.isfinite(out).all())
        assert torch.equal(pb.integrate_batch(out), plain), name
        spectra[name] = out
    assert torch.equal(spectra['auto'], spectra['grid'])
    assert torch.equal(spectra['given'], spectra['grid'])
    assert torch.equal(flux['auto'], flux['grid']) and torch.equal(flux['given'], flux['grid'])
    model = eng.TableSpectrum(m['etable'], m['ttable'], m['wn'], m['radius0'], m['rstar'],
                              itop=m['itop'], rt_path=rt_path, column_order=None)
    got = host(spectra['grid'])
    for w in (0, 3, 5, 8):
        model.set_radius(m['radius'][w])
        one = host(model.eval(m['temps'][w], dd[w]))
        np.testing.assert_allclose(got[w], one, rtol=EVAL_RTOL[rt_path], atol=0, err_msg=f'{w}')
    with pytest.raises(ValueError, match='spectra_out'):
        model.eval_bands(td, dd, pb, radius=rd, spectra_out=out[:, :-1])
    with pytest.raises(ValueError, match='spectra_out'):
        model.eval_bands(td, dd, pb, radius=rd, spectra_out=out.cpu())


def test_spectra_out_two_stream(eng):
    """Two-stream geometry (7 walkers in chunks of 3): the bits of eval()'s flux_up[0]."""
    import torch
    c = tts.case()
    td, dd, rd = tts.device_walkers(eng)
    pb = eng.PassBands(c['wn'], c['bands'])
    model = tts.make_model(eng)
    plain = model.eval_bands(td, dd, pb, radius=rd, chunk=tts.CHUNK).clone()
    out = torch.full((tts.NW, tts.W), float('nan'), dtype=torch.float64, device='cuda')
    flux = model.eval_bands(td, dd, pb, radius=rd, chunk=tts.CHUNK, spectra_out=out)
    assert torch.equal(flux, plain)
    for w in range(tts.NW):
        model.set_radius(c['radius'][w])
        assert torch.equal(out[w], model.eval(c['temps'][w], dd[w])), w


@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_spectra_out_with_clouds(eng, pa, g7, rt_path):
    """Rayleigh + CIA + H- + Na/K, a cloud deck at per-walker pressures and patchy clouds (the
    cloud branch of eval_bands), grid order and column_order='auto': the same bits, and the
    spectra integrate to the band fluxes the call returned."""
    import torch
    nw = 7
    s = tatm.spectrum_case(eng, pa, g7, nw, 77, True, True)
    _, pb = tcont.make_bands(eng, s['wn'])
    prof = s['atm'].evaluate(eng.dev(s['params']))
    rng = np.random.default_rng(5)
    kw = dict(radius=prof.radius, chunk=3, continuum_density=prof.continuum_density,
              alkali_density=prof.alkali_density, deck_logp=eng.dev(rng.uniform(-3.0, 0.5, nw)),
              f_patchy=eng.dev(rng.uniform(0.1, 0.9, nw)))
    good = [w for w in range(nw) if w not in s['rejected']]
    spectra = {}
    for order in (None, 'auto'):
        model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['base_radius'], 8.8e10,
                                  rt_path=rt_path, continuum=s['cont'], column_order=order)
        plain = model.eval_bands(prof.temps, prof.dens, pb, **kw).clone()
        out = torch.full((nw, len(s['wn'])), float('nan'), dtype=torch.float64, device='cuda')
        flux = model.eval_bands(prof.temps, prof.dens, pb, spectra_out=out, **kw)
        assert torch.equal(flux, plain)
        assert (model.column_order is None) == (order is None)
        assert bool(torch.isfinite(out[good]).all())
        assert torch.equal(pb.integrate_batch(out[good].contiguous()), plain[good])
        spectra[order] = out[good]
    assert torch.equal(spectra[None], spectra['auto'])


# ----------------------------------------------------------------------------- posterior_summary
def atmosphere_case(eng, pa, g7, geometry):
    """(model, atmosphere, params[5, npar] on the host, bands, keywords) of a geometry."""
    if geometry == 'two_stream':
        c = tts.case()
        pressure = np.logspace(-2, 0, tts.L)
        species, mass = ['H2', 'He', 'H2O', 'CO'], [2.01588, 4.002602, 18.01528, 28.0101]
        vmr = np.tile([0.85, 0.149, 4e-4, 5e-4], (tts.L, 1))
        base_params = np.array([1400.0, -3.4, -3.3])
        atm = pa.WalkerAtmosphere(pressure, species, mass, vmr, ['H2', 'He'],
                                  pa.Isothermal(pressure),
                                  [pa.IsoVMR('H2O', pressure), pa.IsoVMR('CO', pressure)],
                                  rmodel='hydro_m', mplanet=1.5e30, rplanet=7.4e9,
                                  refpressure=0.1, free=['T_iso', 'log_H2O', 'log_CO'],
                                  base_params=base_params)
        atm.bind(['H2O', 'CO'])
        params = base_params + np.array([400.0, 0.3, 0.3]) * \
            np.random.default_rng(9).uniform(-1, 1, (5, 3))
        model = tts.make_model(eng)
        model.set_radius(atm.base_radius)
        return model, atm, params, eng.PassBands(c['wn'], c['bands']), {}, 3000.0
    clouds = geometry.endswith('_clouds')
    rt_path = geometry.split('_')[0]
    s = tatm.spectrum_case(eng, pa, g7, 7, 77, clouds, clouds)
    params = s['params'][[0, 2, 3, 4, 6]]                   # (rows 1 and 5 are rejected ones)
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['base_radius'], 8.8e10,
                              rt_path=rt_path, continuum=s['cont'])
    kw = {}
    if clouds:
        rng = np.random.default_rng(5)
        kw = dict(deck_logp=eng.dev(rng.uniform(-3.0, 0.5, 5)),
                  f_patchy=eng.dev(rng.uniform(0.1, 0.9, 5)))
    return model, s['atm'], params, tcont.make_bands(eng, s['wn'])[1], kw, 9000.0


def expanded(store, inverse):
    """A sample-minor device store [..., n] -> the reference's models[uinv]: [N, ...]."""
    return np.moveaxis(host(store), -1, 0)[inverse]


@pytest.mark.parametrize('geometry', ['transit', 'emission', 'two_stream', 'transit_clouds'])
def test_posterior_summary(eng, pa, g7, geometry):
    """The four products against np.percentile of the expansion of the stores the same call
    filled, bit for bit; the stores against one eval_bands call over all five samples (the
    chunks' seams); the shapes; one sample outside the table's temperatures."""
    import torch
    model, atm, params, pb, kw, hot = atmosphere_case(eng, pa, g7, geometry)
    chain = np.repeat(params, COUNTS, axis=0)[np.random.default_rng(1).permutation(COUNTS.sum())]
    u_index, counts, inverse = post.unique_samples(chain)
    assert sorted(counts) == sorted(COUNTS) and len(u_index) == 5
    unique = eng.dev(chain[u_index])
    res = model.posterior_summary(atm, unique, counts, pb, chunk=CHUNK, keep_stores=True, **kw)
    nq, W, L = len(post.QUANTILES), model.nwave, model.nlayers
    nspec = model.nspec
    assert res.n_rejected == 0 and res.quantiles == post.QUANTILES
    assert res.spectrum.shape == (nq, W) and res.bands.shape == (nq, pb.nbands)
    assert res.temperature.shape == (nq, L) and res.vmr.shape == (nq, L, nspec)
    assert res.stores['spectrum'].shape == (W, 5) and res.stores['vmr'].shape == (L, nspec, 5)
    q100 = 100 * np.array(post.QUANTILES)
    for name in ('spectrum', 'bands', 'temperature', 'vmr'):
        got = host(getattr(res, name))
        assert np.all(np.isfinite(got)), name
        want = np.percentile(expanded(res.stores[name], inverse), q100, axis=0)
        assert np.array_equal(got, want), name
    assert np.all(host(res.vmr) > 0) and np.all(host(res.vmr) < 1)
    assert np.all(np.diff(host(res.spectrum)[[3, 1, 0, 2, 4]], axis=0) >= 0)
    # the stores: one call over the five samples, transposed
    prof = atm.evaluate(unique)
    ckw = dict(kw)
    if prof.continuum_density is not None:
        ckw.update(continuum_density=prof.continuum_density, alkali_density=prof.alkali_density)
    out = torch.empty((5, W), dtype=torch.float64, device='cuda')
    flux = model.eval_bands(prof.temps, prof.dens, pb, radius=prof.radius, chunk=5,
                            spectra_out=out, **ckw)
    assert torch.equal(res.stores['spectrum'], out.t())
    assert torch.equal(res.stores['bands'], flux.t())
    assert torch.equal(res.stores['temperature'], prof.temps.t())
    assert torch.equal(res.stores['counts'], eng.dev(counts, torch.int64))
    # the default chunk and no stores kept: the same summary
    again = model.posterior_summary(atm, unique, counts, pb, **kw)
    assert again.stores is None and torch.equal(again.spectrum, res.spectrum)
    assert torch.equal(again.vmr, res.vmr)
    # one sample outside the table's temperatures: count 0, the other four with their counts
    bad = chain[u_index].copy()
    bad[2, 0 if geometry == 'two_stream' else 4] = hot
    unique_bad = eng.dev(bad)
    pbad = atm.evaluate(unique_bad)
    assert int(pbad.reject[2]) == 0 and float(pbad.temps[2].max()) > model.tmax
    rej = model.posterior_summary(atm, unique_bad, counts, pb, chunk=CHUNK, keep_stores=True,
                                  **kw)
    assert rej.n_rejected == 1
    keep = np.array([0, 1, 3, 4])
    assert list(host(rej.stores['counts'])) == [counts[0], counts[1], 0, counts[3], counts[4]]
    for name in ('spectrum', 'bands', 'temperature', 'vmr'):
        store = np.moveaxis(host(rej.stores[name]), -1, 0)
        want = post.weighted_quantiles_host(store[keep], counts[keep], post.QUANTILES)
        assert np.array_equal(host(getattr(rej, name)), want), name
        full = store[keep][np.repeat(np.arange(4), counts[keep])]
        assert np.array_equal(want, np.percentile(full, q100, axis=0)), name
    assert np.all(np.isposinf(host(rej.stores['bands'])[:, 2]))


def test_every_sample_rejected_and_argument_checks(eng, pa, g7):
    model, atm, params, pb, kw, hot = atmosphere_case(eng, pa, g7, 'transit')
    unique = eng.dev(params)
    bad = params.copy()
    bad[:, 4] = hot
    with pytest.raises(ValueError, match='5 of 5 rejected'):
        model.posterior_summary(atm, eng.dev(bad), COUNTS, pb, chunk=CHUNK)
    with pytest.raises(ValueError, match='no sample is left'):
        model.posterior_summary(atm, unique, np.zeros(5, int), pb)
    with pytest.raises(ValueError, match='counts'):
        model.posterior_summary(atm, unique, COUNTS[:4], pb)
    with pytest.raises(ValueError, match='negative'):
        model.posterior_summary(atm, unique, -COUNTS, pb)
    with pytest.raises(ValueError, match='fractions'):
        model.posterior_summary(atm, unique, COUNTS, pb, quantiles=[0.5, 1.5])
    with pytest.raises(ValueError, match='radius'):
        model.posterior_summary(atm, unique, COUNTS, pb, radius=None)
    with pytest.raises(ValueError, match='one row per sample'):
        model.posterior_summary(atm, unique, COUNTS, pb, f_patchy=eng.dev(np.ones(4)))


def test_store_larger_than_free_memory(eng, pa, g7, monkeypatch):
    """The spectrum store is checked against the free device memory before anything is
    allocated: both numbers are in the message."""
    import torch
    model, atm, params, pb, kw, hot = atmosphere_case(eng, pa, g7, 'transit')
    unique = eng.dev(params)
    need = 8 * model.nwave * 5
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a: (need - 1, 10**12))

    def no_allocation(*a, **k):
        raise AssertionError('allocated before the check')
    monkeypatch.setattr(torch, 'empty', no_allocation)
    with pytest.raises(ValueError, match=f'{need} bytes, {need - 1} bytes'):
        model.posterior_summary(atm, unique, COUNTS, pb)
