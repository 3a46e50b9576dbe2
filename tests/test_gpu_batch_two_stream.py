"""The retrieval batch in two-stream geometry (TableSpectrum(rt_path='two_stream' /
'emission_two_stream' / 'eclipse_two_stream'): eval() and eval_bands / eval_params) on a small
table model: 2 species, 4 table temperatures, 12 layers, 300 samples, 7 walkers in chunks of 3.
Reference: pyrat/spectrum.py:388-390, 454-522; opacity/optic_depth.py:124-126.

The table values and densities are scaled so that every layer interval of every walker has an
optical depth between about 1e-3 and 5, where the reference's formula is well-conditioned
(docstring of test_two_stream.py); test_model_is_conditioned shows it on the CPU, oracle against
the NumPy restatement with scipy.special.exp1, before any GPU run."""
import functools

import numpy as np
import pytest

from test_gpu_two_stream_batch import close_by_column, numpy_two_stream

RTOL = 1e-11
S, NTEMP, L, W, NW, CHUNK = 2, 4, 12, 300, 7, 3
TINT, RSTAR, RPLANET = 300.0, 8.8e10, 7.4e9


@functools.lru_cache(maxsize=None)
def case():
    rng = np.random.default_rng(12)
    wn = 4000.0 + 0.05 * np.arange(W)
    ttable = np.linspace(500.0, 2500.0, NTEMP)
    radius0 = np.linspace(8.0e9, 7.0e9, L)
    etable = 10.0**rng.uniform(-24.5, -23.5, (S, NTEMP, L, 1)) * \
        10.0**rng.uniform(-0.5, 0.5, (S, 1, 1, W))
    temps = np.linspace(900.0, 1900.0, L)[None] * (1 + 0.1 * rng.uniform(-1, 1, (NW, 1))) + \
        rng.uniform(-20, 20, (NW, L))
    dens = 10.0**rng.uniform(14.5, 15.0, (NW, L, S))
    radius = radius0[None] * (1 + 0.01 * rng.uniform(-1, 1, (NW, 1))) + \
        np.linspace(0, 1, L)[None] * 2e7 * rng.uniform(-1, 1, (NW, 1))
    top = 10**rng.uniform(2, 4, W)
    starflux = 2.0e6 * (1.0 + 0.1 * np.sin(wn / 7.0))
    bands = [(1, np.ones(W - 2), 1.0),
             (W // 3, np.exp(-np.linspace(-1.5, 1.5, W // 2)**2), 0.5)]
    rv = rng.uniform(-8.0, 8.0, NW)
    fd = rng.uniform(0.5, 1.0, NW)
    return dict(wn=wn, ttable=ttable, radius0=radius0, etable=etable, temps=temps, dens=dens,
                radius=radius, top=top, starflux=starflux, bands=bands, rv=rv, fd=fd)


_ORACLE = {}


def oracle(orc, w):
    """(depth[L, W], flux_down, flux_up) of walker w: interp_ec -> depth without a stop ->
    two_stream, computed once."""
    if w not in _ORACLE:
        c = case()
        ec = np.zeros((L, W))
        orc.interp_ec(ec, c['etable'], c['ttable'], c['temps'][w], c['dens'][w], 0, L)
        depth, stop = np.zeros((L, W)), np.zeros(W, np.int32)
        orc.plane_parallel_optical_depth(depth, stop, ec, -np.diff(c['radius'][w]), np.inf, 0, L)
        f_int = orc.internal_flux(c['wn'], TINT)
        _ORACLE[w] = (depth,) + tuple(orc.two_stream(depth, c['wn'], c['temps'][w], f_int,
                                                     c['top'], 0))
    return _ORACLE[w]


def test_model_is_conditioned(orc):
    c = case()
    f_int = orc.internal_flux(c['wn'], TINT)
    for w in range(NW):
        depth, down, up = oracle(orc, w)
        dtau = np.diff(depth, axis=0)
        assert 1e-3 < dtau.min() and dtau.max() < 5.0, (dtau.min(), dtau.max())
        want = numpy_two_stream(depth, orc.blackbody_wn_2D(c['wn'], c['temps'][w]), f_int,
                                c['top'])
        close_by_column(down, want[0], RTOL)
        close_by_column(up, want[1], RTOL)


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def make_model(eng, rt_path='two_stream', **kw):
    c = case()
    kw.setdefault('tint', TINT)
    kw.setdefault('flux_top', c['top'])
    return eng.TableSpectrum(c['etable'], c['ttable'], c['wn'], c['radius0'], RSTAR,
                             rt_path=rt_path, **kw)


def device_walkers(eng):
    c = case()
    return eng.dev(c['temps']), eng.dev(c['dens']), eng.dev(c['radius'])


def hires_data(eng):
    c = case()
    return eng.HiresData(c['wn'], c['wn'][60:240] + 0.013, 25000.0, rv_max=10.0)


@pytest.mark.gpu
@pytest.mark.parametrize('rt_path', ['two_stream', 'emission_two_stream', 'eclipse_two_stream'])
def test_eval_vs_oracle(eng, orc, rt_path):
    """eval(): interpolation -> depth without the maxdepth stop -> two_stream; the spectrum is
    flux_up[0], flux_down / flux_up are kept, the timestamps have the reference's three keys."""
    c = case()
    model = make_model(eng, rt_path, maxdepth=10.0)
    assert model.rt_path == 'two_stream' and model.rt_path_name == rt_path
    assert model.observable == ('eclipse' if rt_path.startswith('eclipse') else 'emission')
    assert model.maxdepth == np.inf and not hasattr(model, 'mu')
    np.testing.assert_allclose(host(model.f_int), orc.internal_flux(c['wn'], TINT), rtol=1e-12)
    for w in range(NW):
        model.set_radius(c['radius'][w])
        spec = model.eval(c['temps'][w], c['dens'][w])
        depth, down, up = oracle(orc, w)
        assert np.array_equal(host(model.ideep), np.full(W, L - 1))
        np.testing.assert_allclose(host(model.depth), depth, rtol=1e-13)
        close_by_column(host(model.flux_down), down, RTOL)
        close_by_column(host(model.flux_up), up, RTOL)
        assert np.array_equal(host(spec), host(model.flux_up[0]))
        assert set(model.timestamps) == {'extinction', 'odepth', 'spectrum'}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['passbands', 'hires'])
def test_eval_bands_rows_are_one_walker_evals(eng, kind):
    """eval_bands row w has the bits of a one-walker eval() of the same model followed by the band
    integration of its spectrum (chunks of 3 for 7 walkers: a chunk keeps no cross-walker state);
    column_order='auto' orders nothing and copies no table, an explicit order is ignored."""
    import torch
    c = case()
    td, dd, rd = device_walkers(eng)
    if kind == 'passbands':
        bands, kw, one_kw = eng.PassBands(c['wn'], c['bands']), {}, lambda w: {}
    else:
        bands = hires_data(eng)
        rv = eng.dev(c['rv'])
        kw, one_kw = {'rv': rv}, lambda w: {'rv': rv[w:w + 1]}
    model = make_model(eng)
    got = model.eval_bands(td, dd, bands, radius=rd, chunk=CHUNK, **kw).clone()
    assert model.etable_ordered is None and model.column_order is None
    assert got.shape == (NW, bands.nbands) and bool(torch.isfinite(got).all())
    for w in range(NW):
        model.set_radius(c['radius'][w])
        spec = model.eval(c['temps'][w], dd[w])
        one = bands.integrate_batch(spec.view(1, -1).contiguous(), **one_kw(w))
        assert torch.equal(got[w], one[0]), f'walker {w}'
    whole = make_model(eng).eval_bands(td, dd, bands, radius=rd, chunk=NW, **kw)
    assert torch.equal(whole, got)
    given = make_model(eng, column_order=np.random.default_rng(1).permutation(W))
    assert torch.equal(given.eval_bands(td, dd, bands, radius=rd, chunk=CHUNK, **kw), got)
    assert given.etable_ordered is None
    # shared radius: the model's own
    shared = make_model(eng)
    got1 = shared.eval_bands(td, dd, bands, chunk=CHUNK, **kw)
    spec = shared.eval(c['temps'][4], dd[4])
    assert torch.equal(got1[4], bands.integrate_batch(spec.view(1, -1).contiguous(),
                                                      **one_kw(4))[0])


@pytest.mark.gpu
def test_with_a_continuum(eng):
    """A haze with per-walker parameters (Lecavelier) + Rayleigh H2 + one CIA pair in the store of
    the interpolation: eval_bands against eval() with the walker's parameters on the models.  The
    haze's 10**x and pow are the device's in one and NumPy's in the other (1e-14 in ec,
    test_gpu_batch_continuum.py), and from ec on the two take different roundings through 11
    intervals whose Bp bracket amplifies one by eps / dtau (dB / B): 11 * 2.2e-16 / 1e-3 * 0.5
    = 1.2e-12."""
    from pyratbay_amd import continuum as ct
    c = case()
    rng = np.random.default_rng(3)
    wn = c['wn']
    pressure = np.logspace(-2, 0, L)
    tab_wn = np.linspace(wn[0] - 5.0, wn[-1] + 5.0, 40)
    tab_temps = np.array([400.0, 1200.0, 2000.0, 2800.0])
    absorption = 1e-40 * ct.AMAGAT**2 * (1 + 0.3 * np.sin(tab_wn / 3.0))[None] * \
        (tab_temps / 1000.0)[:, None]
    cia = ct.Collision_Induced(table=(absorption, ['H2', 'H2'], tab_temps, tab_wn), wn=wn)
    lec = ct.Lecavelier(pressure, wn=wn)
    cont = ct.Continuum(wn, pressure, [ct.Kurucz(wn, 'H2'), lec, cia])
    assert cont.species == ['H2'] and cont.free_pars == [('lecavelier', 0), ('lecavelier', 1)]
    cdens = 10.0**rng.uniform(14.8, 15.2, (NW, L, 1))
    pars = np.stack([rng.uniform(-1, 0, NW), rng.uniform(-5, -3, NW)], axis=1)
    model = make_model(eng, continuum=cont)
    pb = eng.PassBands(wn, c['bands'])
    td, dd, rd = device_walkers(eng)
    plain = host(make_model(eng).eval_bands(td, dd, pb, radius=rd, chunk=CHUNK))
    got = host(model.eval_bands(td, dd, pb, radius=rd, chunk=CHUNK,
                                continuum_density=eng.dev(cdens), continuum_pars=eng.dev(pars)))
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got / plain - 1)) > 1e-3          # (the terms are there)
    for w in range(NW):
        lec.pars[:] = list(pars[w])
        model.set_radius(c['radius'][w])
        spec = model.eval(c['temps'][w], dd[w], {'H2': cdens[w, :, 0].copy()})
        one = host(pb.integrate_batch(spec.view(1, -1).contiguous()))[0]
        np.testing.assert_allclose(got[w], one, rtol=1.2e-12, err_msg=f'walker {w}')


@pytest.mark.gpu
def test_dilution_eclipse_and_reject(eng):
    """f_dilution[nw] and PassBands.set_eclipse against the host formulas fplanet * f and
    / bandflux_star * (rp / rs)**2 (three roundings: 1e-15); a walker outside the table's
    temperatures gets +inf and every other walker keeps its bits."""
    import torch
    c = case()
    td, dd, rd = device_walkers(eng)
    model = make_model(eng, 'eclipse_two_stream')
    pb = eng.PassBands(c['wn'], c['bands'])
    plain = model.eval_bands(td, dd, pb, radius=rd, chunk=CHUNK).clone()
    fd = c['fd']
    diluted = host(model.eval_bands(td, dd, pb, radius=rd, chunk=CHUNK, f_dilution=eng.dev(fd)))
    np.testing.assert_allclose(diluted, host(plain) * fd[:, None], rtol=1e-15)
    star = pb.star_bandflux(c['starflux'])
    want_star = [np.trapezoid(c['starflux'][a:a + len(r)] * r, c['wn'][a:a + len(r)]) * h
                 for a, r, h in c['bands']]
    np.testing.assert_allclose(star, want_star, rtol=1e-12)
    pb.set_eclipse(RPLANET, RSTAR, star)
    ecl = host(model.eval_bands(td, dd, pb, radius=rd, chunk=CHUNK, f_dilution=eng.dev(fd)))
    np.testing.assert_allclose(ecl, host(plain) * fd[:, None] / star[None] * (RPLANET / RSTAR)**2,
                               rtol=1e-15)
    hot = td.clone()
    hot[2, 5] = 2600.0                                      # above the table's 2500 K
    pb2 = eng.PassBands(c['wn'], c['bands'])
    rej = model.eval_bands(hot, dd, pb2, radius=rd, chunk=CHUNK)
    assert bool(torch.isposinf(rej[2]).all())
    keep = [w for w in range(NW) if w != 2]
    assert torch.equal(rej[keep], plain[keep])


@pytest.mark.gpu
def test_eval_params_equals_eval_bands(eng):
    """eval_params on a bound WalkerAtmosphere = eval_bands on the profiles it evaluates."""
    import torch
    from pyratbay_amd import atmosphere as pa
    c = case()
    rng = np.random.default_rng(9)
    pressure = np.logspace(-2, 0, L)
    species, mass = ['H2', 'He', 'H2O', 'CO'], [2.01588, 4.002602, 18.01528, 28.0101]
    vmr = np.tile([0.85, 0.149, 4e-4, 5e-4], (L, 1))
    vmr_models = [pa.IsoVMR('H2O', pressure), pa.IsoVMR('CO', pressure)]
    base_params = np.array([1400.0, -3.4, -3.3])
    atm = pa.WalkerAtmosphere(pressure, species, mass, vmr, ['H2', 'He'], pa.Isothermal(pressure),
                              vmr_models, rmodel='hydro_m', mplanet=1.5e30, rplanet=7.4e9,
                              refpressure=0.1, free=['T_iso', 'log_H2O', 'log_CO'],
                              base_params=base_params)
    atm.bind(['H2O', 'CO'])
    params = base_params + np.array([400.0, 0.3, 0.3]) * rng.uniform(-1, 1, (NW, 3))
    params[3, 0] = 0.0                                      # rejected: T = 0
    params = eng.dev(params)
    model = make_model(eng)
    model.set_radius(atm.base_radius)
    pb = eng.PassBands(c['wn'], c['bands'])
    got = model.eval_params(atm, params, pb, chunk=CHUNK).clone()
    prof = atm.evaluate(params)
    want = model.eval_bands(prof.temps, prof.dens, pb, radius=prof.radius, chunk=CHUNK)
    assert torch.equal(got, want)
    assert bool(torch.isposinf(got[3]).all())
    keep = [w for w in range(NW) if w != 3]
    assert bool(torch.isfinite(got[keep]).all()) and bool((got[keep] > 0).all())


@pytest.mark.gpu
def test_refusals(eng):
    """itop != 0 at construction; a cloud deck, patchy clouds and cloud-type models in eval_bands
    (the reference's two-stream ignores the clear column and its deck leaves zero rows): each a
    ValueError that names eval(); tint / flux_top with another geometry."""
    from pyratbay_amd import continuum as ct
    c = case()
    wn = c['wn']
    for name in ('two_stream', 'emission_two_stream', 'eclipse_two_stream'):
        with pytest.raises(ValueError, match='itop'):
            make_model(eng, name, itop=1)
    with pytest.raises(ValueError, match='two-stream'):
        make_model(eng, 'emission')
    with pytest.raises(ValueError, match=r'flux_top must have shape'):
        make_model(eng, flux_top=c['top'][:-1])
    td, dd, rd = device_walkers(eng)
    pb = eng.PassBands(wn, c['bands'])
    pressure = np.logspace(-2, 0, L)
    cdens = eng.dev(np.full((NW, L, 1), 1e15))
    lec = ct.Lecavelier(pressure, wn=wn)
    deck = ct.Continuum(wn, pressure, [ct.Kurucz(wn, 'H2'), ct.Deck(pressure, wn)])
    cloud = ct.Continuum(wn, pressure, [ct.Kurucz(wn, 'H2'), lec], cloud_models=[lec])
    frac = eng.dev(np.full(NW, 0.5))
    with pytest.raises(ValueError, match=r'deck_logp.*two-stream.*eval\(\)'):
        make_model(eng, continuum=deck).eval_bands(td, dd, pb, radius=rd, continuum_density=cdens,
                                                   deck_logp=eng.dev(np.full(NW, -1.0)))
    with pytest.raises(ValueError, match=r'f_patchy.*two-stream.*eval\(\)'):
        make_model(eng).eval_bands(td, dd, pb, radius=rd, f_patchy=frac)
    with pytest.raises(ValueError, match=r'cloud-type.*two-stream.*eval\(\)'):
        make_model(eng, continuum=cloud).eval_bands(td, dd, pb, radius=rd,
                                                    continuum_density=cdens)
