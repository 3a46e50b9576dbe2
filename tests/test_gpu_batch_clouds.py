"""Cloud deck and patchy clouds per walker in the retrieval batch (TableSpectrum.eval_bands with
deck_logp / f_patchy; engine.deck_state_batch, cloudy_transit_batch, cloudy_emission_batch;
pb_clouds.hip).  Reference: opacity/clouds/gray.py:95-154, pyrat_obj.py:135-139, 285-286,
opacity/optic_depth.py:94-136, spectrum/radiative_transfer.py:63-67, 125-127,
pyrat/spectrum.py:357-384.  Yardsticks: fixture G11 (the reference's own ec, ec_cloud, deck state
and clear / cloudy / mixed spectra) and the oracle chain of test_patchy_golden.py built from
oracle/continuum.py terms; rtol 1e-11, the figure those tests use for this chain."""
import numpy as np
import pytest

# the oracle chain (test_patchy_golden.py::test_oracle_patchy) for one walker
from cases import oracle_patchy

pytestmark = pytest.mark.gpu

RTS = ['transit', 'emission', 'eclipse']
RTOL = 1e-11
RSTAR = 8.8e10


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def oc():
    from oracle import continuum
    return continuum


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# G11 through the low-level batch functions
# ---------------------------------------------------------------------------------------------
def g11_case(g, rt):
    rtop, rstar, maxdepth, rplanet, fpatchy = g[f'{rt}_scalars']
    _, deck_itop, deck_rsurf, deck_tsurf = g[f'{rt}_deck']
    c = dict(rtop=int(rtop), rstar=float(rstar), maxdepth=float(maxdepth), fpatchy=float(fpatchy),
             deck=(int(deck_itop), float(deck_rsurf), float(deck_tsurf)))
    for key in ('wn', 'ec', 'ec_cloud', 'spectrum', 'clear', 'cloudy', 'radius', 'temp',
                'spectrum_f0', 'spectrum_f1'):
        c[key] = np.ascontiguousarray(g[f'{rt}_{key}'])
    c['scale'] = 1.0
    if rt != 'transit':
        c['mu'], c['weights'] = g[f'{rt}_mu'], g[f'{rt}_weights']
    if rt == 'eclipse':
        c['scale'] = 1 / g[f'{rt}_starflux'] * (float(rplanet) / c['rstar'])**2
    if rt != 'transit':
        c['rstar'] = RSTAR                    # (not used by the emission geometry)
    return c


def rank1_factors(ec_cloud):
    """ec_cloud[L, W] of ONE rank-1 model (G11: a Lecavelier haze) as cs[W] x f[L]."""
    l0, w0 = np.unravel_index(np.argmax(ec_cloud), ec_cloud.shape)
    cs = ec_cloud[l0] / ec_cloud[l0, w0]
    f = ec_cloud[:, w0].copy()
    np.testing.assert_allclose(np.outer(f, cs), ec_cloud, rtol=1e-13, atol=0)
    return cs, f


@pytest.mark.parametrize('pos', [0, 5])
@pytest.mark.parametrize('rt', RTS)
def test_g11_low_level(eng, golden, rt, pos):
    """The fixture as walker `pos` of a batch of 8 whose other walkers are perturbed: spectrum,
    clear and cloudy of the reference for f = 0.5, 0 and 1; and every walker of the batch against
    the single-spectrum path (patchy_transit_spectrum / patchy_emission_flux) on its own ec."""
    import torch
    c = g11_case(golden('g11_patchy'), rt)
    geom = 'transit' if rt == 'transit' else 'emission'
    rng = np.random.default_rng(17 + pos)
    nw = 8
    L, W = c['ec'].shape
    itop, dev = c['rtop'], eng.dev
    cs, f = rank1_factors(c['ec_cloud'])
    scale = 10.0**rng.uniform(-0.7, 0.7, (nw, 1, 1))
    scale[pos] = 1.0
    ec = c['ec'][None] * scale
    cf = f[None, :, None] * 10.0**rng.uniform(-1, 1, (nw, 1, 1))
    cf[pos, :, 0] = f
    radius = c['radius'][None] * (1 + 0.01 * rng.uniform(-1, 1, (nw, 1)))
    radius[pos] = c['radius']
    temp = c['temp'][None] * (1 + 0.05 * rng.uniform(-1, 1, (nw, 1)))
    temp[pos] = c['temp']
    ditop = rng.integers(max(itop, 1), L, nw).astype(np.int32)
    ditop[pos] = c['deck'][0]
    dr = np.array([0.5 * (radius[w, k] + radius[w, k - 1]) for w, k in enumerate(ditop)])
    dt = np.array([0.5 * (temp[w, k] + temp[w, k - 1]) for w, k in enumerate(ditop)])
    dr[pos], dt[pos] = c['deck'][1], c['deck'][2]
    deck = (dev(ditop, torch.int32), dev(dr), dev(dt))
    ec_d, cs_d, cf_d = dev(ec), dev(cs[None]), dev(cf)

    def run(fvec, parts):
        fp = dev(np.asarray(fvec, float))
        if geom == 'transit':
            path = eng.transit_path_device(dev(radius), itop)
            return eng.cloudy_transit_batch(ec_d, path, dev(radius), c['rstar'], itop,
                                            c['maxdepth'], deck=deck, cloud_cs=cs_d, cloud_f=cf_d,
                                            f_patchy=fp, want_parts=parts)
        return eng.cloudy_emission_batch(ec_d, dev(-np.diff(radius, axis=1)), dev(c['wn']),
                                         dev(temp), dev(c['mu']), dev(c['weights']), itop,
                                         c['maxdepth'], deck=deck, cloud_cs=cs_d, cloud_f=cf_d,
                                         f_patchy=fp, want_parts=parts)
    fw = rng.uniform(0, 1, nw)
    fw[pos] = c['fpatchy']
    spectrum, clear, cloudy = (host(t) for t in run(fw, True))
    np.testing.assert_allclose(cloudy[pos] * c['scale'], c['cloudy'], rtol=RTOL)
    np.testing.assert_allclose(clear[pos] * c['scale'], c['clear'], rtol=RTOL)
    np.testing.assert_allclose(spectrum[pos] * c['scale'], c['spectrum'], rtol=RTOL)
    for fval, key in ((0.0, 'spectrum_f0'), (1.0, 'spectrum_f1')):
        got = host(run(np.full(nw, fval), False))
        np.testing.assert_allclose(got[pos] * c['scale'], c[key], rtol=RTOL)
    # the batch and the single-spectrum path agree, walker by walker
    for w in range(nw):
        ecw, cloud_w = dev(ec[w]), dev(np.outer(cf[w, :, 0], cs))
        if geom == 'transit':
            path = dev(eng.pack_raypath(eng.transit_path(radius[w], itop), itop))
            one = eng.patchy_transit_spectrum(ecw, cloud_w, float(fw[w]), path, dev(radius[w]),
                                              c['rstar'], itop, c['maxdepth'], float(dr[w]),
                                              int(ditop[w]))
        else:
            one = eng.patchy_emission_flux(ecw, cloud_w, float(fw[w]), dev(-np.diff(radius[w])),
                                           dev(c['wn']), dev(temp[w]), dev(c['mu']),
                                           dev(c['weights']), itop, c['maxdepth'], float(dt[w]),
                                           int(ditop[w]))
        for got, want in zip((spectrum, clear, cloudy), one):
            np.testing.assert_allclose(got[w], host(want), rtol=RTOL)


# ---------------------------------------------------------------------------------------------
# Per-walker variation through eval_bands
# ---------------------------------------------------------------------------------------------
def build_case(g, nw, seed, geom='transit'):
    """G11's pressure grid and atmosphere, a synthetic table, perturbed temperatures, densities and
    radii; the continuum: Rayleigh H2, a Lecavelier haze, a gray cloud[, the deck].  Host only."""
    rng = np.random.default_rng(seed)
    wn = np.ascontiguousarray(g['transit_wn'])
    pressure = np.ascontiguousarray(g['transit_press'])
    L, W = len(pressure), len(wn)
    nspec, ntemp = 3, 9
    ttable = np.linspace(300.0, 3300.0, ntemp)
    # (opacities that put the clear crossings of maxdepth inside the range of the decks drawn
    # below: the vertical paths of the emission geometry are ~100 times shorter)
    lo, hi, spread = (-24.0, -23.0, 1.2) if geom == 'transit' else (-22.2, -21.7, 0.9)
    etable = 10.0**rng.uniform(lo, hi, (nspec, ntemp, L, 1)) * \
        10.0**rng.uniform(-spread, spread, (nspec, 1, 1, W))
    temps = g['transit_temp'][None] * (1 + 0.08 * rng.uniform(-1, 1, (nw, 1)))
    ntot = pressure * 1e6 / temps / 1.380649e-16
    dens = ntot[:, :, None] * 10.0**rng.uniform(-5, -3.5, (nw, 1, nspec))
    radius = g['transit_radius'][None] * (1 + 0.01 * rng.uniform(-1, 1, (nw, 1))) + \
        np.linspace(0, 1, L)[None] * 2e7 * rng.uniform(-1, 1, (nw, 1))
    cdens = (ntot * 0.85 * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))))[:, :, None]
    pars = np.stack([rng.uniform(0, 2, nw), rng.uniform(-6, -2, nw),            # Lecavelier
                     rng.uniform(0, 2, nw), rng.uniform(-4, -2, nw),
                     rng.uniform(-1, 1.5, nw)], axis=1)                          # CCSgray
    logp = rng.uniform(-5, 1, nw)
    logp[0], logp[1] = -5.0, 1.0
    fpatchy = rng.uniform(0.05, 0.95, nw)
    return dict(wn=wn, pressure=pressure, L=L, W=W, ttable=ttable, etable=etable, temps=temps,
                dens=dens, radius=radius, cdens=cdens, pars=pars, logp=logp, fpatchy=fpatchy,
                rng=rng)


def continuum_of(s, cloud, deck=True):
    """-> (Continuum, the models); cloud: the haze and the gray cloud (and the deck) are
    cloud-type, else they go into ec like the Rayleigh term."""
    from pyratbay_amd import continuum as ct
    wn, pressure = s['wn'], s['pressure']
    lec, gray = ct.Lecavelier(pressure, wn=wn), ct.CCSgray(pressure, wn)
    models = [ct.Kurucz(wn, 'H2'), lec, gray] + ([ct.Deck(pressure, wn)] if deck else [])
    return ct.Continuum(wn, pressure, models, cloud_models=models[1:] if cloud else [])


def oracle_ecs(orc, oc, s, w, cloud):
    """(ec, ec_cloud) of walker w: interp_ec + Rayleigh [+ haze + gray cloud], and the cloud-type
    terms summed in model order (None when there are none)."""
    L, W = s['L'], s['W']
    ec = np.zeros((L, W))
    orc.interp_ec(ec, s['etable'], s['ttable'], s['temps'][w], s['dens'][w], 0, L)
    nominal = oc.nominal_density(s['pressure'], s['temps'][w])
    ec += oc.rayleigh_cross_section(s['wn'], 'H2') * s['cdens'][w, :, 0][:, None]
    lec = oc.lecavelier_cross_section(s['wn'], s['pars'][w, :2]) * nominal[:, None]
    gray = (oc.gray_layer_cross_section(s['pressure'], s['pars'][w, 2:5]) * nominal)[:, None]
    if cloud:
        return ec, lec + gray
    ec += lec
    ec += gray
    return ec, None


BANDS = ((10, 150), (120, 300), (280, 400))


def make_bands(eng, wn):
    bands = []
    for lo, hi in BANDS:
        resp = np.exp(-np.linspace(-1.5, 1.5, hi - lo)**2)
        bands.append((lo, resp, 1.0 / np.trapezoid(resp, wn[lo:hi])))
    return bands, eng.PassBands(wn, bands)


def band_flux(spec, wn, bands):
    return [np.trapezoid(spec[a:a + len(r)] * r, wn[a:a + len(r)]) * h for a, r, h in bands]


CASES = {                       # name: (deck, f_patchy, cloud-type haze + gray cloud)
    'deck': (True, False, False),
    'patchy_deck': (True, True, False),
    'patchy_deck_clouds': (True, True, True),
    'patchy_no_deck': (False, True, True),
}


def regimes(s, ideep_clear, deck_itop):
    """Per walker: does the deck decide 'all', 'some' or 'none' of its columns (it lies above every
    clear crossing, above some, below all)?"""
    out = []
    for w, ideep in ideep_clear.items():
        above = deck_itop[w] < ideep
        out.append('all' if above.all() else 'some' if above.any() else 'none')
    return out


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('geom', ['transit', 'emission'])
def test_eval_bands_against_oracle(eng, orc, oc, golden, geom, case):
    from pyratbay_amd import continuum as ct
    use_deck, use_f, cloud = CASES[case]
    nw = 12
    s = build_case(golden('g11_patchy'), nw, 11, geom)
    cont = continuum_of(s, cloud, use_deck)
    dev = eng.dev
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0], RSTAR,
                              rt_path=geom, continuum=cont)
    bands, pb = make_bands(eng, s['wn'])
    kw = dict(radius=dev(s['radius']), chunk=5, continuum_density=dev(s['cdens']),
              continuum_pars=dev(s['pars']))
    if use_deck:
        kw['deck_logp'] = dev(s['logp'])
    if use_f:
        kw['f_patchy'] = dev(s['fpatchy'])
    got = host(model.eval_bands(dev(s['temps']), dev(s['dens']), pb, **kw))
    assert np.all(np.isfinite(got))
    ditop, rsurf, tsurf = ct.deck_state(s['pressure'], s['logp'], s['radius'], s['temps'])
    mu, weights = eng.default_quadrature()
    ideep_clear = {}
    for w in range(nw):
        ec, ec_cloud = oracle_ecs(orc, oc, s, w, cloud)
        deck = (ditop[w], rsurf[w], tsurf[w]) if use_deck else None
        clear, cloudy, ideep_c, _ = oracle_patchy(orc, geom, ec, ec_cloud, s['radius'][w], 0, 10.0,
                                                  deck, s['temps'][w], s['wn'], mu, weights)
        ideep_clear[w] = ideep_c
        f = s['fpatchy'][w] if use_f else 1.0
        spec = f * cloudy + (1 - f) * clear
        print(f'{geom} {case} walker {w}: max rel err',
              np.max(np.abs(got[w] / band_flux(spec, s['wn'], bands) - 1)))
        np.testing.assert_allclose(got[w], band_flux(spec, s['wn'], bands), rtol=RTOL)
    if use_deck:
        # a condition on the inputs: the draw covers "the deck decides every column", "some",
        # "none"
        assert set(regimes(s, ideep_clear, ditop)) == {'all', 'some', 'none'}


# ---------------------------------------------------------------------------------------------
# Edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', ['transit', 'emission'])
def test_deck_above_itop_and_beyond_the_grid(eng, orc, oc, golden, geom):
    """itop = 3 with walkers whose deck_itop <= itop, and decks beyond each end of the grid."""
    from pyratbay_amd import continuum as ct
    nw, itop = 6, 3
    s = build_case(golden('g11_patchy'), nw, 23, geom)
    s['logp'][:4] = [-9.0, 4.0, np.log10(s['pressure'][2]) - 0.01, np.log10(s['pressure'][3]) - 0.01]
    cont = continuum_of(s, True)
    dev = eng.dev
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0], RSTAR,
                              rt_path=geom, itop=itop, continuum=cont)
    bands, pb = make_bands(eng, s['wn'])
    got = host(model.eval_bands(dev(s['temps']), dev(s['dens']), pb, radius=dev(s['radius']),
                                continuum_density=dev(s['cdens']), continuum_pars=dev(s['pars']),
                                deck_logp=dev(s['logp']), f_patchy=dev(s['fpatchy'])))
    ditop, rsurf, tsurf = ct.deck_state(s['pressure'], s['logp'], s['radius'], s['temps'])
    assert ditop[0] == 1 and ditop[1] == s['L'] - 1 and ditop[2] == 2 and ditop[3] == 3
    dstate = [host(t) for t in eng.deck_state_batch(dev(s['pressure']), dev(s['logp']),
                                                    dev(s['radius']), dev(s['temps']))]
    assert np.array_equal(dstate[0], ditop)
    np.testing.assert_allclose(dstate[1], rsurf, rtol=1e-13)
    np.testing.assert_allclose(dstate[2], tsurf, rtol=1e-13)
    mu, weights = eng.default_quadrature()
    for w in range(nw):
        ec, ec_cloud = oracle_ecs(orc, oc, s, w, True)
        clear, cloudy, _, _ = oracle_patchy(orc, geom, ec, ec_cloud, s['radius'][w], itop, 10.0,
                                            (ditop[w], rsurf[w], tsurf[w]), s['temps'][w], s['wn'],
                                            mu, weights)
        f = s['fpatchy'][w]
        np.testing.assert_allclose(got[w], band_flux(f * cloudy + (1 - f) * clear, s['wn'], bands),
                                   rtol=RTOL)


@pytest.mark.parametrize('geom', ['transit', 'emission'])
def test_fractions_rejects_orders_and_chunks(eng, orc, oc, golden, geom):
    """f = 1 is the deck-only batch; f = 0 is the oracle chain's clear column (in emission with the
    deck's temperature in row deck_itop of the Planck array) and, in transit, the cloud-free
    batch; a walker outside the
    table's temperatures gets +inf, its neighbours keep their bits; shared radius = the same
    radius per walker; chunks that split the batch unevenly and column_order None / 'auto' /
    explicit are bit-identical."""
    import torch
    nw = 11
    s = build_case(golden('g11_patchy'), nw, 5, geom)
    dev = eng.dev
    _, pb = make_bands(eng, s['wn'])
    td, dd = dev(s['temps']), dev(s['dens'])
    kw = dict(radius=dev(s['radius']), continuum_density=dev(s['cdens']),
              continuum_pars=dev(s['pars']))
    ckw = dict(kw, deck_logp=dev(s['logp']), f_patchy=dev(s['fpatchy']))

    def model_of(cont, order=None):
        return eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0], RSTAR,
                                 rt_path=geom, continuum=cont, column_order=order)
    cont = continuum_of(s, False)
    model = model_of(cont)
    ref = model.eval_bands(td, dd, pb, **ckw).clone()
    assert bool(torch.isfinite(ref).all())
    one = model.eval_bands(td, dd, pb, **dict(ckw, f_patchy=dev(np.ones(nw))))
    deck_only = model.eval_bands(td, dd, pb, **dict(kw, deck_logp=dev(s['logp'])))
    np.testing.assert_allclose(host(one), host(deck_only), rtol=1e-13)
    from pyratbay_amd import continuum as ct
    bands, _ = make_bands(eng, s['wn'])
    zero = model.eval_bands(td, dd, pb, **dict(ckw, f_patchy=dev(np.zeros(nw))))
    ditop, rsurf, tsurf = ct.deck_state(s['pressure'], s['logp'], s['radius'], s['temps'])
    mu, weights = eng.default_quadrature()
    for w in (0, 1, 4, 10):
        ec, _ = oracle_ecs(orc, oc, s, w, False)
        clear, _, _, _ = oracle_patchy(orc, geom, ec, None, s['radius'][w], 0, 10.0,
                                       (ditop[w], rsurf[w], tsurf[w]), s['temps'][w], s['wn'], mu,
                                       weights)
        np.testing.assert_allclose(host(zero)[w], band_flux(clear, s['wn'], bands), rtol=RTOL)
    if geom == 'transit':
        plain = model_of(continuum_of(s, False, deck=False)).eval_bands(td, dd, pb, **kw)
        np.testing.assert_allclose(host(zero), host(plain), rtol=RTOL)
    # f outside [0, 1] is clamped
    wild = s['fpatchy'].copy()
    wild[2], wild[3] = -0.5, 1.5
    clamped = np.clip(wild, 0, 1)
    assert torch.equal(model.eval_bands(td, dd, pb, **dict(ckw, f_patchy=dev(wild))),
                       model.eval_bands(td, dd, pb, **dict(ckw, f_patchy=dev(clamped))))
    # a walker outside the table
    temps = s['temps'].copy()
    temps[4, 7] = 5000.0
    got = model.eval_bands(dev(temps), dd, pb, **ckw)
    assert bool(torch.isinf(got[4]).all()) and bool((got[4] > 0).all())
    keep = [w for w in range(nw) if w != 4]
    assert torch.equal(got[keep], ref[keep])
    # shared radius
    shared = model.eval_bands(td, dd, pb, **dict(ckw, radius=dev(s['radius'][:1])))
    same = model.eval_bands(td, dd, pb,
                            **dict(ckw, radius=dev(np.repeat(s['radius'][:1], nw, axis=0))))
    assert torch.equal(shared, same)
    assert torch.equal(shared, model_of(cont).eval_bands(td, dd, pb, **dict(ckw, radius=None)))
    # chunks and column orders, with and without cloud-type opacity
    for cloud in (False, True):
        c = continuum_of(s, cloud)
        base = model_of(c).eval_bands(td, dd, pb, **ckw).clone()
        for order, chunk in ((None, 4), ('auto', 64), ('auto', 3),
                             (s['rng'].permutation(s['W']), 7)):
            m = model_of(c, order)
            assert torch.equal(m.eval_bands(td, dd, pb, chunk=chunk, **ckw), base), (cloud, chunk)
            assert (m.column_order is None) == (order is None)


def test_dilution_eclipse_and_hires(eng, orc, oc, golden):
    """f_dilution + set_eclipse on the combined flux against the oracle chain; a HiresData with rv
    equals the same exit (HiresData.integrate_batch) applied to the oracle chain's spectra."""
    from pyratbay_amd import continuum as ct
    nw = 5
    s = build_case(golden('g11_patchy'), nw, 9, 'emission')
    cont = continuum_of(s, True)
    dev = eng.dev
    wn = s['wn']
    rplanet = 7.4e9
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, s['radius'][0], RSTAR,
                              rt_path='emission', continuum=cont)
    bands, pb = make_bands(eng, wn)
    starflux = 2.0e6 * (1.0 + 0.1 * np.sin(wn / 70.0))
    star = pb.star_bandflux(starflux)
    pb.set_eclipse(rplanet, RSTAR, star)
    fd = s['rng'].uniform(0.5, 1.0, nw)
    kw = dict(radius=dev(s['radius']), continuum_density=dev(s['cdens']),
              continuum_pars=dev(s['pars']), deck_logp=dev(s['logp']),
              f_patchy=dev(s['fpatchy']))
    td, dd = dev(s['temps']), dev(s['dens'])
    got = host(model.eval_bands(td, dd, pb, f_dilution=dev(fd), **kw))
    ditop, rsurf, tsurf = ct.deck_state(s['pressure'], s['logp'], s['radius'], s['temps'])
    mu, weights = eng.default_quadrature()
    spectra = []
    for w in range(nw):
        ec, ec_cloud = oracle_ecs(orc, oc, s, w, True)
        clear, cloudy, _, _ = oracle_patchy(orc, 'emission', ec, ec_cloud, s['radius'][w], 0, 10.0,
                                            (ditop[w], rsurf[w], tsurf[w]), s['temps'][w], wn, mu,
                                            weights)
        f = s['fpatchy'][w]
        spectra.append(f * cloudy + (1 - f) * clear)
        _, fplanet = orc.emission_observables(spectra[-1], 'eclipse', starflux, rplanet, RSTAR,
                                              fd[w])
        np.testing.assert_allclose(got[w], orc.eclipse_bandflux(band_flux(fplanet, wn, bands),
                                                                rplanet, RSTAR, star), rtol=RTOL)
    # high-resolution data with a per-walker radial velocity
    data_wn = np.linspace(wn[30], wn[-30], 57)
    res = 0.25 * wn[0] / (wn[1] - wn[0])
    hd = eng.HiresData(wn, data_wn, res, rv_max=30.0)
    rv = dev(s['rng'].uniform(-20, 20, nw))
    got = model.eval_bands(td, dd, hd, rv=rv, **kw)
    want = hd.integrate_batch(dev(np.array(spectra)), rv=rv)
    assert got.shape == (nw, len(data_wn))
    np.testing.assert_allclose(host(got), host(want), rtol=RTOL)


def test_refusals(eng, golden):
    from pyratbay_amd import continuum as ct
    nw = 4
    s = build_case(golden('g11_patchy'), nw, 2)
    dev = eng.dev
    _, pb = make_bands(eng, s['wn'])
    td, dd = dev(s['temps']), dev(s['dens'])
    kw = dict(continuum_density=dev(s['cdens']), continuum_pars=dev(s['pars']))

    def model_of(cont):
        return eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0], RSTAR,
                                 continuum=cont)
    logp, f = dev(s['logp']), dev(s['fpatchy'])
    with_deck = model_of(continuum_of(s, True))
    # a Deck without deck_logp: the old refusal, its text unchanged
    with pytest.raises(ValueError, match=r"continuum models \['deck'\] are not supported in "
                                         r"batched form \(cloud deck, alkali\); use eval\(\)"):
        with_deck.eval_bands(td, dd, pb, f_patchy=f, **kw)
    with pytest.raises(ValueError, match='deck_logp needs a Deck'):
        model_of(continuum_of(s, True, deck=False)).eval_bands(td, dd, pb, deck_logp=logp, **kw)
    with pytest.raises(ValueError, match='deck_logp needs a Deck'):
        eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0],
                          RSTAR).eval_bands(td, dd, pb, deck_logp=logp)
    with pytest.raises(ValueError, match='deck_logp must be a float64 device tensor of shape'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp[:3], **kw)
    with pytest.raises(ValueError, match='f_patchy must be a float64 device tensor of shape'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp, f_patchy=f.view(nw, 1), **kw)
    with pytest.raises(ValueError, match='f_patchy must be a float64 device tensor of shape'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp, f_patchy=s['fpatchy'], **kw)
    with pytest.raises(ValueError, match='radius must have shape'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp, radius=dev(s['radius'][:2]), **kw)
    # (cloud-type models alone take the cloud path too, with neither argument)
    with pytest.raises(ValueError, match='radius must have shape'):
        model_of(continuum_of(s, True, deck=False)).eval_bands(
            td, dd, pb, radius=dev(s['radius'][:2]), **kw)
    # a tensor on the host or of another element type never reaches a kernel
    with pytest.raises(ValueError, match='deck_logp must be a float64 device tensor'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp.cpu(), **kw)
    with pytest.raises(ValueError, match='f_patchy must be a float64 device tensor'):
        with_deck.eval_bands(td, dd, pb, deck_logp=logp, f_patchy=f.float(), **kw)
    # an alkali model stays refused, with the deck's pressures given too
    wn, pressure = s['wn'], s['pressure']
    models = [ct.Kurucz(wn, 'H2'), ct.Lecavelier(pressure, wn=wn), ct.CCSgray(pressure, wn),
              ct.Deck(pressure, wn), ct.SodiumVdW(pressure, wn=wn)]
    alkali = model_of(ct.Continuum(wn, pressure, models))
    with pytest.raises(ValueError, match=r"\['sodium_vdw'\] are not supported in batched form"):
        alkali.eval_bands(td, dd, pb, deck_logp=logp, **kw)
    # the low-level functions check shapes too
    ec = eng.interp_ec_batch(dev(s['etable']), dev(s['ttable']), td, dd)
    path = eng.transit_path_device(dev(s['radius']), 0)
    with pytest.raises(ValueError, match='f_patchy must be a float64 device tensor of shape'):
        eng.cloudy_transit_batch(ec, path, dev(s['radius']), RSTAR, 0, 10.0, f_patchy=f[:2])
    with pytest.raises(ValueError, match='radius'):
        eng.cloudy_transit_batch(ec, path, dev(s['radius'][:3]), RSTAR, 0, 10.0)
    import torch
    ones = dev(np.ones(nw))
    with pytest.raises(ValueError, match='deck itop must be a int32 device tensor'):
        eng.cloudy_transit_batch(ec, path, dev(s['radius']), RSTAR, 0, 10.0,
                                 deck=(ones, ones, ones))
    with pytest.raises(ValueError, match='deck surface must be a float64 device tensor'):
        eng.cloudy_transit_batch(ec, path, dev(s['radius']), RSTAR, 0, 10.0,
                                 deck=(ones.to(torch.int32), ones.cpu(), ones))
    with pytest.raises(ValueError, match='cloud_cs'):
        eng.cloudy_transit_batch(ec, path, dev(s['radius']), RSTAR, 0, 10.0,
                                 cloud_cs=dev(np.ones((2, s['W']))),
                                 cloud_f=dev(np.ones((nw, s['L'], 1))))
