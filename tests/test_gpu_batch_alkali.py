"""The retrieval batch with the alkali resonance doublets (SodiumVdW, PotassiumVdW) per walker:
TableSpectrum.eval_bands(..., alkali_density=...), pb_interp_ec_batch_cont's alkali term and
pb_alkali_voigt_det_batch.  Reference: pyratbay/opacity/alkali/alkali.py:28-262,
opacity/broadening.py:231-260, src_c/_alkali.c:58-104.  Grid, pressures, temperatures and the
expected values come from fixture G7 (W = 1000, L = 12, 1e-6 ... 100 bar, 950 ... 2900 K: 7 layers
on the Faddeeva branch and 5 on the rational one, core and wing samples of every line, 62 % of the
columns outside the cutoff).

Measured worst cases (one MI355X; all in profiles/alkali.md): device voigt_det against G7 3.0e-12,
against the host form 2.2e-15; ec against G7 3.0e-12, against the split chain 5.1e-14 (alkali
alone) and 4.2e-15 (every term); band fluxes against the oracle chain 2.2e-16, against eval()
equal bits; cloud path 6.7e-16."""
import numpy as np
import pytest

import test_gpu_batch_continuum as base

pytestmark = pytest.mark.gpu

host = base.host


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def g(golden):
    return golden('g7_continuum')


@pytest.fixture(scope='module')
def oc():
    from oracle import continuum
    return continuum


def alkali_models(g, ct, pressure=None):
    p = g['pressure'] if pressure is None else pressure
    return [ct.SodiumVdW(p, wn=g['wn']), ct.PotassiumVdW(p, wn=g['wn'])]


def worst(got, want):
    want = np.asarray(want, float)
    nz = want != 0
    return float(np.max(np.abs(np.asarray(got)[nz] / want[nz] - 1.0))) if nz.any() else 0.0


def setup(g, nw, seed, L=None, full=True, tfac=None):
    """base.setup's table and walkers around G7's atmosphere; the continuum: Rayleigh H2 + He,
    Lecavelier, CIA H2-H2 + H2-He, H-, then Na and K (full), or Na and K alone."""
    from pyratbay_amd import continuum as ct
    s = base.setup(g, nw, L=L, seed=seed, hminus=True, clouds=False, tfac=tfac)
    wn, pressure = s['wn'], s['pressure']
    alk = alkali_models(g, ct, pressure)
    if full:
        models = s['models'][:2] + [ct.Lecavelier(pressure, wn=wn)] + s['models'][2:] + alk
        s['pars'] = np.stack([s['rng'].uniform(-1, 1, nw), s['rng'].uniform(-6, -2, nw)], axis=1)
    else:
        models = alk
        s['cdens'] = np.zeros((nw, len(pressure), 0))
    s['models'] = models
    s['cont'] = ct.Continuum(wn, pressure, models)
    ntot = pressure * 1e6 / s['temps'] / 1.380649e-16
    s['adens'] = np.stack([ntot * vmr * (1 + 0.3 * s['rng'].uniform(-1, 1, (nw, 1)))
                           for vmr in (2e-6, 1.5e-7)], axis=-1)
    return s


def density_dict(s, w):
    d = base.density_dict(s, w)
    d.update({sp: s['adens'][w, :, i].copy() for i, sp in enumerate(s['cont'].alkali_species)})
    return d


def fused_ec(eng, s, nw, zero_table=False):
    et = eng.dev(s['etable'] * (0.0 if zero_table else 1.0))
    return eng.interp_ec_batch(et, eng.dev(s['ttable']), eng.dev(s['temps'][:nw]),
                               eng.dev(s['dens'][:nw]), continuum=s['cont'],
                               continuum_density=eng.dev(s['cdens'][:nw]),
                               continuum_pars=None if s['pars'] is None else eng.dev(s['pars'][:nw]),
                               alkali_density=eng.dev(s['adens'][:nw]))


def split_ec(eng, s, nw, zero_table=False):
    """The parent's chain: interp_ec_batch, then Continuum.add walker by walker (host voigt_det
    from SciPy, pb_continuum, pb_alkali_cross_section per species)."""
    et = eng.dev(s['etable'] * (0.0 if zero_table else 1.0))
    ec = eng.interp_ec_batch(et, eng.dev(s['ttable']), eng.dev(s['temps'][:nw]),
                             eng.dev(s['dens'][:nw]))
    for w in range(nw):
        base.set_pars(s, w)
        s['cont'].add(ec[w], s['temps'][w], density_dict(s, w))
    return ec


def oracle_ec(orc, oc, s, w, g):
    """base.oracle_ec + the oracle's alkali cross sections fed the host voigt_det."""
    ec = base.oracle_ec(orc, oc, s, w, g)
    t = s['temps'][w]
    for i, m in enumerate(s['cont'].alkali):
        cs = oc.alkali_cross_section(s['pressure'] * 1e6, s['wn'], t, m.voigt_det(t), m.detuning,
                                     m.mass, m.lpar, m.Z, m.cutoff, m.wn0, m.gf)
        ec += cs * s['adens'][w, :, i][:, None]
    return ec


def test_device_voigt_det(eng, g):
    """pb_alkali_voigt_det_batch against G7 (rtol 1e-9, the bound of test_continuum.py for the host
    form) and against the host voigt_det (SciPy's wofz) at walker temperatures spread +-5 % around
    G7's, at the table's lowest node (40 K) in every layer, and at 3240 K.

    Bound of the second comparison, 1e-11: the device's pow and NumPy's may differ in the last
    place of dsigma, which moves (wn0 + dsigma) - wn0 by up to ulp(wn0) = 3.6e-12 cm-1, 5.5e-13 of
    dsigma = 6.6 cm-1 at 40 K, and the value goes as dsigma^-2: 1.1e-12.  The rational branch's
    leading terms cancel to one part in X = 600 ... 1000: 1000 x 2^-52 = 2e-13 per rounding.  The
    continued fraction itself: 8e-15 (CPU probe against wofz, Re z >= 20).  Sum below 2e-12; the
    bound is 5 x that."""
    from pyratbay_amd import continuum as ct
    rng = np.random.default_rng(4)
    temps = np.concatenate([g['temp'][None], g['temp'] * (1 + 0.05 * rng.uniform(-1, 1, (13, 1))),
                            np.full((1, 12), 40.0), np.full((1, 12), 3240.0)])
    for model, tag in zip(alkali_models(g, ct), ('na', 'k')):
        got = host(eng.alkali_voigt_det_batch(model, eng.dev(temps)))
        assert got.shape == (16, 12, 2)
        hg = np.sqrt(2 * ct.K * g['temp'] / (model.mass * ct.AMU)) * model.wn0[0] / ct.LS
        lor = model.lpar * (g['temp'] / 2000.0)**-0.7 * g['pressure'] * ct.BAR / 1.01e6
        assert np.sum(lor / hg < 0.1) == 7                   # both branches are exercised
        print(f'voigt_det {tag}: G7 {worst(got[0], g[f"alk_{tag}_voigt_det"]):.2e}')
        np.testing.assert_allclose(got[0], g[f'alk_{tag}_voigt_det'], rtol=1e-9)
        want = np.array([model.voigt_det(t) for t in temps])
        print(f'voigt_det {tag}: host {worst(got, want):.2e} '
              f'(40 K {worst(got[14], want[14]):.2e}, 3240 K {worst(got[15], want[15]):.2e})')
        np.testing.assert_allclose(got, want, rtol=1e-11)
        # the Continuum's pressures in barye give the same bits as the model's own
        again = eng.alkali_voigt_det_batch(model, eng.dev(temps), eng.dev(g['pressure'] * 1e6))
        assert np.array_equal(host(again), got)


def test_ec_of_a_batch(eng, g):
    """Table zeroed, alkali models only, walker 0 at G7's temperatures and densities: ec against
    alk_*_ec (rtol 1e-10, the bound of test_continuum.py) with the same zeros; every walker
    against the split chain interp_ec_batch + Continuum.add.

    Bound of the second comparison, 1e-12, for walkers at 900 K and more: voigt_det as in
    test_device_voigt_det but at dsigma >= 28 cm-1, 2 ulp(wn0) / dsigma = 1.3e-13, + 2e-13 for the
    rational branch; the wing's factors are grouped differently (some 8 roundings: 1e-15) and its
    exp has the argument -C2 |dwn| / T, at most 7.2 here: 7.2 x 2^-53 in each form.  Sum 3.6e-13;
    every term is positive, nothing cancels."""
    from pyratbay_amd import continuum as ct
    nw = 7
    s = setup(g, nw, seed=41, full=False)
    assert s['cont'].alkali_species == ['Na', 'K']
    s['temps'][0] = g['temp']
    s['adens'][0] = np.stack([float(g[f'vmr_{sp}']) * g['dens_tot'] for sp in ('Na', 'K')], axis=-1)
    both = host(fused_ec(eng, s, nw, zero_table=True))
    want = host(split_ec(eng, s, nw, zero_table=True))
    assert np.array_equal(both == 0, want == 0)
    print(f'ec Na + K against the split chain: {worst(both, want):.2e}')
    np.testing.assert_allclose(both, want, rtol=1e-12)
    # (62 % of G7's columns lie outside both cutoffs for a single species)
    assert np.mean(np.all(g['alk_na_ec'] == 0, axis=0)) > 0.5
    np.testing.assert_allclose(both[0], g['alk_na_ec'] + g['alk_k_ec'], rtol=1e-10)
    # one species at a time against G7, zeros included
    for i, (model, tag) in enumerate(zip(alkali_models(g, ct), ('na', 'k'))):
        s1 = dict(s, cont=ct.Continuum(g['wn'], g['pressure'], [model]),
                  adens=s['adens'][:, :, i:i + 1].copy())
        got = host(fused_ec(eng, s1, nw, zero_table=True))[0]
        assert np.array_equal(got == 0, g[f'alk_{tag}_ec'] == 0)
        print(f'ec {tag} against G7: {worst(got, g[f"alk_{tag}_ec"]):.2e}')
        np.testing.assert_allclose(got, g[f'alk_{tag}_ec'], rtol=1e-10)
    # on top of a table and every other term: the same additions in Continuum.add's order
    s = setup(g, nw, seed=42)
    got, want = host(fused_ec(eng, s, nw)), host(split_ec(eng, s, nw))
    print(f'ec, every term, against the split chain: {worst(got, want):.2e}')
    np.testing.assert_allclose(got, want, rtol=1e-12)


def test_epilogue_across_a_chunk(eng, g):
    """64 walkers x 32 layers x 770 samples (both doublets inside) run in chunks of four walkers,
    with CIA brackets shared and not shared inside a chunk: Na + K after every other term, against
    the split chain at test_ec_of_a_batch's bound (walkers at 900 K and more)."""
    nw, L, W = 64, 32, 770
    gn = base.narrow(g, W)
    s = setup(gn, nw, seed=47, L=L, tfac=base.chunk_tfac(np.random.default_rng(48), nw))
    assert s['temps'].min() >= 900.0
    base.assert_chunks_of_four(s, 3, 2)
    for m in s['cont'].alkali:
        assert gn['wn'][0] < min(m.wn0) and max(m.wn0) < gn['wn'][-1]
    got, want = host(fused_ec(eng, s, nw)), host(split_ec(eng, s, nw))
    print(f'chunks of four, every term, against the split chain: {worst(got, want):.2e}')
    np.testing.assert_allclose(got, want, rtol=1e-12)


@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_band_fluxes(eng, orc, oc, g, rt_path):
    """5 walkers in chunks of 2, Na + K with Rayleigh, Lecavelier, CIA and H-: band fluxes against
    the oracle chain (1e-11) and the one-walker eval() (1e-13), the bounds of
    test_gpu_batch_continuum.py."""
    nw = 5
    s = setup(g, nw, seed=43)
    cont, wn = s['cont'], s['wn']
    L = len(s['pressure'])
    assert cont.species == ['H2', 'He', 'H', 'e-'] and cont.alkali_species == ['Na', 'K']
    assert cont.free_pars == [('lecavelier', 0), ('lecavelier', 1)]
    rstar = 8.8e10
    base_radius = np.linspace(8.0e9, 7.0e9, L)
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, base_radius, rstar, rt_path=rt_path,
                              continuum=cont)
    bands, pb = base.make_bands(eng, wn)
    radius = np.array([base.hydro_radius(s['rng'], L, 0.01) for _ in range(nw)])
    got = host(model.eval_bands(eng.dev(s['temps']), eng.dev(s['dens']), pb,
                                radius=eng.dev(radius), chunk=2,
                                continuum_density=eng.dev(s['cdens']),
                                continuum_pars=eng.dev(s['pars']),
                                alkali_density=eng.dev(s['adens'])))
    assert np.all(np.isfinite(got))
    # the alkali term is in there: without the densities the fluxes differ
    none = host(model.eval_bands(eng.dev(s['temps']), eng.dev(s['dens']), pb,
                                 radius=eng.dev(radius), chunk=2,
                                 continuum_density=eng.dev(s['cdens']),
                                 continuum_pars=eng.dev(s['pars']),
                                 alkali_density=eng.dev(0.0 * s['adens'])))
    print(f'{rt_path}: the alkali term changes the band fluxes by up to '
          f'{np.max(np.abs(got / none - 1)):.2e}')
    assert np.all(np.any(got != none, axis=1))
    mu, weights = eng.default_quadrature()
    for w in range(nw):
        ec = oracle_ec(orc, oc, s, w, g)
        if rt_path == 'transit':
            depth, ideep = orc.optical_depth_transit(ec, radius[w], 0, L, 10.0)
            spec = orc.transmission(depth, radius[w], rstar, ideep, 0)
        else:
            depth, ideep = np.zeros((L, len(wn))), np.full(len(wn), L - 1, np.int32)
            orc.plane_parallel_optical_depth(depth, ideep, ec, -orc.ediff(radius[w]), 10.0, 0, L)
            spec = orc.emission_deck(depth, ideep, wn, s['temps'][w], mu, weights, 0)
        want = [np.trapezoid(spec[a:a + len(r)] * r, wn[a:a + len(r)]) * h for a, r, h in bands]
        base.set_pars(s, w)
        model.set_radius(radius[w])
        one = model.eval(s['temps'][w], eng.dev(s['dens'][w]), density_dict(s, w))
        one = host(pb.partial_integrate(one) * pb.heights)
        print(f'{rt_path} walker {w}: oracle {worst(got[w], want):.2e}, eval() '
              f'{worst(got[w], one):.2e}')
        np.testing.assert_allclose(got[w], want, rtol=1e-11)
        np.testing.assert_allclose(got[w], one, rtol=1e-13)


@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_bit_identity(eng, g, rt_path, monkeypatch):
    """The term depends on wn[col] and the walker's record only: grid order, column_order='auto',
    an explicit permutation, and layer limits with the gated repair (tile_margin = 0 and walkers
    far thinner than the first, so that walkers are repaired) give the same bits."""
    import torch
    nw, L = 6, 40
    s = setup(g, nw, seed=44, L=L)
    # the limits come from the table's opacity of walker 0 alone (order_columns): made thick, it
    # crosses maxdepth by layer 18 (transit) / 26 (emission); the others, thinned, 10 layers deeper
    s['dens'][0] *= 1e4
    s['dens'][1:] *= 1e-3
    s['cdens'][1:] *= 0.03
    s['adens'][1:] *= 1e-3
    wn = s['wn']
    radius0 = np.linspace(8.0e9, 7.0e9, L)
    _, pb = base.make_bands(eng, wn)
    args = [eng.dev(x) for x in (s['temps'], s['dens'])]
    kw = dict(continuum_density=eng.dev(s['cdens']), continuum_pars=eng.dev(s['pars']),
              alkali_density=eng.dev(s['adens']), chunk=4)
    seen = []
    name = 'transit_spectrum_ordered' if rt_path == 'transit' else 'emission_flux_batch'
    # (eval_bands looks the batch wrappers up in pyratbay_amd.batch)
    from pyratbay_amd import batch
    real = getattr(batch, name)

    def spy(*a, **k):
        if k.get('flags') is not None:
            seen.append(k['flags'])
        return real(*a, **k)
    monkeypatch.setattr(batch, name, spy)
    out = {}
    for tag, order, margin in (('grid', None, 4), ('auto', 'auto', 4), ('tight', 'auto', 0),
                               ('given', s['rng'].permutation(len(wn)), 4)):
        model = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius0, 8.8e10, rt_path=rt_path,
                                  column_order=order, continuum=s['cont'])
        model.tile_margin = margin
        seen.clear()
        out[tag] = model.eval_bands(*args, pb, **kw).clone()
        if tag == 'tight':
            assert model.tile_limit is not None
            flagged = sum(int(f[:-1].sum()) for f in seen)
            assert flagged >= 1, 'no walker ran past its limits: nothing was repaired'
    for tag in ('auto', 'tight', 'given'):
        assert torch.equal(out[tag], out['grid']), tag
    assert bool(torch.isfinite(out['grid']).all())
    # the limited interpolation and its gated repair on the same records, at the level of ec
    ops = s['cont'].batch_operands()
    et, tt = eng.dev(s['etable']), eng.dev(s['ttable'])
    ckw = dict(continuum=ops, continuum_density=kw['continuum_density'],
               continuum_pars=kw['continuum_pars'], alkali_density=kw['alkali_density'])
    full = eng.interp_ec_batch(et, tt, *args, **ckw)
    W = len(wn)
    tile = torch.zeros(-(-W // 256), dtype=torch.int32, device='cuda')     # 16 layers only
    work = torch.empty(ops.work_doubles(L, W, nw), dtype=torch.float64, device='cuda')
    ec = torch.full_like(full, -1.0)
    eng.interp_ec_batch(et, tt, *args, out=ec, tile_limit=tile, row0=2, work=work, **ckw)
    assert torch.equal(ec[:, 2:18], full[:, 2:18]) and bool((ec[:, 18:] == -1).all())
    flags = torch.ones(nw + 1, dtype=torch.int32, device='cuda')
    eng.interp_ec_batch(et, tt, *args, out=ec, gate=flags[nw:], work=work, **ckw)
    assert torch.equal(ec, full)


@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_cloud_path(eng, g, rt_path):
    """deck_logp + f_patchy: the clear and the cloudy column both carry the alkali term -- the two
    parts and the band fluxes against the same pass over the split chain's ec, at the bound of the
    eval() comparison (1e-13: eval() is that chain), and both parts change with the densities."""
    from pyratbay_amd import continuum as ct
    nw = 4
    s = setup(g, nw, seed=45)
    wn, pressure = s['wn'], s['pressure']
    L = len(pressure)
    s['cont'] = cont = ct.Continuum(wn, pressure, s['models'] + [ct.Deck(pressure, wn)])
    radius0 = np.linspace(8.0e9, 7.0e9, L)
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius0, 8.8e10, rt_path=rt_path,
                              continuum=cont, column_order=None)
    _, pb = base.make_bands(eng, wn)
    logp = eng.dev(s['rng'].uniform(-2.0, 0.5, nw))
    fp = eng.dev(s['rng'].uniform(0.2, 0.8, nw))
    td = eng.dev(s['temps'])
    got = model.eval_bands(td, eng.dev(s['dens']), pb, chunk=3,
                           continuum_density=eng.dev(s['cdens']),
                           continuum_pars=eng.dev(s['pars']), alkali_density=eng.dev(s['adens']),
                           deck_logp=logp, f_patchy=fp)
    rad = eng.dev(radius0).view(1, -1)
    deck = eng.deck_state_batch(cont.pressure_d, logp, rad, td)
    mu, weights = (eng.dev(x) for x in eng.default_quadrature())

    def parts(ec):
        if rt_path == 'transit':
            return eng.cloudy_transit_batch(ec, eng.transit_path_device(rad[0], 0), rad, 8.8e10, 0,
                                            10.0, deck=deck, f_patchy=fp, want_parts=True)
        radn = rad.expand(nw, -1)
        return eng.cloudy_emission_batch(ec, (radn[:, :-1] - radn[:, 1:]).contiguous(), eng.dev(wn),
                                         td, mu, weights, 0, 10.0, deck=deck, f_patchy=fp,
                                         want_parts=True)
    fused, split = parts(fused_ec(eng, s, nw)), parts(split_ec(eng, s, nw))
    for name, a, b in zip(('spectrum', 'clear', 'cloudy'), fused, split):
        print(f'{rt_path} {name}: {worst(host(a), host(b)):.2e}')
        np.testing.assert_allclose(host(a), host(b), rtol=1e-13)
    np.testing.assert_allclose(host(got), host(pb.integrate_batch(split[0])), rtol=1e-13)
    s0 = dict(s, adens=0.0 * s['adens'])
    bare = parts(fused_ec(eng, s0, nw))
    for a, b in zip(fused[1:], bare[1:]):
        assert float((a - b).abs().max()) > 0


def test_refusals(eng, g):
    """What eval_bands refuses with an alkali model, each before any launch; a walker outside the
    table's temperatures still gets +inf."""
    import torch
    from pyratbay_amd import continuum as ct
    nw = 4
    s = setup(g, nw, seed=46)
    wn, pressure = s['wn'], s['pressure']
    L = len(pressure)
    radius = np.linspace(8.0e9, 7.0e9, L)
    _, pb = base.make_bands(eng, wn)
    td, dd = eng.dev(s['temps']), eng.dev(s['dens'])
    kw = dict(continuum_density=eng.dev(s['cdens']), continuum_pars=eng.dev(s['pars']))
    ad = eng.dev(s['adens'])
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius, 8.8e10, continuum=s['cont'])
    # without the densities: the refusal of before, in its words
    with pytest.raises(ValueError, match='not supported in batched form'):
        model.eval_bands(td, dd, pb, **kw)
    for bad in (ad[:, :, :1].contiguous(), ad[:3].contiguous(), ad.cpu(), ad.float(),
                s['adens']):
        with pytest.raises(ValueError, match='alkali_density'):
            model.eval_bands(td, dd, pb, alkali_density=bad, **kw)
    ref = model.eval_bands(td, dd, pb, alkali_density=ad, **kw).clone()
    # alkali_density without an alkali model, and without a Continuum
    plain = ct.Continuum(wn, pressure, s['models'][:-2])
    m2 = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius, 8.8e10, continuum=plain)
    with pytest.raises(ValueError, match='alkali_density needs an alkali model'):
        m2.eval_bands(td, dd, pb, alkali_density=ad, **kw)
    m2 = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius, 8.8e10)
    with pytest.raises(ValueError, match='alkali_density'):
        m2.eval_bands(td, dd, pb, alkali_density=ad)
    # a third alkali model
    three = ct.Continuum(wn, pressure, s['models'] + [ct.SodiumVdW(pressure, wn=wn)])
    m3 = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius, 8.8e10, continuum=three)
    with pytest.raises(ValueError, match=r'at most 2 models with 4 lines.*use eval\(\)'):
        m3.eval_bands(td, dd, pb, alkali_density=eng.dev(np.ones((nw, L, 3))), **kw)
    # a VanderWaals subclass below the regime of the device's Faddeeva function at tmin
    from test_batch_alkali_cpu import _Narrow
    narrow = _Narrow.make(ct, pressure, wn)
    assert narrow.detuning_x(model.tmin) < 20
    c4 = ct.Continuum(wn, pressure, s['models'][:-2] + [narrow])
    m4 = eng.TableSpectrum(s['etable'], s['ttable'], wn, radius, 8.8e10, continuum=c4)
    with pytest.raises(ValueError, match=r'narrow_vdw.*below 20.*use eval\(\)'):
        m4.eval_bands(td, dd, pb, alkali_density=ad[:, :, :1].contiguous(), **kw)
    # a walker outside the table: +inf, the others keep their bits
    temps = s['temps'].copy()
    temps[2, 3] = 3300.0
    assert temps[2, 3] > s['ttable'][-1]
    got = model.eval_bands(eng.dev(temps), dd, pb, alkali_density=ad, **kw)
    assert bool(torch.isinf(got[2]).all()) and bool((got[2] > 0).all())
    keep = [0, 1, 3]
    assert torch.equal(got[keep], ref[keep])
