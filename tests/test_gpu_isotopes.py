"""Isotope ratios of sampled cross sections on the device: pb_iso_density (csrc/pb_isotopes.hip)
at the kernel boundary on dirty memory, the loader with an isotope_ratios block, every form of
TableSpectrum.eval_bands, the whole pipeline against the reference (fixture G29,
tests/golden/make_golden_isotopes.py), the retrieval front end, the posterior summary, a repeated
table species through WalkerAtmosphere.bind, and graph capture.

Tolerances: the rule of test_gpu_atmosphere.py -- the worst relative deviation measured on one
MI355X over every case of this file, times ten, rounded up to a power of ten; a measured 0 stays
"equal bits".  Always against the host statement or the reference's fixture, never against another
device result.  Every check prints its figure before it asserts.  Measured (profiles/isotopes.md
has the same table; each gives the tolerance 1e-14):
  ratio of a free slot, pow(10, par) vs ratios_host (NumPy's 10.0**par)     2.22e-16
  band fluxes vs the reference's eval(), entered at eval_bands, transit     2.41e-16
  band fluxes vs the reference's eval(), entered at eval_bands, eclipse     6.05e-16
  band fluxes vs the reference's eval(), entered at eval_params, transit    2.41e-16
  band fluxes vs the reference's eval(), entered at eval_params, eclipse    8.80e-16
Everything else is an equal-bits statement: dens_out = dens_in * ratio and a fill slot =
1 - (sequential sum) given the device's own ratios; the defaults (pars == null) against the
reference's iso_ratios; a model with isotopes against the same table fed pre-scaled densities."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_RATIO = 1e-14
TOL_BANDS = {('eval_bands', 'transmission'): 1e-14, ('eval_bands', 'eclipse'): 1e-14,
             ('eval_params', 'transmission'): 1e-14, ('eval_params', 'eclipse'): 1e-14}
GUARD = 3
SENTINEL = -7.25e77
NEGATIVE_FILLER = (-0.1, -0.2)


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def g29(golden):
    return golden('g29_isotopes')


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, float).view(np.int64)


def max_rel(got, want):
    with np.errstate(all='ignore'):
        dev = np.abs(got - want) / np.abs(want)
    return float(np.max(np.where(got == want, 0.0, dev)))


# -------------------------------------------------------------------------------------------------
# 1. the kernel boundary, on dirty memory
# -------------------------------------------------------------------------------------------------
class Dirty:
    """`shape` elements holding a sentinel between two guard blocks of GUARD sentinels."""

    def __init__(self, shape, dtype=None, sentinel=SENTINEL):
        import torch
        self.n = int(np.prod(shape))
        self.sentinel = sentinel
        self.store = torch.full((2 * GUARD + self.n,), sentinel, dtype=dtype or torch.float64,
                                device='cuda')
        self.body = self.store[GUARD:GUARD + self.n].view(*shape)
        self.ptr = C.c_void_p(self.store.data_ptr() + self.store.element_size() * GUARD)

    def guards_intact(self):
        return bool((self.store[:GUARD] == self.sentinel).all()) and \
            bool((self.store[GUARD + self.n:] == self.sentinel).all())


def boundary_model(kind, nspec):
    """-> (IsotopeRatios, fill slots).  Labels have no underscore ('fill_a_b' splits at them)."""
    from pyratbay_amd import isotopes as iso
    names = [f'iso_s{i}' for i in range(nspec)]

    def free(i):
        return (f'k{i}', names[i], f'{-1.5 - 0.05 * i:.2f}')

    def fill(i, fillers):
        return (f'k{i}', names[i], 'fill_' + '_'.join(f's{j}' for j in fillers))
    if kind == 'none':
        return iso.IsotopeRatios(['X'] * nspec, [''] * nspec, []), {}
    if kind in ('free', 'full'):
        # free: every slot but the last one, which stays unlabelled where there is more than one;
        # full: every slot (at nspec 32: PB_ISO_MAX_SLOTS labelled slots)
        labelled = list(range(nspec if kind == 'full' else max(1, nspec - 1)))
        labels = [names[i] if i in labelled else '' for i in range(nspec)]
        return iso.IsotopeRatios(['X'] * nspec, labels, [free(i) for i in labelled]), {}
    assert kind == 'fill' and nspec >= 4
    if nspec < 9:
        fills = {0: [1], 2: [1, 3]}                        # two fill slots, 1 and 2 fillers
        labelled = [0, 1, 2, 3]
    else:
        fills = {0: [2], 1: list(range(2, 9))}             # 1 filler and 7
        labelled = list(range(21))
    labels = [names[i] if i in labelled else '' for i in range(nspec)]
    entries = [fill(i, fills[i]) if i in fills else free(i) for i in labelled]
    return iso.IsotopeRatios(['X'] * nspec, labels, entries), fills


def launch(model, temps, dens, pars):
    """pb_iso_density at the C ABI on sentinel-filled, guarded outputs -> host (dens_out,
    temps_out, ratios_out, reject_out)."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream, dev
    nw, nlayers = temps.shape
    temps_d, dens_d = dev(np.array(temps)), dev(np.array(dens))
    pars_d = None if pars is None or model.npars == 0 else dev(np.array(pars))
    outs = (Dirty((nw, nlayers, model.nspec)), Dirty((nw, nlayers)), Dirty((nw, model.nspec)),
            Dirty((nw,), torch.int32, -77))
    st = model.model_struct(pars_d is not None)
    _capi.call('pb_iso_density', outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
               _ptr(dens_d), _ptr(temps_d), _ptr(pars_d), C.byref(st), nlayers, nw, _stream())
    torch.cuda.synchronize()
    for o in outs:
        assert o.guards_intact()
    assert np.array_equal(host(temps_d), temps) and np.array_equal(host(dens_d), dens)
    return tuple(host(o.body) for o in outs)


WORST = {'ratio': 0.0}


@pytest.mark.parametrize('nspec', [1, 4, 32])
@pytest.mark.parametrize('L', [2, 51])
@pytest.mark.parametrize('nw', [1, 5, 67])
def test_kernel_boundary(eng, nw, L, nspec):
    from pyratbay_amd import isotopes as iso
    from pyratbay_amd.atmosphere import REJECT_ISOTOPE
    rng = np.random.default_rng(1000 * nw + 10 * L + nspec)
    temps = rng.uniform(600.0, 2000.0, (nw, L))
    dens = 10.0**rng.uniform(8.0, 16.0, (nw, L, nspec))
    for kind in ('none', 'free') + (('fill',) if nspec >= 4 else ()) + \
            (('full',) if nspec == 32 else ()):
        model, fills = boundary_model(kind, nspec)
        pars = rng.uniform(-4.0, -1.0, (nw, model.npars))
        bad = set()
        if nw >= 5 and model.npars:
            pars[1, model.npars - 1] = np.nan
            pars[nw - 1, 0] = np.inf
            bad = {1, nw - 1}
            if fills:
                # the second fill slot goes negative: two of its fillers sum above 1 (the first
                # fill slot, 1 - 10**-0.1, stays positive)
                pars[3, [model.par_column[j] for j in fills[0]]] = -0.1
                pars[3, model.par_column[fills[2][-1] if 2 in fills else fills[1][-1]]] = -0.05
                bad.add(3)
        for given in (pars, None):
            d, t, r, reject = launch(model, temps, dens, given)
            rejected = set() if given is None else bad
            want = model.ratios_host(pars) if given is not None else \
                np.tile(model.iso_ratios, (nw, 1))
            _, _, want_reject = model.scale_host(temps, dens, given)
            assert set(np.flatnonzero(want_reject)) == rejected
            assert np.array_equal(reject, want_reject), (kind, reject)
            assert np.all(reject[list(rejected)] == REJECT_ISOTOPE)
            good = [w for w in range(nw) if w not in rejected]
            # given the device's own ratios: one multiply, the sequential sum, exact ones
            assert np.array_equal(bits(d[good]), bits(dens[good] * r[good][:, None, :])), kind
            assert np.array_equal(bits(t[good]), bits(temps[good]))
            for i in range(nspec):
                if model.kind[i] == iso.KIND_CONST:
                    assert np.all(r[:, i] == 1.0)
                    assert np.array_equal(bits(d[good][:, :, i]), bits(dens[good][:, :, i]))
                elif model.kind[i] == iso.KIND_FILL:
                    total = r[:, model.iso_fill[i][0]].copy()
                    for j in model.iso_fill[i][1:]:
                        total = total + r[:, j]
                    assert np.array_equal(bits(r[good, i]), bits(1.0 - total[good])), (kind, i)
            for w in rejected:
                assert np.all(d[w] == 0.0) and np.all(t[w] == 0.0), (kind, w)
            if kind == 'none':
                assert np.array_equal(bits(d), bits(dens))
            if given is None:
                # constants formed on the host: the bits of the host's defaults
                assert np.array_equal(bits(r), bits(want))
                continue
            free = np.flatnonzero(model.kind == iso.KIND_FREE)
            if len(free) and good:
                dev_ = max_rel(r[good][:, free], want[good][:, free])
                WORST['ratio'] = max(WORST['ratio'], dev_)
                print(f'nw {nw} L {L} nspec {nspec} {kind}: free ratios vs ratios_host max rel '
                      f'{dev_:.2e} (worst so far {WORST["ratio"]:.2e}, tolerance {TOL_RATIO:.0e})')
                assert dev_ <= TOL_RATIO
            for w in rejected:
                # (the ratios as formed: the same non-finite or negative value as on the host)
                with np.errstate(invalid='ignore'):
                    assert np.any(~np.isfinite(r[w]) | (r[w] < 0.0))


def test_kernel_refusals_and_noops(eng):
    import torch
    from pyratbay_amd import _capi, isotopes as iso
    from pyratbay_amd._device import _stream
    model, _ = boundary_model('fill', 4)
    null = C.c_void_p(None)
    # nw = 0 launches nothing, with null pointers
    _capi.call('pb_iso_density', null, null, null, null, null, null, null,
               C.byref(model.model_struct(True)), 5, 0, _stream())
    t, d, reject, ratios = model.scale(torch.empty((0, 5), dtype=torch.float64, device='cuda'),
                                       torch.empty((0, 5, 4), dtype=torch.float64, device='cuda'))
    assert d.shape == (0, 5, 4) and reject.shape == (0,) and ratios is None

    def refused(match, **change):
        st = iso.IsoModelStruct.from_buffer_copy(model.model_struct(True))
        for name, value in change.items():
            field = getattr(st, name)
            if isinstance(value, tuple):
                if len(value) == 3:
                    field[value[0]][value[1]] = value[2]
                else:
                    field[value[0]] = value[1]
            else:
                setattr(st, name, value)
        buf = torch.zeros(64, dtype=torch.float64, device='cuda')
        p = C.c_void_p(buf.data_ptr())
        with pytest.raises(_capi.PbError, match=match):
            _capi.call('pb_iso_density', p, p, p, p, p, p, p, C.byref(st), 2, 1, _stream())
    refused('table slots', nspec=0)
    refused('labelled slots', nlabelled=33)
    refused('is table slot', slot=(1, 4))
    refused('labelled twice', slot=(1, 0))
    refused('kind 3', kind=(1, 3))
    refused('reads column', par=(1, 2))
    refused('fillers', nfill=(0, 8))
    refused('fill slot itself', fill=(0, 0, 2))
    with pytest.raises(_capi.PbError, match='needs pars'):
        buf = torch.zeros(64, dtype=torch.float64, device='cuda')
        p = C.c_void_p(buf.data_ptr())
        _capi.call('pb_iso_density', p, p, p, p, p, p, null, C.byref(model.model_struct(True)), 2,
                   1, _stream())


# -------------------------------------------------------------------------------------------------
# 2. the loader
# -------------------------------------------------------------------------------------------------
def test_loader_equals_the_reference(eng, g29, tmp_path_factory):
    from pyratbay_amd import opacity_table as ot
    block = str(g29['block'])
    folder = str(tmp_path_factory.mktemp('tables'))
    for key in ('12C-16O', '13C-16O', '12C-18O', '13C'):
        assert key not in folder
    names = [str(n) for n in g29['a_file_names']]
    paths = []
    for i, (name, sp) in enumerate(zip(names, g29['a_file_species'])):
        paths.append(os.path.join(folder, name))
        ot.write_opacity(paths[-1], str(sp), g29['a_temp'], g29['a_press'], g29['a_wn'],
                         g29[f'a_file{i}_cs'])
    cs = ot.load_cross_sections(paths, isotope_ratios=block)
    assert [str(s) for s in cs.species] == [str(s) for s in g29['a_species']]
    assert cs.isotopes.isotopes == [str(s) for s in g29['a_isotopes']]
    assert cs.isotopes.pnames == [str(s) for s in g29['a_pnames']]
    assert np.array_equal(bits(cs.isotopes.iso_ratios), bits(g29['a_iso_ratios']))
    got = host(cs.cs_table)
    assert got.shape == g29['a_cs_table'].shape == (4, 4, 7, 33)
    # the files are on the table's grid: untouched values bit for bit, the added slot a sum
    np.testing.assert_allclose(got, g29['a_cs_table'], rtol=1e-12)
    for slot, i in ((0, 0), (2, 2), (3, 3)):
        assert np.array_equal(got[slot], g29[f'a_file{i}_cs'])
    assert np.array_equal(got[1], g29['a_file1_cs'] + g29['a_file4_cs'])
    # without the block: one slot per species, as before
    plain = ot.load_cross_sections(paths)
    assert [str(s) for s in plain.species] == ['CO', 'H2O'] and plain.isotopes is None
    for key in ('multiple', 'filler'):
        with pytest.raises(ValueError) as e:
            ot.load_cross_sections(paths, isotope_ratios=str(g29[f'a_error_{key}_block']))
        assert str(e.value).replace(folder + os.sep, '') == str(g29[f'a_error_{key}'])
    # the model of such a table carries the isotope model
    model = cs.table_spectrum(np.linspace(7.2e9, 6.9e9, 7), 8.8e10)
    assert model.isotopes is cs.isotopes


# -------------------------------------------------------------------------------------------------
# 3. every form of eval_bands
# -------------------------------------------------------------------------------------------------
NW = 5
REJECTED = 2


def forms_case(golden, geom):
    """test_gpu_batch_clouds' small case (L = 51, W = 402, three table slots) with the slots taken
    as three CO isotopologues; walker 2 has a negative filler."""
    import test_gpu_batch_clouds as clouds
    from pyratbay_amd import isotopes as iso
    s = clouds.build_case(golden('g11_patchy'), NW, 29, geom)
    entries = iso.parse('12C-16O 12CO fill_13CO_C18O\n13C-16O 13CO -1.95\n12C-18O C18O -2.7')
    s['iso'] = iso.IsotopeRatios(['CO'] * 3, ['iso_12CO', 'iso_13CO', 'iso_C18O'], entries)
    pars = s['rng'].uniform(-3.0, -0.7, (NW, 2))
    pars[REJECTED] = NEGATIVE_FILLER
    s['iso_pars'] = pars
    return s


FORMS = [('transit', 'grid'), ('transit', 'ordered'), ('transit', 'auto'), ('transit', 'one_pass'),
         ('emission', 'grid'), ('emission', 'ordered'), ('two_stream', 'grid'),
         ('transit', 'clouds'), ('emission', 'clouds'), ('transit', 'contribution'),
         ('emission', 'contribution'), ('transit', 'hires'), ('emission', 'hires')]


@pytest.mark.parametrize('geom,form', FORMS)
def test_every_form_equals_the_prescaled_route(eng, golden, geom, form):
    """The model with isotopes and iso_pars equals, bit for bit, a model on the same table without
    isotopes fed dens * ratios (the ratios read back from the device); the walker with a negative
    filler is +inf and its neighbours keep their bits; iso_pars=None equals the defaults."""
    import torch
    import test_gpu_batch_clouds as clouds
    s = forms_case(golden, 'transit' if geom == 'transit' else 'emission')
    iso, dev = s['iso'], eng.dev
    wn, W, L = s['wn'], s['W'], s['L']
    cont = clouds.continuum_of(s, True) if form == 'clouds' else None
    order = {'ordered': np.random.default_rng(3).permutation(W), 'auto': 'auto'}.get(form)

    def model_of(isotopes):
        m = eng.TableSpectrum(s['etable'], s['ttable'], wn, s['radius'][0], clouds.RSTAR,
                              rt_path=geom, column_order=order, continuum=cont,
                              isotopes=isotopes)
        if form == 'one_pass':
            m.one_pass = True
        return m
    with_iso, plain = model_of(iso), model_of(None)
    _, pb = clouds.make_bands(eng, wn)
    bands, kw = pb, dict(radius=dev(s['radius']), chunk=2)
    if form == 'clouds':
        kw.update(continuum_density=dev(s['cdens']), continuum_pars=dev(s['pars']),
                  deck_logp=dev(s['logp']), f_patchy=dev(s['fpatchy']))
    if form == 'hires':
        bands = eng.HiresData(wn, np.linspace(wn[30], wn[-30], 57),
                              0.25 * wn[0] / (wn[1] - wn[0]), rv_max=30.0)
        kw['rv'] = dev(s['rng'].uniform(-20, 20, NW))
    outs = {}
    if form == 'contribution':
        for key in ('iso', 'plain', 'default', 'explicit'):
            outs[key] = torch.full((NW, L, pb.nbands), float('nan'), dtype=torch.float64,
                                   device='cuda')
        if geom != 'transit':
            kw['contribution_pressure'] = s['pressure']
    temps, dens, pars = dev(s['temps']), dev(s['dens']), dev(s['iso_pars'])
    _, scaled, reject, ratios = iso.scale(temps, dens, pars, want_ratios=True)
    assert list(host(reject) != 0) == [w == REJECTED for w in range(NW)]
    assert float(ratios[REJECTED, 0]) < 0.0
    pre = (dens * ratios[:, None, :]).contiguous()
    pre[REJECTED] = pre[0]                # (no negative densities into the model without isotopes)

    def run(model, d, key, **more):
        extra = dict(kw, **more)
        if form == 'contribution':
            extra['contribution_out'] = outs[key]
        spectra = torch.empty((NW, W), dtype=torch.float64, device='cuda')
        return model.eval_bands(temps, d, bands, spectra_out=spectra, **extra), spectra
    got, got_spec = run(with_iso, dens, 'iso', iso_pars=pars)
    want, want_spec = run(plain, pre, 'plain')
    torch.cuda.synchronize()
    good = [w for w in range(NW) if w != REJECTED]
    assert bool(torch.isposinf(got[REJECTED]).all())
    assert bool(torch.isfinite(got[good]).all())
    assert torch.equal(got[good], want[good]) and torch.equal(got_spec[good], want_spec[good])
    if form == 'contribution':
        a, b = outs['iso'][good], outs['plain'][good]
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    if form == 'auto':
        assert with_iso.column_order is not None and plain.column_order is not None
    # iso_pars = None: the host's defaults, bit for bit the plain model fed dens * defaults ...
    default, default_spec = run(with_iso, dens, 'default')
    ratios0 = iso.scale(temps, dens, want_ratios=True)[3]
    assert np.array_equal(bits(host(ratios0)), bits(np.tile(iso.iso_ratios, (NW, 1))))
    want0, want0_spec = run(plain, (dens * ratios0[:, None, :]).contiguous(), 'plain')
    assert torch.equal(default, want0) and torch.equal(default_spec, want0_spec)
    if form == 'contribution':
        assert torch.equal(torch.isnan(outs['default']), torch.isnan(outs['plain']))
        assert torch.equal(torch.nan_to_num(outs['default']), torch.nan_to_num(outs['plain']))
    # ... and the defaults passed explicitly (measured on the MI355X in all 13 forms: 0, so equal
    # bits; the device's pow has the host's bits at -1.95 and -2.7)
    explicit, _ = run(with_iso, dens, 'explicit', iso_pars=dev(np.tile(iso.pars, (NW, 1))))
    dev_ = max_rel(host(default), host(explicit))
    print(f'{geom} {form}: defaults (host constants) vs the defaults as parameters max rel '
          f'{dev_:.2e}')
    assert bool(torch.isfinite(default).all())
    assert torch.equal(default, explicit)


def test_model_refusals(eng, golden):
    import torch
    import test_gpu_batch_clouds as clouds
    s = forms_case(golden, 'transit')
    dev = eng.dev
    _, pb = clouds.make_bands(eng, s['wn'])

    def model_of(isotopes, **kw):
        return eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['radius'][0], clouds.RSTAR,
                                 isotopes=isotopes, **kw)
    temps, dens, pars = dev(s['temps']), dev(s['dens']), dev(s['iso_pars'])
    launches = []
    from pyratbay_amd import table
    real = table.batch.interp_ec_batch
    table.batch.interp_ec_batch = lambda *a, **k: launches.append(1) or real(*a, **k)
    try:
        with pytest.raises(ValueError, match='iso_pars on a model without isotope ratios'):
            model_of(None).eval_bands(temps, dens, pb, iso_pars=pars)
        with pytest.raises(ValueError, match=r'iso_pars must be a float64 device tensor of shape '
                                             r'\(5, 2\)'):
            model_of(s['iso']).eval_bands(temps, dens, pb, iso_pars=pars[:, :1].contiguous())
        with pytest.raises(ValueError, match='iso_pars must be a float64 device tensor'):
            model_of(s['iso']).eval_bands(temps, dens, pb, iso_pars=s['iso_pars'])
        with pytest.raises(ValueError, match='dens must have shape'):
            model_of(s['iso']).eval_bands(temps, dens[:, :, :2].contiguous(), pb)
    finally:
        table.batch.interp_ec_batch = real
    assert launches == []
    with pytest.raises(ValueError, match='the model has 3 slots, the table 2'):
        eng.TableSpectrum(s['etable'][:2], s['ttable'], s['wn'], s['radius'][0], clouds.RSTAR,
                          isotopes=s['iso'])
    two_stream = model_of(s['iso'], rt_path='two_stream')
    with pytest.raises(ValueError, match='a model with isotope ratios'):
        two_stream.radiative_equilibrium(s['pressure'], np.full((s['L'], 3), 1e-4),
                                         np.array([28.0, 29.0, 30.0]))
    # the one-walker eval(): row 0 of the batch's spectra, a host vector of parameters
    model = model_of(s['iso'], column_order=None)
    spectra = torch.empty((NW, s['W']), dtype=torch.float64, device='cuda')
    model.eval_bands(temps, dens, pb, radius=dev(s['radius'][:1]), iso_pars=pars,
                     spectra_out=spectra)
    one = model.eval(s['temps'][0], s['dens'][0], iso_pars=s['iso_pars'][0]).clone()
    ratios = s['iso'].scale(temps, dens, pars, want_ratios=True)[3]
    pre = (dens[0] * ratios[0][None, :]).contiguous()
    assert torch.equal(one, model_of(None, column_order=None).eval(s['temps'][0], pre))
    assert bool(torch.isfinite(one).all()) and not torch.equal(one, model.eval(s['temps'][0],
                                                                               s['dens'][0]))
    with pytest.raises(ValueError, match='negative or non-finite isotope ratio'):
        model.eval(s['temps'][0], s['dens'][0], iso_pars=NEGATIVE_FILLER)
    with pytest.raises(ValueError, match='iso_pars on a model without'):
        model_of(None).eval(s['temps'][0], s['dens'][0], iso_pars=s['iso_pars'][0])
    # defaults that give a negative filler are refused too, with iso_pars=None
    from pyratbay_amd import isotopes as iso
    entries = iso.parse('a 12CO fill_13CO_C18O\nb 13CO -0.1\nc C18O -0.2')
    bad = iso.IsotopeRatios(['CO'] * 3, ['iso_12CO', 'iso_13CO', 'iso_C18O'], entries)
    assert bad.iso_ratios[0] < 0.0
    with pytest.raises(ValueError, match='negative or non-finite isotope ratio'):
        model_of(bad, column_order=None).eval(s['temps'][0], s['dens'][0])


# -------------------------------------------------------------------------------------------------
# 4. the whole pipeline against the reference (G29 part B)
# -------------------------------------------------------------------------------------------------
def pipeline_case(eng, g, tag):
    """(model, bands, atmosphere, rows) of a geometry of G29 B; rows: per parameter vector the
    reference's results and the tensors of both entries."""
    from pyratbay_amd import atmosphere as pa, isotopes as iso
    entries = iso.parse(str(g['block']))
    species = [str(s) for s in g[f'{tag}_species']]
    ratios = iso.IsotopeRatios(species, [str(s) for s in g[f'{tag}_isotopes']], entries)
    wn, press = g[f'{tag}_wn'], g[f'{tag}_press']
    rstar = float(g[f'{tag}_rstar'])
    kw = {}
    if tag == 'eclipse':
        kw = dict(quadrature_mu=g['eclipse_quadrature_mu'],
                  quadrature_weights=g['eclipse_quadrature_weights'])
    model = eng.TableSpectrum(g['b_cs_table'], g['b_table_temp'], wn, g[f'{tag}_row_radius'][0],
                              rstar, rt_path='transit' if tag == 'transmission' else 'emission',
                              itop=int(g[f'{tag}_rtop']), maxdepth=float(g[f'{tag}_maxdepth']),
                              isotopes=ratios, **kw)
    bands = []
    for i in range(int(g[f'{tag}_nbands'])):
        resp = g[f'{tag}_band{i}_response'] * (g[f'{tag}_band{i}_wl']
                                               if bool(g[f'{tag}_band{i}_photon']) else 1.0)
        bands.append((int(g[f'{tag}_band{i}_idx'][0]), resp, float(g[f'{tag}_band{i}_height'])))
    pb = eng.PassBands(wn, bands)
    if tag == 'eclipse':
        pb.set_eclipse(float(g['eclipse_row_rplanet'][0]), rstar, g['eclipse_bandflux_star'])
        assert len(set(g['eclipse_row_rplanet'])) == 1
    atm_species = [str(s) for s in g[f'{tag}_atm_species']]
    tmodel = pa.Guillot(press)
    pnames = [str(n) for n in g[f'{tag}_pnames']]
    full = g[f'{tag}_row_full']
    tcols = [pnames.index(n) for n in tmodel.pnames]
    params = np.column_stack([full[:, tcols], full[:, pnames.index('log_H2O')],
                              g[f'{tag}_row_rplanet'], g[f'{tag}_row_mplanet']])
    atm = pa.WalkerAtmosphere(press, atm_species, g[f'{tag}_mol_mass'], g[f'{tag}_base_vmr'],
                              [str(b) for b in g[f'{tag}_bulk']], tmodel,
                              [pa.IsoVMR('H2O', press)], rmodel='hydro_m',
                              refpressure=float(g[f'{tag}_refpressure']),
                              free=list(tmodel.pnames) + ['log_H2O', 'rplanet', 'mplanet'],
                              base_params=params[0])
    atm.bind(species)
    cols = [atm_species.index(s) for s in species]
    iso_pars = full[:, [pnames.index(n) for n in ratios.pnames]]
    return dict(model=model, pb=pb, atm=atm, params=params, iso_pars=iso_pars,
                temps=g[f'{tag}_row_temp'], dens=g[f'{tag}_row_dens'][:, :, cols],
                radius=g[f'{tag}_row_radius'], want=g[f'{tag}_row_bandflux'], iso=ratios)


@pytest.mark.parametrize('tag', ['transmission', 'eclipse'])
def test_pipeline_against_the_reference(eng, g29, tag):
    """The band fluxes of the reference's pb.run() + eval() with an isotope_ratios block, entered
    at eval_bands with the reference's own temp / dens / radius and at eval_params with a
    WalkerAtmosphere built from the fixture.  Every vector with a finite reference result; the
    vector with a negative filler must be +inf here (the fixture only documents what the
    reference returns there: -inf band fluxes in transit, NaN in eclipse geometry)."""
    c = pipeline_case(eng, g29, tag)
    dev = eng.dev
    want = c['want']
    finite = np.all(np.isfinite(want), axis=1)
    assert list(finite) == [True] * 5 + [False]
    assert tuple(c['iso_pars'][5]) == NEGATIVE_FILLER
    assert np.array_equal(bits(c['iso'].ratios_host(c['iso_pars'])),
                          bits(g29[f'{tag}_row_iso_ratios']))
    # the ratios move the result: the second vector differs from the first by the ratios alone
    assert np.max(np.abs(want[1] / want[0] - 1)) > 2e-3
    pars = dev(c['iso_pars'])
    got = host(c['model'].eval_bands(dev(c['temps']), dev(c['dens']), c['pb'],
                                     radius=dev(c['radius']), iso_pars=pars, chunk=4))
    dev_ = max_rel(got[finite], want[finite])
    tol = TOL_BANDS['eval_bands', tag]
    print(f'{tag}: band fluxes vs the reference, entered at eval_bands: max rel {dev_:.2e} '
          f'(tolerance {tol:.0e})')
    assert np.all(np.isposinf(got[5]))
    assert dev_ <= tol
    got = host(c['model'].eval_params(c['atm'], dev(c['params']), c['pb'], iso_pars=pars,
                                      chunk=4))
    dev_ = max_rel(got[finite], want[finite])
    tol = TOL_BANDS['eval_params', tag]
    print(f'{tag}: band fluxes vs the reference, entered at eval_params: max rel {dev_:.2e} '
          f'(tolerance {tol:.0e})')
    assert np.all(np.isposinf(got[5]))
    assert dev_ <= tol


# -------------------------------------------------------------------------------------------------
# 5. the retrieval front end
# -------------------------------------------------------------------------------------------------
def retrieval_of(eng, g29, c, c18o_line, **kw):
    block = str(g29['b_retrieval_params'])
    lines = [line for line in block.split('\n') if line.strip()]
    assert lines[-1].split()[0] == 'iso_C18O'
    lines[-1] = c18o_line
    rng = np.random.default_rng(7)
    data = c['want'][0] * (1 + rng.normal(0, 0.01, 3))
    obs = eng.Observation(data, 0.02 * c['want'][0])
    return eng.Retrieval(c['model'], c['atm'], c['pb'], obs, '\n'.join(lines), chunk=2, **kw), obs


@pytest.mark.parametrize('c18o', ['fixed', 'shared'])
def test_retrieval(eng, g29, c18o):
    import torch
    c = pipeline_case(eng, g29, 'transmission')
    line = {'fixed': 'iso_C18O  -2.7  -5.0  -0.05  0.0',
            'shared': 'iso_C18O  -2.7  -5.0  -0.05  -10'}
    ret, obs = retrieval_of(eng, g29, c, line[c18o])
    model, atm, pb = c['model'], c['atm'], c['pb']
    assert ret.dest_names == ['params', 'iso_pars'] and ret.dest_ncols == [9, 2]
    assert ret.iso_pnames == ['iso_13CO', 'iso_C18O']
    assert ret.opacity_pnames == ['iso_13CO', 'iso_C18O']
    assert 'iso_13CO' in ret.available and 'iso_C18O' in ret.available
    # the index maps of the reference
    assert ret.iopacity == {'line sampling': [int(i) for i in g29['transmission_iopacity']]}
    assert ret.map_pars['opacity'] == {'line sampling':
                                       [int(i) for i in g29['transmission_map_opacity']]}
    free = [ret.pnames[i] for i in ret.ifree]
    assert 'iso_13CO' in free and 'iso_C18O' not in free
    nw = 5
    rng = np.random.default_rng(3)
    f = ret.ifree
    theta = ret.params[f] + 0.3 * ret.pstep[f] * rng.uniform(-1, 1, (nw, ret.nfree))
    col = free.index('iso_13CO')
    theta[:, col] = rng.uniform(-3.0, -1.0, nw)
    negative = 3 if c18o == 'shared' else None
    if negative is not None:
        theta[negative, col] = -0.1               # the shared C18O follows: 2 x 0.79 > 1
    assert np.all(ret.inside_host(theta))
    split = ret.split_host(theta)
    assert split['iso_pars'].shape == (nw, 2)
    assert np.array_equal(split['iso_pars'][:, 0], theta[:, col])
    assert np.array_equal(split['iso_pars'][:, 1],
                          theta[:, col] if c18o == 'shared' else np.full(nw, -2.7))
    tensors = {k: eng.dev(v) for k, v in split.items()}
    params = tensors.pop('params')
    want = model.eval_loglike(atm, params, pb, obs, chunk=2, **tensors)
    theta_d = eng.dev(theta)
    args = ret.arguments(theta_d)
    assert set(args.kw) == {'iso_pars'}
    assert np.array_equal(bits(host(args.kw['iso_pars'])), bits(split['iso_pars']))
    got = ret.log_likelihood(theta_d)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(got)), bits(host(want)))
    post = host(ret.log_posterior(theta_d))
    got = host(got)
    good = [w for w in range(nw) if w != negative]
    assert np.all(got[good] > -1e6), got
    if negative is not None:
        assert got[negative] == -1.0e98
        assert np.isfinite(post[negative]) and post[negative] < -9e97
    flux = ret.bandflux(theta_d)
    assert torch.equal(flux, model.eval_params(atm, params, pb, chunk=2, **tensors))
    assert bool(torch.isfinite(flux[good]).all())
    # nothing is read back between theta and the result
    reads = []
    real = torch.Tensor.cpu

    def spy(self, *a, **k):
        reads.append(1)
        return real(self, *a, **k)
    torch.Tensor.cpu = spy
    try:
        again = ret.log_posterior(theta_d)
    finally:
        torch.Tensor.cpu = real
    assert reads == [] and torch.equal(again.cpu(), torch.as_tensor(post))


def test_retrieval_names_and_samplers(eng, g29):
    import torch
    c = pipeline_case(eng, g29, 'transmission')
    with pytest.raises(ValueError) as e:
        retrieval_of(eng, g29, c, 'iso_xx  -2.7  -5.0  -0.05  0.3')
    assert "Invalid retrieval parameter 'iso_xx'" in str(e.value)
    assert "'iso_13CO'" in str(e.value) and "'iso_C18O'" in str(e.value)
    # a column nobody names takes the model's default
    block = '\n'.join(line for line in str(g29['b_retrieval_params']).split('\n')
                      if line.strip() and 'iso_C18O' not in line)
    obs = eng.Observation(c['want'][0], 0.02 * c['want'][0])
    ret = eng.Retrieval(c['model'], c['atm'], c['pb'], obs, block, chunk=4)
    assert ret.dest_names == ['params', 'iso_pars']
    split = ret.split_host(ret.params[ret.ifree][None])
    assert np.array_equal(split['iso_pars'], [[-1.95, -2.7]])
    # a model without isotopes does not know the names
    plain = eng.TableSpectrum(g29['b_cs_table'], g29['b_table_temp'], g29['transmission_wn'],
                              g29['transmission_row_radius'][0], 8.8e10)
    with pytest.raises(ValueError, match="Invalid retrieval parameter 'iso_13CO'"):
        eng.Retrieval(plain, c['atm'], c['pb'], obs, block)
    # the keyword reaches the samplers and the summary
    ret, _ = retrieval_of(eng, g29, c, 'iso_C18O  -2.7  -5.0  -0.05  0.3')
    f = ret.ifree
    z0 = ret.params[f] + 0.1 * ret.pstep[f] * \
        np.random.default_rng(4).standard_normal((30, len(f)))
    demc = ret.sample(6, 4, seed=2, z0=z0)
    theta, counts = demc.unique()
    assert theta.shape[1] == ret.nfree and int(counts.sum()) > 0
    ns = ret.nested(nlive=12, seed=2, dlogz=None, nsteps=3)
    ns.run(2)
    assert ns.it == 2
    summary = ret.summary(demc, chunk=4)
    assert summary.bands.shape[1] == 3 and bool(torch.isfinite(summary.bands).all())


# -------------------------------------------------------------------------------------------------
# 6. the posterior summary
# -------------------------------------------------------------------------------------------------
def test_posterior_summary(eng, g29):
    """With iso_pars rows: vmr is the atmosphere's, unscaled and repeated for a repeated species;
    the spectrum and band quantiles have the bits of the pre-scaled route."""
    import torch
    from pyratbay_amd.atmosphere import BAR, K_BOLTZ
    c = pipeline_case(eng, g29, 'transmission')
    dev = eng.dev
    model, atm, pb = c['model'], c['atm'], c['pb']
    n = 5
    params, pars = dev(c['params'][:n]), dev(c['iso_pars'][:n])
    counts = np.array([3, 1, 2, 1, 4])
    got = model.posterior_summary(atm, params, counts, pb, iso_pars=pars, chunk=2,
                                  keep_stores=True)
    assert got.n_rejected == 0
    vmr = host(got.stores['vmr'])                            # [L, nspec, n]
    assert vmr.shape == (51, 4, n)
    assert np.array_equal(bits(vmr[:, 0]), bits(vmr[:, 1]))
    assert np.array_equal(bits(vmr[:, 0]), bits(vmr[:, 2]))
    prof = atm.evaluate(params)
    pk = dev(np.asarray(atm.pressure, float) * BAR / K_BOLTZ)
    want_vmr = host((prof.dens * (prof.temps / pk).unsqueeze(2)).permute(1, 2, 0))
    assert np.array_equal(bits(vmr), bits(want_vmr))
    np.testing.assert_allclose(vmr[:, 0, 0], 5e-4, rtol=1e-3)          # CO's VMR, not 13CO's
    # the pre-scaled route: the same table without isotopes, densities scaled by the device
    plain = eng.TableSpectrum(g29['b_cs_table'], g29['b_table_temp'], g29['transmission_wn'],
                              c['radius'][0], float(g29['transmission_rstar']),
                              itop=int(g29['transmission_rtop']),
                              maxdepth=float(g29['transmission_maxdepth']))
    _, scaled, _, _ = c['iso'].scale(prof.temps, prof.dens, pars)
    spectra = torch.empty((n, model.nwave), dtype=torch.float64, device='cuda')
    flux = plain.eval_bands(prof.temps, scaled, pb, radius=prof.radius, chunk=2,
                            spectra_out=spectra)
    assert np.array_equal(bits(host(got.stores['spectrum'])), bits(host(spectra.t())))
    assert np.array_equal(bits(host(got.stores['bands'])), bits(host(flux.t())))
    from pyratbay_amd import posterior
    want = posterior.weighted_quantiles(spectra.t().contiguous(), dev(counts, torch.int64),
                                        got.quantiles, total=int(counts.sum()))
    assert torch.equal(got.spectrum, want)
    # a rejected sample is counted out
    pars_bad = pars.clone()
    pars_bad[1] = dev(np.array(NEGATIVE_FILLER))
    bad = model.posterior_summary(atm, params, counts, pb, iso_pars=pars_bad, chunk=2)
    assert bad.n_rejected == 1
    with pytest.raises(ValueError, match='iso_pars must have one row per sample'):
        model.posterior_summary(atm, params, counts, pb, iso_pars=pars[:3])


# -------------------------------------------------------------------------------------------------
# 7. bind with a repeated table species
# -------------------------------------------------------------------------------------------------
def test_bind_repeated_species(eng, g29):
    c = pipeline_case(eng, g29, 'transmission')
    atm = c['atm']
    assert atm._table_species == ['CO', 'CO', 'CO', 'H2O']
    prof = atm.evaluate(eng.dev(c['params'][:3]))
    dens = host(prof.dens)
    assert dens.shape == (3, 51, 4)
    assert np.array_equal(bits(dens[:, :, 0]), bits(dens[:, :, 1]))
    assert np.array_equal(bits(dens[:, :, 0]), bits(dens[:, :, 2]))
    assert not np.array_equal(dens[:, :, 0], dens[:, :, 3])
    for w in range(3):
        want = atm.evaluate_host(c['params'][w])
        assert want.dens.shape == (51, 4) and want.reject == 0
        dev_ = max_rel(dens[w], want.dens)
        print(f'walker {w}: dens vs evaluate_host max rel {dev_:.2e} (tolerance 1e-14, the '
              'density tolerance of test_gpu_atmosphere.py)')
        assert dev_ <= 1e-14


# -------------------------------------------------------------------------------------------------
# 8. graph capture
# -------------------------------------------------------------------------------------------------
def test_graph_capture(eng, g29):
    """One eval_params call with iso_pars, streams = 1 (no parallel branch), captured and
    replayed: the band fluxes of the eager call, bit for bit."""
    import torch
    from test_gpu_atmosphere import capture_or_skip
    capture_or_skip(torch)
    c = pipeline_case(eng, g29, 'transmission')
    dev = eng.dev
    model, atm, pb = c['model'], c['atm'], c['pb']
    model.set_column_order(None)
    model._auto_order = False
    params, pars = dev(c['params']), dev(c['iso_pars'])
    eager = model.eval_params(atm, params, pb, iso_pars=pars, chunk=4, streams=1).clone()
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.copy_(model.eval_params(atm, params, pb, iso_pars=pars, chunk=4, streams=1))
    torch.cuda.synchronize()
    assert not out.any()                              # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert bool(torch.isposinf(out[5]).all()) and bool(torch.isfinite(out[:5]).all())
