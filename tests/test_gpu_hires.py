"""High-resolution data in the batched loop (engine.HiresData, csrc/pb_hires.hip) against fixture
G21 = the reference's ps.inst_convolution, ps.rv_shift and scipy's interp1d
(tests/golden/make_golden_hires.py), and against a NumPy restatement of those three steps.

Tolerance: the worst-case rounding of a T-term FMA sum plus the two-point interpolation is
(T + 5) 2^-53 sum|k_t s|; the taps lie in [0, 1], so for positive spectra there is no cancellation
and the bound is relative to the result: T <= 179 -> below 3e-14 -> rtol = 1e-13.  One fixture
kernel (R_inst 100 000 / R_samp 300 000) has taps down to -2.4e-8: there the bound is on
sum|k_t s|, i.e. atol = 1e-13 max|spectrum| on top."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-13
C_LIGHT, KM = 29979245800.0, 1e5        # the reference's pc.c, pc.km


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def g21(golden):
    return golden('g21_hires')


def host(t):
    return t.cpu().numpy()


def cases(g):
    for c in range(int(g['ncases'])):
        r_inst, r_samp = g[f'c{c}_resolution']
        yield c, float(r_inst), (None if np.isnan(r_samp) else float(r_samp))


def atol_of(g, c, spectrum):
    """Only the kernel with negative taps needs the absolute term (module docstring)."""
    return 1e-13 * np.max(np.abs(spectrum)) if np.min(g[f'c{c}_taps']) < 0 else 0.0


def restate(spectra, wn, taps, data_wn, rv=None, sample_scale=None, f_dilution=None):
    """The three steps in NumPy: np.convolve(mode='same'), the shifted grid, interp1d's formula
    (bracket by searchsorted 'left' clipped to [1, W - 1])."""
    nw, nwave = spectra.shape
    out = np.empty((nw, len(data_wn)))
    conv = np.empty_like(spectra)
    for w in range(nw):
        s = spectra[w]
        if f_dilution is not None:
            s = s * f_dilution[w]
        if sample_scale is not None:
            s = s * sample_scale
        conv[w] = c = np.convolve(s, taps, mode='same')
        vel = (0.0 if rv is None else rv[w]) * KM
        x = wn * np.sqrt((1 - vel / C_LIGHT) / (1 + vel / C_LIGHT))
        hi = np.clip(np.searchsorted(x, data_wn, side='left'), 1, nwave - 1)
        lo = hi - 1
        out[w] = (c[hi] - c[lo]) / (x[hi] - x[lo]) * (data_wn - x[lo]) + c[lo]
    return out, conv


def check(got, want, rtol=RTOL, atol=0.0, what=''):
    err = np.max(np.abs(got - want) / (np.abs(want) + (atol / rtol if atol else 0.0)))
    print(f'{what}: max |diff| / (|want| + atol/rtol) = {err:.2e}')
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


def test_convolve_g21(eng, g21):
    """convolve() = the reference's spec.spectrum_convolved, transit depth and eclipse ratio (the
    ratio applied per sample before the convolution)."""
    g = g21
    for c, r_inst, r_samp in cases(g):
        wn = g[f'c{c}_wn']
        h = eng.HiresData(wn, wn[10:20], r_inst, sampling_res=r_samp, rv_max=0.0)
        assert np.array_equal(h.taps_host, g[f'c{c}_taps']) or \
            np.allclose(h.taps_host, g[f'c{c}_taps'], rtol=0, atol=1e-15 * g[f'c{c}_taps'].max())
        depth = g[f'c{c}_depth']
        got = host(h.convolve(eng.dev(np.stack([depth, depth[::-1]]))))
        check(got[0], g[f'c{c}_depth_convolved'], atol=atol_of(g, c, depth),
              what=f'case {c} depth convolved')
        h.set_eclipse(g['radii'][0], g['radii'][1], g[f'c{c}_starflux'])
        got = host(h.convolve(eng.dev(g[f'c{c}_fplanet']).view(1, -1)))[0]
        ratio = g[f'c{c}_fplanet'] / g[f'c{c}_starflux'] * (g['radii'][0] / g['radii'][1])**2
        check(got, g[f'c{c}_eclipse_convolved'], atol=atol_of(g, c, ratio),
              what=f'case {c} eclipse convolved')


@pytest.mark.parametrize('fused', [True, False])
def test_sampled_g21(eng, g21, fused):
    """integrate_batch() = interp1d(rv_shift(wn), inst_convolution(spectrum))(data) of the
    reference, in the caller's (shuffled) order, data on grid nodes and at both ends of the grid
    included; transit depth and eclipse; the fused launch and the two-launch form."""
    import torch
    g = g21
    for c, r_inst, r_samp in cases(g):
        wn = g[f'c{c}_wn']
        depth, fplanet = g[f'c{c}_depth'], g[f'c{c}_fplanet']
        for r, rv in enumerate(g['rv']):
            data_wn = g[f'c{c}_rv{r}_data_wn']
            assert not np.all(np.diff(data_wn) > 0)             # (shuffled)
            # (the data reach both ends of the grid shifted by THIS rv: no host check)
            h = eng.HiresData(wn, data_wn, r_inst, sampling_res=r_samp, rv_max=40.0,
                              check_data=False)
            h.fused = fused
            # walker 0 carries the case's rv; its neighbour another spectrum and no shift (which
            # may cost it the data at the ends: only walker 0 is looked at)
            rvs = eng.dev(np.array([rv, 0.0]))
            got = host(h.integrate_batch(eng.dev(np.stack([depth, 2.0 * depth])), rv=rvs))
            check(got[0], g[f'c{c}_rv{r}_depth_sampled'], atol=atol_of(g, c, depth),
                  what=f'case {c} rv {rv} depth')
            h.set_eclipse(g['radii'][0], g['radii'][1], g[f'c{c}_starflux'])
            got = host(h.integrate_batch(eng.dev(fplanet).view(1, -1), rv=rvs[:1]))
            ratio = fplanet / g[f'c{c}_starflux'] * (g['radii'][0] / g['radii'][1])**2
            check(got[0], g[f'c{c}_rv{r}_eclipse_sampled'], atol=atol_of(g, c, ratio),
                  what=f'case {c} rv {rv} eclipse')
            # f_dilution: per sample, before the eclipse ratio and the convolution
            fd = np.array([0.75])
            got = host(h.integrate_batch(eng.dev(fplanet).view(1, -1), rv=rvs[:1],
                                         f_dilution=eng.dev(fd)))
            want, _ = restate(fplanet[None], wn, g[f'c{c}_taps'], data_wn, rv=[rv],
                              sample_scale=host(h.sample_scale), f_dilution=fd)
            check(got, want, atol=atol_of(g, c, ratio), what=f'case {c} rv {rv} diluted')
            np.testing.assert_allclose(got[0], 0.75 * g[f'c{c}_rv{r}_eclipse_sampled'],
                                       rtol=2 * RTOL, atol=atol_of(g, c, ratio))
        torch.cuda.synchronize()


def test_one_batch_every_rv(eng, g21):
    """Every case: ONE batch whose walkers carry the fixture's three rv.  The data are the three
    data sets together (the points that stay inside the grid for every |rv| <= 31 km/s); walker r
    is compared at the points of set r with the reference's values, everywhere with the NumPy
    restatement; the fused launch and the two-launch form give the same bits."""
    import torch
    from pyratbay_amd import hires
    g = g21
    rvs = g['rv']
    for c, r_inst, r_samp in cases(g):
        wn = g[f'c{c}_wn']
        depth = g[f'c{c}_depth']
        lo, hi = wn[0] * hires.doppler_factor(-31.0), wn[-1] * hires.doppler_factor(31.0)
        sets = [g[f'c{c}_rv{r}_data_wn'] for r in range(3)]
        keep = [(d >= lo) & (d <= hi) for d in sets]
        data_wn = np.concatenate([d[k] for d, k in zip(sets, keep)])
        owner = np.concatenate([np.full(k.sum(), r) for r, k in enumerate(keep)])
        assert min(k.sum() for k in keep) > 400
        h = eng.HiresData(wn, data_wn, r_inst, sampling_res=r_samp, rv_max=31.0)
        assert h.nbands == len(data_wn)
        spectra = np.stack([depth, depth, depth, depth[::-1].copy()])
        rv4 = np.array([rvs[0], rvs[1], rvs[2], -12.5])
        got_t = h.integrate_batch(eng.dev(spectra), rv=eng.dev(rv4))
        got = host(got_t)
        atol = atol_of(g, c, depth)
        for r in range(3):
            want = g[f'c{c}_rv{r}_depth_sampled'][keep[r]]
            check(got[r][owner == r], want, atol=atol, what=f'case {c} walker rv {rvs[r]}')
        want, _ = restate(spectra, wn, g[f'c{c}_taps'], data_wn, rv=rv4)
        check(got, want, atol=atol, what=f'case {c} batch vs NumPy')
        h.fused = False
        assert torch.equal(h.integrate_batch(eng.dev(spectra), rv=eng.dev(rv4)), got_t)
        # no rv at all = rv 0
        h.fused = True
        assert torch.equal(h.integrate_batch(eng.dev(spectra))[0], got_t[0])


def test_rejected_walkers(eng, g21):
    """|rv| > rv_max, and data that leave the walker's shifted grid: +inf in every output of that
    walker, the neighbours untouched."""
    import torch
    g = g21
    wn, depth = g['c0_wn'], g['c0_depth']
    r_inst, r_samp = g['c0_resolution']
    data_wn = np.random.default_rng(3).uniform(wn[2], wn[-3], 300)
    data_wn[:2] = wn[2], wn[-3]
    h = eng.HiresData(wn, data_wn, r_inst, sampling_res=r_samp, rv_max=20.0, check_data=False)
    # wn[2] / wn[0] - 1 = 1.6e-5 = 4.9 km/s: at -15 km/s the grid has moved above the lowest data
    rv = np.array([3.0, 25.0, -3.0, -15.0, 0.5, np.nan, -20.0001])
    spectra = eng.dev(np.tile(depth, (len(rv), 1)))
    got = host(h.integrate_batch(spectra, rv=eng.dev(rv)))
    bad = [1, 3, 5, 6]
    ok = [0, 2, 4]
    assert np.all(np.isposinf(got[bad]))
    assert np.all(np.isfinite(got[ok]))
    alone = host(h.integrate_batch(spectra[:len(ok)], rv=eng.dev(rv[ok])))
    assert np.array_equal(got[ok], alone)
    want, _ = restate(host(spectra)[ok], wn, g['c0_taps'], data_wn, rv=rv[ok])
    check(got[ok], want, what='neighbours of rejected walkers')
    # the log-likelihood and the reject pass take the result as they take band fluxes
    ll = host(eng.loglike(torch.as_tensor(got, device='cuda'), eng.dev(got[0]),
                          eng.dev(np.full(300, 1e-5))))
    assert np.all(ll[bad] == -1e98) and np.all(ll[ok] > -1e98)


def test_too_many_taps_is_refused(eng):
    """The C ABI names its limit instead of truncating the kernel."""
    import torch
    from pyratbay_amd import _capi
    x = torch.zeros((1, 4000), dtype=torch.float64, device='cuda')
    taps = torch.ones(1027, dtype=torch.float64, device='cuda')
    with pytest.raises(_capi.PbError, match='at most 1025'):
        _capi.call('pb_inst_convolve_batch', x.data_ptr(), x.clone().data_ptr(), taps.data_ptr(),
                   None, 1027, 4000, 1, None)
    with pytest.raises(_capi.PbError, match='odd'):
        _capi.call('pb_inst_convolve_batch', x.data_ptr(), x.clone().data_ptr(), taps.data_ptr(),
                   None, 4, 4000, 1, None)


class Capture:
    """Stands where the bands stand in eval_bands and keeps the spectra it is handed."""
    nbands = 1

    def integrate_batch(self, spectra, out=None, f_dilution=None):
        self.spectra = spectra.clone()
        self.f_dilution = None if f_dilution is None else f_dilution.clone()
        out.zero_()
        return out


def model_inputs(nwave, nlayers, nw, seed):
    from tools import bench_c5
    inp = bench_c5.inputs(nwave=nwave, nlayers=nlayers)
    temps, dens, radius = bench_c5.walkers(inp, nw, seed)
    return inp, temps, dens, radius


def eval_bands_case(eng, rt_path, column_order, nwave, nlayers, nw, ndata, r_inst, seed=5):
    inp, temps, dens, radius = model_inputs(nwave, nlayers, nw, seed)
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    rng = np.random.default_rng(seed)
    rv = rng.uniform(-30.0, 30.0, nw)
    from pyratbay_amd import hires
    lo, hi = wn[0] * hires.doppler_factor(-30.0), wn[-1] * hires.doppler_factor(30.0)
    data_wn = rng.uniform(lo, hi, ndata)
    data_wn[:8] = (wn * hires.doppler_factor(rv[0]))[rng.integers(100, nwave - 100, 8)]
    model = eng.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'],
                              rt_path=rt_path, column_order=column_order)
    h = eng.HiresData(wn, data_wn, r_inst, rv_max=30.0)
    kw = {}
    fd = None
    if rt_path == 'emission':
        starflux = 2.0e6 * (1.0 + 0.2 * np.sin(np.linspace(0, 40, nwave)))
        h.set_eclipse(atm['radius'][-1], atm['rstar'], starflux)
        fd = rng.uniform(0.7, 1.0, nw)
        kw['f_dilution'] = eng.dev(fd)
    td, dd, rd = eng.dev(temps), eng.dev(dens), eng.dev(radius)
    got = model.eval_bands(td, dd, h, radius=rd, chunk=nw, rv=eng.dev(rv), **kw)
    cap = Capture()
    model.eval_bands(td, dd, cap, radius=rd, chunk=nw, **kw)
    spectra = host(cap.spectra)
    assert spectra.shape == (nw, nwave) and np.all(spectra > 0)
    want, _ = restate(spectra, wn, h.taps_host, data_wn, rv=rv,
                      sample_scale=None if h.sample_scale is None else host(h.sample_scale),
                      f_dilution=fd)
    return model, h, got, want, (td, dd, rd, rv, kw)


@pytest.mark.parametrize('column_order', [None, 'auto'])
@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_eval_bands_hires(eng, rt_path, column_order):
    """eval_bands(bands=HiresData, rv=...) = the spectra eval_bands hands to its bands (same
    kernels, grid order or depth order) followed by the NumPy restatement; chunked = unchunked;
    pb_reject_walkers works on the [nw, ndata] result."""
    import torch
    model, h, got, want, (td, dd, rd, rv, kw) = eval_bands_case(
        eng, rt_path, column_order, 6001, 30, 12, 700, 25000.0)
    assert (column_order is None) == (model.column_order is None)
    check(host(got), want, what=f'eval_bands {rt_path} order {column_order}')
    kw5 = {k: v[:10] for k, v in kw.items()}
    part = model.eval_bands(td[:10], dd[:10], h, radius=rd[:10], chunk=4, rv=eng.dev(rv[:10]),
                            **kw5)
    assert torch.equal(part, got[:10])
    hot = td.clone()
    hot[3, 5] = 3000.5                                          # above the table
    rej = host(model.eval_bands(hot, dd, h, radius=rd, chunk=12, rv=eng.dev(rv), **kw))
    assert np.all(np.isposinf(rej[3])) and np.array_equal(np.delete(rej, 3, 0),
                                                          np.delete(host(got), 3, 0))


def test_rv_needs_hires_data(eng):
    inp, temps, dens, radius = model_inputs(2001, 20, 4, 1)
    g, atm = inp['grid'], inp['atm']
    model = eng.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], atm['radius'], atm['rstar'],
                              column_order=None)
    bands = eng.PassBands(g['wn'], inp['bands'])
    td, dd = eng.dev(temps), eng.dev(dens)
    with pytest.raises(ValueError, match='HiresData'):
        model.eval_bands(td, dd, bands, rv=eng.dev(np.zeros(4)))
    h = eng.HiresData(g['wn'], g['wn'][500:600] + 0.01, 25000.0, rv_max=10.0)
    with pytest.raises(ValueError, match='shape'):
        model.eval_bands(td, dd, h, rv=eng.dev(np.zeros(3)))
    assert model.eval_bands(td, dd, h, rv=eng.dev(np.zeros(4))).shape == (4, 100)


def test_full_size_hires_batch(eng):
    """The shape of test_full_size_c5_batch (64 walkers, 1e5 wavenumbers x 80 layers) with 20 000
    data points at R_inst = 25 000, against the NumPy restatement; the fused call allocates no
    [nw, W] buffer."""
    import torch
    model, h, got, want, (td, dd, rd, rv, kw) = eval_bands_case(
        eng, 'transit', 'auto', 100001, 80, 64, 20000, 25000.0, seed=9)
    assert got.shape == (64, 20000)
    check(host(got), want, what='full size')
    cap = Capture()
    model.eval_bands(td, dd, cap, radius=rd, chunk=64)
    spectra = cap.spectra
    out = torch.empty((64, 20000), dtype=torch.float64, device='cuda')
    rvd = eng.dev(rv)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    h.integrate_batch(spectra, out=out, rv=rvd)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f'fused call: peak allocation grew by {grown} bytes (nw W 8 = {64 * 100001 * 8})')
    assert grown < 64 * 100001 * 8
    assert torch.equal(out, got)
