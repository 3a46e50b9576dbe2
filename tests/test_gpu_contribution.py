"""Band contribution functions on the device (pyratbay_amd/csrc/pb_contribution.hip): the two C-ABI
entries against the NumPy statements of pyratbay_amd/contribution.py on the inputs of
tests/golden/g24_contribution.npz, TableSpectrum.eval_bands(contribution_out=...) in transit,
emission and two-stream geometry against the oracle chain, TableSpectrum.band_contribution, two
runs, poisoned allocations and the refusals.

Bound of the entries (the fixture's docstring has the measurement): max(10 sens, 1e-14) absolute on
the max-normalised result, where sens is the change of the reference's result under a 1e-13
relative perturbation of the depth and 1e-14 is ten times the difference between the interval form
and the weight form of the trapezoid; the NaN pattern (the band of one sample) must be identical
and the L = 2 cases exact.

Bound of eval_bands against the oracle chain: the device's ec and the oracle's agree to 1e-11
relative (the bound the band fluxes of the same chain are held to, test_gpu_batch_memory.RTOL), so
the comparison allows 10 times what a 1e-11 relative perturbation of the oracle's depth does to the
host result, and no less than 1e-13."""
import os

import numpy as np
import pytest

import cases
from pyratbay_amd import contribution as cb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 4
# (L, itop, W, factor on the densities) per geometry: the small retrieval model of
# test_gpu_batch_memory.py; two-stream geometry takes itop = 0
MODELS = {'transit': (33, 2, 700, 1.0), 'emission': (33, 2, 700, 100.0),
          'two_stream': (17, 0, 256, 100.0)}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def g24():
    return np.load(os.path.join(HERE, 'golden', 'g24_contribution.npz'))


def case_names():
    with np.load(os.path.join(HERE, 'golden', 'g24_contribution.npz')) as g:
        return [str(c) for c in g['cases']]


def load_case(g, name):
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + '_')}
    W = len(c['wn'])
    start, count = g[f'W{W}_band_start'], g[f'W{W}_band_count']
    offs = np.concatenate([[0], np.cumsum(count)])
    c['responses'] = [g[f'W{W}_response'][offs[b]:offs[b + 1]] for b in range(len(start))]
    c['indices'] = [np.arange(start[b], start[b] + count[b]) for b in range(len(start))]
    c['bands'] = [(int(start[b]), c['responses'][b], 1.0) for b in range(len(start))]
    c['rt'] = str(c['rt'])
    return c


def host(t):
    return t.cpu().numpy()


def entry(eng, c, pb):
    """The C-ABI entry of the case's geometry on the fixture's own inputs -> [nw, L, nbands]."""
    import torch
    L = c['depth'].shape[1]
    if c['rt'] == 'transit':
        return eng.band_transmittance_batch(eng.dev(c['depth']), eng.dev(c['ideep'], torch.int32),
                                            pb, int(c['itop']))
    return eng.band_contribution_emission_batch(
        eng.dev(c['ec']), eng.dev(-np.diff(c['radius'], axis=1)), eng.dev(c['temps']), pb,
        c['press'], int(c['itop']), L, float(c['maxdepth']))


@pytest.mark.parametrize('name', case_names())
def test_entries_against_the_host_form(eng, g24, name):
    c = load_case(g24, name)
    pb = eng.PassBands(c['wn'], c['bands'])
    got = host(entry(eng, c, pb))
    bound = max(10 * float(c['sens']), 1e-14)
    for w in range(got.shape[0]):
        want = cb.band_contribution_host(c['depth'][w], c['ideep'][w], c['responses'], c['wn'],
                                         c['indices'], rt_path=c['rt'], pressure=c['press'],
                                         planck=c['planck'][w] if 'planck' in c else None)
        assert np.array_equal(np.isnan(got[w]), np.isnan(want)), (name, w)
        ok = ~np.isnan(want)
        err = float(np.max(np.abs(got[w][ok] - want[ok])))
        print(f'{name} walker {w}: max abs error {err:.3e}, bound {bound:.3e}')
        if got.shape[1] == 2:
            assert np.array_equal(got[w][ok], want[ok]), (name, w)
        assert err <= bound, (name, w, err, bound)


@pytest.mark.parametrize('name', ['t_w3', 'e_l40', 'e_md', 'ts_l8'])
def test_two_runs_and_poisoned_allocations(eng, g24, name, monkeypatch):
    """Two runs give the same bits, and so does a run in which every fresh buffer (the work
    buffer and the output included) starts as NaN."""
    import torch
    c = load_case(g24, name)
    pb = eng.PassBands(c['wn'], c['bands'])
    first = entry(eng, c, pb).clone()
    second = entry(eng, c, pb)
    assert torch.equal(torch.nan_to_num(first, nan=-7.0), torch.nan_to_num(second, nan=-7.0))
    real_empty, real_empty_like = torch.empty, torch.empty_like
    made = []

    def fill(t):
        if t.numel() and t.is_floating_point():
            t.fill_(float('nan'))
            made.append(t.numel())
        elif t.numel() and t.dtype in (torch.int32, torch.int64):
            t.fill_(torch.iinfo(t.dtype).min // 2)
        return t
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: fill(real_empty_like(*a, **k)))
    third = entry(eng, c, pb)
    torch.cuda.synchronize()
    assert len(made) >= 2                                # (the output and the work buffer)
    assert torch.equal(torch.nan_to_num(first, nan=-7.0), torch.nan_to_num(third, nan=-7.0))
    assert torch.equal(torch.isnan(first), torch.isnan(third))


# ------------------------------------------------------------------ eval_bands(contribution_out)
_MODEL = {}


def table_model(eng, rt_path):
    """limited_table_model of the geometry, its device tensors, bands that include a band of one
    sample and one of more than two chunks, and per walker the oracle chain's result."""
    if rt_path not in _MODEL:
        L, itop, W, opacity = MODELS[rt_path]
        m = cases.limited_table_model(L, itop, W, opacity=opacity)
        m['bands'] = m['bands'] + [(5, np.ones(1), 1.0), (W - 40, np.linspace(0.5, 1.0, 40), 2.0)]
        m['press'] = np.logspace(-6, 2, L)
        m['td'], m['dd'], m['rd'] = eng.dev(m['temps']), eng.dev(m['dens']), eng.dev(m['radius'])
        m['pb'] = eng.PassBands(m['wn'], m['bands'])
        _MODEL[rt_path] = m
    return _MODEL[rt_path]


def make_model(eng, m, rt_path, column_order):
    return eng.TableSpectrum(m['etable'], m['ttable'], m['wn'], m['radius0'], m['rstar'],
                             itop=m['itop'], rt_path=rt_path, column_order=column_order)


def oracle_contribution(orc, m, rt_path, w, scale=None):
    """band_contribution_host on the oracle's depth of walker w (its own radius profile); scale:
    a factor on the depth (the sensitivity of the result)."""
    L, W, itop = m['nlayers'], m['nwave'], m['itop']
    ec = np.zeros((L, W))
    orc.interp_ec(ec, m['etable'], m['ttable'], m['temps'][w], m['dens'][w], 0, L)
    responses = [np.asarray(b[1], float) for b in m['bands']]
    indices = [np.arange(b[0], b[0] + len(b[1])) for b in m['bands']]
    planck = None
    if rt_path == 'transit':
        depth, ideep = orc.optical_depth_transit(ec, m['radius'][w], itop, L, 10.0)
    else:
        depth = np.zeros((L, W))
        ideep = np.full(W, L - 1, np.int32)
        orc.plane_parallel_optical_depth(depth, ideep, ec, -np.diff(m['radius'][w]),
                                         np.inf if rt_path == 'two_stream' else 10.0, itop, L)
        planck = orc.blackbody_wn_2D(m['wn'], m['temps'][w])
    if scale is not None:
        depth = depth * scale
    return cb.band_contribution_host(depth, ideep, responses, m['wn'], indices, rt_path=rt_path,
                                     pressure=m['press'], planck=planck)


@pytest.mark.parametrize('rt_path', ['transit', 'emission', 'two_stream'])
def test_eval_bands_contribution(eng, orc, rt_path):
    """9 walkers with their own radius profiles in chunks of 4 (the seams), on a model WITH a
    column order: the plan ignores it.  Against the oracle chain; the band fluxes and spectra_out
    keep the bits of a call without contribution_out; band_contribution() after eval() is row 0
    of a batch with the model's own radius."""
    import torch
    m = table_model(eng, rt_path)
    nw, L, W, pb = m['nw'], m['nlayers'], m['nwave'], m['pb']
    order = np.random.default_rng(3).permutation(W)
    model = make_model(eng, m, rt_path, order)
    kw = dict(radius=m['rd'], chunk=CHUNK)
    plain_spectra = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
    plain = model.eval_bands(m['td'], m['dd'], pb, spectra_out=plain_spectra, **kw).clone()
    if rt_path != 'two_stream':
        assert model.column_order is not None
    spectra = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
    cf = torch.full((nw, L, pb.nbands), float('nan'), dtype=torch.float64, device='cuda')
    flux = model.eval_bands(m['td'], m['dd'], pb, spectra_out=spectra, contribution_out=cf,
                            contribution_pressure=m['press'], **kw)
    assert torch.equal(flux, plain) and torch.equal(spectra, plain_spectra)
    got = host(cf)
    single = np.array([len(b[1]) == 1 for b in m['bands']])
    rng = np.random.default_rng(8)
    for w in range(nw):
        want = oracle_contribution(orc, m, rt_path, w)
        moved = oracle_contribution(orc, m, rt_path, w,
                                    scale=1 + 1e-11 * rng.uniform(-1, 1, (L, W)))
        bound = max(10 * float(np.max(np.abs(moved - want)[:, ~single])), 1e-13)
        assert np.array_equal(np.isnan(got[w]), np.isnan(want)), w
        assert np.all(np.isnan(want[:, single])) and np.all(np.isfinite(want[:, ~single]))
        err = float(np.max(np.abs(got[w] - want)[:, ~single]))
        print(f'{rt_path} walker {w}: max abs error {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (w, err, bound)
        assert np.all(np.max(got[w][:, ~single], axis=0) == 1.0)
    # a second run, and a device tensor as the pressure: the same bits
    cf2 = torch.empty_like(cf)
    model.eval_bands(m['td'], m['dd'], pb, contribution_out=cf2,
                     contribution_pressure=eng.dev(m['press']), **kw)
    assert torch.equal(torch.isnan(cf), torch.isnan(cf2))
    assert torch.equal(torch.nan_to_num(cf, nan=-7.0), torch.nan_to_num(cf2, nan=-7.0))
    # band_contribution() of the last eval(): row 0 of a batch with the shared radius
    shared = torch.empty_like(cf)
    model.eval_bands(m['td'], m['dd'], pb, chunk=CHUNK, contribution_out=shared,
                     contribution_pressure=m['press'])
    model.eval(m['temps'][0], m['dd'][0])
    one = model.band_contribution(pb, pressure=m['press'])
    assert one.shape == (L, pb.nbands)
    assert torch.equal(torch.isnan(one), torch.isnan(shared[0]))
    assert torch.equal(torch.nan_to_num(one, nan=-7.0), torch.nan_to_num(shared[0], nan=-7.0))


@pytest.mark.parametrize('rt_path', ['transit', 'emission', 'two_stream'])
def test_eval_bands_contribution_poisoned(eng, rt_path, monkeypatch):
    """Every fresh buffer of the call is NaN (floats) or a large negative number (integers): the
    same contribution functions and band fluxes, bit for bit."""
    import torch
    m = table_model(eng, rt_path)
    pb = m['pb']
    model = make_model(eng, m, rt_path, None)
    kw = dict(radius=m['rd'], chunk=CHUNK, contribution_pressure=m['press'])
    cf = torch.zeros((m['nw'], m['nlayers'], pb.nbands), dtype=torch.float64, device='cuda')
    flux = model.eval_bands(m['td'], m['dd'], pb, contribution_out=cf, **kw).clone()
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.numel() and t.is_floating_point():
            t.fill_(float('nan'))
        elif t.numel() and t.dtype in (torch.int32, torch.int64):
            t.fill_(torch.iinfo(t.dtype).min // 2)
        return t
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: fill(real_empty_like(*a, **k)))
    cf2 = torch.empty_like(cf)
    flux2 = model.eval_bands(m['td'], m['dd'], pb, contribution_out=cf2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(flux, flux2)
    assert torch.equal(torch.isnan(cf), torch.isnan(cf2))
    assert torch.equal(torch.nan_to_num(cf, nan=-7.0), torch.nan_to_num(cf2, nan=-7.0))


def test_refusals_before_any_launch(eng, monkeypatch):
    """HiresData, cloudy calls, a missing pressure, a wrong shape, dtype or device of
    contribution_out: ValueError, and no entry of the library has been called."""
    import torch
    from pyratbay_amd import batch, table
    m = table_model(eng, 'emission')
    pb, nw, L = m['pb'], m['nw'], m['nlayers']
    model = make_model(eng, m, 'emission', None)
    tmodel = make_model(eng, table_model(eng, 'transit'), 'transit', None)
    cf = torch.zeros((nw, L, pb.nbands), dtype=torch.float64, device='cuda')
    hires = eng.HiresData(m['wn'], m['wn'][50:60] + 0.01, 30000.0)
    hcf = torch.zeros((nw, L, hires.nbands), dtype=torch.float64, device='cuda')

    def no_launch(name, *a):
        raise AssertionError(f'{name} was called')
    for mod in (batch, table):
        monkeypatch.setattr(mod, 'call', no_launch)
    args = (m['td'], m['dd'], pb)
    with pytest.raises(ValueError, match='PassBands'):
        model.eval_bands(m['td'], m['dd'], hires, contribution_out=hcf,
                         contribution_pressure=m['press'])
    with pytest.raises(ValueError, match='contribution_pressure'):
        model.eval_bands(*args, contribution_out=cf)
    with pytest.raises(ValueError, match='contribution_pressure'):
        model.eval_bands(*args, contribution_out=cf, contribution_pressure=m['press'][:-1])
    with pytest.raises(ValueError, match='without contribution_out'):
        model.eval_bands(*args, contribution_pressure=m['press'])
    for bad in (cf[:, :-1], cf[:-1], cf.float(), cf.cpu(), cf.transpose(1, 2),
                torch.zeros((nw, pb.nbands, L), dtype=torch.float64,
                            device='cuda').transpose(1, 2)):
        with pytest.raises(ValueError, match='contribution_out'):
            model.eval_bands(*args, contribution_out=bad, contribution_pressure=m['press'])
    tm = table_model(eng, 'transit')
    tcf = torch.zeros((tm['nw'], tm['nlayers'], tm['pb'].nbands), dtype=torch.float64,
                      device='cuda')
    with pytest.raises(ValueError, match='clouds'):
        tmodel.eval_bands(tm['td'], tm['dd'], tm['pb'], contribution_out=tcf,
                          f_patchy=eng.dev(np.full(tm['nw'], 0.5)))
    with pytest.raises(ValueError, match='eval\\(\\) first'):
        make_model(eng, m, 'emission', None).band_contribution(pb, pressure=m['press'])
    with pytest.raises(ValueError, match='PassBands'):
        model.band_contribution(hires, pressure=m['press'])
