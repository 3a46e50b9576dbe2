"""TableSpectrum.eval_bands does not depend on what memory held.  The limited path writes only
the layers a block of columns can need and leaves the rest of ec as allocated ("read by no one,
or the walker is flagged and repaired", table.TableSpectrum._interpolate): here every torch.empty /
torch.empty_like returns NaN (floats) or a large negative number (integers), models are reused
for batches that need different layers, and chunks run on side streams -- the band fluxes must
have the bits of a fresh grid-order, single-chunk, single-stream evaluation, which is compared
with the oracle chain at 1e-11.  The small model of test_gpu_batch.test_tile_limited_batch:
walker 0 is the base model of the column order, tile_margin = 0, walker 3 is 30 times more
opaque and walker 5 30 times more transparent.  In emission geometry that model is so thin that
every block of columns reaches the last tile (the oracle's stop layers say so): limits that
cover every layer leave nothing unwritten and nothing to overrun, so the emission rows use it
with 100 times the densities, which puts the base model's stop layers where the transit's are."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-11
SHAPES = [(33, 2, 700), (17, 0, 256)]              # (L, itop, W); the second: the smallest with two row tiles
GEOMETRIES = ['emission', 'transit']
OPACITY = {'emission': 100.0, 'transit': 1.0}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


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


_MODELS = {}


def case(eng, L, itop, W, rt_path):
    """cases.limited_table_model with its device tensors (built once per shape and geometry, never
    changed)."""
    key = (L, itop, W, rt_path)
    if key not in _MODELS:
        m = cases.limited_table_model(L, itop, W, opacity=OPACITY[rt_path])
        m['et'], m['td'], m['dd'] = eng.dev(m['etable']), eng.dev(m['temps']), eng.dev(m['dens'])
        m['rd'] = eng.dev(m['radius'])
        m['pb'] = eng.PassBands(m['wn'], m['bands'])
        _MODELS[key] = m
    return _MODELS[key]


def model(eng, m, rt_path, column_order):
    mod = eng.TableSpectrum(m['et'], m['ttable'], m['wn'], m['radius0'], m['rstar'],
                            itop=m['itop'], rt_path=rt_path, column_order=column_order)
    mod.tile_margin = 0
    return mod


_REFERENCE = {}


def reference(eng, m, rt_path, radius=False):
    """Grid order, one chunk, one stream, nothing poisoned: what every other path must reproduce."""
    key = (m['nlayers'], m['nwave'], rt_path, radius)
    if key not in _REFERENCE:
        mod = model(eng, m, rt_path, None)
        _REFERENCE[key] = mod.eval_bands(m['td'], m['dd'], m['pb'], chunk=m['nw'], streams=1,
                                         radius=m['rd'] if radius else None).clone()
        assert mod.column_order is None and mod.tile_limit is None
    return _REFERENCE[key]


def overruns(eng, mod, m, stops):
    """From the oracle's stop layers (grid order) of some walkers: does each of them have a
    column still open beyond the limit of its block?  Both geometries: a transit wavefront
    (32 ordered columns) lies inside one block of 256, so "a wavefront needs a later row tile
    than its block's" is "a column does"."""
    order = mod.column_order.cpu().numpy()
    tile = mod.tile_limit.cpu().numpy()
    klim = cases.limit_layer(tile, m['itop'], m['nwave'])
    return (np.asarray(stops)[:, order] > klim[None]).any(axis=1)


@pytest.mark.parametrize('rt_path', GEOMETRIES)
@pytest.mark.parametrize('L,itop,W', SHAPES)
def test_reference_against_the_oracle(eng, orc, L, itop, W, rt_path):
    """The result the other tests compare with, against the oracle chain (walkers 0, 3 and 5);
    and what the limits of the ordered model mean for these walkers: the base model stays inside
    them by construction, the opaque walker too, and the transparent one runs past them (so the
    limited kernels flag and the gated repair has work to do in every test below)."""
    m = case(eng, L, itop, W, rt_path)
    ref = reference(eng, m, rt_path).cpu().numpy()
    assert np.all(np.isfinite(ref))
    mu, weights = eng.default_quadrature()
    stops = []
    for w in (0, 3, 5):
        want, stop = cases.table_bandflux_oracle(orc, m, rt_path, m['temps'][w], m['dens'][w],
                                                 m['radius0'], mu=mu, weights=weights)
        np.testing.assert_allclose(ref[w], want, rtol=RTOL, err_msg=f'walker {w}')
        stops.append(stop)
    mod = model(eng, m, rt_path, 'auto')
    got = mod.eval_bands(m['td'], m['dd'], m['pb'])
    assert mod.tile_limit is not None and mod.column_order is not None
    assert np.array_equal(got.cpu().numpy(), ref)
    over = overruns(eng, mod, m, stops)
    assert not over[0] and not over[1] and over[2], over


def test_the_poison_works(eng, poison):
    """Under the fixture a limited interpolation with every limit at tile 0 returns NaN in the
    layers it does not write (above itop, beyond itop + 15) and values in those it does; an
    integer allocation comes back negative.  Without this the tests below would prove nothing."""
    import torch
    poison()
    for L, itop, W in SHAPES:
        m = case(eng, L, itop, W, 'transit')
        tile = torch.zeros(-(-W // 256), dtype=torch.int32, device='cuda')
        ec = eng.interp_ec_batch(m['et'], eng.dev(m['ttable']), m['td'], m['dd'], tile_limit=tile,
                                 row0=itop)
        written = torch.zeros(L, dtype=torch.bool, device='cuda')
        written[itop:itop + 16] = True
        assert not bool(written.all())
        assert bool(torch.isnan(ec[:, ~written]).all())
        assert bool(torch.isfinite(ec[:, written]).all())
    assert bool((torch.empty(5, dtype=torch.int32, device='cuda') < -1000000).all())
    assert bool(torch.isnan(torch.empty_like(ec)).all())


@pytest.mark.parametrize('streams', [1, 2])
@pytest.mark.parametrize('chunk', [9, 4])
@pytest.mark.parametrize('column_order', [None, 'auto'])
@pytest.mark.parametrize('rt_path', GEOMETRIES)
@pytest.mark.parametrize('L,itop,W', SHAPES)
def test_poisoned_allocations(eng, poison, L, itop, W, rt_path, column_order, chunk, streams):
    """eval_bands with every fresh buffer poisoned: grid order and the depth order with its
    limits (tile_limit set: the limited kernels and their gated repair ran), one chunk and chunks
    of 4, 4 and 1 walkers, on the caller's stream and on two side streams."""
    import torch
    m = case(eng, L, itop, W, rt_path)
    assert chunk in (m['nw'], 4)
    ref = reference(eng, m, rt_path)
    poison()
    mod = model(eng, m, rt_path, column_order)
    got = mod.eval_bands(m['td'], m['dd'], m['pb'], chunk=chunk, streams=streams)
    torch.cuda.synchronize()
    if column_order == 'auto':
        assert mod.tile_limit is not None
    assert torch.equal(got, ref)


@pytest.mark.parametrize('L,itop,W', SHAPES)
def test_transit_radius_per_walker_on_side_streams(eng, orc, poison, L, itop, W):
    """The transit geometry with a radius profile per walker, chunks of 4 on two side streams,
    poisoned: transit_path_device runs on the side stream of its chunk."""
    import torch
    m = case(eng, L, itop, W, 'transit')
    ref = reference(eng, m, 'transit', radius=True)
    for w in (0, 3, 5):
        want, _ = cases.table_bandflux_oracle(orc, m, 'transit', m['temps'][w], m['dens'][w],
                                              m['radius'][w])
        np.testing.assert_allclose(ref[w].cpu().numpy(), want, rtol=RTOL, err_msg=f'walker {w}')
    assert not torch.equal(ref, reference(eng, m, 'transit'))       # (the radii matter)
    poison()
    mod = model(eng, m, 'transit', 'auto')
    got = mod.eval_bands(m['td'], m['dd'], m['pb'], radius=m['rd'], chunk=4, streams=2)
    torch.cuda.synchronize()
    assert mod.tile_limit is not None
    assert torch.equal(got, ref)


@pytest.mark.parametrize('dirty', ['stale', 'poisoned'])
@pytest.mark.parametrize('chunk,streams', [(9, 1), (4, 2)])
@pytest.mark.parametrize('rt_path', GEOMETRIES)
def test_one_model_several_batches(eng, orc, poison, rt_path, chunk, streams, dirty):
    """One TableSpectrum (depth order of batch A's first walker, its limits without a margin),
    four batches in a row: A near the base model, B with every walker 100 times more transparent
    (each runs past the limits: flagged and repaired -- checked with the oracle's stop layers),
    C 100 times more opaque (fewer do), A again.  Each has the bits a fresh grid-order model
    gives for it, whatever the earlier batches left in the buffers the allocator hands back
    ('stale') and with poisoned ones."""
    import torch
    L, itop, W = SHAPES[0]
    m = case(eng, L, itop, W, rt_path)
    near = np.ones(m['nw'])
    near[3], near[5] = 1 / 30.0, 30.0                    # (undo the two outliers: A is near the base)
    batches = {name: m['dens'] * (near * f)[:, None, None]
               for name, f in (('A', 1.0), ('B', 0.01), ('C', 100.0))}
    want = {}
    for name, dens in batches.items():
        want[name] = model(eng, m, rt_path, None).eval_bands(m['td'], eng.dev(dens), m['pb'],
                                                             chunk=m['nw'], streams=1).clone()
        assert bool(torch.isfinite(want[name]).all())
    assert not torch.equal(want['A'], want['B']) and not torch.equal(want['A'], want['C'])
    if dirty == 'poisoned':
        poison()
    mod = model(eng, m, rt_path, 'auto')
    for name in ('A', 'B', 'C', 'A'):
        got = mod.eval_bands(m['td'], eng.dev(batches[name]), m['pb'], chunk=chunk,
                             streams=streams)
        torch.cuda.synchronize()
        assert torch.equal(got, want[name]), name
    assert mod.tile_limit is not None
    # which batches ran past the limits (the oracle's stop layers against the model's limits)
    mu, weights = eng.default_quadrature()
    nover = {}
    for name, dens in batches.items():
        stops = [cases.table_bandflux_oracle(orc, m, rt_path, m['temps'][w], dens[w], m['radius0'],
                                             mu=mu, weights=weights)[1] for w in range(m['nw'])]
        nover[name] = int(overruns(eng, mod, m, stops).sum())
    assert nover['B'] == m['nw'] and nover['C'] < m['nw'], nover
