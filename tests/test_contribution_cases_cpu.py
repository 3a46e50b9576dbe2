"""contribution_cases.py without a GPU: its long double reference is anchored -- it reproduces the
`band` arrays that the real package recorded in fixture G24 (all ten cases, fed ec in emission and
two-stream geometry, depth and ideep in transit geometry) within each case's own
max(10 sens, 1e-14), and contribution.band_contribution_host on the oracle's depth -- and every
case is the situation it is named for, asserted on the reference alone."""
import os

import numpy as np
import pytest

import contribution_cases as cc
from pyratbay_amd import contribution as cb

pytestmark = pytest.mark.skipif(not cc.EXTENDED, reason='np.longdouble is not an extended type')
HERE = os.path.dirname(os.path.abspath(__file__))
G24 = os.path.join(HERE, 'golden', 'g24_contribution.npz')


def g24_names():
    with np.load(G24) as g:
        return [str(c) for c in g['cases']]


def g24_case(g, name):
    """The fixture's case as a case of contribution_cases, from the entry's own inputs."""
    f = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + '_')}
    W = len(f['wn'])
    start, count = g[f'W{W}_band_start'], g[f'W{W}_band_count']
    offset = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    bands = (start, count, g[f'W{W}_response'], offset)
    if str(f['rt']) == 'transit':
        return f, cc.case('transit', f['wn'], bands, int(f['itop']), depth=f['depth'],
                          ideep=f['ideep'])
    L = f['ec'].shape[1]
    return f, cc.case('emission', f['wn'], bands, int(f['itop']), ec=f['ec'],
                      intervals=-np.diff(f['radius'], axis=1), dlogp=np.diff(np.log(f['press'])),
                      temps=f['temps'], maxdepth=float(f['maxdepth']), ibottom=L)


def worst(got, want, bound, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    print(f'{what}: max abs difference {err:.3e}, bound {bound:.3e}')
    assert err <= bound, (what, err, bound)
    return err


@pytest.mark.parametrize('name', g24_names())
def test_reference_reproduces_the_real_package(name):
    """The recorded band[nw, L, nbands] of the reference project within bound(case), the case's
    max(10 sens, 1e-14) with the sens of reference() itself.  The fixture's recorded sens (the same
    rule with another seeded r, on the float64 functions) is printed beside it: the two agree
    within a factor of 4, and the recorded values -- float64 results -- lie 1.5e-13 (ts_l8, a band
    of two samples with a column of total depth 4.7e-4; bound 3.4e-13) and 1.3e-13 (e_md; bound
    8.2e-13) from the long double ones.  Evaluated in float64, the same statements reproduce the
    recorded values to 3e-17 and 1.7e-16: the difference is the rounding of exp(-depth) next to 1
    in the recorded values."""
    with np.load(G24) as g:
        f, c = g24_case(g, name)
    assert np.isnan(f['band']).any()                          # (the band of one sample)
    print(f'{name}: sens {c["sens"]:.3e}, recorded sens {float(f["sens"]):.3e}')
    worst(c['ref'], f['band'], cc.bound(c), name)
    assert np.array_equal(cc.reference(c), c['ref'], equal_nan=True)
    if c['rt'] == 'emission':
        # the depth it formed is the oracle's, the stop included
        depth = cc.emission_depth(c)[0].astype(np.float64)
        assert np.array_equal(depth == 0, f['depth'] == 0)
        assert np.all(np.abs(depth - f['depth']) <= 4 * np.spacing(f['depth']))
        assert np.array_equal(c['stop'], f['ideep'])


def host_form(c, w, depth, ideep):
    responses = [c['response'][o:o + n] for o, n in zip(c['response_offset'], c['band_count'])]
    indices = [np.arange(s, s + n) for s, n in zip(c['band_start'], c['band_count'])]
    if c['rt'] == 'transit':
        return cb.band_contribution_host(depth, ideep, responses, c['wn'], indices)
    from oracle import oracle
    # (diff(log(pressure)) of this pressure is dlogp to a rounding)
    pressure = np.exp(np.concatenate([[0.0], np.cumsum(c['dlogp'])]))
    return cb.band_contribution_host(depth, ideep, responses, c['wn'], indices, rt_path='emission',
                                     pressure=pressure,
                                     planck=oracle.blackbody_wn_2D(c['wn'], c['temps'][w]))


@pytest.mark.parametrize('geometry,L,W,itop,ibottom',
                         [('emission', 9, 70, 0, None), ('emission', 9, 70, 2, 5),
                          ('two_stream', 9, 70, 0, None), ('emission', 257, 600, 2, None)])
def test_reference_against_the_host_form_emission(orc, geometry, L, W, itop, ibottom):
    """band_contribution_host on the oracle's plane-parallel depth (ibottom < L included), for
    in-grid bands."""
    c = cc.shape_case(geometry, L, W, 3, itop, ibottom=ibottom)
    for w in range(c['nw']):
        depth, ideep = np.zeros((L, W)), np.full(W, L - 1, np.int32)
        orc.plane_parallel_optical_depth(depth, ideep, c['ec'][w], c['intervals'][w],
                                         c['maxdepth'], itop, c['ibottom'])
        assert np.array_equal(ideep, c['stop'][w])
        worst(c['ref'][w], host_form(c, w, depth, ideep), cc.bound(c), f'{geometry} walker {w}')


def test_reference_against_the_host_form_transit(orc):
    """band_contribution_host on the oracle's transit depth and ideep."""
    L, W, itop = 9, 70, 2
    e = cc.shape_case('emission', L, W, 3, itop)
    depth, ideep = np.empty((3, L, W)), np.empty((3, W), np.int32)
    for w in range(3):
        radius = cc.RJUP + np.concatenate([np.cumsum(e['intervals'][w][::-1])[::-1], [0.0]])
        depth[w], ideep[w] = orc.optical_depth_transit(0.03 * e['ec'][w], radius, itop, L, 10.0)
    bands = (e['band_start'], e['band_count'], e['response'], e['response_offset'])
    c = cc.case('transit', e['wn'], bands, itop, depth=depth, ideep=ideep)
    assert len(np.unique(ideep)) >= 3
    for w in range(3):
        worst(c['ref'][w], host_form(c, w, depth[w], ideep[w]), cc.bound(c), f'walker {w}')


# ------------------------------------------------------------------------------------- situations
def stops_of(c):
    """-> (layers at which columns stopped on maxdepth, number of columns that never did)."""
    depth, stop, _ = cc.emission_depth(c)
    at_stop = np.take_along_axis(depth, stop[:, None, :], axis=1)[:, 0]
    by_depth = (at_stop >= c['maxdepth']) & (stop != c['ibottom'])
    return set(stop[by_depth].tolist()), int(np.sum(~by_depth))


@pytest.mark.parametrize('L', [255, 256, 257, 513, 1024])
def test_emission_columns_stop_at_several_layers(L):
    for itop in (0, 2):
        c = cc.shape_case('emission', L, 70, 3, itop)
        stops, never = stops_of(c)
        assert len(stops) >= 3 and never >= 1, (L, itop, sorted(stops), never)
        jumps = np.diff(np.exp(-cc.emission_depth(c)[0]), axis=1)
        assert np.sum(jumps > 0.1) >= 1                       # zeroed jumps (kept: e_md's case)
        open_ = cc.shape_case('two_stream', L, 70, 3, itop)
        assert stops_of(open_)[0] == set() and np.all(open_['stop'] == L - 1)


def test_small_maxdepth_keeps_and_zeroes_jumps():
    c = cc.small_maxdepth_case()
    assert c['L'] == 257 and c['maxdepth'] == 0.105
    jumps = np.diff(np.exp(-cc.emission_depth(c)[0]), axis=1)
    kept, zeroed = int(np.sum((jumps > 0) & (jumps <= 0.1))), int(np.sum(jumps > 0.1))
    print(f'{kept} jumps kept, {zeroed} set to 0')
    assert kept >= 5 and zeroed >= 5
    assert len(stops_of(c)[0]) >= 3


def test_ibottom_stops_the_columns():
    L, itop = 12, 2
    free = cc.shape_case('two_stream', L, 70, 3, itop)
    for ibottom in (itop + 1, L // 2, L - 1, L, itop, 0, -3):
        c = cc.shape_case('two_stream', L, 70, 3, itop, ibottom=ibottom)
        assert np.all(c['stop'] == (ibottom if itop < ibottom < L else L - 1)), ibottom
        same = np.array_equal(c['ref'], free['ref'], equal_nan=True)
        assert same == (not itop < ibottom < L - 1), ibottom
    zero = cc.shape_case('emission', L, 70, 3, itop, maxdepth=0.0)
    assert np.all(zero['stop'] == itop + 1)


def test_equality_twin_stops_one_layer_apart():
    a, b = cc.equality_case(False), cc.equality_case(True)
    assert a['exact'] and b['exact'] and a['maxdepth'] == 4.0
    assert b['maxdepth'] == np.nextafter(4.0, np.inf)
    depth = cc.emission_depth(a)[0]
    assert np.all(depth[:, 3] == 4) and np.all(depth[:, 3].astype(np.float64) == a['maxdepth'])
    assert np.all(a['stop'] == 3) and np.all(b['stop'] == 4)
    assert not np.array_equal(a['ref'], b['ref'], equal_nan=True)
    for name in ('ec', 'intervals', 'temps', 'dlogp', 'wn', 'response'):
        assert np.array_equal(a[name], b[name])


@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_clipped_bands_cross_the_ends_of_the_grid(geometry):
    c = cc.clipped_case(geometry)
    W, spans = c['W'], cc.clipped_spans(c['W'])
    retained = {}
    for b, (name, ((start, count), want)) in enumerate(spans.items()):
        assert (c['band_start'][b], c['band_count'][b]) == (start, count)
        g, i = cc.band_samples(c, b)
        assert len(g) == want and np.array_equal(g - start, i), name
        if 'past_end' in name or name == 'at_end_0':
            assert start + count > W and start >= 0
        if 'before_start' in name:
            assert start < 0 and start + count <= W
        retained[name] = want
        nan = np.isnan(c['ref'][:, :, b])
        assert np.all(nan) if want <= 1 else not np.any(nan), name
    assert spans['whole_and_more'][0][0] < 0 and sum(spans['whole_and_more'][0]) > W
    assert sorted(set(retained.values())) == [0, 1, 5, 60, 300, W]
    # across a chunk seam: the retained samples lie in two chunks of the band
    for name in ('seam_past_end', 'seam_before_start'):
        b = list(spans).index(name)
        i = cc.band_samples(c, b)[1]
        assert len(np.unique(i // cc.CHUNK)) >= 2 and c['band_count'][b] == 513
    # a clipped band with >= 2 retained samples = the band of the retained samples, bit for bit
    s, which = cc.sliced_case(c)
    assert len(which) == sum(n >= 2 for n in retained.values())
    assert np.all(s['band_start'] >= 0) and np.all(s['band_start'] + s['band_count'] <= W)
    assert np.array_equal(s['ref'].view(np.int64), c['ref'][:, :, which].view(np.int64))


def test_zero_sum_column_is_nan_in_its_bands_only():
    base = cc.shape_case('emission', 9, 70, 3, 0)
    ec = np.array(base['ec'])
    col = 45
    ec[1, :, col] = 0.0
    c = cc.modified(base, ec=ec)
    holds = np.array([col in cc.band_samples(c, b)[0] for b in range(c['nb'])])
    assert 1 <= holds.sum() < c['nb']
    nan = np.isnan(c['ref'])
    assert np.array_equal(nan[1], np.broadcast_to(holds | nan[0, 0], nan[1].shape))
    assert np.array_equal(nan[0], np.isnan(base['ref'][0]))
    assert np.array_equal(c['ref'][[0, 2]], base['ref'][[0, 2]], equal_nan=True)


@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_limit_cases(geometry):
    for what in ('bands', 'walkers'):
        c = cc.limit_case(geometry, what)
        assert (c['nb'], c['nw']) == ((65535, 1) if what == 'bands' else (1, 65535))
        assert (c['L'], c['W'], c['max_band_count']) == (2, 2, 2)
        assert np.all(np.isfinite(c['ref']))
        if geometry == 'transit':
            assert len(np.unique(c['ref'])) > 60              # (L = 2 in emission: 1 and 0)
        else:
            assert np.all(c['ref'][:, 0] == 1.0) and np.all(c['ref'][:, 1] == 0.0)


def all_cases():
    for g in cc.GEOMETRIES:
        top = cc.MAX_LAYERS['transit' if g == 'transit' else 'emission']
        for L in (2, 3, 255, 256, 257, 513, top):
            for itop in cc.itops(L):
                yield f'{g} L={L} itop={itop}', cc.shape_case(g, L, 70, 3, itop)
        yield f'{g} band counts', cc.shape_case(g, 257, 600, 3, 2)
        yield f'{g} clipped', cc.clipped_case(g)
        for what in ('bands', 'walkers'):
            yield f'{g} limit {what}', cc.limit_case(g, what)
    yield 'small maxdepth', cc.small_maxdepth_case()
    yield 'equality', cc.equality_case(False)
    yield 'equality twin', cc.equality_case(True)


def test_no_case_is_ill_conditioned():
    """sens <= 1e-9 for every case (case() refuses the others); the largest per limit shape."""
    largest = {}
    for name, c in all_cases():
        assert c['sens'] <= 1e-9, name
        key = (c['rt'], c['L']) if c['L'] in (1024, 2048) else None
        if key:
            largest[key] = max(largest.get(key, 0.0), c['sens'])
    for key, sens in largest.items():
        print(f'{key}: largest sens {sens:.2e}')
    assert set(largest) == {('emission', 1024), ('transit', 2048)}
    # depths of 1.1e4: 1e-13 of them is 1e-9 of the transmittance's ratio between two layers
    depth = 1.1e4 + 0.1 * np.arange(3.0)[None, :, None] + np.zeros((50, 3, 2))
    with pytest.raises(ValueError, match='ill-conditioned'):
        cc.case('transit', [2000.0, 2001.0], cc.make_bands([(0, 2)]), 0, depth=depth,
                ideep=np.full((50, 2), 3, np.int32))
