"""The cases of test_gpu_batch_clouds_boundary.py (cases.cloud_case, cloud_special_case), checked
on the oracle alone: they are the situations the GPU tests say they run.  The clear crossings of
maxdepth spread over the row blocks of k_cloudy_transit, a column never crosses, the decks sit on
both sides of a row-block boundary and decide all / some / none of a walker's columns, the first
workgroup of transit (80, 0, 600) closes inside the first row block, the ninth quadrature node of
the <16> / <8> bit comparison has a finite intensity, the oracle's transit spectra of the walkers
with an infinite opacity are finite, and the builders are deterministic."""
import numpy as np
import pytest

import cases

MAXDEPTH = cases.CLOUD_MAXDEPTH


def clear_depths(orc, c, w):
    """(depth[L, W], ideep[W]) of the clear column of walker w at MAXDEPTH."""
    L, W = c['ec'].shape[1:]
    if c['geom'] == 'transit':
        return orc.optical_depth_transit(c['ec'][w], c['radius'][w], c['itop'], L, MAXDEPTH)
    depth, ideep = np.zeros((L, W)), np.zeros(W, np.int32)
    orc.plane_parallel_optical_depth(depth, ideep, c['ec'][w], -orc.ediff(c['radius'][w]),
                                     MAXDEPTH, c['itop'], L)
    return depth, np.minimum(ideep, L - 1)


def check_conditions(orc, geom, L, itop, W):
    c = cases.cloud_case(orc, geom, L, itop, W, 0)
    nrow, krows, nw = L - itop, c['krows'], c['nw']
    assert 3 <= nw <= 6
    # every walker has ec, radius, temperatures, deck and fraction of its own
    for key in ('ec', 'radius', 'temps', 'rsurf', 'tsurf', 'fpatchy'):
        flat = c[key].reshape(nw, -1)
        assert len({row.tobytes() for row in flat}) == nw, key
    decks = c['deck_itop']
    assert decks[0] == itop and decks[-1] == L - 1
    if itop > 0:
        assert np.any(decks < itop)
    if nrow > krows + 1:
        assert itop + krows - 1 in decks and itop + krows in decks
        last_block = (nrow - 1) // krows
        assert np.sum((decks - itop) // krows == last_block) >= (2 if nrow % krows != 1 else 1)
    if nrow < 2:
        return
    crossed, ideeps = [], {}
    for w in range(nw):
        depth, ideep = clear_depths(orc, c, w)
        ideeps[w] = ideep
        last = depth[ideep, np.arange(W)]
        crossed.append(last > MAXDEPTH if geom == 'transit' else last >= MAXDEPTH)
    crossed = np.array(crossed)
    # the oracle chain of the GPU tests finds the same stop layers
    quad = ((1.0, 0.5), (1.0, 1.0)) if geom == 'emission' else (None, None)
    same = cases.cloud_oracle(orc, c, MAXDEPTH, False, *quad)
    for w in range(nw):
        got = np.minimum(same[w][2], L - 1)
        assert np.array_equal(got, ideeps[w])
    if W >= 5:
        assert np.any(~crossed.any(axis=0)), 'no column stays below maxdepth in every walker'
    if W >= 64:
        nblocks = -(-nrow // krows)
        blocks = set()
        for w in range(nw):
            blocks |= set(((ideeps[w][crossed[w]] - itop) // krows).tolist())
        assert len(blocks) >= min(3, nblocks), blocks
    if nrow >= 17 and W >= 64:
        assert set(cases.cloud_regimes(ideeps, decks)) == {'all', 'some', 'none'}
    if c['first_group']:
        first = np.array([ideeps[w][:256] for w in range(nw)])
        assert np.all(crossed[:, :256]) and first.max() < itop + krows
        for g0 in range(256, W, 256):
            assert np.any(~crossed[:, g0:g0 + 256].any(axis=0))


@pytest.mark.parametrize('L,itop,W', cases.CLOUD_TRANSIT_SHAPES)
def test_transit_case_conditions(orc, L, itop, W):
    assert cases.cloud_row_block(L - itop) == (16 if L - itop <= 384 else 8)
    check_conditions(orc, 'transit', L, itop, W)
    if (L, itop, W) == (80, 0, 600):
        assert cases.cloud_case(orc, 'transit', L, itop, W, 0)['first_group']


@pytest.mark.parametrize('L,itop,W', cases.CLOUD_EMISSION_SHAPES)
def test_emission_case_conditions(orc, L, itop, W):
    check_conditions(orc, 'emission', L, itop, W)


@pytest.mark.parametrize('nr', [0, 2])
def test_ninth_node_is_finite(orc, nr):
    """The <16> run of the bit comparison adds val * 0 for its ninth node (mu = 0.5): val, the
    oracle's intensity there, is finite in both columns of every walker."""
    c = cases.cloud_case(orc, 'emission', 51, 3, 402, nr)
    mu9, w9 = cases.cloud_quadrature9(np.linspace(0.1, 0.8, 8), np.ones(8))
    assert len(mu9) == 9 and w9[8] == 0.0 and 0 < mu9[8] <= 1
    for use_deck in (False, True):
        res = cases.cloud_oracle(orc, c, MAXDEPTH, use_deck, (mu9[8],), (1.0,))
        for w, (clear, cloudy, _, _) in res.items():
            assert np.all(np.isfinite(clear)) and np.all(np.isfinite(cloudy)), w


@pytest.mark.parametrize('name,nr', cases.CLOUD_SPECIAL_TRANSIT)
def test_transit_infinite_opacity_is_finite_in_the_oracle(orc, name, nr):
    """The reference never touches the infinite layer for the rows above it, and exp(-inf) = 0
    below: clear and cloudy are finite.  The layer lies inside a row block, and columns of the
    walker are still open in the rows of that block above it (where a zero of the staged ray path
    would meet the infinite sum)."""
    base, c = cases.cloud_special_case(orc, 'transit', name)
    w, lay, itop = cases.CLOUD_SPECIAL_WALKER, cases.CLOUD_SPECIAL_LAYER, c['itop']
    assert c['nr'] == nr and 0 < (lay - itop) % c['krows'] < c['krows'] - 1
    assert not np.all(np.isfinite(c['ec'][w])) or not np.all(np.isfinite(c['cf'][w]))
    for use_deck in (False, True):
        for maxdepth in (MAXDEPTH, np.inf):
            clear, cloudy, ideep_c, ideep = cases.cloud_oracle(orc, c, maxdepth, use_deck,
                                                               walkers=[w])[w]
            assert np.all(np.isfinite(clear)) and np.all(np.isfinite(cloudy))
            was = cases.cloud_oracle(orc, base, maxdepth, use_deck, walkers=[w])[w]
            assert np.any(was[2] >= lay)
            if not np.isfinite(maxdepth):
                continue
            if name == 'ec_inf':
                assert np.all(ideep_c <= lay) and np.any(ideep_c == lay)
            if not use_deck:
                assert np.all(ideep <= lay) and np.any(ideep == lay)


@pytest.mark.parametrize('name,maxdepth', cases.CLOUD_SPECIAL_EMISSION)
def test_emission_special_cases(orc, name, maxdepth):
    base, c = cases.cloud_special_case(orc, 'emission', name)
    w, L = cases.CLOUD_SPECIAL_WALKER, c['L']
    assert c['itop'] < c['deck_itop'][w] < L - 1
    if name == 'deep':
        depth, ideep = np.zeros(c['ec'].shape[1:]), np.zeros(c['W'], np.int32)
        orc.plane_parallel_optical_depth(depth, ideep, c['ec'][w], -orc.ediff(c['radius'][w]),
                                         maxdepth, c['itop'], L)
        assert np.all(ideep == L - 1)
        assert np.any((depth[c['itop'] + 1:L - 1] > 1e5) & np.isfinite(depth[c['itop'] + 1:L - 1]))
    mu, weights = np.array([1.0, 0.6, 0.2]), np.array([1.0, 1.0, 1.0])
    clear, cloudy, _, _ = cases.cloud_oracle(orc, c, maxdepth, True, mu, weights, walkers=[w])[w]
    if name == 'tsurf_nan':
        # the deck's row of the Planck array is NaN for both columns: whatever reaches it is NaN
        assert np.any(np.isnan(cloudy)) and not np.all(np.isnan(clear))
    else:
        assert np.all(np.isfinite(clear)) and np.all(np.isfinite(cloudy))


def test_builders_are_deterministic(orc):
    for geom, shape, nr in (('transit', (33, 2, 700), 2), ('transit', (80, 0, 600), 1),
                            ('emission', (51, 3, 402), 2), ('emission', (2, 1, 256), 0)):
        a = cases.cloud_case(orc, geom, *shape, nr)
        b = cases.cloud_case(orc, geom, *shape, nr, cache=False)
        assert a is not b and a.keys() == b.keys()
        for key, v in a.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, b[key]) and not v.flags.writeable, key
            else:
                assert v == b[key], key
        # ec, radius and temperatures do not depend on the number of cloud terms
        other = cases.cloud_case(orc, geom, *shape, 0)
        for key in ('ec', 'radius', 'temps', 'deck_itop', 'rsurf', 'tsurf', 'fpatchy'):
            assert np.array_equal(a[key], other[key]), key
    for name, _ in cases.CLOUD_SPECIAL_TRANSIT:
        a, b = (cases.cloud_special_case(orc, 'transit', name)[1] for _ in range(2))
        assert np.array_equal(a['ec'], b['ec']) and (a['cf'] is None or
                                                     np.array_equal(a['cf'], b['cf']))
