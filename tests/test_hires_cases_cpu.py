"""The cases of hires_cases.py are the situations they are named after (asserted on the brackets
`lo` of hires_cases.reference() alone), and the reference is anchored: it reproduces fixture G21
(the reference project's direct-method convolution, rv_shift and interp1d: a float64 sum, which
carries the rounding the bound covers) within its own bound, and SciPy's mode='same' for T > W.
No GPU."""
import numpy as np
import pytest

import hires_cases as hc

TILE = hc.TILE


def lo_of(c):
    """lo[nw, ndata] in the order of the ascending data."""
    lo = hc.case_reference(c)[4]
    assert np.all(lo >= 0)
    return lo[:, c['slot']]


def test_slots_are_the_four_kinds():
    data = np.sort(np.random.default_rng(1).uniform(0, 1, 50))
    data[10:14] = data[10]
    seen = []
    for kind in ('identity', 'reversed', 'random', 'argsort'):
        slot, caller = hc.slots(kind, data, seed=3)
        assert slot.dtype == np.int32 and np.array_equal(np.sort(slot), np.arange(50))
        assert np.array_equal(caller[slot], data)
        seen.append(slot)
    assert np.array_equal(seen[0], np.arange(50)) and np.array_equal(seen[1], np.arange(50)[::-1])
    assert not np.array_equal(seen[2], seen[3])
    # 'argsort' is HiresData's: the stable argsort of the caller's array
    assert np.array_equal(seen[3], np.argsort(hc.slots('argsort', data, seed=3)[1], kind='stable'))


def test_threshold_is_256_and_257():
    for T in (1, 1025):
        c = hc.layout_case('threshold', T)
        lo = lo_of(c)
        assert hc.tiles(c['W']) == 3
        for w in range(c['nw']):
            assert len(hc.needed_samples(lo[w], 0)) == hc.SPARSE_MAX == 256
            assert len(hc.needed_samples(lo[w], 1)) == 257
            assert len(hc.needed_samples(lo[w], 2)) == 0
        without = hc.layout_case('threshold', T, extra=False)
        lo2 = lo_of(without)
        extra = hc.threshold(c['wn'])[1]
        assert np.array_equal(np.delete(c['data_wn'], extra), without['data_wn'])
        assert np.array_equal(np.delete(lo, extra, axis=1), lo2)
        for w in range(c['nw']):
            # the same needed samples but one, on the other side of the threshold
            assert len(hc.needed_samples(lo2[w], 1)) == 256
            assert np.array_equal(hc.needed_samples(lo2[w], 0), hc.needed_samples(lo[w], 0))
        for name in ('spectra', 'sample_scale', 'taps', 'wn', 'rv'):
            assert np.array_equal(c[name], without[name])


@pytest.mark.parametrize('empty', [0, 1, 2])
def test_one_per_tile_leaves_one_tile_empty(empty):
    c = hc.layout_case('one_per_tile', 1, empty=empty)
    assert hc.tiles(c['W']) == 3 and c['ndata'] == 2
    lo = lo_of(c)
    for w in range(c['nw']):
        per_tile = np.bincount(lo[w] // TILE, minlength=3)
        assert np.array_equal(per_tile, [int(b != empty) for b in range(3)])


@pytest.mark.parametrize('grid_kind', ['resolution', 'step'])
@pytest.mark.parametrize('W', [2, 3, 1023, 1024, 1025, 2047, 2048])
def test_on_every_node_sits_on_the_seams(W, grid_kind):
    wn = hc.grid(grid_kind, W)
    assert len(wn) == W and np.all(np.diff(wn) > 0)
    assert hc.tiles(W) == {2: 1, 3: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 3}[W]
    # one walker: every node and every midpoint, both ends of the grid
    for rv in (0.0, -12.5):
        x = hc.shifted(wn, rv)
        data = hc.on_every_node(wn, rv)
        assert len(data) == 2 * W - 1 and data[0] == x[0] and data[-1] == x[-1]
        lo = hc.reference(np.ones((1, W)), wn, [1.0], data, [rv])[4][0]
        assert np.all(np.isin(x, data))
        for node in hc.seams(W):
            j = np.flatnonzero(data == x[node])
            assert len(j) == 1 and lo[j[0]] == node - 1
        assert np.array_equal(lo, np.maximum(np.arange(2 * W - 1) - 1, 0) // 2)
    # the shape cases: three walkers, each one's seam nodes among the data
    c = hc.shape_case(W, 1, grid_kind)
    assert c['nw'] == 3 and len(set(c['rv'])) == 3 and c['rv'][0] == 0 and \
        c['rv'][1] > 0 > c['rv'][2] and np.all(np.abs(c['rv']) <= c['rv_max'])
    lo = lo_of(c)
    assert c['ndata'] >= 5
    for w in range(3):
        x = hc.shifted(wn, c['rv'][w])
        # (a walker's own end nodes may lie outside another walker's grid: at most those two)
        assert np.sum(np.isin(x, c['data_wn'])) >= W - 2
        for node in hc.seams(W):
            j = np.flatnonzero(c['data_wn'] == x[node])
            assert len(j) == 1 and lo[w, j[0]] == node - 1
        assert len(np.unique(lo[w])) == W - 1            # every bracket has a point


@pytest.mark.parametrize('bracket', [0, TILE])
def test_crowd_is_one_bracket(bracket):
    c = hc.layout_case('crowd', 1, bracket=bracket)
    lo = lo_of(c)
    x = hc.shifted(c['wn'], c['rv'][0])
    d = c['data_wn']
    assert c['ndata'] == 3000 and d[0] == x[bracket] and d[-1] == x[bracket + 1]
    values, counts = np.unique(d, return_counts=True)
    assert counts.max() == 500 and len(values) == 2501
    if bracket == 0:
        assert np.all(lo == 0)
    else:
        # the point on the lower node belongs to the bracket below: the tile below
        assert np.all(lo[:, 1:] == bracket) and np.all(lo[:, 0] == bracket - 1)


def test_single_point():
    c = hc.layout_case('single', 1025)
    assert c['ndata'] == 1 and np.all(lo_of(c) == TILE)


@pytest.mark.parametrize('T', [3, 9, 1025])
def test_unit_tap_is_a_shift(T):
    """A single unit tap at index a: c[i] = s[i + H - a] exactly, zeros beyond the ends."""
    W, H = 700, (T - 1) // 2
    taps = hc.make_taps('unit', T)
    a = int(np.argmax(taps))
    assert a == H // 2 and np.sum(taps != 0) == 1
    s = hc.make_spectra('mixed', 2, W, 5)
    conv, mag = hc.convolve(s, taps)
    want = np.zeros((2, W))
    n = max(W - (H - a), 0)
    want[:, :n] = s[:, H - a:]
    assert np.array_equal(conv, want) and np.array_equal(mag, np.abs(want))


def test_signed_taps_are_signed_and_asymmetric():
    for T in (179, 1025):
        k = hc.make_taps('signed', T)
        assert k.min() < 0 < k.max() and np.max(np.abs(k - k[::-1])) > 0.1 * np.max(np.abs(k))
        g = hc.make_taps('gaussian', T)
        assert g.min() > 0 and abs(g.sum() - 1) < 1e-14


def test_rejection_rule():
    wn = hc.grid('resolution', 50)
    spectra = hc.make_spectra('positive', 7, 50, 1)
    up = np.nextafter(20.0, np.inf)
    rv = np.array([20.0, up, -20.0, -up, np.nan, np.inf, 0.0])
    data = np.linspace(wn[10], wn[40], 9)
    out, bound, _, _, lo = hc.reference(spectra, wn, hc.make_taps('gaussian', 5), data, rv)
    bad = [1, 3, 4, 5]
    assert np.all(np.isposinf(out[bad])) and np.all(bound[bad] == 0) and np.all(lo[bad] == -1)
    assert np.all(np.isfinite(out[[0, 2, 6]])) and np.all(bound[[0, 2, 6]] > 0)
    x = hc.shifted(wn, 3.0)
    for data, ok in ((x[[0, 49]], True), ([np.nextafter(x[0], 0), x[49]], False),
                     ([x[0], np.nextafter(x[49], np.inf)], False)):
        out = hc.reference(spectra[:1], wn, [1.0], np.array(data), [3.0])[0]
        assert bool(np.all(np.isfinite(out))) == ok and (ok or np.all(np.isposinf(out)))


def g21_cases(g):
    for c in range(int(g['ncases'])):
        yield c


def test_reference_reproduces_g21(golden):
    """For every G21 case and rv: depth_convolved, depth_sampled and eclipse_sampled within the
    reference's own bound (the eclipse samples formed as HiresData.set_eclipse forms them: the
    reference project's own expression)."""
    g = golden('g21_hires')
    worst = {'convolved': (0.0, None), 'sampled': (0.0, None)}

    def note(kind, ratio, where):
        if ratio > worst[kind][0]:
            worst[kind] = (ratio, where)

    for c in g21_cases(g):
        wn, taps = g[f'c{c}_wn'], g[f'c{c}_taps']
        scale = 1 / g[f'c{c}_starflux'] * (g['radii'][0] / g['radii'][1])**2
        for r, rv in enumerate(g['rv']):
            data = g[f'c{c}_rv{r}_data_wn']
            for name, spectrum, ss in (('depth', g[f'c{c}_depth'], None),
                                       ('eclipse', g[f'c{c}_fplanet'], scale)):
                out, bound, conv, mag, _ = hc.reference(spectrum[None], wn, taps, data, [rv],
                                                        sample_scale=ss, rv_max=40.0)
                assert np.all(np.isfinite(out)) and np.all(bound > 0)
                ratio, k = hc.deviation(g[f'c{c}_rv{r}_{name}_sampled'][None], out, bound)
                note('sampled', ratio, (c, r, name, k))
                if r == 0:
                    ratio, k = hc.deviation(g[f'c{c}_{name}_convolved'][None], conv,
                                            hc.conv_bound(mag, len(taps)))
                    note('convolved', ratio, (c, name, k))
    for kind, (ratio, where) in worst.items():
        print(f'G21 anchor, {kind}: worst |fixture - ref| / bound = {ratio:.3e} at {where}')
    assert worst['convolved'][0] <= 1 and worst['sampled'][0] <= 1


@pytest.mark.parametrize('W,T', [(5, 9), (700, 1025)])
def test_more_taps_than_samples_is_mode_same(W, T):
    signal = pytest.importorskip('scipy.signal')
    for kind in ('gaussian', 'signed'):
        taps = hc.make_taps(kind, T)
        s = hc.make_spectra('mixed', 1, W, T)
        conv, mag = hc.convolve(s, taps)
        want = signal.convolve(s[0], taps, mode='same', method='direct')
        assert want.shape == (W,) and conv.shape == (1, W)
        ratio, k = hc.deviation(want[None], conv, hc.conv_bound(mag, T))
        print(f'W={W} T={T} {kind}: worst |scipy - ref| / bound = {ratio:.3e} at {k}')
        assert ratio <= 1


@pytest.mark.parametrize('W', [2, 3, 700, 1025])
@pytest.mark.parametrize('T', [1, 5, 179, 1025])
def test_float64_restatement_is_inside_the_bound(W, T):
    """A float64 sum without FMA (two roundings per term: looser than the kernel's chain) and the
    float64 interpolation stay inside the bound, signed inputs included."""
    wn = hc.grid('resolution', W)
    data = hc.on_every_node(wn, hc.RVS)
    H = (T - 1) // 2
    for kind, tk in (('positive', 'gaussian'), ('mixed', 'signed')):
        s = hc.make_spectra(kind, 3, W, W + T)
        taps = hc.make_taps(tk, T)
        out, bound, conv, mag, lo = hc.reference(s, wn, taps, data, hc.RVS)
        padded = np.zeros((3, W + 2 * H))
        padded[:, H:H + W] = s
        c = np.zeros((3, W))
        for t in range(T):
            c += taps[t] * padded[:, 2 * H - t:2 * H - t + W]
        got = np.empty((3, len(data)))
        for w in range(3):
            x = hc.shifted(wn, hc.RVS[w])
            l, h = lo[w], lo[w] + 1
            got[w] = (c[w, h] - c[w, l]) / (x[h] - x[l]) * (data - x[l]) + c[w, l]
        ratio, k = hc.deviation(got, out, bound)
        rc, _ = hc.deviation(c, conv, hc.conv_bound(mag, T))
        print(f'W={W} T={T} {kind}: float64 restatement / bound = {ratio:.3f} (conv {rc:.3f})')
        assert ratio <= 1 and rc <= 1
