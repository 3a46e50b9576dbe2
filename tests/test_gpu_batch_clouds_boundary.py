"""The cloud walker batch at the kernel boundary (pb_clouds.hip): all eight instantiations of the
two column kernels, the deck state and the cloud plan, on dirty memory, against the oracle chain
cases.oracle_patchy (optical_depth_transit -> transmission_deck; plane_parallel_optical_depth ->
emission_deck with the deck's temperature in row deck_itop for both columns; f cloudy +
(1 - f) clear in NumPy) at rtol 1e-11, the figure test_gpu_batch_clouds.py uses for this chain.

Which test launches which instantiation:

  k_cloudy_transit<16, false>   test_transit_shapes_and_row_widths, nr = 0, nrow = L - itop
                                <= 384 ((1, 0, 1) ... (384, 0, 130)); test_special_values_transit
                                (ec = +inf); test_special_values_patchy_fraction
  k_cloudy_transit<16, true>    the same shapes with nr = 1, 2; test_special_values_transit
                                (infinite cloud factor); test_ordered_columns;
                                test_cloud_plan_edges_eight_terms
  k_cloudy_transit<8, false>    test_transit_shapes_and_row_widths, nr = 0 at (385, 0, 130),
                                (400, 15, 130), (1024, 0, 64: 65536 B of LDS)
  k_cloudy_transit<8, true>     the same three shapes with nr = 1, 2
  k_cloudy_emission<8, false>   test_emission_quadrature_width_and_shapes, nmu = 1, 5, 8, nr = 0
  k_cloudy_emission<8, true>    the same with nr = 2; test_special_values_emission;
                                test_ordered_columns; test_special_values_patchy_fraction;
                                test_cloud_plan_edges_eight_terms (nmu = 5)
  k_cloudy_emission<16, false>  test_emission_quadrature_width_and_shapes, nmu = 9, 16, nr = 0;
                                test_emission_sixteen_sums_equal_eight (ninth weight 0)
  k_cloudy_emission<16, true>   the same with nr = 2; test_cloud_plan_edges_eight_terms (nmu = 9)

Every tensor the engine allocates for a kernel's output starts as NaN (dirty_outputs: float
tensors NaN, the deck's int32 itop a sentinel), so a slot no thread writes shows.  The cases come
from cases.cloud_case; that they are the situations named here (crossings in three row blocks, a
column that never crosses, decks on both sides of a row-block boundary, all / some / none
regimes, ...) is asserted on the oracle alone in test_batch_clouds_cases_cpu.py.  Every check
prints its worst relative deviation before it asserts.

The transit kernels stage the ray path as [segment][row] with zeros where segment >= row and run
one predicate-free fma over the rows of a block: an infinite ec (or ec + ec_cloud) in a layer of
the block met those zeros in the rows above it, 0 * inf = NaN, where the reference never touches
that layer.  test_special_values_transit found exactly that; the kernels now clamp the sum of a
segment's two layers to the largest finite double (the bits of every finite input are kept, the
rows that do include the layer still get exp(-huge) = 0)."""
import contextlib

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

RTOL = 1e-11
MAXDEPTH = cases.CLOUD_MAXDEPTH
SENTINEL = -77777


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def uploader(eng):
    """engine.dev on a copy (the cases' arrays are read-only, which torch.from_numpy warns about)."""
    return lambda a, *args: eng.dev(np.array(a), *args)


@contextlib.contextmanager
def dirty_outputs():
    """The engine's wrappers allocate their outputs with torch.empty / torch.empty_like; inside
    this block such a tensor starts as NaN (float) or SENTINEL (integer) instead of whatever the
    allocator's block held -- which may well be the right answer of the previous call."""
    import torch
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float('nan') if t.is_floating_point() else SENTINEL)
    torch.empty = lambda *a, **kw: fill(empty(*a, **kw))
    torch.empty_like = lambda *a, **kw: fill(empty_like(*a, **kw))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def run(eng, c, maxdepth, deck=True, f=True, parts=True, quad=None, column=None):
    """cloudy_transit_batch / cloudy_emission_batch on a case of cases.cloud_case, outputs dirty.
    f: True (the case's fractions), None, or an array.  -> host arrays (spectrum, clear, cloudy)
    or spectrum."""
    import torch
    dev = uploader(eng)
    kw = dict(want_parts=parts, column=column)
    if deck:
        kw['deck'] = (dev(c['deck_itop'], torch.int32), dev(c['rsurf']), dev(c['tsurf']))
    if f is not None:
        kw['f_patchy'] = dev(c['fpatchy'] if f is True else np.asarray(f, float))
    if c['cs'] is not None:
        kw.update(cloud_cs=dev(c['cs']), cloud_f=dev(c['cf']))
    ec, radius = dev(c['ec']), dev(c['radius'])
    with dirty_outputs():
        if c['geom'] == 'transit':
            path = eng.transit_path_device(radius, c['itop'])
            out = eng.cloudy_transit_batch(ec, path, radius, c['rstar'], c['itop'], maxdepth, **kw)
        else:
            mu, weights = quad
            out = eng.cloudy_emission_batch(ec, dev(-np.diff(c['radius'], axis=1)), dev(c['wn']),
                                            dev(c['temps']), dev(np.asarray(mu, float)),
                                            dev(np.asarray(weights, float)), c['itop'], maxdepth,
                                            **kw)
    return tuple(host(t) for t in out) if parts else host(out)


def rel_dev(got, want):
    """Worst |got / want - 1| (0 where both are equal, e.g. both zero or the same infinity; inf
    where one side is not finite and the other differs)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    with np.errstate(all='ignore'):
        d = np.abs(got - want) / np.abs(want)
    d[(got == want) | (np.isnan(got) & np.isnan(want))] = 0.0
    d[np.isnan(d)] = np.inf
    return float(d.max()) if d.size else 0.0


class Worst:
    """The worst deviation of a test, printed before the assertion that uses it."""

    def __init__(self, what):
        self.what, self.value, self.where = what, 0.0, None

    def add(self, got, want, where):
        d = rel_dev(got, want)
        if self.where is None or d > self.value:
            self.value, self.where = d, where
        return d

    def check(self, rtol=RTOL):
        print(f'{self.what}: worst relative deviation {self.value:.3e} at {self.where}')
        assert self.value <= rtol, (self.what, self.value, self.where)


def mixed(c, oracle, fvals=None):
    """(spectrum, clear, cloudy)[nw, W] of the oracle; fvals None: the cloudy column alone."""
    clear = np.array([oracle[w][0] for w in range(c['nw'])])
    cloudy = np.array([oracle[w][1] for w in range(c['nw'])])
    if fvals is None:
        return cloudy, clear, cloudy
    f = np.clip(np.asarray(fvals, float), 0, 1)[:, None]
    with np.errstate(invalid='ignore'):
        return f * cloudy + (1 - f) * clear, clear, cloudy


# ---------------------------------------------------------------------------------------------
# 1. transit: shapes x row widths x cloud terms x deck x patchy x maxdepth
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nr', [0, 1, 2])
@pytest.mark.parametrize('L,itop,W', cases.CLOUD_TRANSIT_SHAPES)
def test_transit_shapes_and_row_widths(eng, orc, L, itop, W, nr):
    """k_cloudy_transit<16 | 8, nr > 0> at every shape of cases.CLOUD_TRANSIT_SHAPES: one layer;
    one impact parameter and no ray path; a second row block of one row; the last shape of <16>
    (384 rows) and the first of <8> (385), <8> through itop, 1024 rows in 64 KiB of LDS.  Crossed
    with the deck given / absent, f_patchy given (want_parts) / absent (want_parts = False: the
    need_clear = false path, and once with the parts), maxdepth 0 / CLOUD_MAXDEPTH / inf.  At
    L <= 80 also against the single-spectrum path, walker by walker, at the same tolerance."""
    c = cases.cloud_case(orc, 'transit', L, itop, W, nr)
    dev = uploader(eng)
    worst, single = Worst(f'transit {(L, itop, W)} nr={nr}'), Worst('  vs single-spectrum path')
    for maxdepth in (0.0, MAXDEPTH, np.inf):
        for deck in (False, True):
            oracle = cases.cloud_oracle(orc, c, maxdepth, deck)
            tag = f'maxdepth={maxdepth} deck={deck}'
            got = run(eng, c, maxdepth, deck, True, True)
            for g, want, name in zip(got, mixed(c, oracle, c['fpatchy']),
                                     ('spectrum', 'clear', 'cloudy')):
                assert np.all(np.isfinite(g)), (tag, name)
                worst.add(g, want, f'{tag} patchy {name}')
            alone = run(eng, c, maxdepth, deck, None, False)
            assert np.all(np.isfinite(alone)), tag
            worst.add(alone, mixed(c, oracle)[0], f'{tag} cloudy alone')
            if maxdepth == MAXDEPTH:
                parts = run(eng, c, maxdepth, deck, None, True)
                for g, want in zip(parts, mixed(c, oracle)):
                    worst.add(g, want, f'{tag} parts without f_patchy')
            if L > 80:
                continue
            for w in range(c['nw']):
                cloud = cases.cloud_ec(c, w)
                cloud = np.zeros((L, W)) if cloud is None else cloud
                path = dev(eng.pack_raypath(eng.transit_path(c['radius'][w], itop), itop))
                one = eng.patchy_transit_spectrum(
                    dev(c['ec'][w]), dev(cloud), float(c['fpatchy'][w]), path,
                    dev(c['radius'][w]), c['rstar'], itop, maxdepth,
                    float(c['rsurf'][w]) if deck else None,
                    int(c['deck_itop'][w]) if deck else None)
                for g, want in zip(got, one):
                    single.add(g[w], host(want), f'{tag} walker {w}')
    worst.check()
    if L <= 80:
        single.check()


def test_transit_refuses_1025_rows(eng):
    """nlayers - itop = 1025 is refused before any launch: the output keeps its NaN."""
    import torch
    from pyratbay_amd import _capi
    nw, L, itop, W = 2, 1030, 5, 3
    nrow = L - itop
    ec = torch.ones((nw, L, W), dtype=torch.float64, device='cuda')
    radius = eng.dev(np.linspace(8e9, 7e9, L))
    path = torch.zeros((nrow * (nrow - 1)) // 2, dtype=torch.float64, device='cuda')
    out = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
    with pytest.raises(_capi.PbError, match='at most 1024 impact parameters'):
        eng.cloudy_transit_batch(ec, path, radius, 8.8e10, itop, MAXDEPTH, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # one row fewer runs
    got = eng.cloudy_transit_batch(ec, path[:(1024 * 1023) // 2], radius, 8.8e10, itop + 1,
                                   MAXDEPTH, out=out)
    assert bool(torch.isfinite(got).all())


# ---------------------------------------------------------------------------------------------
# 2. emission: quadrature widths x shapes x cloud terms x deck x patchy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nmu', cases.CLOUD_NMU)
@pytest.mark.parametrize('L,itop,W', cases.CLOUD_EMISSION_SHAPES)
def test_emission_quadrature_width_and_shapes(eng, orc, L, itop, W, nmu):
    """k_cloudy_emission<8> (nmu = 1, 5, 8) and <16> (9, 16) with nr = 0 and 2, the deck given
    (a deck at and above itop radiates unattenuated) / absent, f_patchy given / absent."""
    mu, weights = eng.gauss_quadrature(nmu)
    assert len(mu) == nmu
    worst = Worst(f'emission {(L, itop, W)} nmu={nmu}')
    for nr in (0, 2):
        c = cases.cloud_case(orc, 'emission', L, itop, W, nr)
        for deck in (False, True):
            oracle = cases.cloud_oracle(orc, c, MAXDEPTH, deck, mu, weights)
            tag = f'nr={nr} deck={deck}'
            got = run(eng, c, MAXDEPTH, deck, True, True, (mu, weights))
            for g, want, name in zip(got, mixed(c, oracle, c['fpatchy']),
                                     ('spectrum', 'clear', 'cloudy')):
                assert np.all(np.isfinite(g)), (tag, name)
                worst.add(g, want, f'{tag} patchy {name}')
            alone = run(eng, c, MAXDEPTH, deck, None, False, (mu, weights))
            assert np.all(np.isfinite(alone)), tag
            worst.add(alone, mixed(c, oracle)[0], f'{tag} cloudy alone')
    worst.check()


def test_emission_refuses_17_angles(eng, orc):
    import torch
    from pyratbay_amd import _capi
    c = cases.cloud_case(orc, 'emission', 17, 0, 257, 0)
    dev = uploader(eng)
    out = torch.full((c['nw'], c['W']), float('nan'), dtype=torch.float64, device='cuda')
    mu = np.linspace(0.05, 1.0, 17)
    with pytest.raises(_capi.PbError, match='nmu must be 1..16'):
        eng.cloudy_emission_batch(dev(c['ec']), dev(-np.diff(c['radius'], axis=1)), dev(c['wn']),
                                  dev(c['temps']), dev(mu), dev(np.ones(17)), 0, MAXDEPTH, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize('nr', [0, 2])
def test_emission_sixteen_sums_equal_eight(eng, orc, nr):
    """<16> tied to <8> bit for bit: nine nodes of which the ninth has weight 0 give the bits of
    the eight (the ninth term adds val * 0 = +0; val is finite, test_batch_clouds_cases_cpu.py)."""
    c = cases.cloud_case(orc, 'emission', 51, 3, 402, nr)
    mu8, w8 = eng.gauss_quadrature(8)
    quad9 = cases.cloud_quadrature9(mu8, w8)
    for deck in (False, True):
        eight = run(eng, c, MAXDEPTH, deck, True, True, (mu8, w8))
        nine = run(eng, c, MAXDEPTH, deck, True, True, quad9)
        for a, b, name in zip(eight, nine, ('spectrum', 'clear', 'cloudy')):
            assert np.all(np.isfinite(a)), name
            assert np.array_equal(a, b), (deck, name, rel_dev(b, a))


# ---------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------
def check_special(eng, orc, base, c, maxdepth, quad, what):
    """The special walker against the oracle (NaN where the oracle has NaN, nowhere else); every
    other walker with the bits of the batch without the special walker."""
    w = cases.CLOUD_SPECIAL_WALKER
    mu, weights = quad if quad else (None, None)
    worst = Worst(what)
    for deck in (True,) if 'tsurf' in what else (False, True):
        plain = run(eng, base, maxdepth, deck, True, True, quad)
        got = run(eng, c, maxdepth, deck, True, True, quad)
        oracle = cases.cloud_oracle(orc, c, maxdepth, deck, mu, weights)
        for g, p, want, name in zip(got, plain, mixed(c, oracle, c['fpatchy']),
                                    ('spectrum', 'clear', 'cloudy')):
            keep = [v for v in range(c['nw']) if v != w]
            assert np.array_equal(g[keep], p[keep]), (deck, name)
            assert np.all(np.isfinite(p)), (deck, name)
            assert np.array_equal(np.isnan(g[w]), np.isnan(want[w])), \
                (deck, name, int(np.isnan(g[w]).sum()), int(np.isnan(want[w]).sum()))
            worst.add(g[w], want[w], f'deck={deck} {name}')
    worst.check()


@pytest.mark.parametrize('name,maxdepth', cases.CLOUD_SPECIAL_EMISSION)
def test_special_values_emission(eng, orc, name, maxdepth):
    """A layer with ec = +inf; depths above 1e5 (clamp_depth); a layer at T = 0; a deck with
    tsurf = 0 and one with tsurf = NaN (sane_divisor): the oracle's values, and the neighbours
    undisturbed."""
    base, c = cases.cloud_special_case(orc, 'emission', name)
    check_special(eng, orc, base, c, maxdepth, eng.default_quadrature(), f'emission {name}')


@pytest.mark.parametrize('maxdepth', [MAXDEPTH, np.inf])
@pytest.mark.parametrize('name,nr', cases.CLOUD_SPECIAL_TRANSIT)
def test_special_values_transit(eng, orc, name, nr, maxdepth):
    """ec = +inf in one layer in the middle of a row block (nr = 0) and one infinite cloud factor
    (nr = 1): the rows above that layer never include it and stay finite, as in the oracle."""
    base, c = cases.cloud_special_case(orc, 'transit', name)
    check_special(eng, orc, base, c, maxdepth, None, f'transit {name} maxdepth={maxdepth}')


@pytest.mark.parametrize('geom', ['transit', 'emission'])
def test_special_values_patchy_fraction(eng, orc, geom):
    """f_patchy = -0.5, 0, 0.3, 1, 1.5 and NaN in one batch: -0.5 gives the bits of 0, 1.5 the bits
    of 1, NaN gives NaN in that walker's spectrum only (its clear and cloudy stay finite)."""
    L, itop, W = cases.CLOUD_SPECIAL_SHAPE
    c = cases.cloud_case(orc, geom, L, itop, W, 0 if geom == 'transit' else 2)
    quad = None if geom == 'transit' else eng.default_quadrature()
    f = np.array([-0.5, 0.0, 0.3, 1.0, 1.5, np.nan])
    got = run(eng, c, MAXDEPTH, True, f, True, quad)
    clamped = run(eng, c, MAXDEPTH, True, np.array([0.0, 0.0, 0.3, 1.0, 1.0, np.nan]), True, quad)
    for a, b in zip(got, clamped):
        assert np.array_equal(a, b, equal_nan=True)
    spectrum, clear, cloudy = got
    assert np.all(np.isnan(spectrum[5])) and np.all(np.isfinite(spectrum[:5]))
    assert np.all(np.isfinite(clear)) and np.all(np.isfinite(cloudy))
    mu, weights = quad if quad else (None, None)
    oracle = cases.cloud_oracle(orc, c, MAXDEPTH, True, mu, weights)
    worst = Worst(f'{geom} f_patchy values')
    for g, want, name in zip(got, mixed(c, oracle, f), ('spectrum', 'clear', 'cloudy')):
        worst.add(g[:5], want[:5], name)
    worst.check()


# ---------------------------------------------------------------------------------------------
# 4. ordered columns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', ['transit', 'emission'])
def test_ordered_columns(eng, orc, geom):
    """ec (and the cloud rows, and wn) in a permuted column order with `column` naming the grid
    index of each: the grid-order run's bits.  Five entries outside the grid (-1, W, W + 1000)
    drop those columns alone: their slots keep the NaN the outputs started with."""
    import torch
    L, itop, W, nr = 33, 2, 700, 2
    c = cases.cloud_case(orc, geom, L, itop, W, nr)
    quad = None if geom == 'transit' else eng.default_quadrature()
    grid = run(eng, c, MAXDEPTH, True, True, True, quad)
    assert all(np.all(np.isfinite(g)) for g in grid)
    rng = np.random.default_rng(8)
    perm = rng.permutation(W)
    p = cases.cloud_modified(c, ec=np.ascontiguousarray(c['ec'][:, :, perm]),
                             cs=np.ascontiguousarray(c['cs'][..., perm]), wn=c['wn'][perm])
    got = run(eng, p, MAXDEPTH, True, True, True, quad, column=eng.dev(perm, torch.int32))
    for a, b in zip(got, grid):
        assert np.array_equal(a, b)
    dropped = {3: -1, 255: W, 256: W + 1000, 511: -1, W - 1: W}    # position in the order -> entry
    bad = perm.copy()
    for j, entry in dropped.items():
        bad[j] = entry
    got = run(eng, p, MAXDEPTH, True, True, True, quad, column=eng.dev(bad, torch.int32))
    lost = perm[list(dropped)]
    kept = np.setdiff1d(np.arange(W), lost)
    for a, b, name in zip(got, grid, ('spectrum', 'clear', 'cloudy')):
        assert np.array_equal(a[:, kept], b[:, kept]), name
        assert np.all(np.isnan(a[:, lost])), name


# ---------------------------------------------------------------------------------------------
# 5. deck state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared_radius', [True, False])
@pytest.mark.parametrize('L,shift', [(1, 0), (2, 0), (51, 0), (51, 1), (51, -1)])
def test_deck_state_edges(eng, L, shift, shared_radius):
    """deck_state_batch against its NumPy mirror continuum.deck_state: integers equal, floats bit
    for bit (both state np.interp's arithmetic).  The pressure nodes are powers of ten, so that
    10**logp lands exactly on a node, on the device as on the host; logp on a node, one ulp below
    and above it, on the first and the last node, beyond each end, +-inf and NaN (itop = L - 1,
    rsurf = tsurf = NaN); 257 walkers: a second block of k_deck_state.

    One ulp off the node, bit for bit: shift = +-1 moves the NODE one ulp up / down, so that the
    deck's pressure 10**4 (exact on both sides) lies one ulp below / above it.  For logp itself one
    ulp off 4.0 the device's pow(10, logp) is not libm's: 10**nextafter(4, inf) is 1e4 + 11 ulp on
    the host (correctly rounded) and one ulp away from that on the device, tsurf then differs by
    up to 9.4e-16 (measured).  The layer index must still be equal there; rsurf and tsurf are held to
    1e-13, the figure of test_gpu_batch_clouds.py for this comparison, and to the bits everywhere
    else."""
    from pyratbay_amd import continuum as ct
    nw = 257
    rng = np.random.default_rng(L)
    top = {1: 0, 2: 2, 51: 10}[L]
    pressure = np.logspace(0, top, L)
    assert pressure[0] == 1.0 and pressure[-1] == 10.0**top
    node = 4.0 if L == 51 else 0.0
    k = int(np.flatnonzero(pressure == 10.0**node)[0])
    if shift:
        pressure[k] = np.nextafter(pressure[k], shift * np.inf)
    vals = [node, np.nextafter(node, -np.inf), np.nextafter(node, np.inf), 0.0, float(top),
            -1.0, -300.0, top + 1.0, 300.0, -np.inf, np.inf, np.nan]
    logp = np.resize(np.array(vals), nw)            # (every walker its own radius and temperatures)
    pow_differs = np.zeros(nw, bool)
    if node != 0.0:
        pow_differs = (np.arange(nw) % len(vals) == 1) | (np.arange(nw) % len(vals) == 2)
    temps = rng.uniform(500, 2500, (nw, L))
    radius = np.linspace(8e9, 7e9, L)[None] * (1 + 0.02 * rng.uniform(-1, 1, (nw, 1)))
    if shared_radius:
        radius = radius[:1]
    with np.errstate(all='ignore'):
        want = ct.deck_state(pressure, logp, radius, temps)
    if L == 51:
        # the deck on the node, one ulp below it, one ulp above it: the node's layer or the next
        assert np.all(want[0][logp == node] == k + (shift < 0))
        assert np.all(want[0][np.arange(nw) % len(vals) == 1] == k)
        assert np.all(want[0][np.arange(nw) % len(vals) == 2] == k + 1)
    dev = eng.dev
    with dirty_outputs():
        got = eng.deck_state_batch(dev(pressure), dev(logp),
                                   dev(radius[0] if shared_radius else radius), dev(temps))
    itop, rsurf, tsurf = (host(t) for t in got)
    assert np.array_equal(itop, want[0])
    nan = np.isnan(logp)
    assert nan.any() and np.all(itop[nan] == L - 1)
    assert np.all(np.isnan(rsurf[nan])) and np.all(np.isnan(tsurf[nan]))
    assert not np.any(np.isnan(rsurf[~nan])) and not np.any(np.isnan(tsurf[~nan]))
    for g, w_, name in ((rsurf, want[1], 'rsurf'), (tsurf, want[2], 'tsurf')):
        print(f'deck state L={L} shift={shift} {name}: worst relative deviation '
              f'{rel_dev(g[~pow_differs], w_[~pow_differs]):.3e}, where the device\'s pow differs '
              f'{rel_dev(g[pow_differs], w_[pow_differs]):.3e}')
        same = (g == w_) | (np.isnan(g) & np.isnan(w_))
        diff = np.flatnonzero(~same & ~pow_differs)
        assert diff.size == 0, (name, diff[:5], logp[diff[:5]], g[diff[:5]], w_[diff[:5]])
        np.testing.assert_allclose(g[pow_differs], w_[pow_differs], rtol=1e-13)


# ---------------------------------------------------------------------------------------------
# 6. cloud plan
# ---------------------------------------------------------------------------------------------
def plan_host(models, pressure, wn, temps, pars, offsets):
    """The factors f[nw, L, nr] and cross-section rows of the host expressions of continuum.py."""
    from pyratbay_amd import continuum as ct
    nw = temps.shape[0]
    f, rows = np.zeros((nw, len(pressure), len(models))), []
    for w in range(nw):
        for m, (model, off) in enumerate(zip(models, offsets)):
            if isinstance(model, ct.Lecavelier):
                model.calc_cross_section(pars[w, off:off + 2])
            else:
                model.pars[:] = pars[w, off:off + 3]
            cs, fac = model.rank1(pressure, temps[w], None)
            f[w, :, m] = fac
            rows.append(np.array(cs, float))
    return f, np.array(rows).reshape(nw, len(models), len(wn))


@pytest.mark.parametrize('W', [1, 257])
@pytest.mark.parametrize('L', [1, 12])
def test_cloud_plan_edges(eng, L, W):
    """pb_cloud_plan through continuum.CloudOperands: Lecavelier, CCSgray, Lecavelier (k_cloud_rows
    maps blockIdx.z past the gray model); a gray cloud whose p_top and p_bottom are layer
    pressures (powers of ten: both ends inclusive) -- against the host expressions of
    continuum.py at 1e-13 (device pow against libm's, a few ulp)."""
    from pyratbay_amd import continuum as ct
    nw = 5
    rng = np.random.default_rng(10 * L + W)
    wn = np.linspace(2000.0, 9000.0, W) if W > 1 else np.array([3000.0])
    pressure = np.logspace(0, L - 1, L)
    lec1, gray, lec2 = ct.Lecavelier(pressure, wn=wn), ct.CCSgray(pressure, wn), \
        ct.Lecavelier(pressure, wn=wn)
    models = [lec1, gray, lec2]
    cont = ct.Continuum(wn, pressure, models, cloud_models=models)
    offsets = [0, 2, 5]
    assert cont._par_offsets() == offsets
    pars = np.stack([rng.uniform(0, 2, nw), rng.uniform(-6, -2, nw), rng.uniform(0, 2, nw),
                     np.full(nw, 2.0 if L > 1 else 0.0), np.full(nw, 5.0 if L > 1 else 0.0),
                     rng.uniform(-1, 1, nw), rng.uniform(-4, 0, nw)], axis=1)
    temps = rng.uniform(500, 2500, (nw, L))
    ops = cont.cloud_operands()
    assert ops.kinds == [1, 2, 1] and ops.nlec == 2
    with dirty_outputs():
        st, keep = ops.plan(eng.dev(temps), eng.dev(pars))
    f, rows = host(keep[0]), host(keep[1])
    want_f, want_rows = plan_host(models, pressure, wn, temps, pars, offsets)
    # both ends of the gray cloud are inclusive: layers 2 ... 5 (L = 12), the only layer (L = 1)
    inside = want_f[:, :, 1] != 0
    assert np.array_equal(inside, np.tile((pressure >= 10.0**pars[0, 3]) &
                                          (pressure <= 10.0**pars[0, 4]), (nw, 1)))
    assert inside.sum() == nw * (4 if L > 1 else 1)
    assert np.array_equal(f[:, :, 1] != 0, inside)
    print(f'cloud plan L={L} W={W}: worst relative deviation factors {rel_dev(f, want_f):.3e}, '
          f'rows {rel_dev(rows[0], want_rows[:, 0]):.3e} {rel_dev(rows[1], want_rows[:, 2]):.3e}')
    np.testing.assert_allclose(f, want_f, rtol=1e-13)
    np.testing.assert_allclose(rows[0], want_rows[:, 0], rtol=1e-13)
    np.testing.assert_allclose(rows[1], want_rows[:, 2], rtol=1e-13)
    assert st.nr == 3 and st.cs_d[1] is None and st.cs_stride[0] == W


@pytest.mark.parametrize('geom,nmu', [('transit', None), ('emission', 5), ('emission', 9)])
def test_cloud_plan_edges_eight_terms(eng, orc, geom, nmu):
    """nr = 8 = PB_CLOUD_MAX terms in a column kernel: gray (no row: ones) and Lecavelier-like
    terms mixed, rows shared by the walkers and rows per walker, against the oracle; nr = 9 is
    refused."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd.continuum import CloudTermsStruct
    L, itop, W, nr = 33, 2, 300, 8
    base = cases.cloud_case(orc, geom, L, itop, W, 2)
    nw = base['nw']
    rng = np.random.default_rng(88)
    gray = [1, 4, 6]
    shared = [0, 5]
    scale = base['cs'][0, 0] / rng.uniform(0.5, 1.5, W)              # ~ the columns' own scale
    rows = rng.uniform(0.2, 1.0, (nr, nw, W)) * scale
    rows[shared] = rows[shared][:, :1]
    rows[gray] = 1.0
    cf = base['cf'][:, :, :1] * rng.uniform(0.1, 0.5, (nw, 1, nr))
    cf[:, :, gray] *= np.median(scale)
    cf[:, :L // 3, 4] = 0.0
    dev = uploader(eng)
    rows_d, cf_d = dev(rows), dev(cf)
    shared_d = {m: dev(rows[m, 0]) for m in shared}
    st = CloudTermsStruct()
    st.nr = nr
    for m in range(nr):
        if m in gray:
            st.cs_d[m], st.cs_stride[m] = None, 0
        elif m in shared:
            st.cs_d[m], st.cs_stride[m] = shared_d[m].data_ptr(), 0
        else:
            st.cs_d[m], st.cs_stride[m] = rows_d[m].data_ptr(), W
    st.f_d = cf_d.data_ptr()
    c = cases.cloud_modified(base, cs=rows, cf=cf, nr=nr)
    deck = (dev(c['deck_itop'], torch.int32), dev(c['rsurf']), dev(c['tsurf']))
    kw = dict(deck=deck, f_patchy=dev(c['fpatchy']), want_parts=True, _terms=st)
    ec, radius = dev(c['ec']), dev(c['radius'])
    mu = weights = None
    with dirty_outputs():
        if geom == 'transit':
            path = eng.transit_path_device(radius, itop)
            got = eng.cloudy_transit_batch(ec, path, radius, c['rstar'], itop, MAXDEPTH, **kw)
        else:
            mu, weights = eng.gauss_quadrature(nmu)
            args = (ec, dev(-np.diff(c['radius'], axis=1)), dev(c['wn']), dev(c['temps']),
                    dev(mu), dev(weights), itop, MAXDEPTH)
            got = eng.cloudy_emission_batch(*args, **kw)
    oracle = cases.cloud_oracle(orc, c, MAXDEPTH, True, mu, weights)
    worst = Worst(f'{geom} nmu={nmu} with 8 cloud terms')
    for g, want, name in zip(got, mixed(c, oracle, c['fpatchy']), ('spectrum', 'clear', 'cloudy')):
        assert np.all(np.isfinite(host(g))), name
        worst.add(host(g), want, name)
    worst.check()
    # the cloud terms matter: the cloudy column differs from the run without them
    assert rel_dev(host(got[2]), run(eng, cases.cloud_modified(base, cs=None, cf=None),
                                     MAXDEPTH, True, True, True, (mu, weights))[2]) > 1e-3
    st.nr = 9
    with pytest.raises(_capi.PbError, match='0 ... 8 cloud terms'):
        if geom == 'transit':
            eng.cloudy_transit_batch(ec, path, radius, c['rstar'], itop, MAXDEPTH, **kw)
        else:
            eng.cloudy_emission_batch(*args, **kw)
