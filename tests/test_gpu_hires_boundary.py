"""The high-resolution exit at the kernel boundary (csrc/pb_hires.hip: pb_inst_convolve_batch,
pb_hires_observe_batch), driven through the C ABI on dirty memory, against the long double
reference of hires_cases.py.

Every launch: `out` is NaN before the call and sits between two guard blocks of 3 NaN (the ABI has
no row stride, so the guards follow the last row and precede the first; they must still be NaN
afterwards); the inputs are uploaded from copies and kept alive by name; one synchronize before
the result is read.  Every comparison is |got - ref| <= bound with hires_cases.reference()'s own
derived bound ((T + 8) 2^-53 conv_mag for a sampled value, (T + 2) 2^-53 conv_mag for a convolved
sample; where the bound is 0 the values must be equal, a rejected row +inf exactly), or an
equal-bits statement between two launches.  No tolerance is a literal.  Each check prints its
worst |got - ref| / bound and where, then asserts <= 1.  That the cases are the situations named
here is asserted in test_hires_cases_cpu.py on the reference alone.

Which test launches which situation:

  seam shapes: W = 2, 3 (minimum), 1024, 2047 (end on a seam),   test_observe_shapes (x T = 1, 3,
    1025, 2048 (last tile of 2 nodes), 1023; a data point ON      179, 1025; both grids at 1025 and
    every shifted node 1023 b of every walker                     2048); test_hires_data_on_a_seam
  dense tiles (conv_dense)                                       test_observe_shapes (W >= 1023: a
                                                                  point in every bracket)
  sparse tiles (conv_one)                                        test_observe_shapes W = 2, 3, the
                                                                  2-node last tiles;
                                                                  test_layouts; test_walker_limit
  the 256 / 257 flip, same bits from either path                 test_threshold_flip_has_equal_bits
  T = 1                                                          test_observe_shapes, test_layouts,
                                                                  test_threshold_flip...,
                                                                  test_walker_limit; the second
                                                                  launch of test_fused...
  T = 1025 (halo of 512, largest LDS carve-up)                   test_observe_shapes, test_layouts,
                                                                  test_threshold_flip...,
                                                                  test_fused...,
                                                                  test_convolve_shapes
  T > W (mode='same' with more taps than samples)                test_observe_shapes (W = 2, 3 with
                                                                  T >= 3; every W with T = 1025),
                                                                  test_convolve_shapes
  empty tile (early return), each of three                       test_layouts[one_per_tile-*]
  crowd: 3000 points in one bracket, 500 equal, both nodes       test_layouts[crowd-*] (bracket 0,
                                                                  and 1023 = the 2-node tile)
  ndata = 1                                                      test_layouts[single-*],
                                                                  test_walker_limit
  slots: random / reversed / argsort / identity                  shapes / one_per_tile / threshold,
                                                                  crowd / single
  fused = convolve + unit-tap launch, bit for bit                test_fused_equals_two_launches
  rejection by rv (+-20 exactly, one ulp beyond, NaN, +-inf;     test_rejection_by_rv,
    rv_max = 0 with -0.0)                                         test_rv_max_zero
  rejection by data (the ends exactly, one ulp outside either)   test_rejection_by_data
  NaN and +inf in one walker's spectrum                          test_non_finite_spectrum
  limits: 65535 walkers, 65536 refused; no-ops; refusals         test_walker_limit,
                                                                  test_observe_noops_and_refusals,
                                                                  test_convolve_noops_and_refusals
  convolve tile seams: W = 1, 2, 1023, 1024, 1025, 2049          test_convolve_shapes

Result: every test passed as the kernels stood; no change to pb_hires.hip or HiresData was
needed (the measured ratios are in profiles/hires.md)."""
import numpy as np
import pytest

import hires_cases as hc
from test_gpu_batch_clouds_boundary import dirty_outputs, rel_dev

pytestmark = pytest.mark.gpu

GUARD = 3
OBSERVE, CONVOLVE = 'pb_hires_observe_batch', 'pb_inst_convolve_batch'


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


_REFERENCES = {}


def reference_of(c):
    """hires_cases.case_reference, computed once per case and left unchanged."""
    key = id(c)
    if key not in _REFERENCES:
        ref = hc.case_reference(c)
        for a in ref:
            a.flags.writeable = False
        _REFERENCES[key] = (c, ref)
    return _REFERENCES[key][1]


class Dirty:
    """[nrow, ncol] doubles, NaN, between two guard blocks of GUARD NaN."""

    def __init__(self, nrow, ncol):
        import torch
        self.n = nrow * ncol
        self.store = torch.full((2 * GUARD + self.n,), float('nan'), dtype=torch.float64,
                                device='cuda')
        self.body = self.store[GUARD:GUARD + self.n].view(nrow, ncol)
        self.ptr = self.store.data_ptr() + 8 * GUARD

    def guards_intact(self):
        import torch
        return bool(torch.isnan(self.store[:GUARD]).all()) and \
            bool(torch.isnan(self.store[GUARD + self.n:]).all())

    def untouched(self):
        import torch
        return bool(torch.isnan(self.store).all())


def upload(eng, a, dtype=None):
    """A device tensor from a copy of a host array (None stays None)."""
    import torch
    if a is None:
        return None
    return eng.dev(np.array(a), dtype or torch.float64)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def observe(eng, c, into=None, spectra_d=None, **over):
    """pb_hires_observe_batch on a case -> host [nw, ndata] in the caller's order (or, with the
    Dirty `into` given, nothing: the caller inspects it).  spectra_d: a device tensor instead of
    the case's spectra; over: arguments replaced by name (a pointer by None, a count by another)."""
    import torch
    from pyratbay_amd import _capi
    spectra = upload(eng, c['spectra']) if spectra_d is None else spectra_d
    wn, taps = upload(eng, c['wn']), upload(eng, c['taps'])
    sample_scale, walker_scale = upload(eng, c['sample_scale']), upload(eng, c['walker_scale'])
    data, slot = upload(eng, c['data_wn']), upload(eng, c['slot'], torch.int32)
    rv = upload(eng, c['rv'])
    mine = into is None
    out = Dirty(c['nw'], c['ndata']) if mine else into
    a = dict(out=out.ptr, spectra=ptr(spectra), wn=ptr(wn), taps=ptr(taps),
             sample_scale=ptr(sample_scale), data=ptr(data), slot=ptr(slot), rv=ptr(rv),
             walker_scale=ptr(walker_scale), rv_max=c['rv_max'], ntaps=c['T'], nwave=c['W'],
             ndata=c['ndata'], nwalkers=c['nw'])
    assert set(over) <= set(a)
    a.update(over)
    try:
        rc = _capi.call(OBSERVE, a['out'], a['spectra'], a['wn'], a['taps'], a['sample_scale'],
                        a['data'], a['slot'], a['rv'], a['walker_scale'], a['rv_max'], a['ntaps'],
                        a['nwave'], a['ndata'], a['nwalkers'], stream())
    finally:
        torch.cuda.synchronize()
    assert rc == _capi.PB_OK and out.guards_intact()
    if mine:
        return out.body.cpu().numpy()


def convolve(eng, spectra_h, taps_h, scale_h=None, into=None, **over):
    """pb_inst_convolve_batch on host arrays -> (host [nw, W], the Dirty that holds the device
    result); over: arguments replaced by name (out='spectra': the in-place call)."""
    import torch
    from pyratbay_amd import _capi
    spectra_h = np.array(spectra_h, np.float64, ndmin=2)
    nw, W = spectra_h.shape
    spectra_d, taps_d, scale_d = upload(eng, spectra_h), upload(eng, taps_h), upload(eng, scale_h)
    out = Dirty(nw, W) if into is None else into
    a = dict(out=out.ptr, spectra=ptr(spectra_d), taps=ptr(taps_d), sample_scale=ptr(scale_d),
             ntaps=len(taps_h), nwave=W, nwalkers=nw)
    assert set(over) <= set(a)
    a.update(over)
    if a['out'] == 'spectra':
        a['out'] = a['spectra']
    try:
        rc = _capi.call(CONVOLVE, a['out'], a['spectra'], a['taps'], a['sample_scale'],
                        a['ntaps'], a['nwave'], a['nwalkers'], stream())
    finally:
        torch.cuda.synchronize()
    assert rc == _capi.PB_OK and out.guards_intact()
    return out.body.cpu().numpy(), out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def in_data_order(got, c):
    """Column j belongs to data_wn[j] (ascending)."""
    return got[:, c['slot']]


class Worst:
    """The worst |got - ref| / bound of a test group, printed before the assertion."""

    def __init__(self, what):
        self.what, self.value, self.where = what, 0.0, None

    def add(self, got, ref, bound, where):
        ratio, k = hc.deviation(got, ref, bound)
        if self.where is None or ratio > self.value:
            self.value, self.where = ratio, (where, k)
        return ratio

    def add_case(self, got, c, where, accepted=None):
        """got[nw, ndata] of observe() against the case's reference; accepted: the rows that must
        be finite (default all), every other row +inf exactly."""
        out, bound = reference_of(c)[:2]
        rows = np.arange(c['nw'])
        accepted = rows if accepted is None else np.asarray(accepted, int)
        rejected = np.setdiff1d(rows, accepted)
        assert got.shape == out.shape
        assert np.all(np.isfinite(got[accepted])) and np.all(bound[accepted] > 0), where
        assert np.all(np.isposinf(got[rejected])) and np.all(np.isposinf(out[rejected])), where
        return self.add(got, out, bound, where)

    def check(self):
        print(f'{self.what}: worst |got - ref| / bound = {self.value:.3e} at {self.where}')
        assert self.value <= 1, (self.what, self.value, self.where)


# ---------------------------------------------------------------------------------------------
# 1. pb_hires_observe_batch: shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 3, 179, 1025])
@pytest.mark.parametrize('W', [2, 3, 1023, 1024, 1025, 2047, 2048])
def test_observe_shapes(eng, W, T):
    """Three walkers (rv 0, +, -), data on every shifted node of every walker and on the
    midpoints, slots a random permutation.  sample_scale is given at even W, walker_scale at
    W = 2, 1023, 2048: each is NULL and non-NULL for every T.  Both grids at W = 1025 and 2048;
    signed spectra and signed (asymmetric) taps at W = 2048, T = 179 and 1025."""
    variants = [dict(grid_kind='resolution')]
    if W in (1025, 2048):
        variants.append(dict(grid_kind='step'))
    if W == 2048 and T in (179, 1025):
        variants.append(dict(taps_kind='signed', spectrum_kind='mixed'))
    worst = Worst(f'observe W={W} T={T}')
    for kw in variants:
        c = hc.shape_case(W, T, sample_scale=(W % 2 == 0), walker_scale=(W in (2, 1023, 2048)),
                          **kw)
        assert (c['sample_scale'] is None) == (W % 2 == 1)
        worst.add_case(observe(eng, c), c, kw)
    worst.check()


# ---------------------------------------------------------------------------------------------
# 2. layouts
# ---------------------------------------------------------------------------------------------
LAYOUTS = [('one_per_tile', dict(empty=0)), ('one_per_tile', dict(empty=1)),
           ('one_per_tile', dict(empty=2)), ('threshold', dict(extra=True)),
           ('threshold', dict(extra=False)), ('crowd', dict(bracket=0)),
           ('crowd', dict(bracket=hc.TILE)), ('single', dict(bracket=hc.TILE)),
           ('single', dict(bracket=0))]


@pytest.mark.parametrize('T', [1, 1025])
@pytest.mark.parametrize('name,kw', LAYOUTS, ids=[f'{n}-{list(k.values())[0]}' for n, k in LAYOUTS])
def test_layouts(eng, name, kw, T):
    """A tile without data beside tiles with one point each; 256 and 257 needed samples; 3000
    points in one bracket (of the first tile, and of the 2-node last tile); one data point."""
    c = hc.layout_case(name, T, **kw)
    worst = Worst(f'layout {name} {kw} T={T}')
    got = observe(eng, c)
    worst.add_case(got, c, 'all')
    if name == 'crowd':
        # equal points get equal values, whichever lane and slot they went through
        d = in_data_order(got, c)
        equal = np.flatnonzero(c['data_wn'] == c['data_wn'][np.argmax(np.diff(c['data_wn']) == 0)])
        assert len(equal) == 500 and np.all(bits(d[:, equal]) == bits(d[:, equal[:1]]))
    worst.check()


@pytest.mark.parametrize('T', [1, 179, 1025])
def test_threshold_flip_has_equal_bits(eng, T):
    """The header's "same bits from either": tile 1 needs 257 samples (conv_dense) with the extra
    point and 256 (conv_one) without it, the other 256 points and their needed samples are the
    same.  The outputs common to both launches have equal bits."""
    dense, sparse = hc.layout_case('threshold', T), hc.layout_case('threshold', T, extra=False)
    extra = hc.threshold(dense['wn'])[1]
    assert np.array_equal(np.delete(dense['data_wn'], extra), sparse['data_wn'])
    worst = Worst(f'threshold flip T={T}')
    a, b = observe(eng, dense), observe(eng, sparse)
    worst.add_case(a, dense, '257 needed samples')
    worst.add_case(b, sparse, '256 needed samples')
    worst.check()
    assert np.array_equal(bits(np.delete(in_data_order(a, dense), extra, axis=1)),
                          bits(in_data_order(b, sparse)))


# ---------------------------------------------------------------------------------------------
# 3. fused against two launches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [3, 1025])
@pytest.mark.parametrize('W', [1025, 2048])
def test_fused_equals_two_launches(eng, W, T):
    """pb_inst_convolve_batch into a NaN-filled [nw, W], then the observe kernel with one unit
    tap on that buffer: the bits of the fused call."""
    c = hc.shape_case(W, T, sample_scale=True)
    assert c['walker_scale'] is None
    worst = Worst(f'fused / two launches W={W} T={T}')
    fused = observe(eng, c)
    worst.add_case(fused, c, 'fused')
    conv, held = convolve(eng, c['spectra'], c['taps'], c['sample_scale'])
    _, _, ref_conv, mag, _ = reference_of(c)
    worst.add(conv, ref_conv, hc.conv_bound(mag, T), 'convolved')
    unit = hc.modified(c, taps=np.ones(1), sample_scale=None)
    two = observe(eng, unit, spectra_d=held.body)
    worst.check()
    assert np.array_equal(bits(two), bits(fused))


# ---------------------------------------------------------------------------------------------
# 4. rejection
# ---------------------------------------------------------------------------------------------
def test_rejection_by_rv(eng):
    """rv_max = 20: +-20 exactly are accepted; one ulp beyond either, NaN and +-inf are rejected
    (+inf in the whole row: three tiles at W = 2048); the accepted rows have the bits of a launch
    without the rejected walkers."""
    W, T = 2048, 179
    wn = hc.grid('resolution', W)
    up = np.nextafter(20.0, np.inf)
    rv = np.array([20.0, up, -20.0, 3.0, -up, np.nan, 0.0, np.inf, -np.inf])
    ok = [0, 2, 3, 6]
    data = hc.on_every_node(wn, rv[ok])
    assert hc.tiles(W) == 3 and len(data) > 4 * (W - 20)
    spectra = hc.make_spectra('positive', len(rv), W, 41)
    c = hc.case(wn, hc.make_taps('gaussian', T), spectra, data, rv, 'random', sample_scale=True,
                walker_scale=True, rv_max=20.0, seed=41)
    worst = Worst('rejection by rv')
    got = observe(eng, c)
    worst.add_case(got, c, 'nine walkers', accepted=ok)
    alone = hc.modified(c, spectra=spectra[ok], rv=rv[ok], walker_scale=c['walker_scale'][ok])
    got_alone = observe(eng, alone)
    worst.add_case(got_alone, alone, 'the accepted four')
    worst.check()
    assert np.array_equal(bits(got[ok]), bits(got_alone))


def test_rejection_by_data(eng):
    """Data whose ends are the walker's own shifted end nodes are accepted, and the values there
    are c[0] and c[W - 1]; the same data reject a walker with another rv; one ulp outside either
    end rejects the walker, while a neighbour whose grid reaches that far is served."""
    W, T, v = 2048, 179, 7.5
    wn = hc.grid('resolution', W)
    x = hc.shifted(wn, v)
    full = hc.on_every_node(wn, v)
    assert full[0] == x[0] and full[-1] == x[-1]
    spectra = hc.make_spectra('positive', 3, W, 43)
    taps = hc.make_taps('gaussian', T)
    worst = Worst('rejection by data')

    def run(data, rv, accepted, what, rows=(0, 1, 2)):
        c = hc.case(wn, taps, spectra[list(rows)], data, rv, 'random', sample_scale=True,
                    rv_max=20.0, seed=43)
        got = observe(eng, c)
        worst.add_case(got, c, what, accepted=accepted)
        return c, got

    c, got = run(full, [v, -3.0, v], [0, 2], 'ends exactly')
    _, _, conv, mag, lo = reference_of(c)
    d = in_data_order(got, c)
    for w in (0, 2):
        for j, node, pair in ((0, 0, [0, 1]), (-1, W - 1, [W - 2, W - 1])):
            assert lo[w, c['slot'][j]] == pair[0]
            worst.add(d[w:w + 1, j], conv[w:w + 1, node],
                      hc.LD(T + 8) * hc.EPS * np.max(mag[w, pair], keepdims=True),
                      f'walker {w} on end node {node}')
    _, got_pair = run(full, [v, v], [0, 1], 'without the rejected walker', rows=(0, 2))
    assert np.array_equal(bits(got[[0, 2]]), bits(got_pair))
    low = full[:-1].copy()
    low[0] = np.nextafter(x[0], -np.inf)
    run(low, [v, 7.6, v], [1], 'one ulp below the first node')
    high = full[1:].copy()
    high[-1] = np.nextafter(x[-1], np.inf)
    run(high, [v, 7.4, v], [1], 'one ulp above the last node')
    worst.check()


def test_rv_max_zero(eng):
    """rv_max = 0: rv = -0.0 and +0.0 are accepted (the same bits), the smallest positive rv is
    not."""
    W, T = 1025, 3
    wn = hc.grid('step', W)
    spectra = np.tile(hc.make_spectra('positive', 1, W, 47), (3, 1))
    c = hc.case(wn, hc.make_taps('gaussian', T), spectra, hc.on_every_node(wn, 0.0),
                [-0.0, 0.0, 5e-324], 'random', rv_max=0.0, seed=47)
    assert np.signbit(c['rv'][0])
    worst = Worst('rv_max = 0')
    got = observe(eng, c)
    worst.add_case(got, c, 'rv -0.0, 0.0, 5e-324', accepted=[0, 1])
    worst.check()
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_non_finite_spectrum(eng):
    """One walker with a NaN in one sample and +inf in another: its neighbours have the bits of a
    launch with that walker's spectrum finite; its own outputs are finite exactly where the
    reference's are (there within the bound), and the reference's non-finite value elsewhere."""
    W, T = 2048, 179
    base = hc.shape_case(W, T, sample_scale=True, walker_scale=True)
    spectra = np.array(base['spectra'])
    spectra[1, 700], spectra[1, 1500] = np.nan, np.inf
    c = hc.modified(base, spectra=spectra)
    plain, got = observe(eng, base), observe(eng, c)
    assert np.all(np.isfinite(plain))
    assert np.array_equal(bits(got[[0, 2]]), bits(plain[[0, 2]]))
    out, bound = reference_of(c)[:2]
    finite = np.isfinite(out[1])
    assert 0 < finite.sum() < finite.size and np.isnan(out[1]).any() and np.isposinf(out[1]).any()
    assert np.array_equal(np.isfinite(got[1]), finite)
    worst = Worst('non-finite spectrum')
    worst.add(got[[0, 2]], out[[0, 2]], bound[[0, 2]], 'neighbours')
    worst.add(got[1:2, finite], out[1:2, finite], bound[1:2, finite], 'own finite outputs')
    worst.check()
    assert rel_dev(got[1, ~finite], out[1, ~finite]) == 0.0


# ---------------------------------------------------------------------------------------------
# 5. limits, no-ops, refusals
# ---------------------------------------------------------------------------------------------
def test_walker_limit(eng):
    """65535 walkers (gridDim.y's last value) of W = 2, T = 1, ndata = 1, every fourth beyond
    rv_max; 65536 are refused and leave `out` alone."""
    from pyratbay_amd import _capi
    nw = 65535
    wn = hc.grid('resolution', 2)
    rv = np.resize(np.array([0.0, 0.7, -0.4, 25.0]), nw)
    c = hc.case(wn, np.ones(1), hc.make_spectra('positive', nw, 2, 53), hc.single(wn, 0), rv,
                'identity', walker_scale=True, seed=53)
    worst = Worst('65535 walkers')
    got = observe(eng, c)
    worst.add_case(got, c, 'all', accepted=np.flatnonzero(rv != 25.0))
    worst.check()
    out = Dirty(nw, 1)
    with pytest.raises(_capi.PbError, match=rf'\): {OBSERVE}: more than 65535 walkers'):
        observe(eng, c, into=out, nwalkers=65536)
    assert out.untouched()


def test_observe_noops_and_refusals(eng):
    """ndata = 0 and nwalkers = 0 return PB_OK; nwave = 1, ntaps = 0, 2, 1027, rv_max < 0 (and
    NaN), rv_max 1e5 >= c and each of the six required pointers NULL raise PbError with the entry
    point's own message.  `out` keeps its NaN through all of it; then the same arguments,
    unmodified, run."""
    from pyratbay_amd import _capi
    c = hc.shape_case(1025, 3)
    out = Dirty(c['nw'], c['ndata'])
    observe(eng, c, into=out, ndata=0)
    observe(eng, c, into=out, nwalkers=0)
    assert out.untouched()
    refused = [dict(nwave=1), dict(ntaps=0), dict(ntaps=2), dict(ntaps=1027), dict(rv_max=-1.0),
               dict(rv_max=float('nan')), dict(rv_max=hc.C_LIGHT / hc.KM),
               dict(rv_max=float('inf'))]
    refused += [{name: None} for name in ('out', 'spectra', 'wn', 'taps', 'data', 'slot')]
    for bad in refused:
        with pytest.raises(_capi.PbError, match=rf'\): {OBSERVE}: '):
            observe(eng, c, into=out, **bad)
        assert out.untouched(), bad
    with pytest.raises(_capi.PbError, match='at most 1025'):
        observe(eng, c, into=out, ntaps=1027)
    # the three optional pointers may be NULL: sample_scale and walker_scale are in this case,
    # and rv NULL is rv = 0 for every walker
    observe(eng, c, into=out, rv=None)
    at_rest = hc.modified(c, rv=np.zeros(3))
    worst = Worst('after the refusals, rv NULL')
    worst.add_case(out.body.cpu().numpy(), at_rest, 'rv NULL = rv 0')
    worst.check()


@pytest.mark.parametrize('nw', [1, 3])
@pytest.mark.parametrize('T', [1, 3, 1023, 1025])
@pytest.mark.parametrize('W', [1, 2, 1023, 1024, 1025, 2049])
def test_convolve_shapes(eng, W, T, nw):
    """pb_inst_convolve_batch around its own tile of 1024 outputs, T > W included, against the
    reference's conv at (T + 2) 2^-53 conv_mag; sample_scale NULL and given; Gaussian, signed and
    single-unit taps, positive and signed spectra."""
    worst = Worst(f'convolve W={W} T={T} nw={nw}')
    rng = np.random.default_rng(W + T)
    for taps_kind, spectrum_kind, scaled in (('gaussian', 'positive', False),
                                            ('signed', 'mixed', True), ('unit', 'mixed', False)):
        taps = hc.make_taps(taps_kind, T)
        spectra = hc.make_spectra(spectrum_kind, nw, W, 3 * W + T)
        scale = rng.uniform(0.5, 2.0, W) if scaled else None
        got, _ = convolve(eng, spectra, taps, scale)
        conv, mag = hc.convolve(hc.samples(spectra, scale), taps)
        assert np.all(np.isfinite(got))
        worst.add(got, conv, hc.conv_bound(mag, T), (taps_kind, spectrum_kind))
        if taps_kind == 'unit':
            assert np.array_equal(got, conv.astype(np.float64))     # a shift: exact
    worst.check()


def test_convolve_noops_and_refusals(eng):
    """nwave = 0 and nwalkers = 0 return PB_OK; an in-place call, ntaps even, 0 or 1027, 65536
    walkers and each required pointer NULL raise; `out` keeps its NaN."""
    from pyratbay_amd import _capi
    W, T = 1025, 3
    spectra, taps = hc.make_spectra('positive', 2, W, 59), hc.make_taps('gaussian', T)
    out = Dirty(2, W)
    convolve(eng, spectra, taps, into=out, nwave=0)
    convolve(eng, spectra, taps, into=out, nwalkers=0)
    assert out.untouched()
    for bad in (dict(out='spectra'), dict(ntaps=0), dict(ntaps=2), dict(ntaps=1027),
                dict(nwalkers=65536), dict(nwave=-1), dict(out=None), dict(spectra=None),
                dict(taps=None)):
        with pytest.raises(_capi.PbError, match=rf'\): {CONVOLVE}: '):
            convolve(eng, spectra, taps, into=out, **bad)
        assert out.untouched(), bad
    got, _ = convolve(eng, spectra, taps, into=out)
    conv, mag = hc.convolve(hc.samples(spectra), taps)
    worst = Worst('convolve after the refusals')
    worst.add(got, conv, hc.conv_bound(mag, T), 'all')
    worst.check()


# ---------------------------------------------------------------------------------------------
# 6. through HiresData
# ---------------------------------------------------------------------------------------------
def test_hires_data_on_a_seam(eng):
    """HiresData at W = 1025 (a last tile of 2 nodes): data on the walkers' shifted node 1023 and
    on both ends of their grid, in a shuffled order; integrate_batch() on outputs that start as
    NaN returns the caller's order; a walker with another rv is rejected by those data; the
    two-launch form gives the same bits."""
    import torch
    W, v = 1025, 7.5
    wn = hc.grid('resolution', W)
    x = hc.shifted(wn, v)
    rng = np.random.default_rng(61)
    data = np.concatenate([x[[0, hc.TILE, W - 1, hc.TILE - 1, 1]], rng.uniform(x[0], x[-1], 60)])
    data = data[rng.permutation(len(data))]
    assert not np.all(np.diff(data) > 0)
    h = eng.HiresData(wn, data, 25000.0, sampling_res=123300.0, rv_max=hc.RV_MAX,
                      check_data=False)
    spectra = hc.make_spectra('positive', 3, W, 61)
    rv, fd = np.array([v, 0.0, v]), np.array([0.9, 0.8, 0.75])
    results = []
    for fused in (True, False):
        h.fused = fused
        with dirty_outputs():
            got = h.integrate_batch(upload(eng, spectra), rv=upload(eng, rv),
                                    f_dilution=upload(eng, fd))
        torch.cuda.synchronize()
        results.append(got.cpu().numpy())
    out, bound, _, _, lo = hc.reference(spectra, wn, h.taps_host, data, rv, walker_scale=fd)
    assert np.all(np.isposinf(out[1])) and np.all(np.isposinf(results[0][1]))
    assert lo[0, np.flatnonzero(data == x[hc.TILE])[0]] == hc.TILE - 1
    worst = Worst(f'HiresData W={W} T={len(h.taps_host)}')
    worst.add(results[0], out, bound, 'fused')
    worst.check()
    assert np.array_equal(bits(results[0]), bits(results[1]))
