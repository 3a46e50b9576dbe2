"""The band contribution kernels at the kernel boundary (csrc/pb_contribution.hip:
pb_band_contribution_emission_batch, pb_band_transmittance_batch -> k_band_cf_emission,
k_band_transmittance, k_band_cf_finish), driven through the C ABI on dirty memory, against the long
double reference of contribution_cases.py.

Every launch: `out` and `work` are NaN before the call and each sits between two guard blocks of 3
NaN that must still be NaN afterwards; `work` has exactly pb_band_contribution_work_doubles(...)
doubles; `wn` is an interior view of a NaN-padded tensor (3 doubles on each side), so a read one
past either end of the grid lands in the test's own allocation and comes out as NaN; the inputs are
uploaded from copies and kept alive by name; one synchronize before the result is read.  Every
comparison is |got - ref| <= contribution_cases.bound(case) = max(10 sens, 1e-14) (fixture G24's
rule; a case with sens > 1e-9 is refused when it is built) with an identical NaN pattern, or an
equal-bits statement between two launches.  Each check prints its worst |got - ref| / bound and
where, then asserts <= 1.  Every band without a NaN has the maximum 1.0 exactly, and where the
reference's peak stands more than 1e-6 above the other layers (case['peak']) it is that layer.
That the cases are the situations named here is asserted in test_contribution_cases_cpu.py on the
reference alone.

Which test launches which situation (the numbers are those of the gaps this file closes):

   1 a band that leaves the grid: start + count > nwave and    test_clipped_bands (against the
     start < 0 with >= 2, 1, 0 samples retained, more than      reference; the bits of the in-grid
     the whole grid, across a chunk seam (513, 300 retained)    band with the sliced response; NaN
                                                                for <= 1 sample; wn's pads intact)
   2 L = 2, 3, 255, 256, 257, 513 and the limits 1024           test_layer_counts (W = 70),
     (emission, two-stream: 65 520 B of LDS) and 2048           test_band_counts (L = 257, W = 600:
     (transit: 65 536 B); band counts 1, 2, 255, 256, 257,      three chunks x more layers than
     513, 600; from sample 0, to the last, overlapping          threads)
   3 ibottom = itop + 1, L // 2, L - 1, L, and <= itop          test_stop_rule
   4 maxdepth = 0; acc == maxdepth exactly and its twin one     test_stop_rule, test_equality_twin,
     ulp above; jumps kept and zeroed at L = 257; itop =        test_small_maxdepth,
     L - 1 (every column sums to 0: NaN) and L - 2; a           test_layer_counts (itop in 0, 2,
     column with ec = 0                                         L - 2, L - 1), test_special_values
   5 three walkers with their own temperatures, intervals       test_layer_counts, test_band_counts,
     and strengths at the entry; one walker                     test_independence
   6 ideep = 0, itop, itop + 1, L - 1, L; -5 and L + 7          test_ideep
   7 work NaN and 1e300, max_band_count 4 x the largest         test_work_layout
     count, a band of count 0 between two others
   8 NaN in the rows above itop, below each column's stop /     test_unread_memory
     from ideep on, in wn, the response and the columns
     outside every band
   9 65 535 bands, 65 535 walkers; 65 536 refused; no-ops;      test_limits,
     every refusal of the header, `out` and `work` untouched    test_noops_and_refusals
  10 a walker alone, a band alone, two runs; NaN and +inf       test_independence,
     in one walker's column                                     test_special_values

Found, both under item 1:
  * band_weight() decided its half-gaps by the position in the band alone, so the last grid
    sample of a band that runs past the end read wn[nwave] (and sample 0 of a band with a negative
    start wn[-1]) -- a read outside wn_d, and a weight that was not the one-sided trapezoid weight
    of the clipped band.  It now also asks for the neighbour to lie on the grid; for in-grid bands
    the conditions are unchanged.
  * With that weight the clipped bands met the reference (worst ratio 8e-3), but a band with a
    negative start did not have the BITS of the in-grid band of its retained samples: its lanes
    counted from the unclipped start, so the same terms met in another order in the wavefront sums
    and chunks.  band_sample() now counts lanes and chunks from the band's first sample on the
    grid (and the finish kernel adds the chunks of the retained samples only); for an in-grid
    band nothing moves.

Result: with these two changes every test passes; nothing else in pb_contribution.hip was changed
(the measured ratios are in profiles/contribution.md)."""
import numpy as np
import pytest

import contribution_cases as cc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not cc.EXTENDED, reason='np.longdouble is not an extended type')]

GUARD = 3
EMISSION, TRANSIT = 'pb_band_contribution_emission_batch', 'pb_band_transmittance_batch'
NAN = float('nan')


def entry_of(c):
    return TRANSIT if c['rt'] == 'transit' else EMISSION


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


class Dirty:
    """n doubles of `fill` between two guard blocks of GUARD NaN."""

    def __init__(self, n, fill=NAN):
        import torch
        self.n, self.fill = n, fill
        self.store = torch.full((2 * GUARD + n,), NAN, dtype=torch.float64, device='cuda')
        self.body = self.store[GUARD:GUARD + n]
        self.body.fill_(fill)
        self.ptr = self.store.data_ptr() + 8 * GUARD

    def guards_intact(self):
        import torch
        return bool(torch.isnan(self.store[:GUARD]).all()) and \
            bool(torch.isnan(self.store[GUARD + self.n:]).all())

    def untouched(self):
        import torch
        same = torch.isnan(self.body) if self.fill != self.fill else self.body == self.fill
        return self.guards_intact() and bool(same.all())


def padded(eng, a):
    """(store, pointer): the array as an interior view of a NaN-padded device tensor."""
    import torch
    store = torch.full((2 * GUARD + len(a),), NAN, dtype=torch.float64, device='cuda')
    store[GUARD:GUARD + len(a)] = eng.dev(np.array(a), torch.float64)
    return store, store.data_ptr() + 8 * GUARD


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def work_doubles(c, **over):
    from pyratbay_amd import _capi
    n = dict(nlayers=c['L'], nbands=c['nb'], max_band_count=c['max_band_count'], nwalkers=c['nw'])
    n.update({k: v for k, v in over.items() if k in n})
    return _capi.call('pb_band_contribution_work_doubles', n['nlayers'], n['nbands'],
                      n['max_band_count'], n['nwalkers'])


def launch(eng, c, into=None, scratch=None, replace=None, **over):
    """The case's entry on dirty memory -> host [nw, L, nb].  into, scratch: the Dirty blocks for
    `out` and `work` (default: fresh NaN ones, work of exactly the size the library asks for);
    replace: host arrays uploaded instead of the case's, by name; over: arguments replaced by name
    (a pointer by None, a count by another)."""
    import torch
    from pyratbay_amd import _capi
    h = dict(c)
    h.update(replace or {})

    def up(name, dtype=torch.float64):
        return eng.dev(np.array(h[name]), dtype)
    wn_store, wn_ptr = padded(eng, h['wn'])
    start, count = up('band_start', torch.int32), up('band_count', torch.int32)
    response, offset = up('response'), up('response_offset', torch.int64)
    nw, L, W, nb = c['nw'], c['L'], c['W'], c['nb']
    out = Dirty(nw * L * nb) if into is None else into
    work = Dirty(work_doubles(c, **over)) if scratch is None else scratch
    a = dict(out=out.ptr, wn=wn_ptr, band_start=start.data_ptr(), band_count=count.data_ptr(),
             response=response.data_ptr(), response_offset=offset.data_ptr(),
             max_band_count=c['max_band_count'], itop=c['itop'], nlayers=L, nwave=W, nbands=nb,
             nwalkers=nw, work=work.ptr)
    if c['rt'] == 'emission':
        ec, intervals, dlogp, temps = up('ec'), up('intervals'), up('dlogp'), up('temps')
        a.update(ec=ec.data_ptr(), intervals=intervals.data_ptr(), dlogp=dlogp.data_ptr(),
                 temps=temps.data_ptr(), maxdepth=c['maxdepth'], ibottom=c['ibottom'])
        order = ('out', 'ec', 'intervals', 'dlogp', 'wn', 'temps', 'band_start', 'band_count',
                 'response', 'response_offset', 'max_band_count', 'maxdepth', 'itop', 'ibottom',
                 'nlayers', 'nwave', 'nbands', 'nwalkers', 'work')
    else:
        depth, ideep = up('depth'), up('ideep', torch.int32)
        a.update(depth=depth.data_ptr(), ideep=ideep.data_ptr())
        order = ('out', 'depth', 'ideep', 'wn', 'band_start', 'band_count', 'response',
                 'response_offset', 'max_band_count', 'itop', 'nlayers', 'nwave', 'nbands',
                 'nwalkers', 'work')
    assert set(over) <= set(a), sorted(set(over) - set(a))
    a.update(over)
    try:
        rc = _capi.call(entry_of(c), *[a[k] for k in order], stream())
    finally:
        torch.cuda.synchronize()
    assert rc == _capi.PB_OK and out.guards_intact() and work.guards_intact()
    assert bool(torch.isnan(wn_store[:GUARD]).all()) and bool(torch.isnan(wn_store[-GUARD:]).all())
    return out.body.cpu().numpy().reshape(nw, L, nb)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Worst:
    """The worst |got - ref| / bound of a test group, printed before the assertion."""

    def __init__(self, what):
        self.what, self.value, self.where = what, 0.0, None

    def add(self, got, c, where):
        """got[nw, L, nb] against the case's reference at the case's bound; the peaks."""
        ratio, k = cc.deviation(got, c)
        if self.where is None or ratio > self.value:
            self.value, self.where = ratio, (where, k, f'bound {cc.bound(c):.2e}')
        assert np.array_equal(np.isnan(got), np.isnan(c['ref'])), (self.what, where)
        whole = ~np.isnan(got).any(axis=1)
        assert np.all(np.max(got, axis=1)[whole] == 1.0), (self.what, where)
        at = np.argmax(np.where(np.isnan(c['ref']), -np.inf, c['ref']), axis=1)
        peak = np.take_along_axis(got, at[:, None, :], axis=1)[:, 0]
        assert np.all(peak[c['peak']] == 1.0), (self.what, where)
        return ratio

    def check(self):
        print(f'{self.what}: worst |got - ref| / bound = {self.value:.3e} at {self.where}')
        assert self.value <= 1, (self.what, self.value, self.where)


def top_layers(geometry):
    return cc.MAX_LAYERS['transit' if geometry == 'transit' else 'emission']


# ---------------------------------------------------------------------------------------------
# 1. shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [2, 3, 255, 256, 257, 513, 'limit'])
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_layer_counts(eng, geometry, L):
    """W = 70, three walkers of their own, itop in {0, 2, L - 2, L - 1}; at itop = 0 also the
    first walker alone, launched as nwalkers = 1 on the batch's arrays: its bits, and the other
    walkers' rows of `out` stay NaN.  'limit': 1024 layers (emission, two-stream) and 2048
    (transit), the largest LDS carve-ups."""
    L = top_layers(geometry) if L == 'limit' else L
    worst = Worst(f'{geometry} L={L}')
    for itop in cc.itops(L):
        c = cc.shape_case(geometry, L, 70, 3, itop)
        got = launch(eng, c)
        worst.add(got, c, f'itop={itop}')
        if geometry != 'transit' and itop == L - 1:
            assert np.all(np.isnan(got))                      # (every column sums to 0)
        if itop == 0:
            one = launch(eng, c, nwalkers=1)
            assert same_bits(one[0], got[0]) and np.all(np.isnan(one[1:]))
    worst.check()


@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_band_counts(eng, geometry):
    """L = 257, W = 600, itop = 2: band counts 1, 2, 255, 256, 257, 513 and 600, a band from
    sample 0, one to the last sample, two overlapping bands; one and three walkers."""
    c = cc.shape_case(geometry, 257, 600, 3, 2)
    assert {1, 2, 255, 256, 257, 513, 600} <= set(c['band_count'].tolist())
    worst = Worst(f'{geometry} band counts')
    got = launch(eng, c)
    worst.add(got, c, 'three walkers')
    one = launch(eng, c, nwalkers=1)
    assert same_bits(one[0], got[0]) and np.all(np.isnan(one[1:]))
    worst.check()


# ---------------------------------------------------------------------------------------------
# 2. the stop rule
# ---------------------------------------------------------------------------------------------
def test_stop_rule(eng):
    """L = 12, itop = 2: ibottom = itop + 1, L // 2, L - 1, L and <= itop (never matches: the
    result of ibottom = L, bit for bit), without maxdepth (inf) and with 10; maxdepth = 0 (every
    column stops at itop + 1)."""
    L, itop = 12, 2
    worst = Worst('stop rule')
    for geometry in ('two_stream', 'emission'):
        results = {}
        for ibottom in (itop + 1, L // 2, L - 1, L, itop, 0, -3):
            c = cc.shape_case(geometry, L, 70, 3, itop, ibottom=ibottom)
            results[ibottom] = launch(eng, c)
            worst.add(results[ibottom], c, f'{geometry} ibottom={ibottom}')
        for ibottom in (itop, 0, -3, L - 1):
            assert same_bits(results[ibottom], results[L]), ibottom
        assert not same_bits(results[L // 2], results[L])
        assert not same_bits(results[itop + 1], results[L // 2])
    c = cc.shape_case('emission', L, 70, 3, itop, maxdepth=0.0)
    worst.add(launch(eng, c), c, 'maxdepth=0')
    worst.check()


def test_equality_twin(eng):
    """ec = 2^-20, intervals powers of two: acc = 4 = maxdepth exactly at layer 3, in double as in
    long double; the column stops there (>=), and one layer later in the twin whose maxdepth is
    one ulp larger."""
    a, b = cc.equality_case(False), cc.equality_case(True)
    worst = Worst('acc == maxdepth')
    got_a, got_b = launch(eng, a), launch(eng, b)
    worst.add(got_a, a, 'maxdepth = 4')
    worst.add(got_b, b, 'maxdepth = nextafter(4)')
    worst.check()
    assert not same_bits(got_a, got_b)


def test_small_maxdepth(eng):
    """G24's e_md at L = 257: maxdepth = 0.105, jumps back to depth 0 kept (<= 0.1) and zeroed."""
    c = cc.small_maxdepth_case()
    worst = Worst('small maxdepth')
    worst.add(launch(eng, c), c, 'L=257')
    worst.check()


# ---------------------------------------------------------------------------------------------
# 3. clipped bands
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_clipped_bands(eng, geometry):
    """Bands that leave the grid at either end (>= 2, 1, 0 samples retained), one that covers
    more than the grid, two of count 513 across a chunk seam with 300 retained: the reference's
    one-sided weight at the clip; no NaN from wn's pads where >= 2 samples are retained; the bits
    of the in-grid band of the retained samples with the sliced response; NaN in every layer for
    <= 1 retained sample."""
    c = cc.clipped_case(geometry)
    worst = Worst(f'{geometry} clipped bands')
    got = launch(eng, c)
    retained = np.array([n for _, n in cc.clipped_spans(c['W']).values()])
    assert np.all(np.isnan(got[:, :, retained <= 1]))
    assert np.all(np.isfinite(got[:, :, retained >= 2]))
    worst.add(got, c, 'clipped')
    s, which = cc.sliced_case(c)
    assert np.array_equal(np.flatnonzero(retained >= 2), which)
    got_s = launch(eng, s)
    worst.add(got_s, s, 'sliced')
    worst.check()
    assert same_bits(got[:, :, which], got_s)


# ---------------------------------------------------------------------------------------------
# 4. the work buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_work_layout(eng, geometry):
    """max_band_count = the largest count and 4 x that (chunks nobody writes), work pre-filled
    with NaN and with 1e300: the same bits.  A band of count 0 between two others: a NaN column,
    and the neighbours have the bits of the call without it."""
    spans = ((3, 300), (50, 0), (20, 257))
    c = cc.shape_case(geometry, 9, 600, 2, 0, spans=spans)
    wide = cc.shape_case(geometry, 9, 600, 2, 0, spans=spans, max_factor=4)
    assert wide['max_band_count'] == 1200 and c['max_band_count'] == 300
    assert work_doubles(wide) == 5 * 2 * 3 * 9 and work_doubles(c) == 2 * 2 * 3 * 9
    worst = Worst(f'{geometry} work layout')
    got = launch(eng, c)
    worst.add(got, c, 'max_band_count = 300')
    assert np.all(np.isnan(got[:, :, 1])) and np.all(np.isfinite(got[:, :, [0, 2]]))
    for case, fill in ((wide, NAN), (c, 1e300), (wide, 1e300)):
        other = launch(eng, case, scratch=Dirty(work_doubles(case), fill))
        worst.add(other, case, f'max_band_count = {case["max_band_count"]}, work = {fill}')
        assert same_bits(other, got), (case['max_band_count'], fill)
    without = cc.shape_case(geometry, 9, 600, 2, 0, spans=(spans[0], spans[2]))
    got_w = launch(eng, without)
    worst.add(got_w, without, 'without the empty band')
    worst.check()
    assert same_bits(got_w, got[:, :, [0, 2]])


# ---------------------------------------------------------------------------------------------
# 5. independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_independence(eng, geometry):
    """Walker w of a batch of three = the launch of walker w alone; band b = the launch with band
    b alone (max_band_count, and with it the chunk grid, changes); two runs: equal bits."""
    c = cc.shape_case(geometry, 9, 600, 3, 2)
    worst = Worst(f'{geometry} independence')
    got = launch(eng, c)
    worst.add(got, c, 'batch')
    assert same_bits(launch(eng, c), got)
    for w in range(3):
        alone = cc.walker(c, w)
        got_w = launch(eng, alone)
        worst.add(got_w, alone, f'walker {w} alone')
        assert same_bits(got_w[0], got[w]), w
    for b in (1, 3, 5, 6, 7, 10):
        alone = cc.one_band(c, b)
        assert alone['max_band_count'] == c['band_count'][b]
        got_b = launch(eng, alone)
        worst.add(got_b, alone, f'band {b} alone')
        assert same_bits(got_b[:, :, 0], got[:, :, b]), b
    worst.check()


# ---------------------------------------------------------------------------------------------
# 6. memory the header says is not read
# ---------------------------------------------------------------------------------------------
GAPPY = ((5, 1), (9, 2), (100, 257), (300, 100), (350, 80))


@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_unread_memory(eng, geometry):
    """NaN in: the rows above itop; the rows below each column's stop (emission) or from ideep on
    (transit); every column outside every band (wn too); the response doubles no band reads.  The
    bits of the clean launch."""
    L, W, itop = 12, 600, 2
    c = cc.shape_case(geometry, L, W, 3, itop, spans=GAPPY)
    in_band = np.zeros(W, bool)
    for b in range(c['nb']):
        in_band[cc.band_samples(c, b)[0]] = True
    assert 0 < in_band.sum() < W and not c['response_used'].all()
    rows = np.arange(L)[None, :, None]
    main = 'depth' if geometry == 'transit' else 'ec'
    dirty = np.array(c[main])
    if geometry == 'transit':
        unread = (rows < itop) | (rows >= c['ideep'][:, None, :])
    else:
        unread = (rows < itop) | (rows > c['stop'][:, None, :])
        if geometry == 'emission':
            assert len(np.unique(c['stop'])) >= 3
    unread = unread | ~in_band[None, None, :]
    if geometry != 'two_stream':                              # (below a stop, inside a band)
        assert unread[:, itop:].any(axis=1)[:, in_band].any()
    dirty[unread] = NAN
    replace = {main: dirty, 'wn': np.where(in_band, c['wn'], NAN),
               'response': np.where(c['response_used'], c['response'], NAN)}
    worst = Worst(f'{geometry} unread memory')
    clean = launch(eng, c)
    worst.add(clean, c, 'clean')
    got = launch(eng, c, replace=replace)
    worst.add(got, c, 'NaN where the header says nothing is read')
    worst.check()
    assert same_bits(got, clean)


# ---------------------------------------------------------------------------------------------
# 7. special values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_special_values(eng, geometry):
    """Walker 1 has a NaN in one column and a +inf in another (of ec / of depth), and in emission
    a third column with ec = 0 throughout (a column sum of 0).  The bands that contain the NaN or
    the zero-sum column are NaN in every layer, the band with the +inf (which merely stops the
    column) is finite, all as in the reference; every other band and walker keeps the bits of the
    clean launch."""
    L, W = 12, 600
    base = cc.shape_case(geometry, L, W, 3, 0, spans=GAPPY)
    main = 'depth' if geometry == 'transit' else 'ec'
    a = np.array(base[main])
    # how far down walker 1 reads each column: the rows 3 (NaN) and 4 (+inf) must be read
    reach = base['ideep'][1] - 1 if geometry == 'transit' else base['stop'][1]
    nan_col = 9 + int(np.argmax(reach[9:11]))                               # band 1 only
    inf_col = 120 + int(np.argmax(reach[120:290] >= 5))                     # band 2 only
    zero_col = 420                                                          # band 4 only
    assert reach[nan_col] >= 4 and reach[inf_col] >= 5
    a[1, 3, nan_col], a[1, 4, inf_col] = NAN, np.inf
    if geometry != 'transit':
        a[1, :, zero_col] = 0.0
    c = cc.modified(base, **{main: a})
    holds = [np.flatnonzero([g0 <= col < g0 + n for g0, n in zip(c['band_start'],
                                                                  c['band_count'])]).tolist()
             for col in (nan_col, inf_col, zero_col)]
    assert holds == [[1], [2], [4]]
    nan = np.isnan(c['ref']).all(axis=1)
    assert np.array_equal(np.isnan(c['ref']).any(axis=1), nan)
    want = np.array([True, True, False, False, geometry != 'transit'])
    assert np.array_equal(nan[1], want)
    assert np.array_equal(nan[0], np.arange(5) == 0) and np.array_equal(nan[2], nan[0])
    clean, got = launch(eng, base), launch(eng, c)
    worst = Worst(f'{geometry} special values')
    worst.add(clean, base, 'clean')
    worst.add(got, c, 'NaN, +inf, zero sum')
    worst.check()
    assert np.all(np.isfinite(got[1, :, 2])) and not same_bits(got[1, :, 2], clean[1, :, 2])
    assert same_bits(got[[0, 2]], clean[[0, 2]])
    assert same_bits(got[1, :, 3], clean[1, :, 3])


# ---------------------------------------------------------------------------------------------
# 8. ideep
# ---------------------------------------------------------------------------------------------
def test_ideep(eng):
    """Transit, L = 9, itop = 2: every column's ideep = 0 (the band maximum is 0: NaN), itop,
    itop + 1, L - 1, L, against the reference; -5 and L + 7 give the bits of 0 and L."""
    L, W, itop = 9, 70, 2
    base = cc.shape_case('transit', L, W, 3, itop)
    worst = Worst('ideep')
    results = {}
    for value in (0, itop, itop + 1, L - 1, L, -5, L + 7):
        ideep = np.full((3, W), value, np.int32)
        ideep[2, ::3] = base['ideep'][2, ::3]                 # (the third walker: mixed)
        c = cc.modified(base, ideep=ideep)
        results[value] = launch(eng, c)
        worst.add(results[value], c, f'ideep={value}')
    worst.check()
    one_sample = base['band_count'] == 1
    assert np.all(np.isnan(results[0][:2])) and np.all(np.isfinite(results[0][2][:, ~one_sample]))
    assert np.all(np.isfinite(results[itop][:, :, ~one_sample]))
    assert same_bits(results[-5], results[0]) and same_bits(results[L + 7], results[L])
    assert not same_bits(results[L - 1], results[L])


# ---------------------------------------------------------------------------------------------
# 9. limits, no-ops, refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['bands', 'walkers'])
@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_limits(eng, geometry, what):
    """65 535 bands x 1 walker and 1 band x 65 535 walkers (gridDim.y's and gridDim.z's last
    value) at L = 2, W = 2, count = 2; 65 536 of either is refused and leaves `out` and `work`
    alone."""
    from pyratbay_amd import _capi
    c = cc.limit_case(geometry, what)
    worst = Worst(f'{geometry} 65535 {what}')
    worst.add(launch(eng, c), c, 'all')
    worst.check()
    out, work = Dirty(c['nw'] * c['L'] * c['nb']), Dirty(work_doubles(c))
    with pytest.raises(_capi.PbError, match=rf'\): {entry_of(c)}: at most 65535 bands and walkers'):
        launch(eng, c, into=out, scratch=work, **{'n' + what: 65536})
    assert out.untouched() and work.untouched()


@pytest.mark.parametrize('geometry', cc.GEOMETRIES)
def test_noops_and_refusals(eng, geometry):
    """nbands = 0 and nwalkers = 0 return PB_OK; bad sizes, itop outside the layers, ibottom >
    nlayers, one layer more than the LDS holds, each required pointer NULL and a NULL work buffer
    with max_band_count > 0 raise PbError with the entry point's own message.  `out` and `work`
    keep their NaN through all of it; then the same arguments, unmodified, run."""
    from pyratbay_amd import _capi
    c = cc.shape_case(geometry, 9, 70, 3, 2)
    L, name = c['L'], entry_of(c)
    out, work = Dirty(c['nw'] * L * c['nb']), Dirty(work_doubles(c))
    launch(eng, c, into=out, scratch=work, nbands=0)
    launch(eng, c, into=out, scratch=work, nwalkers=0)
    assert out.untouched() and work.untouched()
    refused = [dict(nlayers=0), dict(nwave=0), dict(nbands=-1), dict(nwalkers=-1),
               dict(max_band_count=-1), dict(itop=-1), dict(itop=L),
               dict(nlayers=top_layers(geometry) + 1), dict(nbands=65536), dict(nwalkers=65536),
               dict(work=None)]
    pointers = ['out', 'wn', 'band_start', 'band_count', 'response', 'response_offset']
    if geometry == 'transit':
        pointers += ['depth', 'ideep']
    else:
        refused += [dict(nlayers=1), dict(ibottom=L + 1)]
        pointers += ['ec', 'intervals', 'dlogp', 'temps']
    refused += [{p: None} for p in pointers]
    for bad in refused:
        with pytest.raises(_capi.PbError, match=rf'\): {name}: '):
            launch(eng, c, into=out, scratch=work, **bad)
        assert out.untouched() and work.untouched(), bad
    with pytest.raises(_capi.PbError, match=f'at most {top_layers(geometry)} fit'):
        launch(eng, c, into=out, scratch=work, nlayers=top_layers(geometry) + 1)
    got = launch(eng, c, into=out, scratch=work)
    worst = Worst(f'{geometry} after the refusals')
    worst.add(got, c, 'all')
    worst.check()
