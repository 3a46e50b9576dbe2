"""Cases and a plain high-precision reference for the band contribution kernels
(csrc/pb_contribution.hip: pb_band_contribution_emission_batch, pb_band_transmittance_batch).
NumPy only: no GPU, no torch, no SciPy.

reference() is written out from the contract of include/pbhip.h in np.longdouble (64-bit mantissa;
EXTENDED says whether this platform has it -- the users of this module skip where it has not, and
nothing here falls back to double).  It starts from the entry's own inputs:

  emission, two-stream   acc = running trapezoid of ec over intervals from itop; a column stops at
                         the first layer k > itop with acc >= maxdepth, k == ibottom or k == L - 1
                         (orc_plane_parallel_optical_depth's rule; ibottom <= itop never matches);
                         depth = acc between itop and the stop, 0 elsewhere;
                         detau = diff(exp(-depth)), elements > 0.1 set to 0;
                         B = 2 h c^2 wn^3 / expm1(h c wn / (k T)) from pb_common.h's constants;
                         cf = B[:-1] detau / dlogp, a zero last row, each column / its sum
  transit                exp(-depth[r]) for itop <= r < ideep, 1 for r < min(itop, ideep), 0 from
                         ideep on (an ideep outside [0, L] acts as the nearer end by itself)
  both                   a band's samples are start .. start + count intersected with [0, nwave),
                         the response indexed by the unclipped position; np.trapezoid over the
                         retained samples; each band / np.amax over the layers (NaN-propagating)

bound(case) is the project's own rule, from fixture G24: max(10 sens, 1e-14) absolute on the
max-normalised result, sens = the largest change of reference() when the depth it formed is
multiplied by 1 + 1e-13 r (r uniform in [-1, 1], seeded).  A case with sens > 1e-9 is refused.

Every case is built by case(): it evaluates the reference once (case['ref'], read-only), the
sensitivity, and asserts what keeps a branch decision from flipping under rounding:
  * no evaluated acc within 1e-9 maxdepth of maxdepth,
  * no detau within 1e-6 of 0.1,
  * case['peak'][w, b] says where band b's maximum is more than 1e-6 above every other layer --
    only there may a test assert that the reference's peak layer is the one that comes out as 1.0;
except the cases that sit on a decision EXACTLY (exact=True): dyadic inputs, so that the
arithmetic is exact in double and long double alike.

A case is a dict of read-only arrays; a response segment is preceded by GAP doubles that no band
reads (RESPONSE_FILL in a clean case)."""
import functools

import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps < 2e-19)

KH, KLS, KKB = 6.6260755e-27, 2.99792458e10, 1.380658e-16      # pb_common.h: kH, kLS, kKB
CHUNK = 256                      # samples per workgroup of the two band kernels (kBlock)
MAX_LAYERS = {'emission': 1024, 'transit': 2048}
GAP, RESPONSE_FILL = 2, 0.5
RJUP = 7.1492e9
_trapezoid = getattr(np, 'trapezoid', None) or np.trapz


# -------------------------------------------------------------------------------------------------
# the reference
# -------------------------------------------------------------------------------------------------
def emission_depth(c):
    """-> (depth[nw, L, W] long double, stop[nw, W], evaluated[nw, L, W]): the plane-parallel
    depth of every column, the layer at which it stopped, and which acc were formed."""
    ec, h = c['ec'].astype(LD), c['intervals'].astype(LD)
    nw, L, W = ec.shape
    itop, ibottom, maxdepth = c['itop'], c['ibottom'], LD(c['maxdepth'])
    depth = np.zeros((nw, L, W), LD)
    evaluated = np.zeros((nw, L, W), bool)
    stop = np.full((nw, W), L - 1, np.int64)
    acc = np.zeros((nw, W), LD)
    active = np.ones((nw, W), bool)
    with np.errstate(all='ignore'):
        for k in range(itop + 1, L):
            acc = acc + LD(0.5) * h[:, k - 1, None] * (ec[:, k] + ec[:, k - 1])
            depth[:, k] = np.where(active, acc, 0)
            evaluated[:, k] = active
            hit = active & ((acc >= maxdepth) | (k == ibottom) | (k == L - 1))
            stop[hit] = k
            active = active & ~hit
    return depth, stop, evaluated


def planck(wn, temps):
    """B[nw, L, W] in long double."""
    w = wn.astype(LD)[None, None, :]
    kt = LD(KKB) * temps.astype(LD)[:, :, None]
    with np.errstate(all='ignore'):
        return LD(2.0) * LD(KH) * LD(KLS) * LD(KLS) * w**3 / np.expm1(LD(KH) * LD(KLS) * w / kt)


def band_samples(c, b):
    """-> (grid columns g, positions i within the band) of the retained samples of band b."""
    i = np.arange(int(c['band_count'][b]), dtype=np.int64)
    g = int(c['band_start'][b]) + i
    keep = (g >= 0) & (g < c['W'])
    return g[keep], i[keep]


def evaluate(c, factor=None):
    """The reference with its intermediates -> dict(out[nw, L, nb] long double, raw (before the
    division by the maximum), detau, depth, stop, evaluated).  factor: multiplies the depth."""
    assert EXTENDED, 'np.longdouble is not an extended type here'
    nw, L, W = c['nw'], c['L'], c['W']
    res = {}
    with np.errstate(all='ignore'):
        if c['rt'] == 'emission':
            depth, res['stop'], res['evaluated'] = emission_depth(c)
            if factor is not None:
                depth = depth * factor
            detau = np.diff(np.exp(-depth), axis=1)
            detau[detau > LD(0.1)] = 0
            cf = planck(c['wn'], c['temps'])[:, :-1] * detau / c['dlogp'].astype(LD)[None, :, None]
            cf = np.concatenate([cf, np.zeros((nw, 1, W), LD)], axis=1)
            contrib = cf / np.sum(cf, axis=1, keepdims=True)
            res['detau'] = detau
        else:
            depth = c['depth'].astype(LD)
            if factor is not None:
                depth = depth * factor
            rows = np.arange(L)[None, :, None]
            ideep = c['ideep'].astype(np.int64)[:, None, :]
            contrib = np.exp(-depth)
            contrib = np.where(rows < c['itop'], LD(1), contrib)
            contrib = np.where(rows >= ideep, LD(0), contrib)
        res['depth'] = depth
        wn = c['wn'].astype(LD)
        raw = np.zeros((nw, L, c['nb']), LD)
        done = {}
        for b in range(c['nb']):
            key = (int(c['band_start'][b]), int(c['band_count'][b]), int(c['response_offset'][b]))
            if key not in done:
                g, i = band_samples(c, b)
                r = c['response'][int(c['response_offset'][b]) + i].astype(LD)
                done[key] = _trapezoid(contrib[:, :, g] * r, wn[g], axis=-1)
            raw[:, :, b] = done[key]
        res['raw'] = raw
        res['out'] = raw / np.amax(raw, axis=1, keepdims=True)
    return res


def reference(c):
    """-> [nw, L, nbands] float64, NaN where the reference is NaN."""
    return evaluate(c)['out'].astype(np.float64)


def bound(c):
    """max(10 sens, 1e-14): absolute, on the max-normalised result."""
    return max(10 * c['sens'], 1e-14)


def deviation(got, c):
    """Worst |got - ref| / bound(c) and its index; inf where the NaN patterns differ."""
    got, ref = np.asarray(got, np.float64), c['ref']
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0, None
    with np.errstate(all='ignore'):
        ratio = np.abs(got.astype(LD) - ref.astype(LD)) / LD(bound(c))
    both = np.isnan(got) & np.isnan(ref)
    ratio[both] = 0
    ratio[np.isnan(ratio)] = np.inf
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), tuple(int(i) for i in k)


# -------------------------------------------------------------------------------------------------
# construction
# -------------------------------------------------------------------------------------------------
def case(rt, wn, bands, itop, exact=False, max_band_count=None, seed=0, **inputs):
    """A checked, frozen case.  bands: (band_start, band_count, response, response_offset) of
    make_bands().  inputs -- emission: ec, intervals, dlogp, temps, maxdepth, ibottom; transit:
    depth, ideep."""
    assert rt in ('emission', 'transit')
    start, count, response, offset = bands
    c = dict(rt=rt, wn=np.array(wn, np.float64), itop=int(itop), exact=bool(exact), seed=seed,
             band_start=np.array(start, np.int32), band_count=np.array(count, np.int32),
             response=np.array(response, np.float64), response_offset=np.array(offset, np.int64))
    if rt == 'emission':
        c.update(ec=np.array(inputs.pop('ec'), np.float64, ndmin=3),
                 intervals=np.array(inputs.pop('intervals'), np.float64, ndmin=2),
                 dlogp=np.array(inputs.pop('dlogp'), np.float64),
                 temps=np.array(inputs.pop('temps'), np.float64, ndmin=2),
                 maxdepth=float(inputs.pop('maxdepth')), ibottom=int(inputs.pop('ibottom')))
        main = c['ec']
    else:
        c.update(depth=np.array(inputs.pop('depth'), np.float64, ndmin=3),
                 ideep=np.array(inputs.pop('ideep'), np.int32, ndmin=2))
        main = c['depth']
    assert not inputs, sorted(inputs)
    nw, L, W = main.shape
    nb = len(c['band_start'])
    c.update(nw=nw, L=L, W=W, nb=nb)
    assert c['wn'].shape == (W,) and np.all(np.diff(c['wn']) > 0)
    assert c['band_count'].shape == c['response_offset'].shape == (nb,)
    assert 0 <= c['itop'] < L and np.all(c['band_count'] >= 0)
    assert np.all(c['response_offset'] + c['band_count'] <= len(c['response']))
    if rt == 'emission':
        assert L >= 2 and c['intervals'].shape == (nw, L - 1) and c['dlogp'].shape == (L - 1,)
        assert c['temps'].shape == (nw, L) and c['ibottom'] <= L
    else:
        assert c['ideep'].shape == (nw, W)
    largest = int(c['band_count'].max()) if nb else 0
    c['max_band_count'] = largest if max_band_count is None else int(max_band_count)
    assert c['max_band_count'] >= largest
    # which response doubles a band reads
    used = np.zeros(len(c['response']), bool)
    for b in range(nb):
        _, i = band_samples(c, b)
        used[c['response_offset'][b] + i] = True
    c['response_used'] = used

    res = evaluate(c)
    out = res['out']
    c['ref'] = out.astype(np.float64)
    if rt == 'emission':
        c['stop'] = res['stop']
        md = LD(c['maxdepth'])
        if np.isfinite(c['maxdepth']) and not exact:
            acc = res['depth'][res['evaluated']]
            with np.errstate(invalid='ignore'):
                assert not np.any(np.abs(acc - md) < LD(1e-9) * md), 'an acc sits on maxdepth'
        with np.errstate(invalid='ignore'):
            assert not np.any(np.abs(res['detau'] - LD(0.1)) < 1e-6), 'a detau sits on 0.1'
    # the peak of every band: separated from the second layer's value?
    with np.errstate(all='ignore'):
        ordered = np.sort(np.where(np.isnan(out), -np.inf, out), axis=1)
        c['peak'] = ~np.isnan(out).any(axis=1) & (L >= 2) & \
            ((ordered[:, -1] - ordered[:, -2 if L >= 2 else -1]) > 1e-6)
    # the sensitivity, G24's
    shape = res['depth'].shape
    r = np.random.default_rng(2400 + seed).uniform(-1, 1, shape)
    moved = evaluate(c, factor=LD(1) + LD(1e-13) * r.astype(LD))['out']
    assert np.array_equal(np.isnan(moved), np.isnan(out)), 'the NaN pattern moves with the depth'
    diff = np.abs(moved - out)
    c['sens'] = float(np.max(diff[~np.isnan(diff)])) if np.any(~np.isnan(diff)) else 0.0
    if not c['sens'] <= 1e-9:
        raise ValueError(f'sensitivity {c["sens"]:.2e} > 1e-9: ill-conditioned, refused')
    return frozen(c)


def frozen(c):
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


INPUTS = {'emission': ('ec', 'intervals', 'dlogp', 'temps', 'maxdepth', 'ibottom'),
          'transit': ('depth', 'ideep')}


def modified(c, bands=None, **over):
    """The case with inputs replaced by name, built (and checked) anew."""
    kw = {k: c[k] for k in INPUTS[c['rt']]}
    kw.update(wn=c['wn'], itop=c['itop'], exact=c['exact'], seed=c['seed'])
    if bands is None:
        bands = (c['band_start'], c['band_count'], c['response'], c['response_offset'])
        kw['max_band_count'] = c['max_band_count']
    assert set(over) <= set(kw) | {'max_band_count'}, sorted(over)
    kw.update(over)
    return case(c['rt'], bands=bands, **kw)


def walker(c, w):
    """Walker w alone."""
    per_walker = ('ec', 'intervals', 'temps') if c['rt'] == 'emission' else ('depth', 'ideep')
    return modified(c, **{k: c[k][w:w + 1] for k in per_walker})


def one_band(c, b):
    """Band b alone (its own response segment; max_band_count = its count)."""
    o, n = int(c['response_offset'][b]), int(c['band_count'][b])
    return modified(c, bands=make_bands([(int(c['band_start'][b]), c['response'][o:o + n])]))


# -------------------------------------------------------------------------------------------------
# inputs
# -------------------------------------------------------------------------------------------------
def grid(W, seed):
    """Non-uniform, ascending (G24's)."""
    return 2000.0 + np.cumsum(np.random.default_rng(seed).uniform(0.4, 2.5, W))


def curve(count, rng):
    x = np.linspace(-1.0, 1.0, count) if count > 1 else np.zeros(count)
    return (0.2 + np.exp(-2.0 * x**2)) * rng.uniform(0.7, 1.3, count)


def make_bands(spans, seed=5):
    """spans: (start, count) -- a response curve of G24's kind is made -- or (start, response)
    -> (band_start, band_count, response, response_offset), GAP unread doubles before every
    segment and after the last."""
    rng = np.random.default_rng(seed)
    start, count, parts, offset, at = [], [], [], [], 0
    for s, r in spans:
        r = curve(r, rng) if np.isscalar(r) else np.asarray(r, float)
        parts += [np.full(GAP, RESPONSE_FILL), r]
        start.append(s)
        count.append(len(r))
        offset.append(at + GAP)
        at += GAP + len(r)
    parts.append(np.full(GAP, RESPONSE_FILL))
    return (np.array(start, np.int32), np.array(count, np.int32), np.concatenate(parts),
            np.array(offset, np.int64))


def g24_spans(W):
    """The bands of fixture G24 (counts 1, 2, 255, 256, 257, 513; two overlapping; from sample 0;
    to the last sample), clipped to the grid BEFORE the call as there, and the whole grid."""
    spans = [(5, 1), (9, 2), (3, 255), (7, 256), (11, 257), (13, 513), (40, 60), (70, 50), (0, 33),
             (W - 21, 21), (0, W)]
    return [(s, min(n, W - s)) for s, n in spans]


def small_spans(W):
    """For W = 70: counts 1, 2, 33, the whole grid, two overlapping, from 0, to the last."""
    return [(5, 1), (9, 2), (3, 33), (0, W), (20, 30), (40, 25), (0, 7), (W - 11, 11)]


def emission_inputs(L, W, nw, seed, lo=-2.5, hi=4.5):
    """G24's make_inputs: columns from transparent to opaque within a few layers, strengths (the
    depth of the whole column, roughly) over hi - lo decades; per walker its own temperatures,
    intervals and strengths."""
    rng = np.random.default_rng(seed)
    press = np.sort(np.logspace(-6, 2, L) * rng.uniform(0.9, 1.1, L))
    temps, intervals, ec = np.empty((nw, L)), np.empty((nw, L - 1)), np.empty((nw, L, W))
    for w in range(nw):
        t_top, t_bot = rng.uniform(700, 1100), rng.uniform(1500, 2300)
        temps[w] = np.linspace(t_top, t_bot, L) * rng.uniform(0.97, 1.03, L)
        intervals[w] = rng.uniform(0.5e7, 2.0e7, L - 1) * 40.0 / L
        strength = 10.0**rng.uniform(lo, hi, W) / np.sum(intervals[w])
        profile = (press / press[-1])**rng.uniform(0.15, 0.3)
        ec[w] = strength * profile[:, None] * rng.uniform(0.8, 1.2, (L, W))
    return dict(ec=ec, intervals=intervals, dlogp=np.diff(np.log(press)), temps=temps)


JUNK_ABOVE, JUNK_BELOW = 7.0, 3.0


def transit_inputs(L, W, nw, itop, seed, taumax=10.0):
    """depth and ideep of the kind pb_transit_spectrum_batch leaves: rising from 0 at itop,
    ideep the first row above taumax, else the last row.  The rows the header says are not read
    (above itop; from ideep on) hold JUNK, not 0."""
    rng = np.random.default_rng(seed)
    depth = np.empty((nw, L, W))
    ideep = np.empty((nw, W), np.int32)
    rows = np.arange(L)
    for w in range(nw):
        strength = 10.0**rng.uniform(-4.0, 3.0, W)
        x = np.clip((rows - itop) / max(L - 1 - itop, 1), 0.0, 1.0)**rng.uniform(1.5, 2.5)
        d = strength * x[:, None] * rng.uniform(0.8, 1.2, (L, W))
        deep = (d > taumax) & (rows >= itop)[:, None]
        ideep[w] = np.where(deep.any(axis=0), np.argmax(deep, axis=0), L - 1)
        d[rows < itop] = JUNK_ABOVE
        d[rows[:, None] >= ideep[w][None, :]] = JUNK_BELOW
        depth[w] = d
    return dict(depth=depth, ideep=ideep)


# -------------------------------------------------------------------------------------------------
# the cases (built once per process)
# -------------------------------------------------------------------------------------------------
GEOMETRIES = ('emission', 'two_stream', 'transit')


def itops(L):
    """itop in {0, 2, L - 2, L - 1}, those that exist."""
    return sorted({i for i in (0, 2, L - 2, L - 1) if 0 <= i < L})


@functools.lru_cache(maxsize=None)
def shape_case(geometry, L, W, nw, itop, ibottom=None, maxdepth=None, spans='auto', seed=None,
               lo=-2.5, hi=4.5, max_factor=1):
    """A random case of the geometry ('two_stream': the emission entry with maxdepth = inf)."""
    if seed is None:
        seed = 1000 * L + W + 7 * itop + 500000 * (geometry == 'two_stream')
    if spans == 'auto':
        spans = small_spans(W) if W < 600 else g24_spans(W)
    bands = make_bands(list(spans), seed=seed + 1)
    mbc = None if max_factor == 1 else max_factor * int(bands[1].max())
    wn = grid(W, seed + 2)
    if geometry == 'transit':
        return case('transit', wn, bands, itop, seed=seed, max_band_count=mbc,
                    **transit_inputs(L, W, nw, itop, seed + 3))
    if maxdepth is None:
        maxdepth = np.inf if geometry == 'two_stream' else 10.0
    return case('emission', wn, bands, itop, seed=seed, max_band_count=mbc, maxdepth=maxdepth,
                ibottom=L if ibottom is None else ibottom,
                **emission_inputs(L, W, nw, seed + 3, lo, hi))


@functools.lru_cache(maxsize=None)
def small_maxdepth_case(L=257, W=70, nw=1, seed=77):
    """G24's e_md at L layers: maxdepth = 0.105; a jump back to depth 0 is kept only where a
    column stops with 0.105 <= tau <= -log(0.9) = 0.10536, so every 7th column is scaled to reach
    0.1052 at a layer of its own; the others stop higher and lose their jump."""
    kw = emission_inputs(L, W, nw, seed, lo=-3.0, hi=1.0)
    ec = kw['ec']
    probe = dict(ec=ec, intervals=kw['intervals'], itop=0, ibottom=L, maxdepth=np.inf)
    full = emission_depth(probe)[0].astype(np.float64)
    for w in range(nw):
        for j in range(0, W, 7):
            k = 2 + (37 * (j // 7)) % (L - 3)
            ec[w][:, j] *= 0.1052 / full[w, k, j]
    return case('emission', grid(W, seed + 2), make_bands(small_spans(W), seed + 1), 0, seed=seed,
                maxdepth=0.105, ibottom=L, **kw)


@functools.lru_cache(maxsize=None)
def equality_case(twin, L=8, W=70, nw=1, seed=88):
    """The stop rule at equality, exactly: ec = 2^-20 in every layer, intervals powers of two, so
    acc = 1, 3, 4, 8, ... without rounding; maxdepth = acc at layer 3 = 4 (the column stops at
    layer 3); the twin has maxdepth = nextafter(4, inf) and stops one layer later."""
    intervals = np.tile(2.0**np.array([20, 21, 20, 22] + [21] * (L - 5)), (nw, 1))
    rng = np.random.default_rng(seed)
    temps = np.tile(np.linspace(900.0, 1900.0, L), (nw, 1))
    press = np.logspace(-6, 2, L)
    return case('emission', grid(W, seed + 2), make_bands(small_spans(W), seed + 1), 0, exact=True,
                seed=seed, ec=np.full((nw, L, W), 2.0**-20), intervals=intervals,
                dlogp=np.diff(np.log(press)), temps=temps * rng.uniform(0.99, 1.01, (nw, L)),
                maxdepth=np.nextafter(4.0, np.inf) if twin else 4.0, ibottom=L)


# clipped bands on a grid of W samples: name -> ((start, count), retained samples)
def clipped_spans(W):
    return {
        'past_end_5': ((W - 5, 9), 5), 'past_end_1': ((W - 1, 4), 1), 'past_end_0': ((W + 2, 3), 0),
        'at_end_0': ((W, 3), 0),
        'before_start_5': ((-4, 9), 5), 'before_start_1': ((-3, 4), 1),
        'before_start_0': ((-7, 5), 0),
        'whole_and_more': ((-10, W + 25), W),
        'seam_past_end': ((W - 300, 513), 300), 'seam_before_start': ((-213, 513), 300),
        'inside': ((40, 60), 60),
    }


@functools.lru_cache(maxsize=None)
def clipped_case(geometry, L=5, W=600, nw=2, seed=99):
    spans = tuple(s for s, _ in clipped_spans(W).values())
    return shape_case(geometry, L, W, nw, 0, spans=spans, seed=seed)


def sliced_case(c):
    """The clipped case's bands with >= 2 retained samples, each passed as the in-grid band of its
    retained samples with the sliced response -> (case, the bands' indices in c)."""
    spans, which = [], []
    for b in range(c['nb']):
        g, i = band_samples(c, b)
        if len(g) >= 2:
            spans.append((int(g[0]), c['response'][int(c['response_offset'][b]) + i]))
            which.append(b)
    return modified(c, bands=make_bands(spans)), which


@functools.lru_cache(maxsize=None)
def limit_case(geometry, what):
    """L = 2, W = 2, every band the two samples; what = 'bands': 65535 bands (their responses
    windows into one pool) x 1 walker; 'walkers': 1 band x 65535 walkers."""
    n = 65535
    nb, nw = (n, 1) if what == 'bands' else (1, n)
    rng = np.random.default_rng(65535 + (what == 'bands'))
    pool = rng.uniform(0.2, 1.2, 66)
    bands = (np.zeros(nb, np.int32), np.full(nb, 2, np.int32), pool,
             (np.arange(nb) % 64).astype(np.int64))
    wn = np.array([2000.0, 2001.3])
    if geometry == 'transit':
        depth = 10.0**rng.uniform(-3.0, 1.0, (nw, 2, 2))
        ideep = rng.integers(1, 3, (nw, 2)).astype(np.int32)
        ideep[:, 0] = 2                             # (one column at least reaches the last row)
        return case('transit', wn, bands, 0, seed=n, depth=depth, ideep=ideep)
    return case('emission', wn, bands, 0, seed=n,
                ec=10.0**rng.uniform(-9.0, -6.0, (nw, 2, 2)),
                intervals=rng.uniform(0.5e7, 2.0e7, (nw, 1)), dlogp=np.array([1.7]),
                temps=rng.uniform(700.0, 2300.0, (nw, 2)),
                maxdepth=np.inf if geometry == 'two_stream' else 10.0, ibottom=2)
