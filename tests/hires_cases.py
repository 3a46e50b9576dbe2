"""Cases and a plain high-precision reference for the high-resolution exit (csrc/pb_hires.hip:
pb_inst_convolve_batch, pb_hires_observe_batch).  NumPy only: no GPU, no torch, no SciPy.

reference() is written out from the definition in include/pbhip.h,
    s    = spectra[w] [* walker_scale[w]] [* sample_scale]          (float64, in that order)
    c[i] = sum_t taps[t] s[i + H - t],  H = (T - 1) / 2, s = 0 outside [0, W)    (mode='same')
    x    = wn * sqrt((1 - v/c) / (1 + v/c))                   (float64, the kernel's constants)
    out  = (c[hi] - c[lo]) / (x[hi] - x[lo]) * (d - x[lo]) + c[lo],
           hi = searchsorted(x, d, 'left') clipped to [1, W - 1], lo = hi - 1
with the sum and the interpolation formula in np.longdouble (64-bit mantissa: x87 extended; the
import asserts it -- THE LONG DOUBLE FORM IS THE ONE THAT RAN, on the build host and on the GPU
host; an error-free two-product + math.fsum form, the alternative for a host without an extended
type, was not needed and is not implemented).  The samples
s and the nodes x are inputs of the sum and of the interpolation: their float64 roundings belong
to the operation, not to the error.  The definition holds for T > W (an output of W samples),
where np.convolve(mode='same') returns T samples.

bound[w, j] = (T + 8) 2^-53 max(conv_mag[lo], conv_mag[lo + 1]), conv_mag[i] = sum_t |taps[t]
s[i + H - t]|: the worst-case rounding of a T-term FMA chain (T 2^-53 conv_mag per sample; the
result is a convex combination of two samples) plus a few roundings for the two differences, the
quotient, the product and the final sum.  Derived, not measured.  For the convolved samples
themselves the bound is (T + 2) 2^-53 conv_mag (conv_bound()).

A walker is rejected (+inf in its row, bound 0, lo -1) when not |rv| <= rv_max, or when
data.min() < x[0] or data.max() > x[-1].

The case builders return plain dicts of read-only arrays.  That the layouts are the situations
they are named after is asserted in test_hires_cases_cpu.py on reference()'s `lo` alone."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'np.longdouble is not an extended type here'

C_LIGHT, KM = 29979245800.0, 1.0e5      # the kernel's kC, kKm = the reference's pc.c, pc.km
TILE = 1023                             # brackets per workgroup of k_hires_observe (kOut - 1)
CONV_TILE = 1024                        # outputs per workgroup of k_inst_convolve (kOut)
SPARSE_MAX = 256                        # needed samples up to which a tile runs conv_one
MAX_TAPS = 1025
RV_MAX = 20.0
EPS = LD(2.0)**-53


def doppler_factor(v):
    """The kernel's f of one walker: every operation a float64 operation, in its order."""
    vel = np.float64(v) * np.float64(KM)
    with np.errstate(all='ignore'):
        return np.sqrt((np.float64(1.0) - vel / np.float64(C_LIGHT)) /
                       (np.float64(1.0) + vel / np.float64(C_LIGHT)))


def shifted(wn, v):
    return np.asarray(wn, np.float64) * doppler_factor(v)


def samples(spectra, sample_scale=None, walker_scale=None):
    """s[nw, W] in float64: row * walker_scale, then * sample_scale[p] (the kernel's order)."""
    s = np.array(spectra, np.float64, ndmin=2)
    with np.errstate(all='ignore'):
        if walker_scale is not None:
            s = s * np.asarray(walker_scale, np.float64)[:, None]
        if sample_scale is not None:
            s = s * np.asarray(sample_scale, np.float64)[None, :]
    return s


def convolve(s, taps):
    """(conv, conv_mag)[nw, W] in long double from the definition, term by term in t."""
    nw, W = s.shape
    taps = np.asarray(taps, np.float64)
    T = len(taps)
    assert T % 2 == 1
    H = (T - 1) // 2
    padded = np.zeros((nw, W + 2 * H), LD)
    padded[:, H:H + W] = s
    k = taps.astype(LD)
    conv, mag = np.zeros((nw, W), LD), np.zeros((nw, W), LD)
    with np.errstate(all='ignore'):
        for t in range(T):
            term = k[t] * padded[:, 2 * H - t:2 * H - t + W]        # s[i + H - t]
            conv += term
            mag += np.abs(term)
    return conv, mag


def conv_bound(conv_mag, T):
    return LD(T + 2) * EPS * conv_mag


def reference(spectra, wn, taps, data_wn, rv, sample_scale=None, walker_scale=None,
              rv_max=RV_MAX):
    """-> (out[nw, ndata], bound[nw, ndata], conv[nw, W], conv_mag[nw, W], lo[nw, ndata]): the
    first four in long double, lo int64; out in the order of data_wn (any order)."""
    wn = np.asarray(wn, np.float64)
    d = np.asarray(data_wn, np.float64)
    s = samples(spectra, sample_scale, walker_scale)
    nw, W = s.shape
    assert wn.shape == (W,) and W >= 2 and d.ndim == 1 and d.size >= 1
    T = len(taps)
    rv = np.zeros(nw) if rv is None else np.asarray(rv, np.float64)
    assert rv.shape == (nw,)
    conv, mag = convolve(s, taps)
    out = np.full((nw, len(d)), np.inf, LD)
    bound = np.zeros((nw, len(d)), LD)
    lo_all = np.full((nw, len(d)), -1, np.int64)
    dl = d.astype(LD)
    # walkers of equal rv (equal bits) share their nodes and brackets
    for bits in np.unique(rv.view(np.int64)):
        rows = np.flatnonzero(rv.view(np.int64) == bits)
        v = rv[rows[0]]
        if not abs(v) <= rv_max:
            continue
        x = wn * doppler_factor(v)
        if d.min() < x[0] or d.max() > x[-1]:
            continue
        hi = np.clip(np.searchsorted(x, d, side='left'), 1, W - 1)
        lo = hi - 1
        xl = x.astype(LD)
        with np.errstate(all='ignore'):
            c = conv[rows]
            out[rows] = (c[:, hi] - c[:, lo]) / (xl[hi] - xl[lo]) * (dl - xl[lo]) + c[:, lo]
            m = mag[rows]
            bound[rows] = LD(T + 8) * EPS * np.maximum(m[:, lo], m[:, hi])
        lo_all[rows] = lo
    return out, bound, conv, mag, lo_all


def deviation(got, ref, bound):
    """Worst |got - ref| / bound and its index.  Where bound == 0 the two values must be equal
    (ratio 0, else inf); +inf = +inf counts as equal anywhere; any other non-finite difference is
    inf."""
    got = np.asarray(got, np.float64)
    ref, bound = np.asarray(ref, LD), np.asarray(bound, LD)
    assert got.shape == ref.shape == bound.shape
    if got.size == 0:
        return 0.0, None
    with np.errstate(all='ignore'):
        ratio = np.abs(got.astype(LD) - ref) / bound
    same = got.astype(LD) == ref
    ratio[same] = 0
    ratio[~same & ~(bound > 0)] = np.inf
    ratio[np.isnan(ratio)] = np.inf
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), tuple(int(i) for i in k)


def frozen(**arrays):
    out = {}
    for name, a in arrays.items():
        if isinstance(a, np.ndarray):
            a = a.copy()
            a.flags.writeable = False
        out[name] = a
    return out


# -------------------------------------------------------------------------------------------------
# grids, taps, spectra
# -------------------------------------------------------------------------------------------------
def grid(kind, W):
    """'resolution': constant resolving power, ratio 1 + 1/123300 from 4000 cm-1 (2.43 km/s per
    node); 'step': constant 0.05 cm-1 from 6000 cm-1 (2.5 km/s per node at its low end)."""
    if kind == 'resolution':
        return 4000.0 * (1.0 + 1.0 / 123300.0)**np.arange(W)
    assert kind == 'step'
    return 6000.0 + 0.05 * np.arange(W)


def make_taps(kind, T, at=None):
    """'gaussian': normalised, sigma = T / 6; 'signed': that Gaussian times a cosine of period 7.3
    samples and phase 0.6 (signed AND asymmetric: c[i] is not what the mirrored taps give);
    'unit': a single 1 at index `at` (default H // 2: off the centre for T >= 3), zeros elsewhere,
    so c[i] = s[i + H - at] exactly."""
    assert T % 2 == 1 and T >= 1
    H = (T - 1) // 2
    x = np.arange(T) - float(H)
    if kind == 'unit':
        k = np.zeros(T)
        k[H // 2 if at is None else at] = 1.0
        return k
    k = np.exp(-0.5 * (x / max(T / 6.0, 0.5))**2)
    if kind == 'signed':
        k = k * np.cos(2.0 * np.pi * x / 7.3 + 0.6)
        return k / np.sum(np.abs(k))
    assert kind == 'gaussian'
    return k / np.sum(k)


def make_spectra(kind, nw, W, seed):
    """'positive': ~1e-2 (a transit depth with structure); 'mixed': both signs, ~1e-2."""
    rng = np.random.default_rng(seed)
    if kind == 'positive':
        return 1.0e-2 * (1.0 + 0.3 * rng.uniform(size=(nw, W)) +
                         0.2 * np.sin(np.arange(W) / 9.0)[None, :] * rng.uniform(size=(nw, 1)))
    assert kind == 'mixed'
    return 1.0e-2 * rng.standard_normal((nw, W))


def tiles(W):
    """Number of workgroups of k_hires_observe per walker."""
    return -(-(W - 1) // TILE)


def seams(W):
    """Nodes 1023 b, b >= 1, that separate two tiles."""
    return [TILE * b for b in range(1, tiles(W))]


# -------------------------------------------------------------------------------------------------
# data layouts: ascending data for a grid and the walkers' rv
# -------------------------------------------------------------------------------------------------
def on_every_node(wn, rvs):
    """Every shifted node wn * f (the same float64 product as the kernel's) of every rv, and the
    midpoints of its brackets -- those inside every walker's shifted grid (for one rv: all of
    them, both ends included)."""
    rvs = np.atleast_1d(np.asarray(rvs, np.float64))
    xs = [shifted(wn, v) for v in rvs]
    low, high = max(x[0] for x in xs), min(x[-1] for x in xs)
    pts = np.concatenate([np.concatenate([x, 0.5 * (x[:-1] + x[1:])]) for x in xs])
    return np.sort(pts[(pts >= low) & (pts <= high)])


def bracket_point(wn, bracket, frac=0.5):
    """A point of the grid at rest inside bracket `bracket`, away from its ends: walkers whose
    grid is shifted by less than min(frac, 1 - frac) of a node keep it in that bracket."""
    return wn[bracket] + frac * (wn[bracket + 1] - wn[bracket])


def one_per_tile(wn, empty):
    """A single point in the middle of every tile except tile `empty`."""
    nt = tiles(len(wn))
    assert nt >= 3 and 0 <= empty < nt
    pts = []
    for b in range(nt):
        if b != empty:
            g0, g1 = TILE * b, min(TILE * (b + 1), len(wn) - 1)
            pts.append(bracket_point(wn, (g0 + g1) // 2))
    return np.array(pts)


def threshold(wn, extra=True):
    """Tile 0: the brackets 0, 3, ..., 381 (128 pairwise disjoint: 256 needed samples).  Tile 1:
    the brackets 1023 + 0, 3, ..., 381 and, with `extra`, bracket 1023 + 1, which shares node
    1023 + 1 with its neighbour: 257 needed samples.  -> (data, index of the extra point)."""
    assert tiles(len(wn)) >= 2 and len(wn) - 1 >= TILE + 383
    first = [bracket_point(wn, 3 * k) for k in range(128)]
    second = [bracket_point(wn, TILE + 3 * k) for k in range(128)]
    if extra:
        second.insert(1, bracket_point(wn, TILE + 1))
    data = np.array(first + second)
    assert np.all(np.diff(data) > 0)
    return data, 129


def crowd(wn, rv, bracket=0, n=3000, nequal=500, seed=0):
    """n points in one bracket of the grid shifted by rv: its two nodes, nequal equal points, the
    rest anywhere inside.  (A point on a bracket's lower node belongs to the bracket below unless
    that node is the grid's first: only in bracket 0 do all n share one bracket.)"""
    x = shifted(wn, rv)
    a, b = x[bracket], x[bracket + 1]
    rng = np.random.default_rng(seed)
    inside = a + (b - a) * rng.uniform(0.01, 0.99, n - 2 - nequal)
    return np.sort(np.concatenate([[a, b], np.full(nequal, a + 0.37 * (b - a)), inside]))


def single(wn, bracket):
    return np.array([bracket_point(wn, bracket)])


def slots(kind, data, seed=0):
    """-> (slot[ndata] int32, caller[ndata]) with caller[slot[j]] = data[j] (data ascending).
    'identity', 'reversed', 'random' (a seeded permutation), 'argsort' (the data shuffled by the
    caller, sorted by a stable argsort: what HiresData makes)."""
    n = len(data)
    rng = np.random.default_rng(seed)
    if kind == 'identity':
        slot = np.arange(n)
    elif kind == 'reversed':
        slot = np.arange(n)[::-1].copy()
    elif kind == 'random':
        slot = rng.permutation(n)
    else:
        assert kind == 'argsort'
        shuffled = data[rng.permutation(n)]
        slot = np.argsort(shuffled, kind='stable')
        assert np.array_equal(shuffled[slot], data)
    caller = np.empty(n)
    caller[slot] = data
    return slot.astype(np.int32), caller


# -------------------------------------------------------------------------------------------------
# cases
# -------------------------------------------------------------------------------------------------
RVS = (0.0, 0.7, -0.4)      # km/s: less than a third of a node either way on both grids


def case(wn, taps, spectra, data, rv, slot_kind='random', sample_scale=False, walker_scale=False,
         rv_max=RV_MAX, seed=0):
    """A launch of pb_hires_observe_batch: data ascending, slot / caller from slots()."""
    wn, data = np.asarray(wn, np.float64), np.asarray(data, np.float64)
    spectra = np.array(spectra, np.float64, ndmin=2)
    nw, W = spectra.shape
    assert np.all(np.diff(data) >= 0) and wn.shape == (W,)
    rng = np.random.default_rng(1000 + seed)
    slot, caller = slots(slot_kind, data, seed)
    return frozen(
        wn=wn, taps=np.asarray(taps, np.float64), spectra=spectra, data_wn=data, slot=slot,
        caller=caller, rv=np.asarray(rv, np.float64),
        sample_scale=rng.uniform(0.5, 2.0, W) if sample_scale is True else
        (None if sample_scale is False else np.asarray(sample_scale, np.float64)),
        walker_scale=rng.uniform(0.7, 1.0, nw) if walker_scale is True else
        (None if walker_scale is False else np.asarray(walker_scale, np.float64)),
        rv_max=float(rv_max), nw=nw, W=W, T=len(taps), ndata=len(data))


def modified(c, **kw):
    """The case with some entries replaced (not the data: their slots belong to them)."""
    assert 'data_wn' not in kw
    d = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    d.update(kw)
    d['spectra'] = np.array(d['spectra'], np.float64, ndmin=2)
    d.update(nw=d['spectra'].shape[0], W=d['spectra'].shape[1], T=len(d['taps']),
             ndata=len(d['data_wn']))
    return frozen(**d)


def case_reference(c):
    """reference() of a case, out in the CALLER's order: out[w, slot[j]] belongs to data_wn[j]."""
    return reference(c['spectra'], c['wn'], c['taps'], c['caller'], c['rv'], c['sample_scale'],
                     c['walker_scale'], c['rv_max'])


def shape_case(W, T, grid_kind='resolution', taps_kind='gaussian', spectrum_kind='positive',
               sample_scale=False, walker_scale=False):
    """The observe shape (W, T): three walkers at RVS, data on every node, a random permutation."""
    wn = grid(grid_kind, W)
    seed = 7 * W + T
    return case(wn, make_taps(taps_kind, T), make_spectra(spectrum_kind, len(RVS), W, seed),
                on_every_node(wn, RVS), RVS, 'random', sample_scale, walker_scale, seed=seed)


def layout_case(name, T, **kw):
    """The layouts of the issue at their W: 'one_per_tile' (W = 3070, empty=...), 'threshold'
    (W = 2100, extra=...), 'crowd' and 'single' (W = 1025, bracket=...)."""
    seed = {'one_per_tile': 1, 'threshold': 2, 'crowd': 3, 'single': 4}[name] * 10000 + T
    rv = RVS
    if name == 'one_per_tile':
        wn = grid('resolution', 3070)
        data, slot_kind = one_per_tile(wn, kw.get('empty', 1)), 'reversed'
    elif name == 'threshold':
        wn = grid('resolution', 2100)
        data, slot_kind = threshold(wn, kw.get('extra', True))[0], 'argsort'
    elif name == 'crowd':
        wn = grid('resolution', 1025)
        rv = (0.7, 0.7, 0.7)
        data, slot_kind = crowd(wn, 0.7, kw.get('bracket', 0), seed=seed), 'argsort'
    else:
        assert name == 'single'
        wn = grid('resolution', 1025)
        data, slot_kind = single(wn, kw.get('bracket', TILE)), 'identity'
    W = len(wn)
    return case(wn, make_taps('gaussian', T), make_spectra('positive', 3, W, seed), data, rv,
                slot_kind, sample_scale=True, walker_scale=(T == 1), seed=seed)


def needed_samples(lo, tile):
    """The distinct convolved samples that the points of tile `tile` bracket (lo[ndata] of one
    walker)."""
    mine = lo[(lo >= TILE * tile) & (lo < TILE * (tile + 1))]
    return np.union1d(mine, mine + 1)
