"""The two-stream walker batch (k_two_stream_batch: plane-parallel optical depth without a stop +
diffusivity transmissions + both sweeps of a batch of walkers in one pass) through the C ABI --
pb_two_stream_batch -- against the oracle chain plane_parallel_optical_depth(maxdepth = inf) ->
two_stream (1e-11 of the column's largest flux: RTOL_TIGHT / close_by_column of
test_two_stream.py, the RTOL of test_gpu_batch_emission.py), and bit for bit against the
single-spectrum kernels run one after the other per walker.

Inputs are this module's own (cases.column_case has transparent columns and dtau down to 1e-12,
where the reference's formula is ill-conditioned: docstring of test_two_stream.py).  Per walker
every interval gets a target optical depth 10**U(-3, 0.7) and ec is solved from it row by row; a
target that would make the next row non-positive is re-drawn from the same distribution above
that limit (what rejection gives, in bounded time).  The first interval of every walker is a power
of two, so that 0.5 h (ec[1] + ec[0]) IS the target there: depth[0] = 0 makes that interval's
dtau0 the increment itself, and the first columns hold exactly 1 (the boundary between exp1's
series and its continued fraction), its two neighbours, 80, 40 and 4 (where the continued
fraction's 20 + int(80 / x) terms change), 1e-3, and 1e3 (exp(-dtau0) underflows).  Behind a
thick first interval no target of the distribution keeps ec positive; the column then takes
1.05 ... 2 times the limit (only those few columns pass a total depth of 200).

With a single interval (L = 2) the column's largest flux is the thin layer's own emission,
~pi B dtau0, while Bp = dB / dtau0 multiplies a bracket that a 1-ulp difference between two exp()
implementations moves by eps: an error of eps / dtau0**2 * dB / B relative to that flux, 2e-10 at
dtau0 = 1e-3 for the 1000 K between the two layers of the emission test's walkers (the CPU check
below found 4e-11 between the oracle and NumPy there).  The two layers of an L = 2 walker are
therefore within 5e-4 of each other in temperature (dB / B < 1e-2: 2e-12); every other shape
has the walkers' profiles as they are, and there the layers below a thin one carry the flux.

Before any GPU run, test_inputs_are_conditioned shows on the CPU that the oracle agrees with the
NumPy restatement using scipy.special.exp1 to 1e-11 on exactly these inputs."""
import functools

import numpy as np
import pytest

import cases

RTOL = 1e-11
SHAPES = [(1, 1), (2, 1), (2, 63), (5, 70), (17, 256), (33, 257), (33, 515)]
FIRST = [1.0, 0.999999, 1.000001, 80.0, 40.0, 4.0, 1e-3, 1e3]
SOURCES = ['both', 'none', 'f_int', 'flux_top']


def numpy_two_stream(depth, B, f_int, top):
    """The reference's statements, with scipy's exp1 (copied from test_two_stream.py)."""
    from scipy.special import exp1
    L = depth.shape[0]
    dtau0 = np.diff(depth, n=1, axis=0)
    trans = (1 - dtau0) * np.exp(-dtau0) + dtau0**2 * exp1(dtau0)
    Bp = np.diff(B, n=1, axis=0) / dtau0
    down = np.zeros_like(depth)
    up = np.zeros_like(depth)
    if top is not None:
        down[0] = top
    for i in range(L - 1):
        down[i + 1] = (trans[i] * down[i] + np.pi * B[i] * (1 - trans[i])
                       + np.pi * Bp[i] * (-2 / 3 * (1 - np.exp(-dtau0[i]))
                                          + dtau0[i] * (1 - trans[i] / 3)))
    up[L - 1] = down[L - 1] + f_int
    for i in reversed(range(L - 1)):
        up[i] = (trans[i] * up[i + 1] + np.pi * B[i + 1] * (1 - trans[i])
                 + np.pi * Bp[i] * (2 / 3 * (1 - np.exp(-dtau0[i]))
                                    - dtau0[i] * (1 - trans[i] / 3)))
    return down, up


def close_by_column(got, want, rtol, scale=None):
    """|got - want| <= rtol * (largest value of the column)."""
    if scale is None:
        scale = np.max(np.abs(want), axis=0)
    scale = np.where(scale > 0, scale, 1.0)      # (a column of zeros: absolute)
    assert np.all(np.isfinite(got))
    err = np.max(np.abs(got - want) / scale)
    assert err <= rtol, err
    return err


def solve_ec(rng, h, W):
    """ec[L, W] of one walker from per-interval target depths (module docstring)."""
    L = len(h) + 1
    lo_t, hi_t = -3.0, 0.7
    ec = np.empty((L, W))
    if L == 1:
        ec[0] = 10.0**rng.uniform(-14, -9, W)
        return ec
    target = 10.0**rng.uniform(lo_t, hi_t, (L - 1, W))
    n = min(W, len(FIRST))
    target[0, :n] = FIRST[:n]
    ec[0] = target[0] / h[0]
    for i in range(L - 1):
        # ec[i + 1] = 2 target / h[i] - ec[i] > 0  <=>  target > 0.5 h[i] ec[i]
        floor = 0.5 * h[i] * ec[i] * (1 + 1e-6)
        bad = target[i] <= floor
        if i == 0:
            assert not bad.any()                 # (ec[1] = ec[0]: half the target each)
        redraw = bad & (floor < 10.0**hi_t * 0.99)
        lo = np.log10(np.maximum(floor[redraw], 10.0**lo_t))
        target[i, redraw] = 10.0**(lo + (hi_t - lo) * rng.uniform(0, 1, redraw.sum()))
        thick = bad & ~redraw
        target[i, thick] = floor[thick] * rng.uniform(1.05, 2.0, thick.sum())
        ec[i + 1] = 2 * target[i] / h[i] - ec[i]
    assert np.all(ec > 0)
    return ec


@functools.lru_cache(maxsize=None)
def case(L, W, nw):
    """ec[nw, L, W], intervals[nw, L - 1], temps[nw, L] (every walker its own radius profile and
    temperatures, as test_gpu_batch_emission.walkers makes them), wn[W], f_int[W], flux_top[W]
    (as test_two_stream.conditioned_case makes them).  Cached: no test writes to them."""
    seed = 7000 + 100 * L + W + nw
    rng = np.random.default_rng(seed)
    c = cases.column_case(seed=seed, nlayers=L, nwave=W)
    radius = np.array([np.sort(c['radius'] * (1 + 0.01 * rng.uniform(-1, 1)))[::-1]
                       for _ in range(nw)])
    intervals = np.ascontiguousarray(-np.diff(radius, axis=1))
    if L > 1:
        intervals[:, 0] = 2.0**np.round(np.log2(intervals[:, 0]))
    temps = c['temp'][None] * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))) + rng.uniform(-20, 20, (nw, L))
    if L == 2:
        # (a single interval: module docstring)
        temps[:, 1] = temps[:, 0] * (1 + 5e-4 * rng.uniform(-1, 1, nw))
    ecs = np.array([solve_ec(rng, intervals[w], W) for w in range(nw)])
    f_int = 10**rng.uniform(0, 2, W)
    top = 10**rng.uniform(2, 4, W)
    return ecs, intervals, temps, c['wn'], f_int, top


def oracle_depth(orc, ec, h):
    L, W = ec.shape
    depth = np.zeros((L, W))
    stop = np.zeros(W, np.int32)
    orc.plane_parallel_optical_depth(depth, stop, np.ascontiguousarray(ec), h, np.inf, 0, L)
    return depth


_ORACLE = {}


def oracle(orc, L, W, nw, sources):
    """(depth[nw, L, W], flux_up[nw, L, W]) of the oracle chain, computed once per case."""
    key = (L, W, nw, sources)
    if key not in _ORACLE:
        ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
        fi = f_int if sources in ('both', 'f_int') else np.zeros(W)
        ft = top if sources in ('both', 'flux_top') else None
        depths = np.array([oracle_depth(orc, ecs[w], intervals[w]) for w in range(nw)])
        ups = np.array([orc.two_stream(depths[w], wn, temps[w], fi, ft, 0)[1] for w in range(nw)])
        _ORACLE[key] = (depths, ups)
    return _ORACLE[key]


@pytest.mark.parametrize('L,W', SHAPES)
def test_inputs_are_conditioned(orc, L, W):
    """CPU: on these inputs the oracle's two_stream is the reference's statements with
    scipy.special.exp1 to 1e-11, both sweeps, every layer; and the first interval holds the
    special values exactly."""
    nw = 5
    ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
    depths, _ = oracle(orc, L, W, nw, 'both')
    for w in range(nw):
        if L > 1:
            n = min(W, len(FIRST))
            assert np.array_equal(depths[w, 1, :n], FIRST[:n])
            assert np.all(np.diff(depths[w], axis=0) > 0)
        for fi, ft in ((f_int, top), (np.zeros(W), None)):
            got = orc.two_stream(depths[w], wn, temps[w], fi, ft, 0)
            want = numpy_two_stream(depths[w], orc.blackbody_wn_2D(wn, temps[w]), fi, ft)
            close_by_column(got[0], want[0], RTOL)
            close_by_column(got[1], want[1], RTOL)
    # the distribution's promise: but for the columns behind a thick first interval, the total
    # depth stays below about 200
    if L > 1:
        thin = np.ones(W, bool)
        thin[[i for i, v in enumerate(FIRST[:W]) if v > 5.02]] = False
        assert depths[:, -1, thin].max() < 200.0


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def run_batch(eng, ecs, intervals, temps, wn, f_int, top, **kw):
    """engine.two_stream_batch on host arrays (ec is a fresh device copy: the call consumes it);
    the output starts as NaN (a column the kernel does not write shows)."""
    import torch
    nw, _, W = ecs.shape
    if 'out' not in kw:
        kw['out'] = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
    return eng.two_stream_batch(eng.dev(ecs), eng.dev(intervals), eng.dev(wn), eng.dev(temps),
                                None if f_int is None else eng.dev(f_int),
                                None if top is None else eng.dev(top), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('nw', [1, 5])
@pytest.mark.parametrize('L,W', SHAPES)
def test_shapes(eng, orc, L, W, nw):
    """No interval (flux_top + f_int); one interval; less than a wavefront; exactly one and more
    than one workgroup of 256 columns; a ragged last workgroup -- each with and without the
    internal flux and the irradiation."""
    ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
    for sources in SOURCES:
        _, ups = oracle(orc, L, W, nw, sources)
        got = host(run_batch(eng, ecs, intervals, temps, wn,
                             f_int if sources in ('both', 'f_int') else None,
                             top if sources in ('both', 'flux_top') else None))
        for w in range(nw):
            assert np.all(np.isfinite(ups[w]))
            err = close_by_column(got[w], ups[w, 0], RTOL, np.max(np.abs(ups[w]), axis=0))
            print(f'L={L} W={W} nw={nw} {sources} walker {w}: {err:.2e}')
        if L == 1:
            want = (f_int if sources in ('both', 'f_int') else 0.0) + \
                (top if sources in ('both', 'flux_top') else 0.0)
            assert np.array_equal(got, np.broadcast_to(want, got.shape))


@pytest.mark.gpu
def test_bit_for_bit_with_single_spectrum_kernels(eng, orc):
    """Per walker the batch row has the bits of plane_parallel_optical_depth(inf) ->
    engine.two_stream -> flux_up[0] ("same operations in the same order")."""
    import torch
    L, W, nw = 33, 515, 4
    ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
    ec_d, h_d, t_d = eng.dev(ecs), eng.dev(intervals), eng.dev(temps)
    wn_d, fi_d, ft_d = eng.dev(wn), eng.dev(f_int), eng.dev(top)
    for fi, ft in ((fi_d, ft_d), (None, None)):
        got = eng.two_stream_batch(ec_d.clone(), h_d, wn_d, t_d, fi, ft)
        for w in range(nw):
            depth, _ = eng.plane_parallel_optical_depth(ec_d[w], h_d[w], 0, L, np.inf)
            one = eng.two_stream(depth, wn_d, t_d[w], fi, ft, 0)[1][0]
            assert torch.equal(got[w], one), f'walker {w}'
    _, ups = oracle(orc, L, W, nw, 'both')
    got = host(eng.two_stream_batch(ec_d.clone(), h_d, wn_d, t_d, fi_d, ft_d))
    for w in range(nw):
        close_by_column(got[w], ups[w, 0], RTOL, np.max(np.abs(ups[w]), axis=0))


@pytest.mark.gpu
def test_dirty_memory(eng, orc):
    """out and work start as NaN, ec is a clone; the row after out[nw] and the tail after the
    work the entry point asks for stay untouched; what the call leaves in ec is each interval's
    optical depth, np.diff of the oracle's running sums (the bits: the same IEEE operations in
    the same order on both sides, no contraction); a second call on a fresh clone, with work
    holding the first call's leftovers, gives the same bits."""
    import torch
    from pyratbay_amd import _capi
    L, W, nw, guard = 33, 257, 5, 64
    ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
    depths, ups = oracle(orc, L, W, nw, 'both')
    need = _capi.lib().pb_two_stream_batch_work_doubles(L, W, nw)
    assert need >= nw * (L - 1) * W
    ec_d, h_d, t_d = eng.dev(ecs), eng.dev(intervals), eng.dev(temps)
    wn_d, fi_d, ft_d = eng.dev(wn), eng.dev(f_int), eng.dev(top)
    results = []
    work = torch.full((need + guard,), float('nan'), dtype=torch.float64, device='cuda')
    work[need:] = -7.0
    for _ in range(2):
        out = torch.full((nw + 1, W), float('nan'), dtype=torch.float64, device='cuda')
        out[nw] = -7.0
        ec = ec_d.clone()
        got = eng.two_stream_batch(ec, h_d, wn_d, t_d, fi_d, ft_d, out=out[:nw], work=work[:need])
        assert got.data_ptr() == out.data_ptr()
        assert bool((out[nw] == -7.0).all()) and bool((work[need:] == -7.0).all())
        assert bool(torch.isfinite(work[:need]).all())
        assert np.array_equal(host(ec[:, :L - 1]), np.diff(depths, axis=1))
        results.append(out[:nw].clone())
    assert torch.equal(results[0], results[1])
    for w in range(nw):
        close_by_column(host(results[0][w]), ups[w, 0], RTOL, np.max(np.abs(ups[w]), axis=0))
    with pytest.raises(ValueError, match='work'):
        eng.two_stream_batch(ec_d.clone(), h_d, wn_d, t_d, fi_d, ft_d, work=work[:need - 1])


@pytest.mark.gpu
def test_degenerate_column(eng, orc):
    """An all-zero ec column: dtau0 = 0 -> 0 * exp1(0) = NaN in the oracle and in the batch; its
    neighbours (other threads of the same wavefront) stay within tolerance."""
    L, W, nw, dead = 17, 256, 1, 100
    ecs, intervals, temps, wn, f_int, top = case(L, W, nw)
    ecs = ecs.copy()
    ecs[0, :, dead] = 0.0
    depth = oracle_depth(orc, ecs[0], intervals[0])
    want = orc.two_stream(depth, wn, temps[0], f_int, top, 0)[1]
    assert np.isnan(want[0, dead])
    got = host(run_batch(eng, ecs, intervals, temps, wn, f_int, top))[0]
    assert np.isnan(got[dead])
    live = np.arange(W) != dead
    assert np.all(np.isfinite(want[:, live]))
    close_by_column(got[live], want[0, live], RTOL, np.max(np.abs(want[:, live]), axis=0))
