"""The fused emission batch (k_emission_fused: plane-parallel optical depth + Planck + intensity +
quadrature sum of a batch of walkers in one pass) through the C ABI -- pb_emission_flux_batch,
pb_emission_flux_ordered, pb_emission_flux_limited -- against the oracle chain
plane_parallel_optical_depth -> blackbody_wn_2D -> intensity -> weighted sum (1e-11, the
tolerance of test_gpu_batch.py / test_gpu_columns.py for emission fluxes), and bit for bit
against the device paths the code says do the same operations in the same order.  Buffers the
kernels are documented not to read hold NaN, outputs they must write or must leave alone hold a
sentinel."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-11


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def walkers(seed, L, W, nw, spread=1.0):
    """cases.column_case scaled per walker: ec[nw, L, W], intervals[nw, L - 1], temps[nw, L] (every
    walker its own opacity scale, radius profile and temperatures) and wn[W]."""
    rng = np.random.default_rng(seed)
    c = cases.column_case(seed=seed, nlayers=L, nwave=W)
    ecs = np.array([c['ec'] * 10.0**rng.uniform(-spread, spread) for _ in range(nw)])
    radius = np.array([np.sort(c['radius'] * (1 + 0.01 * rng.uniform(-1, 1)))[::-1]
                       for _ in range(nw)])
    intervals = np.ascontiguousarray(-np.diff(radius, axis=1))
    temps = c['temp'][None] * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))) + rng.uniform(-20, 20, (nw, L))
    return ecs, intervals, temps, c['wn']


def batch(eng, ecs, intervals, wn, temps, mu, weights, itop, ibottom, maxdepth, **kw):
    """engine.emission_flux_batch on host arrays; the output starts as NaN (a column the kernel
    does not write shows)."""
    import torch
    nw, _, W = ecs.shape
    if 'out' not in kw:
        kw['out'] = torch.full((nw, W), float('nan'), dtype=torch.float64, device='cuda')
    return eng.emission_flux_batch(eng.dev(ecs), eng.dev(intervals), eng.dev(wn), eng.dev(temps),
                                   eng.dev(mu), eng.dev(weights), itop, ibottom, maxdepth, **kw)


SHAPES = [(1, 0, 1, 1), (2, 0, 2, 63), (5, 4, 5, 70), (17, 0, 17, 256), (33, 2, 20, 515),
          (33, 2, 33, 257)]


@pytest.mark.parametrize('stop_rule', ['zero', 'half', 'inf'])
@pytest.mark.parametrize('L,itop,ibottom,W', SHAPES)
def test_shapes_and_stop_rules(eng, orc, L, itop, ibottom, W, stop_rule):
    """pb_emission_flux_batch in grid order against the oracle: one layer and one column; one
    interval; itop == L - 1 (no interval: the top layer's emission); exactly one and more than
    one workgroup of 256 columns, ragged; ibottom inside the grid and at its end -- each with
    maxdepth 0 (every column stops after its first interval), a maxdepth that about half of the
    columns cross before the bottom (the median of the depths the oracle finds there; 1 where no
    column has an interval) and inf (no column stops early)."""
    nw = 5
    ecs, intervals, temps, wn = walkers(100 + L + W, L, W, nw)
    mu, weights = eng.default_quadrature()
    bottom = min(ibottom, L - 1)
    reach = np.array([cases.emission_oracle(orc, ecs[w], intervals[w], wn, temps[w], mu, weights,
                                            itop, ibottom, np.inf)[2][bottom] for w in range(nw)])
    half = float(np.median(reach[reach > 0])) if np.any(reach > 0) else 1.0
    maxdepth = {'zero': 0.0, 'half': half, 'inf': np.inf}[stop_rule]
    got = host(batch(eng, ecs, intervals, wn, temps, mu, weights, itop, ibottom, maxdepth))
    stops = []
    for w in range(nw):
        want, stop, _ = cases.emission_oracle(orc, ecs[w], intervals[w], wn, temps[w], mu,
                                              weights, itop, ibottom, maxdepth)
        assert np.all(np.isfinite(want))
        np.testing.assert_allclose(got[w], want, rtol=RTOL, err_msg=f'walker {w}')
        stops.append(stop)
    stops = np.array(stops)
    if bottom > itop:
        # the stop rule did what its name says
        if stop_rule == 'zero':
            assert np.all(stops == itop + 1)
        elif stop_rule == 'inf':
            assert np.all(stops == bottom)
        elif bottom > itop + 1:
            early = np.mean(stops < bottom)
            assert 0.2 < early < 0.8, early


@pytest.mark.parametrize('nmu', [1, 8, 9, 16])
def test_quadrature_width(eng, orc, nmu):
    """Both instantiations of the batch kernel: k_emission_fused<8> up to 8 angles (1, 8),
    k_emission_fused<16> beyond (9; 16 fills every running sum) -- against the oracle, and bit
    for bit against the pair of single-spectrum kernels run one after the other per walker
    (plane_parallel_optical_depth + emission_flux: "same operations in the same order")."""
    import torch
    L, itop, ibottom, W, nw, maxdepth = 33, 2, 20, 515, 4, 10.0
    ecs, intervals, temps, wn = walkers(300 + nmu, L, W, nw)
    mu, weights = eng.gauss_quadrature(nmu)
    assert len(mu) == nmu
    got = batch(eng, ecs, intervals, wn, temps, mu, weights, itop, ibottom, maxdepth)
    ec_d, h_d, t_d = eng.dev(ecs), eng.dev(intervals), eng.dev(temps)
    wn_d, mu_d, we_d = eng.dev(wn), eng.dev(mu), eng.dev(weights)
    for w in range(nw):
        want, stop, _ = cases.emission_oracle(orc, ecs[w], intervals[w], wn, temps[w], mu,
                                              weights, itop, ibottom, maxdepth)
        np.testing.assert_allclose(host(got[w]), want, rtol=RTOL, err_msg=f'walker {w}')
        depth, ideep = eng.plane_parallel_optical_depth(ec_d[w], h_d[w], itop, ibottom, maxdepth)
        assert np.array_equal(host(ideep), stop)
        one = eng.emission_flux(depth, ideep, wn_d, t_d[w], mu_d, we_d, itop)
        assert torch.equal(got[w], one), f'walker {w}'


@pytest.mark.parametrize('maxdepth', [10.0, np.inf])
def test_special_values(eng, orc, maxdepth):
    """The batch kernel's own clamp_depth / quot_fast handling: columns whose running depth
    overflows to inf (ec so large in the deepest layers that the product with the interval does;
    ec = inf itself), a walker whose depths pass 1e5 -- the clamp -- and go on (maxdepth = inf),
    layers at T = 0 (at itop, inside the column, at the layer where the depth becomes inf and at
    the bottom).  exp(-inf / mu) = 0 and B(T = 0) = 0 like the reference's divisions: the flux
    is finite wherever the oracle's is, and equal to it."""
    L, itop, W, nw = 17, 1, 259, 4
    ecs, intervals, temps, wn = walkers(17, L, W, nw, spread=0.3)
    ecs[:, 12:, ::3] = 1e305                      # 0.5 h (ec + ec) overflows: depth = inf at layer 12
    ecs[:, 9:, 1::7] = np.inf
    with np.errstate(over='ignore'):
        ecs[2] *= 1e6                             # (the huge values become inf)
    temps[0, 3] = 0.0
    temps[1, itop] = 0.0
    temps[2, L - 1] = 0.0
    temps[3, 12] = 0.0
    mu, weights = eng.default_quadrature()
    got = host(batch(eng, ecs, intervals, wn, temps, mu, weights, itop, L, maxdepth))
    seen_inf = seen_clamp = False
    for w in range(nw):
        want, stop, depth = cases.emission_oracle(orc, ecs[w], intervals[w], wn, temps[w], mu,
                                                  weights, itop, L, maxdepth)
        last = depth[np.minimum(stop, L - 1), np.arange(W)]
        seen_inf |= bool(np.any(np.isinf(last)))
        seen_clamp |= bool(np.any((depth[itop + 1:L - 1] > 1e5) & np.isfinite(depth[itop + 1:L - 1]) &
                                  (stop[None] == L - 1)))
        ok = np.isfinite(want)
        assert ok.mean() > 0.9                    # (the oracle handles these values itself)
        assert np.all(np.isfinite(got[w][ok])), f'walker {w}'
        np.testing.assert_allclose(got[w][ok], want[ok], rtol=RTOL, err_msg=f'walker {w}')
    assert seen_inf
    assert seen_clamp or np.isfinite(maxdepth)


def test_ordered_columns(eng, orc):
    """pb_emission_flux_ordered: the columns of ec and wn in a random order, `column` naming the
    grid index of each -- the flux comes back in grid order with the bits of the unordered call.
    An entry of `column` outside the grid (the kernel tests it before it stores) drops that
    column alone: its place keeps what the output held, every other column its value."""
    import torch
    L, itop, W, nw, maxdepth = 33, 2, 515, 4, 10.0
    rng = np.random.default_rng(8)
    ecs, intervals, temps, wn = walkers(41, L, W, nw)
    mu, weights = eng.default_quadrature()
    grid = batch(eng, ecs, intervals, wn, temps, mu, weights, itop, L, maxdepth)
    want, _, _ = cases.emission_oracle(orc, ecs[1], intervals[1], wn, temps[1], mu, weights, itop,
                                       L, maxdepth)
    np.testing.assert_allclose(host(grid[1]), want, rtol=RTOL)
    perm = rng.permutation(W)
    ecs_p, wn_p = np.ascontiguousarray(ecs[:, :, perm]), wn[perm]
    col = eng.dev(perm, torch.int32)
    got = batch(eng, ecs_p, intervals, wn_p, temps, mu, weights, itop, L, maxdepth, column=col)
    assert torch.equal(got, grid)
    dropped = {3: -1, 255: W, 256: W + 1000000, W - 1: -W}      # position in the order -> entry
    bad = perm.copy()
    for j, entry in dropped.items():
        bad[j] = entry
    out = torch.full((nw, W), -7.0, dtype=torch.float64, device='cuda')
    batch(eng, ecs_p, intervals, wn_p, temps, mu, weights, itop, L, maxdepth,
          column=eng.dev(bad, torch.int32), out=out)
    expect = grid.clone()
    expect[:, torch.as_tensor(perm[list(dropped)], device='cuda')] = -7.0
    assert torch.equal(out, expect)


def limited_case(L, itop, W, nw=9, maxdepth=10.0):
    """Walkers for the tile-limited call: column_case scaled so that the weakest of the base
    walker's columns crosses maxdepth by layer L - 3 -- but for its four transparent columns, which
    end at the bottom for every walker (sorted last, they give the last block its last tile, and
    with limits that are too low they make every walker overrun); walker 3 is 30 times more
    opaque, walker 5 30 times more transparent, the others within 12 % of the base."""
    rng = np.random.default_rng(2000 + L + W)
    c = cases.column_case(seed=500 + L + W, nlayers=L, nwave=W)
    ec0 = c['ec'].copy()
    h0 = -np.diff(c['radius'])
    depth0 = np.cumsum(0.5 * h0[itop:, None] * (ec0[itop + 1:] + ec0[itop:-1]), axis=0)
    ec0 *= 3.0 * maxdepth / depth0[L - 3 - itop - 1, 4:].min()
    scale = 10.0**rng.uniform(-0.05, 0.05, nw)
    scale[0], scale[3], scale[5] = 1.0, 30.0, 1.0 / 30.0
    ecs = ec0[None] * scale[:, None, None]
    intervals = h0[None] * (1 + 0.01 * rng.uniform(-1, 1, (nw, 1)))
    intervals[0] = h0
    temps = c['temp'][None] * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))) + rng.uniform(-20, 20, (nw, L))
    return ecs, np.ascontiguousarray(intervals), temps, c['wn']


def limit_sets(stops_ordered, itop, L):
    """The three sets of per-block limits and, from the oracle's stop layers alone, which columns
    (in the worked order) of which walkers run past them."""
    W = stops_ordered.shape[1]
    sets = {}
    for name, tile in (('exact', cases.block_tiles(stops_ordered.max(axis=0), itop, L)),
                       ('base model, no margin', cases.block_tiles(stops_ordered[0], itop, L)),
                       ('far too low', np.zeros(-(-W // 256), np.int32))):
        klim = cases.limit_layer(tile, itop, W)
        sets[name] = (tile, klim, stops_ordered > klim[None])
    return sets


@pytest.mark.parametrize('L,itop,W', [(33, 2, 700), (17, 0, 300), (80, 0, 515)])
def test_limited_and_gated_repair(eng, orc, L, itop, W):
    """pb_emission_flux_limited with emission semantics (test_gpu_batch.test_tile_limited_batch is
    the transit half).  Columns in the order of walker 0's stop layer, limits per block of 256:
    right for every walker / walker 0's own / all zero.  A column runs past a limit iff the layer
    at which the oracle's depth loop leaves it lies beyond the last layer of the block's tile,
    itop + 16 (tile + 1) - 1 (the kernel walks layer by layer and a workgroup is one block: no
    per-wavefront granularity); flags[w] is set iff a column of walker w does, flags[nw] iff any.
    ec holds NaN above itop and beyond each block's limit: a read past a limit would show in a
    column that did not overrun, which must have the bits of the unlimited ordered call.  The
    repair (ec complete, gate = flags) writes the flagged walkers and leaves the others alone."""
    import torch
    nw, maxdepth = 9, 10.0
    ecs, intervals, temps, wn = limited_case(L, itop, W, nw, maxdepth)
    mu, weights = eng.default_quadrature()
    fluxes, stops = [], []
    for w in range(nw):
        f, s, _ = cases.emission_oracle(orc, ecs[w], intervals[w], wn, temps[w], mu, weights,
                                        itop, L, maxdepth)
        fluxes.append(f)
        stops.append(s)
    stops = np.array(stops)
    order = np.argsort(stops[0], kind='stable')
    ecs_o, wn_o = np.ascontiguousarray(ecs[:, :, order]), wn[order]
    col = eng.dev(order, torch.int32)
    want = batch(eng, ecs_o, intervals, wn_o, temps, mu, weights, itop, L, maxdepth, column=col)
    for w in (0, 3, 5):
        np.testing.assert_allclose(host(want[w]), fluxes[w], rtol=RTOL, err_msg=f'walker {w}')
    sets = limit_sets(stops[:, order], itop, L)
    # the three sets are the three situations (else the assertions below would be vacuous)
    nflag = {name: int(over.any(axis=1).sum()) for name, (_, _, over) in sets.items()}
    assert nflag['exact'] == 0 and 0 < nflag['base model, no margin'] < nw and \
        nflag['far too low'] == nw, nflag
    lay = np.arange(L)[None, :, None]
    clean = ecs_o.copy()
    clean[:, :itop] = np.nan
    for name, (tile, klim, over) in sets.items():
        flagged = over.any(axis=1)
        ec = np.where(lay > klim[None, None, :], np.nan, clean)
        flags = torch.zeros(nw + 1, dtype=torch.int32, device='cuda')
        out = torch.full((nw, W), -7.0, dtype=torch.float64, device='cuda')
        got = batch(eng, ec, intervals, wn_o, temps, mu, weights, itop, L, maxdepth, column=col,
                    tile_limit=eng.dev(tile, torch.int32), flags=flags, out=out)
        f = host(flags)
        assert np.array_equal(f[:nw] != 0, flagged), (name, f, flagged)
        assert f[nw] == int(flagged.any()), (name, f)
        # first pass: every column that stayed inside its limit (grid order)
        inside = np.zeros((nw, W), bool)
        inside[:, order] = ~over
        inside_d = torch.as_tensor(inside, device='cuda')
        assert bool(torch.isfinite(got[inside_d]).all()), name
        assert torch.equal(got[inside_d], want[inside_d]), name
        if name == 'exact':
            assert torch.equal(got, want)
        # repair pass: only the flagged walkers are written
        keep = torch.as_tensor(~flagged, device='cuda')
        got[keep] = -3.0
        batch(eng, clean, intervals, wn_o, temps, mu, weights, itop, L, maxdepth, column=col,
              gate=flags, out=got)
        assert torch.equal(got[~keep], want[~keep]), name
        assert bool((got[keep] == -3.0).all()), name
        assert np.array_equal(host(flags), f), name          # (the repair does not touch the flags)
