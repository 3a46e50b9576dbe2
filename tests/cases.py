"""Seeded small inputs shared by the golden-vector generator and the parity tests.

Pure NumPy; the only expected values computed here are the oracle's Voigt tables
(oracle_voigt_table, oracle_voigt_rows), built by the oracle passed in."""
import os

import numpy as np
import pytest

from pyratbay_amd import synth

# The measured dead ends (gather modes scatter / rounds / wave, the one-pass and layers-outer
# matrix transit kernels, predicted `resolution` run plans) live in libpbhip_exp.so only
# (`make -C pyratbay_amd/csrc EXPERIMENTS=1`, PB_LIBPBHIP=pyratbay_amd/libpbhip_exp.so); their
# tests carry the marker `gpu_experiments` and are deselected otherwise (tests/conftest.py).
EXPERIMENTS = os.environ.get('PB_LIBPBHIP', '').endswith('libpbhip_exp.so')
EXPERIMENTAL_GATHERS = ('scatter', 'rounds', 'wave')


def exp(*values):
    """pytest.param(...) marked gpu_experiments."""
    return pytest.param(*values, marks=pytest.mark.gpu_experiments)


def gathers(*modes):
    """Parametrisation over gather modes: the experimental ones marked gpu_experiments."""
    return [exp(m) if m in EXPERIMENTAL_GATHERS else m for m in modes]


def live(*modes):
    """The gather modes of a loop inside a test that the loaded library carries."""
    return tuple(m for m in modes if EXPERIMENTS or m not in EXPERIMENTAL_GATHERS)


def voigt_case():
    """6 x 4 width grid at a coarse step: contains skipped cells (size 0), cells whose
    step resolves the Doppler core (two-point mean), oversampled/Simpson cells and one
    cell above 99999 samples (QUICK point sampling) -- voigt.h:235-290."""
    lorentz = np.array([1e-4, 2e-3, 0.02, 0.3, 2.0, 6.0])
    doppler = np.array([4e-3, 0.012, 0.05, 0.7])
    dwn = 2.5e-4
    size = np.array([
        [40, 60, 400, 1500],
        [35, 0, 420, 900],
        [300, 0, 0, 2000],
        [2000, 0, 0, 2500],
        [3000, 0, 0, 0],
        [50001, 0, 0, 0],
    ])
    return dict(lorentz=lorentz, doppler=doppler, dwn=dwn, size=size)


def extinction_inputs(resolution=False, seed=7):
    """~2400 lines, 3 isotopes of two species, coarse fine-grid; includes exact
    duplicates / near-coincident lines (co-adding), lines outside the grid and
    an exact tie for the nearest fine-grid index."""
    rng = np.random.default_rng(seed)
    wnlow, wnstep, osamp = 5000.0, 0.05, 12
    nwave = 801
    if resolution:
        # constant resolving power output grid; fine grid keeps wnstep=1/osamp rule
        R = 120000.0
        wn = wnlow * np.exp(np.arange(nwave) / R)
        ownstep = wnstep / osamp
        onwave = int(np.ceil((wn[-1] - wnlow) / ownstep)) + 1
        own = wnlow + np.arange(onwave) * ownstep
    else:
        g = synth.spectral_grid(wnlow, wnlow + (nwave - 1) * wnstep + 0.01, wnstep, osamp)
        wn, own, ownstep, onwave = g['wn'], g['own'], g['ownstep'], g['onwave']
    divisors = synth.divisors(osamp)

    niso = 3
    counts = [1500, 500, 400]
    lwn, lid = [], []
    for i, c in enumerate(counts):
        v = rng.uniform(own[0] - 1.0, own[-1] + 1.0, c)      # some out of range
        # near-coincident pairs -> co-added lines
        v[:c // 10] = v[c // 10:2 * (c // 10)] + rng.uniform(-0.4, 0.4, c // 10) * ownstep
        # an exact mid-point tie between two fine samples
        v[-1] = own[1234 + i] + 0.5 * ownstep
        lwn.append(np.sort(v))
        lid.append(np.full(c, i, np.int32))
    lwn = np.concatenate(lwn)
    lid = np.concatenate(lid)
    nlines = len(lwn)
    elow = rng.uniform(0, 6000.0, nlines)
    gf = 10.0**rng.uniform(-9, -4, nlines)

    atm = synth.synthetic_atmosphere(9, ('H2', 'He', 'H2O', 'CO'),
                                     (0.85, 0.1485, 1e-3, 5e-4), ptop=1e-5, pbottom=50.0)
    iso = dict(
        isoimol=np.array([2, 2, 3], np.int32),
        isomass=np.array([18.01, 20.01, 28.01]),
        isoratio=np.array([0.997, 0.002, 0.99]),
        isoiext=np.array([0, 0, 1], np.int32),
    )
    lorentz, doppler = synth.voigt_widths(
        wn, atm['press'], atm['mol_mass'][2:4], atm['mol_radius'][2:4], 14, 7)
    extent, cutoff = 40.0, 6.0
    size = synth.voigt_sizes(lorentz, doppler, extent, cutoff, ownstep, onwave, 0.1)
    return dict(wn=wn, own=own, divisors=divisors, lwn=lwn, lid=lid, elow=elow, gf=gf,
                atm=atm, iso=iso, lorentz=lorentz, doppler=doppler, size=size,
                cutoff=cutoff, nspec=2)


def iso_z(temp, niso):
    """Synthetic partition functions, one per isotope."""
    return (1.0 + temp**1.5 / 10.0) * (1.0 + 0.1 * np.arange(niso))


def extinction_variants():
    """(layer, add, cutoff_on, ethresh, skip_iso) combinations of fixture G2."""
    out = []
    for add in (0, 1):
        for cut in (0, 1):
            for eth in (1e-30, 1e-3):
                out.append((4, add, cut, eth, 0))
    for layer in (0, 8):
        for add in (0, 1):
            out.append((layer, add, 1, 1e-30, 0))
    out.append((4, 0, 1, 1e-30, 1))      # isoiext = -1 for one isotope
    out.append((2, 1, 1, 1e-6, 1))
    return out


def column_case(seed=3, nlayers=24, nwave=96):
    """Random ec field spanning optically thin..thick columns, plus geometry."""
    rng = np.random.default_rng(seed)
    radius = np.linspace(8.0e9, 7.0e9, nlayers) + rng.uniform(-1e6, 1e6, nlayers)
    radius = np.sort(radius)[::-1].copy()
    press = np.logspace(-6, 2, nlayers)
    scale = 10.0**rng.uniform(-14, -8.5, nwave)
    ec = press[:, None]**0.9 * scale[None, :] * rng.uniform(0.5, 1.5, (nlayers, nwave))
    ec[:, :4] = 0.0                                           # transparent columns
    temp = np.linspace(900.0, 1900.0, nlayers) + rng.uniform(-30, 30, nlayers)
    wn = np.linspace(2000.0, 9000.0, nwave)
    mu = np.cos(np.radians([0.0, 20.0, 40.0, 60.0, 80.0]))
    return dict(radius=radius, ec=ec, temp=temp, wn=wn, mu=mu, rstar=8.8e10,
                nlayers=nlayers, nwave=nwave)


def emission_oracle(orc, ec, intervals, wn, temp, mu, weights, itop, ibottom, maxdepth):
    """The oracle chain of the emission geometry for one walker: plane-parallel optical depth ->
    Planck -> intensity per mu -> weighted sum.  Returns (flux[W], stop[W], depth[L, W]); stop is
    the layer at which the depth loop left each column (nlayers where there is no interval below
    itop: the reference clips it to the last layer before it forms the intensity)."""
    ec = np.ascontiguousarray(ec, np.float64)
    L, W = ec.shape
    depth = np.zeros((L, W))
    stop = np.zeros(W, np.int32)
    orc.plane_parallel_optical_depth(depth, stop, ec, intervals, maxdepth, itop, ibottom)
    B = orc.blackbody_wn_2D(wn, temp)
    inten = orc.intensity(depth, np.minimum(stop, L - 1), B, mu, itop)
    return np.sum(inten * np.asarray(weights)[:, None], axis=0), stop, depth


def block_tiles(stop, itop, nlayers, margin=0):
    """The last row tile (16 layers from itop) each block of 256 columns can need, from the layers
    `stop` at which its columns end (in the order the columns are worked in) -- derived as
    TableSpectrum.order_columns does: the ragged last block padded with the last column."""
    stop = np.asarray(stop, np.int64)
    nblk = -(-len(stop) // 256)
    padded = np.concatenate([stop, np.full(nblk * 256 - len(stop), stop[-1])])
    ntiles = -(-(nlayers - itop) // 16)
    return np.clip((padded.reshape(nblk, 256).max(axis=1) - itop + margin) // 16, 0,
                   ntiles - 1).astype(np.int32)


def limit_layer(tile, itop, nwave):
    """The last layer available to each column under the per-block limits `tile`."""
    return itop + 16 * (np.asarray(tile, np.int64)[np.arange(nwave) // 256] + 1) - 1


def limited_table_model(L, itop, W, nw=9, opacity=1.0):
    """The small retrieval model of test_gpu_batch.test_tile_limited_batch: 3 species, 6 table
    temperatures, columns over six decades of opacity, nw walkers of which walker 3 is 30 times
    more opaque and walker 5 30 times more transparent than the rest.  opacity: a factor on every
    density (the emission geometry looks down the column, not along the slant path of a transit,
    and finds the same atmosphere some 50 times thinner)."""
    rng = np.random.default_rng(1000 + L + W)
    nspec, ntemp = 3, 6
    ttable = np.linspace(300.0, 3000.0, ntemp)
    press = np.logspace(-6, 2, L)
    etable = 10.0**rng.uniform(-27, -21, (nspec, ntemp, L, 1)) * \
        10.0**rng.uniform(-3, 3, (nspec, 1, 1, W))
    radius0 = np.linspace(8.0e9, 7.0e9, L)
    temps = 1500.0 * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))) * np.linspace(0.8, 1.2, L)
    dens = (press / temps)[:, :, None] * 7.2e21 * 10.0**rng.uniform(-7, -3, (nw, 1, nspec))
    dens[3] *= 30.0
    dens[5] /= 30.0
    dens *= opacity
    g = synth.spectral_grid(4000.0, 4000.0 + (W - 1) * 0.05 + 0.01, 0.05, 12)
    # per-walker radius profiles (strictly decreasing) for the rows that want them
    radius = radius0[None] * (1 + 0.01 * rng.uniform(-1, 1, (nw, 1))) + \
        np.linspace(0, 1, L)[None] * 2e7 * rng.uniform(-1, 1, (nw, 1))
    bands = [(1, np.ones(W - 2), 1.0),
             (W // 3, np.exp(-np.linspace(-1.5, 1.5, W // 2)**2), 0.5)]
    return dict(etable=etable, ttable=ttable, temps=temps, dens=dens, radius0=radius0,
                radius=radius, wn=g['wn'], bands=bands, rstar=8.8e10, nlayers=L, itop=itop,
                nwave=W, nw=nw)


def table_bandflux_oracle(orc, m, rt_path, temp, dens, radius, maxdepth=10.0, mu=None,
                          weights=None):
    """Band fluxes of one walker of limited_table_model through the oracle chain (interp_ec ->
    optical depth -> transmission, or -> Planck -> intensity -> weighted sum; bands by
    np.trapezoid) and the layer at which each column stopped."""
    L, W, itop, wn = m['nlayers'], m['nwave'], m['itop'], m['wn']
    ec = np.zeros((L, W))
    orc.interp_ec(ec, m['etable'], m['ttable'], temp, dens, 0, L)
    if rt_path == 'transit':
        depth, stop = orc.optical_depth_transit(ec, radius, itop, L, maxdepth)
        spec = orc.transmission(depth, radius, m['rstar'], stop, itop)
    else:
        spec, stop, _ = emission_oracle(orc, ec, -np.diff(radius), wn, temp, mu, weights, itop,
                                        L, maxdepth)
    flux = [np.trapezoid(spec[s:s + len(r)] * r, wn[s:s + len(r)]) * h for s, r, h in m['bands']]
    return np.array(flux), np.asarray(stop)


def table_case(seed=11):
    rng = np.random.default_rng(seed)
    nmol, ntemp, nlayers, nwave = 3, 5, 7, 50
    ttable = np.array([300.0, 700.0, 1100.0, 1800.0, 3000.0])
    etable = 10.0**rng.uniform(-30, -20, (nmol, ntemp, nlayers, nwave))
    temps = np.array([300.0, 450.0, 700.0, 1099.999, 1800.0, 2999.0, 3000.0])
    dens = 10.0**rng.uniform(8, 18, (nlayers, nmol))
    return dict(etable=etable, ttable=ttable, temps=temps, dens=dens)


# ---------------------------------------------------------------------------
# Voigt tables: the planner's regime decisions, a boundary grid, independent tables
# ---------------------------------------------------------------------------
def voigt_plan(half, dwn, alphaD):
    """(regime, over) of one table cell of half-size `half`: the decisions voigtn takes before
    it evaluates (voigt.h:235-262), restated in binary64 like pb_voigt.hip's plan_cell and the
    oracle.  'quick' = point samples (more than 99 999 samples), 'mean' = mean of the two
    bounding points (the step resolves the Doppler core), 'simpson' = Simpson mean over `over`
    sub-intervals (`over` is rounded up to an even number, so the trapezoid form with
    over > 1 never runs)."""
    nwn = 2 * int(half) + 1
    halfwidth = dwn * (nwn // 2)
    step = 2.0 * halfwidth / (nwn - 1)
    fine = alphaD / (50 - 1)
    if nwn > 99999:
        return 'quick', 1
    if step < fine:
        return 'mean', 1
    over = int(step / fine) + 1
    if over & 1:
        over += 1
    return 'simpson', over


def voigt_regimes(doppler, size, dwn):
    """Regime of every cell of a width grid ('' for the aliased cells, size 0)."""
    out = np.full(np.shape(size), '', dtype=object)
    for (m, n), half in np.ndenumerate(np.asarray(size)):
        if half:
            out[m, n] = voigt_plan(half, dwn, float(doppler[n]))[0]
    return out


def _doppler_at_ratio(step, k):
    """Doppler widths a with step / (a / 49) == k exactly and with the largest quotient below k
    (searched over the doubles next to 49 * step / k, evaluated as the planner does)."""
    a0 = 49.0 * step / k
    cands = [a0]
    up = down = a0
    for _ in range(256):
        up, down = np.nextafter(up, np.inf), np.nextafter(down, 0.0)
        cands += [float(up), float(down)]
    ratio = {a: step / (a / 49) for a in cands}
    at = [a for a in cands if ratio[a] == k]
    below = max((a for a in cands if ratio[a] < k), key=lambda a: ratio[a])
    assert at, f'no Doppler width puts step/fine at {k}'
    return at[0], below


def voigt_boundary_case():
    """A hand-made width grid whose cells sit exactly on the switches of voigtn (voigt.h:147-359):

    * half 49 999 / 50 000: 99 999 samples (oversampled) / 100 001 samples (QUICK);
    * half 1: the 3-sample minimum;
    * step / fine = 1, 2, 3 exactly and just below each (two-point mean vs Simpson at 1;
      over = 2 vs 4 at 2; the odd over = 3 rounded up to 4 at 3);
    * a Doppler width 5 000 times below the step (over in the thousands);
    * y = sqrt(ln 2) alphaL / alphaD within 1e-12 on either side of 1.8 and of 5 (the switches
      between the series (Region I), the 3-term and the 2-term rational forms);
    * a row whose Doppler columns after the first are all aliased (size 0).

    Returns dict(lorentz, doppler, dwn, size, ratio_cols, y): ratio_cols[n] = (k, 'at' | 'below')
    for the columns placed on step / fine = k (at half-size 40), y[m, n] the cells' y."""
    dwn = 1.0e-3
    hb = 40                                   # half-size of the cells of the step/fine columns
    step = 2.0 * (dwn * hb) / (2 * hb)
    doppler = [4.0e-3]                        # column 0: step/fine = 12.25 -> over 14
    ratio_cols = {}
    for k in (1, 2, 3):
        at, below = _doppler_at_ratio(step, k)
        ratio_cols[len(doppler)] = (k, 'at')
        ratio_cols[len(doppler) + 1] = (k, 'below')
        doppler += [at, below]
    big = len(doppler)
    doppler.append(1.0e-5)                    # step / fine = 4 900 -> over 4 902
    doppler.append(0.3)                       # step < fine: two-point mean at any half
    sq = float(np.sqrt(np.log(2.0)))
    d0 = doppler[0]
    # y at column 0 on either side of 1.8 and 5, and two generic rows
    lorentz = [1.0e-4, 0.02]
    for yb in (1.8, 5.0):
        for rel in (-1e-12, 1e-12):
            lorentz.append(yb * (1.0 + rel) * d0 / sq)
    nd = len(doppler)
    size = np.zeros((len(lorentz) + 1, nd), np.int64)
    lorentz.append(3.0e-3)                    # the aliased row
    # row 0: the step/fine columns at half hb, the extremes of the half-size elsewhere
    size[0] = hb
    size[0, 0] = 1
    size[0, big] = 12
    size[0, big + 1] = 50000
    # row 1: 99 999 samples (Simpson in column 0, two-point mean in the last), 100 001 samples,
    # a 3-sample cell followed by aliases
    size[1] = 0
    size[1, 0] = 49999
    size[1, big + 1] = 49999
    size[1, 2] = 50000
    size[1, 3] = 1
    size[1, big] = 7
    # rows 2..5 (y on a switch): the whole row, mixed sizes
    for m in range(2, 6):
        size[m] = [300, hb, hb, hb, hb, hb, hb, 9, 2500][:nd]
    # the last row: every column after the first aliased
    size[-1, 0] = 777
    lorentz = np.asarray(lorentz)
    doppler = np.asarray(doppler)
    return dict(lorentz=lorentz, doppler=doppler, dwn=dwn, size=size, ratio_cols=ratio_cols,
                y=sq * lorentz[:, None] / doppler[None, :])


# the width grids of the full-size configurations (bench.py WORKLOADS, test_gpu_configs.FULL);
# the widths do not depend on the line list, so a handful of lines builds them
C4_SPECIES = ('H2', 'He', 'H2O', 'CO', 'CO2', 'CH4')
C4_VMR = (0.85, 0.149, 4e-4, 5e-4, 1e-7, 1e-4)
FULL_GRIDS = {
    'c2': ((100001, 80), dict(wnstep=0.05, niso=1)),
    'c3': ((1000001, 80), dict(wnstep=0.005, niso=4)),
    'c4': ((1000001, 120), dict(wnstep=0.005, niso=4, species=C4_SPECIES, vmr=C4_VMR,
                                line_species=('H2O', 'CO', 'CO2', 'CH4'))),
    'c2-res': ((100001, 80), dict(wnstep=0.05, niso=1, resolution=123300.0)),
}


def full_width_grid(name, nlines=16):
    """synth.lbl_case of a full-size configuration with a short line list."""
    args, kw = FULL_GRIDS[name]
    return synth.lbl_case(args[0], args[1], nlines, seed=42, **kw)


_ORACLE_TABLE = {}


def oracle_voigt_table(orc, voigt, ownstep):
    """(profile, size, index) of the width grid voigt = dict(lorentz, doppler, size) as the
    oracle builds it (orc.voigt_grid, the plain-C restatement of vprofile.grid): NumPy arrays,
    read-only.  Parity tests of the extinction hand THIS table to the oracle, not the one the
    GPU built, so that a wrong table cell cannot hide behind both sides reading it.  The last
    grid is kept: configurations that share a width grid reuse it, and at full size one table
    is up to 1.9 GB."""
    lorentz = np.ascontiguousarray(voigt['lorentz'], np.float64)
    doppler = np.ascontiguousarray(voigt['doppler'], np.float64)
    size_in = np.asarray(voigt['size'])
    key = (lorentz.tobytes(), doppler.tobytes(), size_in.shape,
           size_in.astype(np.int64).tobytes(), float(ownstep))
    if key not in _ORACLE_TABLE:
        _ORACLE_TABLE.clear()
        size = size_in.astype(np.int32)
        index = np.zeros_like(size)
        profile = np.zeros(int(np.sum(2 * size[size > 0].astype(np.int64) + 1)))
        orc.voigt_grid(profile, size, index, lorentz, doppler, float(ownstep))
        for a in (profile, size, index):
            a.flags.writeable = False
        _ORACLE_TABLE[key] = (profile, size, index)
    return _ORACLE_TABLE[key]


def oracle_voigt_rows(orc, lorentz, doppler, size, dwn, grid=None):
    """The oracle's table one Lorentz row at a time (host memory stays near one row):
    yields (m, start, profile_row, size_row, index_row) with index_row in the whole table's
    numbering.  grid = orc.voigt_grid or a function of the same signature (the compiled
    reference's vprofile.grid without its trailing `verb`)."""
    grid = grid or orc.voigt_grid
    size = np.asarray(size)
    start = 0
    for m in range(size.shape[0]):
        srow = size[m:m + 1].astype(np.int32)
        irow = np.zeros_like(srow)
        prow = np.zeros(int(np.sum(2 * srow[srow > 0].astype(np.int64) + 1)))
        grid(prow, srow, irow, np.ascontiguousarray(lorentz[m:m + 1], np.float64),
             np.ascontiguousarray(doppler, np.float64), float(dwn))
        yield m, start, prow, srow[0], irow[0] + start
        start += prow.size


def compare_voigt_tables(got_row, want_rows, regimes, rtol):
    """Compare a table with the rows of oracle_voigt_rows: for every row the same size and
    index, the same zero pattern and every sample within rtol.  got_row(m, start, n) returns
    (profile_row, size_row, index_row) of the table under test.  Returns the worst relative
    error and the number of cells per regime (regimes: voigt_regimes of the input sizes) and
    the number of samples compared."""
    worst = {'quick': 0.0, 'mean': 0.0, 'simpson': 0.0}
    count = {'quick': 0, 'mean': 0, 'simpson': 0}
    total = 0
    for m, start, want, wsize, windex in want_rows:
        got, gsize, gindex = got_row(m, start, want.size)
        assert np.array_equal(gsize, wsize), f'row {m}: size differs'
        assert np.array_equal(gindex, windex), f'row {m}: index differs'
        assert got.shape == want.shape, f'row {m}: {got.shape} samples, want {want.shape}'
        assert np.array_equal(got == 0, want == 0), f'row {m}: zero pattern differs'
        rel = np.zeros(want.size)
        nz = want != 0
        rel[nz] = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
        cells = np.flatnonzero(regimes[m] != '')
        per_cell = np.maximum.reduceat(rel, windex[cells] - start)
        for n, err in zip(cells, per_cell):
            kind = regimes[m, n]
            worst[kind] = max(worst[kind], float(err))
            count[kind] += 1
            assert err <= rtol, f'cell ({m}, {n}), {kind}: relative error {err:.3e} > {rtol:.0e}'
        total += want.size
    return worst, count, total


# ---------------------------------------------------------------------------
# The cloud walker batch (pb_clouds.hip) at the kernel boundary: test_gpu_batch_clouds_boundary.py
# runs these cases on the device, test_batch_clouds_cases_cpu.py checks on the oracle alone that
# they are the situations their names say
# ---------------------------------------------------------------------------
CLOUD_RSTAR = 8.8e10
CLOUD_MAXDEPTH = 10.0
# (L, itop, W)
CLOUD_TRANSIT_SHAPES = [(1, 0, 1), (2, 1, 256), (2, 0, 255), (17, 0, 257), (33, 2, 700),
                        (80, 0, 600), (384, 0, 130), (385, 0, 130), (400, 15, 130), (1024, 0, 64)]
CLOUD_EMISSION_SHAPES = [(1, 0, 1), (2, 1, 256), (2, 0, 255), (17, 0, 257), (51, 3, 402),
                         (130, 0, 300)]
CLOUD_NMU = [1, 5, 8, 9, 16]


def oracle_patchy(orc, geom, ec, ec_cloud, radius, itop, maxdepth, deck, temp=None, wn=None,
                  mu=None, weights=None, rstar=CLOUD_RSTAR):
    """The oracle chain of one walker with a deck and / or patchy clouds
    (test_patchy_golden.py::test_oracle_patchy): optical_depth_transit -> transmission_deck, or
    plane_parallel_optical_depth -> emission_deck with the deck's temperature in row deck_itop
    for both columns.  -> (clear, cloudy, ideep_clear, ideep_cloudy); deck = (itop, rsurf or
    tsurf ...) as (itop, rsurf, tsurf), or None."""
    L, W = ec.shape
    ec_cloudy = ec.copy()
    if ec_cloud is not None:
        ec_cloudy[itop:] += ec_cloud[itop:]
    ibottom = L if deck is None else int(deck[0]) + 1
    if geom == 'transit':
        depth, ideep = orc.optical_depth_transit(ec_cloudy, radius, itop, ibottom, maxdepth)
        cloudy = orc.transmission_deck(depth, radius, rstar, ideep, itop,
                                       None if deck is None else float(deck[1]),
                                       None if deck is None else int(deck[0]))
        depth_c, ideep_c = orc.optical_depth_transit(ec, radius, itop, L, maxdepth)
        clear = orc.transmission_deck(depth_c, radius, rstar, ideep_c, itop, None, None)
        return clear, cloudy, ideep_c, ideep
    h = -orc.ediff(radius)
    depth, ideep = np.zeros((L, W)), np.full(W, L - 1, np.int32)
    orc.plane_parallel_optical_depth(depth, ideep, ec_cloudy, h, maxdepth, itop, ibottom)
    depth_c, ideep_c = np.zeros((L, W)), np.full(W, L - 1, np.int32)
    orc.plane_parallel_optical_depth(depth_c, ideep_c, ec, h, maxdepth, itop, L)
    # (itop == L - 1: the depth loop leaves at L; the reference clips to the last layer before it
    # forms the intensity, as cases.emission_oracle does)
    ideep, ideep_c = np.minimum(ideep, L - 1), np.minimum(ideep_c, L - 1)
    if deck is None:
        cloudy = orc.emission_deck(depth, ideep, wn, temp, mu, weights, itop, None, None)
        clear = orc.emission_deck(depth_c, ideep_c, wn, temp, mu, weights, itop, None, None)
        return clear, cloudy, ideep_c, ideep
    cloudy = orc.emission_deck(depth, ideep, wn, temp, mu, weights, itop, float(deck[2]),
                               int(deck[0]))
    # the reference's cloudy pass has overwritten row deck_itop of its Planck array in place
    # (spectrum/radiative_transfer.py:125-126); its clear pass integrates that array
    temp_clear = temp.copy()
    temp_clear[int(deck[0])] = float(deck[2])
    clear = orc.emission_deck(depth_c, ideep_c, wn, temp_clear, mu, weights, itop, None, None)
    return clear, cloudy, ideep_c, ideep


def cloud_row_block(nrow):
    """Rows of ray path per block of k_cloudy_transit: 16 while 16 rows of nrow segments fit in
    48 KiB of LDS (nrow <= 384), else 8."""
    return 16 if nrow * 16 * 8 <= 48 * 1024 else 8


def cloud_decks(L, itop, krows):
    """The deck layers of a batch of six walkers: at itop (row 0 of the first row block); above
    itop (itop = 0: inside the first row block instead); on each side of the first row-block
    boundary (rows krows - 1, the last of the first block, and krows); inside the last row block;
    at L - 1.  Clipped to the grid where the shape is smaller than that."""
    nrow = L - itop
    last_block = itop + ((nrow - 1) // krows) * krows
    want = [itop, itop - 1 if itop > 0 else itop + 2, itop + krows - 1, itop + krows,
            min(last_block + 1, L - 2), L - 1]
    return np.clip(want, 0, L - 1).astype(np.int32)


_CLOUD_CASES, _CLOUD_ORACLE = {}, {}


def cloud_case(orc, geom, L, itop, W, nr, nw=6, cache=True):
    """nw walkers for cloudy_transit_batch / cloudy_emission_batch at one shape: per-walker ec,
    radius, temperatures, deck (cloud_decks) and patchy fraction, nr rank-1 cloud terms (nr = 1:
    one cross-section row for all walkers; nr = 2: a row per walker, the second term confined to
    the middle half of the layers like a gray cloud).

    The opacities are scaled column by column from the oracle's own depths of walker 0 (maxdepth =
    inf): column j crosses CLOUD_MAXDEPTH at row 1 + (7 j + 3) mod (nrow - 1) -- every row block
    gets crossings -- and every fifth column stays below 0.2 CLOUD_MAXDEPTH down to the bottom
    (0.3 with the most opaque walker: it never crosses).  The other walkers are up to 1.4 times
    more or less opaque.  Transit (80, 0, 600): columns 0 ... 255, the first workgroup, cross at
    rows 2 ... 9 instead, so that it alone leaves before the second row block.
    ec, radius and temperatures do not depend on nr.  The arrays are read-only."""
    key = (geom, L, itop, W, nr, nw)
    if cache and key in _CLOUD_CASES:
        return _CLOUD_CASES[key]
    rng = np.random.default_rng([L, itop, W, geom == 'emission'])
    nrow = L - itop
    press = np.logspace(-6, 2, L) if L > 1 else np.ones(1)
    radius = np.linspace(8.0e9, 7.0e9, L)[None] * (1 + 0.01 * rng.uniform(-1, 1, (nw, 1))) + \
        np.linspace(0, 1, L)[None] * 2e7 * rng.uniform(-1, 1, (nw, 1))
    assert np.all(np.diff(radius, axis=1) < 0)
    temps = np.linspace(900.0, 1900.0, L)[None] * (1 + 0.1 * rng.uniform(-1, 1, (nw, 1))) + \
        rng.uniform(-20, 20, (nw, L))
    wn = np.linspace(2000.0, 9000.0, W) if W > 1 else np.array([2000.0])
    profile = press**0.9
    base = profile[:, None] * rng.uniform(0.8, 1.2, (L, W))
    colscale = np.full(W, 1e-10)
    first_group = geom == 'transit' and (L, itop, W) == (80, 0, 600)
    if nrow > 1:
        if geom == 'transit':
            depth, _ = orc.optical_depth_transit(base, radius[0], itop, L, np.inf)
        else:
            depth, stop = np.zeros((L, W)), np.zeros(W, np.int32)
            orc.plane_parallel_optical_depth(depth, stop, base, -orc.ediff(radius[0]), np.inf,
                                             itop, L)
        cols = np.arange(W)
        target = itop + 1 + (7 * cols + 3) % (nrow - 1)
        never = cols % 5 == 4
        if first_group:
            target[:256] = itop + 2 + cols[:256] % 8
            never[:256] = False
        colscale = np.where(never, 0.2 * CLOUD_MAXDEPTH / depth[L - 1, cols],
                            1.05 * CLOUD_MAXDEPTH / depth[target, cols])
    wscale = 10.0**rng.uniform(-0.15, 0.15, nw)
    wscale[0] = 1.0
    ec = base[None] * colscale[None, None, :] * wscale[:, None, None]
    krows = cloud_row_block(nrow) if geom == 'transit' else 16
    deck_itop = cloud_decks(L, itop, krows)[:nw]
    up = np.maximum(deck_itop - 1, 0)
    walkers = np.arange(nw)
    rsurf = radius[walkers, deck_itop] + 0.4 * (radius[walkers, up] - radius[walkers, deck_itop])
    tsurf = temps[walkers, deck_itop] + 0.4 * (temps[walkers, up] - temps[walkers, deck_itop])
    fpatchy = rng.uniform(0.05, 0.95, nw)
    cs = cf = None
    if nr:
        crng = np.random.default_rng([L, itop, W, geom == 'emission', nr])
        shape = (nr, W) if nr == 1 else (nr, nw, W)
        cs = crng.uniform(0.5, 1.5, shape) * colscale
        cf = profile[None, :, None] * crng.uniform(0.2, 1.0, (nw, 1, nr))
        if nr > 1:
            cf[:, :L // 4, 1] = 0.0
            cf[:, L - L // 4:, 1] = 0.0
    c = dict(key=key, geom=geom, L=L, itop=itop, W=W, nr=nr, nw=nw, krows=krows, ec=ec,
             radius=radius, temps=temps, wn=wn, deck_itop=deck_itop, rsurf=rsurf, tsurf=tsurf,
             fpatchy=fpatchy, cs=cs, cf=cf, rstar=CLOUD_RSTAR, first_group=first_group)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    if cache:
        _CLOUD_CASES[key] = c
    return c


def cloud_ec(c, w):
    """ec_cloud[L, W] of walker w: sum_m cs_m (x) f_m in the models' order, or None."""
    if c['cs'] is None:
        return None
    out = np.zeros(c['ec'].shape[1:])
    for m in range(c['cf'].shape[2]):
        row = c['cs'][m] if c['cs'].ndim == 2 else c['cs'][m, w]
        out += np.outer(c['cf'][w, :, m], row)
    return out


def cloud_oracle(orc, c, maxdepth, use_deck, mu=None, weights=None, walkers=None):
    """oracle_patchy for the walkers of a cloud_case -> dict w -> (clear[W], cloudy[W],
    ideep_clear[W], ideep_cloudy[W]).  Kept per (case, maxdepth, deck, quadrature) when the case
    is one of cloud_case's own (c['key']); a modified copy drops its key and is computed anew."""
    key = None
    if c.get('key') is not None:
        key = (c['key'], float(maxdepth), bool(use_deck),
               None if mu is None else (tuple(mu), tuple(weights)))
    have = _CLOUD_ORACLE.setdefault(key, {}) if key is not None else {}
    out = {}
    for w in range(c['nw']) if walkers is None else walkers:
        if w not in have:
            deck = (c['deck_itop'][w], c['rsurf'][w], c['tsurf'][w]) if use_deck else None
            with np.errstate(all='ignore'):
                have[w] = oracle_patchy(orc, c['geom'], c['ec'][w], cloud_ec(c, w), c['radius'][w],
                                        c['itop'], maxdepth, deck, c['temps'][w], c['wn'], mu,
                                        weights, c['rstar'])
        out[w] = have[w]
    return out


def cloud_regimes(ideep_clear, deck_itop):
    """Per walker: does the deck decide 'all', 'some' or 'none' of its columns (it lies above every
    clear crossing, above some, below all)?  ideep_clear: dict w -> ideep[W]."""
    out = []
    for w, ideep in ideep_clear.items():
        above = deck_itop[w] < ideep
        out.append('all' if above.all() else 'some' if above.any() else 'none')
    return out


def cloud_modified(c, **arrays):
    """A writable copy of a cloud_case with some arrays replaced (no key: not cached)."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    out.update(arrays)
    out['key'] = None
    return out


def cloud_quadrature9(mu8, weights8):
    """The eight nodes with a ninth of weight zero (mu = 0.5): k_cloudy_emission<16> on the same
    sums as k_cloudy_emission<8>."""
    return np.append(mu8, 0.5), np.append(weights8, 0.0)


# test_special_values: (name, maxdepth); the special walker is walker 2 of six
CLOUD_SPECIAL_EMISSION = [('ec_inf', CLOUD_MAXDEPTH), ('deep', np.inf), ('t_zero', CLOUD_MAXDEPTH),
                          ('tsurf_zero', CLOUD_MAXDEPTH), ('tsurf_nan', CLOUD_MAXDEPTH)]
CLOUD_SPECIAL_TRANSIT = [('ec_inf', 0), ('cloud_inf', 1)]          # (name, nr)
CLOUD_SPECIAL_SHAPE = (33, 2, 300)
CLOUD_SPECIAL_WALKER = 2
CLOUD_SPECIAL_LAYER = 9         # row 7 of the first row block of 16 (itop = 2)


def cloud_special_case(orc, geom, name):
    """-> (base case, the case with walker CLOUD_SPECIAL_WALKER made special).  Emission (nr = 2):
    'ec_inf' a layer of ec = +inf; 'deep' ec x 1e7, depths far above 1e5 (run with maxdepth =
    inf, the kernel's clamp_depth); 't_zero' a layer at T = 0; 'tsurf_zero' / 'tsurf_nan' the
    deck's temperature (the walker's deck lies inside the grid, above most clear crossings).
    Transit: 'ec_inf' (nr = 0) ec = +inf in a layer in the middle of a row block; 'cloud_inf'
    (nr = 1) one infinite cloud factor there."""
    L, itop, W = CLOUD_SPECIAL_SHAPE
    nr = dict(CLOUD_SPECIAL_TRANSIT)[name] if geom == 'transit' else 2
    base = cloud_case(orc, geom, L, itop, W, nr)
    w, lay = CLOUD_SPECIAL_WALKER, CLOUD_SPECIAL_LAYER
    c = cloud_modified(base)
    if name == 'ec_inf':
        c['ec'][w, lay] = np.inf
    elif name == 'cloud_inf':
        c['cf'][w, lay, 0] = np.inf
    elif name == 'deep':
        c['ec'][w] *= 1e7
    elif name == 't_zero':
        c['temps'][w, lay] = 0.0
    elif name == 'tsurf_zero':
        c['tsurf'][w] = 0.0
    elif name == 'tsurf_nan':
        c['tsurf'][w] = np.nan
    else:
        raise ValueError(name)
    return base, c
