"""Staged gather, the walk of one (segment, sub-tile) pair (k_ext_staged): a pair's hit word holds
the address of its first record, the bytes of its four-record trips and the 0-3 records left after
them; the trips loop on the record address, the records left are visited by straight-line code (one
if the count is odd, then two).  A record dropped, repeated or visited out of its pair shows in the
sums, so the call is made on a line list of crafted CLUSTERS: cluster n is n lines of equal gf and
elow on one fine-grid phase, three output samples apart, centred in one 256-sample span, with
windows of at most 41 samples -- one segment whose pair for that span holds exactly n records.
The spans of tile 0 hold n = 1 ... 8 in sub-tile 0 (samples below 2048) and 2 ... 8 in sub-tile 1;
tile 1 holds 9 in sub-tile 0 and 1 and 9 in sub-tile 1; a cluster of three straddles the edge
between the tiles, every window clipped by it.  The counts are asserted on the host from the
table's sizes and the device's rules for the cell and the window of a line (restated below), not
assumed.  One cell of the table that no layer selects holds a long profile: the row area is sized
by the table's longest row, and only then does it hold the four slots of two rows per step.

  0 empty pair | 1, 2, 3 the records left alone | 4 one trip, nothing left | 5, 6, 7 a trip and
  each count left | 8 two trips | 9 two trips and one

Checks: the oracle in every layer (same zero pattern, rtol 1e-10 as test_gpu_extinction.py: with
equal strengths in a cluster a dropped or repeated record shows at 1/n); the same bits from
PB_STAGE_ROWS=1 (one row per step: the other step loop), PB_STAGE_DMA=0 (rows via registers),
PB_STAGE_SPLIT=3, PB_STAGE_S=1 (every pair in sub-tile 0) and from calls that begin at samples 1,
64, 130 and 200, which move every cluster against the span grid until a cluster of n is n1 + n2
records in two spans.  The long case (rows of 1201 samples) runs the chunked rows through the
one-row instance.  Needs an MI355X."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-10
SPAN = 256                       # kStageSpan: samples of a wavefront in a sub-tile
WAVES = 8                        # kStagedWaves
S = 2                            # PB_STAGE_S of every call but one
TILE = S * WAVES * SPAN
STAGE_ROW_MAX = 1024             # kStageRowMax
K_B, AMU, C_LIGHT = 1.380658e-16, 1.66053886e-24, 2.99792458e10      # pb_common.h
SQRT_LN2 = 0.83255461115769775635
STEP = 3                         # output samples between the lines of a cluster
LONG_HALF = 2100                 # half-length of the one long profile of the table, fine samples


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def nearest_index(a, v):
    """pb::nearest_index (pb_common.h) over the whole array."""
    lo, hi = 0, len(a) - 1
    while hi - lo > 1:
        mid = (hi + lo) // 2
        if a[mid] > v:
            hi = mid
        else:
            lo = mid
    return hi if abs(a[hi] - v) < abs(a[lo] - v) else lo


def cluster_plan():
    """[(n, first sample of the span it is centred in or None, centre sample)]: see the module
    docstring.  The edge cluster is centred on the first sample of tile 1."""
    plan = []
    for w in range(8):                                   # tile 0, sub-tile 0: 1 ... 8
        plan.append((w + 1, w * SPAN))
    for w in range(7):                                   # tile 0, sub-tile 1: 2 ... 8
        plan.append((w + 2, WAVES * SPAN + w * SPAN))
    plan.append((9, TILE + 1 * SPAN))                    # tile 1, sub-tile 0
    plan.append((1, TILE + WAVES * SPAN))                # tile 1, sub-tile 1
    plan.append((9, TILE + WAVES * SPAN + 1 * SPAN))
    out = [(n, s0, s0 + SPAN // 2) for n, s0 in plan]
    out.append((3, None, TILE))
    return out


def crafted_case():
    """The small case with its line list replaced by the clusters; -> (case, clusters) with
    clusters = [(n, span start or None, [fine-grid index of every line])]."""
    from pyratbay_amd import synth
    case = synth.lbl_case(9001, 5, 100, wnstep=0.05, wnosamp=12, nlor=8, ndop=4, extent=60.0,
                          cutoff=1.0, niso=1, seed=5, ptop=0.3, pbottom=30.0)
    g = case['grid']
    osamp = g['wnosamp']
    # Two rows per step need a row area of four slots (stage_slots(), pb_ext_args.h), and the area
    # is sized by the longest row of the TABLE: the cell of the widest Lorentz row, which no layer
    # selects (asserted in test_clusters_give_the_counts), gets a profile of LONG_HALF fine samples.
    case['voigt']['size'][-1, 0] = LONG_HALF
    lwn, elow, gf, clusters = [], [], [], []
    for c, (n, s0, centre) in enumerate(cluster_plan()):
        first = centre - (STEP * (n - 1)) // 2
        iown = [(first + STEP * i) * osamp + c % osamp for i in range(n)]
        clusters.append((n, s0, iown))
        lwn += [g['own'][i] for i in iown]
        elow += [1000.0 + 50.0 * c] * n
        gf += [1e-8 * (1.0 + 0.1 * c)] * n
    order = np.argsort(lwn, kind='stable')
    case['lines'] = dict(lwn=np.asarray(lwn)[order], elow=np.asarray(elow)[order],
                         gf=np.asarray(gf)[order], lid=np.zeros(len(lwn), np.int32))
    return case, clusters


def line_halves(case, iown):
    """half[L, len(iown)]: the half-length in fine-grid samples of the profile that every layer
    selects for lines at the fine-grid positions iown, and the cell it comes from, as k_layer_state
    and k_records (pb_ext_records.hip) choose them: the Lorentz row nearest to the layer's width,
    the Doppler column nearest to the line's width; a cell of size 0 is the previous column's."""
    g, atm, iso, vg = (case[k] for k in ('grid', 'atm', 'iso', 'voigt'))
    lor, dop, size = vg['lorentz'], vg['doppler'], np.asarray(vg['size'])
    mass = iso['isomass'][0]
    half = np.zeros((atm['nlayers'], len(iown)), np.int64)
    cell = np.zeros_like(half)
    for layer in range(atm['nlayers']):
        temp = atm['temp'][layer]
        flor = np.sqrt(2 * K_B * temp / np.pi / AMU) / C_LIGHT
        dia = atm['mol_radius'][iso['isoimol'][0]] + atm['mol_radius']
        alphal = flor * np.sum(atm['dens'][layer] * dia * dia *
                               np.sqrt(1 / mass + 1 / atm['mol_mass']))
        alphad = np.sqrt(2 * K_B * temp / AMU) * SQRT_LN2 / C_LIGHT / np.sqrt(mass)
        ilor = nearest_index(lor, alphal)
        for j, i in enumerate(iown):
            d = nearest_index(dop, alphad * g['own'][i])
            while size[ilor, d] == 0:
                d -= 1
            half[layer, j] = size[ilor, d]
            cell[layer, j] = ilor * len(dop) + d
    return half, cell


def span_counts(case, clusters, layer):
    """{(cluster, span start): records}: for the call at wbegin 0, how many records of every
    cluster reach every span, by the device's rules: a line at fine-grid position i with a profile
    of half-length h covers the samples ceil((i - h) / osamp) ... floor((i + h) / osamp)
    (k_records), clipped by the tile that walks it (k_ext_staged), and reaches a span that its
    clipped window overlaps (find_hits)."""
    osamp, nwave = case['grid']['wnosamp'], case['grid']['nwave']
    out = {}
    for c, (n, s0, iown) in enumerate(clusters):
        half, cell = line_halves(case, iown)
        assert len(set(cell[layer])) == 1, f'cluster {c} is not one segment in layer {layer}'
        assert half[layer].max() < LONG_HALF, 'a layer selects the long profile'
        for i, h in zip(iown, half[layer]):
            lo, hi = -((h - i) // osamp), min((i + h) // osamp + 1, nwave)
            for tile in range((nwave + TILE - 1) // TILE):
                tlo, thi = max(lo, tile * TILE), min(hi, (tile + 1) * TILE)
                for span in range(tlo // SPAN, (thi - 1) // SPAN + 1 if thi > tlo else 0):
                    key = (c, span * SPAN)
                    out[key] = out.get(key, 0) + 1
    return out


class Plan:
    """One synthetic case on the device, with a staged-gather plan and its inputs (the harness of
    test_gpu_stage_request.py)."""

    def __init__(self, eng, case, niso):
        g, atm, iso, vg, ln = (case[k] for k in ('grid', 'atm', 'iso', 'voigt', 'lines'))
        self.eng, self.case, self.g, self.atm, self.iso, self.vg, self.ln = \
            eng, case, g, atm, iso, vg, ln
        self.nl, self.nwave, self.niso = atm['nlayers'], g['nwave'], niso
        self.vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                                       g['wnosamp'])
        self.ll = eng.LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'], niso, g['own'])
        self.lbl = eng.LBL(self.vt, self.ll, g['wn'], g['divisors'], atm['mol_radius'],
                           atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                           iso['isoiext'], vg['cutoff'], 1e-30, max_layers=self.nl)
        self.lbl.set_gather_mode('staged')
        self.t, self.d, self.z = eng.dev(atm['temp']), eng.dev(atm['dens']), eng.dev(iso['isoz'])

    def run(self, wbegin=0, **env):
        """-> (ec[L, 1, nwave - wbegin], rows per step[L, niso]); the output buffer holds a
        pattern of large negative numbers before the call."""
        import torch
        wcount = self.nwave - wbegin
        out = (-1e200 * (1 + torch.arange(self.nl * wcount, dtype=torch.float64,
                                          device=self.t.device) % 97)
               ).reshape(self.nl, 1, wcount)
        mp = pytest.MonkeyPatch()
        try:
            for k, v in env.items():
                mp.setenv(k, str(v))
            got = self.lbl.extinction(self.t, self.d, self.z, add=True, out=out, wbegin=wbegin,
                                      wcount=wcount)
            assert got.data_ptr() == out.data_ptr()
            ext = host(got)
            assert self.lbl.last_gather_kernel == 'k_ext_staged'
            rows = self.lbl.last_rows_per_step(self.nl, self.niso)
        finally:
            mp.undo()
        return ext, rows

    def oracle(self, orc):
        g, atm, ln, iso, vg = self.g, self.atm, self.ln, self.iso, self.vg
        profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
        want = np.zeros((self.nl, g['nwave']))
        for layer in range(self.nl):
            row = np.zeros((1, g['nwave']))
            orc.extinction(row, profile, size, index, vg['lorentz'], vg['doppler'],
                           g['wn'], g['own'], g['divisors'], atm['dens'][layer],
                           atm['mol_radius'], atm['mol_mass'], iso['isoimol'], iso['isomass'],
                           iso['isoratio'], iso['isoz'][:, layer].copy(), iso['isoiext'],
                           ln['lwn'], ln['elow'], ln['gf'], ln['lid'], vg['cutoff'], 1e-30,
                           atm['temp'][layer], 0, 1, 0)
            want[layer] = row[0]
        return want


def check_oracle(got, want, what):
    worst = 0.0
    for layer in range(len(want)):
        assert np.array_equal(got[layer, 0] == 0, want[layer] == 0), (what, layer)
        nz = want[layer] != 0
        worst = max(worst, np.max(np.abs(got[layer, 0][nz] / want[layer][nz] - 1)))
        np.testing.assert_allclose(got[layer, 0], want[layer], rtol=RTOL)
    print(f'walk counts, {what}: max rel err vs oracle = {worst:.2e}')


@pytest.fixture(scope='module')
def crafted(eng):
    """(Plan, clusters, (ec, rows per step) of the default call at S = 2, one workgroup per
    tile): computed once and left unchanged."""
    case, clusters = crafted_case()
    p = Plan(eng, case, 1)
    ext, rows = p.run(PB_STAGE_S=S, PB_STAGE_SPLIT=1)
    ext.flags.writeable = False
    return p, clusters, (ext, rows)


def test_clusters_give_the_counts(crafted):
    """What the other tests rest on: in every layer every cluster is one segment, cluster n puts
    exactly n records into the span it is centred in and none into any other, the edge cluster
    puts its three records into the last span of tile 0 and the first of tile 1, and between them
    the pairs of sub-tile 0 and those of sub-tile 1 hold every count from 0 to 9."""
    p, clusters, (ext, rows) = crafted
    size = np.asarray(p.vg['size'])
    halves = sorted(set(size[size > 0].tolist()))
    print(f'profile half-lengths {halves} fine samples, osamp {p.g["wnosamp"]}; '
          f'rows per step {rows.T.tolist()}')
    assert p.nwave > 2 * TILE
    for layer in range(p.nl):
        counts = span_counts(p.case, clusters, layer)
        want = {}
        for c, (n, s0, iown) in enumerate(clusters):
            if s0 is None:
                want[(c, TILE - SPAN)] = want[(c, TILE)] = n
            else:
                want[(c, s0)] = n
        assert counts == want, (layer, counts, want)
        per_sub = {0: {0}, 1: {0}}               # (most pairs of any segment are empty)
        for (c, s0), n in counts.items():
            per_sub[(s0 % TILE) // (WAVES * SPAN)].add(n)
        assert per_sub[0] >= set(range(10)) and per_sub[1] >= set(range(10)), per_sub
    assert (rows == 2).all(), 'rows this short are staged two to a step'


def test_default_call_vs_oracle(crafted, orc):
    p, clusters, (ext, rows) = crafted
    check_oracle(ext, p.oracle(orc), 'clusters')


@pytest.mark.parametrize('env', [dict(PB_STAGE_ROWS=1), dict(PB_STAGE_DMA=0),
                                 dict(PB_STAGE_SPLIT=3), dict(PB_STAGE_S=1)],
                         ids=lambda e: '-'.join(f'{k}={v}' for k, v in e.items()))
def test_control_paths_leave_every_bit(crafted, env):
    p, clusters, (want, rows) = crafted
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() > 0
    got, rows1 = p.run(**{'PB_STAGE_S': S, 'PB_STAGE_SPLIT': 1, **env})
    if 'PB_STAGE_ROWS' in env or 'PB_STAGE_DMA' in env:
        assert (rows1 == 1).all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize('wbegin', [1, 64, 130, 200])
def test_clusters_moved_against_the_spans(crafted, wbegin):
    """A call at wbegin moves the span grid by wbegin samples: at 130 and 200 every cluster lies
    across the edge of two spans, n1 + n2 records, and some across the edge of two sub-tiles or
    tiles."""
    p, clusters, (want, rows) = crafted
    got, _ = p.run(wbegin=wbegin, PB_STAGE_S=S, PB_STAGE_SPLIT=1)
    assert np.array_equal(got, want[:, :, wbegin:])
    one, _ = p.run(wbegin=wbegin, PB_STAGE_S=S, PB_STAGE_SPLIT=1, PB_STAGE_ROWS=1)
    assert np.array_equal(one, got)


def test_long_rows(eng, orc):
    """Rows of 1201 samples (make_case('long') of test_gpu_stage_request.py): chunks of 1024
    through the one-row instance, the bits of the register path, and the oracle."""
    from pyratbay_amd import synth
    case = synth.lbl_case(6001, 6, 1500, wnstep=0.05, wnosamp=12, nlor=8, ndop=4, extent=300.0,
                          cutoff=30.0, niso=2, seed=12, ptop=0.1, pbottom=100.0)
    p = Plan(eng, case, 2)
    got, rows = p.run(PB_STAGE_S=S, PB_STAGE_SPLIT=1)
    assert (rows == 1).all()
    reg, _ = p.run(PB_STAGE_S=S, PB_STAGE_SPLIT=1, PB_STAGE_DMA=0)
    assert np.array_equal(reg, got)
    check_oracle(got, p.oracle(orc), 'long rows')
