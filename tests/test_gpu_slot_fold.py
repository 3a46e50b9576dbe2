"""Staged gather (k_ext_staged, LDS-DMA path): the batch set-up adds the slot of a record's
segment to the record's row offset (stage_slot_off8(), pb_ext_args.h), so the walk reads every
segment from one lane address.  A record that carries the wrong slot reads another segment's row
(or a pad), so the call is made on a crafted line list whose batches hold the shapes at which the
slot of a record can go wrong, each asserted on the host from the line list, the table's sizes and
the device's rules for a line's cell (restated below):

  * layers of two rows per step and layers of one in the same launch (the Lorentz rows that the
    two deepest layers select hold profiles too long for four slots), and two isotopes of different
    longest rows in every layer, so the pitch changes between the isotopes of a workgroup;
  * strong lines (live records) alternating with lines below `ethresh` (dead records) on one
    phase: every strong line is a segment of its own with a dead segment before the next, the
    live-segment index differs from the count of segment starts, and one batch holds more than 64
    segments (hit words renewed mid-batch, slot parity across a block of 64);
  * a tile with more than 512 live records: two batches, slot numbering restarts in the second,
    and the batch boundary cuts the range of one phase; phases with no candidate lie between
    the others; batches with an odd number of segments;
  * runs of live records on one phase that form segments of many records.

Checks: the oracle in every layer (rtol 1e-10, same zero pattern, as test_gpu_extinction.py); the
same bits from PB_STAGE_DMA=0 (rows via registers: the buffer's offset added per segment, not per
record), PB_STAGE_ROWS=1, PB_STAGE_SPLIT=3, PB_STAGE_S=1 and from calls that begin at samples 1, 64
and 130; rows of 1201 samples (chunked rows, more virtual phases than
phases) through the one-row instance.  One cell that no layer selects holds a long profile: the
row area is sized by the table's longest row, and only then does it hold four slots.
Needs an MI355X."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-10
SPAN, WAVES, S = 256, 8, 2           # kStageSpan, kStagedWaves, PB_STAGE_S of the base call
TILE = S * WAVES * SPAN
THREADS = WAVES * 64                 # records of a batch
K_B, AMU, C_LIGHT = 1.380658e-16, 1.66053886e-24, 2.99792458e10      # pb_common.h
SQRT_LN2 = 0.83255461115769775635
LONG_HALF = 2100                     # half-length of the one long profile, fine samples
ETHRESH = 1e-4
STRONG, WEAK = 1e-8, 1e-15           # gf: a weak line is 1e-7 of a strong one, below ETHRESH even
                                     # for the main isotope against the minor one (ratio 2e-3)


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


def layer_rows(case):
    """(ilor[L, niso], alphad[L, niso]): the Lorentz row and the Doppler width per unit
    wavenumber of every (layer, isotope), as k_layer_state (pb_ext_records.hip) forms them."""
    atm, iso, vg = (case[k] for k in ('atm', 'iso', 'voigt'))
    niso = len(iso['isomass'])
    ilor = np.zeros((atm['nlayers'], niso), int)
    alphad = np.zeros((atm['nlayers'], niso))
    for layer in range(atm['nlayers']):
        temp = atm['temp'][layer]
        flor = np.sqrt(2 * K_B * temp / np.pi / AMU) / C_LIGHT
        for i in range(niso):
            dia = atm['mol_radius'][iso['isoimol'][i]] + atm['mol_radius']
            alphal = flor * np.sum(atm['dens'][layer] * dia * dia *
                                   np.sqrt(1 / iso['isomass'][i] + 1 / atm['mol_mass']))
            ilor[layer, i] = nearest_index(vg['lorentz'], alphal)
            alphad[layer, i] = (np.sqrt(2 * K_B * temp / AMU) * SQRT_LN2 / C_LIGHT
                                / np.sqrt(iso['isomass'][i]))
    return ilor, alphad


def line_plan():
    """[(tile, isotope, phase, [(sample within the tile, live)])]: see the module docstring."""
    alt = lambda n, first, step: [(first + step * i, i % 2 == 0) for i in range(n)]
    run = lambda n, first, step: [(first + step * i, True) for i in range(n)]
    # PB_STAGE_SPLIT=3 gives the phases 0-3, 4-7 and 8-11 to three workgroups whose sums are added
    # afterwards: the same bits only where no sample has terms from two of them, so the lines of
    # the three groups of phases keep to sample ranges more than two windows apart.
    return [
        # tile 0, isotope 0: 139 + 300 + 6 + 150 + 5 = 600 candidates, 526 live
        (0, 0, 0, alt(139, 700, 18)),           # 70 live segments, a dead one between any two
        (0, 0, 3, run(300, 700, 8)),            # long segments: trips of four records
        (0, 0, 5, [(3720, True), (3723, True), (3726, True), (3729, False), (3732, True),
                   (3735, True)]),
        (0, 0, 7, run(150, 3400, 2)),           # cut by the batch boundary at 512 candidates
        (0, 0, 11, alt(5, 300, 40)),
        # tile 0, isotope 1: three segments of one record and one of ten
        (0, 1, 4, alt(5, 3400, 30)),
        (0, 1, 9, run(10, 500, 7)),
        # tile 1: a few segments per isotope
        (1, 0, 6, [(900, True), (904, True), (908, False), (912, True)]),
        (1, 1, 2, alt(5, 300, 25)),             # three segments: an odd count
    ]


def crafted_case():
    """-> (case, lines) with lines = [(isotope, fine-grid index, live)] in the order of the plan."""
    from pyratbay_amd import synth
    case = synth.lbl_case(9001, 5, 100, wnstep=0.05, wnosamp=12, nlor=8, ndop=4, extent=60.0,
                          cutoff=1.0, niso=2, seed=5, ptop=0.3, pbottom=30.0,
                          iso_masses=(18.0, 300.0))
    g, vg = case['grid'], case['voigt']
    osamp = g['wnosamp']
    # The table's sizes, by hand: half-lengths that grow with the Doppler column, so two isotopes
    # that can select different columns have different longest rows; long ones (1 row per step) in
    # the Lorentz rows of the two deepest layers, short ones (2 rows per step) elsewhere; one
    # profile of LONG_HALF fine samples in a Lorentz row that no layer selects, which sizes the area.
    ilor, _ = layer_rows(case)
    deep = set(ilor[-2:].ravel().tolist())
    assert not deep & set(ilor[:-2].ravel().tolist()), ilor
    size = np.asarray(vg['size'])
    for r in range(size.shape[0]):
        size[r] = (400 if r in deep else 60) + 48 * np.arange(size.shape[1])
    free = [r for r in range(size.shape[0]) if r not in set(ilor.ravel().tolist())]
    assert free, ilor
    size[free[-1], 0] = LONG_HALF
    vg['size'] = size
    lwn, elow, gf, lid, lines = [], [], [], [], []
    for tile, iso, phase, members in line_plan():
        for sample, live in members:
            i = (tile * TILE + sample) * osamp + phase
            lines.append((iso, i, live))
            lwn.append(g['own'][i])
            elow.append(1000.0)
            gf.append(STRONG if live else WEAK)
            lid.append(iso)
    # sorted by isotope, then wavenumber, as the line-list reader returns them
    order = np.lexsort((lwn, lid))
    case['lines'] = dict(lwn=np.asarray(lwn)[order], elow=np.asarray(elow)[order],
                         gf=np.asarray(gf)[order], lid=np.asarray(lid, np.int32)[order])
    case['ethresh'] = ETHRESH
    return case, lines


def batch_shapes(case, lines, layer):
    """The batches of every (tile, isotope) of the call at wbegin 0, S = 2, one workgroup per tile:
    [dict(tile, iso, phases = phase of every record of the batch, segs = [live?] of the batch's
    segments in order)].  The candidates of a (tile, isotope) are its lines in (phase, position)
    order (every line of the plan lies at least 300 samples inside its tile, farther than any
    profile reaches); a batch is the next 512 of them; a segment is a run of live records of one
    (cell, phase), or a run of dead ones."""
    g, vg = case['grid'], case['voigt']
    osamp = g['wnosamp']
    ilor, alphad = layer_rows(case)
    out = []
    for tile in range((g['nwave'] + TILE - 1) // TILE):
        for iso in range(2):
            cand = sorted((i % osamp, i, live) for k, i, live in lines
                          if k == iso and i // osamp // TILE == tile)
            for x0 in range(0, len(cand), THREADS):
                segs, keys = [], []
                for phase, i, live in cand[x0:x0 + THREADS]:
                    cell = nearest_index(vg['doppler'], alphad[layer, iso] * g['own'][i])
                    key = (cell, phase) if live else None
                    if not keys or key != keys[-1]:
                        keys.append(key)
                        segs.append(live)
                out.append(dict(tile=tile, iso=iso, segs=segs, x0=x0, ncand=len(cand),
                                phases=[p for p, _, _ in cand[x0:x0 + THREADS]],
                                live=sum(l for _, _, l in cand[x0:x0 + THREADS])))
    return out


class Plan:
    """One synthetic case on the device with a staged-gather plan and its inputs."""

    def __init__(self, eng, case, niso):
        g, atm, iso, vg, ln = (case[k] for k in ('grid', 'atm', 'iso', 'voigt', 'lines'))
        self.case, self.nl, self.nwave, self.niso = case, atm['nlayers'], g['nwave'], niso
        self.vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                                       g['wnosamp'])
        self.ll = eng.LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'], niso, g['own'])
        self.lbl = eng.LBL(self.vt, self.ll, g['wn'], g['divisors'], atm['mol_radius'],
                           atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                           iso['isoiext'], vg['cutoff'], case['ethresh'], max_layers=self.nl)
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
        g, atm, ln, iso, vg = (self.case[k] for k in ('grid', 'atm', 'lines', 'iso', 'voigt'))
        profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
        want = np.zeros((self.nl, g['nwave']))
        for layer in range(self.nl):
            row = np.zeros((1, g['nwave']))
            orc.extinction(row, profile, size, index, vg['lorentz'], vg['doppler'],
                           g['wn'], g['own'], g['divisors'], atm['dens'][layer],
                           atm['mol_radius'], atm['mol_mass'], iso['isoimol'], iso['isomass'],
                           iso['isoratio'], iso['isoz'][:, layer].copy(), iso['isoiext'],
                           ln['lwn'], ln['elow'], ln['gf'], ln['lid'], vg['cutoff'],
                           self.case['ethresh'], atm['temp'][layer], 0, 1, 0)
            want[layer] = row[0]
        return want


def check_oracle(got, want, what):
    worst = 0.0
    for layer in range(len(want)):
        assert np.array_equal(got[layer, 0] == 0, want[layer] == 0), (what, layer)
        nz = want[layer] != 0
        worst = max(worst, np.max(np.abs(got[layer, 0][nz] / want[layer][nz] - 1)))
        np.testing.assert_allclose(got[layer, 0], want[layer], rtol=RTOL)
    print(f'slot fold, {what}: max rel err vs oracle = {worst:.2e}')


BASE = dict(PB_STAGE_S=S, PB_STAGE_SPLIT=1)


@pytest.fixture(scope='module')
def crafted(eng):
    """(Plan, lines, (ec, rows per step) of the base call): computed once, left unchanged."""
    case, lines = crafted_case()
    p = Plan(eng, case, 2)
    ext, rows = p.run(**BASE)
    ext.flags.writeable = False
    return p, lines, (ext, rows)


def test_the_shapes_occur(crafted):
    """What the other tests rest on: see the module docstring."""
    p, lines, (ext, rows) = crafted
    case = p.case
    g, vg = case['grid'], case['voigt']
    osamp, size = g['wnosamp'], np.asarray(vg['size'])
    print(f'rows per step [layer][isotope] {rows.tolist()}')
    assert p.nwave > 2 * TILE
    # rows per step: one and two in the same launch
    assert (rows[:-2] == 2).all() and (rows[-2:] == 1).all(), rows
    ilor, alphad = layer_rows(case)
    assert LONG_HALF not in size[np.unique(ilor)], 'a layer selects the long profile'
    # every profile reaches less than the 300 samples that the lines keep from the tile edges
    # (the candidate search adds the grid's oversampling twice and a few samples to the half-length)
    assert size[np.unique(ilor)].max() / osamp + 2 * osamp + 8 < 300
    for layer in range(p.nl):
        # the Doppler columns an isotope can select (k_layer_state): the longest rows differ
        longest = []
        for iso in range(2):
            dlo = max(0, nearest_index(vg['doppler'], alphad[layer, iso] * g['own'][0]) - 1)
            dhi = min(size.shape[1] - 1,
                      nearest_index(vg['doppler'], alphad[layer, iso] * g['own'][-1]) + 1)
            longest.append(size[ilor[layer, iso], dlo:dhi + 1].max())
        assert longest[0] - longest[1] >= 2 * osamp, (layer, longest)
        batches = batch_shapes(case, lines, layer)
        nlive = [sum(b['segs']) for b in batches]
        print(f'layer {layer}: live segments per batch {nlive}, longest rows {longest}')
        assert any(n % 2 == 1 for n in nlive), 'a batch with an odd number of segments'
        assert any(n > 64 for n in nlive), 'hit words renewed inside a batch'
        # a tile with more than a batch of live records, in batches that both hold live segments
        t0 = [b for b in batches if b['tile'] == 0 and b['iso'] == 0]
        assert len(t0) == 2 and sum(b['live'] for b in t0) > THREADS
        assert all(sum(b['segs']) > 0 for b in t0)
        # the batch boundary cuts the range of a phase
        assert t0[0]['phases'][-1] == t0[1]['phases'][0]
        # a dead segment between two live ones
        assert any(b['segs'][i - 1] and not b['segs'][i] and b['segs'][i + 1]
                   for b in batches for i in range(1, len(b['segs']) - 1))
        # phases without a candidate between phases that have some
        for b in batches:
            have = sorted(set(b['phases']))
            if len(have) > 1:
                assert any(q - p_ > 1 for p_, q in zip(have, have[1:])), have
        # segments of many records: trips of four and the records left
        assert any(b['live'] - sum(b['segs']) >= 100 for b in batches)


def test_base_call_vs_oracle(crafted, orc):
    p, lines, (ext, rows) = crafted
    check_oracle(ext, p.oracle(orc), 'crafted batches')


@pytest.mark.parametrize('env', [dict(PB_STAGE_DMA=0), dict(PB_STAGE_ROWS=1),
                                 dict(PB_STAGE_SPLIT=3), dict(PB_STAGE_S=1)],
                         ids=lambda e: '-'.join(f'{k}={v}' for k, v in e.items()))
def test_other_paths_give_every_bit(crafted, env):
    import torch
    p, lines, (want, rows) = crafted
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() > 0
    got, rows1 = p.run(**{**BASE, **env})
    if 'PB_STAGE_ROWS' in env or 'PB_STAGE_DMA' in env:
        assert (rows1 == 1).all()
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(np.array(want)))


@pytest.mark.parametrize('wbegin', [1, 64, 130])
def test_calls_that_begin_inside_the_grid(crafted, wbegin):
    """A call at wbegin moves the tiles and spans by wbegin samples against the lines."""
    import torch
    p, lines, (want, rows) = crafted
    got, _ = p.run(wbegin=wbegin, **BASE)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(np.array(want[:, :, wbegin:])))
    reg, _ = p.run(wbegin=wbegin, **BASE, PB_STAGE_DMA=0)
    assert torch.equal(torch.from_numpy(reg), torch.from_numpy(got))


def test_long_rows(eng, orc):
    """Rows of 1201 samples: chunks of 1024 through the one-row instance, (phase, chunk) pairs as
    virtual phases, the bits of the register path, and the oracle."""
    import torch
    from pyratbay_amd import synth
    case = synth.lbl_case(6001, 6, 1500, wnstep=0.05, wnosamp=12, nlor=8, ndop=4, extent=300.0,
                          cutoff=30.0, niso=2, seed=12, ptop=0.1, pbottom=100.0)
    case['ethresh'] = 1e-30
    assert (2 * np.asarray(case['voigt']['size']).max() + 1) // 12 + 1 > 1024
    p = Plan(eng, case, 2)
    got, rows = p.run(**BASE)
    assert (rows == 1).all()
    reg, _ = p.run(**BASE, PB_STAGE_DMA=0)
    assert torch.equal(torch.from_numpy(reg), torch.from_numpy(got))
    check_oracle(got, p.oracle(orc), 'long rows')
