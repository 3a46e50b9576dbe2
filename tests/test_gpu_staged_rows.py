"""Staged gather, several rows per barrier step (pbhip.h: pb_lbl_rows_per_step).  Where the rows
of a (layer, isotope) are short enough for four slots in the LDS of two full rows, a step of
k_ext_staged stages and walks R = 2 consecutive segments; every lane still adds its terms in the
order of the one-row step, so the result is bit-identical to PB_STAGE_ROWS=1 (one row per step)
and to PB_STAGE_DMA=0 (rows via registers).  Needs an MI355X.

The main case has a table whose longest row reaches kStageRowMax (cutoff 25 cm-1 at a step of
0.05 cm-1: rows of 1001 samples, LDS buffers of 1002) and layers from 1e-5 to 100 bar, so that
the call holds (layer, isotope) pairs with R = 1 and with R = 2 and a layer whose two isotopes
(masses 18 and 2.5) differ in R.  That is asserted from last_rows_per_step, not assumed.
Tolerance against the oracle: that of test_gpu_extinction.py (rtol 1e-10, same zero pattern)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-10
NL, NISO, NWAVE = 8, 2, 9001
TILE = 4096                      # samples of a workgroup (S = 2 sub-tiles of 8 x 256)
BATCH = 512                      # records of a batch (one per thread)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


class Plan:
    """One synthetic case on the device, with a staged-gather plan and its inputs."""

    def __init__(self, eng, case, lines=None, max_layers=None):
        g, atm, iso, vg = (case[k] for k in ('grid', 'atm', 'iso', 'voigt'))
        ln = case['lines'] if lines is None else lines
        self.case, self.g, self.atm, self.iso, self.vg, self.ln = case, g, atm, iso, vg, ln
        self.nl = atm['nlayers']
        self.osamp = g['wnosamp']
        self.vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                                       self.osamp)
        self.ll = eng.LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'], NISO, g['own'])
        self.lbl = eng.LBL(self.vt, self.ll, g['wn'], g['divisors'], atm['mol_radius'],
                           atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                           iso['isoiext'], vg['cutoff'], 1e-30, max_layers=self.nl)
        self.lbl.set_gather_mode('staged')
        self.t, self.d, self.z = eng.dev(atm['temp']), eng.dev(atm['dens']), eng.dev(iso['isoz'])

    def run(self, monkeypatch, wbegin=0, wcount=None, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        out = host(self.lbl.extinction(self.t, self.d, self.z, add=True, wbegin=wbegin,
                                       wcount=wcount))
        assert self.lbl.last_gather_kernel == 'k_ext_staged'
        rows = self.lbl.last_rows_per_step(self.nl, NISO)
        for k in env:
            monkeypatch.delenv(k)
        return out, rows

    def rowcap(self):
        size = np.asarray(self.vt.size)
        return int(np.max((2 * size + 1 + self.osamp - 1) // self.osamp))


def main_case():
    from pyratbay_amd import synth
    return synth.lbl_case(NWAVE, NL, 4000, wnstep=0.05, wnosamp=12, nlor=14, ndop=4, cutoff=25.0,
                          niso=NISO, seed=11, ptop=1e-5, pbottom=1e2, iso_masses=(18.0, 2.5))


@pytest.fixture(scope='module')
def main(eng):
    return Plan(eng, main_case())


@pytest.fixture(scope='module')
def base(main):
    """The default call at one workgroup per tile and at a split of 3, computed once."""
    mp = pytest.MonkeyPatch()
    try:
        out = {split: main.run(mp, PB_STAGE_SPLIT=split) for split in (1, 3)}
    finally:
        mp.undo()
    for ext, rows in out.values():
        ext.flags.writeable = False
    return out


def test_case_holds_every_class_of_rows(main, base):
    """What the other tests rest on: buffers of about 1002 samples, (layer, isotope) pairs with
    one and with two rows per step, a workgroup whose two isotopes differ, and tiles of more than
    one batch."""
    from pyratbay_amd import _capi
    assert 990 <= main.rowcap() <= 1024, main.rowcap()
    rows = base[1][1]
    assert rows.shape == (NL, NISO)
    print('rows per step [layer, isotope]:', rows.tolist())
    cap = max(_capi.call('pb_lbl_rows_per_step', 1024, r, None) for r in (1, 100, 200))
    for r in range(1, cap + 1):
        assert (rows == r).any(), f'no (layer, isotope) with R = {r}'
    assert rows.max() == cap
    assert (rows[:, 0] != rows[:, 1]).any(), 'no layer whose isotopes differ in R'
    assert np.array_equal(base[3][1], rows)
    # groups with their centre inside tile 0 alone fill more than one batch of the first isotope
    _, _, iown, start = main.ll.groups()
    inside = iown[start[0]:start[1]] // main.osamp < TILE
    assert inside.sum() > BATCH


@pytest.mark.parametrize('split', [1, 3])
def test_rows_per_step_leave_every_bit(main, base, monkeypatch, split):
    want, rows = base[split]
    assert np.isfinite(want).all() and want.max() > 0
    one, rows1 = main.run(monkeypatch, PB_STAGE_SPLIT=split, PB_STAGE_ROWS=1)
    assert (rows1 == 1).all()
    assert np.array_equal(one, want)
    reg, rowsr = main.run(monkeypatch, PB_STAGE_SPLIT=split, PB_STAGE_DMA=0)
    assert (rowsr == 1).all()
    assert np.array_equal(reg, want)
    # and the same call twice
    again, rows2 = main.run(monkeypatch, PB_STAGE_SPLIT=split)
    assert np.array_equal(again, want) and np.array_equal(rows2, rows)


def test_default_call_vs_oracle(main, base, orc):
    g, atm, ln, iso, vg = main.g, main.atm, main.ln, main.iso, main.vg
    profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
    worst = 0.0
    for split in (1, 3):
        ext = base[split][0]
        for layer in range(NL):
            want = np.zeros((1, g['nwave']))
            orc.extinction(want, profile, size, index, vg['lorentz'], vg['doppler'],
                           g['wn'], g['own'], g['divisors'], atm['dens'][layer],
                           atm['mol_radius'], atm['mol_mass'], iso['isoimol'], iso['isomass'],
                           iso['isoratio'], iso['isoz'][:, layer].copy(), iso['isoiext'],
                           ln['lwn'], ln['elow'], ln['gf'], ln['lid'], vg['cutoff'], 1e-30,
                           atm['temp'][layer], 0, 1, 0)
            got = ext[layer]
            assert np.array_equal(got == 0, want == 0), (split, layer)
            nz = want != 0
            worst = max(worst, np.max(np.abs(got[nz] / want[nz] - 1)))
            np.testing.assert_allclose(got, want, rtol=RTOL)
    print(f'rows per step, default call: max rel err vs oracle = {worst:.2e}')


def test_shards_cut_inside_a_tile_concatenate(main, base, monkeypatch):
    want = base[1][0]
    bounds = [0, 1500, 4097, 6001, NWAVE]
    parts = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        part, rows = main.run(monkeypatch, wbegin=a, wcount=b - a, PB_STAGE_SPLIT=1)
        assert rows.max() > 1
        parts.append(part)
    assert np.array_equal(np.concatenate(parts, axis=2), want)


def test_two_record_chunks_continue_the_sums(main, base, monkeypatch):
    """accumulate: the second chunk of the line list goes on from the sums of the first, with
    two rows per step in play."""
    want = base[1][0]
    monkeypatch.setenv('PB_STAGE_SPLIT', '1')
    try:
        main.lbl.set_record_budget(int(main.ll.ngroups * NL * 16 / 1.7))
        got = host(main.lbl.extinction(main.t, main.d, main.z, add=True))
        assert main.lbl.last_chunks >= 2
        assert main.lbl.last_rows_per_step(NL, NISO).max() > 1
        assert np.array_equal(got, want)
    finally:
        main.lbl.set_record_budget(96 << 30)


def test_batch_of_more_than_64_segments(eng, monkeypatch):
    """A sparse list on a finely oversampled grid (120 phases, a few records each): the records of
    a (tile, isotope) fit one batch, and those of the groups centred in the tile alone lie in more
    than 64 phases -- more than 64 segments in one batch, in layers with R = 2, so a step meets
    the boundary at which the per-segment hit table is rebuilt."""
    from pyratbay_amd import synth
    osamp = 120
    case = synth.lbl_case(NWAVE, 4, 900, wnstep=0.05, wnosamp=osamp, nlor=8, ndop=4, cutoff=12.5,
                          extent=60.0, niso=NISO, seed=12)
    p = Plan(eng, case)
    want, rows = p.run(monkeypatch, PB_STAGE_SPLIT=1)
    assert rows.max() > 1 and rows.min() == 1
    # host count for tile 0 and the first isotope: every group within the widest reach is a
    # candidate (upper bound of the batch), every group centred in the tile is live
    _, _, iown, start = p.ll.groups()
    pos = iown[start[0]:start[1]].astype(np.int64)
    reach = int(np.max(p.vt.size)) + 3 * osamp
    assert np.sum(pos < TILE * osamp + reach) <= BATCH
    phases = np.unique(pos[pos < TILE * osamp] % osamp)
    assert len(phases) > 64, len(phases)
    assert np.isfinite(want).all() and want.max() > 0
    one, rows1 = p.run(monkeypatch, PB_STAGE_SPLIT=1, PB_STAGE_ROWS=1)
    assert (rows1 == 1).all()
    assert np.array_equal(one, want)
    reg, _ = p.run(monkeypatch, PB_STAGE_SPLIT=1, PB_STAGE_DMA=0)
    assert np.array_equal(reg, want)
    for split in (3,):
        got, _ = p.run(monkeypatch, PB_STAGE_SPLIT=split)
        assert np.array_equal(p.run(monkeypatch, PB_STAGE_SPLIT=split, PB_STAGE_ROWS=1)[0], got)
        np.testing.assert_allclose(got, want, rtol=1e-13)


def test_odd_segment_count_and_single_segment(eng, main, monkeypatch):
    """Three lines of the first isotope at three different phases and one line of the second, all
    centred in tile 0: its workgroups have exactly three segments (a full step and a short one at
    R = 2) for the first isotope and a single segment for the second."""
    g = main.g
    own = np.asarray(g['own'])
    centre = np.array([1000 * 12 + 1, 1500 * 12 + 5, 2100 * 12 + 10, 1800 * 12 + 7])
    lines = dict(lwn=own[centre].copy(), elow=np.array([100.0, 900.0, 2500.0, 400.0]),
                 gf=np.array([1e-7, 3e-8, 2e-6, 5e-7]), lid=np.array([0, 0, 0, 1], np.int32))
    p = Plan(eng, main.case, lines=lines)
    _, _, iown, start = p.ll.groups()
    assert list(start) == [0, 3, 4]
    assert len(set(int(i) % 12 for i in iown[:3])) == 3          # three phases: three segments
    assert (iown // 12 < TILE).all() and (iown // 12 > 600).all()
    want, rows = p.run(monkeypatch, PB_STAGE_SPLIT=1)
    assert (rows == 2).any()
    assert (want[:, 0, 1000] > 0).all() and (want[:, 0, 1800] > 0).all()
    assert np.array_equal(p.run(monkeypatch, PB_STAGE_SPLIT=1, PB_STAGE_ROWS=1)[0], want)
    assert np.array_equal(p.run(monkeypatch, PB_STAGE_SPLIT=1, PB_STAGE_DMA=0)[0], want)
