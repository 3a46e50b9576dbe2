"""Staged gather, the request of a row (k_ext_staged, LDS-DMA path): a row of ceil(rowlim / 128)
pieces of 1 KiB is requested by one or two statements -- one write of M0 and up to four loads with
the immediate offsets 0 / 1024 / 2048 / 3072 each -- chosen by the piece count of the (layer,
isotope).  Whatever the count, the result has the bits of PB_STAGE_DMA=0 (rows via registers, no
DMA at all) and of PB_STAGE_ROWS=1 (one row per step), at one workgroup per tile and at a split of
3, on an output buffer that held other numbers before the call.  Needs an MI355X.

The main case (cutoff 25 cm-1 at a step of 0.05 cm-1, extent 60, layers from 0.3 to 30 bar, two
isotopes of masses 18 and 2.5) holds (layer, isotope) pairs with 1, 2, 3, 4, 5, 6 and 8 pieces:
both sides of the boundary between the two M0 groups (4 | 5), the full row (8), and rows of three
pieces short enough for two rows per step.  That is asserted: the longest row of every pair is
restated on the host from the table's sizes as k_layer_state forms it, and checked against the
rows per step the device reports (last_rows_per_step).  The long case (cutoff 30 cm-1: rows of
1201 samples) runs the chunked rows.  A call that starts one sample later moves the start of
every window in its rows by one: calls at wbegin 1 and 2 cover both parities of the LDS image.
Tolerance against the oracle: that of test_gpu_extinction.py (rtol 1e-10, same zero pattern)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-10
NISO = 2
STAGE_ROW_MAX = 1024             # kStageRowMax: longest row (or chunk of one) in an LDS buffer
K_B, AMU, C_LIGHT = 1.380658e-16, 1.66053886e-24, 2.99792458e10      # pb_common.h
SQRT_LN2 = 0.83255461115769775635


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


def row_lengths(size, osamp):
    """Samples per phase row of every table cell (pb_voigt.hip: pm_stride); a cell of size 0
    aliases the previous Doppler column."""
    size = np.asarray(size)
    stride = (2 * size + 1 + osamp - 1) // osamp
    for d in range(1, size.shape[1]):
        stride[:, d] = np.where(size[:, d] == 0, stride[:, d - 1], stride[:, d])
    return stride


def longest_rows(case):
    """rowmax[L, niso]: the longest phase row a (layer, isotope) can select, as k_layer_state
    (pb_ext_records.hip) forms li_rowmax: the Lorentz row nearest to the layer's width, the Doppler
    columns nearest to the widths at both ends of the grid with one column of margin."""
    g, atm, iso, vg = (case[k] for k in ('grid', 'atm', 'iso', 'voigt'))
    lor, dop, own = vg['lorentz'], vg['doppler'], g['own']
    stride = row_lengths(vg['size'], g['wnosamp'])
    out = np.zeros((atm['nlayers'], len(iso['isomass'])), np.int64)
    for layer in range(atm['nlayers']):
        temp = atm['temp'][layer]
        fdop = np.sqrt(2 * K_B * temp / AMU) * SQRT_LN2 / C_LIGHT
        flor = np.sqrt(2 * K_B * temp / np.pi / AMU) / C_LIGHT
        for i, mass in enumerate(iso['isomass']):
            dia = atm['mol_radius'][iso['isoimol'][i]] + atm['mol_radius']
            alphal = flor * np.sum(atm['dens'][layer] * dia * dia *
                                   np.sqrt(1 / mass + 1 / atm['mol_mass']))
            alphad = fdop / np.sqrt(mass)
            ilor = nearest_index(lor, alphal)
            dlo = max(0, nearest_index(dop, alphad * own[0]) - 1)
            dhi = min(len(dop) - 1, nearest_index(dop, alphad * own[-1]) + 1)
            out[layer, i] = stride[ilor, dlo:dhi + 1].max()
    return out


class Plan:
    """One synthetic case on the device, with a staged-gather plan and its inputs."""

    def __init__(self, eng, case):
        g, atm, iso, vg, ln = (case[k] for k in ('grid', 'atm', 'iso', 'voigt', 'lines'))
        self.eng, self.case, self.g, self.atm, self.iso, self.vg, self.ln = \
            eng, case, g, atm, iso, vg, ln
        self.nl, self.nwave, self.osamp = atm['nlayers'], g['nwave'], g['wnosamp']
        self.vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                                       self.osamp)
        self.ll = eng.LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'], NISO, g['own'])
        self.lbl = eng.LBL(self.vt, self.ll, g['wn'], g['divisors'], atm['mol_radius'],
                           atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                           iso['isoiext'], vg['cutoff'], 1e-30, max_layers=self.nl)
        self.lbl.set_gather_mode('staged')
        self.t, self.d, self.z = eng.dev(atm['temp']), eng.dev(atm['dens']), eng.dev(iso['isoz'])
        self.rowmax = longest_rows(case)
        self.rowcap = int(row_lengths(vg['size'], self.osamp).max())
        # LblArgs::rowlds (plan_gather): the buffer of a row or of a chunk, rounded up to even
        self.rowlds = (min(self.rowcap, STAGE_ROW_MAX) + 1) & ~1
        self.pieces = (np.minimum(self.rowmax, self.rowlds) + 127) // 128

    def run(self, monkeypatch, wbegin=0, wcount=None, **env):
        """-> (ec[L, 1, wcount], rows per step[L, niso]); the output buffer holds a pattern of
        large negative numbers before the call."""
        import torch
        wcount = self.nwave - wbegin if wcount is None else wcount
        n = self.nl * wcount
        out = (-1e200 * (1 + torch.arange(n, dtype=torch.float64, device=self.t.device) % 97)
               ).reshape(self.nl, 1, wcount)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        got = self.lbl.extinction(self.t, self.d, self.z, add=True, out=out, wbegin=wbegin,
                                  wcount=wcount)
        assert got.data_ptr() == out.data_ptr()
        ext = host(got)
        assert self.lbl.last_gather_kernel == 'k_ext_staged'
        rows = self.lbl.last_rows_per_step(self.nl, NISO)
        for k in env:
            monkeypatch.delenv(k)
        return ext, rows


def make_case(name):
    from pyratbay_amd import synth
    if name == 'main':
        return synth.lbl_case(9001, 8, 3000, wnstep=0.05, wnosamp=12, nlor=24, ndop=4,
                              extent=60.0, cutoff=25.0, niso=NISO, seed=11, ptop=0.3, pbottom=30.0,
                              iso_masses=(18.0, 2.5))
    return synth.lbl_case(6001, 6, 1500, wnstep=0.05, wnosamp=12, nlor=8, ndop=4, extent=300.0,
                          cutoff=30.0, niso=NISO, seed=12, ptop=0.1, pbottom=100.0)


_PLANS = {}


@pytest.fixture(scope='module', params=['main', 'long'])
def plan(request, eng):
    """(Plan, {split: (ec, rows per step)}): the default call at one workgroup per tile and at a
    split of 3, computed once per case and left unchanged."""
    name = request.param
    if name not in _PLANS:
        p = Plan(eng, make_case(name))
        mp = pytest.MonkeyPatch()
        try:
            base = {split: p.run(mp, PB_STAGE_SPLIT=split) for split in (1, 3)}
        finally:
            mp.undo()
        for ext, rows in base.values():
            ext.flags.writeable = False
        _PLANS[name] = (name, p, base)
    return _PLANS[name]


def test_cases_hold_the_piece_counts(plan):
    """What the other tests rest on.  main: pairs with 1, 3, 4, 5 and 8 pieces, three pieces also
    in rows short enough for two rows per step, and the device's rows per step are those of the
    host's row lengths in every pair.  long: rows beyond kStageRowMax (chunks), full buffers."""
    from pyratbay_amd import _capi
    name, p, base = plan
    rows = base[1][1]
    print(f'{name}: longest rows {p.rowmax.T.tolist()}, pieces {p.pieces.T.tolist()}, '
          f'rows per step {rows.T.tolist()}, buffers of {p.rowlds}')
    assert rows.shape == (p.nl, NISO) and np.array_equal(base[3][1], rows)
    if name == 'long':
        assert p.rowcap > STAGE_ROW_MAX and p.rowlds == STAGE_ROW_MAX
        assert (p.rowmax > STAGE_ROW_MAX).any() and (p.pieces == 8).any()
        return
    assert 990 <= p.rowcap <= STAGE_ROW_MAX, p.rowcap
    for n in (1, 3, 4, 5, 8):
        assert (p.pieces == n).any(), f'no (layer, isotope) with {n} pieces'
    want_rows = np.array([[_capi.call('pb_lbl_rows_per_step', p.rowlds,
                                      int(min(p.rowlds, p.rowmax[layer, i])), None)
                           for i in range(NISO)] for layer in range(p.nl)])
    assert np.array_equal(rows, want_rows), (rows.tolist(), want_rows.tolist())
    assert ((p.pieces == 3) & (rows == 2)).any(), 'no pair with three pieces and two rows per step'
    assert ((p.pieces >= 4) & (rows == 1)).any()


@pytest.mark.parametrize('split', [1, 3])
def test_request_leaves_every_bit(plan, monkeypatch, split):
    name, p, base = plan
    want, rows = base[split]
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() > 0
    reg, rowsr = p.run(monkeypatch, PB_STAGE_SPLIT=split, PB_STAGE_DMA=0)
    assert (rowsr == 1).all()
    assert np.array_equal(reg, want)
    one, rows1 = p.run(monkeypatch, PB_STAGE_SPLIT=split, PB_STAGE_ROWS=1)
    assert (rows1 == 1).all()
    assert np.array_equal(one, want)


def test_default_call_vs_oracle(plan, orc):
    name, p, base = plan
    g, atm, ln, iso, vg = p.g, p.atm, p.ln, p.iso, p.vg
    profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
    worst = 0.0
    for layer in range(p.nl):
        want = np.zeros((1, g['nwave']))
        orc.extinction(want, profile, size, index, vg['lorentz'], vg['doppler'],
                       g['wn'], g['own'], g['divisors'], atm['dens'][layer],
                       atm['mol_radius'], atm['mol_mass'], iso['isoimol'], iso['isomass'],
                       iso['isoratio'], iso['isoz'][:, layer].copy(), iso['isoiext'],
                       ln['lwn'], ln['elow'], ln['gf'], ln['lid'], vg['cutoff'], 1e-30,
                       atm['temp'][layer], 0, 1, 0)
        for split in (1, 3):
            got = base[split][0][layer]
            assert np.array_equal(got == 0, want == 0), (split, layer)
            nz = want != 0
            worst = max(worst, np.max(np.abs(got[nz] / want[nz] - 1)))
            np.testing.assert_allclose(got, want, rtol=RTOL)
    print(f'stage request, {name}: max rel err vs oracle = {worst:.2e}')


@pytest.mark.parametrize('wbegin', [1, 2])
def test_windows_at_odd_and_even_row_samples(plan, monkeypatch, wbegin):
    """The tiles of a call at wbegin start wbegin samples later than those of the whole call, so
    the window of a (group, tile) pair starts wbegin row samples later: one of the two calls has
    it at an odd, the other at an even row sample, for every pair that lies inside both."""
    name, p, base = plan
    want = base[1][0]
    got, rows = p.run(monkeypatch, wbegin=wbegin, PB_STAGE_SPLIT=1)
    assert np.array_equal(rows, base[1][1])
    assert np.array_equal(got, want[:, :, wbegin:])
    reg, _ = p.run(monkeypatch, wbegin=wbegin, PB_STAGE_SPLIT=1, PB_STAGE_DMA=0)
    assert np.array_equal(reg, got)
