#!/usr/bin/env python3
"""Generate tests/golden/g27_contribution_clouds.npz: band contribution functions WITH clouds of
the REAL reference package, called unmodified, on small seeded inputs.  Build container only (needs
the reference checkout that make_golden_e2e.py names):

    python tests/golden/make_golden_contribution_clouds.py

What Pyrat.band_contribution (pyrat/pyrat_obj.py:671-696) does after optical_depth
(pyrat_obj.py:129-164) and spectrum() (pyrat/spectrum.py:346-385), step by step with the
reference's own functions:
  opacity.clouds.Deck / CCSgray / Lecavelier          deck_itop, rsurf, tsurf and ec_cloud
  opacity.optic_depth.optical_depth(rt, ec, radius, itop, deck_itop + 1, maxdepth, ec_cloud)
                                                      both depths and ideeps (a model without a
                                                      patchy fraction: the cloud models are part of
                                                      ec, pyrat/opacity.py:252-255, one column)
  spectrum.blackbody_wn_2D + spectrum.plane_parallel_rt   B, with the deck's row written in place
  spectrum.contribution_funcs: transmittance, contribution_function, band_cf

Every case has a NON-UNIFORM wavenumber grid, make_golden_contribution.make_bands' bands (1, 2,
255, 256, 257, 513 samples clipped to the grid, two overlapping, from sample 0, to the last
sample) and `nw` walkers.  Stored per case `{case}_...` (ec is rounded to float32 values, which
halves its size in the archive; everything else is what the reference returns):
  rt, itop, maxdepth, wn[W], press[L] (bar), temps[nw, L], radius[nw, L], ec[nw, L, W]   inputs
  deck_logp[nw], deck_itop[nw], deck_rsurf[nw], deck_tsurf[nw]     (cases with a deck)
  cloud_cs[nr, nw, W], cloud_f[nw, L, nr], cloud_gray[nr]  ec_cloud = sum_m cs_m f_m, the rank-1
                                  factors of the models (CCSgray: cs = 1, cloud_gray True)
  f_patchy[nw], f_clamped[nw]     (patchy cases) the fraction given, and what `band` was made with
  depth[nw, L, W], ideep[nw, W]   the cloudy column (the only one without f_patchy)
  depth_clear, ideep_clear        (patchy cases) the clear column
  planck[nw, L, W]                (emission) B with the deck's row
  contrib[nw, L, W], band[nw, L, nbands], sens
and, shared by the cases of one grid size, `W{W}_band_start`, `W{W}_band_count`, `W{W}_response`.

Cases (L, itop; the deck's layer per walker):
  t_l2, t_l3      transit, L = 2 / 3: the deck at layer 1, the lowest the reference can put it
  t_top           transit L = 9, itop = 2: deck_itop = 1 and 2, at or above itop -- no cloudy row
  t_next          deck_itop = itop + 1, Deck + CCSgray + Lecavelier, f = 1
  t_mid           a deck in the middle, all three models, f = 0.37, W = 270
  t_bot           deck_itop = L - 1, the deck alone, f = 1.4 (band made with the clamped 1.0)
  t_nodeck        CCSgray + Lecavelier, no deck, no f_patchy
  t_l40           L = 40, W = 600: 40 impact parameters (blocks of 16: not a multiple), deck at 17
  t_w3            three walkers: different decks, fractions (0, 0.37, -0.2 -> 0) and radii
  e_next .. e_bot2  emission L = 9, itop = 2: deck_itop = itop + 1, middle, L - 1, L - 2; tsurf set
                  more than 50 K from the layer temperature; e_mid is given f_patchy (no effect)
  e_nodeck        cloud models without a deck;  e_md: maxdepth = 0.105 with a deck

Preconditions, asserted -- a case that misses one is refused:
  * every deck lands on the layer the case names;
  * transit, L >= 9 with a deck below itop and f_patchy: some columns close in the cloudy column
    strictly above the clear column's ideep, some at the deck and some by maxdepth above it, and
    at least one clear column never closes;
  * emission with a deck: at least one column reaches the row past the deck and one stops above;
    e_md: jumps kept (<= 0.1) and zeroed; |tsurf - T[deck_itop]| > 50 K, and a host recomputation
    without the deck's Planck row moves `band` by more than 1e-6 somewhere;
  * emission given f_patchy (pyrat_obj.py:691-693 reads od.depth and od.B only; the clear
    column's depth is computed and dropped): the same bits as the reference's route without a
    patchy fraction, with the cloud models inside ec;
  * everything is finite except the one-sample band (NaN in every layer); no column sum and no
    band maximum is 0.
Sensitivity `{case}_sens` (G24's): the reference's functions again on both depths times
1 + 1e-13 r, r uniform in [-1, 1] (seeded): the largest absolute change of the max-normalised
band result.  A case above 1e-9 is refused.  Only data is stored.

Printed summary of the committed file:
t_l2: transit L=2 W=130 nw=1 itop=0 deck=[1] clouds=False f_patchy=None sensitivity 0.00e+00
t_l3: transit L=3 W=130 nw=1 itop=0 deck=[1] clouds=True f_patchy=[0.37] sensitivity 1.17e-15
t_top: transit L=9 W=130 nw=2 itop=2 deck=[1, 2] clouds=False f_patchy=[0.0, 0.37] sensitivity 5.00e-15
    w0: deck 1 <= itop, no cloudy row
    w1: deck 2 <= itop, no cloudy row
t_next: transit L=9 W=130 nw=1 itop=2 deck=[3] clouds=True f_patchy=[1.0] sensitivity 0.00e+00
    w0: deck 3: 0 columns close by maxdepth above the deck, 102 at the deck, 102 above the clear ideep, 75 clear columns never close
t_mid: transit L=9 W=270 nw=1 itop=2 deck=[5] clouds=True f_patchy=[0.37] sensitivity 1.27e-14
    w0: deck 5: 83 columns close by maxdepth above the deck, 184 at the deck, 184 above the clear ideep, 153 clear columns never close
t_bot: transit L=9 W=130 nw=1 itop=2 deck=[8] clouds=False f_patchy=[1.4] sensitivity 2.78e-15
    w0: deck 8: 52 columns close by maxdepth above the deck, 73 at the deck, 0 above the clear ideep, 73 clear columns never close
t_nodeck: transit L=9 W=130 nw=1 itop=2 deck=None clouds=True f_patchy=None sensitivity 7.67e-15
t_l40: transit L=40 W=600 nw=1 itop=0 deck=[17] clouds=True f_patchy=[0.37] sensitivity 3.33e-15
    w0: deck 17: 142 columns close by maxdepth above the deck, 449 at the deck, 451 above the clear ideep, 363 clear columns never close
t_w3: transit L=6 W=130 nw=3 itop=0 deck=[2, 4, 3] clouds=True f_patchy=[0.0, 0.37, -0.2] sensitivity 1.35e-14
e_next: emission L=9 W=130 nw=1 itop=2 deck=[3] clouds=True f_patchy=None sensitivity 3.77e-15
    w0: deck 3, tsurf - T = -220 K: 108 columns reach the row past the deck, 22 stop above it
    the deck row of B moves band by 5.3e-01
e_mid: emission L=9 W=270 nw=1 itop=2 deck=[5] clouds=True f_patchy=[0.37] sensitivity 5.52e-15
    w0: deck 5, tsurf - T = -191 K: 192 columns reach the row past the deck, 78 stop above it
    the deck row of B moves band by 7.1e-02
    without f_patchy: the same bits
e_bot: emission L=9 W=130 nw=1 itop=2 deck=[8] clouds=False f_patchy=None sensitivity 2.37e-14
    w0: deck 8, tsurf - T = -272 K: 88 columns reach the row past the deck, 130 stop above it
    the deck row of B moves band by 0.0e+00
e_bot2: emission L=9 W=130 nw=1 itop=2 deck=[7] clouds=True f_patchy=None sensitivity 5.43e-14
    w0: deck 7, tsurf - T = -270 K: 77 columns reach the row past the deck, 53 stop above it
    the deck row of B moves band by 2.1e-02
e_nodeck: emission L=9 W=130 nw=1 itop=2 deck=None clouds=True f_patchy=None sensitivity 5.86e-14
e_md: emission L=10 W=130 nw=1 itop=0 deck=[6] clouds=False f_patchy=None sensitivity 2.34e-14
    w0: deck 6, tsurf - T = -232 K: 105 columns reach the row past the deck, 25 stop above it
    the deck row of B moves band by 8.5e-02
    101 jumps kept, 29 set to 0
wrote tests/golden/g27_contribution_clouds.npz: 906536 bytes (g24_contribution.npz: 1030330)
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden_e2e as e2e                      # noqa: E402
from make_golden_contribution import make_bands, make_inputs   # noqa: E402

# name: rt, L, W, nw, itop, maxdepth, deck (layer per walker or None), clouds, f_patchy (or None)
CASES = {
    't_l2': ('transit', 2, 130, 1, 0, 10.0, [1], False, None),
    't_l3': ('transit', 3, 130, 1, 0, 10.0, [1], True, [0.37]),
    't_top': ('transit', 9, 130, 2, 2, 10.0, [1, 2], False, [0.0, 0.37]),
    't_next': ('transit', 9, 130, 1, 2, 10.0, [3], True, [1.0]),
    't_mid': ('transit', 9, 270, 1, 2, 10.0, [5], True, [0.37]),
    't_bot': ('transit', 9, 130, 1, 2, 10.0, [8], False, [1.4]),
    't_nodeck': ('transit', 9, 130, 1, 2, 10.0, None, True, None),
    't_l40': ('transit', 40, 600, 1, 0, 10.0, [17], True, [0.37]),
    't_w3': ('transit', 6, 130, 3, 0, 10.0, [2, 4, 3], True, [0.0, 0.37, -0.2]),
    'e_next': ('emission', 9, 130, 1, 2, 10.0, [3], True, None),
    'e_mid': ('emission', 9, 270, 1, 2, 10.0, [5], True, [0.37]),
    'e_bot': ('emission', 9, 130, 1, 2, 10.0, [8], False, None),
    'e_bot2': ('emission', 9, 130, 1, 2, 10.0, [7], True, None),
    'e_nodeck': ('emission', 9, 130, 1, 2, 10.0, None, True, None),
    'e_md': ('emission', 10, 130, 1, 0, 0.105, [6], False, None),
}


def main():
    if not os.path.isdir(e2e.REF):
        sys.exit(f'needs {e2e.REF}')
    work = tempfile.mkdtemp(prefix='pb_g27_')
    store = {}
    try:
        e2e.reference_package(work)
        import pyratbay.constants as pc
        import pyratbay.opacity as op
        import pyratbay.spectrum as ps
        from pyratbay.opacity.optic_depth import optical_depth
        from pyratbay.spectrum.contribution_funcs import (band_cf, contribution_function,
                                                          transmittance)
        rng = np.random.default_rng(27)
        bands_of = {}
        for name, (rt, L, W, nw, itop, maxdepth, decks, clouds, fp) in CASES.items():
            if W not in bands_of:
                bands_of[W] = make_bands(rng, W)
                store[f'W{W}_band_start'] = np.array([b[0] for b in bands_of[W]], np.int32)
                store[f'W{W}_band_count'] = np.array([len(b[1]) for b in bands_of[W]], np.int32)
                store[f'W{W}_response'] = np.concatenate([b[1] for b in bands_of[W]])
            bands = bands_of[W]
            responses = [b[1] for b in bands]
            indices = [np.arange(b[0], b[0] + len(b[1])) for b in bands]
            single = np.array([len(b[1]) == 1 for b in bands])
            wn, press, temps, radius, ec = make_inputs(rng, rt, L, W, nw, maxdepth)
            ec = ec.astype(np.float32).astype(np.float64)
            patchy = fp is not None
            nr = 2 if clouds else 0
            case = dict(rt=np.array(rt), itop=np.array(itop), maxdepth=np.array(maxdepth), wn=wn,
                        press=press, temps=temps, radius=radius)
            depth = np.zeros((nw, L, W))
            ideep = np.zeros((nw, W), np.int32)
            depth_clear = np.zeros((nw, L, W))
            ideep_clear = np.zeros((nw, W), np.int32)
            planck = np.zeros((nw, L, W))
            contrib = np.zeros((nw, L, W))
            band = np.zeros((nw, L, len(bands)))
            deck_state = np.zeros((4, nw))
            cloud_cs = np.ones((nr, nw, W))
            cloud_f = np.zeros((nw, L, nr))
            f_clamped = None if fp is None else np.clip(np.array(fp, float), 0.0, 1.0)
            sens = 0.0
            notes = []
            for w in range(nw):
                # ---- the cloud models of the reference ----
                ibottom, dk, tsurf = L, None, None
                if decks is not None:
                    dk = decks[w]
                    if rt == 'emission':
                        # a deck temperature that differs from the layer's: a kink in the profile
                        temps[w, dk - 1] -= 180.0
                    deck = op.clouds.Deck(press, wn)
                    logp = 0.5 * (np.log10(press[dk - 1]) + np.log10(press[dk]))
                    deck.calc_extinction_coefficient(radius[w], temps[w], pars=[logp])
                    assert deck.itop == dk, f'{name}: deck at {deck.itop}, wanted {dk}'
                    ibottom, tsurf = deck.itop + 1, deck.tsurf
                    deck_state[:, w] = logp, deck.itop, deck.rsurf, deck.tsurf
                    if rt == 'emission':
                        assert abs(tsurf - temps[w, dk]) > 50.0, f'{name}: tsurf near the layer'
                ec_cloud = np.zeros((L, W))
                if clouds:
                    gray = op.clouds.CCSgray(press, wn)
                    lec = op.clouds.Lecavelier(press, wn=wn)
                    # strengths that make ec_cloud comparable to ec half way down
                    mid = (itop + L) // 2
                    g0 = np.array(gray.calc_extinction_coefficient(
                        temps[w], pars=[0.0, np.log10(press[max(itop - 1, 0)]) - 0.1, 3.0]))
                    l0 = np.array(lec.calc_extinction_coefficient(temps[w], pars=[0.0, -4.0]))
                    level = np.median(ec[w, mid])
                    gpars = [np.log10(0.5 * level / g0[mid, 0]) + rng.uniform(-0.3, 0.3),
                             np.log10(press[min(itop + 1, L - 1)]) - 0.1, 3.0]
                    lpars = [np.log10(0.5 * level / np.median(l0[mid])) + rng.uniform(-0.3, 0.3),
                             -4.0 + rng.uniform(-0.5, 0.5)]
                    ec_gray = np.array(gray.calc_extinction_coefficient(temps[w], pars=gpars))
                    ec_lec = np.array(lec.calc_extinction_coefficient(temps[w], pars=lpars))
                    ec_cloud = ec_gray + ec_lec
                    # the rank-1 factors: CCSgray = 1 x (cs density), Lecavelier = cs x density
                    cloud_f[w, :, 0] = ec_gray[:, 0]
                    cloud_cs[1, w] = lec.cross_section
                    cloud_f[w, :, 1] = press * pc.bar / temps[w] / pc.k      # (lecavelier.py:109)
                    rebuilt = cloud_f[w, :, 0, None] * cloud_cs[0, w] + \
                        cloud_f[w, :, 1, None] * cloud_cs[1, w]
                    assert np.allclose(rebuilt, ec_cloud, rtol=1e-14, atol=0.0), name
                    assert np.any(ec_gray == 0) and np.any(ec_gray > 0), f'{name}: gray layers'
                # ---- optical depth, as Pyrat.optical_depth ----
                if patchy:
                    _, d, idp, dc, idc = optical_depth(rt, ec[w], radius[w], itop, ibottom,
                                                       maxdepth, ec_cloud)
                    depth_clear[w], ideep_clear[w] = dc, idc
                else:
                    _, d, idp, _, _ = optical_depth(rt, ec[w] + ec_cloud, radius[w], itop,
                                                    ibottom, maxdepth, None)
                depth[w], ideep[w] = d, idp
                # ---- spectrum(): B with the deck's row ----
                if rt == 'emission':
                    B = np.zeros((L, W))
                    ps.blackbody_wn_2D(wn, temps[w], B)
                    mu = np.array([0.5])
                    ps.plane_parallel_rt(depth[w], B, wn, mu, np.array([[1.0]]),
                                         np.array(idp), itop, tsurf, dk)
                    planck[w] = B

                def reference(d, dc, pl):
                    if rt == 'transit':
                        c = transmittance(d, ideep[w])
                        if patchy:
                            c = f_clamped[w] * c + \
                                (1.0 - f_clamped[w]) * transmittance(dc, ideep_clear[w])
                    else:
                        c = contribution_function(d, press, pl)
                    with np.errstate(invalid='ignore', divide='ignore'):
                        return c, band_cf(c, responses, wn, indices)

                contrib[w], band[w] = reference(depth[w].copy(), depth_clear[w].copy(), planck[w])
                assert np.all(np.isnan(band[w][:, single])), f'{name}: one-sample band not NaN'
                assert np.all(np.isfinite(band[w][:, ~single])), f'{name}: a band maximum is 0'
                assert np.all(np.isfinite(contrib[w])), f'{name}: contrib not finite'
                r = np.random.default_rng(2700 + w).uniform(-1, 1, (2,) + depth[w].shape)
                _, band2 = reference(depth[w] * (1 + 1e-13 * r[0]),
                                     depth_clear[w] * (1 + 1e-13 * r[1]), planck[w])
                sens = max(sens, float(np.max(np.abs(band2 - band[w])[:, ~single])))

                cols = np.arange(W)
                if rt == 'transit' and decks is not None and dk <= itop:
                    assert np.all(ideep[w] == itop) and np.all(depth[w] == 0), name
                    assert np.all(transmittance(depth[w].copy(), ideep[w])[itop:] == 0), name
                    notes.append(f'w{w}: deck {dk} <= itop, no cloudy row')
                elif rt == 'transit' and patchy and L >= 9 and decks is not None:
                    by_depth = depth[w][ideep[w], cols] > maxdepth
                    at_deck = ~by_depth & (ideep[w] == dk)
                    above = ideep[w] < ideep_clear[w]
                    open_clear = ~(depth_clear[w][ideep_clear[w], cols] > maxdepth)
                    notes.append(f'w{w}: deck {dk}: {int(np.sum(by_depth & (ideep[w] < dk)))} '
                                 f'columns close by maxdepth above the deck, {int(at_deck.sum())} '
                                 f'at the deck, {int(above.sum())} above the clear ideep, '
                                 f'{int(open_clear.sum())} clear columns never close')
                    if dk > itop + 1 and dk < L - 1:
                        assert np.any(by_depth & (ideep[w] < dk)), f'{name}: none by maxdepth'
                        assert np.any(above), f'{name}: no cloudy column closes above the clear'
                    assert np.any(at_deck), f'{name}: no column closes at the deck'
                    assert np.any(open_clear), f'{name}: every clear column closes'
                if rt == 'emission':
                    e = np.exp(-depth[w])
                    jump = np.diff(e, axis=0)
                    col_sum = np.sum(planck[w][:-1] * np.where(jump > 0.1, 0.0, jump) /
                                     np.diff(np.log(press))[:, None], axis=0)
                    assert np.all(col_sum != 0), f'{name}: a column sum is 0'
                    if decks is not None:
                        past = int(np.sum(ideep[w] == min(dk + 1, L - 1)))
                        stopped_above = int(np.sum(ideep[w] <= dk))
                        notes.append(f'w{w}: deck {dk}, tsurf - T = {tsurf - temps[w, dk]:+.0f} K: '
                                     f'{past} columns reach the row past the deck, '
                                     f'{stopped_above} stop above it')
                        if dk < L - 1:
                            assert past >= 1 and stopped_above >= 1, f'{name}: both kinds of stop'
                            assert np.all(depth[w][dk + 2:] == 0), f'{name}: depth below the deck'
                        # tsurf is seen: the same with the layer's own Planck row
                        plain = np.zeros((L, W))
                        ps.blackbody_wn_2D(wn, temps[w], plain)
                        _, other = reference(depth[w].copy(), None, plain)
                        moved = float(np.max(np.abs(other - band[w])[:, ~single]))
                        if dk < L - 1:
                            assert moved > 1e-6, f'{name}: tsurf moves band by {moved:.1e} only'
                        notes.append(f'the deck row of B moves band by {moved:.1e}')
                    if name == 'e_md':
                        kept = int(np.sum((jump > 0) & (jump <= 0.1)))
                        zeroed = int(np.sum(jump > 0.1))
                        notes.append(f'{kept} jumps kept, {zeroed} set to 0')
                        assert kept >= 1 and zeroed >= 1, f'{name}: needs both kinds of jump'
                    if patchy:
                        # (pyrat_obj.py:691-693 reads od.depth and od.B only)
                        # the same model without a patchy fraction, the reference's other route
                        _, d1, _, _, _ = optical_depth(rt, ec[w] + ec_cloud, radius[w], itop,
                                                       ibottom, maxdepth, None)
                        _, same = reference(d1, None, planck[w])
                        assert np.array_equal(same, band[w], equal_nan=True), \
                            f'{name}: f_patchy changes the emission result'
                        notes.append('without f_patchy: the same bits')
            print(f'{name}: {rt} L={L} W={W} nw={nw} itop={itop} deck={decks} clouds={clouds} '
                  f'f_patchy={fp} sensitivity {sens:.2e}')
            for n in notes:
                print(f'    {n}')
            if not sens <= 1e-9:
                sys.exit(f'case {name}: sensitivity {sens:.2e} > 1e-9: ill-conditioned')
            case.update(ec=ec, temps=temps, depth=depth, ideep=ideep, contrib=contrib, band=band,
                        sens=np.array(sens))
            if decks is not None:
                case.update(deck_logp=deck_state[0], deck_itop=deck_state[1].astype(np.int32),
                            deck_rsurf=deck_state[2], deck_tsurf=deck_state[3])
            if clouds:
                case.update(cloud_cs=cloud_cs, cloud_f=cloud_f,
                            cloud_gray=np.array([True, False]))
            if patchy:
                case.update(f_patchy=np.array(fp, float), f_clamped=f_clamped)
                if rt == 'transit':
                    case.update(depth_clear=depth_clear, ideep_clear=ideep_clear)
            if rt != 'transit':
                case['planck'] = planck
            store.update({f'{name}_{k}': v for k, v in case.items()})
        store['cases'] = np.array(list(CASES))
        out = os.path.join(HERE, 'g27_contribution_clouds.npz')
        np.savez_compressed(out, **store)
        limit = os.path.getsize(os.path.join(HERE, 'g24_contribution.npz'))
        print(f'wrote {out}: {os.path.getsize(out)} bytes (g24_contribution.npz: {limit})')
        assert os.path.getsize(out) <= limit, 'larger than g24_contribution.npz'
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
