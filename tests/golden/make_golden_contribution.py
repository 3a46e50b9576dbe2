#!/usr/bin/env python3
"""Generate tests/golden/g24_contribution.npz: band contribution functions of the REAL reference
package (spectrum/contribution_funcs.py: transmittance, contribution_function, band_cf, called
unmodified) on small seeded inputs.  Build container only (needs the reference checkout that
make_golden_e2e.py names and `make -C oracle ref liboracle.so`):

    python tests/golden/make_golden_contribution.py

The real package is imported as in make_golden_e2e.py.  Every case has a NON-UNIFORM wavenumber
grid and `nw` walkers (leading axis of every per-walker array); stored per case `{case}_...`:
  rt ('transit', 'emission', 'two_stream'), itop, maxdepth, wn[W], press[L] (bar), temps[nw, L],
  radius[nw, L], ec[nw, L, W]                                             the inputs
  depth[nw, L, W], ideep[nw, W]   the oracle's optical_depth_transit / plane_parallel_optical_depth
  planck[nw, L, W]                the oracle's blackbody_wn_2D (emission and two-stream)
  contrib[nw, L, W]               transmittance / contribution_function of the reference
  band[nw, L, nbands]             band_cf of the reference
  sens                            see below
and, shared by the cases of one grid size `W{W}_...`: band_start[nbands], band_count[nbands],
response (the bands' response curves, concatenated).

Bands of every case, clipped to the grid (a band never runs past the last sample): counts 1, 2,
255, 256, 257 and 513, two overlapping bands, a band starting at sample 0 and one ending at the
last sample.

Cases: L = 2 and L = 3 (transit and emission), L = 9 with itop = 2 (transit and emission),
L = 40 with W = 600 (emission), an emission case with maxdepth = 0.105 (columns that stop with
1 - exp(-tau) <= 0.1 keep their jump, the others lose it), a two-stream case (no stop), and three
walkers with different profiles and radii (transit).

Preconditions, asserted -- a case that misses one is refused:
  * where there are layers enough (L >= 9, a finite maxdepth): columns stop at three or more
    different layers, and at least one column never stops;
  * the small-maxdepth case: at least one jump in (0, 0.1] and at least one > 0.1;
  * no column sum and no band maximum is 0, except the band of one sample (NaN in every layer).

Sensitivity `{case}_sens` (G23's precedent): the reference's functions run again on
depth * (1 + 1e-13 r), r uniform in [-1, 1] (seeded); stored is the largest absolute change of the
max-normalised band result.  A case above 1e-9 is ill-conditioned and refused.  Only data is
stored."""
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

RJUP = 7.1492e9

# name: (rt, L, W, nw, itop, maxdepth)
CASES = {
    't_l2': ('transit', 2, 130, 1, 0, 10.0),
    'e_l2': ('emission', 2, 130, 1, 0, 10.0),
    't_l3': ('transit', 3, 130, 1, 0, 10.0),
    'e_l3': ('emission', 3, 130, 1, 0, 10.0),
    't_l9': ('transit', 9, 270, 1, 2, 10.0),
    'e_l9': ('emission', 9, 270, 1, 2, 10.0),
    'e_l40': ('emission', 40, 600, 1, 0, 10.0),
    'e_md': ('emission', 10, 270, 1, 0, 0.105),
    'ts_l8': ('two_stream', 8, 270, 1, 0, np.inf),
    't_w3': ('transit', 6, 270, 3, 0, 10.0),
}


def make_bands(rng, W):
    """(start, response) of the bands on a grid of W samples, clipped to the grid."""
    spans = [(5, 1), (9, 2), (3, 255), (7, 256), (11, 257), (13, 513),
             (40, 60), (70, 50),                 # overlapping: samples 70 .. 99 in both
             (0, 33), (W - 21, 21)]              # from sample 0; to the last sample
    bands = []
    for start, count in spans:
        count = min(count, W - start)
        assert count >= 1 and start >= 0 and start + count <= W
        x = np.linspace(-1.0, 1.0, count) if count > 1 else np.zeros(1)
        bands.append((start, (0.2 + np.exp(-2.0 * x**2)) * rng.uniform(0.7, 1.3, count)))
    return bands


def make_inputs(rng, rt, L, W, nw, maxdepth):
    wn = 2000.0 + np.cumsum(rng.uniform(0.4, 2.5, W))           # non-uniform, ascending
    press = np.logspace(-6, 2, L) * rng.uniform(0.9, 1.1, L)
    press.sort()
    temps = np.empty((nw, L))
    radius = np.empty((nw, L))
    ec = np.empty((nw, L, W))
    for w in range(nw):
        t_top, t_bot = rng.uniform(700, 1100), rng.uniform(1500, 2300)
        temps[w] = np.linspace(t_top, t_bot, L) * rng.uniform(0.97, 1.03, L)
        steps = rng.uniform(0.5e7, 2.0e7, L - 1)
        radius[w] = rng.uniform(0.9, 1.3) * RJUP + np.concatenate([np.cumsum(steps[::-1])[::-1],
                                                                  [0.0]])
        span = radius[w, 0] - radius[w, -1]
        # columns from transparent to opaque within a few layers: strengths over six decades
        lo, hi = (-2.5, 4.5) if np.isfinite(maxdepth) and maxdepth > 1 else (-3.0, 1.0)
        if rt == 'transit':
            lo, hi = lo - 1.5, hi - 1.5                          # (chords are longer)
        strength = 10.0**rng.uniform(lo, hi, W) / span
        profile = (press / press[-1])**rng.uniform(0.15, 0.3)
        ec[w] = strength * profile[:, None] * rng.uniform(0.8, 1.2, (L, W))
    return wn, press, temps, radius, ec


def main():
    if not os.path.isdir(e2e.REF):
        sys.exit(f'needs {e2e.REF}')
    from oracle import oracle as orc
    work = tempfile.mkdtemp(prefix='pb_g24_')
    store = {}
    try:
        e2e.reference_package(work)
        from pyratbay.spectrum.contribution_funcs import (band_cf, contribution_function,
                                                          transmittance)
        rng = np.random.default_rng(24)
        bands_of = {}
        for name, (rt, L, W, nw, itop, maxdepth) in CASES.items():
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
            if name == 'e_md':
                # a jump is kept only where a column stops with 0.105 <= tau <= -log(0.9) =
                # 0.10536: every 7th column is scaled to reach 0.1052 at a layer of its own
                full = np.zeros((L, W))
                orc.plane_parallel_optical_depth(full, np.full(W, L - 1, np.int32), ec[0],
                                                 -np.diff(radius[0]), np.inf, itop, L)
                for j in range(0, W, 7):
                    k = 2 + (j // 7) % (L - 3)
                    ec[0][:, j] *= 0.1052 / full[k, j]
            depth = np.zeros((nw, L, W))
            ideep = np.zeros((nw, W), np.int32)
            planck = np.zeros((nw, L, W))
            contrib = np.zeros((nw, L, W))
            band = np.zeros((nw, L, len(bands)))
            sens = 0.0
            stops, open_columns = set(), 0

            def reference(w, d):
                if rt == 'transit':
                    c = transmittance(d, ideep[w])
                else:
                    c = contribution_function(d, press, planck[w])
                with np.errstate(invalid='ignore', divide='ignore'):
                    return c, band_cf(c, responses, wn, indices)

            for w in range(nw):
                if rt == 'transit':
                    depth[w], ideep[w] = orc.optical_depth_transit(ec[w], radius[w], itop, L,
                                                                   maxdepth)
                    stopped = depth[w][ideep[w], np.arange(W)] > maxdepth
                else:
                    idp = np.full(W, L - 1, np.int32)
                    orc.plane_parallel_optical_depth(depth[w], idp, ec[w], -np.diff(radius[w]),
                                                     maxdepth, itop, L)
                    ideep[w] = idp
                    planck[w] = orc.blackbody_wn_2D(wn, temps[w])
                    stopped = depth[w][ideep[w], np.arange(W)] >= maxdepth
                stops |= set(ideep[w][stopped].tolist())
                open_columns += int(np.sum(~stopped))
                contrib[w], band[w] = reference(w, depth[w].copy())
                if rt != 'transit':
                    e = np.exp(-depth[w])
                    col_sum = np.sum(planck[w][:-1] * np.where(np.diff(e, axis=0) > 0.1, 0.0,
                                                               np.diff(e, axis=0)) /
                                     np.diff(np.log(press))[:, None], axis=0)
                    assert np.all(col_sum != 0), f'{name}: a column sum is 0'
                    if name == 'e_md':
                        jump = np.diff(e, axis=0)
                        kept = np.sum((jump > 0) & (jump <= 0.1))
                        zeroed = np.sum(jump > 0.1)
                        print(f'{name}: {kept} jumps kept, {zeroed} set to 0')
                        assert kept >= 1 and zeroed >= 1, f'{name}: needs both kinds of jump'
                assert np.all(np.isnan(band[w][:, single])), f'{name}: one-sample band not NaN'
                assert np.all(np.isfinite(band[w][:, ~single])), f'{name}: a band maximum is 0'
                assert np.all(np.isfinite(contrib[w])), f'{name}: contrib not finite'
                r = np.random.default_rng(2400 + w).uniform(-1, 1, depth[w].shape)
                _, band2 = reference(w, depth[w] * (1 + 1e-13 * r))
                sens = max(sens, float(np.max(np.abs(band2 - band[w])[:, ~single])))
            if L >= 9 and np.isfinite(maxdepth):
                assert len(stops) >= 3, f'{name}: columns stop at {sorted(stops)} only'
                assert open_columns >= 1, f'{name}: every column stops'
            if not np.isfinite(maxdepth):
                assert not stops
            print(f'{name}: {rt} L={L} W={W} nw={nw} stops at {sorted(stops)}, {open_columns} '
                  f'open columns, sensitivity {sens:.2e}')
            if not sens <= 1e-9:
                sys.exit(f'case {name}: sensitivity {sens:.2e} > 1e-9: ill-conditioned')
            case = dict(rt=np.array(rt), itop=np.array(itop), maxdepth=np.array(maxdepth), wn=wn,
                        press=press, temps=temps, radius=radius, ec=ec, depth=depth, ideep=ideep,
                        contrib=contrib, band=band, sens=np.array(sens))
            if rt != 'transit':
                case['planck'] = planck
            store.update({f'{name}_{k}': v for k, v in case.items()})
        store['cases'] = np.array(list(CASES))
        out = os.path.join(HERE, 'g24_contribution.npz')
        np.savez_compressed(out, **store)
        print(f'wrote {out}: {os.path.getsize(out)} bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
