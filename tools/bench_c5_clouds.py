#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 species) with
a cloud deck and patchy clouds per walker: TableSpectrum.eval_bands(..., deck_logp, f_patchy)
(pb_clouds.hip), transit and emission geometry.

Legs (every one with Rayleigh H2 + He in ec, so that the interpolation is the same):
  clear           no cloud arguments: the clear path (depth-ordered columns, layer limits)
  deck            a deck per walker, no f_patchy: the cloudy column alone
  patchy_deck     f cloudy + (1 - f) clear with a deck: one optical-depth sum for both columns
  patchy_deck_lec the same + one Lecavelier haze as cloud-type opacity: two sums side by side
Prints one JSON line: evals/s and ms per 64 walkers of every leg, and the ratios to the clear leg.
`--legs clear` runs on a checkout without the cloud path too (the parent's number in
profiles/clouds.md comes from that).

    python tools/bench_c5_clouds.py [--steps K] [--warmup W] [--legs clear,deck,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import bench_c5  # noqa: E402

BATCH = bench_c5.BATCH
LEGS = ('clear', 'deck', 'patchy_deck', 'patchy_deck_lec')

_INPUTS = []


def run(rt, leg, steps, warmup):
    import torch
    from pyratbay_amd import continuum as ct
    from pyratbay_amd import engine
    if not _INPUTS:
        _INPUTS.append(bench_c5.inputs())
    inp = _INPUTS[0]
    g, atm = inp['grid'], inp['atm']
    wn, pressure = g['wn'], atm['press']
    models = [ct.Kurucz(wn, 'H2'), ct.Kurucz(wn, 'He')]
    if leg == 'clear':
        cont = ct.Continuum(wn, pressure, models)
    else:
        haze = [ct.Lecavelier(pressure, wn=wn)] if leg == 'patchy_deck_lec' else []
        cont = ct.Continuum(wn, pressure, models + haze + [ct.Deck(pressure, wn)],
                            cloud_models=haze)
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'],
                                 rt_path=rt, continuum=cont)
    pb = engine.PassBands(wn, inp['bands'])
    batches = []
    for b in range(4):
        rng = np.random.default_rng(1300 + b)
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 700 + b)
        ntot = pressure * 1e6 / temps / 1.380649e-16
        cdens = np.stack([ntot * 0.85, ntot * 0.149], axis=-1)
        kw = dict(continuum_density=engine.dev(cdens))
        if leg != 'clear':
            # decks between 1 mbar and 1 bar: above, among and below the clear crossings
            kw['deck_logp'] = engine.dev(rng.uniform(-3, 0, BATCH))
        if leg.startswith('patchy'):
            kw['f_patchy'] = engine.dev(rng.uniform(0, 1, BATCH))
        if leg == 'patchy_deck_lec':
            kw['continuum_pars'] = engine.dev(np.stack([rng.uniform(0, 2, BATCH),
                                                        rng.uniform(-6, -2, BATCH)], axis=1))
        batches.append((engine.dev(temps), engine.dev(dens), engine.dev(radius), kw))

    def step(i):
        temps, dens, radius, kw = batches[i % len(batches)]
        return model.eval_bands(temps, dens, pb, radius=radius, chunk=bench_c5.CHUNK, **kw)
    for i in range(warmup):
        out = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step(i)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    finite = bool(torch.isfinite(out).all())
    ordered = model.column_order is not None
    del model, batches
    torch.cuda.empty_cache()
    return {'evals_per_s': steps * BATCH / elapsed, 'ms_per_batch': 1e3 * elapsed / steps,
            'finite': finite, 'ordered_columns': ordered}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--legs', default=','.join(LEGS))
    args = ap.parse_args()
    legs = [leg for leg in args.legs.split(',') if leg]
    assert all(leg in LEGS for leg in legs), f'legs: {LEGS}'
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-clouds', 'walkers_per_batch': BATCH, 'steps': args.steps}
    for rt in ('transit', 'emission'):
        res[rt] = {leg: run(rt, leg, args.steps, args.warmup) for leg in legs}
        if 'clear' in legs:
            for leg in legs:
                res[rt][leg]['time_over_clear'] = \
                    res[rt][leg]['ms_per_batch'] / res[rt]['clear']['ms_per_batch']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
