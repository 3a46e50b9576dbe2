#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples) with CO split
into three isotopologue slots (4 -> 6 table slots) and the isotope ratios per walker:
TableSpectrum(..., isotopes=).eval_bands(..., iso_pars) (pb_isotopes.hip: one launch per call
that scales dens[64, 80, 6] before the chunks).

Legs, alternated in blocks inside one process (transit geometry):
  isotopes   the six-slot table with an isotope model, iso_pars[64, 2] per batch
  prescaled  the same table without an isotope model, fed densities scaled on the host beforehand
             (outside the timed window): what the batch costs without the scaling launch
  kernel     IsotopeRatios.scale alone, device events around `--kernel-launches` launches back to
             back: the time of one launch with its launch gap, not a profiler's kernel time
Prints one JSON line: per leg the median ms per 64 walkers over the blocks and their spread, the
bytes the kernel moves, and whether the two routes gave equal band fluxes.

    python tools/bench_c5_isotopes.py [--steps K] [--warmup W] [--blocks B]
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
BLOCK = '12C-16O 12CO fill_13CO_C18O\n13C-16O 13CO -1.95\n12C-18O C18O -2.7'
# table slots: H2O, three CO isotopologues, CO2, CH4 (bench_c5's species are columns 0..3)
SLOT_SPECIES = [0, 1, 1, 1, 2, 3]
NAMES = ['H2O', 'CO', 'CO', 'CO', 'CO2', 'CH4']
LABELS = ['', 'iso_12CO', 'iso_13CO', 'iso_C18O', '', '']


def six_slot_table(inp):
    """bench_c5's table with two more CO slots of the same recipe."""
    rng = np.random.default_rng(29)
    etable, ttable = inp['etable'], inp['ttable']
    press = inp['atm']['press']
    extra = []
    for _ in range(2):
        base = rng.uniform(-30.0, -20.0, (1, 1, etable.shape[3]))
        slope = rng.uniform(-1.0, 1.0) * (ttable[:, None, None] / 3000.0)
        extra.append(10.0**np.clip(base + slope + 0.1 * np.log10(press)[None, :, None],
                                   -30.0, -20.0))
    return np.stack([etable[0], etable[1], extra[0], extra[1], etable[2], etable[3]])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--kernel-launches', type=int, default=200)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine, isotopes as iso
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    table = engine.dev(six_slot_table(inp))
    ratios = iso.IsotopeRatios(NAMES, LABELS, iso.parse(BLOCK))
    models = {'isotopes': engine.TableSpectrum(table, inp['ttable'], wn, atm['radius'],
                                               atm['rstar'], isotopes=ratios),
              'prescaled': engine.TableSpectrum(table, inp['ttable'], wn, atm['radius'],
                                                atm['rstar'])}
    pb = engine.PassBands(wn, inp['bands'])
    batches = []
    for b in range(4):
        rng = np.random.default_rng(2900 + b)
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 700 + b)
        dens = np.ascontiguousarray(dens[:, :, SLOT_SPECIES])
        pars = np.column_stack([rng.uniform(-2.5, -1.5, BATCH), rng.uniform(-3.2, -2.2, BATCH)])
        scaled = ratios.scale_host(temps, dens, pars)[1]
        batches.append(dict(temps=engine.dev(temps), dens=engine.dev(dens),
                            radius=engine.dev(radius), pars=engine.dev(pars),
                            scaled=engine.dev(scaled)))

    def step(leg, i):
        b = batches[i % len(batches)]
        if leg == 'isotopes':
            return models[leg].eval_bands(b['temps'], b['dens'], pb, radius=b['radius'],
                                          chunk=bench_c5.CHUNK, iso_pars=b['pars'])
        return models[leg].eval_bands(b['temps'], b['scaled'], pb, radius=b['radius'],
                                      chunk=bench_c5.CHUNK)
    out = {}
    for leg in models:
        for i in range(max(args.warmup, len(batches))):
            out[leg] = step(leg, i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in models}
    for _ in range(args.blocks):
        for leg in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                out[leg] = step(leg, i)
            torch.cuda.synchronize()
            times[leg].append(1e3 * (time.perf_counter() - t0) / args.steps)
    # the host's 10.0**par against the device's pow: equal band fluxes where the ratios agree
    same = [bool(torch.equal(step('isotopes', i), step('prescaled', i)))
            for i in range(len(batches))]
    worst = max(float(((step('isotopes', i) / step('prescaled', i)) - 1).abs().max())
                for i in range(len(batches)))
    b = batches[0]
    for _ in range(10):
        ratios.scale(b['temps'], b['dens'], b['pars'])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel = []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.kernel_launches):
            ratios.scale(b['temps'], b['dens'], b['pars'])
        stop.record()
        torch.cuda.synchronize()
        kernel.append(start.elapsed_time(stop) / args.kernel_launches)
    nlayers = b['temps'].shape[1]
    moved = 16 * BATCH * nlayers * len(NAMES) + 16 * BATCH * nlayers + 8 * BATCH * 2 + 4 * BATCH
    res = {'workload': 'c5-isotopes', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'blocks': args.blocks, 'table_slots': len(NAMES),
           'ordered_columns': models['isotopes'].column_order is not None,
           'kernel_bytes': moved, 'equal_band_fluxes': same, 'worst_rel_difference': worst}
    for leg, t in times.items():
        res[leg] = {'ms_per_batch': float(np.median(t)), 'min': min(t), 'max': max(t)}
    res['kernel'] = {'ms_per_launch': float(np.median(kernel)), 'min': min(kernel),
                     'max': max(kernel), 'launches': args.kernel_launches}
    res['isotopes_over_prescaled'] = res['isotopes']['ms_per_batch'] / \
        res['prescaled']['ms_per_batch']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
