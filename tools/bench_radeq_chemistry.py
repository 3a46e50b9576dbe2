#!/usr/bin/env python3
"""The radiative-equilibrium iteration with the equilibrium chemistry of every iteration
(RadiativeEquilibrium(chemistry=...), csrc/pb_chemistry.hip: pb_radeq_equilibrium) at the table
shape of tools/bench_radeq.py (80 layers x 100001 samples, table species H2O CO CO2 CH4), for 1
and 64 profiles, hydro_m radius, tint = 300 K and an irradiation row; the 16-species C-H-N-O-He
network and synthetic Gibbs table of tests/chemistry_cases.py, solar [M/H] and C/O = 0.55.

Legs, each in ms per iteration (the whole batch of nw profiles):
  fixed_loop      the loop at fixed VMRs, as tools/bench_radeq.py measures it (three launches)
  cold_loop       the loop with chemistry_start='cold' (five launches)
  previous_loop   the loop with chemistry_start='previous'
  eq_cold / eq_warm   pb_radeq_equilibrium alone on the state the loop left: from the cold start,
                  and from the stored iterate at temperatures moved by the last iteration's step
  update_temps_only / update_init   the two halves the update is split into
and, over the 32 iterations of a run, the solver's iteration counts per cell (min, mean, max) of
both settings, the failed solves, and the largest relative difference of the two trajectories.
Prints one JSON line.  Kernel times are device-side (events around `--steps` back-to-back
launches); the loops are wall clock over whole runs of 32 iterations with a synchronisation at
both ends, tools/bench_radeq.py's method.

    python tools/bench_radeq_chemistry.py [--steps K] [--warmup W] [--profiles 1,64]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import chemistry_cases as cc  # noqa: E402
from tools import bench_c5  # noqa: E402
from tools.bench_radeq import MJUP, RJUP, TINT, device_ms, wall_ms  # noqa: E402

NITER = 32


def run(inp, nw, steps, warmup):
    import torch
    from pyratbay_amd import _capi, chemistry, engine
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    flux_top = 0.25 * (atm['rstar'] / 7.5e11)**2 * 2.0e6 * (1.0 + 0.1 * np.sin(wn / 70.0))
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'],
                                 rt_path='two_stream', tint=TINT, flux_top=flux_top,
                                 timestamps=False)
    kw = dict(radius_model='hydro_m', mplanet=0.6 * MJUP, p0=0.1, r0=1.0 * RJUP, tint=TINT,
              flux_top=flux_top, table_species=atm['species'][2:6])
    rng = np.random.default_rng(5)
    temp0 = atm['temp'][None, :] * (1.0 + 0.05 * rng.uniform(-1, 1, (nw, 1)))
    res = {'profiles': nw}
    repeats = max(steps // 8, 1)
    fixed = model.radiative_equilibrium(atm['press'], atm['vmr'], atm['mol_mass'],
                                        species=atm['species'], **kw)
    res['fixed_loop_ms'] = wall_ms(lambda: fixed.run(temp0, NITER), repeats, 1) / NITER
    del fixed
    torch.cuda.empty_cache()
    net = cc.network(chemistry)
    runs = {}
    for start in ('cold', 'previous'):
        re = model.radiative_equilibrium(atm['press'], None, cc.MASS, chemistry=net,
                                         metallicity=0.0, e_ratio={'C/O': 0.55},
                                         chemistry_start=start, **kw)
        res[f'{start}_loop_ms'] = wall_ms(lambda: re.run(temp0, NITER), repeats, 1) / NITER
        temps = re.run(temp0, NITER, diagnostics=True)
        its = re.history['chem_iterations'].cpu().numpy()
        res[f'{start}_iterations'] = [int(its.min()), round(float(its.mean()), 2), int(its.max())]
        res[f'{start}_failures'] = int(re.chem_failures.sum())
        runs[start] = temps.cpu().numpy()
        res['finite'] = res.get('finite', True) and bool(torch.isfinite(temps).all())
        if start == 'cold':
            del re
            torch.cuda.empty_cache()
    res['previous_minus_cold_ms'] = res['previous_loop_ms'] - res['cold_loop_ms']
    res['cold_minus_fixed_ms'] = res['cold_loop_ms'] - res['fixed_loop_ms']
    res['previous_minus_fixed_ms'] = res['previous_loop_ms'] - res['fixed_loop_ms']
    res['trajectories_differ_by'] = float(np.max(np.abs(runs['previous'] / runs['cold'] - 1.0)))
    # the launches alone, on the state the 'previous' loop left: the VMRs and iterate are those of
    # the last row, one step away from the row before
    d = re._state
    chem, st = d['chem'], d['struct']
    last, before = re.temps[:, -1].contiguous(), re.temps[:, -2].contiguous()
    res['eq_cold_ms'] = device_ms(lambda: chem.solve(last, False), steps, warmup)

    def warm():
        # (each launch overwrites the iterate: alternate the two rows, so that every solve starts
        # one step of the loop away from its solution)
        chem.solve(before, True)
        chem.solve(last, True)
    res['eq_warm_ms'] = device_ms(warm, steps, warmup) / 2.0
    res['step_kelvin_max'] = float((last - before).abs().max())

    def update(init_only):
        d['iter'].zero_()
        _capi.call('pb_radeq_update', C.byref(st), init_only, engine._stream())
    res['update_temps_only_ms'] = device_ms(lambda: update(0), steps, warmup)
    res['update_init_ms'] = device_ms(lambda: update(1), steps, warmup)
    del model, re, d
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profiles', default='1,64')
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    res = {'workload': 'c5-radeq-chemistry', 'steps': args.steps,
           'shape': [bench_c5.NLAYERS, bench_c5.NWAVE, bench_c5.NSPEC]}
    for nw in (int(v) for v in args.profiles.split(',')):
        res[f'nw{nw}'] = run(inp, nw, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
