#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 table
species, transit) driven from the walkers' PARAMETER vectors: Guillot T(p) + 3 IsoVMR + hydro_m
with rplanet free (10 parameters), within +-10 % of a base vector, seed 7.

Five figures, each the median of `--blocks` timed blocks of `--steps` batches after a warm-up
(min ... max beside it), all in one process on the same walkers:
  a  eval_bands on profiles made in advance           (what the loop could already do)
  b  eval_params: evaluate + eval_bands               (parameters in, band fluxes out)
  c  WalkerAtmosphere.evaluate alone, ms per 64 walkers
  d  the host route: evaluate_host per walker + stacking + upload, ms per 64 walkers
  e  d over a: the host mapping against the 64 evaluations it feeds
Prints one JSON line.  Measured: profiles/atmosphere.md.

    python tools/bench_c5_atmosphere.py [--steps K] [--blocks B] [--warmup W]
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
GRAVITY = 2200.0
# log kappa', log gamma1, log gamma2, alpha, T_irr, T_int | log H2O, CO, CH4 | rplanet (cm)
BASE = [-1.5, -0.8, -0.8, 0.5, 1200.0, 100.0, -3.4, -3.3, -4.0, 7.1492e9]


def atmosphere(inp):
    from pyratbay_amd import atmosphere as pa
    atm = inp['atm']
    pressure, species = atm['press'], atm['species']
    tmodel = pa.Guillot(pressure, GRAVITY)
    vmr_models = [pa.IsoVMR(s, pressure) for s in ('H2O', 'CO', 'CH4')]
    free = list(tmodel.pnames) + [m.pnames[0] for m in vmr_models] + ['rplanet']
    model = pa.WalkerAtmosphere(pressure, species, atm['mol_mass'], atm['vmr'], ['H2', 'He'],
                                tmodel, vmr_models, rmodel='hydro_m', mplanet=0.6 * 1.8982e30,
                                refpressure=0.1, free=free, base_params=BASE)
    return model.bind(species[2:2 + bench_c5.NSPEC])


def blocks(fn, steps, nblocks, sync):
    out = []
    for _ in range(nblocks):
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        sync()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return {'median_ms': float(np.median(out)), 'min_ms': min(out), 'max_ms': max(out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    watm = atmosphere(inp)
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], watm.base_radius,
                                 atm['rstar'], rt_path='transit')
    pb = engine.PassBands(g['wn'], inp['bands'])
    rng = np.random.default_rng(7)
    base = np.array(BASE)
    params_h = [base * (1.0 + 0.1 * rng.uniform(-1, 1, (BATCH, len(base)))) for _ in range(4)]
    params = [engine.dev(p) for p in params_h]
    made = [type(p)(*[None if t is None else t.clone() for t in p])
            for p in (watm.evaluate(q) for q in params)]
    rejected = int(sum(int((p.reject != 0).sum().item()) for p in made))

    def sync():
        torch.cuda.synchronize()

    def leg_a(i):
        p = made[i % 4]
        return model.eval_bands(p.temps, p.dens, pb, radius=p.radius, chunk=bench_c5.CHUNK)

    def leg_b(i):
        return model.eval_params(watm, params[i % 4], pb, chunk=bench_c5.CHUNK)

    def leg_c(i):
        return watm.evaluate(params[i % 4])

    def leg_d(i):
        rows = [watm.evaluate_host(p) for p in params_h[i % 4]]
        return [engine.dev(np.stack([getattr(r, name) for r in rows]))
                for name in ('temps', 'dens', 'radius')]
    for i in range(args.warmup):
        a, b = leg_a(i), leg_b(i)
        leg_c(i)
    leg_d(0)
    sync()
    same = bool(torch.equal(leg_a(0), leg_b(0)))
    res = {'workload': 'c5-atmosphere', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'blocks': args.blocks, 'npar': len(base), 'rejected_walkers': rejected,
           'eval_params_equals_eval_bands': same}
    # a and b alternate block by block, so that drift of the clocks hits both alike
    la, lb = [], []
    for _ in range(args.blocks):
        la.append(blocks(leg_a, args.steps, 1, sync)['median_ms'])
        lb.append(blocks(leg_b, args.steps, 1, sync)['median_ms'])
    for key, v in (('a_eval_bands', la), ('b_eval_params', lb)):
        res[key] = {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v),
                    'evals_per_s': 1e3 * BATCH / float(np.median(v))}
    res['c_evaluate'] = blocks(leg_c, 50 * args.steps, args.blocks, sync)
    res['d_host_route'] = blocks(leg_d, max(2, args.steps // 10), args.blocks, sync)
    res['e_host_over_loop'] = res['d_host_route']['median_ms'] / res['a_eval_bands']['median_ms']
    res['b_minus_a_ms'] = res['b_eval_params']['median_ms'] - res['a_eval_bands']['median_ms']
    res['a_spread_ms'] = res['a_eval_bands']['max_ms'] - res['a_eval_bands']['min_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
