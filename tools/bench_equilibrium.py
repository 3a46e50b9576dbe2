#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 table
species, transit) with equilibrium chemistry per walker: Guillot T(p), [M/H] and C/O free, hydro_m
with rplanet free (9 parameters), within +-10 % of a base vector, seed 7, on the 16-species
C-H-N-O-He network and synthetic Gibbs table of tests/chemistry_cases.py.

Figures, each the median of `--blocks` timed blocks of `--steps` batches after a warm-up
(min ... max beside it), all in one process:
  a  eval_params with free VMRs (tools/bench_c5_atmosphere.py's model: what the loop could do)
  b  eval_params with [M/H] and C/O free            (parameters in, band fluxes out)
  c  WalkerAtmosphere.evaluate with chemistry alone (three launches), ms per 64 walkers
  d  the equilibrium launch alone, ms per 64 x 80 cells, and its share of b
  e  ChemNetwork.equilibrium_host over the same cells (NumPy, all cells of a walker at once)
and the iterations per cell (min, mean, max) with the count of cells that did not converge.
Prints one JSON line.  Measured: profiles/chemistry.md.

    python tools/bench_equilibrium.py [--steps K] [--blocks B] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import chemistry_cases as cc  # noqa: E402
from tools import bench_c5, bench_c5_atmosphere  # noqa: E402
from tools.bench_c5_atmosphere import blocks  # noqa: E402

BATCH = bench_c5.BATCH
# log kappa', log gamma1, log gamma2, alpha, T_irr, T_int | [M/H], C/O | rplanet (cm)
BASE = [-1.5, -0.8, -0.8, 0.5, 1200.0, 100.0, 0.3, 0.55, 7.1492e9]


def atmosphere(inp, net):
    from pyratbay_amd import atmosphere as pa
    pressure = inp['atm']['press']
    tmodel = pa.Guillot(pressure, bench_c5_atmosphere.GRAVITY)
    vmr_models = [pa.MetalEquil(), pa.RatioEquil('C/O')]
    free = list(tmodel.pnames) + [m.pnames[0] for m in vmr_models] + ['rplanet']
    model = pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel, vmr_models,
                                rmodel='hydro_m', mplanet=0.6 * 1.8982e30, refpressure=0.1,
                                free=free, base_params=BASE, chemistry=net)
    return model.bind(inp['atm']['species'][2:2 + bench_c5.NSPEC])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import chemistry, engine
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    net = cc.network(chemistry)
    free_atm = bench_c5_atmosphere.atmosphere(inp)
    chem_atm = atmosphere(inp, net)
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], chem_atm.base_radius,
                                 atm['rstar'], rt_path='transit')
    pb = engine.PassBands(g['wn'], inp['bands'])
    rng = np.random.default_rng(7)

    def draw(base):
        base = np.array(base)
        return [base * (1.0 + 0.1 * rng.uniform(-1, 1, (BATCH, len(base)))) for _ in range(4)]
    free_params = [engine.dev(p) for p in draw(bench_c5_atmosphere.BASE)]
    chem_params_h = draw(BASE)
    chem_params = [engine.dev(p) for p in chem_params_h]
    profs = [chem_atm.evaluate(p) for p in chem_params]
    rejected = int(sum(int((p.reject != 0).sum().item()) for p in profs))
    L = chem_atm.nlayers
    launch = chem_atm.equilibrium_launch(BATCH, chem_params[0].device)
    temps_d, vmr_d, status_d = launch['temps'], launch['vmr'], launch['status']
    pressure_d, columns = launch['pressure'], launch['columns']
    chem_atm.evaluate(chem_params[0])
    torch.cuda.synchronize()
    status = status_d.cpu().numpy()
    temps_h = temps_d.cpu().numpy()
    vmr_dev = vmr_d.cpu().numpy()

    def sync():
        torch.cuda.synchronize()

    def leg_a(i):
        return model.eval_params(free_atm, free_params[i % 4], pb, chunk=bench_c5.CHUNK)

    def leg_b(i):
        return model.eval_params(chem_atm, chem_params[i % 4], pb, chunk=bench_c5.CHUNK)

    def leg_c(i):
        return chem_atm.evaluate(chem_params[i % 4], out=profs[i % 4])

    def leg_d(i):
        return chemistry.equilibrium_vmr(net, temps_d, pressure_d, chem_params[0],
                                         out=(vmr_d, status_d), **columns)

    def host_cells():
        out = []
        for w in range(BATCH):
            p = chem_params_h[0][w]
            b = net.element_abundances_host(p[6], None, {'C/O': p[7]})
            out.append(net.equilibrium_host(temps_h[w], chem_atm.pressure, b)[0])
        return np.stack(out)
    for i in range(args.warmup):
        leg_a(i), leg_b(i), leg_c(i), leg_d(i)
    sync()
    ok = status > 0
    res = {'workload': 'c5-equilibrium', 'walkers_per_batch': BATCH, 'layers': L,
           'species': net.nspecies, 'elements': net.nelements, 'steps': args.steps,
           'blocks': args.blocks, 'rejected_walkers': rejected,
           'cells': int(status.size), 'cells_not_converged': int((~ok).sum()),
           'iterations': {'min': int(status[ok].min()), 'mean': float(status[ok].mean()),
                          'max': int(status[ok].max())}}
    # a and b alternate block by block, so that drift of the clocks hits both alike
    la, lb = [], []
    for _ in range(args.blocks):
        la.append(blocks(leg_a, args.steps, 1, sync)['median_ms'])
        lb.append(blocks(leg_b, args.steps, 1, sync)['median_ms'])
    for key, v in (('a_eval_params_free_vmr', la), ('b_eval_params_equilibrium', lb)):
        res[key] = {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v),
                    'evals_per_s': 1e3 * BATCH / float(np.median(v))}
    res['c_evaluate'] = blocks(leg_c, 20 * args.steps, args.blocks, sync)
    res['d_equilibrium_launch'] = blocks(leg_d, 20 * args.steps, args.blocks, sync)
    res['d_share_of_b'] = res['d_equilibrium_launch']['median_ms'] / \
        res['b_eval_params_equilibrium']['median_ms']
    res['d_us_per_cell_iteration'] = 1e3 * res['d_equilibrium_launch']['median_ms'] / \
        float(status[ok].sum())
    t0 = time.perf_counter()
    host_vmr = host_cells()
    res['e_equilibrium_host_ms'] = 1e3 * (time.perf_counter() - t0)
    res['e_over_d'] = res['e_equilibrium_host_ms'] / res['d_equilibrium_launch']['median_ms']
    seen = (host_vmr >= 1e-250) & ok[:, :, None]
    res['device_vs_host_max_rel'] = float(np.max(np.abs(vmr_dev[seen] / host_vmr[seen] - 1.0)))
    res['b_minus_a_ms'] = res['b_eval_params_equilibrium']['median_ms'] - \
        res['a_eval_params_free_vmr']['median_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
