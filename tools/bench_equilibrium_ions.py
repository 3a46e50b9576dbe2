#!/usr/bin/env python3
"""The C5 batch with equilibrium chemistry (tools/bench_equilibrium.py: 64 walkers x 80 layers x
1e5 samples, Guillot T(p), [M/H], C/O and rplanet free, seed 7) on a network with ions and
electrons: the 16 species of tests/chemistry_cases.py with H+, H-, e-, Na, Na+, K and K+ added
(tests/ion_cases.py: 23 species, 7 elements and the charge balance), against the neutral 16-species
network in the same process.

Figures, each the median of `--blocks` timed blocks of `--steps` batches after a warm-up
(min ... max beside it):
  b   eval_params, neutral network, no continuum        (tools/bench_equilibrium.py's b)
  bi  eval_params, ion network, no continuum
  bh  eval_params, ion network, a Continuum with H- (its H and e- columns from the equilibrium)
  d   the equilibrium launch alone, neutral network, ms per 64 x 80 cells
  di  the equilibrium launch alone, ion network
and per network the iterations per cell (min, mean, max), for the ion network also those of the
neutral step alone (the host's count on the first walker), the cells that did not converge, the
device against the host on the first walker, and the worst neutrality of the batch.
Prints one JSON line.  Measured: profiles/chemistry_ions.md.

    python tools/bench_equilibrium_ions.py [--steps K] [--blocks B] [--warmup W]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import chemistry_cases as cc  # noqa: E402
import ion_cases as ic  # noqa: E402
from tools import bench_c5, bench_c5_atmosphere, bench_equilibrium  # noqa: E402
from tools.bench_c5_atmosphere import blocks  # noqa: E402

BATCH = bench_c5.BATCH
BASE = bench_equilibrium.BASE


def ion_atmosphere(inp, net, mass, continuum=None):
    from pyratbay_amd import atmosphere as pa
    pressure = inp['atm']['press']
    tmodel = pa.Guillot(pressure, bench_c5_atmosphere.GRAVITY)
    vmr_models = [pa.MetalEquil(), pa.RatioEquil('C/O')]
    free = list(tmodel.pnames) + [m.pnames[0] for m in vmr_models] + ['rplanet']
    model = pa.WalkerAtmosphere(pressure, net.species, mass, None, None, tmodel, vmr_models,
                                rmodel='hydro_m', mplanet=0.6 * 1.8982e30, refpressure=0.1,
                                free=free, base_params=BASE, chemistry=net)
    return model.bind(inp['atm']['species'][2:2 + bench_c5.NSPEC], continuum)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import chemistry, continuum as ct, engine
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    neutral = cc.network(chemistry)
    ions, mass, _ = ic.sixteen_with_ions(chemistry)
    cont = ct.Continuum(g['wn'], atm['press'], [ct.Hydrogen_Ion(g['wn'])])
    atms = {'b': bench_equilibrium.atmosphere(inp, neutral),
            'bi': ion_atmosphere(inp, ions, mass),
            'bh': ion_atmosphere(inp, ions, mass, cont)}
    models = {k: engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], a.base_radius,
                                      atm['rstar'], rt_path='transit',
                                      continuum=cont if k == 'bh' else None)
              for k, a in atms.items()}
    pb = engine.PassBands(g['wn'], inp['bands'])
    rng = np.random.default_rng(7)
    base = np.array(BASE)
    params_h = [base * (1.0 + 0.1 * rng.uniform(-1, 1, (BATCH, len(base)))) for _ in range(4)]
    params = [engine.dev(p) for p in params_h]

    def sync():
        torch.cuda.synchronize()
    res = {'workload': 'c5-equilibrium-ions', 'walkers_per_batch': BATCH,
           'layers': atms['b'].nlayers, 'steps': args.steps, 'blocks': args.blocks}
    launches = {}
    for key, net, a in (('neutral', neutral, atms['b']), ('ions', ions, atms['bi'])):
        prof = a.evaluate(params[0])
        sync()
        launch = a.equilibrium_launch(BATCH, params[0].device)
        launches[key] = launch
        status, vmr = launch['status'].cpu().numpy(), launch['vmr'].cpu().numpy()
        ok = status > 0
        p = params_h[0][0]
        b = net.element_abundances_host(p[6], None, {'C/O': p[7]})
        temps0 = launch['temps'][0].cpu().numpy()
        host_vmr, _, host_status = net.equilibrium_host(temps0, a.pressure, b)
        seen = (host_vmr >= 1e-250) & ok[0][:, None]
        info = {'species': net.nspecies, 'elements': net.nelements,
                'rejected_walkers': int((prof.reject != 0).sum().item()),
                'cells': int(status.size), 'cells_not_converged': int((~ok).sum()),
                'iterations': {'min': int(status[ok].min()), 'mean': float(status[ok].mean()),
                               'max': int(status[ok].max())},
                'iterations_sum': int(status[ok].sum()),
                'host_iterations_walker0': {'min': int(host_status.min()),
                                            'mean': float(host_status.mean()),
                                            'max': int(host_status.max())},
                'device_vs_host_max_rel_walker0':
                    float(np.max(np.abs(vmr[0][seen] / host_vmr[seen] - 1.0)))}
        if net.charged:
            keep = net.charges == 0
            sub = chemistry.ChemNetwork([s for s, k in zip(net.species, keep) if k], net.elements,
                                        net.stoich[keep], net.gibbs_temps,
                                        net.gibbs_over_RT[:, keep], net.base_dex)
            first = sub.equilibrium_host(temps0, a.pressure, b)[1]
            info['host_neutral_step_walker0'] = {'min': int(first.min()),
                                                 'mean': float(first.mean()),
                                                 'max': int(first.max())}
            info['neutrality_max'] = float(ic.neutrality(net, vmr[ok]).max())
            info['electron_vmr'] = {'min': float(vmr[ok][:, net.species.index('e-')].min()),
                                    'max': float(vmr[ok][:, net.species.index('e-')].max())}
        res[key] = info

    def leg(key):
        return lambda i: models[key].eval_params(atms[key], params[i % 4], pb,
                                                 chunk=bench_c5.CHUNK)

    def launch_leg(key, net):
        la = launches[key]
        return lambda i: chemistry.equilibrium_vmr(net, la['temps'], la['pressure'], params[0],
                                                   out=(la['vmr'], la['status']), **la['columns'])
    legs = {k: leg(k) for k in ('b', 'bi', 'bh')}
    legs['d'], legs['di'] = launch_leg('neutral', neutral), launch_leg('ions', ions)
    for i in range(args.warmup):
        for f in legs.values():
            f(i)
    sync()
    # the eval_params legs alternate block by block, so that drift of the clocks hits all alike
    times = {k: [] for k in ('b', 'bi', 'bh')}
    for _ in range(args.blocks):
        for k in times:
            times[k].append(blocks(legs[k], args.steps, 1, sync)['median_ms'])
    for k, v in times.items():
        res[k + '_eval_params'] = {'median_ms': float(np.median(v)), 'min_ms': min(v),
                                   'max_ms': max(v)}
    for k in ('d', 'di'):
        res[k + '_equilibrium_launch'] = blocks(legs[k], 20 * args.steps, args.blocks, sync)
    d, di = (res[k + '_equilibrium_launch']['median_ms'] for k in ('d', 'di'))
    res['di_over_d'] = di / d
    res['iterations_ratio'] = res['ions']['iterations_sum'] / res['neutral']['iterations_sum']
    res['d_us_per_cell_iteration'] = 1e3 * d / res['neutral']['iterations_sum']
    res['di_us_per_cell_iteration'] = 1e3 * di / res['ions']['iterations_sum']
    res['bi_over_b'] = res['bi_eval_params']['median_ms'] / res['b_eval_params']['median_ms']
    res['bh_over_b'] = res['bh_eval_params']['median_ms'] / res['b_eval_params']['median_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
