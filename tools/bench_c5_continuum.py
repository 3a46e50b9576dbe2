#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 species) with
continuum opacity, as a retrieval with CIA and clouds runs it: TableSpectrum.eval_bands with a
Continuum whose terms the interpolation adds before it stores ec (pb_interp_ec_batch_cont).

Continuum (synthetic, smooth): CIA H2-H2 and H2-He (21 temperatures 50-7000 K, tabulated on a
coarse grid inside the model's and spline-resampled to it, so that each has a validity window),
Rayleigh H2 + He, and a Lecavelier haze whose (log_k, alpha) differ per walker; the emission
variant adds H- bound-free + free-free.  Prints one JSON line: evals/s with and without the
continuum, transit and emission, and the interpolation kernel's mean time per launch (64 walkers)
from a `rocprofv3 --kernel-trace --stats` run of its own (a child process, before this process
touches the GPU; --no-prof skips it).

    python tools/bench_c5_continuum.py [--steps K] [--warmup W] [--no-prof]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import bench_c5  # noqa: E402

BATCH = bench_c5.BATCH


def continuum_models(wn, pressure, hminus):
    from pyratbay_amd import continuum as ct
    rng = np.random.default_rng(11)
    temps = np.linspace(50.0, 7000.0, 21)
    tab_wn = np.linspace(wn[0] + 300.0, wn[-1] - 300.0, 400)
    models = [ct.Kurucz(wn, 'H2'), ct.Kurucz(wn, 'He'), ct.Lecavelier(pressure, wn=wn)]
    for species, amp in ((['H2', 'H2'], 1e-8), (['H2', 'He'], 3e-9)):
        shape = np.exp(-((tab_wn - tab_wn.mean()) / (0.4 * np.ptp(tab_wn)))**2)
        absorption = amp * (1 + 0.1 * rng.uniform(-1, 1)) * \
            np.sqrt(temps[:, None] / 1000.0) * shape[None, :]
        models.append(ct.Collision_Induced(table=(absorption, species, temps, tab_wn), wn=wn))
    if hminus:
        models.append(ct.Hydrogen_Ion(wn))
    return ct.Continuum(wn, pressure, models)


def continuum_inputs(inp, cont, temps, seed):
    """continuum_density[n, L, ncs] (H2, He from the synthetic atmosphere, H and e- at fixed
    fractions) and per-walker Lecavelier (log_k, alpha)."""
    rng = np.random.default_rng(seed)
    atm = inp['atm']
    n = temps.shape[0]
    ntot = atm['press'] * 1e6 / temps / 1.380649e-16
    vmr = {'H2': 0.85, 'He': 0.149, 'H': 1e-5, 'e-': 1e-8}
    cdens = np.stack([ntot * vmr[s] for s in cont.species], axis=-1)
    pars = np.stack([rng.uniform(-1, 1, n), rng.uniform(-6, -2, n)], axis=1)
    return cdens, pars


_INPUTS = []


def run(rt, with_cont, steps, warmup):
    import torch
    from pyratbay_amd import engine
    if not _INPUTS:
        _INPUTS.append(bench_c5.inputs())
    inp = _INPUTS[0]
    g, atm = inp['grid'], inp['atm']
    cont = continuum_models(g['wn'], atm['press'], rt == 'emission') if with_cont else None
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], atm['radius'],
                                 atm['rstar'], rt_path=rt, continuum=cont)
    pb = engine.PassBands(g['wn'], inp['bands'])
    batches = []
    for b in range(4):
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 700 + b)
        kw = {}
        if cont is not None:
            cdens, pars = continuum_inputs(inp, cont, temps, 900 + b)
            kw = dict(continuum_density=engine.dev(cdens), continuum_pars=engine.dev(pars))
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
    del model, batches
    torch.cuda.empty_cache()
    return {'evals_per_s': steps * BATCH / elapsed, 'ms_per_batch': 1e3 * elapsed / steps,
            'finite': finite}


def profile(steps):
    """Mean time per launch of the interpolation kernels (the continuum's: template argument
    kCont = 1, 2 last), from rocprofv3 kernel stats of a child running every leg."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out = tempfile.mkdtemp(prefix='pb_c5cont_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--',
           sys.executable, os.path.abspath(__file__), '--inner', '--steps', str(steps),
           '--warmup', '2']
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return {'error': f'rocprofv3 exit {r.returncode}', 'tail': r.stderr[-400:]}
        res = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row['Name']
                if 'k_interp_ec_batch' in name or 'k_cont_' in name:
                    key = name.replace('void ', '').replace('(anonymous namespace)::', '')
                    key = key.split('(')[0]
                    res[key] = {'calls': int(row['Calls']),
                                'mean_ms': float(row['AverageNs']) * 1e-6}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-prof', action='store_true')
    ap.add_argument('--inner', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:                     # (the profiled child)
        for rt in ('transit', 'emission'):
            for with_cont in (False, True):
                run(rt, with_cont, args.steps, args.warmup)
        return
    prof = None if args.no_prof else profile(min(args.steps, 10))
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-continuum', 'walkers_per_batch': BATCH, 'steps': args.steps}
    for rt in ('transit', 'emission'):
        plain = run(rt, False, args.steps, args.warmup)
        cont = run(rt, True, args.steps, args.warmup)
        res[rt] = {'plain': plain, 'continuum': cont,
                   'slowdown': plain['evals_per_s'] / cont['evals_per_s']}
    res['continuum'] = {'transit': 'CIA H2-H2 + H2-He, Rayleigh H2 + He, Lecavelier per walker',
                        'emission': 'the same + H- bound-free/free-free'}
    if prof is not None:
        res['interp_kernels_rocprofv3'] = prof
    print(json.dumps(res))


if __name__ == '__main__':
    main()
