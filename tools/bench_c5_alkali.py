#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 species) with
the Na and K resonance doublets per walker, as an optical retrieval of a hot Jupiter runs it:
TableSpectrum.eval_bands(..., alkali_density=...), the doublets added in the store of the batched
interpolation (pb_interp_ec_batch_cont, kernel template argument kAlk).

The grid is moved to the optical, 8500-21500 cm-1, so that both doublets' +-4500 cm-1 windows lie
inside it: every sample is inside at least one window, most inside both (up to 4 FP64 exp per
stored sample).  Three cases, transit and emission, evals/s each:
  plain  CIA H2-H2 + H2-He and Rayleigh H2 + He alone (tools/bench_c5_continuum.py's tables)
  fused  the same + Na + K in the one batched call
  split  what the same walkers cost without the batched form: the batch without the alkali
         models' densities (the interpolation stores ec with CIA + Rayleigh), then per walker the
         host voigt_det (SciPy), its upload and pb_alkali_cross_section per species on that
         walker's ec, then the batched geometry and band integration (grid order, every layer:
         the second pass needs all of ec)
and the interpolation kernels' mean time per launch (64 walkers) from a `rocprofv3 --kernel-trace
--stats` run of its own (a child process, before this process touches the GPU; --no-prof skips
it).  Prints one JSON line.  Measured: profiles/alkali.md.

    python tools/bench_c5_alkali.py [--steps K] [--warmup W] [--no-prof]
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

from tools import bench_c5, bench_c5_continuum  # noqa: E402

BATCH = bench_c5.BATCH
WN_LO, WN_HI = 8500.0, 21500.0
VMR = {'Na': 2e-6, 'K': 1.5e-7}

_INPUTS = []


def inputs():
    """bench_c5's table, atmosphere and bands on an optical grid of the same length."""
    if not _INPUTS:
        inp = bench_c5.inputs()
        wn = np.linspace(WN_LO, WN_HI, inp['grid']['nwave'])
        inp['grid'] = dict(inp['grid'], wn=wn)
        inp['bands'] = [(lo, resp, 1.0 / np.trapezoid(resp, wn[lo:lo + len(resp)]))
                        for lo, resp, _ in inp['bands']]
        _INPUTS.append(inp)
    return _INPUTS[0]


def models(inp, alkali):
    from pyratbay_amd import continuum as ct
    wn, pressure = inp['grid']['wn'], inp['atm']['press']
    cont = bench_c5_continuum.continuum_models(wn, pressure, False)
    keep = [m for m in cont.rank1 if isinstance(m, ct.Kurucz)] + cont.cia
    if alkali:
        keep += [ct.SodiumVdW(pressure, wn=wn), ct.PotassiumVdW(pressure, wn=wn)]
    return ct.Continuum(wn, pressure, keep)


def add_alkali(cont, ec, temp_h, dens_h):
    """The alkali part of Continuum.add on one walker's ec: host voigt_det, one upload, one
    launch per species."""
    from pyratbay_amd import engine
    from pyratbay_amd._capi import call, hptr
    nlayers = len(temp_h)
    vds = [np.ascontiguousarray(m.voigt_det(temp_h), float).ravel() for m in cont.alkali]
    packed = engine.dev(np.concatenate([temp_h] + [dens_h[:, i] for i in range(len(vds))] + vds))
    at = (1 + len(vds)) * nlayers
    for i, m in enumerate(cont.alkali):
        vd = packed[at:at + len(vds[i])]
        at += len(vds[i])
        call('pb_alkali_cross_section', ec.data_ptr(), cont.pressure_barye.data_ptr(),
             cont.wn.data_ptr(), packed[:nlayers].data_ptr(), vd.data_ptr(), float(m.detuning),
             float(m.mass), float(m.lpar), float(m.Z), float(m.cutoff),
             hptr(np.array(m.wn0, float)), hptr(np.array(m.gf, float)), m.nlines,
             packed[(1 + i) * nlayers:(2 + i) * nlayers].data_ptr(), nlayers, cont.nwave,
             engine._stream())


def run(rt, case, steps, warmup):
    import torch
    from pyratbay_amd import engine
    inp = inputs()
    g, atm = inp['grid'], inp['atm']
    cont = models(inp, case != 'plain')
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], atm['radius'],
                                 atm['rstar'], rt_path=rt, continuum=cont,
                                 column_order=None if case == 'split' else 'auto')
    pb = engine.PassBands(g['wn'], inp['bands'])
    batches = []
    for b in range(4):
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 700 + b)
        ntot = atm['press'] * 1e6 / temps / 1.380649e-16
        cdens = np.stack([ntot * {'H2': 0.85, 'He': 0.149}[s] for s in cont.species], axis=-1)
        adens = np.stack([ntot * VMR[s] for s in ('Na', 'K')], axis=-1)
        batches.append(dict(temps=engine.dev(temps), dens=engine.dev(dens),
                            radius=engine.dev(radius), cdens=engine.dev(cdens),
                            adens=engine.dev(adens), temps_h=temps, adens_h=adens))

    def step(i):
        b = batches[i % len(batches)]
        if case != 'split':
            kw = dict(alkali_density=b['adens']) if case == 'fused' else {}
            return model.eval_bands(b['temps'], b['dens'], pb, radius=b['radius'],
                                    chunk=bench_c5.CHUNK, continuum_density=b['cdens'], **kw)
        # the batch without the alkali densities stores ec with CIA + Rayleigh ...
        ec = engine.interp_ec_batch(model.etable, model.ttable, b['temps'], b['dens'],
                                    continuum=cont, continuum_density=b['cdens'])
        # ... and the doublets go on top walker by walker
        for w in range(BATCH):
            add_alkali(cont, ec[w], b['temps_h'][w], b['adens_h'][w])
        rad = b['radius']
        if rt == 'transit':
            spectra = engine.transit_spectrum_batch(
                ec, engine.transit_path_device(rad, 0), rad, model.rstar, 0, model.nlayers,
                model.maxdepth)
        else:
            spectra = engine.emission_flux_batch(
                ec, (rad[:, :-1] - rad[:, 1:]).contiguous(), model.wn, b['temps'], model.mu,
                model.weights, 0, model.nlayers, model.maxdepth)
        return pb.integrate_batch(spectra)
    for i in range(warmup):
        out = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step(i)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    res = {'evals_per_s': steps * BATCH / elapsed, 'ms_per_batch': 1e3 * elapsed / steps,
           'finite': bool(torch.isfinite(out).all()), 'bandflux0': out[0, :3].tolist()}
    del model, batches
    torch.cuda.empty_cache()
    return res


def profile(steps):
    """Mean time per launch of the interpolation kernels (kAlk: the last template argument) and
    of the split form's pb_alkali_cross_section kernel, from rocprofv3 kernel stats of a child
    running every leg."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out = tempfile.mkdtemp(prefix='pb_c5alk_prof_')
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
                if 'k_interp_ec_batch' in name or 'k_cont_' in name or 'k_alkali' in name:
                    key = name.replace('void ', '').replace('(anonymous namespace)::', '')
                    key = key.split('(')[0]
                    res[key] = {'calls': int(row['Calls']),
                                'mean_ms': float(row['AverageNs']) * 1e-6}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-prof', action='store_true')
    ap.add_argument('--inner', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:                     # (the profiled child)
        for rt in ('transit', 'emission'):
            for case in ('plain', 'fused', 'split'):
                run(rt, case, args.steps, args.warmup)
        return
    prof = None if args.no_prof else profile(min(args.steps, 5))
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-alkali', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'grid_cm-1': [WN_LO, WN_HI]}
    for rt in ('transit', 'emission'):
        legs = {case: run(rt, case, args.steps, args.warmup) for case in ('plain', 'fused', 'split')}
        legs['fused_over_split'] = legs['fused']['evals_per_s'] / legs['split']['evals_per_s']
        legs['fused_over_plain'] = legs['fused']['evals_per_s'] / legs['plain']['evals_per_s']
        res[rt] = legs
    if prof is not None:
        res['interp_kernels_rocprofv3'] = prof
    print(json.dumps(res))


if __name__ == '__main__':
    main()
