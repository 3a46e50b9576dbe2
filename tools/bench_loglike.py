#!/usr/bin/env python3
"""The C5 retrieval batch in emission geometry (tools/bench_c5.py: 64 walkers x 80 layers x 1e5
samples, 4 table species) from the walkers' PARAMETER vectors to their LOG-LIKELIHOODS: the
atmosphere of tools/bench_c5_atmosphere.py (10 parameters, rplanet free), an eclipse with a free
stellar temperature on a 12-node SED grid, 24 bands over three instruments with 3 offset models
and 2 error models (one scale, one quadrature, ppm), seed 7.

Three legs, each the median of `--blocks` timed blocks of `--steps` batches after a warm-up
(min ... max beside it; wall clock around a device synchronise), alternating block by block in
one process on the same walkers:
  a  eval_params alone (frozen eclipse factor: what the loop gave before)
  b  eval_loglike: eval_params with tstar[nw] + the free rplanet, then pb_loglike_obs
  c  the host route: eval_params WITHOUT the eclipse factor, read-back of bandflux[nw, nbands],
     per walker flux_host + star_bandflux + the factor, offset_data_host / scale_errors_host and
     the NumPy likelihood
and the two new kernels alone, timed with device events on the launch stream:
pb_star_band_scale_batch and pb_loglike_obs at the batch's shape.  Prints one JSON line.
Measured: profiles/observation.md.

    python tools/bench_loglike.py [--steps K] [--blocks B] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import bench_c5, bench_c5_atmosphere  # noqa: E402

BATCH = bench_c5.BATCH
NT = 12
INSTRUMENTS = ('nrs1', 'nrs2', 'miri')
OFFSETS = ['offset_nrs1', 'offset_nrs2', 'offset_miri']
ERRORS = ['err_scale_nrs1', 'err_quad_miri']


def stellar_grid(wn):
    sed_temps = np.linspace(4000.0, 6750.0, NT)
    x = np.linspace(0.0, 1.0, len(wn))
    fluxes = 2.0e5 * (sed_temps[:, None] / 5000.0)**3 * (1 + 0.2 * np.sin(7 * x)[None, :])
    return sed_temps, fluxes


def block(fn, steps, sync):
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    sync()
    return 1e3 * (time.perf_counter() - t0) / steps


def summary(v):
    return {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v)}


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
    wn, bands = g['wn'], inp['bands']
    nb = len(bands)
    watm = bench_c5_atmosphere.atmosphere(inp)
    col = watm.par_scalar['rplanet']
    rstar = float(atm['rstar'])
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, watm.base_radius, rstar,
                                 rt_path='emission')
    sed_temps, fluxes = stellar_grid(wn)
    grid = engine.StellarGrid(wn, sed_temps, fluxes)
    pb_grid = engine.PassBands(wn, bands).set_eclipse_grid(rstar, grid)
    pb_plain = engine.PassBands(wn, bands)
    pb_frozen = engine.PassBands(wn, bands)
    base = np.array(bench_c5_atmosphere.BASE)
    pb_frozen.set_eclipse(base[col], rstar, pb_frozen.star_bandflux(grid.flux_host(5000.0)))
    rng = np.random.default_rng(7)
    params_h = [base * (1.0 + 0.1 * rng.uniform(-1, 1, (BATCH, len(base)))) for _ in range(4)]
    tstar_h = [rng.uniform(sed_temps[0], sed_temps[-1], BATCH) for _ in range(4)]
    params = [engine.dev(p) for p in params_h]
    tstar = [engine.dev(t) for t in tstar_h]
    # data near the first walker's model; offsets and quadrature terms of a few per cent of it
    first = model.eval_params(watm, params[0], pb_grid, tstar=tstar[0], chunk=bench_c5.CHUNK)
    first = first.cpu().numpy()
    ok = np.isfinite(first).all(axis=1)
    level = first[ok][0]
    names = [INSTRUMENTS[(3 * b) // nb] for b in range(nb)]
    obs = engine.Observation(level * (1 + rng.normal(0, 0.02, nb)), 0.03 * level, names, OFFSETS,
                             ERRORS, units='ppm')
    scale = float(np.max(level)) * 1e6
    offsets_h = [rng.uniform(-0.01, 0.01, (BATCH, len(OFFSETS))) * scale for _ in range(4)]
    err_h = [np.stack([rng.uniform(-0.3, 0.5, BATCH),
                       np.log10(scale * rng.uniform(0.01, 0.05, BATCH))], axis=1)
             for _ in range(4)]
    offsets = [engine.dev(o) for o in offsets_h]
    err_pars = [engine.dev(e) for e in err_h]

    def sync():
        torch.cuda.synchronize()

    def leg_a(i):
        return model.eval_params(watm, params[i % 4], pb_frozen, chunk=bench_c5.CHUNK)

    def leg_b(i):
        k = i % 4
        return model.eval_loglike(watm, params[k], pb_grid, obs, offsets=offsets[k],
                                  err_pars=err_pars[k], tstar=tstar[k], chunk=bench_c5.CHUNK)

    def leg_c(i):
        k = i % 4
        flux = model.eval_params(watm, params[k], pb_plain, chunk=bench_c5.CHUNK).cpu().numpy()
        out = np.empty(BATCH)
        for w in range(BATCH):
            star = pb_plain.star_bandflux(grid.flux_host(tstar_h[k][w]))
            rprs = params_h[k][w, col] / rstar
            out[w] = obs.loglike_host(flux[w] * (rprs**2.0 / star), offsets_h[k][w], err_h[k][w])
        return out

    for i in range(args.warmup):
        leg_a(i), leg_b(i)
    host0 = leg_c(0)
    sync()
    dev0 = leg_b(0).cpu().numpy()
    live = dev0 > -1e90
    res = {'workload': 'c5-emission-loglike', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'blocks': args.blocks, 'npar': len(base), 'nbands': nb, 'sed_nodes': NT,
           'offset_models': len(OFFSETS), 'err_models': len(ERRORS),
           'rejected_walkers': int((~live).sum()),
           'loglike_max_rel_vs_host_route':
               float(np.max(np.abs(dev0[live] / host0[live] - 1))) if live.any() else None}
    la, lb, lc = [], [], []
    host_steps = max(2, args.steps // 10)
    for _ in range(args.blocks):
        la.append(block(leg_a, args.steps, sync))
        lb.append(block(leg_b, args.steps, sync))
        lc.append(block(leg_c, host_steps, sync))
    res['a_eval_params'] = summary(la)
    res['b_eval_loglike'] = summary(lb)
    res['c_host_route'] = summary(lc)
    res['b_minus_a_ms'] = res['b_eval_loglike']['median_ms'] - res['a_eval_params']['median_ms']
    res['a_spread_ms'] = res['a_eval_params']['max_ms'] - res['a_eval_params']['min_ms']
    res['c_over_b'] = res['c_host_route']['median_ms'] / res['b_eval_loglike']['median_ms']

    # the two new kernels alone: device events around `reps` launches on the launch stream
    flux = torch.as_tensor(first, device='cuda').contiguous()
    rplanet = params[0][:, col].contiguous()
    spectra = torch.ones((BATCH, len(wn)), dtype=torch.float64, device='cuda')
    out = torch.empty((BATCH, nb), dtype=torch.float64, device='cuda')

    def timed(fn, reps=200):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(10):
            fn()
        ev0.record()
        for _ in range(reps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / reps

    both = timed(lambda: pb_grid.integrate_batch(spectra, out, tstar=tstar[0], rplanet=rplanet))
    integ = timed(lambda: pb_plain.integrate_batch(spectra, out))
    res['kernels_ms'] = {
        'pb_band_integrate_batch': integ,
        'pb_star_band_scale_batch': both - integ,
        'pb_loglike_obs': timed(lambda: obs.loglike(flux, offsets[0], err_pars[0])),
        'note': 'back-to-back launches between two events, host submission included; the star '
                'kernel as the difference of the band exit with and without it'}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
