#!/usr/bin/env python3
"""The C5 retrieval batch (tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 4 species) in
two-stream geometry: TableSpectrum(rt_path='two_stream', tint=300, flux_top=...).eval_bands
(pb_two_stream_batch, pb_two_stream.hip).

Legs:
  emission         the five-angle quadrature batch (rt_path='emission'), for scale
  two_stream       the two-stream batch: interpolation, ONE launch for depth + both sweeps, bands
  two_stream_loop  the route without the batch kernel: interp_ec_batch for the chunk, then per
                   walker plane_parallel_optical_depth(inf) + two_stream (three launches and
                   [L, W] intermediates each), then the bands
Prints one JSON line: evals/s and ms per 64 walkers of every leg, and the ratios.
`--legs emission,two_stream_loop` runs on a checkout without the batch kernel too.

    python tools/bench_c5_two_stream.py [--steps K] [--warmup W] [--legs emission,...]
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
LEGS = ('emission', 'two_stream', 'two_stream_loop')
TINT = 300.0

_INPUTS = []


def loop_eval(engine, model, f_int, flux_top, temps, dens, radius, pb):
    """eval_bands of the two-stream geometry from the single-spectrum entry points."""
    import torch
    nw = temps.shape[0]
    L = model.nlayers
    out = torch.empty((nw, pb.nbands), dtype=torch.float64, device='cuda')
    for w0 in range(0, nw, bench_c5.CHUNK):
        w1 = min(w0 + bench_c5.CHUNK, nw)
        ec = engine.interp_ec_batch(model.etable, model.ttable, temps[w0:w1], dens[w0:w1])
        rad = radius[w0:w1]
        intervals = (rad[:, :-1] - rad[:, 1:]).contiguous()
        spectra = torch.empty((w1 - w0, model.nwave), dtype=torch.float64, device='cuda')
        for w in range(w1 - w0):
            depth, _ = engine.plane_parallel_optical_depth(ec[w], intervals[w], 0, L, np.inf)
            _, up = engine.two_stream(depth, model.wn, temps[w0 + w], f_int, flux_top, 0)
            spectra[w] = up[0]
        pb.integrate_batch(spectra, out[w0:w1])
    return out


def run(leg, steps, warmup):
    import torch
    from pyratbay_amd import engine
    if not _INPUTS:
        _INPUTS.append(bench_c5.inputs())
    inp = _INPUTS[0]
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    # the irradiation row beta_irr * (rstar / smaxis)**2 * starflux of a hot Jupiter
    flux_top = 0.25 * (atm['rstar'] / 7.5e11)**2 * 2.0e6 * (1.0 + 0.1 * np.sin(wn / 70.0))
    if leg == 'two_stream':
        model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'],
                                     atm['rstar'], rt_path='two_stream', tint=TINT,
                                     flux_top=flux_top)
    else:
        # (the loop leg takes only the table, the grid and the shape from the model)
        model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'],
                                     atm['rstar'], rt_path='emission',
                                     column_order='auto' if leg == 'emission' else None)
    pb = engine.PassBands(wn, inp['bands'])
    f_int = engine.internal_flux(model.wn, TINT)
    top_d = engine.dev(flux_top)
    batches = []
    for b in range(4):
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 700 + b)
        batches.append((engine.dev(temps), engine.dev(dens), engine.dev(radius)))

    def step(i):
        temps, dens, radius = batches[i % len(batches)]
        if leg == 'two_stream_loop':
            return loop_eval(engine, model, f_int, top_d, temps, dens, radius, pb)
        return model.eval_bands(temps, dens, pb, radius=radius, chunk=bench_c5.CHUNK)
    for i in range(warmup):
        out = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step(i)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    res = {'evals_per_s': steps * BATCH / elapsed, 'ms_per_batch': 1e3 * elapsed / steps,
           'finite': bool(torch.isfinite(out).all()),
           'ordered_columns': model.column_order is not None,
           'bandflux_first': [float(v) for v in out[0, :2].cpu()]}
    del model, batches
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--legs', default=','.join(LEGS))
    args = ap.parse_args()
    legs = [leg for leg in args.legs.split(',') if leg]
    assert all(leg in LEGS for leg in legs), f'legs: {LEGS}'
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-two-stream', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'chunk': bench_c5.CHUNK}
    for leg in legs:
        res[leg] = run(leg, args.steps, args.warmup)
    if 'two_stream' in legs:
        for other in ('two_stream_loop', 'emission'):
            if other in legs:
                res[f'two_stream_time_over_{other}'] = \
                    res['two_stream']['ms_per_batch'] / res[other]['ms_per_batch']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
