#!/usr/bin/env python3
"""Band contribution functions per walker (pyratbay_amd/csrc/pb_contribution.hip) at the C5 shape
(tools/bench_c5.py: 64 walkers x 80 layers x 1e5 samples, 24 bands), in transit and in emission
geometry.

Legs per geometry, ms per batch of 64 walkers:
  eval_bands               TableSpectrum.eval_bands without contribution_out (the calls of the
                           library are those of every earlier version: column_order='auto')
  eval_bands_contribution  the same call with contribution_out (grid order, every layer; transit:
                           a second transit pass that stores the depth)
  kernels                  the new entry alone on a prepared chunk: pb_band_transmittance_batch on
                           a stored depth / pb_band_contribution_emission_batch on ec
  depth_pass               transit only: pb_transit_spectrum_batch storing depth and ideep
  host_route               what a user had to do before: the depth (and B) of `--host-walkers`
                           walkers read back and contribution.band_contribution_host on each,
                           scaled to 64 walkers (stated in the output)
and each kernel's traffic floor at `--floor-gbps` (default 5000, what k_interp_ec_batch2 reaches):
transit: one write and one read of the stored depth, 2 x 8 nw L W bytes (the write belongs to
depth_pass, the read to the kernel); emission: two reads of ec down to the stop, the stop taken
from the host walkers' ideep.  Prints one JSON line.

    python tools/bench_contribution.py [--steps K] [--warmup W] [--geometries transit,emission]
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
from tools.bench_posterior import device_ms  # noqa: E402

BATCH = bench_c5.BATCH


def host_route(engine, model, rt_path, inp, ec, rad, temps, pressure, nhost):
    """Seconds for `nhost` walkers: depth (and B) on the device, read back, the NumPy forms."""
    import torch
    from pyratbay_amd import contribution as cb
    wn = inp['grid']['wn']
    responses = [np.asarray(b[1], float) for b in inp['bands']]
    indices = [np.arange(b[0], b[0] + len(b[1])) for b in inp['bands']]
    L = model.nlayers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, stops = [], []
    for w in range(nhost):
        if rt_path == 'transit':
            r = rad[w:w + 1].contiguous()
            _, depth, ideep = engine.transit_spectrum_batch(
                ec[w:w + 1], engine.transit_path_device(r, model.itop), r, model.rstar,
                model.itop, L, model.maxdepth, want_depth=True)
            out.append(cb.band_contribution_host(depth[0].cpu().numpy(), ideep[0].cpu().numpy(),
                                                 responses, wn, indices))
        else:
            intervals = (rad[w, :-1] - rad[w, 1:]).contiguous()
            depth, ideep = engine.plane_parallel_optical_depth(ec[w], intervals, model.itop, L,
                                                               model.maxdepth)
            planck = engine.blackbody_wn_2D(model.wn, temps[w])
            ideep = ideep.cpu().numpy()
            out.append(cb.band_contribution_host(depth.cpu().numpy(), ideep, responses, wn,
                                                 indices, rt_path='emission', pressure=pressure,
                                                 planck=planck.cpu().numpy()))
            stops.append(float(np.mean(ideep + 1.0)) / L)
    return time.perf_counter() - t0, np.array(out), stops


def run(rt_path, args):
    import torch
    from pyratbay_amd import engine
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    pressure = np.asarray(atm['press'], float)
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], g['wn'], atm['radius'],
                                 atm['rstar'], rt_path=rt_path)
    pb = engine.PassBands(g['wn'], inp['bands'])
    L, W = model.nlayers, model.nwave
    batches = []
    for b in range(2):
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 900 + b)
        batches.append((engine.dev(temps), engine.dev(dens), engine.dev(radius)))
    cf = torch.empty((BATCH, L, pb.nbands), dtype=torch.float64, device='cuda')
    count = [0]

    def step(contribution):
        temps, dens, radius = batches[count[0] % len(batches)]
        count[0] += 1
        kw = dict(contribution_out=cf, contribution_pressure=pressure) if contribution else {}
        return model.eval_bands(temps, dens, pb, radius=radius, chunk=bench_c5.CHUNK, **kw)
    res = {'eval_bands_ms': device_ms(lambda: step(False), args.steps, args.warmup),
           'ordered_columns': model.column_order is not None}
    res['eval_bands_contribution_ms'] = device_ms(lambda: step(True), args.steps, args.warmup)
    res['contribution_over_plain'] = res['eval_bands_contribution_ms'] / res['eval_bands_ms']
    res['finite'] = bool(torch.isfinite(cf).all())
    # the kernels alone, on the first batch's chunk
    temps, dens, rad = batches[0]
    ec = engine.interp_ec_batch(model.etable, model.ttable, temps, dens)
    nbytes = 8.0 * BATCH * L * W
    floor = lambda n: n / (args.floor_gbps * 1e9) * 1e3                       # noqa: E731
    if rt_path == 'transit':
        path = engine.transit_path_device(rad, model.itop)
        depth_pass = lambda: engine.transit_spectrum_batch(                   # noqa: E731
            ec, path, rad, model.rstar, model.itop, L, model.maxdepth, want_depth=True)
        _, depth, ideep = depth_pass()
        res['depth_pass_ms'] = device_ms(depth_pass, args.steps, args.warmup)
        res['kernels_ms'] = device_ms(
            lambda: engine.band_transmittance_batch(depth, ideep, pb, model.itop, out=cf),
            args.steps, args.warmup)
        # (only the bands' samples, and only the rows above ideep, are read)
        covered = float(sum(len(b[1]) for b in inp['bands'])) / W
        res['band_coverage'] = covered
        res['floor_ms'] = {'depth_write': floor(nbytes), 'depth_read': floor(nbytes * covered)}
        del depth
    else:
        intervals = (rad[:, :-1] - rad[:, 1:]).contiguous()
        res['kernels_ms'] = device_ms(
            lambda: engine.band_contribution_emission_batch(
                ec, intervals, temps, pb, pressure, model.itop, L, model.maxdepth, out=cf),
            args.steps, args.warmup)
    seconds, host, stops = host_route(engine, model, rt_path, inp, ec, rad, temps, pressure,
                                      args.host_walkers)
    got = cf[:args.host_walkers].cpu().numpy()
    res['host_walkers'] = args.host_walkers
    res['host_route_ms_scaled'] = 1e3 * seconds * BATCH / args.host_walkers
    res['host_route_over_contribution_call'] = res['host_route_ms_scaled'] / \
        res['eval_bands_contribution_ms']
    res['max_abs_difference_from_host'] = float(np.nanmax(np.abs(got - host)))
    if rt_path != 'transit':
        covered = float(sum(len(b[1]) for b in inp['bands'])) / W
        res['band_coverage'] = covered
        res['mean_stop_fraction'] = float(np.mean(stops))
        res['floor_ms'] = {'two_reads_of_ec_to_the_stop':
                           floor(2 * nbytes * covered * float(np.mean(stops)))}
    res['kernels_over_floor'] = res['kernels_ms'] / \
        (res['floor_ms']['depth_read'] if rt_path == 'transit'
         else res['floor_ms']['two_reads_of_ec_to_the_stop'])
    del model, batches, ec, cf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--geometries', default='transit,emission')
    ap.add_argument('--host-walkers', type=int, default=2)
    ap.add_argument('--floor-gbps', type=float, default=5000.0)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-contribution', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'chunk': bench_c5.CHUNK, 'floor_GBps': args.floor_gbps}
    for rt_path in (v for v in args.geometries.split(',') if v):
        res[rt_path] = run(rt_path, args)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
