#!/usr/bin/env python3
"""Band contribution functions per walker WITH clouds (pyratbay_amd/csrc/pb_contribution.hip:
k_band_transmittance_cloudy, k_band_cf_emission<true>) at the C5 shape (tools/bench_c5.py:
64 walkers x 80 layers x 1e5 samples, 24 bands), in transit and in emission geometry.  The cloudy
model: Rayleigh H2 + He in ec, a Deck, a Lecavelier haze and a CCSgray cloud as cloud-type models,
per walker a deck pressure between 1 mbar and 1 bar, a cloudy fraction and cloud parameters.

Legs per geometry, ms per batch of 64 walkers:
  cloudy_contribution   eval_bands(deck_logp, f_patchy, continuum_pars, contribution_out)
  cloudy_plain          the same call without contribution_out
  clear_contribution    the clear contribution call of the parent commit (Rayleigh only, no cloud
                        arguments, contribution_out), in the same session
  kernels               the new entry alone on a prepared chunk (deck state and cloud factors made
                        before): pb_band_transmittance_cloudy_batch / pb_band_contribution_
                        emission_cloudy_batch, finish kernel included
  stored_depth_pair     transit only: the parent's pair on the same chunk, pb_transit_spectrum_batch
                        storing depth and ideep + pb_band_transmittance_batch (one column; a cloudy
                        call by that route would need it twice, and a second ec)
  host_route            the depths of both columns (and B) of `--host-walkers` walkers formed on
                        the device, read back, contribution.band_contribution_cloudy_host on each;
                        scaled to 64 walkers
and the largest absolute difference between the new entry and the host route on those walkers.
Prints one JSON line.

    python tools/bench_contribution_clouds.py [--steps K] [--warmup W] [--geometries transit]
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


def cloud_columns(cops, keep, w):
    """ec_cloud[L, W] of walker w from the factors pb_cloud_plan made (f[nw, L, nr] and the
    Lecavelier rows[nlec, nw, W]): the models' terms added in their order."""
    f, rows = keep[0], keep[1]
    total, j = 0.0, 0
    for m, kind in enumerate(cops.kinds):
        if kind == 1:
            total = total + f[w, :, m, None] * rows[j, w][None, :]
            j += 1
        else:
            total = total + f[w, :, m, None].expand(-1, cops.wn.shape[0])
    return total


def host_route(engine, model, rt_path, inp, ec, rad, temps, pressure, deck, fp, cops, keep,
               nhost):
    """Seconds for `nhost` walkers: both depths (and B) on the device, read back, the NumPy
    form."""
    import torch
    from pyratbay_amd import contribution as cb
    wn = inp['grid']['wn']
    responses = [np.asarray(b[1], float) for b in inp['bands']]
    indices = [np.arange(b[0], b[0] + len(b[1])) for b in inp['bands']]
    L = model.nlayers
    ditop = deck[0].cpu().numpy()
    fh = np.clip(fp.cpu().numpy(), 0.0, 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = []
    for w in range(nhost):
        cloudy = ec[w] + cloud_columns(cops, keep, w)
        dk = int(ditop[w])
        if rt_path == 'transit':
            path = engine.transit_path_device(rad[w].contiguous(), model.itop).view(-1)
            dc, ic = engine.optical_depth_transit(cloudy, path, model.itop, dk + 1,
                                                  model.maxdepth)
            dl, il = engine.optical_depth_transit(ec[w], path, model.itop, L, model.maxdepth)
            dc = dc.cpu().numpy()
            dc[dk + 1:] = 0.0                         # (rows the cloudy column does not have)
            out.append(cb.band_contribution_cloudy_host(
                dc, ic.cpu().numpy(), responses, wn, indices, depth_clear=dl.cpu().numpy(),
                ideep_clear=il.cpu().numpy(), f_patchy=fh[w]))
        else:
            intervals = (rad[w, :-1] - rad[w, 1:]).contiguous()
            depth, ideep = engine.plane_parallel_optical_depth(cloudy, intervals, model.itop,
                                                               dk + 1, model.maxdepth)
            planck = engine.blackbody_wn_2D(model.wn, temps[w])
            planck[dk] = engine.blackbody_wn_2D(model.wn, deck[2][w:w + 1])[0]
            out.append(cb.band_contribution_cloudy_host(
                depth.cpu().numpy(), ideep.cpu().numpy(), responses, wn, indices,
                rt_path='emission', pressure=pressure, planck=planck.cpu().numpy()))
    return time.perf_counter() - t0, np.array(out)


def run(rt_path, args):
    import torch
    from pyratbay_amd import continuum as ct
    from pyratbay_amd import engine
    inp = bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    pressure = np.asarray(atm['press'], float)
    rayleigh = [ct.Kurucz(wn, 'H2'), ct.Kurucz(wn, 'He')]
    clouds = [ct.Lecavelier(pressure, wn=wn), ct.CCSgray(pressure, wn)]
    cont = ct.Continuum(wn, pressure, rayleigh + clouds + [ct.Deck(pressure, wn)],
                        cloud_models=clouds)
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'],
                                 rt_path=rt_path, continuum=cont)
    clear_model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'],
                                       atm['rstar'], rt_path=rt_path,
                                       continuum=ct.Continuum(wn, pressure, rayleigh))
    pb = engine.PassBands(wn, inp['bands'])
    L, W = model.nlayers, model.nwave
    batches = []
    for b in range(2):
        rng = np.random.default_rng(1300 + b)
        temps, dens, radius = bench_c5.walkers(inp, BATCH, 900 + b)
        ntot = pressure * 1e6 / temps / 1.380649e-16
        kw = dict(continuum_density=engine.dev(np.stack([ntot * 0.85, ntot * 0.149], axis=-1)))
        ckw = dict(deck_logp=engine.dev(rng.uniform(-3, 0, BATCH)),
                   f_patchy=engine.dev(rng.uniform(0, 1, BATCH)),
                   continuum_pars=engine.dev(np.stack(
                       [rng.uniform(0, 2, BATCH), rng.uniform(-6, -2, BATCH),
                        rng.uniform(0, 2, BATCH), rng.uniform(-4, -2, BATCH),
                        rng.uniform(-1, 1.5, BATCH)], axis=1)))
        batches.append((engine.dev(temps), engine.dev(dens), engine.dev(radius), kw, ckw))
    cf = torch.empty((BATCH, L, pb.nbands), dtype=torch.float64, device='cuda')
    count = [0]

    def step(which, cloudy, contribution):
        temps, dens, radius, kw, ckw = batches[count[0] % len(batches)]
        count[0] += 1
        kw = dict(kw, **ckw) if cloudy else kw
        if contribution:
            kw = dict(kw, contribution_out=cf)
            if rt_path != 'transit':
                kw['contribution_pressure'] = pressure
        return which.eval_bands(temps, dens, pb, radius=radius, chunk=bench_c5.CHUNK, **kw)
    res = {'cloudy_plain_ms': device_ms(lambda: step(model, True, False), args.steps,
                                        args.warmup)}
    res['cloudy_contribution_ms'] = device_ms(lambda: step(model, True, True), args.steps,
                                              args.warmup)
    res['finite'] = bool(torch.isfinite(cf).all())
    res['clear_contribution_ms'] = device_ms(lambda: step(clear_model, False, True), args.steps,
                                             args.warmup)
    res['contribution_over_plain'] = res['cloudy_contribution_ms'] / res['cloudy_plain_ms']
    res['cloudy_over_clear_contribution'] = res['cloudy_contribution_ms'] / \
        res['clear_contribution_ms']
    del clear_model
    # the kernels alone, on the first batch's chunk
    temps, dens, rad, _, ckw = batches[0]
    ec = engine.interp_ec_batch(model.etable, model.ttable, temps, dens)
    deck = engine.deck_state_batch(cont.pressure_d, ckw['deck_logp'], rad, temps)
    cops = cont.cloud_operands(None)
    terms, keep = cops.plan(temps.contiguous(), ckw['continuum_pars'])
    if rt_path == 'transit':
        path = engine.transit_path_device(rad, model.itop)
        new = lambda: engine.band_transmittance_cloudy_batch(                 # noqa: E731
            ec, path, pb, model.itop, model.maxdepth, deck=deck, f_patchy=ckw['f_patchy'],
            out=cf, _terms=terms)
        depth_pass = lambda: engine.transit_spectrum_batch(                   # noqa: E731
            ec, path, rad, model.rstar, model.itop, L, model.maxdepth, want_depth=True)
        _, depth, ideep = depth_pass()
        res['stored_depth_pair_ms'] = {
            'depth_pass': device_ms(depth_pass, args.steps, args.warmup),
            'band_transmittance': device_ms(
                lambda: engine.band_transmittance_batch(depth, ideep, pb, model.itop, out=cf),
                args.steps, args.warmup)}
        res['stored_depth_pair_ms']['sum'] = sum(res['stored_depth_pair_ms'].values())
        del depth, ideep
    else:
        intervals = (rad[:, :-1] - rad[:, 1:]).contiguous()
        new = lambda: engine.band_contribution_emission_cloudy_batch(         # noqa: E731
            ec, intervals, temps, pb, pressure, model.itop, L, model.maxdepth, deck=deck, out=cf,
            _terms=terms)
    res['kernels_ms'] = device_ms(new, args.steps, args.warmup)
    new()
    got = cf[:args.host_walkers].cpu().numpy()
    seconds, host = host_route(engine, model, rt_path, inp, ec, rad, temps, pressure, deck,
                               ckw['f_patchy'], cops, keep, args.host_walkers)
    res['host_walkers'] = args.host_walkers
    res['host_route_ms_scaled'] = 1e3 * seconds * BATCH / args.host_walkers
    res['host_route_over_contribution_call'] = res['host_route_ms_scaled'] / \
        res['cloudy_contribution_ms']
    res['max_abs_difference_from_host'] = float(np.nanmax(np.abs(got - host)))
    res['band_coverage'] = float(sum(len(b[1]) for b in inp['bands'])) / W
    del model, batches, ec, cf, keep
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--geometries', default='transit,emission')
    ap.add_argument('--host-walkers', type=int, default=2)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {'workload': 'c5-contribution-clouds', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'chunk': bench_c5.CHUNK}
    for rt_path in (v for v in args.geometries.split(',') if v):
        res[rt_path] = run(rt_path, args)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
