#!/usr/bin/env python3
"""The radiative-equilibrium iteration (pyratbay_amd/radeq.py, csrc/pb_radeq.hip) at the table
shape of `bench.py --workload c5` (80 layers x 100001 samples, 4 table species), for 1 and 64
profiles, hydro_m radius, tint = 300 K and an irradiation row.

Legs, each in ms per iteration (the whole batch of nw profiles):
  loop         RadiativeEquilibrium.run: interpolation, pb_two_stream_net_batch, pb_radeq_update
  interp / net / update   each of its three launches alone, on the state the loop left
  two_stream   pb_two_stream_batch alone at the same shape (what the net-flux kernel adds to)
  conv_loop / conv_update   (--convection) the loop with run(convection=True) and its third
               launch, pb_radeq_update_convective, alone, with a cp / R table of 12 temperatures and
               a start that is superadiabatic in the bottom third (conv_profiles_convecting:
               the profiles whose last iteration ran the second half)
  host_route   (nw = 1) what a checkout without this loop can do: TableSpectrum.eval() in
               two-stream geometry (three launches, two [L, W] arrays), torch.trapezoid of both,
               the read-back, radeq.step_host in NumPy, the new densities and radius on the host
Prints one JSON line.  Kernel times are device-side (events around `--steps` back-to-back
launches); loop and host_route are wall clock with a synchronisation at both ends.

    python tools/bench_radeq.py [--steps K] [--warmup W] [--profiles 1,64] [--convection]
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

TINT = 300.0
MJUP, RJUP = 1.8982e30, 7.1492e9


def device_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def wall_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def run(inp, nw, steps, warmup, convection=False):
    import torch
    from pyratbay_amd import engine, radeq
    g, atm = inp['grid'], inp['atm']
    wn = g['wn']
    L, W = atm['nlayers'], len(wn)
    flux_top = 0.25 * (atm['rstar'] / 7.5e11)**2 * 2.0e6 * (1.0 + 0.1 * np.sin(wn / 70.0))
    model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'],
                                 rt_path='two_stream', tint=TINT, flux_top=flux_top,
                                 timestamps=False)
    kw = dict(radius_model='hydro_m', mplanet=0.6 * MJUP, p0=0.1, r0=1.0 * RJUP, tint=TINT,
              flux_top=flux_top, species=atm['species'], table_species=atm['species'][2:6])
    if convection:
        cp_temps = np.array([100.0, 200.0, 300.0, 450.0, 600.0, 800.0, 1000.0, 1300.0, 1700.0,
                             2200.0, 3000.0, 4000.0])
        rise = cp_temps / (cp_temps + 1500.0)
        kw['heat_capacity'] = (cp_temps, 3.5 + np.outer(rise, np.linspace(0.5, 2.5,
                                                                        len(atm['species']))))
    re = model.radiative_equilibrium(atm['press'], atm['vmr'], atm['mol_mass'], **kw)
    rng = np.random.default_rng(5)
    temp0 = atm['temp'][None, :] * (1.0 + 0.05 * rng.uniform(-1, 1, (nw, 1)))
    res = {'profiles': nw}
    res['loop_ms'] = wall_ms(lambda: re.run(temp0, 32), max(steps // 8, 1), 1) / 32
    d = re._state
    res['interp_ms'] = device_ms(lambda: engine.interp_ec_batch(
        model.etable, model.ttable, d['temp'], d['dens'], out=d['ec'], work=d['iwork']),
        steps, warmup)
    ec0 = d['ec'].clone()

    def net():
        radeq.two_stream_net_batch(d['ec'], d['intervals'], model.wn, d['tw'], d['temp'],
                                   d['f_int'], d['flux_top'], out=d['flux'], parts=d['parts'],
                                   work=d['work'])

    def plain():
        engine.two_stream_batch(d['ec'], d['intervals'], model.wn, d['temp'], d['f_int'],
                                d['flux_top'], out=d['flux'], work=d['work'])
    # (both kernels consume ec: every launch gets a fresh copy, whose time is measured and taken off)
    copy = device_ms(lambda: d['ec'].copy_(ec0), steps, warmup)
    res['net_ms'] = device_ms(lambda: (d['ec'].copy_(ec0), net()), steps, warmup) - copy
    res['two_stream_ms'] = device_ms(lambda: (d['ec'].copy_(ec0), plain()), steps, warmup) - copy
    res['net_over_two_stream'] = res['net_ms'] / res['two_stream_ms']
    import ctypes as C
    from pyratbay_amd import _capi
    st = d['struct']

    def update():
        d['iter'].zero_()
        _capi.call('pb_radeq_update', C.byref(st), 0, engine._stream())
    res['update_ms'] = device_ms(update, steps, warmup)
    res['finite'] = bool(torch.isfinite(re.temps).all())
    if convection:
        # T ~ p**0.35 below the top two thirds of the layers, kept within the table's range
        knee = atm['press'][2 * L // 3]
        start = np.clip(temp0 * np.maximum(atm['press'] / knee, 1.0)**0.35, 1.02 * re.tmin,
                        0.98 * re.tmax)
        res['conv_loop_ms'] = wall_ms(lambda: re.run(start, 32, convection=True),
                                      max(steps // 8, 1), 1) / 32
        res['conv_profiles_convecting'] = int(re.convective.sum())
        res['conv_loop_minus_loop_ms'] = res['conv_loop_ms'] - res['loop_ms']
        cv = d['convection']

        def conv_update():
            d['iter'].zero_()
            _capi.call('pb_radeq_update_convective', C.byref(st), C.byref(cv), engine._stream())
        res['conv_update_ms'] = device_ms(conv_update, steps, warmup)
        res['finite'] = res['finite'] and bool(torch.isfinite(re.temps).all())
    if nw == 1:
        itab = [atm['species'].index(s) for s in atm['species'][2:6]]
        dpress = radeq.log_pressure_steps(atm['press'])
        state = dict(temp=temp0[0].copy(), dts=np.full(L, radeq.DT_SCALE0), signs=np.zeros((0, L)))

        def host_step():
            dens, radius = radeq.atmosphere_host(state['temp'], atm['press'], atm['vmr'],
                                                 atm['mol_mass'], 'hydro_m', mplanet=0.6 * MJUP,
                                                 p0=0.1, r0=1.0 * RJUP)
            model.set_radius(radius)
            model.eval(state['temp'], np.ascontiguousarray(dens[:, itab]))
            qup = torch.trapezoid(model.flux_up, model.wn, dim=1).cpu().numpy()
            qdown = torch.trapezoid(model.flux_down, model.wn, dim=1).cpu().numpy()
            s = radeq.step_host(state['temp'], state['dts'], state['signs'], qup, qdown, dpress,
                                re.tmin, re.tmax)
            state['temp'], state['dts'] = s['temp'], s['dt_scale']
            state['signs'] = np.vstack([state['signs'], s['sign']])[-4:]
        res['host_route_ms'] = wall_ms(host_step, steps, warmup)
        res['host_route_over_loop'] = res['host_route_ms'] / res['loop_ms']
    del model, re, d
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profiles', default='1,64')
    ap.add_argument('--convection', action='store_true',
                    help='also time the loop and its update with convection=True')
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    inp = bench_c5.inputs()
    res = {'workload': 'c5-radeq', 'steps': args.steps,
           'shape': [bench_c5.NLAYERS, bench_c5.NWAVE, bench_c5.NSPEC]}
    for nw in (int(v) for v in args.profiles.split(',')):
        res[f'nw{nw}'] = run(inp, nw, args.steps, args.warmup, args.convection)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
