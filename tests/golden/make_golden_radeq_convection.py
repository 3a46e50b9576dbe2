#!/usr/bin/env python3
"""Fixture G26: radiative-equilibrium trajectories of the reference's own loop WITH convection.
Build container only (CPU):

    python tests/golden/make_golden_radeq_convection.py

Like make_golden_radeq.py (fixture G23) the real package is imported as in make_golden_e2e.py and
its pyratbay.spectrum.radiative_equilibrium (spectrum/radiative_transfer.py:141-272) is called
UNMODIFIED, here with convection=True, with
  * a stand-in chem_model: thermochemical_equilibrium(temp) returns the case's fixed VMR,
    heat_capacity(temp) is np.interp per species on the case's table of cp / R;
  * the two_stream_rt callback of G23 (the host chain of tests/radeq_cases.py), which also leaves
    radius, d (the number densities of ALL species) and mm of the profile it evaluated in `atm`;
  * an `atm` that carries _dt_scale, mplanet and mol_mass.
The function returns only the temperatures.  The other rows are read while it runs: Qup, Qdown in
the callback; conv_flux through a wrapper around convection.convective_flux that records what it
returns; the loop's own dt_scale from the caller's frame at the next callback (atm._dt_scale is
stale after the first convective iteration: the documented deviation of pyratbay_amd/radeq.py), for
which the function runs one iteration more than is recorded.

Recorded per case and profile, 8 iterations each: the inputs (radeq_cases' keys, cp_temps[nT],
cp_table[nw, nT, S]) and per iteration temp, dt_scale, Qup, Qdown, conv_flux and convective
(whether the second half ran: conv_flux not all zero).

Cases: (a) L = 2, W = 70, layer 1 superadiabatic at the start -- and yet no iteration convects:
the flux is evaluated at the temperatures the radiative half produced, whose top is isothermal,
which for two layers is the whole profile (a flux taken at the profile of the evaluation would
convect here); (b) L = 9, W = 130, the starting
profile steep (d ln T / d ln p = 0.4) in the bottom third; (c) L = 70, W = 300, hydro_m, the same
kind of start; (d) L = 9, three profiles: cp / R = 1.05 for every species (grad_ad = 0.95: it never
convects), cp / R = 8 (grad_ad = 0.125: it convects in every iteration) and the gas table (the
first iterations convect, the last do not).  Both outcomes of the all-zero test therefore occur
within ONE trajectory -- (b), and (d) profile 2 -- and across the batch of (d).

Trajectory sensitivity `{case}_sens`, G23's way: a second run with every row of flux_up, flux_down
AND conv_flux multiplied by 1 + 1e-12 r, r uniform in [-1, 1] (seeded); stored is the largest
relative temperature deviation over the 8 iterations.  A case above 1e-8 is ill-conditioned and
refused, as is one that misses a precondition of test_radeq_convection_cpu.py: at every iteration
and layer >= 1, |dF| >= 1e-9 max(Qup, Qdown) for the radiative dF and for the one with the
convective flux; no temperature on a clip bound; |grad_t - grad_ad| >= 1e-6 (no layer on the
switch); a finite positive radius; and in every convecting trajectory an iteration with at least two
convecting layers.  Only data is stored.

The pressure ranges are narrower than G23's: a gradient of 0.4 over more than 1.5 decades leaves
the tables' temperature range."""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden_e2e as e2e                      # noqa: E402
import make_golden_radeq as g23                    # noqa: E402
import radeq_cases as rc                           # noqa: E402
import radeq_convection_cases as cc                # noqa: E402
from pyratbay_amd import radeq                     # noqa: E402

NITER = cc.NITER
FLOOR = 1e-9
SWITCH = 1e-6


def steep(pressure, t_top, knee, slope):
    """t_top above pressure[knee], T ~ p**slope below it."""
    return t_top * np.maximum(pressure / pressure[knee], 1.0)**slope


def inputs(orc):
    from pyratbay_amd import atmosphere as pa
    store = {}

    def add(name, seed, pressure, wn, temp0, tint, flux_top, radius_model, tables, p0):
        rng = np.random.default_rng(seed)
        L, W = len(pressure), len(wn)
        ttable, a, b = g23.make_table(rng, L, W, wn)
        vmr = g23.base_vmr(L)
        mu = pa.mean_weight(vmr, mass=np.array(rc.MASS))
        gravity, mplanet, r0 = 2200.0, 0.6 * g23.MJUP, 1.0 * g23.RJUP
        radius = pa.hydro_g(pressure, np.atleast_2d(temp0)[0], mu, gravity, p0, r0)
        store[f'{name}_pressure'], store[f'{name}_wn'] = pressure, wn
        store[f'{name}_ttable'], store[f'{name}_tab_a'], store[f'{name}_tab_b'] = ttable, a, b
        store[f'{name}_vmr'] = vmr
        store[f'{name}_temp0'] = np.atleast_2d(temp0)
        store[f'{name}_tint'] = np.atleast_1d(np.asarray(tint, float))
        store[f'{name}_flux_top'] = np.atleast_2d(flux_top)
        store[f'{name}_radius'] = radius
        store[f'{name}_scalars'] = rc.pack_scalars(radius_model, gravity, mplanet, p0, r0, 200.0,
                                                   3800.0, False)
        store[f'{name}_cp_temps'] = cc.CP_TEMPS
        store[f'{name}_cp_table'] = np.array([cc.cp_table(t) for t in tables])

    wn_a = np.linspace(300.0, 9000.0, 70)
    add('a', 21, np.array([1.0, 100.0]), wn_a, np.array([700.0, 2600.0]), 100.0,
        g23.stellar(orc, wn_a, 5500.0, 1300.0), None, ['gas'], 10.0)
    wn_b = 250.0 * (12000.0 / 250.0)**np.linspace(0.0, 1.0, 130)
    p_b = np.logspace(-2.5, 1.5, 9)
    add('b', 22, p_b, wn_b, steep(p_b, 800.0, 5, 0.4), 150.0,
        g23.stellar(orc, wn_b, 5500.0, 1300.0), None, ['gas'], 0.1)
    idx = np.arange(0, 600, 2)
    wn_c = rc.g7()['wn'][idx]
    p_c = np.logspace(-3.0, 1.0, 70)
    add('c', 23, p_c, wn_c, steep(p_c, 900.0, 46, 0.4), 100.0,
        g23.stellar(orc, wn_c, 5500.0, 1400.0), 'hydro_m', ['gas'], 0.1)
    add('d', 22, p_b, wn_b,
        np.array([steep(p_b, 800.0, 5, 0.4), steep(p_b, 800.0, 5, 0.4),
                  steep(p_b, 820.0, 5, 0.4)]),
        [150.0, 60.0, 400.0],
        np.array([g23.stellar(orc, wn_b, 5500.0, 1300.0), g23.stellar(orc, wn_b, 4000.0, 900.0),
                  g23.stellar(orc, wn_b, 6500.0, 1500.0)]), None, ['stiff', 8.0, 'gas'], 0.1)
    return store


def reference_run(rt, orc, c, w, nsamples, temps0, dt_scale, noise=None):
    """The reference's loop with convection on profile w of case c, nsamples + 1 iterations of
    which nsamples are returned: -> dict of temps[1 + nsamples, L] and, per iteration, dt_scale,
    qup, qdown, conv_flux [nsamples, L], radius [nsamples, L].  noise[nsamples + 1, 3, L]: factors
    on the rows of flux_up / flux_down and on conv_flux."""
    vmr = c['vmr'][w] if c['vmr'].ndim == 3 else c['vmr']
    table = c['cp_table'][w]
    spec = types.SimpleNamespace()
    atm = types.SimpleNamespace(_dt_scale=dt_scale, mplanet=c['mplanet'], mol_mass=c['mol_mass'])
    rows = dict(dt_scale=[], qup=[], qdown=[], conv_flux=[], radius=[])
    chem = types.SimpleNamespace(
        thermochemical_equilibrium=lambda temp: vmr,
        heat_capacity=lambda temp: np.array([np.interp(temp, c['cp_temps'], table[:, s])
                                             for s in range(table.shape[1])]).T)
    count = [0]

    def two_stream_rt(temp, vmr):
        if count[0] > 0:
            rows['dt_scale'].append(sys._getframe(1).f_locals['dt_scale'].copy())
        temp = np.ascontiguousarray(temp)
        atm.d, atm.radius = rc.host_atmosphere(c, temp, w)
        atm.mm = np.sum(vmr * c['mol_mass'], axis=1)
        down, up = rc.host_fluxes(orc, c, temp, w)
        if noise is not None:
            up = up * noise[count[0], 0][:, None]
            down = down * noise[count[0], 1][:, None]
        spec.flux_up, spec.flux_down = up, down
        rows['qup'].append(np.trapezoid(up, c['wn'], axis=1))
        rows['qdown'].append(np.trapezoid(down, c['wn'], axis=1))
        rows['radius'].append(atm.radius.copy())
        count[0] += 1

    original = rt.ps

    def convective_flux(*args, **kw):
        flux = original.convective_flux(*args, **kw)
        if noise is not None:
            flux = flux * noise[count[0] - 1, 2]
        rows['conv_flux'].append(np.array(flux))
        return flux
    rt.ps = types.SimpleNamespace(convective_flux=convective_flux)
    try:
        temps = rt.radiative_equilibrium(c['pressure'] * 1e6, temps0, nsamples + 1, chem,
                                         two_stream_rt, c['wn'], spec, atm, convection=True,
                                         tmin=c['tmin'], tmax=c['tmax'])
    finally:
        rt.ps = original
    out = {k: np.array(v[:nsamples]) for k, v in rows.items()}
    out['temps'] = temps[:len(temps0) + nsamples]
    return out


def check_preconditions(name, c, w, run):
    """sys.exit on a missed precondition; returns what the docstring's claims rest on."""
    temps, qup, qdown, conv = run['temps'], run['qup'], run['qdown'], run['conv_flux']
    convective = np.array([not np.all(f == 0.0) for f in conv])
    qmax = np.maximum(qup, qdown)[:, 1:]
    floor = np.min(np.abs(np.diff(qup - qdown, axis=1)) / qmax)
    used = np.abs(np.diff(qup - qdown + conv, axis=1)) / qmax
    if convective.any():
        floor = min(floor, np.min(used[convective]))
    if not floor >= FLOOR:
        sys.exit(f'case {name} profile {w}: |dF| / max(Qup, Qdown) = {floor:.2e} < {FLOOR}')
    if np.any(temps <= c['tmin']) or np.any(temps >= c['tmax']):
        sys.exit(f'case {name} profile {w}: a temperature on a clip bound')
    if not (np.all(np.isfinite(run['radius'])) and np.all(run['radius'] > 0)):
        sys.exit(f'case {name} profile {w}: a radius that is not finite and positive')
    steps = cc.replay(c, w, fx={f'{name}_{k}': {w: v} for k, v in run.items()})
    margin, layers = np.inf, []
    for k, s in enumerate(steps):
        grad_t, grad_ad = cc.gradients(c, w, s['radiative']['temp'])
        margin = min(margin, np.min(np.abs(grad_t - grad_ad)[1:]))
        layers.append(int(np.sum(s['conv_flux'] != 0.0)))
        if s['convective'] != convective[k] or (np.sum(conv[k] != 0.0) != layers[-1]):
            sys.exit(f'case {name} profile {w} iteration {k}: the host statement convects in '
                     'other layers than the reference')
    if not margin >= SWITCH:
        sys.exit(f'case {name} profile {w}: |grad_t - grad_ad| = {margin:.2e} < {SWITCH}')
    return floor, margin, layers, convective


def main():
    if not os.path.isdir(e2e.REF):
        sys.exit(f'needs the reference checkout at {e2e.REF}')
    from oracle import oracle as orc
    orc.lib()
    work = tempfile.mkdtemp(prefix='pb_radeq_conv_')
    try:
        e2e.reference_package(work)
        from pyratbay.spectrum import radiative_transfer as rt
        store = inputs(orc)
        outcomes = set()
        for name in cc.CASES:
            c = cc.unpack(store, name)
            out = dict(temps=[], dt_scale=[], qup=[], qdown=[], conv_flux=[], convective=[])
            sens = 0.0
            for w in range(c['nw']):
                t0 = np.atleast_2d(c['temp0'][w])
                run = reference_run(rt, orc, c, w, NITER, t0, np.full(c['L'], radeq.DT_SCALE0))
                floor, margin, layers, convective = check_preconditions(name, c, w, run)
                rng = np.random.default_rng(2000 + 10 * ord(name) + w)
                noise = 1.0 + 1e-12 * rng.uniform(-1, 1, (NITER + 1, 3, c['L']))
                noisy = reference_run(rt, orc, c, w, NITER, t0,
                                      np.full(c['L'], radeq.DT_SCALE0), noise)['temps']
                s = float(np.max(np.abs(noisy - run['temps']) / run['temps']))
                sens = max(sens, s)
                print(f'case {name} profile {w}: T {run["temps"].min():.1f}-'
                      f'{run["temps"].max():.1f} K, floor {floor:.2e}, switch margin {margin:.2e}, '
                      f'convecting layers {layers}, sensitivity {s:.2e}')
                never = name == 'a' or (name == 'd' and w == 0)
                if never and convective.any():
                    sys.exit(f'case {name} profile {w} convects')
                if name == 'a':
                    grad_t, grad_ad = cc.gradients(c, w, c['temp0'][w])
                    if not grad_t[1] - grad_ad[1] >= 1e-2:
                        sys.exit('case a: layer 1 is not superadiabatic at the start')
                if not never and max(layers) < 2:
                    sys.exit(f'case {name} profile {w}: no iteration with two convecting layers')
                if name == 'd' and w == 1 and not convective.all():
                    sys.exit('case d profile 1 does not convect in every iteration')
                if name == 'd' and w == 2 and (convective.all() or not convective.any()):
                    sys.exit('case d profile 2: a single outcome of the all-zero test')
                outcomes |= set(convective.tolist())
                run['convective'] = convective
                for key in out:
                    out[key].append(run[key])
            if not sens <= 1e-8:
                sys.exit(f'case {name}: sensitivity {sens:.2e} > 1e-8: ill-conditioned, replace it')
            for key, val in out.items():
                store[f'{name}_{key}'] = np.array(val)
            store[f'{name}_sens'] = np.array(sens)
        if outcomes != {True, False}:
            sys.exit('a single outcome of the all-zero test in the whole fixture')
        path = os.path.join(HERE, 'g26_radeq_convection.npz')
        np.savez_compressed(path, **store)
        print(os.path.getsize(path), 'bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
