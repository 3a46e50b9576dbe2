#!/usr/bin/env python3
"""Fixture G31: radiative-equilibrium trajectories with the equilibrium chemistry of every
iteration.  Build container only (CPU):

    python tests/golden/make_golden_radeq_chemistry.py

Unlike G23 and G26 nothing of the reference runs here: its loop asks chemcat for the equilibrium,
which is not available, so no parity with it is claimed (pyratbay_amd/chemistry.py).  The
trajectories are those of the repository's host statements chained by
tests/radeq_chemistry_cases.run_host -- ChemNetwork.equilibrium_host from the previous iterate,
radeq.atmosphere_host, the oracle's interp_ec, plane_parallel_optical_depth and two_stream,
radeq.step_host / step_convective_host -- on the 16-species network of tests/chemistry_cases.py
with its synthetic Gibbs table; the table's species are H2O, CO and CH4, the table is stored as
its two factors like G23's.

Cases, 8 iterations each: (p) L = 9, W = 130, irradiation and tint, one profile; (q) = (p) with
three profiles of their own [M/H] (-0.5, 0, 1), C/O (0.3, 0.55, 1.1) and start; (r) L = 70,
W = 300, hydro_m, Rayleigh H2 + He and CIA H2-H2 + H2-He (fixture G7's tables), convection, a
start that rises from 800 K to 2200 K so that the CH4 / CO changeover lies inside the profile.
For (r) a restarted run is recorded too (`r_restart_*`): 4 iterations, then 4 more from the last
row with its dt_scale, VMRs and iterate and a fresh sign history.

Recorded per case and profile: the inputs, and per iteration temp, dt_scale, Qup, Qdown, sign,
wobble, vmr, chem_iterations and convective.

Trajectory sensitivity `{case}_sens`, G23's way: the chain is run a second time with every row of
flux_up and flux_down (hence Qup, Qdown) and every VMR multiplied by 1 + 1e-12 r, r uniform in
[-1, 1] (seeded); stored is the largest relative temperature deviation over the 8 iterations.  A
case above 1e-8 is ill-conditioned and refused, as is one with a failed solve, a temperature on a
clip bound, or, in (r), without a convecting iteration, with CH4 > CO and CH4 < CO not both
present in the profile of row 1, or with no layer that changes sides of CH4 = CO during the run.
Only data is stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import radeq_cases as rc                           # noqa: E402
import radeq_chemistry_cases as rq                 # noqa: E402

NITER = rq.NITER
RJUP, MJUP = 7.1492e9, 1.8982e30
FLOOR, SWITCH = 1e-9, 1e-6


def make_table(rng, L, W, wn, ntemp=7):
    """Factors of a smooth table, G23's kind for three species: a[S, ntemp, L] (rising with
    temperature, mildly with depth) and b[S, W] (bands over a continuum)."""
    ttable = np.linspace(200.0, 3800.0, ntemp)
    S = len(rq.TABLE_SPECIES)
    x = np.linspace(0.0, 1.0, L)
    a, b = np.empty((S, ntemp, L)), np.empty((S, W))
    for s in range(S):
        a[s] = (1.0 + 0.4 * (ttable[:, None] / 2000.0)**(1.0 + 0.5 * s)) * (1.0 + 0.3 * x[None, :])
        centre = (0.2 + 0.3 * s) * (wn[-1] - wn[0]) + wn[0]
        band = np.exp(-0.5 * ((wn - centre) / (0.15 * (wn[-1] - wn[0])))**2)
        b[s] = 10.0**(-23.5 + 2.0 * band + 0.5 * rng.uniform(-1, 1, W) - 0.4 * s)
    return ttable, a, b


def stellar(orc, wn, tstar, teq):
    """pi B(tstar) diluted to the bolometric flux of a black body at teq."""
    return np.pi * orc.blackbody_wn(wn, tstar) * (teq / tstar)**4


def steep(pressure, t_top, knee, slope):
    """t_top above pressure[knee], T ~ p**slope below it."""
    return t_top * np.maximum(pressure / pressure[knee], 1.0)**slope


def inputs(orc):
    from pyratbay_amd import atmosphere as pa
    g7 = rc.g7()
    net = rq.network()
    store = {}

    def add(name, seed, pressure, wn, temp0, tint, flux_top, radius_model, metal, c_o,
            continuum=False, cia_idx=None, convection=False, p0=0.1):
        rng = np.random.default_rng(seed)
        L, W = len(pressure), len(wn)
        ttable, a, b = make_table(rng, L, W, wn)
        temp0 = np.atleast_2d(temp0)
        gravity, mplanet, r0 = 2200.0, 0.6 * MJUP, 1.0 * RJUP
        # the radius the TableSpectrum is constructed with (the fixed one of (p), (q)): hydro_g
        # of the first starting profile with its equilibrium mean mass
        abund = net.element_abundances_host(metal[0], None, {'C/O': c_o[0]})
        vmr0 = net.equilibrium_host(temp0[0], pressure, abund)[0]
        mu = pa.mean_weight(vmr0, mass=np.array(rq.MASS))
        store[f'{name}_radius'] = pa.hydro_g(pressure, temp0[0], mu, gravity, p0, r0)
        store[f'{name}_pressure'], store[f'{name}_wn'] = pressure, wn
        store[f'{name}_ttable'], store[f'{name}_tab_a'], store[f'{name}_tab_b'] = ttable, a, b
        store[f'{name}_temp0'] = temp0
        store[f'{name}_tint'] = np.atleast_1d(np.asarray(tint, float))
        store[f'{name}_flux_top'] = np.atleast_2d(flux_top)
        store[f'{name}_metal'], store[f'{name}_c_o'] = np.array(metal, float), np.array(c_o, float)
        store[f'{name}_convection'] = np.array(convection)
        tmin, tmax = 200.0, 3800.0
        if continuum:
            tmin = max(tmin, *(float(g7[f'cia_{tag}_temps'].min()) for tag, _ in rc.CIA))
            tmax = min(tmax, *(float(g7[f'cia_{tag}_temps'].max()) for tag, _ in rc.CIA))
            store[f'{name}_cia_idx'] = cia_idx
        store[f'{name}_scalars'] = rc.pack_scalars(radius_model, gravity, mplanet, p0, r0, tmin,
                                                   tmax, continuum)

    wn_p = 250.0 * (12000.0 / 250.0)**np.linspace(0.0, 1.0, 130)           # constant resolution
    p_p = np.logspace(-6, 2, 9)
    star = stellar(orc, wn_p, 5500.0, 1300.0)
    add('p', 31, p_p, wn_p, np.full(9, 1200.0), 150.0, star, None, [0.0], [0.55])
    add('q', 31, p_p, wn_p, np.array([np.full(9, 1200.0), np.full(9, 1000.0),
                                      np.linspace(900.0, 1600.0, 9)]), 150.0, star, None,
        [-0.5, 0.0, 1.0], [0.3, 0.55, 1.1])
    idx = np.arange(0, 600, 2)
    wn_r = g7['wn'][idx]
    p_r = np.logspace(-3.0, 1.0, 70)
    add('r', 33, p_r, wn_r, steep(p_r, 800.0, 50, 0.4), 100.0,
        stellar(orc, wn_r, 5500.0, 1400.0), 'hydro_m', [0.0], [0.55], continuum=True,
        cia_idx=idx, convection=True)
    return store


def checked_run(orc, name, c, w, seed):
    """The trajectory of profile w, its preconditions checked, and its sensitivity."""
    run = rq.run_host(orc, c, w, NITER)
    if run['failures'].any() or np.any(run['chem_status'] <= 0):
        sys.exit(f'case {name} profile {w}: a failed solve')
    temps = run['temps']
    if np.any(temps <= c['tmin']) or np.any(temps >= c['tmax']):
        sys.exit(f'case {name} profile {w}: a temperature on a clip bound')
    # the preconditions of exact signs and convective flags (G23's and G26's floors)
    qnet, qmax = run['qup'] - run['qdown'], np.maximum(run['qup'], run['qdown'])[:, 1:]
    floor = min(np.min(np.abs(np.diff(qnet, axis=1)) / qmax),
                np.min(np.abs(np.diff(qnet + run['conv_flux'], axis=1)) / qmax))
    if not floor >= FLOOR:
        sys.exit(f'case {name} profile {w}: |dF| / max(Qup, Qdown) = {floor:.2e} < {FLOOR}')
    if not run['margin'].min() >= SWITCH:
        sys.exit(f'case {name} profile {w}: |grad_t - grad_ad| = {run["margin"].min():.2e} < '
                 f'{SWITCH}')
    print(f'case {name} profile {w}: floor {floor:.2e}, switch margin {run["margin"].min():.2e}')
    rng = np.random.default_rng(seed)
    noise = 1.0 + 1e-12 * rng.uniform(-1, 1, (NITER, 3, c['L']))
    noisy = rq.run_host(orc, c, w, NITER, noise=noise)['temps']
    sens = float(np.max(np.abs(noisy - temps) / temps))
    its = run['chem_iterations']
    print(f'case {name} profile {w}: T {temps.min():.1f}-{temps.max():.1f} K, wobbling layers '
          f'{run["wobble"].sum(axis=1).tolist()}, convective {run["convective"].tolist()}, '
          f'solver iterations {its.min()}-{its.max()} (mean {its.mean():.2f}), sensitivity '
          f'{sens:.2e}')
    return run, sens


KEYS = ('temps', 'dt_scale', 'qup', 'qdown', 'sign', 'wobble', 'vmr', 'chem_iterations',
        'convective')


def main():
    from oracle import oracle as orc
    orc.lib()
    store = inputs(orc)
    for name in rq.CASES:
        c = rq.unpack(store, name)
        out, sens = {k: [] for k in KEYS}, 0.0
        for w in range(c['nw']):
            run, s = checked_run(orc, name, c, w, 3100 + 10 * ord(name) + w)
            sens = max(sens, s)
            for k in KEYS:
                out[k].append(run[k])
        if not sens <= 1e-8:
            sys.exit(f'case {name}: sensitivity {sens:.2e} > 1e-8: ill-conditioned, replace it')
        for k, v in out.items():
            # (`_vmr` is radeq_cases' key of an input)
            store[f'{name}_{"vmr_hist" if k == "vmr" else k}'] = np.array(v)
        store[f'{name}_sens'] = np.array(sens)
        if name == 'r':
            if not run['convective'].any():
                sys.exit('case r: no convecting iteration')
            ch4, co = (run['vmr'][:, :, rq.SPECIES.index(s)] for s in ('CH4', 'CO'))
            if not (np.any(ch4[0] > co[0]) and np.any(ch4[0] < co[0])):
                sys.exit('case r: the CH4 / CO changeover is not inside the profile of row 1')
            moved = int(np.sum((ch4[0] > co[0]) != (ch4[-1] > co[-1])))
            print(f'case r: {moved} layers change sides of CH4 = CO between rows 1 and {NITER}')
            if not moved:
                sys.exit('case r: no layer crosses CH4 = CO during the run')
            half = NITER // 2
            first = rq.run_host(orc, c, 0, half)
            second = rq.run_host(orc, c, 0, half, carried=first)
            restart = np.vstack([first['temps'], second['temps'][1:]])
            if np.array_equal(restart, run['temps']):
                sys.exit('case r: the restarted run equals the straight one: it pins nothing')
            noise = 1.0 + 1e-12 * np.random.default_rng(78).uniform(-1, 1, (NITER, 3, c['L']))
            n1 = rq.run_host(orc, c, 0, half, noise=noise[:half])
            n2 = rq.run_host(orc, c, 0, half, carried=n1, noise=noise[half:])
            rsens = float(np.max(np.abs(np.vstack([n1['temps'], n2['temps'][1:]]) - restart) /
                                 restart))
            dev = np.max(np.abs(restart - run['temps']) / run['temps'])
            print(f'case r restarted after {half} iterations: differs from the straight run by up '
                  f'to {dev:.2e} in temperature; sensitivity {rsens:.2e}')
            if not rsens <= 1e-8:
                sys.exit(f'case r restarted: sensitivity {rsens:.2e} > 1e-8')
            store['r_restart_temps'], store['r_restart_sens'] = restart, np.array(rsens)
            store['r_restart_dt_scale'] = np.vstack([first['dt_scale'], second['dt_scale']])
    path = os.path.join(HERE, 'g31_radeq_chemistry.npz')
    np.savez_compressed(path, **store)
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
