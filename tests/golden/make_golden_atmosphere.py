#!/usr/bin/env python3
"""Fixture G22: atmospheres from retrieval parameters -- the functions Atmosphere.calc_profiles
(pyratbay/pyrat/atmosphere.py:399-526) chains.  Build container only:

    python tests/golden/make_golden_atmosphere.py

Calls of the real package (imported as in make_golden_e2e.py): pa.tmodels.Isothermal / Guillot /
Madhu, pa.vmr_models.IsoVMR / ScaleVMR / SlantVMR, pa.vmr_scale, pa.qcapcheck,
pa.ideal_gas_density, pa.mean_weight, pa.hydro_m, pa.hydro_g.

A full Atmosphere.calc_profiles run is NOT recorded: the reference ships no ready config of the
families that need no line data (its tests write them from a template at run time, through their
conftest), so driving one here would mean restating that template.  Every case instead chains the
functions in calc_profiles' order -- temperature, vmr_scale with the bulk ratios of the base VMR,
ideal_gas_density, mean_weight(mass=...), the radius model -- with the arguments calc_profiles
passes (iscale, ibulk, bratio, invsrat given).

Every case is one such chain; a case varies one step and keeps the others at a default.  The
case list travels in the archive as JSON (`cases`), the arrays as c{i}_{temp,vmr,dens,mm,radius}.
Only data is stored."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_e2e as e2e                      # noqa: E402

REF = e2e.REF
SPECIES = ['H2', 'He', 'H2O', 'CH4', 'CO', 'CO2']
MASS = [2.01588, 4.002602, 18.01528, 16.0425, 28.0101, 44.0095]
MJUP, RJUP = 1.8982e30, 7.1492e9

# pressure grids (bar): log-uniform 1e-8 ... 100 bar, and a narrow one on which madhu's filter
# radius (13) exceeds the number of layers
GRIDS = {'p2': (-8.0, 2.0, 2), 'p11': (-8.0, 2.0, 11), 'p65': (-8.0, 2.0, 65),
         'p81': (-8.0, 2.0, 81), 'narrow11': (-2.0, -1.0, 11)}

GUILLOT = [
    # log kappa', log gamma1, log gamma2, alpha, T_irr, T_int; gravity
    ([-4.8, -0.6, 0.0, 0.0, 1200.0, 100.0], None),       # inverted; tau gamma crosses 1
    ([-4.8, 0.2, 0.0, 0.0, 1200.0, 100.0], None),        # non-inverted
    ([-1.5, -0.8, -0.8, 0.5, 1200.0, 100.0], 2200.0),    # scalar gravity
    ([-1.0, 0.0, 0.3, 0.3, 1500.0, 150.0], None),        # tau gamma > 88.03 at the bottom
    ([-9.5, -0.3, 0.4, 0.7, 900.0, 50.0], None),         # tau gamma < 1 in every layer
    ([-2.0, 1.0, -1.0, 0.25, 2000.0, 300.0], 980.0),
]
MADHU = [
    ([-3.5, 0.0, 0.5, 3.0, 0.5, 1500.0], 'p81'),         # inverted (p2 > p1)
    ([-3.5, -4.0, 0.5, 3.0, 0.5, 1100.0], 'p81'),        # non-inverted
    ([0.7, -1.0, 0.5, 3.0, 0.5, 1100.0], 'p11'),         # log_p1 > log_p3: zeros
    ([-1.6, -1.4, -1.2, 1.0, 0.8, 1000.0], 'narrow11'),  # filter radius > L
    ([-4.0, -2.0, 1.0, 2.0, 0.7, 900.0], 'p2'),          # two layers: one-tap filter
]
VMR = [
    # bulk, models (kind, species), parameters, qcap
    (['H2'], [('iso', 'H2O')], [-3.2], None),
    (['H2', 'He'], [('iso', 'H2O')], [-3.2], None),
    (['H2'], [('iso', 'H2O'), ('scale', 'CO')], [-2.5, 0.7], None),
    (['H2', 'He'], [('iso', 'H2O'), ('scale', 'CO')], [-2.5, -1.2], None),
    (['H2', 'He'], [('slant', 'H2O'), ('scale', 'CH4'), ('iso', 'CO2')],
     [0.75, -3.3, -3.0, -6.0, -2.5, 0.4, -5.5], None),   # the slant hits both clips
    (['H2'], [('slant', 'CO'), ('iso', 'CH4'), ('scale', 'H2O')],
     [-0.2, -4.0, 0.0, -10.0, -1.0, -3.7, 1.1], None),
    (['H2', 'He'], [('iso', 'H2O'), ('iso', 'CO')], [-0.8, -1.1], 0.2),   # above the cap
]
# radius model, grid, reference pressure ('layer k': pressure[k]; or bar), r0, mplanet, gplanet
RADIUS = [
    ('hydro_m', 'p11', 'layer 7', 1.0 * RJUP, 0.6 * MJUP, None),
    ('hydro_m', 'p11', 0.03, 1.0 * RJUP, 0.6 * MJUP, None),
    ('hydro_m', 'p11', 'layer 0', 1.3 * RJUP, 1.0 * MJUP, None),
    ('hydro_m', 'p65', 'layer 64', 0.9 * RJUP, 1.0 * MJUP, None),
    ('hydro_g', 'p11', 'layer 7', 1.0 * RJUP, None, 2478.0),
    ('hydro_g', 'p65', 0.03, 1.0 * RJUP, None, 2478.0),
    ('hydro_g', 'p11', 'layer 0', 1.3 * RJUP, None, 1000.0),
    ('hydro_g', 'p11', 'layer 10', 0.9 * RJUP, None, 1000.0),
    ('hydro_m', 'p11', 0.1, 1.5 * RJUP, 0.02 * MJUP, None),      # diverges: low mass, hot
]


def base_vmr(nlayers):
    """Layer-dependent abundances (float32-representable: the archive stays small), so that the
    bulk ratios differ from layer to layer."""
    x = np.linspace(0.0, 1.0, nlayers)
    vmr = np.zeros((nlayers, len(SPECIES)))
    vmr[:, 1] = 0.149 * (1.0 + 0.05 * np.cos(3.0 * x))
    vmr[:, 2] = 4e-4 * (1.0 + 0.5 * x)
    vmr[:, 3] = 1e-4 * (1.0 - 0.3 * x)
    vmr[:, 4] = 5e-4 * (1.0 + 0.2 * np.sin(5.0 * x))
    vmr[:, 5] = 1e-7
    vmr = np.asarray(vmr, np.float32).astype(np.float64)
    vmr[:, 0] = 1.0 - np.sum(vmr[:, 1:], axis=1)
    return vmr


def case_list():
    default = dict(grid='p11', tmodel='guillot', tpars=GUILLOT[0][0], gravity=None,
                   bulk=['H2', 'He'], vmr_models=[['iso', 'H2O']], vmr_pars=[-3.2], qcap=None,
                   rmodel='hydro_m', refpressure=0.1, rplanet=1.0 * RJUP, mplanet=0.6 * MJUP,
                   gplanet=None)
    cases = []

    def add(group, **kw):
        cases.append(dict(default, group=group, **kw))
    add('isothermal', tmodel='isothermal', tpars=[1500.0], grid='p11')
    add('isothermal', tmodel='isothermal', tpars=[873.25], grid='p2')
    for i, (pars, gravity) in enumerate(GUILLOT):
        add('guillot', tpars=pars, gravity=gravity, grid='p81' if i == 0 else
            ('p65' if i == 3 else 'p11'))
    # (hot top layers on a 0.6 Mjup planet: fixed gravity keeps these about the T model)
    for pars, grid in MADHU:
        add('madhu', tmodel='madhu', tpars=pars, grid=grid, rmodel='hydro_g', gplanet=2478.0,
            refpressure=0.03 if grid == 'narrow11' else 0.1)
    for bulk, models, pars, qcap in VMR:
        add('vmr', bulk=bulk, vmr_models=[list(m) for m in models], vmr_pars=pars, qcap=qcap)
    for rmodel, grid, p0, r0, mass, grav in RADIUS:
        kw = {}
        if rmodel == 'hydro_m' and mass == 0.02 * MJUP:
            kw = dict(tmodel='isothermal', tpars=[3000.0])
        add('radius', rmodel=rmodel, grid=grid, refpressure=p0, rplanet=r0, mplanet=mass,
            gplanet=grav, **kw)
    return cases


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_atm_')
    store = {}
    try:
        e2e.reference_package(work)
        import pyratbay.atmosphere as pa
        import pyratbay.constants as pc
        import scipy

        store['scipy_version'] = np.array(scipy.__version__)
        store['constants'] = np.array([pc.k, pc.G, scipy.constants.N_A, pc.bar])
        store['species'] = np.array(SPECIES)
        store['mass'] = np.array(MASS)
        for name, (lo, hi, n) in GRIDS.items():
            store[f'grid_{name}'] = np.logspace(lo, hi, n)
            store[f'base_vmr_{name}'] = base_vmr(n)
        cases = case_list()
        for i, c in enumerate(cases):
            pressure = store[f'grid_{c["grid"]}']
            vmr0 = store[f'base_vmr_{c["grid"]}']
            if isinstance(c['refpressure'], str):
                c['refpressure'] = float(pressure[int(c['refpressure'].split()[1])])
                c['on_layer'] = True
            # --- calc_profiles' order
            if c['tmodel'] == 'isothermal':
                tmodel = pa.tmodels.Isothermal(pressure)
            elif c['tmodel'] == 'guillot':
                tmodel = pa.tmodels.Guillot(pressure, c['gravity'])
            else:
                tmodel = pa.tmodels.Madhu(pressure)
            temp = tmodel(np.array(c['tpars']))
            store[f'c{i}_temp'] = temp
            c['stops_after'] = 'temp' if np.any(temp <= 0) else None
            if c['stops_after']:
                continue
            models, pars, k = [], [], 0
            for kind, spec in c['vmr_models']:
                if kind == 'iso':
                    models.append(pa.vmr_models.IsoVMR(spec, pressure))
                elif kind == 'scale':
                    models.append(pa.vmr_models.ScaleVMR(spec, pressure,
                                                         vmr0[:, SPECIES.index(spec)]))
                else:
                    models.append(pa.vmr_models.SlantVMR(spec, pressure))
                pars.append(np.array(c['vmr_pars'][k:k + models[-1].npars]))
                k += models[-1].npars
            assert k == len(c['vmr_pars'])
            ibulk = [SPECIES.index(b) for b in c['bulk']]
            iscale = [SPECIES.index(m.species) for m in models]
            bratio, invsrat = pa.ratio(vmr0, ibulk)
            vmr = pa.vmr_scale(vmr0, np.array(SPECIES), models, pars, c['bulk'], iscale=iscale,
                               ibulk=ibulk, bratio=bratio, invsrat=invsrat)
            c['qcap_flag'] = bool(pa.qcapcheck(vmr, c['qcap'], ibulk))
            dens = pa.ideal_gas_density(vmr, pressure, temp)
            mm = pa.mean_weight(vmr, mass=np.array(MASS))
            if c['rmodel'] == 'hydro_m':
                radius = pa.hydro_m(pressure, temp, mm, c['mplanet'], c['refpressure'],
                                    c['rplanet'])
            else:
                radius = pa.hydro_g(pressure, temp, mm, c['gplanet'], c['refpressure'],
                                    c['rplanet'])
            c['divergent'] = bool(np.any(np.isinf(radius)))
            store[f'c{i}_vmr'], store[f'c{i}_dens'] = vmr, dens
            store[f'c{i}_mm'], store[f'c{i}_radius'] = mm, radius
            print(i, c['group'], c['grid'], c['tmodel'], c['rmodel'],
                  f'T {temp.min():.1f}-{temp.max():.1f}', 'qcap' if c['qcap_flag'] else '',
                  'divergent' if c['divergent'] else '')
        # what the issue's list asks of the parameter sets, checked where it can be
        islant = [i for i, c in enumerate(cases) if c['vmr_models'][0] == ['slant', 'H2O']][0]
        slant = store[f'c{islant}_vmr'][:, SPECIES.index('H2O')]
        assert np.isclose(slant.min(), 10.0**-6.0) and np.isclose(slant.max(), 10.0**-2.5)
        assert sum(c.get('qcap_flag', False) for c in cases) == 1
        assert sum(c.get('divergent', False) for c in cases) == 1
        store['cases'] = np.array(json.dumps(cases))
        out = os.path.join(HERE, 'g22_atmosphere.npz')
        np.savez_compressed(out, **store)
        print(len(cases), 'cases,', os.path.getsize(out), 'bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
