"""Shared by the atmosphere tests: fixture G22 (tests/golden/make_golden_atmosphere.py) and the
WalkerAtmosphere of one of its cases."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUTPUTS = ('temp', 'vmr', 'dens', 'mm', 'radius')
TABLE_SPECIES = ['H2O', 'CH4', 'CO', 'CO2']
_g22 = None


def g22():
    global _g22
    if _g22 is None:
        z = np.load(os.path.join(HERE, 'golden', 'g22_atmosphere.npz'))
        _g22 = {k: z[k] for k in z.files}
        _g22['case_list'] = json.loads(str(_g22['cases']))
    return _g22


def models(case, pressure, base_vmr, species):
    from pyratbay_amd import atmosphere as pa
    if case['tmodel'] == 'isothermal':
        tmodel = pa.Isothermal(pressure)
    elif case['tmodel'] == 'guillot':
        tmodel = pa.Guillot(pressure, case['gravity'])
    else:
        tmodel = pa.Madhu(pressure)
    vmr_models = []
    for kind, spec in case['vmr_models']:
        if kind == 'iso':
            vmr_models.append(pa.IsoVMR(spec, pressure))
        elif kind == 'scale':
            vmr_models.append(pa.ScaleVMR(spec, pressure, base_vmr[:, species.index(spec)]))
        else:
            vmr_models.append(pa.SlantVMR(spec, pressure))
    return tmodel, vmr_models


def walker_atmosphere(case, base_radius=None, free_scalars=(), **kw):
    """(WalkerAtmosphere bound to TABLE_SPECIES, parameter vector) of a G22 case; free_scalars:
    scalars moved from the constants to the end of the parameter vector."""
    from pyratbay_amd import atmosphere as pa
    g = g22()
    species = [str(s) for s in g['species']]
    pressure, base_vmr = g[f'grid_{case["grid"]}'], g[f'base_vmr_{case["grid"]}']
    tmodel, vmr_models = models(case, pressure, base_vmr, species)
    params = list(case['tpars']) + list(case['vmr_pars'])
    const = dict(mplanet=case['mplanet'], gplanet=case['gplanet'], rplanet=case['rplanet'],
                 refpressure=case['refpressure'])
    free = list(tmodel.pnames) + [n for m in vmr_models for n in m.pnames]
    for s in free_scalars:
        free.append(s)
        key = 'refpressure' if s == 'log_refpressure' else s
        value = const.pop(key)
        params.append(np.log10(value) if s == 'log_refpressure' else value)
    if base_radius is None:
        base_radius = np.linspace(1.1, 0.9, len(pressure)) * case['rplanet']
    args = dict(rmodel=case['rmodel'], qcap=case['qcap'], base_radius=base_radius, free=free)
    args.update(const)
    args.update(kw)
    atm = pa.WalkerAtmosphere(pressure, species, g['mass'], base_vmr, case['bulk'], tmodel,
                              vmr_models, **args)
    atm.bind(TABLE_SPECIES)
    return atm, np.array(params, float)


def max_rel(got, want):
    """Worst relative deviation over the finite, non-zero reference values; inf and zeros must
    match exactly."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[special], want[special])
    if np.all(special):
        return 0.0
    return float(np.max(np.abs(got[~special] / want[~special] - 1.0)))
