#!/usr/bin/env python3
"""Fixture G28: what the reference makes of a `retrieval_params` block -- the parsed columns, the
index maps of the name resolution (pyrat/retrieval.py:77-121, 167-284), the state eval() leaves in
its objects for a handful of parameter vectors (pyrat_obj.py:258-297) and the full vector
Loglike.__call__ builds from a free vector (tools/retrieval_tools.py:91-93).  Build container only:

    python tests/golden/make_golden_retrieval.py

Runs of the real package (imported as in make_golden_e2e.py) from the reference's own
spectrum_{eclipse,transmission}_filters_test.cfg without `sampled_cross_sec`, with a
retrieval_params block that has lines of 2, 5, 7 and 8 fields, a fixed and a shared line.  T_eff
needs spec.flux_interp, which the run does not set for a black-body star: it is set by hand to an
interp1d over three scaled copies of spec.starflux.  The Loglike object is created without its
constructor, as in make_golden_loglike.py.  Only data is stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_e2e as e2e                      # noqa: E402
import make_golden_reference_cases as rc           # noqa: E402

REF = e2e.REF
REMOVE = ['sampled_cross_sec']
NROWS = 6
SED_TEMPS = np.array([5000.0, 5800.0, 6500.0])
SED_SCALES = np.array([0.8, 1.0, 1.25])

#   name          value    pmin    pmax  pstep   prior priorlow priorup
BLOCK = """
    log_kappa'     -4.2    -6.0     3.0    0.3
    log_gamma1     -1.0    -3.0     3.0    0.3    -1.0     0.5
    log_gamma2      0.0    -3.0     3.0   -2
    alpha           0.0
    T_irr        1485.0   100.0  3000.0   50.0  1500.0   100.0   200.0
    T_int         100.0     0.0  1000.0    0.0
    {radius}
    M_planet        0.6     0.1     2.0    0.05
    log_H2O        -4.0   -10.0    -1.0    0.3
    log_p_cl        1.0    -6.0     2.0    0.3
    log_k_ray       0.0    -5.0     5.0    0.3     0.5     1.0     2.0
    alpha_ray      -4.0    -8.0     0.0    0.2
    f_patchy        0.5     0.0     1.0    0.1
    T_eff        5800.0  5000.0  6500.0   50.0
    f_dilution      0.9     0.0     1.0    0.05
"""
RADIUS = {'eclipse': 'R_planet      1.105     0.5     2.5    0.05',
          'transmission': 'log_p_ref      -1.0    -3.0     1.0    0.2'}


def index(a):
    return np.array([] if a is None else a, dtype=np.int64).reshape(-1)


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_ret_')
    store = {}
    try:
        pb = e2e.reference_package(work)
        import pyratbay.constants as pc
        import pyratbay.tools as pt
        from pyratbay.tools.retrieval_tools import Loglike
        from scipy.interpolate import interp1d
        os.chdir(work)
        store['rjup'], store['mjup'] = np.array(pc.rjup), np.array(pc.mjup)
        # (Atmosphere.mplanet is a descriptor that re-derives the mass from the gravity it implies,
        # pyrat/atmosphere.py:20-48: what eval() leaves there can be an ulp from what it assigned)
        store['G'] = np.array(pc.G)
        for tag in ('eclipse', 'transmission'):
            base = f'{REF}/tests/configs/spectrum_{tag}_filters_test.cfg'
            block = BLOCK.format(radius=RADIUS[tag])
            pyrat = pb.run(rc.make_config(work, base, {'retrieval_params': block}, REMOVE,
                                          f'{tag}_retrieval'))
            ret, atm, spec, opacity = pyrat.ret, pyrat.atm, pyrat.spec, pyrat.opacity
            store[f'{tag}_block'] = np.array(block)
            store[f'{tag}_runits'] = np.array(str(atm.runits))
            store[f'{tag}_mass_units'] = np.array(str(atm.mass_units))
            store[f'{tag}_pnames'] = np.array(ret.pnames)
            for name in ('params', 'pmin', 'pmax', 'pstep', 'prior', 'priorlow', 'priorup'):
                store[f'{tag}_{name}'] = np.array(getattr(ret, name), float)
            for name in ('irad', 'ipress', 'imass', 'ipatchy', 'itstar', 'idilut', 'irv', 'itemp',
                         'imol'):
                store[f'{tag}_{name}'] = index(getattr(ret, name))
            store[f'{tag}_map_temp'] = index(ret.map_pars['temp'])
            store[f'{tag}_map_mol'] = np.array(ret.map_pars['mol'], np.int64).reshape(-1, 2)
            store[f'{tag}_temp_pnames'] = np.array(atm.temp_model.pnames)
            store[f'{tag}_mol_pnames'] = np.array(atm.mol_pnames)
            store[f'{tag}_nopacity'] = np.array(len(opacity.models))
            for j, model in enumerate(opacity.models):
                store[f'{tag}_opacity{j}_name'] = np.array(str(getattr(model, 'name', '')))
                store[f'{tag}_opacity{j}_pnames'] = np.array(list(opacity.pnames[j]), dtype=str)
                store[f'{tag}_iopacity{j}'] = index(ret.iopacity[j])
                store[f'{tag}_map_opacity{j}'] = index(ret.map_pars['opacity'][j])

            # T_eff: a stellar grid by hand (three scaled copies of the run's black body)
            starflux = np.copy(spec.starflux)
            spec.flux_interp = interp1d(SED_TEMPS, SED_SCALES[:, None] * starflux[None, :],
                                        axis=0)
            store[f'{tag}_sed_temps'], store[f'{tag}_sed_scales'] = SED_TEMPS, SED_SCALES

            # free vectors inside the bounds, the first one at the block's values
            ifree = ret.pstep > 0
            rng = np.random.default_rng(28)
            lo = np.maximum(ret.pmin[ifree], ret.params[ifree] - 2.0 * ret.pstep[ifree])
            hi = np.minimum(ret.pmax[ifree], ret.params[ifree] + 2.0 * ret.pstep[ifree])
            theta = rng.uniform(lo, hi, (NROWS, int(np.sum(ifree))))
            theta[0] = ret.params[ifree]

            ll = object.__new__(Loglike)
            ll.obs = pyrat.obs
            # (the obsfile holds filters without data: __call__'s sums get stand-ins)
            ll.data, ll.uncert = np.ones(2), np.ones(2)
            ll.params = np.copy(ret.params)
            ll.pstep = ret.pstep
            ll.ifree = ifree
            ll.ishare = np.where(ret.pstep < 0)[0]
            ll._dt_snapshot = 0.0
            seen = {}

            def func(params, retmodel=False):
                seen['full'] = np.copy(params)
                pyrat.eval(params, retmodel=False)
                return np.copy(ll.data)
            ll.func = func
            rows = {k: [] for k in ('full', 'tpars', 'vmr_pars', 'rplanet', 'mplanet',
                                    'mplanet_assigned',
                                    'refpressure', 'fpatchy', 'tstar', 'f_dilution')}
            opars = [[] for _ in opacity.models]
            for row in theta:
                ll(row)
                rows['full'].append(seen['full'])
                rows['tpars'].append(np.array(atm.tpars, float))
                rows['vmr_pars'].append(np.array([p for pars in atm.vmr_pars for p in pars],
                                                 float))
                rows['rplanet'].append(float(atm.rplanet))
                rows['mplanet'].append(float(atm.mplanet))
                rows['mplanet_assigned'].append(
                    float(seen['full'][ret.imass][0] * pt.u(atm.mass_units)))
                rows['refpressure'].append(float(atm.refpressure))
                rows['fpatchy'].append(float(opacity.fpatchy))
                rows['tstar'].append(float(atm.tstar))
                rows['f_dilution'].append(float(spec.f_dilution))
                for j, model in enumerate(opacity.models):
                    opars[j].append(np.array(getattr(model, 'pars', []), float).reshape(-1))
            store[f'{tag}_theta'] = theta
            for k, v in rows.items():
                store[f'{tag}_row_{k}'] = np.array(v)
            for j, v in enumerate(opars):
                store[f'{tag}_row_opacity{j}_pars'] = np.array(v)
            print(tag, ret.pnames, 'free', int(np.sum(ifree)))
            print('  rplanet', rows['rplanet'][:2], 'mplanet', rows['mplanet'][:2])
        np.savez_compressed(os.path.join(HERE, 'g28_retrieval.npz'), **store)
        print({k: np.shape(v) for k, v in store.items()})
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
