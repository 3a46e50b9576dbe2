"""Helpers of the tests of radiative equilibrium with the equilibrium chemistry of every iteration
(test_radeq_chemistry_cpu.py, test_gpu_radeq_chemistry.py) and of
tests/golden/make_golden_radeq_chemistry.py, on top of radeq_cases.py and chemistry_cases.py: the
warm-start grid, the cases of fixture G31 as dicts, and the host chain of one trajectory --
ChemNetwork.equilibrium_host, radeq.atmosphere_host with that VMR, the oracle's interp_ec,
plane_parallel_optical_depth(maxdepth = inf) and two_stream, then radeq.step_host or
step_convective_host.

The network is the 16-species one of chemistry_cases.py with its synthetic Gibbs table; the table's
species are H2O, CO and CH4.  chemcat is not used: no parity with it is claimed (chemistry.py)."""
import functools
import os

import numpy as np

import chemistry_cases as cc
import radeq_cases as rc

CASES = ('p', 'q', 'r')
NITER = rc.NITER
SPECIES, MASS = cc.SPECIES, cc.MASS
TABLE_SPECIES = ['H2O', 'CO', 'CH4']
# cp / R of the 16 species on radeq_convection_cases' kind of grid: atoms 2.5, diatomic molecules
# 3.5-4.5, the others 4-6.5, rising smoothly with temperature
CP_TEMPS = np.array([100.0, 200.0, 300.0, 450.0, 600.0, 800.0, 1000.0, 1300.0, 1700.0, 2200.0,
                     3000.0, 4000.0])
ATOMS, DIATOMIC = ('H', 'He', 'O', 'C', 'N'), ('H2', 'CO', 'N2', 'OH', 'O2')

# ------------------------------------------------------------------------- the warm-start grid
GRID_P = [1e-8, 1e-6, 1e-4, 1e-2, 1.0, 100.0]
GRID_T = [350.0, 700.0, 1000.0, 1500.0, 2500.0, 4000.0, 5500.0]
GRID_DT = [1.0, -1.0, 10.0, -10.0, 50.0, -50.0, 300.0, -300.0, 1500.0, -1500.0]


def warm_grid():
    """(pressure, t_start, t_solve, dT) of the warm-start grid, each [n]: every (p, T, dT) with
    300 K <= T - dT <= 6000 K, in BOTH directions -- started from the solution at T and solved at
    T - dT, and started at T - dT and solved at T (2 x 384 cells)."""
    cells = [(p, t, d) for p in GRID_P for t in GRID_T for d in GRID_DT if 300.0 <= t - d <= 6000.0]
    p, t, d = (np.array(v) for v in zip(*cells))
    return (np.concatenate([p, p]), np.concatenate([t, t - d]), np.concatenate([t - d, t]),
            np.concatenate([d, d]))


def network():
    from pyratbay_amd import chemistry as ch
    return cc.network(ch)


def cp_table():
    x = CP_TEMPS / (CP_TEMPS + 1500.0)
    cols = [np.full_like(x, 2.5) if s in ATOMS else 3.5 + 1.0 * x if s in DIATOMIC else
            4.0 + 2.5 * x for s in SPECIES]
    return np.stack(cols, axis=1)


# ----------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(rc.GOLDEN, 'g31_radeq_chemistry.npz'))


def unpack(store, name):
    """The inputs of case `name`: radeq_cases' keys without vmr, plus metal[nw], c_o[nw],
    convection and the heat-capacity table."""
    c = rc.unpack(store, name)
    c['mol_mass'] = np.array(MASS)
    c['metal'], c['c_o'] = np.asarray(store[f'{name}_metal']), np.asarray(store[f'{name}_c_o'])
    c['convection'] = bool(store[f'{name}_convection'])
    c['cp_temps'], c['cp_table'] = CP_TEMPS, cp_table()
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return unpack(fixture(), name)


def abundances(c, w):
    return network().element_abundances_host(float(c['metal'][w]), None,
                                             {'C/O': float(c['c_o'][w])})


def build(eng, c, w=None, **kw):
    """(TableSpectrum, RadiativeEquilibrium) of a case on the device; w: that profile alone."""
    from pyratbay_amd import radeq
    cont = rc.continuum_models(c) if c['continuum'] else None
    top = None if c['flux_top'].size == 0 else c['flux_top'][0]
    model = eng.TableSpectrum(c['etable'], c['ttable'], c['wn'], c['radius'], 1.0,
                              rt_path='emission_two_stream', continuum=cont, timestamps=False,
                              tint=float(c['tint'][0]), flux_top=top)
    pick = (lambda v: v if c['nw'] > 1 else float(v[0])) if w is None else (lambda v: float(v[w]))
    args = dict(tint=float(c['tint'][0]), flux_top=top, tmin=c['tmin'], tmax=c['tmax'],
                table_species=TABLE_SPECIES, chemistry=network(), metallicity=pick(c['metal']),
                e_ratio={'C/O': pick(c['c_o'])})
    args.update(rc.radius_kwargs(c))
    if c['convection']:
        args.update(heat_capacity=(c['cp_temps'], c['cp_table']), mplanet=c['mplanet'])
    args.update(kw)
    return model, radeq.RadiativeEquilibrium(model, c['pressure'], None, c['mol_mass'], **args)


# ------------------------------------------------------------------------------ the host chain
def host_fluxes(orc, c, temp, vmr):
    """(flux_down, flux_up, radius) of one profile at `temp` with the VMRs vmr[L, S]:
    radeq_cases.host_fluxes with the network's species."""
    from oracle import continuum as oc
    from pyratbay_amd import radeq
    L, W = c['L'], c['W']
    temp = np.ascontiguousarray(temp)
    dens, radius = radeq.atmosphere_host(temp, c['pressure'], vmr, c['mol_mass'],
                                         **rc.radius_kwargs(c))
    radius = c['radius'] if radius is None else radius
    ec = np.zeros((L, W))
    itab = [SPECIES.index(s) for s in TABLE_SPECIES]
    orc.interp_ec(ec, c['etable'], c['ttable'], temp, np.ascontiguousarray(dens[:, itab]), 0, L)
    if c['continuum']:
        d = {s: dens[:, i] for i, s in enumerate(SPECIES)}
        for s in ('H2', 'He'):
            ec += oc.rayleigh_cross_section(c['wn'], s) * d[s][:, None]
        for species, tab, temps, lo, hi in rc.cia_tables(c):
            ec += oc.cia_cross_section(tab, temps, temp, lo, hi) * \
                (d[species[0]] * d[species[1]])[:, None]
    depth = np.zeros((L, W))
    stop = np.zeros(W, np.int32)
    orc.plane_parallel_optical_depth(depth, stop, ec, np.ascontiguousarray(-np.diff(radius)),
                                     np.inf, 0, L)
    f_int = orc.internal_flux(c['wn'], float(c['tint'][0]))
    top = None if c['flux_top'].size == 0 else np.ascontiguousarray(c['flux_top'][0])
    down, up = orc.two_stream(depth, c['wn'], temp, f_int, top, 0)
    return down, up, radius


def switch_margin(c, vmr, temp_next):
    """min over the layers >= 1 of |grad_t - grad_ad| (convection.py:49-55) at the temperatures the
    radiative half produced: how far the profile is from the switch of the convective flux."""
    from pyratbay_amd import atmosphere as pa, radeq
    cp = np.sum(radeq.heat_capacity_host(c['cp_temps'], c['cp_table'], temp_next) * vmr,
                axis=1) * pa.K_BOLTZ / radeq.AMU
    dpress = np.ediff1d(np.log(c['pressure'] * 1e6), to_begin=1.0)
    grad_t = np.ediff1d(np.log(temp_next), to_begin=0.0) / dpress
    grad_ad = 1.0 - (cp - pa.K_BOLTZ / radeq.AMU) / cp
    return float(np.min(np.abs(grad_t - grad_ad)[1:]))


def run_host(orc, c, w, nsamples, temp0=None, start='previous', carried=None, noise=None):
    """The loop with chemistry on the host, profile w of case c: per iteration the fluxes of the
    profile with its VMRs, the update (with convection where the case has it), then the
    equilibrium at the new temperatures -- from the previous iterate (start='previous', with
    ChemNetwork's TOL_ALL) or from the cold start -- whose failed layers keep their VMRs.
    carried: the dict a run returned, to go on from its last row with its dt_scale, VMRs and
    iterate and a fresh sign history (continue_run).  noise[nsamples, 3, L]: factors on the rows of
    flux_up, flux_down and of the VMRs of the iteration's solve.
    Returns a dict: temps[1 + nsamples, L], and per iteration dt_scale, qup, qdown, sign, wobble
    conv_flux [nsamples, L], vmr[nsamples, L, S], chem_iterations, chem_status [nsamples, L],
    convective, margin (switch_margin; inf without convection) [nsamples]; vmr_last, iterate,
    failures[L]."""
    from pyratbay_amd import radeq
    net, L, p = network(), c['L'], c['pressure']
    b = abundances(c, w)
    if carried is None:
        temp = np.array(c['temp0'][w] if temp0 is None else temp0, float)
        dt_scale = np.full(L, radeq.DT_SCALE0)
        vmr, _, status, iterate = net.equilibrium_host(temp, p, b, start='cold')
        assert np.all(status > 0)
    else:
        temp, dt_scale = carried['temps'][-1], carried['dt_scale'][-1]
        vmr, iterate = carried['vmr_last'], carried['iterate']
    signs = np.zeros((0, L))
    out = {k: [] for k in ('dt_scale', 'qup', 'qdown', 'sign', 'wobble', 'vmr', 'chem_iterations',
                           'chem_status', 'convective', 'conv_flux', 'margin')}
    temps, failures = [temp], np.zeros(L, np.int32)
    dpress = radeq.log_pressure_steps(p)
    for i in range(nsamples):
        down, up, radius = host_fluxes(orc, c, temp, vmr)
        if noise is not None:
            up, down = up * noise[i, 0][:, None], down * noise[i, 1][:, None]
        qup, qdown = np.trapezoid(up, c['wn'], axis=1), np.trapezoid(down, c['wn'], axis=1)
        if c['convection']:
            s = radeq.step_convective_host(temp, dt_scale, signs, qup, qdown, dpress, p, vmr,
                                           c['mol_mass'], radius, c['cp_temps'], c['cp_table'],
                                           c['mplanet'], tmin=c['tmin'], tmax=c['tmax'])
            out['margin'].append(switch_margin(c, vmr, s['radiative']['temp']))
        else:
            s = dict(radeq.step_host(temp, dt_scale, signs, qup, qdown, dpress, c['tmin'],
                                     c['tmax']), convective=False, conv_flux=np.zeros(L))
            out['margin'].append(np.inf)
        temp, dt_scale = s['temp'], s['dt_scale']
        signs = np.vstack([signs, s['sign']])
        new, its, status, new_iterate = net.equilibrium_host(
            temp, p, b, start=iterate if start == 'previous' else 'cold')
        good = status > 0
        failures += ~good
        vmr = np.where(good[:, None], new, vmr)
        iterate = tuple(np.where(good.reshape((-1,) + (1,) * (n.ndim - 1)), n, o)
                        for n, o in zip(new_iterate, iterate))
        if noise is not None:
            vmr = vmr * noise[i, 2][:, None]
        temps.append(temp)
        for k, v in (('dt_scale', dt_scale), ('qup', qup), ('qdown', qdown), ('sign', s['sign']),
                     ('wobble', s['wobble']), ('vmr', vmr), ('chem_iterations', its),
                     ('chem_status', status), ('convective', s['convective']),
                     ('conv_flux', s['conv_flux'])):
            out[k].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    out.update(temps=np.array(temps), vmr_last=vmr, iterate=iterate, failures=failures)
    return out
