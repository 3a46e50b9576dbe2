"""Helpers of the convective radiative-equilibrium tests (test_radeq_convection_cpu.py,
test_gpu_radeq_convection.py) and of tests/golden/make_golden_radeq_convection.py, on top of
radeq_cases.py: the cases of fixture G26 as dicts (radeq_cases' keys plus the heat-capacity table
cp_temps[nT], cp_table[nw, nT, S], one table per profile), the host statements chained along a
trajectory, and pb_radeq_update_convective on a hand-made state."""
import functools
import os

import numpy as np

import radeq_cases as rc

CASES = ('a', 'b', 'c', 'd')
NITER = rc.NITER
# cp / R on a non-uniform grid: He constant, the others rising smoothly with temperature
CP_TEMPS = np.array([100.0, 200.0, 300.0, 450.0, 600.0, 800.0, 1000.0, 1300.0, 1700.0, 2200.0,
                     3000.0, 4000.0])


def cp_table(kind='gas'):
    """cp / R [nT, S] of radeq_cases.SPECIES: 'gas' (H2 3.5-4.5, He 2.5, H2O 4-6.5, CO 3.5-4.5),
    'stiff' (1.05 for every species: grad_ad = 0.95, nothing convects), or a number (that value
    for every species)."""
    x = CP_TEMPS / (CP_TEMPS + 1500.0)
    if kind == 'gas':
        return np.stack([3.5 + 1.0 * x, np.full_like(x, 2.5), 4.0 + 2.5 * x, 3.5 + 1.0 * x], axis=1)
    value = 1.05 if kind == 'stiff' else float(kind)
    return np.full((len(CP_TEMPS), len(rc.SPECIES)), value)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(rc.GOLDEN, 'g26_radeq_convection.npz'))


def unpack(store, name):
    c = rc.unpack(store, name)
    c['cp_temps'] = np.asarray(store[f'{name}_cp_temps'])
    c['cp_table'] = np.asarray(store[f'{name}_cp_table'])
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return unpack(fixture(), name)


def build(eng, c, **kw):
    """(TableSpectrum, RadiativeEquilibrium) of a case with its heat capacities and mplanet."""
    table = c['cp_table'] if c['nw'] > 1 else c['cp_table'][0]
    args = dict(heat_capacity=(c['cp_temps'], table), mplanet=c['mplanet'])
    args.update(kw)
    return rc.build(eng, c, **args)


def host_step(c, w, temp, dt_scale, signs, qup, qdown):
    """radeq.step_convective_host on profile w of case c at `temp`, with the radius of that
    profile (the host atmosphere of radeq_cases) and dpress from the pressure in barye, as the
    reference forms it (its bits differ from those of the pressure in bar, and a layer close to
    the switch grad_t = grad_ad magnifies a last bit of the temperatures in conv_flux)."""
    from pyratbay_amd import radeq
    vmr = c['vmr'][w] if c['vmr'].ndim == 3 else c['vmr']
    radius = rc.host_atmosphere(c, temp, w)[1]
    return radeq.step_convective_host(
        temp, dt_scale, signs, qup, qdown, radeq.log_pressure_steps(c['pressure'] * 1e6),
        c['pressure'], vmr, c['mol_mass'], radius, c['cp_temps'], c['cp_table'][w], c['mplanet'],
        tmin=c['tmin'], tmax=c['tmax'])


def replay(c, w, fx=None, prefix=None, restart=None):
    """host_step along the recorded trajectory of profile w: per iteration the step's dict, from
    the recorded temperatures, dt_scale and fluxes of that iteration.  restart: the iteration at
    which the sign history starts afresh."""
    from pyratbay_amd import radeq
    fx = fixture() if fx is None else fx
    pre = c['name'] if prefix is None else prefix
    temps, dts = fx[f'{pre}_temps'][w], fx[f'{pre}_dt_scale'][w]
    qup, qdown = fx[f'{pre}_qup'][w], fx[f'{pre}_qdown'][w]
    signs, out = np.zeros((0, c['L'])), []
    for k in range(len(qup)):
        if k == restart:
            signs = np.zeros((0, c['L']))
        s = host_step(c, w, temps[k], dts[k - 1] if k else np.full(c['L'], radeq.DT_SCALE0), signs,
                      qup[k], qdown[k])
        signs = np.vstack([signs, s['sign']])
        out.append(s)
    return out


def gradients(c, w, temp_next):
    """(grad_t, grad_ad) [L] of convection.py:49-55 at the temperatures temp_next of profile w."""
    from pyratbay_amd import atmosphere as pa, radeq
    vmr = c['vmr'][w] if c['vmr'].ndim == 3 else c['vmr']
    cp = np.sum(radeq.heat_capacity_host(c['cp_temps'], c['cp_table'][w], temp_next) * vmr,
                axis=1) * pa.K_BOLTZ / radeq.AMU
    dpress = np.ediff1d(np.log(c['pressure'] * 1e6), to_begin=1.0)
    grad_t = np.ediff1d(np.log(temp_next), to_begin=0.0) / dpress
    return grad_t, 1.0 - (cp - pa.K_BOLTZ / radeq.AMU) / cp


# ------------------------------------------------------------------ the update kernel on its own
def update_on_device(eng, s):
    """One pb_radeq_update_convective on the state s of radeq_cases.update_on_device plus radius
    [nw, L] (on entry), cp_temps, cp_table ([nT, S] or [nw, nT, S]), mplanet, alpha, beta -> dict
    of host arrays.  Every output is pre-filled with NaN / -1, the radius and intervals of a fixed
    radius model included."""
    import ctypes as C
    import torch
    from pyratbay_amd import _capi, radeq
    nw, P, _, L = s['parts'].shape
    k = s['signs'].shape[1]
    vmr = np.asarray(s['vmr'], float)
    S = vmr.shape[-1]

    def nan(*shape):
        return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
    ring = np.full((nw, 4, L), np.nan)
    for it in range(max(k - 4, 0), k):
        ring[:, it % 4] = s['signs'][:, it]
    cp_table = np.asarray(s['cp_table'], float)
    t = dict(parts=eng.dev(s['parts']), dpress=eng.dev(radeq.log_pressure_steps(s['pressure'])),
             temps=nan(nw, k + 2, L), temp=eng.dev(s['temp']), dt_scale=eng.dev(s['dt_scale']),
             signs=eng.dev(ring), iter=torch.full((nw,), k, dtype=torch.int32, device='cuda'),
             q_up=nan(nw, L), q_down=nan(nw, L),
             wobble=torch.full((nw, L), -1, dtype=torch.int32, device='cuda'), sigma=nan(nw),
             pressure=eng.dev(s['pressure']), lnp=eng.dev(np.log(s['pressure'])),
             vmr=eng.dev(vmr), mm=eng.dev(np.sum(vmr * np.array(rc.MASS), axis=-1)),
             tab_map=eng.dev(s['tab_map'], torch.int32),
             cont_map=eng.dev(s['cont_map'] or [0], torch.int32),
             dens=nan(nw, L, len(s['tab_map'])), cdens=nan(nw, L, max(len(s['cont_map']), 1)),
             radius=eng.dev(s['radius']), intervals=nan(nw, L - 1),
             cp_temps=eng.dev(s['cp_temps']), cp_table=eng.dev(cp_table),
             mol_mass=eng.dev(np.array(rc.MASS)),
             conv_dpress=eng.dev(np.ediff1d(np.log(s['pressure'] * 1e6), to_begin=1.0)),
             conv_flux=nan(nw, L),
             convective=torch.full((nw,), -1, dtype=torch.int32, device='cuda'))
    st = radeq.RadeqStruct()
    st.nlayers, st.nwalkers, st.nparts, st.nrows = L, nw, P, k + 2
    st.tmin, st.tmax = s['tmin'], s['tmax']
    for name in ('parts', 'dpress', 'temps', 'temp', 'dt_scale', 'signs', 'iter', 'q_up',
                 'q_down', 'wobble', 'sigma', 'pressure', 'lnp', 'vmr', 'mm', 'tab_map', 'dens',
                 'radius', 'intervals'):
        setattr(st, name + '_d', t[name].data_ptr())
    st.vmr_stride, st.nspecies = (L * S if vmr.ndim == 3 else 0), S
    st.mm_stride = L if vmr.ndim == 3 else 0
    st.ntab, st.ncont = len(s['tab_map']), len(s['cont_map'])
    if s['cont_map']:
        st.cont_map_d, st.cdens_d = t['cont_map'].data_ptr(), t['cdens'].data_ptr()
    kw = s['radius_kwargs']
    st.rmodel = radeq.RMODELS[kw['radius_model']]
    st.has_ref = int(kw.get('p0') is not None)
    st.mplanet, st.gplanet = float(kw.get('mplanet') or 0.0), float(kw.get('gravity') or 0.0)
    st.p0, st.r0 = float(kw.get('p0') or 0.0), float(kw.get('r0') or 0.0)
    cv = radeq.ConvectionStruct()
    for name in ('cp_temps', 'cp_table', 'mol_mass', 'conv_dpress', 'conv_flux', 'convective'):
        setattr(cv, name + '_d', t[name].data_ptr())
    cv.cp_table_stride = cp_table.shape[1] * S if cp_table.ndim == 3 else 0
    cv.ntemps = len(s['cp_temps'])
    cv.mplanet = float(s['mplanet'])
    cv.coeff = float(s['alpha']**2 * np.sqrt(s['beta']))
    _capi.call('pb_radeq_update_convective', C.byref(st), C.byref(cv), eng._stream())
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in t.items()}


def update_on_host(s, w, temp_factor=None):
    """Profile w of the same state through radeq.step_convective_host and the host atmosphere.
    temp_factor[L]: factors on the temperatures the convective flux is evaluated at (for the
    sensitivity of conv_flux to the last bits of those temperatures); only conv_flux of the
    result means anything then."""
    from pyratbay_amd import radeq
    qup, qdown = rc.sum_parts(s['parts'])
    vmr = np.asarray(s['vmr'], float)
    vmr = vmr[w] if vmr.ndim == 3 else vmr
    table = np.asarray(s['cp_table'], float)
    table = table[w] if table.ndim == 3 else table
    dpress = radeq.log_pressure_steps(s['pressure'])
    args = (s['pressure'], vmr, np.array(rc.MASS), s['radius'][w], s['cp_temps'], table,
            s['mplanet'], s['alpha'], s['beta'], s['tmin'], s['tmax'])
    step = radeq.step_convective_host(s['temp'][w], s['dt_scale'][w], s['signs'][w], qup[w],
                                      qdown[w], dpress, *args)
    if temp_factor is not None:
        from pyratbay_amd import atmosphere as pa
        tn = step['radiative']['temp'] * temp_factor
        cp = np.sum(radeq.heat_capacity_host(s['cp_temps'], table, tn) * vmr, axis=1) \
            * pa.K_BOLTZ / radeq.AMU
        g = pa.G_GRAV * s['mplanet'] / s['radius'][w]**2.0
        rho = np.sum(pa.ideal_gas_density(vmr, s['pressure'], s['temp'][w]) * np.array(rc.MASS),
                     axis=1) * radeq.AMU
        return dict(conv_flux=radeq.convective_flux_host(
            s['pressure'] * 1e6, tn, cp, g, pa.mean_weight(vmr, mass=np.array(rc.MASS)), rho,
            s['alpha'], s['beta']))
    dens, radius = radeq.atmosphere_host(step['temp'], s['pressure'], vmr, np.array(rc.MASS),
                                         **s['radius_kwargs'])
    step.update(q_up=qup[w], q_down=qdown[w], dens=dens, radius=radius)
    return step
