"""Helpers of the radiative-equilibrium tests (test_radeq_cpu.py, test_gpu_two_stream_net.py,
test_gpu_radeq_update.py, test_gpu_radeq.py) and of tests/golden/make_golden_radeq.py: the
fixture's cases as dicts, and the host chain -- atmosphere from pyratbay_amd's host forms, then
the oracle's interp_ec, plane_parallel_optical_depth(maxdepth = inf) and two_stream -- that stands
for the reference's two_stream_rt.

The opacity table of a case is stored as its two factors (a[S, ntemp, L] b[S, W]: 2 MB otherwise)
and formed here, by the generator and the tests alike."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('a', 'b', 'c', 'd', 'e')
NITER = 8
SPECIES = ['H2', 'He', 'H2O', 'CO']
MASS = [2.01588, 4.002602, 18.01528, 28.0101]
TABLE_SPECIES = ['H2O', 'CO']
CIA = (('h2h2', ['H2', 'H2']), ('h2he', ['H2', 'He']))
KEYS = ('pressure', 'wn', 'ttable', 'tab_a', 'tab_b', 'vmr', 'temp0', 'tint', 'flux_top', 'radius',
        'scalars', 'cia_idx')


def table(tab_a, tab_b):
    """etable[S, ntemp, L, W] from its stored factors."""
    return np.ascontiguousarray(tab_a[:, :, :, None] * tab_b[:, None, None, :])


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, 'g23_radeq.npz'))


@functools.lru_cache(maxsize=None)
def g7():
    return np.load(os.path.join(GOLDEN, 'g7_continuum.npz'))


def unpack(store, name):
    """The inputs of case `name` out of an archive (or the generator's dict)."""
    c = {k: np.asarray(store[f'{name}_{k}']) for k in KEYS if f'{name}_{k}' in store}
    rmodel, gravity, mplanet, p0, r0, tmin, tmax, continuum = c.pop('scalars')
    c['radius_model'] = {0.0: None, 1.0: 'hydro_g', 2.0: 'hydro_m'}[float(rmodel)]
    c['gravity'], c['mplanet'] = float(gravity), float(mplanet)
    c['p0'], c['r0'] = float(p0), float(r0)
    c['tmin'], c['tmax'] = float(tmin), float(tmax)
    c['continuum'] = bool(continuum)
    c['etable'] = table(c['tab_a'], c['tab_b'])
    c['name'] = name
    c['nw'] = c['temp0'].shape[0]
    c['L'], c['W'] = len(c['pressure']), len(c['wn'])
    c['mol_mass'] = np.array(MASS)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return unpack(fixture(), name)


def pack_scalars(radius_model, gravity, mplanet, p0, r0, tmin, tmax, continuum):
    return np.array([{None: 0.0, 'hydro_g': 1.0, 'hydro_m': 2.0}[radius_model], gravity, mplanet,
                     p0, r0, tmin, tmax, float(continuum)])


def radius_kwargs(c):
    """The radius-model keywords of RadiativeEquilibrium / radeq.atmosphere_host."""
    if c['radius_model'] == 'hydro_g':
        return dict(radius_model='hydro_g', gravity=c['gravity'], p0=c['p0'], r0=c['r0'])
    if c['radius_model'] == 'hydro_m':
        return dict(radius_model='hydro_m', mplanet=c['mplanet'], p0=c['p0'], r0=c['r0'])
    return dict(radius_model=None)


def cia_tables(c):
    """[(species, tab[ntemp, W], temps, lo, hi)] of fixture G7 on the case's grid, which is G7's
    grid at the indices cia_idx (all inside both tables' wavenumber ranges)."""
    g, idx = g7(), c['cia_idx']
    out = []
    for tag, species in CIA:
        lo, hi = (int(v) for v in g[f'cia_{tag}_lohi'])
        assert lo <= idx.min() and idx.max() < hi
        out.append((species, np.ascontiguousarray(g[f'cia_{tag}_tab'][:, idx]),
                    g[f'cia_{tag}_temps'], 0, len(idx)))
    return out


def host_atmosphere(c, temp, w=0):
    """(density[L, S], radius[L]) of profile w at `temp` from pyratbay_amd.atmosphere's host forms."""
    from pyratbay_amd import radeq
    vmr = c['vmr'][w] if c['vmr'].ndim == 3 else c['vmr']
    dens, radius = radeq.atmosphere_host(temp, c['pressure'], vmr, c['mol_mass'],
                                         **radius_kwargs(c))
    return dens, (c['radius'] if radius is None else radius)


def host_extinction(orc, c, temp, dens):
    from oracle import continuum as oc
    L, W = c['L'], c['W']
    ec = np.zeros((L, W))
    itab = [SPECIES.index(s) for s in TABLE_SPECIES]
    orc.interp_ec(ec, c['etable'], c['ttable'], np.ascontiguousarray(temp),
                  np.ascontiguousarray(dens[:, itab]), 0, L)
    if c['continuum']:
        d = {s: dens[:, i] for i, s in enumerate(SPECIES)}
        for s in ('H2', 'He'):
            ec += oc.rayleigh_cross_section(c['wn'], s) * d[s][:, None]
        for species, tab, temps, lo, hi in cia_tables(c):
            cs = oc.cia_cross_section(tab, temps, temp, lo, hi)
            ec += cs * (d[species[0]] * d[species[1]])[:, None]
    return ec


def host_fluxes(orc, c, temp, w=0):
    """(flux_down, flux_up) [L, W] of profile w of case c at `temp`: what the reference's
    two_stream_rt leaves in spec.flux_down / spec.flux_up."""
    L, W = c['L'], c['W']
    dens, radius = host_atmosphere(c, temp, w)
    ec = host_extinction(orc, c, temp, dens)
    depth = np.zeros((L, W))
    stop = np.zeros(W, np.int32)
    orc.plane_parallel_optical_depth(depth, stop, ec, np.ascontiguousarray(-np.diff(radius)),
                                     np.inf, 0, L)
    f_int = orc.internal_flux(c['wn'], float(c['tint'][w]))
    top = None if c['flux_top'].size == 0 else np.ascontiguousarray(c['flux_top'][w])
    return orc.two_stream(depth, c['wn'], temp, f_int, top, 0)


def continuum_models(c):
    """The Continuum of a case with continuum terms (needs a GPU): Rayleigh H2 + He, CIA H2-H2 +
    H2-He from fixture G7 on the case's grid."""
    from pyratbay_amd import continuum as ct
    models = [ct.Kurucz(c['wn'], 'H2'), ct.Kurucz(c['wn'], 'He')]
    for species, tab, temps, lo, hi in cia_tables(c):
        m = ct.Collision_Induced.__new__(ct.Collision_Induced)
        m.species, m.nspec = species, 2
        m.name = 'CIA ' + '-'.join(species)
        m.tab_cross_section, m.temps = tab, temps
        m.ntemp, m.tmin, m.tmax = len(temps), temps.min(), temps.max()
        m._wn_lo_idx, m._wn_hi_idx = lo, hi
        models.append(m)
    return ct.Continuum(c['wn'], c['pressure'], models)


def build(eng, c, **kw):
    """(TableSpectrum, RadiativeEquilibrium) of a case on the device."""
    from pyratbay_amd import radeq
    cont = continuum_models(c) if c['continuum'] else None
    model = eng.TableSpectrum(c['etable'], c['ttable'], c['wn'], c['radius'], 1.0,
                              rt_path='emission_two_stream', continuum=cont, timestamps=False,
                              tint=float(c['tint'][0]),
                              flux_top=None if c['flux_top'].size == 0 else c['flux_top'][0])
    args = dict(tint=c['tint'] if c['nw'] > 1 else float(c['tint'][0]),
                flux_top=None if c['flux_top'].size == 0 else
                (c['flux_top'] if c['nw'] > 1 else c['flux_top'][0]),
                tmin=c['tmin'], tmax=c['tmax'], species=SPECIES, table_species=TABLE_SPECIES)
    args.update(radius_kwargs(c))
    args.update(kw)
    return model, radeq.RadiativeEquilibrium(model, c['pressure'], c['vmr'], c['mol_mass'], **args)


# ------------------------------------------------------------------ the update kernel on its own
def sum_parts(parts, threads=256):
    """(Qup, Qdown) [nw, L] of parts[nw, nparts, 2, L] in k_radeq_update's order (pbhip.h): up to
    threads / L groups of consecutive parts, each added left to right, then the groups."""
    nw, P, _, L = parts.shape
    groups = max(min(threads // L, P), 1) if L <= threads else 1
    chunk = -(-P // groups)
    q = np.zeros((nw, 2, L))
    for g in range(groups):
        c = np.zeros((nw, 2, L))
        for p in range(g * chunk, min((g + 1) * chunk, P)):
            c = c + parts[:, p]
        q = q + c
    return q[:, 0], q[:, 1]


def update_on_device(eng, s, init_only=False):
    """One pb_radeq_update on the state s: parts[nw, P, 2, L], temp[nw, L], dt_scale[nw, L],
    signs[nw, k, L] (the sign rows of iterations 0 .. k-1), pressure[L], vmr ([L, S] or
    [nw, L, S]), tab_map, cont_map, tmin, tmax and radius_kwargs -> dict of host arrays.  The
    history has nrows = k + 2 rows, pre-filled with NaN like every other output."""
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
    t = dict(parts=eng.dev(s['parts']), dpress=eng.dev(radeq.log_pressure_steps(s['pressure'])),
             temps=nan(nw, k + 2, L), temp=eng.dev(s['temp']), dt_scale=eng.dev(s['dt_scale']),
             signs=eng.dev(ring), iter=torch.full((nw,), k, dtype=torch.int32, device='cuda'),
             q_up=nan(nw, L), q_down=nan(nw, L),
             wobble=torch.full((nw, L), -1, dtype=torch.int32, device='cuda'), sigma=nan(nw),
             pressure=eng.dev(s['pressure']), lnp=eng.dev(np.log(s['pressure'])),
             vmr=eng.dev(vmr), mm=eng.dev(np.sum(vmr * np.array(MASS), axis=-1)),
             tab_map=eng.dev(s['tab_map'], torch.int32),
             cont_map=eng.dev(s['cont_map'] or [0], torch.int32),
             dens=nan(nw, L, len(s['tab_map'])), cdens=nan(nw, L, max(len(s['cont_map']), 1)),
             radius=nan(nw, L), intervals=nan(nw, L - 1))
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
    _capi.call('pb_radeq_update', C.byref(st), int(init_only), eng._stream())
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in t.items()}


def update_on_host(s, w):
    """Profile w of the same state through radeq.step_host and the host atmosphere."""
    from pyratbay_amd import radeq
    qup, qdown = sum_parts(s['parts'])
    step = radeq.step_host(s['temp'][w], s['dt_scale'][w], s['signs'][w], qup[w], qdown[w],
                           radeq.log_pressure_steps(s['pressure']), s['tmin'], s['tmax'])
    vmr = np.asarray(s['vmr'], float)
    dens, radius = radeq.atmosphere_host(step['temp'], s['pressure'],
                                         vmr[w] if vmr.ndim == 3 else vmr, np.array(MASS),
                                         **s['radius_kwargs'])
    step.update(q_up=qup[w], q_down=qdown[w], dens=dens, radius=radius)
    return step
