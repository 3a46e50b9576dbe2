"""Radiative equilibrium on the device: runmode = radeq of the reference
(Pyrat.radiative_equilibrium, pyrat/pyrat_obj.py:559-646 -> ps.radiative_equilibrium,
spectrum/radiative_transfer.py:141-272) for a batch of profiles.

One iteration evaluates the two-stream fluxes of every layer, integrates them over wavenumber to
the bolometric Qup and Qdown, and moves each layer's temperature by an adaptive step along the
sign of the net-flux divergence.  Here that is three launches per iteration and nothing read back:
the interpolation of the table (with the Continuum's terms when one is attached),
pb_two_stream_net_batch (the two-stream batch kernel that also reduces t_j flux[i][j] over its
columns) and pb_radeq_update (the update and the atmosphere of the next iteration): csrc/pb_radeq.hip.
With run(convection=True) the third launch is pb_radeq_update_convective: the same update, the
mixing-length convective flux (spectrum/convection.py:13-67) at the temperatures it produced and,
for a profile with a superadiabatic layer, the update again with that flux added to the net flux
(radiative_transfer.py:239-272).

With RadiativeEquilibrium(chemistry=ChemNetwork) the loop is the reference's radiative-
thermochemical equilibrium (chem_model.thermochemical_equilibrium(temp) at the top of every
iteration, radiative_transfer.py:202-203): five launches per iteration, still nothing read back.
The update runs with pb_radeq.temps_only and stops behind the new temperatures;
pb_radeq_equilibrium (csrc/pb_chemistry.hip) solves the gas-phase equilibrium of every layer there,
by default from the iterate the previous iteration left (chemistry_start='previous'), and writes the
mean mass; pb_radeq_update(init_only=1) forms densities, radius and intervals from them.  The
convective half reads the VMRs, mean mass and radius of the evaluated profile, as the reference
does.

Deviations from the reference:
  * without chemistry= the volume mixing ratios are FIXED (the reference calls chemcat's
    thermochemical equilibrium every iteration); the mean molecular mass is then constant;
  * with chemistry= the equilibrium is this package's own solver on the caller's table of G°/RT
    (chemistry.py), not chemcat; a layer whose solve fails (a temperature outside the Gibbs table,
    no convergence) KEEPS the VMRs and mean mass of the iteration before and counts in
    .chem_failures -- zeros would silently empty the layer of the next evaluation;
  * the heat capacities of the convective half are np.interp on the caller's table of cp / R per
    species (the reference asks chemcat's chem_model.heat_capacity);
  * in the reference the convective branch's in-place dt_scale[wobble] *= 0.5 followed by the
    rebinding dt_scale = gaussf(...) leaves atm._dt_scale stale for a later continue_run; here a
    continued run goes on from the dt_scale the loop itself was using;
  * continue_run starts a fresh sign history (what a second call of the reference's function with
    radeq_temps = atleast_2d(last row) does; with a longer history its df_sign index runs out of
    bounds);
  * the wavenumber integral is sum_j t_j flux_j with the trapezoid weights t_j, summed per
    wavefront of 64 columns and then over the wavefronts in order; np.trapezoid sums pairwise.

step_host is the NumPy form of one update under the reference's names, step_convective_host that
of an update with convection; convective_flux_host and heat_capacity_host are its two parts.
"""
import ctypes as C

import numpy as np

from . import _capi, atmosphere as pa
from ._device import _ptr, _stream, dev, require_gpu
from .batch import interp_ec_batch
from .columns import internal_flux

SIGMA_SB = 5.6703744191844314e-08 * 1e3     # pc.sigma = sc.sigma * 1e3 (erg s-1 cm-2 K-4)
MAXF = 1.0e08                               # maximum temperature scale factor
DT_SCALE0 = 1.0e5                           # dt_scale of a fresh run (pyrat_obj.py:605-606)
RMODELS = {None: -1, 'hydro_m': 0, 'hydro_g': 1}
MAX_LAYERS = 744                            # 64 KiB of LDS / (11 doubles per layer): pb_radeq.hip
# with convection: pb_radeq_update_convective keeps 8 vectors per profile in LDS and takes
# (8192 - 17 - 512) // 8 = 957 layers; the net-flux kernel of the same iteration still takes 744
MAX_LAYERS_CONVECTION = min(MAX_LAYERS, 957)
AMU = 1.66053906892e-27 * 1e3               # pc.amu = sc 'unified atomic mass unit' * 1e3 (g)


# ---------------------------------------------------------------------------------------------
# Host forms
# ---------------------------------------------------------------------------------------------
def trapezoid_weights(wn):
    """t[W] with sum(t * y) = np.trapezoid(y, wn) in exact arithmetic: half the neighbouring gaps,
    one-sided at the ends (any grid, uniform or not); a single sample has weight 0."""
    wn = np.asarray(wn, float)
    t = np.zeros(len(wn))
    if len(wn) > 1:
        gaps = np.diff(wn)
        t[0], t[-1] = gaps[0] / 2.0, gaps[-1] / 2.0
        t[1:-1] = (wn[2:] - wn[:-2]) / 2.0
    return t


def gaussian_filter1d(values, sigma):
    """scipy.ndimage.gaussian_filter1d(values, sigma) (truncate = 4, mode = 'reflect') in its order
    of operations: the weights of atmosphere.gaussian_weights, the centre tap, then the pairs from
    the outermost inwards; the line is extended d c b a | a b c d | d c b a as often as needed."""
    values = np.asarray(values, float)
    weights = pa.gaussian_weights(float(sigma))
    n, radius = len(values), (len(weights) - 1) // 2
    idx = np.arange(n)

    def reflect(i):
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    out = values * weights[radius]
    for k in range(-radius, 0):
        out = out + (values[reflect(idx + k)] + values[reflect(idx - k)]) * weights[k + radius]
    return out


def step_host(temp, dt_scale, df_sign, Qup, Qdown, dpress, tmin=0.0, tmax=6000.0):
    """One update of radiative_transfer.py:207-237 (convection=False).  temp[L], dt_scale[L] of
    this iteration; df_sign: the sign rows of the up to four previous iterations ([n, L], n = 0 at
    the first one; only the last four are read); Qup, Qdown [L]; dpress = ediff1d(log p) with
    element 0 = element 1.  Returns a dict: temp (the next profile), dt_scale, sign, wobble, dF,
    dT, sigma."""
    temp, dt_scale = np.asarray(temp, float), np.asarray(dt_scale, float)
    df_sign = np.asarray(df_sign, float).reshape(-1, len(temp))[-4:]
    Q_net = np.asarray(Qup, float) - np.asarray(Qdown, float)
    dF = np.ediff1d(Q_net, to_begin=0)
    sign = np.sign(dF)
    wobble = np.any(df_sign - sign, axis=0)
    dt_scale_tmp = np.copy(dt_scale)
    dt_scale_tmp[wobble] *= 0.5
    dt_scale_tmp[~wobble] *= 1.15
    dt_scale_tmp = gaussian_filter1d(np.clip(dt_scale_tmp, 1.0, MAXF), 1.5)
    dT = dt_scale_tmp * np.sign(dF) * np.abs(dF)**0.1 / (SIGMA_SB * temp**3 * dpress)
    new = temp + dT
    new[0] = new[1]                                  # isothermal top
    avg_dT = np.mean(np.abs(dT))
    sigma = np.clip(avg_dT / 10.0, 0.75, 2.0)
    new[:-1] = gaussian_filter1d(new, sigma)[:-1]
    new = np.clip(new, tmin, tmax)
    return dict(temp=new, dt_scale=dt_scale_tmp, sign=sign, wobble=wobble, dF=dF, dT=dT,
                sigma=float(sigma))


def convective_flux_host(pressure_barye, temperature, cp, gravity, mu, rho, alpha=1.5, beta=0.5):
    """convection.convective_flux (spectrum/convection.py:13-67) in its order of operations: the
    mixing-length flux [L] (erg s-1 cm-2), zero where grad_t <= grad_ad.  Its own dpress keeps
    element 0 = 1 (unlike log_pressure_steps), so grad_t[0] = 0."""
    temperature, cp = np.asarray(temperature, float), np.asarray(cp, float)
    dpress = np.ediff1d(np.log(np.asarray(pressure_barye, float)), to_begin=1.0)
    grad_t = np.ediff1d(np.log(temperature), to_begin=0.0) / dpress
    cv = cp - pa.K_BOLTZ / AMU
    gamma = cp / cv
    grad_ad = 1.0 - 1.0 / gamma
    delta_grad = np.clip(grad_t - grad_ad, 0, np.inf)
    H = pa.K_BOLTZ * temperature / (mu * AMU * gravity)
    return (alpha**2 * np.sqrt(beta) * cp / mu * rho * temperature * np.sqrt(gravity * H)
            * delta_grad**1.5)


def heat_capacity_host(cp_temps, cp_table, temp):
    """cp / R [L, S] of the S species at temp[L]: np.interp per column of cp_table[nT, S] on
    cp_temps[nT], the end values outside the table -- the stand-in for chemcat's
    chem_model.heat_capacity."""
    cp_table = np.asarray(cp_table, float)
    return np.stack([np.interp(temp, cp_temps, cp_table[:, s]) for s in range(cp_table.shape[1])],
                    axis=1)


def step_convective_host(temp, dt_scale, df_sign, Qup, Qdown, dpress, pressure, vmr, mol_mass,
                         radius, cp_temps, cp_table, mplanet, alpha=1.5, beta=0.5, tmin=0.0,
                         tmax=6000.0):
    """step_host followed by radiative_transfer.py:239-272 (convection=True).  Beyond step_host's
    arguments: pressure[L] (bar), vmr[L, S], mol_mass[S], radius[L] (that of the evaluation the
    fluxes come from, like temp), the heat-capacity table and mplanet (g).  Returns step_host's
    dict of the update that stands, plus conv_flux[L], convective (whether the second half ran)
    and radiative (the radiative half's dict)."""
    temp, dt_scale = np.asarray(temp, float), np.asarray(dt_scale, float)
    vmr, mol_mass = np.asarray(vmr, float), np.asarray(mol_mass, float)
    first = step_host(temp, dt_scale, df_sign, Qup, Qdown, dpress, tmin, tmax)
    heat_capacity = heat_capacity_host(cp_temps, cp_table, first['temp'])
    cp = np.sum(heat_capacity * vmr, axis=1) * pa.K_BOLTZ / AMU
    gplanet = pa.G_GRAV * mplanet / np.asarray(radius, float)**2.0
    d = pa.ideal_gas_density(vmr, pressure, temp)
    rho = np.sum(d * mol_mass, axis=1) * AMU
    mm = pa.mean_weight(vmr, mass=mol_mass)
    conv_flux = convective_flux_host(np.asarray(pressure, float) * pa.BAR, first['temp'], cp,
                                     gplanet, mm, rho, alpha, beta)
    if np.all(conv_flux == 0.0):
        return dict(first, conv_flux=conv_flux, convective=False, radiative=first)
    # the update again with the convective flux: the new signs replace this iteration's row, the
    # factors apply to the dt_scale of the start of the iteration
    Q_net = np.asarray(Qup, float) - np.asarray(Qdown, float)
    second = step_host(temp, dt_scale, df_sign, Q_net + conv_flux, 0.0, dpress, tmin, tmax)
    return dict(second, conv_flux=conv_flux, convective=True, radiative=first)


def log_pressure_steps(pressure):
    """dpress of radiative_transfer.py:188-189."""
    dpress = np.ediff1d(np.log(np.asarray(pressure, float)), to_begin=1.0)
    dpress[0] = dpress[1]
    return dpress


def atmosphere_host(temp, pressure, vmr, mol_mass, radius_model=None, gravity=None, mplanet=None,
                    p0=None, r0=None):
    """(density[L, S], radius[L] or None) of one profile from atmosphere's host forms, as the
    update kernel makes them: ideal_gas_density, then hydro_g / hydro_m with the mean mass of
    the fixed VMR."""
    dens = pa.ideal_gas_density(vmr, pressure, temp)
    if radius_model is None:
        return dens, None
    mu = pa.mean_weight(vmr, mass=mol_mass)
    if radius_model == 'hydro_g':
        return dens, pa.hydro_g(pressure, temp, mu, gravity, p0, r0)
    return dens, pa.hydro_m(pressure, temp, mu, mplanet, p0, r0)


# ---------------------------------------------------------------------------------------------
# The device forms
# ---------------------------------------------------------------------------------------------
RadeqStruct = _capi.struct('pb_radeq')
ConvectionStruct = _capi.struct('pb_radeq_convection')


def net_parts(nwave):
    """Number of parts pb_two_stream_net_batch writes per (profile, direction, layer)."""
    return int(_capi.lib().pb_two_stream_net_parts(int(nwave)))


def two_stream_net_batch(ec, intervals, wn, trapz_weights, temps, f_int=None, flux_top=None,
                         out=None, parts=None, work=None):
    """batch.two_stream_batch that also integrates every layer's fluxes over wavenumber:
    ec[nw, L, W] (consumed), intervals[nw, L - 1], wn[W], trapz_weights[W]
    (trapezoid_weights(wn)), temps[nw, L]; f_int / flux_top: [W] shared by the profiles,
    [nw, W] per profile, or None.  Returns (flux_up[0] [nw, W], parts[nw, nparts, 2, L]): summed
    over the parts in order, parts[:, :, 0] is Qup and parts[:, :, 1] Qdown
    (pb_two_stream_net_batch).  Device tensors; out, parts and work (at least
    pb_two_stream_net_work_doubles(L, W, nw) doubles) are allocated here when None."""
    import torch
    nw, nlayers, nwave = ec.shape
    assert ec.is_contiguous() and temps.shape == (nw, nlayers)
    assert nlayers == 1 or intervals.shape == (nw, nlayers - 1)
    assert wn.shape == (nwave,) and trapz_weights.shape == (nwave,)

    def stride(name, t):
        if t is None or tuple(t.shape) == (nwave,):
            return 0
        if tuple(t.shape) != (nw, nwave):
            raise ValueError(f'two_stream_net_batch: {name} must have shape ({nwave},) or '
                             f'({nw}, {nwave}), got {tuple(t.shape)}')
        return nwave
    fs, ts = stride('f_int', f_int), stride('flux_top', flux_top)
    npart = net_parts(nwave)
    if out is None:
        out = torch.empty((nw, nwave), dtype=torch.float64, device=ec.device)
    if parts is None:
        parts = torch.empty((nw, npart, 2, nlayers), dtype=torch.float64, device=ec.device)
    if tuple(parts.shape) != (nw, npart, 2, nlayers) or not parts.is_contiguous():
        raise ValueError(f'two_stream_net_batch: parts must be contiguous of shape '
                         f'{(nw, npart, 2, nlayers)}')
    need = _capi.lib().pb_two_stream_net_work_doubles(nlayers, nwave, nw)
    if work is None:
        work = torch.empty(max(need, 1), dtype=torch.float64, device=ec.device)
    if work.numel() < need or not work.is_contiguous():
        raise ValueError(f'two_stream_net_batch: work must hold {need} contiguous doubles')
    _capi.call('pb_two_stream_net_batch', _ptr(out), _ptr(parts), _ptr(ec),
               _ptr(intervals.contiguous()), _ptr(wn), _ptr(trapz_weights), _ptr(temps.contiguous()),
               _ptr(None if f_int is None else f_int.contiguous()), fs,
               _ptr(None if flux_top is None else flux_top.contiguous()), ts, _ptr(work),
               nlayers, nwave, nw, _stream())
    return out, parts


def _check(cond, text):
    if not cond:
        raise ValueError('RadiativeEquilibrium: ' + text)


class RadiativeEquilibrium:
    """Radiative-equilibrium iteration of nw profiles at fixed volume mixing ratios, or
    (chemistry=) at the gas-phase equilibrium of every iteration's temperatures.

    spectrum: a TableSpectrum in a two-stream rt_path (its table, grid and Continuum);
    pressure[L] (bar, ascending); vmr[L, S] or [nw, L, S]; mol_mass[S] (g mol-1).
    species (names of the S columns of vmr) and table_species (the names of the table's species in
    its order) say which columns feed the table and the Continuum; without them the table takes
    the first columns of vmr, and a Continuum needs them.
    radius_model: None (the spectrum's radius stays), 'hydro_g' (gravity, cm s-2; p0 in bar and
    r0 in cm, or neither: radius 0 at the bottom) or 'hydro_m' (mplanet in g, p0, r0).
    tint: internal temperature (K), a scalar or [nw]; flux_top: the irradiation at the top, [W],
    [nw, W] or None.  tmin / tmax: the bounds the new temperatures are clipped to; default the
    intersection of the table's and the CIA tables' ranges.
    heat_capacity: (cp_temps[nT] ascending, cp_over_R[nT, S] or [nw, nT, S]), cp / R > 1 of every
    column of vmr, read by np.interp (the end values outside the table); mixing_length: (alpha,
    beta) of convection.convective_flux.  Both are read only by run(convection=True), which also
    needs mplanet (the gravity is G mplanet / radius**2 whatever the radius model).
    chemistry: a chemistry.ChemNetwork -- the VMRs of every iteration are its gas-phase equilibrium
    at that iteration's temperatures.  vmr must then be None, the species are the network's
    (mol_mass[S] and heat_capacity cover them; table_species and the Continuum's species must be
    among them), and the default tmin / tmax are also cut to the Gibbs table's range.  metallicity
    ([M/H]), e_scale ({'C': [C/H]}) and e_ratio ({'C/O': value}) are the abundances by the rule of
    ChemNetwork.element_abundances_host, each value a scalar or [nw], fixed over a run.
    chemistry_start: 'previous' (a layer's solve starts from the iterate of the iteration before)
    or 'cold' (every solve from the cold start; the same VMRs to the solver's convergence).
    After run(): .vmr[nw, L, S] and .mean_mass[nw, L] of the last row temps[:, -1] (like .radius),
    .chem_status[nw, L] of the last solve, and .chem_failures[nw, L], the number of solves of the
    run that failed in that layer -- to be checked after a run: a failed layer keeps its VMRs.

    For tests and diagnosis, beyond what the reference's loop leaves behind: run(...,
    diagnostics=True) keeps every iteration's q_up, q_down, dt_scale, wobbling layers and filter
    sigma in .history, and .radius is the radius of the next profile (hydrostatic models).

    Refused with ValueError before any launch: a spectrum that is not two-stream, alkali models,
    a Deck or cloud-type models in its Continuum, fewer than 2 layers, shapes that do not match,
    a heat-capacity table that is not finite, not ascending or has cp / R <= 1, and (in run) a
    starting temperature outside [tmin, tmax], or convection=True without heat_capacity, without
    mplanet > 0, or with a radius that is 0 at the bottom (hydro_g without p0, r0).  With
    chemistry=: a vmr, species other than the network's, a table or continuum species outside
    the network, an element ratio <= 0 or a non-finite abundance (naming the profile), a
    chemistry_start other than 'previous' / 'cold', and (in run) a starting temperature outside
    the Gibbs table."""

    def __init__(self, spectrum, pressure, vmr, mol_mass, radius_model=None, gravity=None,
                 mplanet=None, p0=None, r0=None, tint=0.0, flux_top=None, tmin=None, tmax=None,
                 species=None, table_species=None, heat_capacity=None, mixing_length=(1.5, 0.5),
                 chemistry=None, metallicity=None, e_scale=None, e_ratio=None,
                 chemistry_start='previous'):
        self.model = spectrum
        self.chemistry = chemistry
        _check(chemistry_start in ('previous', 'cold'),
               f"chemistry_start {chemistry_start!r}: 'previous' or 'cold'")
        self.chemistry_start = chemistry_start
        if chemistry is None:
            _check(metallicity is None and not e_scale and not e_ratio,
                   'metallicity, e_scale and e_ratio are the abundances of chemistry=')
        else:
            _check(vmr is None, 'with chemistry= the volume mixing ratios are the equilibrium '
                   "ones of every iteration: vmr must be None")
            _check(species is None or [str(s) for s in species] == chemistry.species,
                   f"with chemistry= the species are the network's ({chemistry.species})")
            species = chemistry.species
            _check(table_species is not None, 'with chemistry= table_species must name the '
                   "table's species among the network's")
        _check(getattr(spectrum, 'rt_path', None) == 'two_stream',
               f"rt_path {getattr(spectrum, 'rt_path_name', getattr(spectrum, 'rt_path', None))!r}: "
               "the net fluxes come from the two-stream geometry ('two_stream', "
               "'emission_two_stream', 'eclipse_two_stream')")
        cont = spectrum.continuum
        if cont is not None:
            for name, models in (('alkali models', cont.alkali), ('a Deck', cont.deck),
                                 ('cloud-type models', cont.cloud)):
                _check(not models, f'a Continuum with {name} is not supported in this loop '
                       '(the batched two-stream geometry takes neither); use eval()')
        L, W, S = spectrum.nlayers, spectrum.nwave, spectrum.nspec
        self.nlayers, self.nwave = L, W
        _check(L >= 2, f'{L} layer: the update differences neighbouring layers, at least 2')
        most = MAX_LAYERS if heat_capacity is None else MAX_LAYERS_CONVECTION
        _check(L <= most, f'{L} layers: at most {most} (the net-flux kernel keeps the profile and '
               "its workgroup's flux sums in LDS" +
               ('' if heat_capacity is None else ', the convective update eight vectors of it') + ')')
        self.pressure = np.asarray(pressure, float)
        _check(self.pressure.shape == (L,), f'pressure must have shape ({L},), got '
               f'{self.pressure.shape}')
        _check(np.all(np.diff(self.pressure) > 0) and self.pressure[0] > 0,
               'pressure must be positive and ascending')
        if chemistry is None:
            self.vmr = np.asarray(vmr, float)
            _check(self.vmr.ndim in (2, 3) and self.vmr.shape[-2] == L,
                   f'vmr must have shape ({L}, S) or (nw, {L}, S), got {self.vmr.shape}')
            nsp = self.vmr.shape[-1]
        else:
            self.vmr, nsp = None, chemistry.nspecies
        self.nspecies = nsp
        self.mol_mass = np.asarray(mol_mass, float)
        _check(self.mol_mass.shape == (nsp,), f'mol_mass must have shape ({nsp},), got '
               f'{self.mol_mass.shape}')
        # the columns of vmr behind the table's and the Continuum's densities
        cont_species = [] if cont is None else [str(s) for s in cont.species]
        if species is None:
            _check(not cont_species, f'a Continuum (species {cont_species}) needs species= and '
                   'table_species= to find its columns in vmr')
            _check(nsp >= S, f'vmr has {nsp} species, the table {S}')
            self.tab_map, self.cont_map = list(range(S)), []
        else:
            species = [str(s) for s in species]
            _check(len(species) == nsp, f'species names {len(species)} columns, vmr has {nsp}')
            _check(table_species is not None and len(table_species) == S,
                   f'table_species must name the {S} species of the table')
            for what, names in (('table', table_species), ('continuum', cont_species)):
                for s in names:
                    _check(str(s) in species, f'{what} species {s} is not in species ({species})')
            self.tab_map = [species.index(str(s)) for s in table_species]
            self.cont_map = [species.index(s) for s in cont_species]
        _check(radius_model in RMODELS, f"radius_model {radius_model!r}: None, 'hydro_g' or "
               "'hydro_m'")
        self.radius_model = radius_model
        self.gravity, self.mplanet, self.p0, self.r0 = gravity, mplanet, p0, r0
        if radius_model == 'hydro_g':
            _check(gravity is not None and gravity > 0, f'hydro_g needs gravity > 0, got {gravity}')
            _check((p0 is None) == (r0 is None), 'hydro_g: give both p0 and r0, or neither')
        elif radius_model == 'hydro_m':
            _check(mplanet is not None and mplanet > 0, f'hydro_m needs mplanet > 0, got {mplanet}')
            _check(p0 is not None and r0 is not None, 'hydro_m needs p0 and r0')
        if radius_model is not None and p0 is not None:
            _check(r0 > 0 and self.pressure[0] <= p0 <= self.pressure[-1],
                   f'p0 = {p0} bar outside the pressure grid, or r0 = {r0} <= 0')
        self.tint = np.asarray(tint, float)
        _check(self.tint.ndim in (0, 1), f'tint must be a scalar or [nw], got {self.tint.shape}')
        self.flux_top = None if flux_top is None else flux_top
        ftshape = None if flux_top is None else tuple(flux_top.shape)
        _check(ftshape is None or (len(ftshape) in (1, 2) and ftshape[-1] == W),
               f'flux_top must have shape ({W},) or (nw, {W}), got {ftshape}')
        self.heat_capacity = None
        if heat_capacity is not None:
            _check(len(heat_capacity) == 2, 'heat_capacity = (cp_temps[nT], cp_over_R[nT, S])')
            cp_temps = np.asarray(heat_capacity[0], float)
            cp_table = np.asarray(heat_capacity[1], float)
            _check(cp_temps.ndim == 1 and len(cp_temps) >= 1 and cp_table.ndim in (2, 3) and
                   cp_table.shape[-2:] == (len(cp_temps), nsp),
                   f'heat_capacity = (cp_temps[nT], cp_over_R[nT, {nsp}] or [nw, nT, {nsp}]), got '
                   f'shapes {cp_temps.shape} and {cp_table.shape}')
            _check(np.all(np.isfinite(cp_temps)) and np.all(np.isfinite(cp_table)),
                   'heat_capacity: a value that is not finite')
            _check(np.all(np.diff(cp_temps) > 0), 'heat_capacity: cp_temps must be ascending')
            _check(np.all(cp_table > 1.0), 'heat_capacity: cp_over_R <= 1 (cv = cp - R <= 0)')
            self.heat_capacity = (cp_temps, cp_table)
        # the abundances of the chemistry: per name a scalar or [nw]
        self.abundances = {}
        if chemistry is not None:
            given = [] if metallicity is None else [(('metal',), metallicity)]
            given += [(('scale', str(k)), v) for k, v in (e_scale or {}).items()]
            given += [(('ratio', str(k)), v) for k, v in (e_ratio or {}).items()]
            for key, v in given:
                v = np.asarray(v, float)
                _check(v.ndim in (0, 1), f'{key[-1]}: a scalar or [nw], got shape {v.shape}')
                if key[0] == 'scale':
                    chemistry.element_index(key[1])
                elif key[0] == 'ratio':
                    chemistry.ratio_elements(key[1])
                self.abundances[key] = v
        counts = {'vmr': self.vmr.shape[0] if self.vmr is not None and self.vmr.ndim == 3
                  else None,
                  **{key[-1]: v.shape[0] for key, v in self.abundances.items() if v.ndim == 1},
                  'tint': self.tint.shape[0] if self.tint.ndim == 1 else None,
                  'flux_top': ftshape[0] if ftshape is not None and len(ftshape) == 2 else None,
                  'heat_capacity': self.heat_capacity[1].shape[0] if self.heat_capacity is not None
                  and self.heat_capacity[1].ndim == 3 else None}
        given = {k: v for k, v in counts.items() if v is not None}
        _check(len(set(given.values())) <= 1, f'different numbers of profiles: {given}')
        self.nprofiles = next(iter(given.values())) if given else None     # None: temp0 decides
        for w in range(self.nprofiles or 1):
            _check(chemistry is None or self._abundances_host(w) is not None,
                   f'profile {w}: an element ratio <= 0 or an abundance that is not finite and '
                   f'positive ({self._abundance_text(w)})')
        lo, hi = float(spectrum.tmin), float(spectrum.tmax)
        for m in ([] if cont is None else cont.cia):
            lo, hi = max(lo, float(m.tmin)), min(hi, float(m.tmax))
        if chemistry is not None:
            lo = max(lo, float(chemistry.gibbs_temps[0]))
            hi = min(hi, float(chemistry.gibbs_temps[-1]))
        self.tmin = lo if tmin is None else float(tmin)
        self.tmax = hi if tmax is None else float(tmax)
        _check(self.tmin < self.tmax, f'tmin = {self.tmin} >= tmax = {self.tmax}')
        _check(len(mixing_length) == 2 and all(np.isfinite(v) and v >= 0 for v in mixing_length),
               f'mixing_length = (alpha, beta), both finite and >= 0, got {mixing_length}')
        self.mixing_length = (float(mixing_length[0]), float(mixing_length[1]))
        self.temps = self.dt_scale = self.q_up = self.q_down = self.spectrum = None
        self.conv_flux = self.convective = None
        self.mean_mass = self.chem_status = self.chem_failures = None
        self._state = None

    # --------------------------------------------------------------------------- chemistry
    def _abundance_values(self, w):
        """(metallicity or None, e_scale, e_ratio) of profile w."""
        metal, scale, ratio = None, {}, {}
        for key, v in self.abundances.items():
            value = float(v[w]) if v.ndim else float(v)
            if key[0] == 'metal':
                metal = value
            else:
                (scale if key[0] == 'scale' else ratio)[key[1]] = value
        return metal, scale, ratio

    def _abundances_host(self, w):
        """b[E] of profile w (ChemNetwork.element_abundances_host), None where it is refused."""
        return self.chemistry.element_abundances_host(*self._abundance_values(w))

    def _abundance_text(self, w):
        metal, scale, ratio = self._abundance_values(w)
        return ', '.join([f'[M/H] = {metal}'] * (metal is not None) +
                         [f'[{k}/H] = {v}' for k, v in scale.items()] +
                         [f'{k} = {v}' for k, v in ratio.items()])

    def _carried_equilibrium(self, nw, pressure_d):
        """The CarriedEquilibrium of nw profiles: one column of params per abundance."""
        from . import chemistry as ch
        net = self.chemistry
        for w in range(nw):
            _check(self._abundances_host(w) is not None,
                   f'profile {w}: an element ratio <= 0 or an abundance that is not finite and '
                   f'positive ({self._abundance_text(w)})')
        columns = dict(par_metal=-1, scales=[], ratios=[])
        params = np.empty((nw, len(self.abundances)))
        for col, (key, v) in enumerate(self.abundances.items()):
            params[:, col] = v
            if key[0] == 'metal':
                columns['par_metal'] = col
            elif key[0] == 'scale':
                columns['scales'].append((net.element_index(key[1]), col))
            else:
                columns['ratios'].append((*net.ratio_elements(key[1]), col))
        return ch.CarriedEquilibrium(net, nw, pressure_d, self.mol_mass,
                                     dev(params) if params.shape[1] else None, **columns)

    # ------------------------------------------------------------------------------ set-up
    def _allocate(self, nw):
        """Everything the loop touches, once per object: device copies of the constants, the
        state, and the buffers of the three launches."""
        import torch
        require_gpu()
        m, L, W = self.model, self.nlayers, self.nwave
        d = {}

        def new(*shape, dtype=torch.float64, fill=None):
            t = torch.empty(shape, dtype=dtype, device='cuda')
            return t if fill is None else t.fill_(fill)
        d['pressure'], d['lnp'] = dev(self.pressure), dev(np.log(self.pressure))
        d['dpress'] = dev(log_pressure_steps(self.pressure))
        if self.chemistry is None:
            d['vmr'] = dev(self.vmr)
            d['mm'] = dev(np.sum(self.vmr * self.mol_mass, axis=-1))
            per_profile = self.vmr.ndim == 3
        else:
            # the VMRs and the mean mass are what pb_radeq_equilibrium writes, per profile
            d['chem'] = self._carried_equilibrium(nw, d['pressure'])
            d['vmr'], d['mm'] = d['chem'].vmr, d['chem'].mm
            d['chem_iterations'] = d['chem'].status
            per_profile = True
        d['tab_map'] = torch.tensor(self.tab_map, dtype=torch.int32, device='cuda')
        d['cont_map'] = torch.tensor(self.cont_map or [0], dtype=torch.int32, device='cuda')
        d['tw'] = dev(trapezoid_weights(m.wn.cpu().numpy()))
        if self.tint.ndim == 0:
            d['f_int'] = internal_flux(m.wn, float(self.tint))
        else:
            d['f_int'] = torch.stack([internal_flux(m.wn, float(t)) for t in self.tint])
        d['flux_top'] = None if self.flux_top is None else \
            (self.flux_top if isinstance(self.flux_top, torch.Tensor) else dev(self.flux_top))
        npart = net_parts(W)
        ntab, ncont = len(self.tab_map), len(self.cont_map)
        d['temp'] = new(nw, L)
        d['dt_scale'] = new(nw, L, fill=DT_SCALE0)
        d['signs'] = new(nw, 4, L, fill=0.0)
        d['iter'] = new(nw, dtype=torch.int32, fill=0)
        d['q_up'], d['q_down'] = new(nw, L, fill=0.0), new(nw, L, fill=0.0)
        d['dens'] = new(nw, L, ntab)
        d['cdens'] = new(nw, L, ncont) if ncont else None
        d['radius'] = m.radius.view(1, L).expand(nw, L).contiguous()
        d['intervals'] = (d['radius'][:, :-1] - d['radius'][:, 1:]).contiguous()
        d['parts'] = new(nw, npart, 2, L)
        d['flux'] = new(nw, W)
        d['ec'] = new(nw, L, W)
        d['work'] = new(max(int(_capi.lib().pb_two_stream_net_work_doubles(L, W, nw)), 1))
        cont = m.continuum
        if cont is None:
            d['iwork'] = new(int(_capi.lib().pb_interp_ec_batch_work_doubles(L, nw)))
        else:
            d['ops'] = cont.batch_operands(None)
            d['iwork'] = new(d['ops'].work_doubles(L, W, nw))
        st = RadeqStruct()
        st.nlayers, st.nwalkers, st.nparts = L, nw, npart
        st.tmin, st.tmax = self.tmin, self.tmax
        st.parts_d, st.dpress_d = d['parts'].data_ptr(), d['dpress'].data_ptr()
        st.temp_d, st.dt_scale_d = d['temp'].data_ptr(), d['dt_scale'].data_ptr()
        st.signs_d, st.iter_d = d['signs'].data_ptr(), d['iter'].data_ptr()
        st.q_up_d, st.q_down_d = d['q_up'].data_ptr(), d['q_down'].data_ptr()
        st.pressure_d, st.lnp_d = d['pressure'].data_ptr(), d['lnp'].data_ptr()
        st.vmr_d, st.nspecies = d['vmr'].data_ptr(), self.nspecies
        st.vmr_stride = L * self.nspecies if per_profile else 0
        st.mm_d, st.mm_stride = d['mm'].data_ptr(), L if per_profile else 0
        st.temps_only = int(self.chemistry is not None)
        st.ntab, st.ncont = ntab, ncont
        st.tab_map_d = d['tab_map'].data_ptr()
        st.cont_map_d = d['cont_map'].data_ptr() if ncont else None
        st.dens_d = d['dens'].data_ptr()
        st.cdens_d = d['cdens'].data_ptr() if ncont else None
        st.rmodel = RMODELS[self.radius_model]
        st.has_ref = int(self.p0 is not None)
        st.mplanet, st.gplanet = float(self.mplanet or 0.0), float(self.gravity or 0.0)
        st.p0, st.r0 = float(self.p0 or 0.0), float(self.r0 or 0.0)
        st.radius_d, st.intervals_d = d['radius'].data_ptr(), d['intervals'].data_ptr()
        d['struct'] = st
        if self.heat_capacity is not None:
            cp_temps, cp_table = self.heat_capacity
            alpha, beta = self.mixing_length
            d['cp_temps'], d['cp_table'] = dev(cp_temps), dev(cp_table)
            d['mol_mass'] = dev(self.mol_mass)
            d['conv_dpress'] = dev(np.ediff1d(np.log(self.pressure * pa.BAR), to_begin=1.0))
            d['conv_flux'] = new(nw, L, fill=0.0)
            d['convective'] = new(nw, dtype=torch.int32, fill=0)
            cv = ConvectionStruct()
            cv.cp_temps_d, cv.cp_table_d = d['cp_temps'].data_ptr(), d['cp_table'].data_ptr()
            cv.cp_table_stride = cp_table.shape[1] * cp_table.shape[2] if cp_table.ndim == 3 else 0
            cv.ntemps = len(cp_temps)
            cv.mol_mass_d, cv.conv_dpress_d = d['mol_mass'].data_ptr(), d['conv_dpress'].data_ptr()
            cv.mplanet = float(self.mplanet or 0.0)
            cv.coeff = float(alpha**2 * np.sqrt(beta))
            cv.conv_flux_d, cv.convective_d = d['conv_flux'].data_ptr(), d['convective'].data_ptr()
            d['convection'] = cv
        self._state = d

    # --------------------------------------------------------------------------------- run
    def run(self, temp0=None, nsamples=100, continue_run=False, diagnostics=False,
            convection=False):
        """nsamples iterations from temp0 ([L] for every profile, or [nw, L]; host array or device
        tensor) -> the history temps[nw, 1 + nsamples, L] (device tensor; row 0 is temp0).
        continue_run=True: from the last row of the previous run with its dt_scale and a fresh
        sign history (temp0 is then not given).  The loop is launches only.  Leaves .temps,
        .dt_scale [nw, L], .q_up, .q_down [nw, L] and .spectrum [nw, W] (flux_up[0]) of the last
        evaluated profile, temps[:, -2].  diagnostics=True also keeps every iteration's q_up,
        q_down, dt_scale [nw, nsamples, L], wobble (int32, the wobbling layers) and sigma
        [nw, nsamples] in .history (device-to-device copies on the stream, still nothing read
        back).
        convection=True (the reference's flag; needs heat_capacity= and mplanet=): every
        iteration's update is pb_radeq_update_convective, which adds the mixing-length convective
        flux to the net flux of a profile with a superadiabatic layer and redoes its update.
        Leaves .conv_flux [nw, L] and .convective [nw] (int32: whether the second half ran) of the
        last iteration; with diagnostics, history['conv_flux'] [nw, nsamples, L] and
        history['convective'] [nw, nsamples].
        With chemistry=: five launches per iteration (module docstring); a continued run keeps the
        stored iterate, which belongs to the last row.  With diagnostics, history['vmr']
        [nw, nsamples, L, S] and history['chem_iterations'] [nw, nsamples, L] (int32) hold the
        VMRs and the status of every iteration's solve, i.e. at the temperatures of row 1 + i."""
        import torch
        L = self.nlayers
        nsamples = int(nsamples)
        _check(nsamples >= 0, f'nsamples = {nsamples}')
        if convection:
            _check(self.heat_capacity is not None, 'convection=True needs the heat capacities: '
                   'heat_capacity=(cp_temps[nT], cp_over_R[nT, S])')
            _check(self.mplanet is not None and self.mplanet > 0,
                   f'convection=True needs mplanet > 0 (gravity = G mplanet / radius**2), got '
                   f'{self.mplanet}')
            _check(not (self.radius_model == 'hydro_g' and self.p0 is None),
                   'convection=True with hydro_g needs p0 and r0: the radius is 0 at the bottom '
                   'without them')
        if continue_run:
            _check(self.temps is not None, 'continue_run without an earlier run')
            _check(temp0 is None, 'continue_run starts from the last row, not from a temp0')
            start = self.temps[:, -1]
        else:
            _check(temp0 is not None, 'run needs a starting profile temp0')
            host0 = temp0.cpu().numpy() if isinstance(temp0, torch.Tensor) else \
                np.asarray(temp0, float)
            _check(host0.ndim in (1, 2) and host0.shape[-1] == L,
                   f'temp0 must have shape ({L},) or (nw, {L}), got {host0.shape}')
            # the number of profiles: that of the per-profile inputs (vmr[nw, L, S], tint[nw],
            # flux_top[nw, W]); when all of them are shared, temp0 decides, run by run
            rows = host0.shape[0] if host0.ndim == 2 else None
            if self.nprofiles is None:
                nw = 1 if rows is None else rows
            else:
                nw = self.nprofiles
                _check(rows is None or rows == nw,
                       f'temp0 has {rows} profiles, the model {nw}')
            _check(np.all(host0 >= self.tmin) and np.all(host0 <= self.tmax),
                   f'temp0 outside the {self.tmin:.1f}-{self.tmax:.1f} K range of the opacities '
                   '(the table and the CIA tables)')
            if self.chemistry is not None:
                glo, ghi = self.chemistry.gibbs_temps[[0, -1]]
                _check(np.all(host0 >= glo) and np.all(host0 <= ghi),
                       f'temp0 outside the {glo:.1f}-{ghi:.1f} K range of the Gibbs table')
            if self._state is None or self._state['struct'].nwalkers != nw:
                self._allocate(nw)
            start = torch.as_tensor(np.broadcast_to(host0, (nw, L)).copy(), device='cuda')
        d = self._state
        st, m = d['struct'], self.model
        nw = st.nwalkers
        temps = torch.empty((nw, 1 + nsamples, L), dtype=torch.float64, device='cuda')
        temps[:, 0] = start
        d['temp'].copy_(start)
        d['iter'].zero_()
        d['signs'].zero_()
        if not continue_run:
            d['dt_scale'].fill_(DT_SCALE0)
        st.temps_d, st.nrows = temps.data_ptr(), 1 + nsamples
        stream = _stream()
        hist = None
        if diagnostics:
            hist = {k: torch.empty((nw, nsamples, L), dtype=torch.float64, device='cuda')
                    for k in ('q_up', 'q_down', 'dt_scale')}
            hist['wobble'] = torch.empty((nw, nsamples, L), dtype=torch.int32, device='cuda')
            hist['sigma'] = torch.empty((nw, nsamples), dtype=torch.float64, device='cuda')
            if convection:
                hist['conv_flux'] = torch.empty((nw, nsamples, L), dtype=torch.float64,
                                                device='cuda')
                hist['convective'] = torch.empty((nw, nsamples), dtype=torch.int32, device='cuda')
            d['wobble'] = torch.empty((nw, L), dtype=torch.int32, device='cuda')
            d['sigma'] = torch.empty(nw, dtype=torch.float64, device='cuda')
            st.wobble_d, st.sigma_d = d['wobble'].data_ptr(), d['sigma'].data_ptr()
        else:
            st.wobble_d = st.sigma_d = None
        chem = d.get('chem')
        if chem is not None:
            warm = self.chemistry_start == 'previous'
            chem.failures.zero_()
            if hist is not None:
                hist['vmr'] = torch.empty((nw, nsamples, L, self.nspecies), dtype=torch.float64,
                                          device='cuda')
                hist['chem_iterations'] = torch.empty((nw, nsamples, L), dtype=torch.int32,
                                                      device='cuda')
            # the equilibrium of the starting profile, from the cold start; a continued run's
            # VMRs, mean mass and iterate are those of the last row already, which is its start
            if not continue_run:
                chem.solve(d['temp'], warm=False)
        _capi.call('pb_radeq_update', C.byref(st), 1, stream)
        ckw = {}
        if 'ops' in d:
            ckw = dict(continuum=d['ops'], continuum_density=d['cdens'])
        for i in range(nsamples):
            interp_ec_batch(m.etable, m.ttable, d['temp'], d['dens'], out=d['ec'], work=d['iwork'],
                            **ckw)
            two_stream_net_batch(d['ec'], d['intervals'], m.wn, d['tw'], d['temp'], d['f_int'],
                                 d['flux_top'], out=d['flux'], parts=d['parts'], work=d['work'])
            # (with chemistry temps_only is set: the update stops behind the new temperatures)
            if convection:
                _capi.call('pb_radeq_update_convective', C.byref(st), C.byref(d['convection']),
                           stream)
            else:
                _capi.call('pb_radeq_update', C.byref(st), 0, stream)
            if chem is not None:
                chem.solve(d['temp'], warm=warm)
                _capi.call('pb_radeq_update', C.byref(st), 1, stream)
            if hist is not None:
                for k in hist:
                    hist[k][:, i].copy_(d[k])
        self.history = hist
        self.temps = temps
        self.dt_scale, self.q_up, self.q_down = d['dt_scale'], d['q_up'], d['q_down']
        self.spectrum = d['flux']
        self.radius = d['radius']
        if chem is not None:
            self.vmr, self.mean_mass = chem.vmr, chem.mm
            self.chem_status, self.chem_failures = chem.status, chem.failures
        if convection:
            self.conv_flux, self.convective = d['conv_flux'], d['convective']
        return temps
