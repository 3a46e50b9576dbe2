"""Atmospheres from retrieval parameters: what Atmosphere.calc_profiles
(pyratbay/pyrat/atmosphere.py:399-526) makes of the parameter vector eval() maps
(pyrat/pyrat_obj.py:258-275) -- T(p) model, VMR models and the bulk balance, ideal-gas density,
mean molecular mass, hydrostatic radius.

Two forms of the same arithmetic:
  * host forms in plain NumPy with the reference's names (Isothermal, Guillot, Madhu, IsoVMR,
    ScaleVMR, SlantVMR, vmr_scale, ideal_gas_density, mean_weight, hydro_m, hydro_g, qcapcheck),
    for TableSpectrum.eval() users and CPU tests;
  * WalkerAtmosphere.evaluate: params[nw, npar] -> the device tensors TableSpectrum.eval_bands
    takes, one launch of pb_walker_atmosphere (csrc/pb_atmosphere.hip), nothing read back; with
    chemistry=ChemNetwork(...) (chemistry.py) the VMRs are the equilibrium of every layer at the
    walker's [M/H], [X/H] and X/Y, three launches.

Constants: those of pyratbay.constants (CODATA 2018 as scipy.constants carries them, the products
NumPy forms), not the legacy set of the reference's C extensions.
"""
import collections
import ctypes as C
from collections.abc import Iterable

import numpy as np

from ._device import dev, require_gpu

# pyratbay.constants: k = sc.k * 1e7, G = sc.G * 1e3, sc.N_A, bar
K_BOLTZ = 1.380649e-23 * 1e7
G_GRAV = 6.67430e-11 * 1e3
N_AVOGADRO = 6.02214076e23
BAR = 1e6
EULER = 0.57721566490153286061
E2_CUTOFF = 88.029691931113054296     # log(2**127): the reference's E2 returns 0 above it

MAX_SPECIES, MAX_VMR, MAX_BULK, MAX_LAYERS = 32, 16, 4, 1024
# isotope ratios of the table's slots (isotopes.py): labelled slots, fillers of one fill slot
MAX_ISO_SLOTS, MAX_ISO_FILLERS = 32, 7
REJECT_TEMP, REJECT_MADHU, REJECT_QCAP, REJECT_REFPRESSURE, REJECT_DIVERGENT = 1, 2, 4, 8, 16
REJECT_ISOTOPE = 32                    # a non-finite or negative isotope ratio (isotopes.py)
# (32 is taken by the isotope ratios, which share the mask: the chemistry's bit is the next one)
REJECT_CHEMISTRY = 64                  # an equilibrium cell without VMRs (chemistry.py)
REJECT_NAMES = {REJECT_TEMP: 'temperature <= 0 or not finite', REJECT_MADHU: 'madhu log_p1 > log_p3',
                REJECT_QCAP: 'trace abundances above qcap',
                REJECT_REFPRESSURE: 'reference pressure outside the grid',
                REJECT_DIVERGENT: 'divergent hydro_m profile, or a radius <= 0 or not finite',
                REJECT_ISOTOPE: 'a negative or non-finite isotope ratio',
                REJECT_CHEMISTRY: 'equilibrium chemistry: not converged, a temperature outside '
                                  'the Gibbs table, or an element ratio <= 0'}


# ---------------------------------------------------------------------------------------------
# Temperature models (pyratbay/atmosphere/tmodels/tmodels.py)
# ---------------------------------------------------------------------------------------------
def expn2(x):
    """Exponential integral E2(x) for x >= 0, from its definitions (Abramowitz & Stegun 5.1.12,
    5.1.22): the power series for x <= 1, the continued fraction (modified Lentz) above; 0 for
    x > log(2**127) like the reference's.  The device evaluates the same steps in the same order."""
    x = np.atleast_1d(np.asarray(x, float))
    out = np.zeros_like(x)
    out[x == 0.0] = 1.0
    small = (x > 0.0) & (x <= 1.0)
    if np.any(small):
        xs = x[small]
        term = -xs
        total = np.zeros_like(xs)
        for m in range(2, 25):
            term = term * (-xs) / float(m)
            total += term / float(m - 1)
        out[small] = (1.0 + (-xs) * ((1.0 - EULER) - np.log(xs))) - total
    large = (x > 1.0) & (x <= E2_CUTOFF)
    if np.any(large):
        xl = x[large]
        b = xl + 2.0
        c = np.full_like(xl, 1.0e300)
        d = 1.0 / b
        h = d.copy()
        live = np.ones(xl.shape, bool)
        for i in range(1, 401):
            an = -float(i) * float(i + 1)
            b = b + 2.0
            d = np.where(live, 1.0 / (an * d + b), d)
            c = np.where(live, b + an / c, c)
            delta = c * d
            h = np.where(live, h * delta, h)
            live = live & ~(np.abs(delta - 1.0) < 1.0e-16)
            if not np.any(live):
                break
        out[large] = h * np.exp(-xl)
    return out


class Isothermal:
    """Isothermal temperature profile model."""

    def __init__(self, pressure):
        self.name = 'isothermal'
        self.pnames = ['T_iso']
        self.npars = 1
        self.pressure = np.asarray(pressure, float)

    def __call__(self, params):
        _check_npars(self, params)
        value = params[0] if isinstance(params, Iterable) else params
        return np.full(len(self.pressure), value, np.double)


def _check_npars(model, params):
    if np.size(params) != model.npars:
        raise ValueError(f'Number of parameters ({np.size(params)}) does not match the required '
                         f'number of parameters ({model.npars}) of the {model.name} model')


class Guillot:
    """Guillot (2010) profile in the parameterization of Line et al. (2013): src_c/_pt.c:11-15,
    88-109.  gravity: None (taken as 1), a scalar or a profile (cm s-2)."""

    def __init__(self, pressure, gravity=None):
        self.name = 'guillot'
        self.pnames = ["log_kappa'", 'log_gamma1', 'log_gamma2', 'alpha', 'T_irr', 'T_int']
        self.npars = 6
        self.pressure = np.asarray(pressure, float)
        self.gravity_scalar = 1.0 if gravity is None else \
            (float(gravity) if np.isscalar(gravity) else None)
        if gravity is None:
            gravity = np.tile(1.0, len(self.pressure))
        elif np.isscalar(gravity):
            gravity = np.tile(float(gravity), len(self.pressure))
        self.gravity = np.asarray(gravity, float)

    @staticmethod
    def _xi(gamma, tau):
        gt = gamma * tau
        return (2.0 / 3.0) * (((1.0 / gamma) * (1.0 + ((0.5 * gamma) * tau - 1.0) * np.exp(-gt)) +
                               (gamma * (1.0 - 0.5 * (tau * tau))) * expn2(gt)) + 1.0)

    def __call__(self, params):
        _check_npars(self, params)
        params = np.asarray(params, np.double)
        kappa, gamma1, gamma2 = (np.float64(10.0)**params[i] for i in range(3))
        alpha, t_irr, t_int = params[3], params[4], params[5]
        tau = kappa * (self.pressure * BAR) / self.gravity
        tirr4, tint4 = t_irr**4.0, t_int**4.0
        with np.errstate(invalid='ignore', over='ignore'):
            xi1, xi2 = self._xi(gamma1, tau), self._xi(gamma2, tau)
            return (0.75 * ((tint4 * (2.0 / 3.0 + tau) + (tirr4 * (1.0 - alpha)) * xi1) +
                            (tirr4 * alpha) * xi2))**0.25


TCEA = Guillot


def gaussian_weights(sigma):
    """The kernel scipy.ndimage.gaussian_filter1d(sigma=sigma) correlates with (truncate = 4):
    radius int(4 sigma + 0.5), exp(-0.5 x^2 / sigma^2) normalised to a sum of 1."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x**2)
    return phi / phi.sum()


def correlate_nearest(values, weights):
    """scipy.ndimage.correlate1d(values, weights, mode='nearest') for symmetric weights, in its
    order: the centre tap, then the pairs from the outermost inwards.  The radius may exceed
    len(values)."""
    values = np.asarray(values, float)
    n, radius = len(values), (len(weights) - 1) // 2
    idx = np.arange(n)
    out = values * weights[radius]
    for k in range(-radius, 0):
        out = out + (values[np.maximum(idx + k, 0)] + values[np.minimum(idx - k, n - 1)]) \
            * weights[k + radius]
    return out


class Madhu:
    """Temperature profile model by Madhusudhan & Seager (2009): tmodels.py:232-325."""

    def __init__(self, pressure):
        self.name = 'madhu'
        self.pnames = ['log_p1', 'log_p2', 'log_p3', 'a1', 'a2', 'T0']
        self.npars = 6
        self.pressure = np.asarray(pressure, float)
        self.logp = np.log10(self.pressure)
        self.logp0 = np.amin(self.logp)
        # standard deviation of the smoothing kernel (~0.3 dex in pressure), in layers
        self.fsmooth = 0.33 / np.ediff1d(self.logp)[0]
        self.loge = np.log10(np.e)
        self.weights = gaussian_weights(self.fsmooth)

    def __call__(self, params):
        _check_npars(self, params)
        logp1, logp2, logp3, a1, a2, T0 = (np.float64(p) for p in params)
        if logp1 > logp3:
            return np.zeros(len(self.pressure))
        d1, d2 = a1 * self.loge, a2 * self.loge
        q1, q2, q3 = (logp1 - self.logp0) / d1, (logp1 - logp2) / d2, (logp3 - logp2) / d2
        T1 = T0 + q1 * q1
        T2 = T1 - q2 * q2
        T3 = T2 + q3 * q3
        layer1 = self.logp < logp1
        layer2 = (self.logp >= logp1) & (self.logp < logp3)
        temperature = np.full(len(self.pressure), T3)
        temperature[layer1] = T0 + ((self.logp[layer1] - self.logp0) / d1)**2
        temperature[layer2] = T2 + ((self.logp[layer2] - logp2) / d2)**2
        return correlate_nearest(temperature, self.weights)


# ---------------------------------------------------------------------------------------------
# VMR models (pyratbay/atmosphere/vmr_models/vmr_models.py:129-347)
# ---------------------------------------------------------------------------------------------
class IsoVMR:
    """Isobaric VMR model: one parameter, log10(VMR)."""
    kind = 0

    def __init__(self, species, pressure):
        self.species = species
        self.name = f'log_{species}'
        self.pnames = [f'log_{species}']
        self.npars = 1
        self.pressure = np.asarray(pressure, float)
        self.type = 'free'

    def __call__(self, params):
        _check_npars(self, params)
        value = params[0] if isinstance(params, Iterable) else params
        return np.full(len(self.pressure), np.float64(10.0)**value)


class ScaleVMR:
    """Scaled VMR model: vmr0 * 10**parameter."""
    kind = 1

    def __init__(self, species, pressure, vmr0):
        self.species = species
        self.name = f'scale_{species}'
        self.pnames = [f'log_{species}']
        self.npars = 1
        self.pressure = np.asarray(pressure, float)
        self.vmr0 = np.array(vmr0, float)
        self.type = 'free'

    def __call__(self, params):
        _check_npars(self, params)
        value = params[0] if isinstance(params, Iterable) else params
        return self.vmr0 * np.float64(10.0)**value


class SlantVMR:
    """Slanted VMR model: slope, log VMR0, log p0, min log VMR, max log VMR."""
    kind = 2

    def __init__(self, species, pressure):
        self.species = species
        self.name = f'slant_{species}'
        self.pnames = [f'slope_{species}', f'log_VMR0_{species}', f'log_p0_{species}',
                       f'min_log_{species}', f'max_log_{species}']
        self.npars = 5
        self.pressure = np.asarray(pressure, float)
        self.log_press = np.log10(self.pressure)
        self.type = 'free'

    def __call__(self, params):
        _check_npars(self, params)
        slope, vmr_0, log_p0, vmr_min, vmr_max = params
        log_vmr = slope * (self.log_press - log_p0) + vmr_0
        return 10.0**np.clip(log_vmr, vmr_min, vmr_max)


# Equilibrium-chemistry models (vmr_models.py:60-126): the names of the parameters that set the
# elemental abundances of a chemistry.ChemNetwork; they carry no arithmetic of their own
# (ChemNetwork.element_abundances_host has the rule).
class MetalEquil:
    """Metallicity of a thermochemical-equilibrium model: [M/H], in dex relative to solar, on
    every element but H and He."""

    def __init__(self):
        self.name = 'metal_equil'
        self.pnames = ['[M/H]']
        self.texnames = ['[M/H]']
        self.npars = 1
        self.type = 'equil'


class ScaleEquil:
    """Abundance of one element of a thermochemical-equilibrium model: name '[X/H]' (e.g. '[C/H]'),
    in dex relative to solar; overrides the metallicity for X."""

    def __init__(self, name):
        name = str(name)
        if len(name) < 5 or name[0] != '[' or name[-3:] != '/H]':
            raise ValueError(f"ScaleEquil: the format is [X/H], got '{name}'")
        self.name = 'scale_equil'
        self.element = name[1:-3]
        self.pnames = [name]
        self.texnames = [name]
        self.npars = 1
        self.type = 'equil'


class RatioEquil:
    """Abundance ratio of two elements of a thermochemical-equilibrium model: name 'X/Y' (e.g.
    'C/O'), the ratio itself (not its logarithm); sets X from Y."""

    def __init__(self, name):
        name = str(name)
        if name.count('/') != 1 or name[0] == '/' or name[-1] == '/':
            raise ValueError(f"RatioEquil: the format is X/Y, got '{name}'")
        self.name = 'ratio_equil'
        idx = name.index('/')
        self.elements = [name[0:idx], name[idx + 1:]]
        self.element_ratio = name.replace('/', '_')
        self.pnames = [name]
        self.texnames = [name]
        self.npars = 1
        self.type = 'equil'


# ---------------------------------------------------------------------------------------------
# Abundance scaling (pyratbay/atmosphere/vmr_scaling.py)
# ---------------------------------------------------------------------------------------------
def qcapcheck(vmr, qcap, ibulk):
    """Whether the trace abundances sum above qcap in any layer (vmr_scaling.py:52-66)."""
    if qcap is None:
        return False
    nspecies = np.shape(vmr)[1]
    itrace = np.setdiff1d(np.arange(nspecies), ibulk)
    return bool(np.any(np.sum(np.asarray(vmr)[:, itrace], axis=1) > qcap))


def ratio(vmr, ibulk):
    """Abundance ratios of the bulk species relative to the first, and the inverse of their sum."""
    vmr = np.asarray(vmr, float)
    bratio = np.ones((vmr.shape[0], len(ibulk)))
    for j in range(1, len(ibulk)):
        bratio[:, j] = vmr[:, ibulk[j]] / vmr[:, ibulk[0]]
    return bratio, 1.0 / np.sum(bratio, axis=1)


def balance(vmr, ibulk, bratio, invsrat):
    """Set the bulk species such that sum(vmr) = 1 in each layer (in place)."""
    itrace = np.setdiff1d(np.arange(vmr.shape[1]), ibulk)
    rest = 1.0 - np.sum(vmr[:, itrace], axis=1)
    for j in range(len(ibulk)):
        vmr[:, ibulk[j]] = bratio[:, j] * rest * invsrat


def vmr_scale(vmr, species, vmr_models, vmr_pars, bulk, qsat=None, iscale=None, ibulk=None,
              bratio=None, invsrat=None):
    """Scale the modelled species and balance the bulk (vmr_scaling.py:178-280; qsat = None)."""
    if qsat is not None:
        raise ValueError('vmr_scale: qsat is not supported (the reference marks it for removal)')
    if not isinstance(vmr_models, Iterable):
        vmr_models, vmr_pars = [vmr_models], [vmr_pars]
    species = list(species)
    if iscale is None:
        iscale = [species.index(model.species) for model in vmr_models]
    if ibulk is None:
        ibulk = [species.index(mol) for mol in bulk]
    if bratio is None:
        bratio, invsrat = ratio(vmr, ibulk)
    scaled = np.array(vmr, float)
    for i, model in enumerate(vmr_models):
        scaled[:, iscale[i]] = model(vmr_pars[i])
    balance(scaled, ibulk, bratio, invsrat)
    return scaled


# ---------------------------------------------------------------------------------------------
# Density, mean mass, hydrostatic radius (pyratbay/atmosphere/atmosphere.py)
# ---------------------------------------------------------------------------------------------
def ideal_gas_density(abundances, pressure, temperature):
    """Number density (molecules cm-3): atmosphere.py:629-664."""
    abundances = np.asarray(abundances, float)
    pressure, temperature = np.asarray(pressure, float), np.asarray(temperature, float)
    if np.shape(abundances) == np.shape(pressure):
        return abundances * (pressure * BAR) / (temperature * K_BOLTZ)
    return abundances * np.expand_dims(pressure / temperature, axis=1) * BAR / K_BOLTZ


def mean_weight(abundances, species=None, molfile=None, mass=None):
    """Mean molecular mass per layer (atmosphere.py:581-626); the masses must be given."""
    if mass is None:
        raise ValueError('mean_weight: give the species masses (mass=...); this package ships '
                         'no molecules file')
    return np.sum(np.atleast_2d(abundances) * np.asarray(mass, float), axis=1)


def _cumulative_trapezoid(y, x):
    return np.concatenate(([0.0], np.cumsum(np.diff(x) * (y[1:] + y[:-1]) / 2.0)))


def _slinear_at(x, y, x0):
    """scipy.interpolate.interp1d(x, y, kind='slinear')(x0) for a scalar x0: SciPy's first-order
    spline (its de Boor recurrence) and interp1d's error outside the range."""
    if not (x0 >= x[0]):
        raise ValueError(f"A value ({x0}) in x_new is below the interpolation range's minimum "
                         f"value ({x[0]}).")
    if not (x0 <= x[-1]):
        raise ValueError(f"A value ({x0}) in x_new is above the interpolation range's maximum "
                         f"value ({x[-1]}).")
    lo = int(np.clip(np.searchsorted(x, x0, 'right') - 1, 0, len(x) - 2))
    xa, xb = x[lo], x[lo + 1]
    w = 1.0 / (xb - xa)
    return y[lo] * (w * (xb - x0)) + y[lo + 1] * (w * (x0 - xa))


def hydro_g(pressure, temperature, mu, g, p0=None, r0=None):
    """Hydrostatic radius with a constant gravity (atmosphere.py:350-415)."""
    pressure, temperature = np.asarray(pressure, float), np.asarray(temperature, float)
    radius = _cumulative_trapezoid(-K_BOLTZ * N_AVOGADRO * temperature / (np.asarray(mu) * g),
                                   np.log(pressure))
    if p0 is not None and r0 is not None:
        radius += r0 - _slinear_at(pressure, radius, p0)
    else:
        radius -= radius[-1]
    return radius


def hydro_m(pressure, temperature, mu, mass, p0, r0):
    """Hydrostatic radius with g(r) = G mass / r^2 (atmosphere.py:418-485).  A divergent profile
    has inf above the layer where the radius stops decreasing."""
    pressure, temperature = np.asarray(pressure, float), np.asarray(temperature, float)
    integral = _cumulative_trapezoid(
        K_BOLTZ * N_AVOGADRO * temperature / (G_GRAV * np.asarray(mu) * mass), np.log(pressure))
    i0 = _slinear_at(pressure, integral, p0)
    with np.errstate(divide='ignore'):
        radius = 1.0 / (integral - i0 + 1 / r0)
    for j in range(len(radius) - 1):
        if radius[j] <= radius[j + 1]:
            radius[0:j + 1] = np.inf
    return radius


# ---------------------------------------------------------------------------------------------
# The batched form
# ---------------------------------------------------------------------------------------------
class AtmModelStruct(C.Structure):
    """pb_atm_model of include/pbhip.h."""
    _fields_ = [
        ('nlayers', C.c_int), ('nspecies', C.c_int), ('npar', C.c_int),
        ('tmodel', C.c_int),
        ('guillot_gravity', C.c_double),
        ('madhu_radius', C.c_int),
        ('madhu_logp0', C.c_double), ('madhu_loge', C.c_double),
        ('madhu_weights_d', C.c_void_p),
        ('nvmr', C.c_int),
        ('vmr_kind', C.c_int * MAX_VMR),
        ('vmr_species', C.c_int * MAX_VMR),
        ('vmr_par', C.c_int * MAX_VMR),
        ('vmr0_d', C.c_void_p),
        ('nbulk', C.c_int),
        ('bulk_species', C.c_int * MAX_BULK),
        ('bulk_ratio_d', C.c_void_p), ('invsrat_d', C.c_void_p),
        ('base_vmr_d', C.c_void_p),
        ('pressure_d', C.c_void_p),
        ('log10p_d', C.c_void_p), ('lnp_d', C.c_void_p),
        ('mass_d', C.c_void_p),
        ('rmodel', C.c_int),
        ('base_vmr_stride', C.c_int),
        ('mplanet', C.c_double), ('gplanet', C.c_double), ('rplanet', C.c_double),
        ('refpressure', C.c_double),
        ('par_rplanet', C.c_int), ('par_log_refpressure', C.c_int), ('par_mplanet', C.c_int),
        ('has_qcap', C.c_int),
        ('qcap', C.c_double),
        ('base_radius_d', C.c_void_p),
        ('ntab', C.c_int), ('ncont', C.c_int), ('nalk', C.c_int),
        ('tab_map_d', C.c_void_p), ('cont_map_d', C.c_void_p), ('alk_map_d', C.c_void_p),
    ]


Profiles = collections.namedtuple(
    'Profiles', 'temps dens radius mm continuum_density alkali_density reject')

_TMODELS = {Isothermal: 0, Guillot: 1, Madhu: 2}


def _chemistry():
    from . import chemistry
    return chemistry
_SCALARS = ('rplanet', 'log_refpressure', 'mplanet')


class WalkerAtmosphere:
    """params[nw, npar] -> the atmospheres of nw walkers, on the device in one launch.

    pressure[L] (bar, ascending, 2 <= L <= 1024), species (names), mol_mass[nspec] (g mol-1),
    base_vmr[L, nspec], bulk (names of 1-4 bulk species), tmodel (an Isothermal, a Guillot with
    gravity None or a scalar, or a Madhu of this module), vmr_models (IsoVMR / ScaleVMR / SlantVMR,
    each on a species of its own that is not a bulk species), rmodel 'hydro_m' (needs mplanet, g)
    or 'hydro_g' (needs gplanet, cm s-2), rplanet (cm) at refpressure (bar), qcap (None: no cap).

    free names the columns of params: the T model's parameters, each VMR model's parameters in
    model order, then any of 'rplanet' (cm), 'log_refpressure' (log10 bar) and 'mplanet' (g)
    -- the scalars pyrat_obj.py:269-275 maps; 'rplanet' and 'log_refpressure' together are refused
    (the reference's elif).  None: the models' parameters and no scalar.  What is not free is a
    constant of the model.

    base_radius[L]: the radius a rejected walker is given (finite and decreasing, so that no later
    kernel sees non-finite geometry); default: the radius of the model at base_params.

    Rejected walkers (reject[w] != 0, one bit per reason: REJECT_*) get temps = 0 in every layer
    -- which TableSpectrum.eval_bands turns into +inf band fluxes, the reference's reject value
    (pyrat_obj.py:302-320, 378-380) -- densities and mean masses of 0 and base_radius.  A madhu
    profile with log_p1 > log_p3 has both its own bit and the temperature bit (its temperatures
    are 0 in the reference).  DEVIATION: the reference carries on with a divergent hydro_m
    profile, neglecting the layers above the turn-over (rtop > 0); eval_bands has one itop for
    all walkers, so such a walker is rejected here.  The same bit covers, for either radius
    model, a radius that is <= 0 or not finite in any layer (a free rplanet or mplanet that is
    NaN, zero or negative), where the reference would go on with NaNs.

    base_params is an ADDITION to the reference-style signature: base_radius defaults to the
    radius of the base model, and a base model needs a parameter vector, so when base_radius is
    None, base_params[npar] (in `free` order) must be given; it is used for nothing else.

    chemistry (an ADDITION: the reference asks chemcat): None, or a chemistry.ChemNetwork; then
    the VMRs are the gas-phase equilibrium of every layer at the walker's elemental abundances
    (Atmosphere.calc_profiles' chemistry == 'equilibrium' branch, pyrat/atmosphere.py:445-473):
      * species must be the network's; base_vmr, bulk and qcap are not taken (pass None): the
        reference balances no bulk in equilibrium;
      * vmr_models holds MetalEquil(), ScaleEquil('[C/H]'), RatioEquil('C/O') (the rule:
        ChemNetwork.element_abundances_host) and IsoVMR models on network species, the hybrid
        ones: their column is clip(10**value, 0, max_vmr) on top of the equilibrium, max_vmr
        from the elements the equilibrium mixture holds (hybrid_vmr, vmr_models.py:40-57),
        nothing renormalised.  ScaleVMR and SlantVMR are refused, as the reference's hybrid is
        hard-wired to IsoVMR.  The reference's out-of-bounds flag of a hybrid value above its cap
        is inert (it sets out_of_bounds_vmr, the check reads _out_of_bounds_vmr,
        pyrat/atmosphere.py:473, 494), so no walker is rejected for it here either;
      * evaluate is three launches with nothing read back: the temperatures
        (pb_walker_temperature), the equilibrium of every (walker, layer) cell
        (pb_equilibrium_vmr), then pb_walker_atmosphere_chem on those VMRs;
      * a walker with a cell that did not converge, a temperature outside the network's Gibbs
        table or an X/Y <= 0 is rejected under REJECT_CHEMISTRY (64: 32 is the isotope ratios').
    Without a network the equilibrium models are refused (ValueError)."""

    def __init__(self, pressure, species, mol_mass, base_vmr, bulk, tmodel, vmr_models,
                 rmodel='hydro_m', mplanet=None, gplanet=None, rplanet=None, refpressure=None,
                 qcap=None, base_radius=None, free=None, base_params=None, chemistry=None):
        self.chemistry = chemistry
        self.pressure = np.ascontiguousarray(pressure, float)
        L = self.nlayers = len(self.pressure)
        if self.pressure.ndim != 1 or not 2 <= L <= MAX_LAYERS:
            raise ValueError(f'pressure: 2 ... {MAX_LAYERS} layers, got shape '
                             f'{self.pressure.shape}')
        if not np.all(np.diff(self.pressure) > 0) or self.pressure[0] <= 0:
            raise ValueError('pressure must be positive and ascending (top to bottom)')
        self.species = [str(s) for s in species]
        S = self.nspecies = len(self.species)
        if not 1 <= S <= MAX_SPECIES or len(set(self.species)) != S:
            raise ValueError(f'species: 1 ... {MAX_SPECIES} distinct names, got {self.species}')
        self.mol_mass = np.ascontiguousarray(mol_mass, float)
        if self.mol_mass.shape != (S,):
            raise ValueError(f'mol_mass must have shape {(S,)}, got {self.mol_mass.shape}')
        if chemistry is None:
            self.base_vmr = np.ascontiguousarray(base_vmr, float)
            if self.base_vmr.shape != (L, S):
                raise ValueError(f'base_vmr must have shape {(L, S)}, got {self.base_vmr.shape}')
            self.bulk = [str(b) for b in bulk]
            if not 1 <= len(self.bulk) <= MAX_BULK or len(set(self.bulk)) != len(self.bulk):
                raise ValueError(f'bulk: 1 ... {MAX_BULK} distinct species, got {self.bulk}')
            for b in self.bulk:
                if b not in self.species:
                    raise ValueError(f'bulk species {b} is not in the atmosphere ({self.species})')
            self.ibulk = [self.species.index(b) for b in self.bulk]
            self.bratio, self.invsrat = ratio(self.base_vmr, self.ibulk)
        else:
            if self.species != list(chemistry.species):
                raise ValueError(f'chemistry: species must be the network\'s {chemistry.species}, '
                                 f'got {self.species}')
            if base_vmr is not None or (bulk is not None and len(bulk)):
                raise ValueError('chemistry: base_vmr and bulk are not taken (pass None): the '
                                 'equilibrium gives every VMR, and the reference balances no bulk '
                                 'in equilibrium')
            if qcap is not None:
                raise ValueError('chemistry: qcap is not taken (there are no bulk species)')
            self.base_vmr, self.bulk, self.ibulk = None, [], []
            self.bratio = self.invsrat = None

        if type(tmodel) not in _TMODELS:
            raise ValueError('tmodel: an Isothermal, Guillot or Madhu of pyratbay_amd.atmosphere, '
                             f'got {type(tmodel).__name__}')
        if not np.array_equal(np.asarray(tmodel.pressure, float), self.pressure):
            raise ValueError('tmodel is defined on another pressure grid')
        if isinstance(tmodel, Guillot) and tmodel.gravity_scalar is None:
            raise ValueError('Guillot: the batched form takes gravity = None or a scalar, not a '
                             'profile')
        if isinstance(tmodel, Guillot) and not tmodel.gravity_scalar > 0:
            raise ValueError(f'Guillot: gravity must be positive, got {tmodel.gravity_scalar}')
        self.tmodel = tmodel
        self.vmr_models = list(vmr_models)
        if len(self.vmr_models) > MAX_VMR:
            raise ValueError(f'at most {MAX_VMR} VMR models, got {len(self.vmr_models)}')
        taken = set(self.bulk)
        self._equil = dict(par_metal=-1, scales=[], ratios=[], hybrids=[])
        for model in self.vmr_models if chemistry is not None else []:
            if not isinstance(model, (MetalEquil, ScaleEquil, RatioEquil, IsoVMR)):
                raise ValueError(
                    f'VMR model {getattr(model, "name", type(model).__name__)}: with chemistry, '
                    'only MetalEquil, ScaleEquil, RatioEquil and (hybrid) IsoVMR models are '
                    'taken; the reference\'s hybrid is hard-wired to IsoVMR')
            if isinstance(model, ScaleEquil):
                chemistry.element_index(model.element)
                if model.element == 'H':
                    raise ValueError('ScaleEquil: [H/H] is no parameter (abundances are relative '
                                     'to hydrogen)')
            if isinstance(model, RatioEquil):
                chemistry.ratio_elements(model.pnames[0])
        if chemistry is not None:
            pnames = [n for m in self.vmr_models for n in m.pnames]
            if len(set(pnames)) != len(pnames):
                raise ValueError(f'VMR models: a parameter is named twice ({pnames})')
            limit = _chemistry().MAX_ELEMENTS
            for cls in (ScaleEquil, RatioEquil):
                if sum(isinstance(m, cls) for m in self.vmr_models) > limit:
                    raise ValueError(f'at most {limit} {cls.__name__} models')
        for model in self.vmr_models:
            if chemistry is not None and not isinstance(model, IsoVMR):
                continue
            if getattr(model, 'type', 'free') != 'free' or \
                    not isinstance(model, (IsoVMR, ScaleVMR, SlantVMR)):
                raise ValueError(
                    f'VMR model {getattr(model, "name", type(model).__name__)}: '
                    'equilibrium-chemistry and hybrid models are not supported without '
                    'chemistry=ChemNetwork(...), only IsoVMR, ScaleVMR and SlantVMR')
            if model.species not in self.species:
                raise ValueError(f'VMR model {model.name}: species {model.species} is not in the '
                                 f'atmosphere ({self.species})')
            if model.species in taken:
                raise ValueError(f'VMR model {model.name}: species {model.species} is a bulk '
                                 'species or has a model already')
            taken.add(model.species)
            if not np.array_equal(np.asarray(model.pressure, float), self.pressure):
                raise ValueError(f'VMR model {model.name} is defined on another pressure grid')
        self.iscale = [self.species.index(m.species) if hasattr(m, 'species') else -1
                       for m in self.vmr_models]

        names = list(tmodel.pnames)
        self.tpar = slice(0, tmodel.npars)
        self.vmr_par = []
        for model in self.vmr_models:
            self.vmr_par.append(len(names))
            names += list(model.pnames)
        for model, col, isp in zip(self.vmr_models if chemistry is not None else [],
                                   self.vmr_par, self.iscale):
            if isinstance(model, MetalEquil):
                self._equil['par_metal'] = col
            elif isinstance(model, ScaleEquil):
                self._equil['scales'].append((chemistry.element_index(model.element), col))
            elif isinstance(model, RatioEquil):
                self._equil['ratios'].append(chemistry.ratio_elements(model.pnames[0]) + (col,))
            else:
                self._equil['hybrids'].append((isp, col))
        nmodel = len(names)
        free = names if free is None else [str(f) for f in free]
        if free[:nmodel] != names:
            raise ValueError(f'free must begin with the models\' parameters {names}, got {free}')
        scalars = free[nmodel:]
        for s in scalars:
            if s not in _SCALARS:
                raise ValueError(f"free: '{s}' is not one of {_SCALARS}")
        if len(set(scalars)) != len(scalars):
            raise ValueError(f'free: a scalar is listed twice ({scalars})')
        if 'rplanet' in scalars and 'log_refpressure' in scalars:
            raise ValueError("free: 'rplanet' and 'log_refpressure' cannot both be free (the "
                             'reference maps one or the other, pyrat_obj.py:269-272)')
        self.free = free
        self.npar = len(free)
        self.par_scalar = {s: (free.index(s) if s in scalars else -1) for s in _SCALARS}

        if rmodel not in ('hydro_m', 'hydro_g'):
            raise ValueError(f"rmodel: 'hydro_m' or 'hydro_g', got {rmodel!r}")
        self.rmodel = rmodel
        self.mplanet, self.gplanet = mplanet, gplanet
        self.rplanet, self.refpressure = rplanet, refpressure
        if rmodel == 'hydro_m' and mplanet is None and self.par_scalar['mplanet'] < 0:
            raise ValueError('hydro_m needs mplanet (g), as a constant or a free parameter')
        if rmodel == 'hydro_g' and gplanet is None:
            raise ValueError('hydro_g needs gplanet (cm s-2)')
        if rplanet is None and self.par_scalar['rplanet'] < 0:
            raise ValueError('rplanet (cm) is needed, as a constant or a free parameter')
        if refpressure is None and self.par_scalar['log_refpressure'] < 0:
            raise ValueError('refpressure (bar) is needed, as a constant or a free parameter')
        self.qcap = None if qcap is None else float(qcap)

        self._table_species = None
        self._cont_species, self._alk_species = [], []
        self._maps = None
        self._dev = None
        self._struct = None
        self._chem_buffers = {}
        # (kept for the retrieval front end: the value of a column no retrieval parameter names)
        self.base_params = None if base_params is None else \
            np.array(base_params, dtype=np.float64)
        if base_radius is None:
            if base_params is None:
                raise ValueError('give base_radius[L], or base_params (the parameter vector of '
                                 'the base model, whose radius it then is)')
            base = self._chain(np.asarray(base_params, float))
            if base['reject']:
                raise ValueError('base_params give a rejected model: '
                                 + ', '.join(n for b, n in REJECT_NAMES.items()
                                             if base['reject'] & b))
            base_radius = base['radius']
        self.base_radius = np.ascontiguousarray(base_radius, float)
        if self.base_radius.shape != (L,) or not np.all(np.isfinite(self.base_radius)) or \
                not np.all(np.diff(self.base_radius) < 0):
            raise ValueError(f'base_radius must be {L} finite, strictly decreasing radii')

    # ----------------------------------------------------------------------------- host form
    def _chain(self, params):
        """calc_profiles' order through the host forms, with the reject contract."""
        if params.shape != (self.npar,):
            raise ValueError(f'params must have shape {(self.npar,)} ({self.free}), got '
                             f'{params.shape}')
        reject = 0
        temp = self.tmodel(params[self.tpar])
        if isinstance(self.tmodel, Madhu) and params[0] > params[2]:
            reject |= REJECT_MADHU
        if np.any(~(temp > 0)) or not np.all(np.isfinite(temp)):
            reject |= REJECT_TEMP
        no_vmr = False
        if self.chemistry is not None:
            vmr, status = self.equilibrium_host(params, temp)
            if np.any((status < 0) & (status != _chemistry().STATUS_REJECTED)):
                reject |= REJECT_CHEMISTRY
            # a cell without VMRs has no mean mass: the walker is rejected already (this bit, or
            # the temperature's), and its radius is not judged
            no_vmr = bool(np.any(status < 0))
        else:
            pars = [params[o:o + m.npars] for o, m in zip(self.vmr_par, self.vmr_models)]
            vmr = vmr_scale(self.base_vmr, self.species, self.vmr_models, pars, self.bulk,
                            iscale=self.iscale, ibulk=self.ibulk, bratio=self.bratio,
                            invsrat=self.invsrat)
            if qcapcheck(vmr, self.qcap, self.ibulk):
                reject |= REJECT_QCAP
        with np.errstate(all='ignore'):
            dens = ideal_gas_density(vmr, self.pressure, temp)
            mm = mean_weight(vmr, mass=self.mol_mass)

            def scalar(name, const):
                return params[self.par_scalar[name]] if self.par_scalar[name] >= 0 else const
            r0 = scalar('rplanet', self.rplanet)
            mass = scalar('mplanet', self.mplanet)
            p0 = np.float64(10.0)**params[self.par_scalar['log_refpressure']] \
                if self.par_scalar['log_refpressure'] >= 0 else self.refpressure
            radius = None
            if not (p0 >= self.pressure[0] and p0 <= self.pressure[-1]):
                reject |= REJECT_REFPRESSURE
            elif no_vmr:
                pass
            elif self.rmodel == 'hydro_m':
                radius = hydro_m(self.pressure, temp, mm, mass, p0, r0)
                # (hydro_m has marked the layers above a turn-over with inf)
                if np.any(np.isinf(radius)) or np.any(radius[:-1] <= radius[1:]):
                    reject |= REJECT_DIVERGENT
            else:
                radius = hydro_g(self.pressure, temp, mm, self.gplanet, p0, r0)
            # either model: a free rplanet or mplanet that is NaN, zero or negative
            if radius is not None and not (np.all(np.isfinite(radius)) and np.all(radius > 0)):
                reject |= REJECT_DIVERGENT
        return dict(temps=temp, vmr=vmr, dens=dens, mm=mm, radius=radius, reject=reject)

    def equilibrium_host(self, params, temp):
        """The VMRs of one walker with chemistry: the elemental abundances from its [M/H], [X/H]
        and X/Y, the equilibrium of every layer, then the hybrid columns, each capped from the
        equilibrium VMRs -> vmr[L, S], status[L] (chemistry.equilibrium_host's)."""
        net, eq = self.chemistry, self._equil
        metallicity = None if eq['par_metal'] < 0 else params[eq['par_metal']]
        e_scale = {net.elements[j]: params[col] for j, col in eq['scales']}
        e_ratio = {f'{net.elements[x]}/{net.elements[y]}': params[col]
                   for x, y, col in eq['ratios']}
        b = net.element_abundances_host(metallicity, e_scale, e_ratio)
        equil, _, status = net.equilibrium_host(temp, self.pressure, b)
        vmr = equil.copy()
        for isp, col in eq['hybrids']:
            column = net.hybrid_host(equil, self.species[isp], params[col])
            vmr[:, isp] = np.where(status > 0, column, 0.0)
        return vmr, status

    def evaluate_host(self, params):
        """One walker through the host forms: the same result tuple as evaluate() (NumPy arrays,
        no walker axis), with the same reject contract.  Needs bind() first."""
        if self._table_species is None:
            raise ValueError('bind(table_species) first')
        c = self._chain(np.asarray(params, float))
        L = self.nlayers
        itab, icont, ialk = self._index_maps()
        if c['reject']:
            zeros = np.zeros((L, self.nspecies))
            return Profiles(np.zeros(L), zeros[:, itab], self.base_radius.copy(), np.zeros(L),
                            zeros[:, icont] if self._cont_species else None,
                            zeros[:, ialk] if self._alk_species else None, c['reject'])
        d = c['dens']
        return Profiles(c['temps'], d[:, itab], c['radius'], c['mm'],
                        d[:, icont] if self._cont_species else None,
                        d[:, ialk] if self._alk_species else None, 0)

    # ------------------------------------------------------------------------------ binding
    def _index_maps(self):
        return tuple([self.species.index(s) for s in names] for names in
                     (self._table_species, self._cont_species, self._alk_species))

    def bind(self, table_species, continuum=None):
        """Fix the species of the three density outputs: dens (the opacity table's species, in
        its order), continuum_density (continuum.species) and alkali_density
        (continuum.alkali_species).  continuum: a pyratbay_amd.continuum.Continuum, or anything
        with those two attributes."""
        table_species = [str(s) for s in table_species]
        cont = [] if continuum is None else [str(s) for s in getattr(continuum, 'species', [])]
        alk = [] if continuum is None else \
            [str(s) for s in getattr(continuum, 'alkali_species', [])]
        if not table_species:
            raise ValueError('bind: no table species')
        for what, names in (('table', table_species), ('continuum', cont), ('alkali', alk)):
            for s in names:
                if s not in self.species:
                    raise ValueError(f'bind: {what} species {s} is not in the atmosphere '
                                     f'({self.species})')
        self._table_species, self._cont_species, self._alk_species = table_species, cont, alk
        self._struct = None
        return self

    def _build_struct(self):
        import torch
        require_gpu()
        if self._dev is None:
            d = {}
            d['pressure'] = dev(self.pressure)
            d['log10p'] = dev(np.log10(self.pressure))
            d['lnp'] = dev(np.log(self.pressure))
            if self.chemistry is None:
                d['base_vmr'] = dev(self.base_vmr)
                d['bratio'] = dev(self.bratio)
                d['invsrat'] = dev(self.invsrat)
            d['mass'] = dev(self.mol_mass)
            d['base_radius'] = dev(self.base_radius)
            if isinstance(self.tmodel, Madhu):
                d['weights'] = dev(self.tmodel.weights)
            vmr0 = np.zeros((max(len(self.vmr_models), 1), self.nlayers))
            for i, model in enumerate(self.vmr_models):
                if isinstance(model, ScaleVMR):
                    vmr0[i] = model.vmr0
            d['vmr0'] = dev(vmr0)
            self._dev = d
        d = self._dev
        for key, idx in zip(('tab_map', 'cont_map', 'alk_map'), self._index_maps()):
            d[key] = torch.tensor(idx if idx else [0], dtype=torch.int32, device='cuda')
        st = self.model_struct()
        st.madhu_weights_d = d['weights'].data_ptr() if 'weights' in d else None
        st.vmr0_d = d['vmr0'].data_ptr()
        if self.chemistry is None:
            st.bulk_ratio_d, st.invsrat_d = d['bratio'].data_ptr(), d['invsrat'].data_ptr()
            st.base_vmr_d = d['base_vmr'].data_ptr()
        else:                   # base_vmr_d: the equilibrium VMRs of a call (_chemistry_buffers)
            self._chem_struct = self.chemistry.bound_struct(d['pressure'], self.npar,
                                                            **self._equil)
        st.pressure_d = d['pressure'].data_ptr()
        st.log10p_d, st.lnp_d = d['log10p'].data_ptr(), d['lnp'].data_ptr()
        st.mass_d, st.base_radius_d = d['mass'].data_ptr(), d['base_radius'].data_ptr()
        st.tab_map_d = d['tab_map'].data_ptr()
        st.cont_map_d = d['cont_map'].data_ptr() if self._cont_species else None
        st.alk_map_d = d['alk_map'].data_ptr() if self._alk_species else None
        self._struct = st
        self._chem_buffers = {}

    def _chemistry_buffers(self, nw, device):
        """The buffers between the three launches of a call with chemistry, kept per nw so that a
        call with `out` allocates nothing: the temperatures as formed, the equilibrium VMRs and
        cell statuses, and this model's struct pointing at those VMRs."""
        import torch
        key = (nw, str(device))
        if key not in self._chem_buffers:
            L, S = self.nlayers, self.nspecies
            temps = torch.empty((nw, L), dtype=torch.float64, device=device)
            vmr = torch.empty((nw, L, S), dtype=torch.float64, device=device)
            status = torch.empty((nw, L), dtype=torch.int32, device=device)
            st = AtmModelStruct.from_buffer_copy(self._struct)
            st.base_vmr_d, st.base_vmr_stride = vmr.data_ptr(), L * S
            self._chem_buffers[key] = (temps, vmr, status, st)
        return self._chem_buffers[key]

    def model_struct(self):
        """The pb_atm_model of this model with its scalar fields set (device pointers: null)."""
        st = AtmModelStruct()
        st.nlayers, st.nspecies, st.npar = self.nlayers, self.nspecies, self.npar
        st.tmodel = _TMODELS[type(self.tmodel)]
        if isinstance(self.tmodel, Guillot):
            st.guillot_gravity = self.tmodel.gravity_scalar      # positive: checked in __init__
        else:
            st.guillot_gravity = 1.0
        if isinstance(self.tmodel, Madhu):
            st.madhu_radius = (len(self.tmodel.weights) - 1) // 2
            st.madhu_logp0, st.madhu_loge = float(self.tmodel.logp0), float(self.tmodel.loge)
        # (with chemistry every VMR comes from the equilibrium launch: no model, no bulk here)
        st.nvmr = len(self.vmr_models) if self.chemistry is None else 0
        for i, model in enumerate(self.vmr_models if self.chemistry is None else []):
            st.vmr_kind[i], st.vmr_species[i] = model.kind, self.iscale[i]
            st.vmr_par[i] = self.vmr_par[i]
        st.nbulk = len(self.ibulk)
        for j, i in enumerate(self.ibulk):
            st.bulk_species[j] = i
        st.rmodel = 0 if self.rmodel == 'hydro_m' else 1
        st.mplanet = float(self.mplanet or 0.0)
        st.gplanet = float(self.gplanet or 0.0)
        st.rplanet = float(self.rplanet or 0.0)
        st.refpressure = float(self.refpressure or 0.0)
        st.par_rplanet = self.par_scalar['rplanet']
        st.par_log_refpressure = self.par_scalar['log_refpressure']
        st.par_mplanet = self.par_scalar['mplanet']
        st.has_qcap = int(self.qcap is not None)
        st.qcap = self.qcap if self.qcap is not None else 0.0
        st.ntab = len(self._table_species or [])
        st.ncont, st.nalk = len(self._cont_species), len(self._alk_species)
        return st

    # ----------------------------------------------------------------------------- evaluate
    def evaluate(self, params, out=None):
        """params[nw, npar] (float64 device tensor, columns in `free` order) -> Profiles of
        device tensors: temps[nw, L], dens[nw, L, ntab], radius[nw, L], mm[nw, L],
        continuum_density[nw, L, ncont] / alkali_density[nw, L, nalk] (None without such
        species), reject[nw] (int32 bit mask).  One launch, nothing read back, no allocation
        when `out` (a Profiles of an earlier call with the same nw) is given: capturable into a
        graph.  Shape and dtype are checked before any HIP call."""
        import torch
        from ._capi import call
        if self._table_species is None:
            raise ValueError('evaluate: bind(table_species) first')
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float64 or \
                params.dim() != 2 or params.shape[1] != self.npar:
            got = (tuple(params.shape), params.dtype) if isinstance(params, torch.Tensor) \
                else type(params).__name__
            raise ValueError(f'evaluate: params must be a float64 tensor of shape (nw, '
                             f'{self.npar}) ({self.free}), got {got}')
        if not params.is_cuda:
            raise ValueError('evaluate: params must be a device tensor')
        params = params.contiguous()
        if self._struct is None:
            self._build_struct()
        st = self._struct
        nw, L = params.shape[0], self.nlayers
        if out is None:
            def new(*shape, dtype=torch.float64):
                return torch.empty(shape, dtype=dtype, device=params.device)
            out = Profiles(new(nw, L), new(nw, L, st.ntab), new(nw, L), new(nw, L),
                           new(nw, L, st.ncont) if st.ncont else None,
                           new(nw, L, st.nalk) if st.nalk else None,
                           new(nw, dtype=torch.int32))
        else:
            want = ((nw, L), (nw, L, st.ntab), (nw, L), (nw, L),
                    (nw, L, st.ncont) if st.ncont else None,
                    (nw, L, st.nalk) if st.nalk else None, (nw,))
            for name, t, shape in zip(Profiles._fields, out, want):
                dtype = torch.int32 if name == 'reject' else torch.float64
                if (t is None) != (shape is None) or \
                        (t is not None and (not isinstance(t, torch.Tensor) or
                                            tuple(t.shape) != shape or not t.is_contiguous() or
                                            t.dtype != dtype or t.device != params.device)):
                    raise ValueError(f'evaluate: out.{name} must be a contiguous {dtype} tensor '
                                     f'of shape {shape} on {params.device}')
        outputs = (out.temps.data_ptr(), out.dens.data_ptr(), out.radius.data_ptr(),
                   out.mm.data_ptr(),
                   None if out.continuum_density is None else out.continuum_density.data_ptr(),
                   None if out.alkali_density is None else out.alkali_density.data_ptr(),
                   out.reject.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if self.chemistry is not None:
            temps, vmr, status, cst = self._chemistry_buffers(nw, params.device)
            stream = outputs[-1]
            call('pb_walker_temperature', C.byref(st), params.data_ptr(), nw, temps.data_ptr(),
                 stream)
            call('pb_equilibrium_vmr', C.byref(self._chem_struct), temps.data_ptr(),
                 params.data_ptr(), nw, vmr.data_ptr(), status.data_ptr(), stream)
            call('pb_walker_atmosphere_chem', C.byref(cst), params.data_ptr(), nw,
                 status.data_ptr(), *outputs)
            return out
        call('pb_walker_atmosphere', C.byref(st), params.data_ptr(), nw,
             out.temps.data_ptr(), out.dens.data_ptr(), out.radius.data_ptr(),
             out.mm.data_ptr(),
             None if out.continuum_density is None else out.continuum_density.data_ptr(),
             None if out.alkali_density is None else out.alkali_density.data_ptr(),
             out.reject.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out
