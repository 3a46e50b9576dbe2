"""The host forms of one atmosphere, in plain NumPy with the reference's names: the T(p) models
(Isothermal, Guillot, Madhu), the VMR models (IsoVMR, ScaleVMR, SlantVMR; MetalEquil, ScaleEquil,
RatioEquil name the parameters of a chemistry.ChemNetwork), vmr_scale and the bulk balance,
qcapcheck, ideal_gas_density, mean_weight, hydro_m, hydro_g -- what Atmosphere.calc_profiles
(pyratbay/pyrat/atmosphere.py:399-526) calls, for TableSpectrum.eval() users and CPU tests.  The
batched form (atmosphere.py, which carries every name of this module too) runs the same arithmetic
per walker on the device.

Constants: those of pyratbay.constants (CODATA 2018 as scipy.constants carries them, the products
NumPy forms), not the legacy set of the reference's C extensions.
"""
from collections.abc import Iterable

import numpy as np

# pyratbay.constants: k = sc.k * 1e7, G = sc.G * 1e3, sc.N_A, bar
K_BOLTZ = 1.380649e-23 * 1e7
G_GRAV = 6.67430e-11 * 1e3
N_AVOGADRO = 6.02214076e23
BAR = 1e6
EULER = 0.57721566490153286061
E2_CUTOFF = 88.029691931113054296     # log(2**127): the reference's E2 returns 0 above it


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
