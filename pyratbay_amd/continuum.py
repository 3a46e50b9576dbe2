"""Continuum opacity models on the device.

Host side mirrors the reference's model classes -- same names, constructor arguments and
parameters -- and keeps what depends only on the spectral grid (cross sections, tables
resampled to the grid) resident in HBM.  What depends on the atmosphere is evaluated by
ONE fused kernel (pb_continuum) plus one windowed kernel per alkali species
(pb_alkali_cross_section), accumulating into the extinction coefficient that the
line-by-line or table stage left on the device.  The batched form (TableSpectrum.eval_bands)
adds every term, the alkali doublets included, in the store of the batched interpolation.

    models = [Kurucz(wn, 'H2'), Lecavelier(pressure, wn), Collision_Induced(path, wn=wn), ...]
    cont = Continuum(wn, pressure, models)
    cont.add(ec, temp, {'H2': n_H2, 'He': n_He, ...})      # ec[L,W] += all terms

Reference: pyratbay/opacity/rayleigh/rayleigh.py, clouds/lecavelier.py, clouds/gray.py,
cia.py, hydrogen_ion.py, alkali/alkali.py; io/io.py:866-950 (read_cs)."""
import ctypes as C
import functools

import numpy as np
import torch

from ._capi import call, constant, hptr, struct
from ._device import dev, _ptr, _stream

# pyratbay/constants/astrophysical_constants.py:67-131 (scipy.constants, CODATA 2018)
H = 6.62607015e-27
K = 1.380649e-16
LS = 29979245800.0
BAR = 1e6
AMU = 1.6605390666e-24
AMAGAT = 2.6867801117984436e+19
UM = 1e-4
KM = 1e5


def _grid(wn, wl):
    if (wn is None) == (wl is None):
        raise ValueError('Either provide wavelength or wavenumber array, not both')
    return np.asarray(1.0 / (np.asarray(wl) * UM) if wn is None else wn, float)


class Kurucz:
    """Rayleigh scattering of H, He, H2 or e- (rayleigh.py:13-107)."""

    def __init__(self, wn, species):
        self.name = f'rayleigh_{species}'
        self.species = species
        self.wn = np.asarray(wn, float)
        wn = self.wn
        if species in ('H', 'H2'):
            c = {'H': (5.799e-45, 1.422e-54, 2.784e-64),
                 'H2': (8.140e-45, 1.280e-54, 1.610e-64)}[species]
            self.cross_section = c[0] * wn**4.0 + c[1] * wn**6.0 + c[2] * wn**8.0
        elif species == 'He':
            c = (5.484e-46, 2.440e-11, 5.940e-42, 2.900e-11)
            self.cross_section = c[0] * wn**4 * (
                1.0 + c[1] * wn**2 + c[2] * wn**4 / (1 - c[3] * wn**2))**2.0
        elif species == 'e-':
            self.cross_section = np.tile(6.653e-25, len(wn))
        else:
            raise ValueError(f"no Rayleigh model for '{species}'")

    def rank1(self, pressure, temperature, density):
        return self.cross_section, density[self.species]


class Lecavelier:
    """Rayleigh-like haze, kappa = 10**pars[0] * s0 * (wn*l0)**(-pars[1]) on a nominal
    density p/kT (lecavelier.py:14-100)."""

    def __init__(self, pressure, wl=None, wn=None):
        self.name = 'lecavelier'
        self.pressure = np.asarray(pressure, float)
        self.wn = _grid(wn, wl)
        self.pars = [0.0, -4.0]
        self.s0, self.l0 = 5.31e-27, 3.5e-5
        self.calc_cross_section()

    def calc_cross_section(self, pars=None):
        if pars is not None:
            self.pars[:] = pars
        self.cross_section = 10.0**self.pars[0] * self.s0 * (self.wn * self.l0)**(-self.pars[1])
        return self.cross_section

    def rank1(self, pressure, temperature, density):
        return self.cross_section, self.pressure * BAR / temperature / K


class CCSgray:
    """Constant-cross-section gray cloud between two pressures (gray.py:17-90)."""

    def __init__(self, pressure, wn):
        self.name = 'ccsgray'
        self.pressure = np.asarray(pressure, float)
        self.wn = np.asarray(wn, float)
        self.pars = [0.0, -4.0, 2.0]
        self.s0 = 5.31e-27

    def calc_cross_section(self):
        p_top, p_bottom = 10**self.pars[2], 10**self.pars[1]
        mask = (self.pressure >= p_bottom) & (self.pressure <= p_top)
        cs = np.zeros(len(self.pressure))
        cs[mask] = 10**self.pars[0] * self.s0
        return cs

    def rank1(self, pressure, temperature, density):
        return np.ones(len(self.wn)), self.calc_cross_section() * (
            self.pressure * BAR / temperature / K)


class Deck:
    """Instantly opaque gray cloud deck at pressure 10**pars[0] bar (gray.py:92-150).  It adds
    nothing to ec; it sets the bottom of the optical-depth integration (ibottom = itop + 1)
    and the cloud-top radius / temperature that the radiative transfer uses."""

    def __init__(self, pressure, wn):
        self.name = 'deck'
        self.pressure = np.asarray(pressure, float)
        self.wn = np.asarray(wn, float)
        self.pars = [-1.0]
        self.itop, self.rsurf, self.tsurf = None, 0.0, 0.0

    def calc_extinction_coefficient(self, radius, temperature, pars=None):
        if pars is not None:
            self.pars[:] = pars
        ptop = 10**self.pars[0]
        nlayers = len(self.pressure)
        if ptop >= self.pressure[-1]:
            self.itop = nlayers - 1
        elif ptop < self.pressure[0]:
            self.itop = 1
        else:
            self.itop = int(np.where(self.pressure >= ptop)[0][0])
        # scipy.interpolate.interp1d (linear) in pressure
        self.tsurf = float(np.interp(ptop, self.pressure, temperature))
        self.rsurf = float(np.interp(ptop, self.pressure, radius))
        return self.itop, self.rsurf, self.tsurf


def read_cs(csfile):
    """Cross-section table file (io/io.py:866-950): '@SPECIES', '@TEMPERATURES', '@DATA'
    blocks -> (cs[ntemp, nwave], species, temps, wn)."""
    species = temps = None
    rows = []
    with open(csfile) as f:
        lines = iter(f.readlines())
    for line in lines:
        line = line.strip()
        if line == '@SPECIES':
            species = next(lines).split()
        elif line == '@TEMPERATURES':
            temps = np.array(next(lines).split(), float)
        elif line == '@DATA':
            break
    for line in lines:
        line = line.strip()
        if line and not line.startswith('#'):
            rows.append(np.array(line.split(), float))
    data = np.array(rows)
    return data[:, 1:].T.copy(), species, temps, data[:, 0].copy()


def second_deriv(yin, xin):
    """src_c/_spline.c:25-74, including its (xin[i+1] - YIN[i-1]) denominator."""
    n = len(yin) - 1
    y2 = np.zeros(n + 1)
    u = np.zeros(max(n, 1))
    for i in range(1, n):
        sig = (xin[i] - xin[i - 1]) / (xin[i + 1] - yin[i - 1])
        p = sig * y2[i - 1] + 2.0
        y2[i] = (sig - 1.0) / p
        u[i] = ((yin[i + 1] - yin[i]) / (xin[i + 1] - xin[i])
                - (yin[i] - yin[i - 1]) / (xin[i] - xin[i - 1]))
        u[i] = (6.0 * u[i] / (xin[i + 1] - xin[i - 1]) - sig * u[i - 1]) / p
    for i in range(n - 1, -1, -1):
        y2[i] = y2[i] * y2[i + 1] + u[i]
    return y2


def splinterp_1D(yin, xin, y2nd, xout, extrap):
    """src_c/_spline.c:95-131 + include/spline.h:6-35 (vectorised; same bracket rule)."""
    xout = np.asarray(xout, float)
    out = np.full(len(xout), float(extrap))
    inside = (xout >= xin[0]) & (xout <= xin[-1])
    x = xout[inside]
    i = np.clip(np.searchsorted(xin, x, side='right') - 1, 0, len(xin) - 2)
    dx = xin[i + 1] - xin[i]
    a = (xin[i + 1] - x) / dx
    b = (x - xin[i]) / dx
    out[inside] = (a * yin[i] + b * yin[i + 1]
                   + ((a * a * a - a) * y2nd[i] + (b * b * b - b) * y2nd[i + 1]) * dx * dx / 6.0)
    return out


class Collision_Induced:
    """CIA table resampled to the model grid at construction (cia.py:20-117); linear in
    temperature per evaluation, on the device."""

    def __init__(self, cia_file=None, *, wn=None, wl=None, table=None):
        absorption, species, temps, tab_wn = table if table is not None else read_cs(cia_file)
        self.cia_file = cia_file
        self.species = list(species)
        self.nspec = len(self.species)
        self.name = 'CIA ' + '-'.join(self.species)
        order = np.argsort(temps)
        absorption = np.asarray(absorption, float)[order]
        self.temps = np.asarray(temps, float)[order]
        self.ntemp = len(self.temps)
        self.tmin, self.tmax = self.temps.min(), self.temps.max()
        if wl is not None and wn is not None:
            raise ValueError('Either provide wl or wn array for CIA, not both')
        if wl is not None:
            wn = 1.0 / (np.asarray(wl) * UM)
        if wn is None:
            self.wn = tab_wn
            cross_section = absorption
        else:
            self.wn = np.asarray(wn, float)
            grid = self.wn[::-1] if self.wn[1] < self.wn[0] else self.wn
            tab = tab_wn[::-1] if tab_wn[1] < tab_wn[0] else tab_wn
            cross_section = np.zeros((self.ntemp, len(self.wn)))
            for j in range(self.ntemp):
                ddev = second_deriv(absorption[j], tab)
                cross_section[j] = splinterp_1D(absorption[j], tab, ddev, grid, 0.0)
            if self.wn[1] < self.wn[0]:
                cross_section = np.fliplr(cross_section)
        self.nwave = len(self.wn)
        self.tab_cross_section = cross_section / AMAGAT**self.nspec
        good = np.where((self.wn >= tab_wn.min()) & (self.wn <= tab_wn.max()))[0]
        self._wn_lo_idx, self._wn_hi_idx = int(good[0]), int(good[-1]) + 1


class Hydrogen_Ion:
    """H- bound-free and free-free opacity (hydrogen_ion.py:17-276; John 1988)."""
    species = ['H', 'e-']

    def __init__(self, wn):
        self.name = 'H- bound-free/free-free'
        self.wn = np.asarray(wn, float)
        wn0 = 6090.5
        c_bf = [152.519, 49.534, -118.858, 92.536, -34.194, 4.982]
        mask = self.wn > wn0
        reduced_wl = 1e-2 * np.sqrt(self.wn[mask] - wn0)
        f_lambda = np.zeros(np.sum(mask))
        for n in range(6):
            f_lambda += c_bf[n] * reduced_wl**n
        self.sigma_bf = np.zeros(len(self.wn))
        self.sigma_bf[mask] = 1.0e-6 * (reduced_wl / self.wn[mask])**3.0 * f_lambda
        # Equation (6): rows multiplying sqrt(5040/T)**(i+2), i = 0..5
        wl = 1e4 / self.wn
        short = [[518.1021, 473.2636, -482.2089, 115.5291],
                 [-734.8666, 1443.4137, -737.1616, 169.6374],
                 [1021.1775, -1977.3395, 1096.8827, -245.649],
                 [-479.0721, 922.3575, -521.1341, 114.243],
                 [93.1373, -178.9275, 101.7963, -21.9972],
                 [-6.4285, 12.3600, -7.0571, 1.5097]]
        long_ = [[2483.346, -3449.889, 2200.040, -696.271, 88.283],
                 [285.827, -1158.382, 2427.719, -1841.400, 444.517],
                 [-2054.291, 8746.523, -13651.105, 8624.970, -1863.864],
                 [2827.776, -11485.632, 16755.524, -10051.530, 2095.288],
                 [-1341.537, 5303.609, -7510.494, 4400.067, -901.788],
                 [208.952, -812.939, 1132.738, -655.020, 132.985]]
        sw = (0.182 < wl) & (wl < 0.3645)
        lw = wl >= 0.3645

        def poly(co, i, x):
            return (co[0][i] * x**2.0 + co[1][i] + co[2][i] / x + co[3][i] / x**2.0
                    + co[4][i] / x**3.0 + co[5][i] / x**4.0)
        self.ff_factors = np.zeros((6, len(self.wn)))
        for i in range(4):
            self.ff_factors[i, sw] = 1.0e-29 * poly(short, i, wl[sw])
        for i in range(5):
            self.ff_factors[i + 1, lw] = 1.0e-29 * poly(long_, i, wl[lw])


class VanderWaals:
    """Alkali resonance doublet, Burrows et al. (2000) (alkali.py:28-262)."""

    def __init__(self, pressure, wn, cutoff):
        self.pressure = np.asarray(pressure, float)
        self.wn = np.asarray(wn, float)
        self.cutoff = cutoff
        self.nlines = len(self.wn0)

    def voigt_det(self, temperature):
        """Voigt value at the detuning distance, [nlayers, nlines] (alkali.py:56-89);
        broadening.Voigt.eval (broadening.py:231-260): Faddeeva function when
        hwhm_L/hwhm_G < 0.1, else the four-term rational approximation."""
        from scipy.special import wofz
        temperature = np.asarray(temperature, float)
        dsigma = self.detuning * (temperature / 500.0)**0.6
        lor = self.lpar * (temperature / 2000.0)**(-0.7) * self.pressure * BAR / 1.01e6
        A = np.array([[-1.2150, -1.3509, -1.2150, -1.3509]]).T
        B = np.array([[1.2359, 0.3786, -1.2359, -0.3786]]).T
        Cc = np.array([[-0.3085, 0.5906, -0.3085, 0.5906]]).T
        D = np.array([[0.0210, -1.1858, -0.0210, 1.1858]]).T
        out = np.zeros((len(temperature), self.nlines))
        ln2 = np.sqrt(np.log(2))
        for j, wn0 in enumerate(self.wn0):
            hg = np.sqrt(2 * K * temperature / (self.mass * AMU)) * wn0 / LS
            x = wn0 + dsigma
            # Faddeeva branch
            sigma = hg / ln2
            z = (x + 1j * lor - wn0) / sigma
            faddeeva = wofz(z).real / (sigma * np.sqrt(np.pi))
            # rational branch (all layers at once; rows = the four terms)
            X = (x - wn0) * ln2 / hg
            Y = lor * ln2 / hg
            V = np.sum((Cc * (Y - A) + D * (X - B)) / ((Y - A)**2 + (X - B)**2), axis=0)
            rational = V * np.sqrt(np.pi * np.log(2.0)) / (np.pi * hg)
            out[:, j] = np.where(lor / hg < 0.1, faddeeva, rational)
        return out

    def detuning_x(self, temperature):
        """Re z of voigt_det's Faddeeva argument, dsigma / sigma, at `temperature`: the smallest
        over the lines.  It grows as T**0.1 (Na: 570 at 40 K, 941 at 6000 K), so its minimum over
        a range of temperatures is at the lowest.  The device form of voigt_det
        (pb_alkali_voigt_det_batch, eval_bands) evaluates w(z) by a continued fraction that needs
        Re z >= BATCH_MIN_X."""
        temperature = float(temperature)
        dsigma = self.detuning * (temperature / 500.0)**0.6
        hg = np.sqrt(2 * K * temperature / (self.mass * AMU)) * np.asarray(self.wn0, float) / LS
        return float(np.min(dsigma * np.sqrt(np.log(2)) / hg))


# the regime of the device's Faddeeva function (csrc/pb_alkali_voigt.h: kFaddeevaMinX)
BATCH_MIN_X = 20.0


class SodiumVdW(VanderWaals):
    def __init__(self, pressure, *, wn=None, wl=None, cutoff=4500.0):
        self.name, self.species = 'sodium_vdw', 'Na'
        self.wn0, self.gf = [16960.87, 16978.07], [0.65464, 1.30918]
        self.lpar, self.Z, self.detuning, self.mass = 0.071, 2.0, 30.0, 22.989769
        super().__init__(pressure, _grid(wn, wl), cutoff)


class PotassiumVdW(VanderWaals):
    def __init__(self, pressure, *, wn=None, wl=None, cutoff=4500.0):
        self.name, self.species = 'potassium_vdw', 'K'
        self.wn0, self.gf = [12988.76, 13046.486], [0.701455, 1.40929]
        self.lpar, self.Z, self.detuning, self.mass = 0.14, 2.0, 20.0, 39.0983
        super().__init__(pressure, _grid(wn, wl), cutoff)


class Continuum:
    """All continuum terms of a run, resident on the device; add(ec, temp, density) is one
    fused pass over ec plus one pass per alkali species.  The batched form
    (TableSpectrum.eval_bands, BatchOperands) adds them all in the interpolation's store."""

    def __init__(self, wn, pressure, models, cloud_models=()):
        """cloud_models: the models of `models` (the same objects) that are CLOUD-type -- what the
        reference lists under `clouds` (pyrat/opacity.py:252-255): in a patchy batch
        (eval_bands(..., f_patchy=...)) their terms make up ec_cloud, the extinction of the cloudy
        column only.  Lecavelier, CCSgray (rank-1 terms) and the Deck (always a property of the
        cloudy column) may be cloud-type; anything else is refused.  Default: none, every term
        goes into ec.  eval() / add() put every term into the one ec whatever is listed here."""
        self.wn_h = np.asarray(wn, float)
        self.pressure = np.asarray(pressure, float)
        self.nwave = len(self.wn_h)
        self.rank1 = [m for m in models if hasattr(m, 'rank1')]
        cloud_models = list(cloud_models or ())
        for m in cloud_models:
            if not any(m is x for x in models):
                raise ValueError('cloud_models: every entry must be one of the models')
            if not isinstance(m, (Lecavelier, CCSgray, Deck)):
                raise ValueError(f"cloud_models: '{getattr(m, 'name', type(m).__name__)}' cannot "
                                 'be cloud-type (Lecavelier, CCSgray and the Deck can)')
        # the rank-1 cloud-type models, in model order
        self.cloud = [m for m in self.rank1 if any(m is c for c in cloud_models)]
        self.cia = [m for m in models if isinstance(m, Collision_Induced)]
        self.hminus = [m for m in models if isinstance(m, Hydrogen_Ion)]
        self.alkali = [m for m in models if isinstance(m, VanderWaals)]
        self.deck = [m for m in models if isinstance(m, Deck)]
        if len(self.cia) > 4 or len(self.hminus) > 1:
            raise ValueError('at most 4 CIA tables and one H- model per Continuum')
        self.cia_tab = [dev(m.tab_cross_section) for m in self.cia]
        self.cia_temps = [dev(m.temps) for m in self.cia]
        if self.hminus:
            self.hm_sigma_bf = dev(self.hminus[0].sigma_bf)
            self.hm_ff = dev(self.hminus[0].ff_factors)
        self._cs_key = None
        self._batch = []         # [(column order, BatchOperands)]
        self._cloud_batch = []   # [(column order, CloudOperands)]
        self._pars_key = None    # default_pars

    # (uploaded on first use: the bookkeeping of a Continuum without tables needs no device)
    @functools.cached_property
    def wn(self):
        return dev(self.wn_h)

    @functools.cached_property
    def pressure_barye(self):
        return dev(self.pressure * BAR)

    @functools.cached_property
    def pressure_d(self):
        return dev(self.pressure)

    def _rank1_cross_sections(self):
        """[nrank1, nwave] on the device; uploaded again only when a model's parameters
        (Lecavelier: scale and exponent) change."""
        key = tuple((id(m), tuple(np.ravel(getattr(m, 'pars', ())).tolist())) for m in self.rank1)
        if key != self._cs_key:
            rows = []
            for m in self.rank1:
                if isinstance(m, Lecavelier):
                    m.calc_cross_section()
                rows.append(np.ones(self.nwave) if isinstance(m, CCSgray) else m.cross_section)
            self._cs_d = dev(np.array(rows).reshape(len(rows), self.nwave))
            self._cs_key = key
        return self._cs_d

    @property
    def species(self):
        """The species of the [nw, L, ncs] continuum density tensor of eval_bands, in model order."""
        return _species_of(self.rank1 + self.cia + self.hminus)

    @property
    def alkali_species(self):
        """The species of the [nw, L, len(alkali)] alkali density tensor of eval_bands: one per
        alkali model, in model order (a species two models share is listed twice)."""
        return [m.species for m in self.alkali]

    @property
    def free_pars(self):
        """(model name, index) of every free parameter, models in order: Lecavelier has 2
        (log10 scale, exponent), CCSgray 3 (log10 cross section, log10 bottom / top pressure)."""
        return [(m.name, i) for m in self.rank1 if isinstance(m, (Lecavelier, CCSgray))
                for i in range(len(m.pars))]

    def _par_offsets(self):
        out, k = [], 0
        for m in self.rank1:
            out.append(k)
            if isinstance(m, (Lecavelier, CCSgray)):
                k += len(m.pars)
        return out

    def current_pars(self):
        """The models' current parameters in free_pars order (host array)."""
        return np.array([float(p) for m in self.rank1 if isinstance(m, (Lecavelier, CCSgray))
                         for p in m.pars], float)

    def default_pars(self):
        """[1, npars] device tensor of current_pars(), shared by BatchOperands and CloudOperands
        (uploaded again only when a model's parameters change)."""
        key = tuple(self.current_pars().tolist())
        if key != self._pars_key:
            self._pars_d = dev(np.array(key, float)).view(1, -1)
            self._pars_key = key
        return self._pars_d

    def is_cloud(self, model):
        return any(model is c for c in self.cloud)

    def batch_unsupported(self, deck=False, alkali=False):
        """Names of the models the batched form does not take.  The alkali doublets unless
        `alkali` is set: eval_bands takes them only together with the walkers' alkali densities
        (its alkali_density argument), and then at most _MAX_ALKALI models with
        _MAX_ALKALI_LINES lines in all (more: every alkali model is listed).  A cloud deck unless
        `deck` is set: eval_bands takes one only together with the walkers' deck pressures (its
        deck_logp argument), which put the bottom of each walker's cloudy column
        (pb_clouds.hip)."""
        fits = len(self.alkali) <= _MAX_ALKALI and \
            sum(m.nlines for m in self.alkali) <= _MAX_ALKALI_LINES
        return [getattr(m, 'name', type(m).__name__)
                for m in ([] if deck else self.deck) + ([] if alkali and fits else self.alkali)]

    def check_alkali_batch(self, tmin):
        """The batched form's conditions on the alkali models, on the host, once per model: its
        pressures are the Continuum's, and Re z of the Faddeeva argument at the lowest temperature
        of the table, `tmin`, is in the regime of the device's continued fraction."""
        for m in self.alkali:
            if not np.array_equal(m.pressure, self.pressure):
                raise ValueError(f"eval_bands: alkali model '{m.name}' has a pressure grid of its "
                                 "own, not the Continuum's; use eval()")
            x = m.detuning_x(tmin)
            if not x >= BATCH_MIN_X:
                raise ValueError(f"eval_bands: alkali model '{m.name}': detuning / Gaussian width "
                                 f'= {x:.3g} at {tmin:.1f} K is below {BATCH_MIN_X:g}, outside '
                                 "the regime of the device's Faddeeva function; use eval()")

    def cloud_operands(self, order=None):
        """The device-side operands of the cloud-type rank-1 models (CloudOperands), in grid order
        or permuted to `order`; cached per order like batch_operands.  None without such models."""
        if not self.cloud:
            return None
        for o, ops in self._cloud_batch:
            if o is order:
                return ops
        ops = CloudOperands(self, order)
        self._cloud_batch = [b for b in self._cloud_batch if b[0] is None] + [(order, ops)]
        return ops

    def batch_operands(self, order=None):
        """The device-side operands for eval_bands (BatchOperands), in grid order or permuted to
        `order` (a column order of TableSpectrum.set_column_order); cached per order."""
        for o, ops in self._batch:
            if o is order:
                return ops
        ops = BatchOperands(self, order)
        # (grid order and the latest column order are kept)
        self._batch = [b for b in self._batch if b[0] is None] + [(order, ops)]
        return ops

    def add(self, ec, temperature, density):
        """ec[L,W] (device, float64) += every term.  temperature[L] and the number
        densities {species: n[L]} (molecules cm-3) are host arrays: L values each; they
        travel to the device in ONE packed upload per call."""
        temperature = np.asarray(temperature, float)
        nlayers = len(temperature)
        assert ec.shape == (nlayers, self.nwave) and ec.is_contiguous()
        for m in self.cia:
            if np.any(temperature < m.tmin) or np.any(temperature > m.tmax):
                raise ValueError('Invalid temperature, values must be in the '
                                 f'{m.tmin:.1f}-{m.tmax:.1f} K range')
        nr1, ncia = len(self.rank1), len(self.cia)
        # per-layer factors, packed: temperature | rank-1 | CIA | H- | alkali densities
        parts = [temperature]
        parts += [np.asarray(m.rank1(self.pressure, temperature, density)[1], float)
                  for m in self.rank1]
        parts += [np.prod([density[s] for s in m.species], axis=0) for m in self.cia]
        if self.hminus:
            parts.append(np.asarray(density['H'], float) * np.asarray(density['e-'], float))
        parts += [np.asarray(density[m.species], float) for m in self.alkali]
        # ... | the alkali models' Voigt values at the detuning distance [nlayers, nlines] each
        vds = [np.ascontiguousarray(m.voigt_det(temperature), float).ravel() for m in self.alkali]
        packed = dev(np.concatenate([np.broadcast_to(p, nlayers) for p in parts] + vds))
        row = [packed[i * nlayers:(i + 1) * nlayers] for i in range(len(parts))]
        temp_d = row[0]
        f_d = packed[nlayers:(1 + nr1) * nlayers] if nr1 else None
        cia_f_d = packed[(1 + nr1) * nlayers:(1 + nr1 + ncia) * nlayers] if ncia else None
        nxt = 1 + nr1 + ncia
        cs_d = self._rank1_cross_sections() if nr1 else None
        tabs = (C.c_void_p * max(ncia, 1))(*[t.data_ptr() for t in self.cia_tab])
        temps = (C.c_void_p * max(ncia, 1))(*[t.data_ptr() for t in self.cia_temps])
        ntemp = np.array([m.ntemp for m in self.cia] or [0], np.int32)
        lo = np.array([m._wn_lo_idx for m in self.cia] or [0], np.int32)
        hi = np.array([m._wn_hi_idx for m in self.cia] or [0], np.int32)
        hm = (None, None, None)
        if self.hminus:
            hm = (self.hm_sigma_bf, self.hm_ff, row[nxt])
            nxt += 1
        if nr1 or ncia or self.hminus:
            call('pb_continuum', _ptr(ec), _ptr(self.wn), _ptr(temp_d), nlayers, self.nwave,
                 nr1, _ptr(cs_d), _ptr(f_d), ncia,
                 C.cast(tabs, C.c_void_p) if ncia else None,
                 C.cast(temps, C.c_void_p) if ncia else None,
                 hptr(ntemp), hptr(lo), hptr(hi), _ptr(cia_f_d), _ptr(hm[0]), _ptr(hm[1]),
                 _ptr(hm[2]), _stream())
        keep = [packed]
        vd_at = len(parts) * nlayers
        for ia, m in enumerate(self.alkali):
            vd = packed[vd_at:vd_at + len(vds[ia])]
            vd_at += len(vds[ia])
            dens_d = row[nxt + ia]
            wn0, gf = np.array(m.wn0, float), np.array(m.gf, float)
            call('pb_alkali_cross_section', _ptr(ec), _ptr(self.pressure_barye), _ptr(self.wn),
                 _ptr(temp_d), _ptr(vd), float(m.detuning), float(m.mass), float(m.lpar),
                 float(m.Z), float(m.cutoff), hptr(wn0), hptr(gf), m.nlines, _ptr(dens_d),
                 nlayers, self.nwave, _stream())
        del keep        # stream-ordered allocator: safe to release after the launches
        return ec


# ---------------------------------------------------------------------------------------------
# Batched form (TableSpectrum.eval_bands): every walker has its own temperatures, densities and
# free continuum parameters; the terms are added by the batched interpolation before it stores ec
# (pb_interp_ec_batch_cont), in the order of Continuum.add.
# ---------------------------------------------------------------------------------------------
_MAX_RANK1, _MAX_CIA = constant('PB_CONT_MAX_RANK1'), constant('PB_CONT_MAX_CIA')
_MAX_ALKALI, _MAX_ALKALI_LINES = (constant('PB_CONT_MAX_ALKALI'),
                                  constant('PB_CONT_MAX_ALKALI_LINES'))
ContBatchStruct = struct('pb_cont_batch')


class BatchOperands:
    """The device-side operands of a Continuum for pb_interp_ec_batch_cont, every per-sample one
    (Rayleigh cross sections, CIA rows and validity mask, H- rows, wn) in one column order.  The
    alkali models' constants are carried along; they take part in a call that has the walkers'
    alkali densities (args(..., alkali_density))."""

    def __init__(self, cont, order=None):
        idx = None if order is None else torch.as_tensor(order, device='cuda').to(torch.int64)

        def cols(t):
            return t.contiguous() if idx is None else t.index_select(-1, idx).contiguous()
        species = cont.species
        st = ContBatchStruct()
        keep = []
        # (cloud-type models are not part of ec: CloudOperands; the parameter offsets are those of
        # the full list, the walkers' parameter rows do not change with what is cloud-type)
        clear = [(model, off) for model, off in zip(cont.rank1, cont._par_offsets())
                 if not cont.is_cloud(model)]
        st.nrank1 = len(clear)
        offsets = [off for _, off in clear]
        for m, (model, _) in enumerate(clear):
            if isinstance(model, Kurucz):
                st.rank1_kind[m] = 0
                st.rank1_species[m] = species.index(model.species)
                cs = cols(dev(model.cross_section))
                keep.append(cs)
                st.rank1_cs_d[m] = cs.data_ptr()
            else:
                st.rank1_kind[m] = 1 if isinstance(model, Lecavelier) else 2
                st.rank1_par[m] = offsets[m]
                st.rank1_s0[m] = float(model.s0)
                st.rank1_l0[m] = float(getattr(model, 'l0', 0.0))
                pr = dev(model.pressure)
                keep.append(pr)
                st.rank1_pressure_d[m] = pr.data_ptr()
        st.ncia = len(cont.cia)
        mask = np.zeros(cont.nwave, np.uint8)
        for c, model in enumerate(cont.cia):
            tab = cols(cont.cia_tab[c])
            keep += [tab, cont.cia_temps[c]]
            st.cia_tab_d[c] = tab.data_ptr()
            st.cia_temps_d[c] = cont.cia_temps[c].data_ptr()
            st.cia_ntemp[c] = model.ntemp
            st.cia_nspec[c] = len(model.species)
            for j, sp in enumerate(model.species):
                st.cia_species[c][j] = species.index(sp)
            mask[model._wn_lo_idx:model._wn_hi_idx] |= np.uint8(1 << c)
        self.mask = cols(dev(mask, torch.int64).to(torch.uint8))
        st.cia_mask_d = self.mask.data_ptr()
        st.hminus = len(cont.hminus)
        if cont.hminus:
            st.hm_species[0] = species.index('H')
            st.hm_species[1] = species.index('e-')
            self.hm_sigma_bf = cols(cont.hm_sigma_bf)
            self.hm_ff = cols(cont.hm_ff)
            st.hm_sigma_bf_d = self.hm_sigma_bf.data_ptr()
            st.hm_ff_d = self.hm_ff.data_ptr()
        self.wn = cols(cont.wn)
        st.wn_d = self.wn.data_ptr()
        st.ncs = len(species)
        st.npars = len(cont.free_pars)
        self._keep = keep
        self.struct = st
        self.ncs, self.npars = len(species), len(cont.free_pars)
        self.nlec = sum(isinstance(m, Lecavelier) for m, _ in clear)
        self.cont = cont
        # the alkali models (None: more than the batched form takes)
        self.nalkali = None
        if not cont.batch_unsupported(deck=True, alkali=True):
            self.nalkali = len(cont.alkali)
            for m, model in enumerate(cont.alkali):
                st.alkali_nlines[m] = model.nlines
                for j in range(model.nlines):
                    st.alkali_wn0[m][j] = float(model.wn0[j])
                    st.alkali_gf[m][j] = float(model.gf[j])
                st.alkali_detuning[m] = float(model.detuning)
                st.alkali_mass[m] = float(model.mass)
                st.alkali_lpar[m] = float(model.lpar)
                st.alkali_part_func[m] = float(model.Z)
                st.alkali_cutoff[m] = float(model.cutoff)
            if self.nalkali:
                st.alkali_pressure_d = cont.pressure_barye.data_ptr()

    def args(self, density, pars, alkali_density=None):
        """The pb_cont_batch of one call: density[nw, L, ncs], pars[nw, npars] or [1, npars],
        alkali_density[nw, L, nalkali] or None (the alkali models add nothing)."""
        st = self.struct
        st.density_d = density.data_ptr() if density is not None else None
        st.pars_d = pars.data_ptr() if pars is not None else None
        st.pars_stride = 0 if pars is None or pars.shape[0] == 1 else self.npars
        if alkali_density is not None and not self.nalkali:
            raise ValueError('alkali_density: the Continuum has no alkali model, or more than '
                             f'{_MAX_ALKALI} models / {_MAX_ALKALI_LINES} lines in all')
        st.nalkali = self.nalkali if alkali_density is not None else 0
        st.alkali_density_d = alkali_density.data_ptr() if alkali_density is not None else None
        return C.byref(st)

    def work_doubles(self, nlayers, nwave, nwalkers):
        """Scratch of a call, in doubles (with room for the alkali records whether or not the
        call has alkali densities: args() decides that per call)."""
        from ._capi import lib
        self.struct.nalkali = self.nalkali or 0
        return int(lib().pb_interp_ec_batch_cont_work_doubles(C.byref(self.struct), nlayers,
                                                              nwave, nwalkers))


_MAX_CLOUD = constant('PB_CLOUD_MAX')
CloudTermsStruct = struct('pb_cloud_terms')
CloudModelsStruct = struct('pb_cloud_models')


def cloud_terms(cloud_cs, cloud_f):
    """pb_cloud_terms from explicit factors: cloud_cs[nr, W] (one row per term for all walkers) or
    [nr, nw, W] (a row per walker), cloud_f[nw, L, nr], device tensors.  -> (struct, keep-alive)."""
    nr = cloud_f.shape[-1]
    if not 1 <= nr <= _MAX_CLOUD:
        raise ValueError(f'1 ... {_MAX_CLOUD} rank-1 cloud terms, got {nr}')
    if cloud_cs.shape[0] != nr or cloud_cs.dim() not in (2, 3) or \
            (cloud_cs.dim() == 3 and cloud_cs.shape[1] != cloud_f.shape[0]):
        raise ValueError(f'cloud_cs must have shape [{nr}, W] or [{nr}, {cloud_f.shape[0]}, W], '
                         f'got {tuple(cloud_cs.shape)}')
    cs, f = cloud_cs.contiguous(), cloud_f.contiguous()
    st = CloudTermsStruct()
    st.nr = nr
    for m in range(nr):
        st.cs_d[m] = cs[m].data_ptr()
        st.cs_stride[m] = cs.shape[-1] if cs.dim() == 3 else 0
    st.f_d = f.data_ptr()
    return st, (cs, f)


class CloudOperands:
    """The cloud-type rank-1 models of a Continuum for pb_cloud_plan: per batch it writes their
    factors f[nw, L, nr] and the Lecavelier rows [nlec, nw, W] (in one column order) from the
    walkers' parameters, on the device."""

    def __init__(self, cont, order=None):
        idx = None if order is None else torch.as_tensor(order, device='cuda').to(torch.int64)
        self.wn = cont.wn if idx is None else cont.wn.index_select(0, idx).contiguous()
        st = CloudModelsStruct()
        self._keep = []
        pairs = [(model, off) for model, off in zip(cont.rank1, cont._par_offsets())
                 if cont.is_cloud(model)]
        if len(pairs) > _MAX_CLOUD:
            raise ValueError(f'at most {_MAX_CLOUD} cloud-type rank-1 models')
        st.nr = len(pairs)
        for m, (model, off) in enumerate(pairs):
            st.kind[m] = 1 if isinstance(model, Lecavelier) else 2
            st.par[m] = off
            st.s0[m] = float(model.s0)
            st.l0[m] = float(getattr(model, 'l0', 0.0))
            pr = dev(model.pressure)
            self._keep.append(pr)
            st.pressure_d[m] = pr.data_ptr()
        self.struct = st
        self.kinds = [st.kind[m] for m in range(st.nr)]
        self.nr, self.nlec = st.nr, self.kinds.count(1)
        self.npars = len(cont.free_pars)
        self.cont = cont

    def plan(self, temps, pars):
        """temps[nw, L], pars[nw, npars] / [1, npars] / None (the models' current parameters)
        -> (pb_cloud_terms struct, keep-alive tensors) of this batch."""
        from ._capi import call
        nw, nlayers = temps.shape
        nwave = self.wn.shape[0]
        if pars is None:
            pars = self.cont.default_pars()
        pars = pars.contiguous()
        f = torch.empty((nw, nlayers, self.nr), dtype=torch.float64, device=temps.device)
        rows = torch.empty((max(self.nlec, 1), nw, nwave), dtype=torch.float64,
                           device=temps.device) if self.nlec else None
        temps = temps.contiguous()
        call('pb_cloud_plan', f.data_ptr(), None if rows is None else rows.data_ptr(),
             C.byref(self.struct), temps.data_ptr(), pars.data_ptr(),
             0 if pars.shape[0] == 1 else self.npars, self.wn.data_ptr(), nlayers, nwave, nw,
             torch.cuda.current_stream().cuda_stream)
        st = CloudTermsStruct()
        st.nr = self.nr
        j = 0
        for m, kind in enumerate(self.kinds):
            if kind == 1:
                st.cs_d[m] = rows[j].data_ptr()
                st.cs_stride[m] = nwave
                j += 1
            else:
                st.cs_d[m] = None            # (CCSgray: a row of ones)
                st.cs_stride[m] = 0
        st.f_d = f.data_ptr()
        return st, (f, rows, temps, pars)


def deck_state(pressure, logp, radius, temps):
    """NumPy mirror of pb_deck_state_batch: the state of an opaque deck at 10**logp[w] bar for every
    walker, by Deck.calc_extinction_coefficient's rule (gray.py:129-150).  pressure[L] (bar),
    logp[nw], radius[nw or 1, L], temps[nw, L] -> (itop int32[nw], rsurf[nw], tsurf[nw]).
    rsurf / tsurf are CLAMPED to the end values when the deck lies outside the pressure grid (the
    reference's interp1d raises there); a NaN pressure gives itop = L - 1 and NaN."""
    pressure = np.asarray(pressure, float)
    logp = np.atleast_1d(np.asarray(logp, float))
    temps = np.atleast_2d(np.asarray(temps, float))
    radius = np.atleast_2d(np.asarray(radius, float))
    nw, nlayers = len(logp), len(pressure)
    itop = np.empty(nw, np.int32)
    rsurf, tsurf = np.empty(nw), np.empty(nw)
    for w in range(nw):
        ptop = 10**logp[w]
        if ptop >= pressure[-1] or np.isnan(ptop):
            itop[w] = nlayers - 1
        elif ptop < pressure[0]:
            itop[w] = min(1, nlayers - 1)
        else:
            itop[w] = int(np.where(pressure >= ptop)[0][0])
        if np.isnan(ptop):                 # (np.interp returns the node's value at one layer)
            rsurf[w] = tsurf[w] = np.nan
            continue
        rsurf[w] = np.interp(ptop, pressure, radius[w if radius.shape[0] > 1 else 0])
        tsurf[w] = np.interp(ptop, pressure, temps[w])
    return itop, rsurf, tsurf


def _species_of(models):
    out = []
    for m in models:
        names = ([m.species] if isinstance(m, Kurucz) else list(m.species)
                 if isinstance(m, (Collision_Induced, Hydrogen_Ion)) else [])
        out += [s for s in names if s not in out]
    return out
