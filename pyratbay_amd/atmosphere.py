"""Atmospheres from retrieval parameters: what Atmosphere.calc_profiles
(pyratbay/pyrat/atmosphere.py:399-526) makes of the parameter vector eval() maps
(pyrat/pyrat_obj.py:258-275) -- T(p) model, VMR models and the bulk balance, ideal-gas density,
mean molecular mass, hydrostatic radius.

Two forms of the same arithmetic:
  * host forms in plain NumPy with the reference's names (atm_models.py; every name of that
    module is a name of this one too: atmosphere.Guillot, atmosphere.vmr_scale, ...);
  * WalkerAtmosphere.evaluate: params[nw, npar] -> the device tensors TableSpectrum.eval_bands
    takes, nothing read back.  Where a walker's VMRs come from is one object the constructor
    picks: _FreeVmr (base VMR, Iso / Scale / Slant models, bulk balance, qcap: one launch of
    pb_walker_atmosphere, csrc/pb_atmosphere.hip) or, with chemistry=ChemNetwork(...)
    (chemistry.py), _EquilibriumVmr (the equilibrium of every layer at the walker's [M/H], [X/H]
    and X/Y: three launches).  Each owns its constructor checks, its host step, its part of
    pb_atm_model and its launches.
"""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from ._capi import call, constant, struct
from ._device import dev, require_gpu
from .atm_models import (  # noqa: F401 -- imported back: every earlier spelling keeps working
    BAR, E2_CUTOFF, EULER, G_GRAV, K_BOLTZ, N_AVOGADRO, TCEA, Guillot, IsoVMR, Isothermal, Madhu,
    MetalEquil, RatioEquil, ScaleEquil, ScaleVMR, SlantVMR, balance, correlate_nearest, expn2,
    gaussian_weights, hydro_g, hydro_m, ideal_gas_density, mean_weight, qcapcheck, ratio,
    vmr_scale)

MAX_SPECIES, MAX_VMR = constant('PB_ATM_MAX_SPECIES'), constant('PB_ATM_MAX_VMR')
MAX_BULK, MAX_LAYERS = constant('PB_ATM_MAX_BULK'), constant('PB_ATM_MAX_LAYERS')
# isotope ratios of the table's slots (isotopes.py): labelled slots, fillers of one fill slot
MAX_ISO_SLOTS, MAX_ISO_FILLERS = constant('PB_ISO_MAX_SLOTS'), constant('PB_ISO_MAX_FILLERS')
REJECT_TEMP, REJECT_MADHU = constant('PB_ATM_REJECT_TEMP'), constant('PB_ATM_REJECT_MADHU')
REJECT_QCAP, REJECT_REFPRESSURE = (constant('PB_ATM_REJECT_QCAP'),
                                   constant('PB_ATM_REJECT_REFPRESSURE'))
REJECT_DIVERGENT = constant('PB_ATM_REJECT_DIVERGENT')
REJECT_ISOTOPE = constant('PB_ISO_REJECT')  # a non-finite or negative isotope ratio (isotopes.py)
# an equilibrium cell without VMRs (chemistry.py); the isotope ratios share the mask: its bit is
# the next one
REJECT_CHEMISTRY = constant('PB_ATM_REJECT_CHEMISTRY')
REJECT_NAMES = {REJECT_TEMP: 'temperature <= 0 or not finite', REJECT_MADHU: 'madhu log_p1 > log_p3',
                REJECT_QCAP: 'trace abundances above qcap',
                REJECT_REFPRESSURE: 'reference pressure outside the grid',
                REJECT_DIVERGENT: 'divergent hydro_m profile, or a radius <= 0 or not finite',
                REJECT_ISOTOPE: 'a negative or non-finite isotope ratio',
                REJECT_CHEMISTRY: 'equilibrium chemistry: not converged, a temperature outside '
                                  'the Gibbs table, or an element ratio <= 0'}


# ---------------------------------------------------------------------------------------------
# The batched form
# ---------------------------------------------------------------------------------------------
AtmModelStruct = struct('pb_atm_model')


Profiles = collections.namedtuple(
    'Profiles', 'temps dens radius mm continuum_density alkali_density reject')

_TMODELS = {Isothermal: 0, Guillot: 1, Madhu: 2}
_SCALARS = ('rplanet', 'log_refpressure', 'mplanet')


def _chemistry():
    from . import chemistry
    return chemistry


def _check_free_model(atm, model, taken):
    """What either composition path asks of a model that sets the column of one species: its
    class, a species of the atmosphere that no bulk and no earlier model has (`taken`, which
    gains it), the atmosphere's pressure grid."""
    if getattr(model, 'type', 'free') != 'free' or \
            not isinstance(model, (IsoVMR, ScaleVMR, SlantVMR)):
        raise ValueError(
            f'VMR model {getattr(model, "name", type(model).__name__)}: '
            'equilibrium-chemistry and hybrid models are not supported without '
            'chemistry=ChemNetwork(...), only IsoVMR, ScaleVMR and SlantVMR')
    if model.species not in atm.species:
        raise ValueError(f'VMR model {model.name}: species {model.species} is not in the '
                         f'atmosphere ({atm.species})')
    if model.species in taken:
        raise ValueError(f'VMR model {model.name}: species {model.species} is a bulk '
                         'species or has a model already')
    taken.add(model.species)
    if not np.array_equal(np.asarray(model.pressure, float), atm.pressure):
        raise ValueError(f'VMR model {model.name} is defined on another pressure grid')


class _FreeVmr:
    """Free VMRs: the base VMR, the IsoVMR / ScaleVMR / SlantVMR models, the bulk balance and the
    qcap cap, all inside the one launch of pb_walker_atmosphere.  The constructor sets the
    atmosphere's base_vmr, bulk, ibulk, bratio, invsrat and qcap."""

    def __init__(self, atm, base_vmr, bulk, qcap):
        self.atm = atm
        L, S = atm.nlayers, atm.nspecies
        atm.base_vmr = np.ascontiguousarray(base_vmr, float)
        if atm.base_vmr.shape != (L, S):
            raise ValueError(f'base_vmr must have shape {(L, S)}, got {atm.base_vmr.shape}')
        atm.bulk = [str(b) for b in bulk]
        if not 1 <= len(atm.bulk) <= MAX_BULK or len(set(atm.bulk)) != len(atm.bulk):
            raise ValueError(f'bulk: 1 ... {MAX_BULK} distinct species, got {atm.bulk}')
        for b in atm.bulk:
            if b not in atm.species:
                raise ValueError(f'bulk species {b} is not in the atmosphere ({atm.species})')
        atm.ibulk = [atm.species.index(b) for b in atm.bulk]
        atm.bratio, atm.invsrat = ratio(atm.base_vmr, atm.ibulk)
        atm.qcap = None if qcap is None else float(qcap)

    def check_models(self):
        taken = set(self.atm.bulk)
        for model in self.atm.vmr_models:
            _check_free_model(self.atm, model, taken)

    def host_vmr(self, params, temp):
        """-> vmr[L, S], its reject bits, whether a layer is without VMRs (never)."""
        a = self.atm
        pars = [params[o:o + m.npars] for o, m in zip(a.vmr_par, a.vmr_models)]
        vmr = vmr_scale(a.base_vmr, a.species, a.vmr_models, pars, a.bulk, iscale=a.iscale,
                        ibulk=a.ibulk, bratio=a.bratio, invsrat=a.invsrat)
        return vmr, REJECT_QCAP if qcapcheck(vmr, a.qcap, a.ibulk) else 0, False

    def scalars(self, st):
        a = self.atm
        st.nvmr = len(a.vmr_models)
        for i, model in enumerate(a.vmr_models):
            st.vmr_kind[i], st.vmr_species[i] = model.kind, a.iscale[i]
            st.vmr_par[i] = a.vmr_par[i]
        st.nbulk = len(a.ibulk)
        for j, i in enumerate(a.ibulk):
            st.bulk_species[j] = i
        st.has_qcap = int(a.qcap is not None)
        st.qcap = a.qcap if a.qcap is not None else 0.0

    def device(self, st, d):
        """Its arrays into d (once) and their pointers into st."""
        a = self.atm
        if 'base_vmr' not in d:
            d['base_vmr'], d['bratio'], d['invsrat'] = (dev(x) for x in
                                                       (a.base_vmr, a.bratio, a.invsrat))
            vmr0 = np.zeros((max(len(a.vmr_models), 1), a.nlayers))
            for i, model in enumerate(a.vmr_models):
                if isinstance(model, ScaleVMR):
                    vmr0[i] = model.vmr0
            d['vmr0'] = dev(vmr0)
        st.vmr0_d, st.base_vmr_d = d['vmr0'].data_ptr(), d['base_vmr'].data_ptr()
        st.bulk_ratio_d, st.invsrat_d = d['bratio'].data_ptr(), d['invsrat'].data_ptr()

    def launch(self, st, params, nw, outputs):
        call('pb_walker_atmosphere', C.byref(st), params.data_ptr(), nw, *outputs)


class _EquilibriumVmr:
    """Equilibrium chemistry on atm.chemistry (a chemistry.ChemNetwork): the VMRs of every layer
    from the walker's [M/H], [X/H] and X/Y, hybrid IsoVMR columns on top; no base VMR, no bulk,
    no cap.  Three launches: pb_walker_temperature, pb_equilibrium_vmr, then
    pb_walker_atmosphere_chem on those VMRs, through buffers kept per nw."""

    def __init__(self, atm, base_vmr, bulk, qcap):
        self.atm, self.net = atm, atm.chemistry
        if atm.species != list(self.net.species):
            raise ValueError(f'chemistry: species must be the network\'s {self.net.species}, '
                             f'got {atm.species}')
        if base_vmr is not None or (bulk is not None and len(bulk)):
            raise ValueError('chemistry: base_vmr and bulk are not taken (pass None): the '
                             'equilibrium gives every VMR, and the reference balances no bulk '
                             'in equilibrium')
        if qcap is not None:
            raise ValueError('chemistry: qcap is not taken (there are no bulk species)')
        atm.base_vmr, atm.bulk, atm.ibulk = None, [], []
        atm.bratio = atm.invsrat = atm.qcap = None
        self._buffers = {}

    def check_models(self):
        models = self.atm.vmr_models
        for model in models:
            if not isinstance(model, (MetalEquil, ScaleEquil, RatioEquil, IsoVMR)):
                raise ValueError(
                    f'VMR model {getattr(model, "name", type(model).__name__)}: with chemistry, '
                    'only MetalEquil, ScaleEquil, RatioEquil and (hybrid) IsoVMR models are '
                    'taken; the reference\'s hybrid is hard-wired to IsoVMR')
            if isinstance(model, ScaleEquil):
                self.net.element_index(model.element)
                if model.element == 'H':
                    raise ValueError('ScaleEquil: [H/H] is no parameter (abundances are relative '
                                     'to hydrogen)')
            if isinstance(model, RatioEquil):
                self.net.ratio_elements(model.pnames[0])
        pnames = [n for m in models for n in m.pnames]
        if len(set(pnames)) != len(pnames):
            raise ValueError(f'VMR models: a parameter is named twice ({pnames})')
        limit = _chemistry().MAX_ELEMENTS
        for cls in (ScaleEquil, RatioEquil):
            if sum(isinstance(m, cls) for m in models) > limit:
                raise ValueError(f'at most {limit} {cls.__name__} models')
        taken = set()
        for model in models:
            if isinstance(model, IsoVMR):
                _check_free_model(self.atm, model, taken)
                self.net.refuse_charged_hybrid(self.net.species.index(model.species))

    @functools.cached_property
    def columns(self):
        """The parameter columns as ChemNetwork.model_struct takes them (filed on first use, from
        the atmosphere's vmr_par and iscale): par_metal, scales, ratios, hybrids."""
        a, net = self.atm, self.net
        eq = dict(par_metal=-1, scales=[], ratios=[], hybrids=[])
        for model, col, isp in zip(a.vmr_models, a.vmr_par, a.iscale):
            if isinstance(model, MetalEquil):
                eq['par_metal'] = col
            elif isinstance(model, ScaleEquil):
                eq['scales'].append((net.element_index(model.element), col))
            elif isinstance(model, RatioEquil):
                eq['ratios'].append(net.ratio_elements(model.pnames[0]) + (col,))
            else:
                eq['hybrids'].append((isp, col))
        return eq

    def equilibrium_host(self, params, temp):
        net, eq = self.net, self.columns
        metallicity = None if eq['par_metal'] < 0 else params[eq['par_metal']]
        e_scale = {net.elements[j]: params[col] for j, col in eq['scales']}
        e_ratio = {f'{net.elements[x]}/{net.elements[y]}': params[col]
                   for x, y, col in eq['ratios']}
        b = net.element_abundances_host(metallicity, e_scale, e_ratio)
        equil, _, status = net.equilibrium_host(temp, self.atm.pressure, b)
        vmr = equil.copy()
        for isp, col in eq['hybrids']:
            column = net.hybrid_host(equil, self.atm.species[isp], params[col])
            vmr[:, isp] = np.where(status > 0, column, 0.0)
        return vmr, status

    def host_vmr(self, params, temp):
        """-> vmr[L, S], its reject bits, whether a layer is without VMRs."""
        vmr, status = self.equilibrium_host(params, temp)
        reject = REJECT_CHEMISTRY \
            if np.any((status < 0) & (status != _chemistry().STATUS_REJECTED)) else 0
        # a cell without VMRs has no mean mass: the walker is rejected already (this bit, or
        # the temperature's), and its radius is not judged
        return vmr, reject, bool(np.any(status < 0))

    def scalars(self, st):
        """Nothing: every VMR comes from the equilibrium launch (nvmr = nbulk = has_qcap = 0)."""

    def device(self, st, d):
        """The network's own struct; st.base_vmr_d is set per call (buffers)."""
        self.chem_struct = self.net.bound_struct(d['pressure'], self.atm.npar, **self.columns)
        self._buffers = {}

    def buffers(self, nw, device):
        """The buffers between the three launches of a call, kept per nw so that a call with
        `out` allocates nothing: the temperatures as formed, the equilibrium VMRs and cell
        statuses, and the atmosphere's struct pointing at those VMRs."""
        key = (nw, str(device))
        if key not in self._buffers:
            L, S = self.atm.nlayers, self.atm.nspecies
            temps = torch.empty((nw, L), dtype=torch.float64, device=device)
            vmr = torch.empty((nw, L, S), dtype=torch.float64, device=device)
            status = torch.empty((nw, L), dtype=torch.int32, device=device)
            st = AtmModelStruct.from_buffer_copy(self.atm._struct)
            st.base_vmr_d, st.base_vmr_stride = vmr.data_ptr(), L * S
            self._buffers[key] = (temps, vmr, status, st)
        return self._buffers[key]

    def launch(self, st, params, nw, outputs):
        temps, vmr, status, cst = self.buffers(nw, params.device)
        stream = outputs[-1]
        call('pb_walker_temperature', C.byref(st), params.data_ptr(), nw, temps.data_ptr(),
             stream)
        call('pb_equilibrium_vmr', C.byref(self.chem_struct), temps.data_ptr(),
             params.data_ptr(), nw, vmr.data_ptr(), status.data_ptr(), stream)
        call('pb_walker_atmosphere_chem', C.byref(cst), params.data_ptr(), nw,
             status.data_ptr(), *outputs)


class WalkerAtmosphere:
    """params[nw, npar] -> the atmospheres of nw walkers, on the device: one launch with free
    VMRs, three with chemistry.

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
        # where the VMRs come from: the one place that asks (it sets base_vmr ... qcap)
        self._composition = (_FreeVmr if chemistry is None else _EquilibriumVmr)(
            self, base_vmr, bulk, qcap)

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
        self._composition.check_models()
        self.iscale = [self.species.index(m.species) if hasattr(m, 'species') else -1
                       for m in self.vmr_models]

        names = list(tmodel.pnames)
        self.tpar = slice(0, tmodel.npars)
        self.vmr_par = []
        for model in self.vmr_models:
            self.vmr_par.append(len(names))
            names += list(model.pnames)
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

        self._table_species = None
        self._cont_species, self._alk_species = [], []
        self._maps = None
        self._dev = None
        self._struct = None
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
        vmr, bits, no_vmr = self._composition.host_vmr(params, temp)
        reject |= bits
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
        return self._composition.equilibrium_host(params, temp)

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
        require_gpu()
        if self._dev is None:
            d = {}
            d['pressure'] = dev(self.pressure)
            d['log10p'] = dev(np.log10(self.pressure))
            d['lnp'] = dev(np.log(self.pressure))
            d['mass'] = dev(self.mol_mass)
            d['base_radius'] = dev(self.base_radius)
            if isinstance(self.tmodel, Madhu):
                d['weights'] = dev(self.tmodel.weights)
            self._dev = d
        d = self._dev
        for key, idx in zip(('tab_map', 'cont_map', 'alk_map'), self._index_maps()):
            d[key] = torch.tensor(idx if idx else [0], dtype=torch.int32, device='cuda')
        st = self.model_struct()
        st.madhu_weights_d = d['weights'].data_ptr() if 'weights' in d else None
        self._composition.device(st, d)
        st.pressure_d = d['pressure'].data_ptr()
        st.log10p_d, st.lnp_d = d['log10p'].data_ptr(), d['lnp'].data_ptr()
        st.mass_d, st.base_radius_d = d['mass'].data_ptr(), d['base_radius'].data_ptr()
        st.tab_map_d = d['tab_map'].data_ptr()
        st.cont_map_d = d['cont_map'].data_ptr() if self._cont_species else None
        st.alk_map_d = d['alk_map'].data_ptr() if self._alk_species else None
        self._struct = st

    def _chemistry_buffers(self, nw, device):
        """With chemistry: (temps, vmr, status, struct) of _EquilibriumVmr.buffers."""
        return self._composition.buffers(nw, device)

    def equilibrium_launch(self, nw, device):
        """With chemistry, for tools that time or inspect the equilibrium launch alone: what
        pb_equilibrium_vmr reads and writes in an evaluate() of nw walkers on `device`, as
        chemistry.equilibrium_vmr names it -- dict(temps[nw, L], pressure[L], vmr[nw, L, S],
        status[nw, L]: device tensors, the three per-nw ones those evaluate() reuses; columns:
        par_metal, scales, ratios, hybrids).  Needs bind() first."""
        if self._struct is None:
            self._build_struct()
        temps, vmr, status, _ = self._composition.buffers(nw, device)
        return dict(temps=temps, pressure=self._dev['pressure'], vmr=vmr, status=status,
                    columns=self._composition.columns)

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
        self._composition.scalars(st)
        st.rmodel = 0 if self.rmodel == 'hydro_m' else 1
        st.mplanet = float(self.mplanet or 0.0)
        st.gplanet = float(self.gplanet or 0.0)
        st.rplanet = float(self.rplanet or 0.0)
        st.refpressure = float(self.refpressure or 0.0)
        st.par_rplanet = self.par_scalar['rplanet']
        st.par_log_refpressure = self.par_scalar['log_refpressure']
        st.par_mplanet = self.par_scalar['mplanet']
        st.ntab = len(self._table_species or [])
        st.ncont, st.nalk = len(self._cont_species), len(self._alk_species)
        return st

    # ----------------------------------------------------------------------------- evaluate
    def evaluate(self, params, out=None):
        """params[nw, npar] (float64 device tensor, columns in `free` order) -> Profiles of
        device tensors: temps[nw, L], dens[nw, L, ntab], radius[nw, L], mm[nw, L],
        continuum_density[nw, L, ncont] / alkali_density[nw, L, nalk] (None without such
        species), reject[nw] (int32 bit mask).  One launch with free VMRs, three with chemistry
        (the class docstring names them); nothing read back, no allocation when `out` (a Profiles
        of an earlier call with the same nw) is given: capturable into a graph.  Shape and dtype
        are checked before any HIP call."""
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
        # the fields of Profiles in order: shape (None: no such output) and element type
        want = [((nw, L), torch.float64), ((nw, L, st.ntab), torch.float64),
                ((nw, L), torch.float64), ((nw, L), torch.float64),
                ((nw, L, st.ncont) if st.ncont else None, torch.float64),
                ((nw, L, st.nalk) if st.nalk else None, torch.float64), ((nw,), torch.int32)]
        if out is None:
            out = Profiles(*[None if shape is None else
                             torch.empty(shape, dtype=dtype, device=params.device)
                             for shape, dtype in want])
        else:
            for name, t, (shape, dtype) in zip(Profiles._fields, out, want):
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
        self._composition.launch(st, params, nw, outputs)
        return out
