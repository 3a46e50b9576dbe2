"""The front end of the batched loop towards the sampler: Retrieval takes what a sampler holds,
theta[nw, nfree], and returns one log-posterior (or log-likelihood, or prior-transformed vector)
per walker with launches only.

It restates three places of the reference: the `retrieval_params` block, the name resolution and
the index maps of pyrat/retrieval.py:77-121, 167-284; their use in every eval()
(pyrat_obj.py:258-297); Loglike's free / fixed / shared rule by pstep and the priors
(tools/retrieval_tools.py:45-46, 91-93).  mc3 is not part of this package: the NumPy statements
here (expand_host, split_host, log_prior_host, inside_host, prior_transform_host) are the
specification of the kernels in csrc/pb_retrieval.hip.  The sampler that drives the loop is this
package's own (sampler.py: DEMC-zs on the device, csrc/pb_sampler.hip): draw_initial draws from the
priors, sample builds and runs a sampler.DEMC over log_posterior, summary reduces its chain with
model.posterior_summary.  residuals is the same posterior as a residual vector, and optimize runs
optimize.py's batched Levenberg-Marquardt over it (csrc/pb_optimize.hip): the maximum, the
reference's `bestp`, and its Laplace covariance.

DEVIATIONS from the reference:
  * a shared parameter (pstep < 0) whose target is itself shared is refused; the reference copies
    whatever value that slot holds at that moment;
  * a walker outside the bounds (inside == 0) is evaluated at the block's `value` column instead
    of its own row, so that no later kernel sees NaN or out-of-range input; it comes out as -inf
    from log_posterior and as -1e98 from log_likelihood;
  * the Gaussian priors carry no normalisation term;
  * residuals and optimize refuse a retrieval with a free err_scale_* / err_quad_* parameter: its
    objective is not a sum of squares (mc3's least-squares fit has the same limit).
"""
from collections import namedtuple
import ctypes as C

import numpy as np
import torch

from . import table as _table
from ._capi import call, constant
from ._device import _ptr, _stream, dev
from .bands import HiresData
from .continuum import CCSgray, Lecavelier

# pt.u() of atm.runits / atm.mass_units (pyratbay.constants), in cm and g
RUNITS = {'rjup': 7.1492e9, 'rearth': 6.3781e8, 'km': 1.0e5, 'm': 1.0e2, 'cm': 1.0}
MASS_UNITS = {'mjup': 1.8982e30, 'mearth': 5.9724e27, 'kg': 1.0e3, 'gram': 1.0}

MAX_PARAMS, MAX_DESTS = constant('PB_RETRIEVAL_MAX_PARAMS'), constant('PB_RETRIEVAL_MAX_DESTS')
SOLO_PARAMS = ['log_p_ref', 'R_planet', 'M_planet', 'rv_shift', 'f_patchy', 'T_eff',
               'f_dilution']
_CONT_PNAMES = {Lecavelier: ['log_k_ray', 'alpha_ray'],
                CCSgray: ['log_k_gray', 'log_p_top', 'log_p_bot']}
# the destinations with one column come out as [nw]
_SCALAR_DESTS = ('deck_logp', 'f_patchy', 'rv', 'tstar', 'f_dilution')
_SOLO_DESTS = {'log_p_cl': 'deck_logp', 'f_patchy': 'f_patchy', 'rv_shift': 'rv',
               'T_eff': 'tstar', 'f_dilution': 'f_dilution'}
COLUMNS = ('pnames', 'params', 'pmin', 'pmax', 'pstep', 'prior', 'priorlow', 'priorup')

ParsedParams = namedtuple('ParsedParams', COLUMNS)
# What Retrieval.arguments returns: params[nw, npar] for the atmosphere, kw = the per-walker
# keyword tensors of eval_loglike / eval_params, offsets / err_pars (None without such models),
# log_prior[nw], inside[nw] (int32).
RetrievalArguments = namedtuple('RetrievalArguments',
                                'params kw offsets err_pars log_prior inside')


def parse_retrieval_params(block):
    """The `retrieval_params` block (pyrat/retrieval.py:77-121) -> ParsedParams: one line per
    parameter, `name value [pmin pmax pstep [prior priorlow [priorup]]]`: 2, 5, 7 or 8 fields.
    Defaults: pmin = -inf, pmax = +inf, pstep = 0, prior = priorlow = priorup = 0; with 7 fields
    priorup = priorlow.  The eight columns as arrays (a ParsedParams, or a mapping / sequence in
    COLUMNS order) are taken as they are.  Repeated names are refused."""
    if isinstance(block, str):
        lines = [line for line in block.splitlines() if line.strip() != '']
        n = len(lines)
        pnames = []
        params, pstep = np.zeros(n), np.zeros(n)
        pmin, pmax = np.full(n, -np.inf), np.full(n, np.inf)
        prior, priorlow, priorup = np.zeros(n), np.zeros(n), np.zeros(n)
        for i, line in enumerate(lines):
            fields = line.split()
            if len(fields) not in (2, 5, 7, 8):
                raise ValueError('Invalid number of fields for retrieval_params entry\n'
                                 f"'{line}'")
            pnames.append(fields[0])
            params[i] = fields[1]
            if len(fields) >= 5:
                pmin[i], pmax[i], pstep[i] = fields[2:5]
            if len(fields) >= 7:
                prior[i], priorlow[i] = fields[5:7]
                priorup[i] = fields[6] if len(fields) == 7 else fields[7]
        parsed = ParsedParams(pnames, params, pmin, pmax, pstep, prior, priorlow, priorup)
    else:
        cols = [block[k] for k in COLUMNS] if hasattr(block, 'keys') else list(block)
        if len(cols) != len(COLUMNS):
            raise ValueError(f'retrieval_params: the text block, or the eight columns {COLUMNS}')
        pnames = [str(name) for name in cols[0]]
        arrays = [np.array(c, dtype=np.float64) for c in cols[1:]]
        if any(a.shape != (len(pnames),) for a in arrays):
            raise ValueError(f'retrieval_params: every column must have {len(pnames)} entries')
        parsed = ParsedParams(pnames, *arrays)
    names, counts = np.unique(parsed.pnames, return_counts=True)
    if np.any(counts > 1):
        raise ValueError(f'Repeated parameter names: {names[counts > 1]}')
    return parsed


def log_prior_terms(p, prior, priorlow, priorup):
    """The terms of the log-prior of p[..., nfree]: 0 for a uniform parameter (priorlow == 0 and
    priorup == 0, pyrat/retrieval.py:362), else -0.5 ((p - prior) / s)**2 with s = priorlow for
    p < prior, else priorup.  No normalisation term."""
    p = np.asarray(p, float)
    uniform = (priorlow == 0) & (priorup == 0)
    s = np.where(p < prior, priorlow, priorup)
    with np.errstate(all='ignore'):
        terms = -0.5 * ((p - prior) / np.where(uniform, 1.0, s))**2
    return np.where(uniform, 0.0, terms)


def below_split(u, lo, up):
    """u (lo + up) < lo, the side of prior an element of the unit cube falls on, decided exactly:
    the sum lo + up with its rounding error (two-sum), u times that sum with its rounding error
    (Dekker's product: NumPy has no fma), and a difference p - lo that is exact near the split.
    fl(lo / (lo + up)) lies an ulp or two off the split, and a u between the two would be computed
    by the other side's statement: right to first order, but with the rounding of the OTHER
    side's width, a thousand units of eps (|prior| + s (1 + |z|)) where lo = 1000 up.
    u = 0: below; u = 1 and NaN: not below."""
    def halves(a):
        c = 134217729.0 * a                                  # 2^27 + 1: Veltkamp's split
        high = c - (c - a)
        return high, a - high
    with np.errstate(all='ignore'):
        s = lo + up
        t = s - lo
        es = (lo - (s - t)) + (up - t)
        p = u * s
        uh, ul = halves(u)
        sh, sl = halves(s)
        ep = ((uh * sh - p) + uh * sl + ul * sh) + ul * sl
        return (p - lo) + (ep + u * es) < 0.0


def residual_rows_host(obs, theta, inside, model, offsets, err_pars, gauss_index, prior, priorlow,
                       priorup):
    """The statement of pb_lm_residuals: obs, an Observation; theta[nw, nfree]; inside[nw];
    model[nw, ndata]; offsets[nw, noff] and err_pars[nw, nerr] or None (the defaults);
    gauss_index[ngauss], columns of theta; prior, priorlow, priorup [nfree] -> R[nw, ndata +
    ngauss] (Retrieval.residuals_host).  A walker that is not inside, or has a non-finite model
    value, gets a row of +inf."""
    theta = np.asarray(theta, dtype=np.float64)
    model = np.asarray(model, dtype=np.float64)
    ig = np.asarray(gauss_index, dtype=np.int64)
    nw, nd = model.shape
    out = np.full((nw, nd + len(ig)), np.inf)
    ok = (np.asarray(inside) != 0) & np.all(np.isfinite(model), axis=1)
    for w in np.where(ok)[0]:
        data = obs.offset_data_host(None if offsets is None else offsets[w])
        uncert = obs.scale_errors_host(obs.err_defaults if err_pars is None else err_pars[w])
        out[w, :nd] = (data - model[w]) / uncert
        p = theta[w, ig]
        s = np.where(p < prior[ig], priorlow[ig], priorup[ig])
        out[w, nd:] = (p - prior[ig]) / s
    return out


class Retrieval:
    """Retrieval(model, atmosphere, bands, observation, retrieval_params, runits='rjup',
    mass_units='mjup', fixed=None, **eval_kw): model, a TableSpectrum; atmosphere, a bound
    WalkerAtmosphere; bands, a PassBands or a HiresData; observation, an Observation;
    retrieval_params, the reference's text block or its eight columns (parse_retrieval_params);
    eval_kw: whatever else eval_loglike takes that is not per parameter (chunk, streams, ...).

    Names (pyrat/retrieval.py:179-275) and where their values go:
        the T model's and every VMR model's pnames   that column of the atmosphere's params
        R_planet     the atmosphere's free 'rplanet', times runits in cm
        M_planet     the atmosphere's free 'mplanet', times mass_units in g
        log_p_ref    the atmosphere's free 'log_refpressure'
        log_k_ray, alpha_ray                  the Lecavelier columns of continuum_pars
        log_k_gray, log_p_top, log_p_bot      the CCSgray columns of continuum_pars
        iso_<label> (model.isotopes.pnames)   that column of iso_pars (log10 of the isotope ratio
                                              of a table slot, line_sampling.py:282-298)
        log_p_cl -> deck_logp    f_patchy -> f_patchy    rv_shift -> rv
        T_eff -> tstar           f_dilution -> f_dilution
        observation.offset_models -> offsets         observation.err_models -> err_pars
    Every column of a destination that no line names is a constant of the map: fixed[name] (in
    the units of a retrieval_params line), else the objects' current value (the atmosphere's
    base_params, cont.current_pars(), the isotope model's default pars, no offset, the error
    models' defaults); neither: ValueError.

    pstep (tools/retrieval_tools.py:45-46, 91-93): > 0 free; == 0 fixed at `value`; < 0 shared with
    parameter -int(pstep) - 1, which must not be shared itself (DEVIATION, module docstring).

    Priors: a free parameter with priorlow == priorup == 0 is uniform and contributes 0; otherwise
    -0.5 ((p - prior) / s)**2, s = priorlow for p < prior, else priorup -- WITHOUT a normalisation
    term.  A free parameter with a negative or non-finite priorlow or priorup, or with exactly one
    of the two zero, is refused.  inside: every free value is finite and pmin <= p <= pmax; the
    log-prior of a walker that is not inside is -inf, and it is evaluated at the `value` column
    (DEVIATION).

    The *_host methods are NumPy and carry the specification; arguments, log_likelihood,
    log_posterior, prior_transform and bandflux take float64 device tensors, read nothing back and
    put no torch arithmetic on the path (pb_retrieval_map, pb_prior_transform,
    pb_log_posterior)."""

    def __init__(self, model, atmosphere, bands, observation, retrieval_params, runits='rjup',
                 mass_units='mjup', fixed=None, **eval_kw):
        if runits not in RUNITS:
            raise ValueError(f"runits '{runits}': one of {list(RUNITS)}")
        if mass_units not in MASS_UNITS:
            raise ValueError(f"mass_units '{mass_units}': one of {list(MASS_UNITS)}")
        self.model, self.atmosphere, self.bands = model, atmosphere, bands
        self.observation = observation
        self.runits, self.mass_units = runits, mass_units
        self.eval_kw = eval_kw
        parsed = parse_retrieval_params(retrieval_params)
        self.pnames = list(parsed.pnames)
        (self.params, self.pmin, self.pmax, self.pstep, self.prior, self.priorlow,
         self.priorup) = (np.array(a, dtype=np.float64) for a in parsed[1:])
        self.npar = len(self.pnames)

        self.ifree = np.where(self.pstep > 0)[0]
        self.nfree = len(self.ifree)
        if self.nfree == 0:
            raise ValueError('Attempting to compute a log-likelihood for a model with no free '
                             'parameters')
        # the theta column every parameter reads (-1: a constant), Loglike's rule
        self.source = np.full(self.npar, -1, np.int32)
        self.source[self.ifree] = np.arange(self.nfree)
        self.ishare = np.where(self.pstep < 0)[0]
        self.share_target = {}
        for i in self.ishare:
            j = -int(self.pstep[i]) - 1
            if not 0 <= j < self.npar:
                raise ValueError(f"'{self.pnames[i]}' (pstep {self.pstep[i]:g}) is shared with "
                                 f'parameter {j}: there are {self.npar}')
            if self.pstep[j] < 0:
                raise ValueError(f"'{self.pnames[i]}' is shared with '{self.pnames[j]}', which is "
                                 'shared itself: share it with the parameter that one follows')
            self.share_target[int(i)] = j
            self.source[i] = self.source[j]
        # the constant of a parameter that reads no theta column
        self.constant = self.params.copy()
        for i, j in self.share_target.items():
            self.constant[i] = self.params[j]
        self.value_free = self.params[self.ifree].copy()
        self._check_prior_widths()

        self._resolve(dict(fixed or {}))
        self._device = None

    # ------------------------------------------------------------------ name resolution
    def _slots(self):
        """{name: (destination, column, unit factor)} of every name the objects can take, and
        {name: reason} of the names they know but cannot take."""
        model, atm, obs, bands = self.model, self.atmosphere, self.observation, self.bands
        cont = getattr(model, 'continuum', None)
        rt_path = getattr(model, 'rt_path', None)
        slots, refused = {}, {}
        for name, scalar, factor in (('log_p_ref', 'log_refpressure', 1.0),
                                     ('R_planet', 'rplanet', RUNITS[self.runits]),
                                     ('M_planet', 'mplanet', MASS_UNITS[self.mass_units])):
            col = atm.par_scalar.get(scalar, -1)
            if col >= 0:
                slots[name] = ('params', col, factor)
            else:
                refused[name] = (f"'{name}': the atmosphere has no free '{scalar}' (free: "
                                 f'{atm.free})')
        nmodel = atm.npar - sum(1 for c in atm.par_scalar.values() if c >= 0)
        self.model_pnames = list(atm.free[:nmodel])
        for col, name in enumerate(self.model_pnames):
            slots.setdefault(name, ('params', col, 1.0))
        # the continuum's free parameters, in cont.free_pars order
        self.opacity_pnames, self.cont_pnames = [], []
        if cont is not None:
            seen = {}
            for m in cont.rank1:
                for cls, names in _CONT_PNAMES.items():
                    if isinstance(m, cls):
                        for name in names:
                            col = len(self.cont_pnames)
                            self.cont_pnames.append(name)
                            seen.setdefault(name, []).append(col)
            assert len(self.cont_pnames) == len(cont.free_pars)
            for name, cols in seen.items():
                self.opacity_pnames.append(name)
                if len(cols) > 1:
                    refused[name] = (f"'{name}': {len(cols)} continuum models of one kind claim "
                                     'it; the name cannot tell them apart')
                else:
                    slots.setdefault(name, ('continuum_pars', cols[0], 1.0))
        two_stream = rt_path == 'two_stream'
        cloudy_two_stream = ('eval_bands: {}: clouds are not supported in batched form in '
                             'two-stream geometry; use eval()')
        # the isotope ratios of the sampled cross sections ('line sampling' in the reference)
        iso = getattr(model, 'isotopes', None)
        self.iso_pnames = [] if iso is None else list(iso.pnames)
        for col, name in enumerate(self.iso_pnames):
            self.opacity_pnames.append(name)
            slots.setdefault(name, ('iso_pars', col, 1.0))
        ndeck = 0 if cont is None else len(cont.deck)
        if ndeck:
            self.opacity_pnames.append('log_p_cl')
        if two_stream:
            refused['log_p_cl'] = cloudy_two_stream.format('deck_logp')
            refused['f_patchy'] = cloudy_two_stream.format('f_patchy')
        elif ndeck == 0:
            refused['log_p_cl'] = _table.MSG_DECK_NEEDS_DECK
        elif ndeck > 1:
            refused['log_p_cl'] = (f"'log_p_cl': {ndeck} continuum models of one kind claim it; "
                                   'the name cannot tell them apart')
        hires = isinstance(bands, HiresData)
        if not hires:
            refused['rv_shift'] = _table.MSG_RV_NEEDS_HIRES
        if hires:
            refused['T_eff'] = _table.MSG_STAR_HIRES
        elif rt_path == 'transit':
            refused['T_eff'] = _table.MSG_STAR_TRANSIT
        elif getattr(bands, 'star_grid', None) is None and \
                getattr(model, 'irradiation', None) is None:
            refused['T_eff'] = _table.MSG_STAR_NEEDS_GRID
        if rt_path == 'transit':
            refused['f_dilution'] = "'f_dilution' belongs to emission and two-stream geometry"
        for name, dest in _SOLO_DESTS.items():
            if name not in refused:
                slots[name] = (dest, 0, 1.0)
        for col, name in enumerate(obs.offset_models):
            slots.setdefault(name, ('offsets', col, 1.0))
        for col, name in enumerate(obs.err_models):
            slots.setdefault(name, ('err_pars', col, 1.0))
        self.available = (SOLO_PARAMS + self.model_pnames + self.opacity_pnames +
                          list(obs.offset_models) + list(obs.err_models))
        return slots, refused

    def _lookup(self, name, slots, refused):
        if name in refused and name not in slots:
            raise ValueError(refused[name])
        if name not in slots:
            raise ValueError(f"Invalid retrieval parameter '{name}'. Possible values are:\n"
                             f'{self.available}')
        return slots[name]

    def _resolve(self, fixed):
        model, atm, obs = self.model, self.atmosphere, self.observation
        cont = getattr(model, 'continuum', None)
        slots, refused = self._slots()
        # entries of the map: the block's parameters first, then the constants
        dest_of = [self._lookup(name, slots, refused) for name in self.pnames]
        for name in fixed:
            if name in self.pnames:
                raise ValueError(f"fixed: '{name}' is a line of retrieval_params")
        fixed_of = {name: self._lookup(name, slots, refused) for name in fixed}
        taken = {}
        for name, (dest, col, _) in list(zip(self.pnames, dest_of)) + list(fixed_of.items()):
            if (dest, col) in taken:
                raise ValueError(f"'{name}' and '{taken[dest, col]}' name the same value "
                                 f'({dest}, column {col})')
            taken[dest, col] = name

        # the destination tensors of this retrieval, in a fixed order, with their column counts
        ncols = {'params': atm.npar,
                 'continuum_pars': 0 if cont is None else len(cont.free_pars),
                 'iso_pars': len(self.iso_pnames), 'offsets': obs.noff, 'err_pars': obs.nerr}
        wanted = {'params'} | {d for d, _, _ in dest_of} | {d for d, _, _ in fixed_of.values()}
        if 'tstar' not in wanted:
            if getattr(self.bands, 'star_grid', None) is not None:
                raise ValueError(_table.MSG_GRID_NEEDS_TSTAR)
            if getattr(model, 'irradiation', None) is not None:
                raise ValueError(_table.MSG_IRRADIATION_NEEDS_TSTAR)
        order = ('params', 'continuum_pars', 'iso_pars') + _SCALAR_DESTS + ('offsets', 'err_pars')
        self.dest_names = [d for d in order if d in wanted]
        self.dest_ncols = [ncols.get(d, 1) for d in self.dest_names]
        if len(self.dest_names) > MAX_DESTS:
            raise ValueError(f'{len(self.dest_names)} destinations: at most {MAX_DESTS}')

        # what the objects hold now, for the columns nobody names
        current = {'params': getattr(atm, 'base_params', None),
                   'continuum_pars': None if cont is None else cont.current_pars(),
                   'iso_pars': None if not self.iso_pnames else
                   np.array(model.isotopes.pars, float),
                   'offsets': np.zeros(obs.noff), 'err_pars': np.array(obs.err_defaults, float)}
        column_names = {'params': list(atm.free), 'continuum_pars': self.cont_pnames,
                        'iso_pars': self.iso_pnames,
                        'offsets': list(obs.offset_models), 'err_pars': list(obs.err_models)}
        src, cons, factor, dest, col = [], [], [], [], []

        def entry(s, c, f, d, k):
            src.append(s), cons.append(c), factor.append(f)
            dest.append(self.dest_names.index(d)), col.append(k)
        for i, (d, k, f) in enumerate(dest_of):
            entry(self.source[i], self.constant[i], f, d, k)
        for name, (d, k, f) in fixed_of.items():
            entry(-1, float(fixed[name]), f, d, k)
        for d, n in zip(self.dest_names, self.dest_ncols):
            for k in range(n):
                if (d, k) in taken:
                    continue
                have = current.get(d)
                if have is None or not np.isfinite(have[k]):
                    label = column_names[d][k] if d in column_names else d
                    raise ValueError(f"'{label}' ({d}, column {k}) is named neither in "
                                     'retrieval_params nor in fixed, and the objects hold no '
                                     'value for it')
                entry(-1, float(have[k]), 1.0, d, k)
        self.nmap = len(src)
        if self.nmap > MAX_PARAMS:
            raise ValueError(f'{self.nmap} mapped values ({self.npar} parameters and '
                             f'{self.nmap - self.npar} constants): at most {MAX_PARAMS}')
        self.map_src = np.array(src, np.int32)
        self.map_const = np.array(cons, np.float64)
        self.map_factor = np.array(factor, np.float64)
        self.map_dest = np.array(dest, np.int32)
        self.map_col = np.array(col, np.int32)
        self.destination = [(d, k) for d, k, _ in dest_of]
        # the index maps under the reference's names (pyrat/retrieval.py:197-284)
        where = {name: i for i, name in enumerate(self.pnames)}
        self.irad, self.ipress, self.imass, self.irv, self.ipatchy, self.itstar, self.idilut = (
            np.array([where[n]]) if n in where else None
            for n in ('R_planet', 'log_p_ref', 'M_planet', 'rv_shift', 'f_patchy', 'T_eff',
                      'f_dilution'))
        solo = set(SOLO_PARAMS)
        tnames = list(getattr(getattr(atm, 'tmodel', None), 'pnames', []))
        vmodels = [list(m.pnames) for m in getattr(atm, 'vmr_models', [])]
        self.map_pars = {'temp': [], 'mol': [], 'opacity': {}, 'offset': [], 'error': []}
        index = {'temp': [], 'mol': [], 'offset': [], 'error': []}
        self.iopacity = {}
        for i, name in enumerate(self.pnames):
            d, k = self.destination[i]
            if name in solo:
                continue
            if d == 'params' and name in tnames:
                index['temp'].append(i)
                self.map_pars['temp'].append(tnames.index(name))
            elif d == 'params':
                imodel = next((j for j, names in enumerate(vmodels) if name in names), None)
                if imodel is None:
                    continue
                index['mol'].append(i)
                self.map_pars['mol'].append((imodel, vmodels[imodel].index(name)))
            elif d == 'continuum_pars':
                mname, idx = cont.free_pars[k]
                self.iopacity.setdefault(mname, []).append(i)
                self.map_pars['opacity'].setdefault(mname, []).append(idx)
            elif d == 'iso_pars':
                self.iopacity.setdefault('line sampling', []).append(i)
                self.map_pars['opacity'].setdefault('line sampling', []).append(k)
            elif d == 'deck_logp':
                self.iopacity.setdefault('deck', []).append(i)
                self.map_pars['opacity'].setdefault('deck', []).append(0)
            elif d == 'offsets':
                index['offset'].append(i)
                self.map_pars['offset'].append(k)
            elif d == 'err_pars':
                index['error'].append(i)
                self.map_pars['error'].append(k)
        self.itemp, self.imol, self.ioffset, self.ierror = (
            index[key] or None for key in ('temp', 'mol', 'offset', 'error'))

    # ------------------------------------------------------------------ host statements
    def _theta_host(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.nfree:
            raise ValueError(f'theta must have shape (nw, {self.nfree}), got {theta.shape}')
        return theta

    def expand_host(self, theta):
        """theta[nw, nfree] -> full[nw, npar]: free parameters from theta, fixed ones at `value`,
        shared ones from their target (the vector Loglike.__call__ hands to eval())."""
        theta = self._theta_host(theta)
        full = np.tile(self.params, (theta.shape[0], 1))
        full[:, self.ifree] = theta
        for i, j in self.share_target.items():
            full[:, i] = full[:, j]
        return full

    def inside_host(self, theta):
        """[nw] bool: every free value is finite and pmin <= p <= pmax."""
        theta = self._theta_host(theta)
        lo, hi = self.pmin[self.ifree], self.pmax[self.ifree]
        with np.errstate(invalid='ignore'):
            return np.all(np.isfinite(theta) & (theta >= lo) & (theta <= hi), axis=1)

    def log_prior_host(self, theta):
        """[nw]: the sum of log_prior_terms over the free parameters (no normalisation term);
        -inf for a walker that is not inside."""
        theta = self._theta_host(theta)
        f = self.ifree
        terms = log_prior_terms(theta, self.prior[f], self.priorlow[f], self.priorup[f])
        return np.where(self.inside_host(theta), np.sum(terms, axis=1), -np.inf)

    def split_host(self, theta, substitute=True):
        """theta[nw, nfree] -> {destination: array}: 'params'[nw, npar of the atmosphere] and, as
        far as this retrieval has them, 'continuum_pars'[nw, ncont], 'iso_pars'[nw, niso],
        'deck_logp', 'f_patchy',
        'rv', 'tstar', 'f_dilution' [nw], 'offsets'[nw, noff], 'err_pars'[nw, nerr]: copies, and
        one multiply where the unit factor is not 1.  substitute: a walker that is not inside is
        mapped from the `value` column, as the device does."""
        theta = self._theta_host(theta).copy()
        if substitute:
            theta[~self.inside_host(theta)] = self.value_free
        nw = theta.shape[0]
        out = {d: np.full((nw, n), np.nan) for d, n in zip(self.dest_names, self.dest_ncols)}
        for e in range(self.nmap):
            s = self.map_src[e]
            v = theta[:, s] if s >= 0 else np.full(nw, self.map_const[e])
            if self.map_factor[e] != 1.0:
                v = v * self.map_factor[e]
            out[self.dest_names[self.map_dest[e]]][:, self.map_col[e]] = v
        return {d: (a[:, 0] if d in _SCALAR_DESTS else a) for d, a in out.items()}

    def prior_transform_host(self, cube):
        """cube[nw, nfree] in (0, 1) -> theta: uniform: pmin + u (pmax - pmin); two-sided Gaussian
        (lo = priorlow, up = priorup): where u (lo + up) < lo, decided exactly (below_split),
        prior + lo ndtri(0.5 u (lo + up) / lo), otherwise prior - up ndtri(0.5 (1 - u) (1 + lo /
        up)): either branch hands ndtri the tail mass itself (1 minus it would lose the tail from
        three sigma upward).  u = 0 gives -inf, u = 1 +inf.  Not truncated to [pmin, pmax]:
        inside catches what falls out."""
        from scipy.special import ndtri
        u = self._theta_host(cube)
        self._check_transform()
        f = self.ifree
        pmin, pmax, prior = self.pmin[f], self.pmax[f], self.prior[f]
        lo, up = self.priorlow[f], self.priorup[f]
        uniform = (lo == 0) & (up == 0)
        lo1, up1 = np.where(uniform, 1.0, lo), np.where(uniform, 1.0, up)
        with np.errstate(all='ignore'):
            flat = np.where(uniform, pmin, 0.0) + u * np.where(uniform, pmax - pmin, 0.0)
            low = prior + lo1 * ndtri(0.5 * u * (lo1 + up1) / lo1)
            high = prior - up1 * ndtri(0.5 * (1.0 - u) * (1.0 + lo1 / up1))
            gauss = np.where(below_split(u, lo1, up1), low, high)
        return np.where(uniform, flat, gauss)

    def _check_prior_widths(self):
        """A free parameter's priorlow and priorup are finite and not negative, and both zero
        (uniform) or neither: with one of them zero the prior term is 0 / 0 at p == prior and the
        transform is infinite (the reference gives that case no meaning: it tests only
        priorlow == 0 and priorup == 0, pyrat/retrieval.py:362)."""
        f = self.ifree
        lo, up = self.priorlow[f], self.priorup[f]
        with np.errstate(invalid='ignore'):
            bad = ~(np.isfinite(lo) & np.isfinite(up) & (lo >= 0) & (up >= 0))
        if np.any(bad):
            names = [self.pnames[i] for i in f[bad]]
            raise ValueError(f'retrieval_params: free parameters {names} have a negative or '
                             'non-finite priorlow or priorup')
        half = (lo == 0) != (up == 0)
        if np.any(half):
            names = [self.pnames[i] for i in f[half]]
            raise ValueError(f'retrieval_params: free parameters {names} have exactly one of '
                             'priorlow and priorup equal to zero: a half-open prior is not '
                             'defined (both zero: uniform)')

    def _check_transform(self):
        f = self.ifree
        uniform = (self.priorlow[f] == 0) & (self.priorup[f] == 0)
        bad = uniform & ~(np.isfinite(self.pmin[f]) & np.isfinite(self.pmax[f]))
        if np.any(bad):
            names = [self.pnames[i] for i in f[bad]]
            raise ValueError(f'prior_transform: uniform parameters {names} have an infinite '
                             'bound')

    # ------------------------------------------------------------------ device methods
    def _resident(self):
        if self._device is None:
            f = self.ifree
            self._device = dict(
                src=dev(self.map_src, torch.int32), const=dev(self.map_const),
                factor=dev(self.map_factor), dest=dev(self.map_dest, torch.int32),
                col=dev(self.map_col, torch.int32), value=dev(self.value_free),
                pmin=dev(self.pmin[f]), pmax=dev(self.pmax[f]), prior=dev(self.prior[f]),
                priorlow=dev(self.priorlow[f]), priorup=dev(self.priorup[f]))
        return self._device

    def _theta_device(self, who, theta):
        if not isinstance(theta, torch.Tensor) or not theta.is_cuda or \
                theta.dtype != torch.float64 or theta.dim() != 2 or \
                theta.shape[1] != self.nfree:
            raise ValueError(f'{who} must be a float64 device tensor of shape (nw, {self.nfree}), '
                             f'got {type(theta).__name__} {getattr(theta, "dtype", "")} '
                             f'{tuple(getattr(theta, "shape", ()))}')
        return theta.contiguous()

    def arguments(self, theta):
        """theta[nw, nfree] -> RetrievalArguments, one launch (pb_retrieval_map)."""
        theta = self._theta_device('theta', theta)
        nw = theta.shape[0]
        d = self._resident()
        outs = [torch.empty((nw,) if name in _SCALAR_DESTS else (nw, n), dtype=torch.float64,
                            device=theta.device)
                for name, n in zip(self.dest_names, self.dest_ncols)]
        log_prior = torch.empty(nw, dtype=torch.float64, device=theta.device)
        inside = torch.empty(nw, dtype=torch.int32, device=theta.device)
        ndest = len(outs)
        ptrs = (C.c_void_p * ndest)(*[t.data_ptr() if nw else None for t in outs])
        ncols = (C.c_int32 * ndest)(*self.dest_ncols)
        call('pb_retrieval_map', ptrs, ncols, ndest, _ptr(log_prior), _ptr(inside), _ptr(theta),
             _ptr(d['src']), _ptr(d['const']), _ptr(d['factor']), _ptr(d['dest']), _ptr(d['col']),
             _ptr(d['value']), _ptr(d['pmin']), _ptr(d['pmax']), _ptr(d['prior']),
             _ptr(d['priorlow']), _ptr(d['priorup']), self.nmap, self.nfree, nw, _stream())
        named = dict(zip(self.dest_names, outs))
        kw = {k: named[k] for k in ('continuum_pars', 'iso_pars') + _SCALAR_DESTS if k in named}
        return RetrievalArguments(named['params'], kw, named.get('offsets'),
                                  named.get('err_pars'), log_prior, inside)

    def _combine(self, loglike, args, outside_value, add_prior):
        out = torch.empty_like(loglike)
        call('pb_log_posterior', _ptr(out), _ptr(loglike), _ptr(args.log_prior),
             _ptr(args.inside), outside_value, int(add_prior), loglike.shape[0], _stream())
        return out

    def _loglike(self, args):
        return self.model.eval_loglike(self.atmosphere, args.params, self.bands,
                                       self.observation, offsets=args.offsets,
                                       err_pars=args.err_pars, **args.kw, **self.eval_kw)

    def log_likelihood(self, theta):
        """theta[nw, nfree] -> [nw]: eval_loglike through the map; -1e98, the reference's reject
        value, for a walker outside the bounds."""
        args = self.arguments(theta)
        return self._combine(self._loglike(args), args, -1.0e98, False)

    def log_posterior(self, theta):
        """theta[nw, nfree] -> [nw]: log-likelihood + log-prior; -inf outside the bounds.  A walker
        the model rejects keeps about -1e98."""
        args = self.arguments(theta)
        return self._combine(self._loglike(args), args, -np.inf, True)

    def bandflux(self, theta):
        """theta[nw, nfree] -> [nw, nbands]: eval_params through the map (for posterior_summary
        and plots); a walker outside the bounds gives the band fluxes of the `value` column."""
        args = self.arguments(theta)
        return self.model.eval_params(self.atmosphere, args.params, self.bands, **args.kw,
                                      **self.eval_kw)

    def prior_transform(self, cube):
        """cube[nw, nfree] in (0, 1) -> theta[nw, nfree] (prior_transform_host on the device, with
        the device library's inverse normal CDF).  A uniform parameter with an infinite bound is
        refused."""
        self._check_transform()
        cube = self._theta_device('cube', cube)
        d = self._resident()
        theta = torch.empty_like(cube)
        call('pb_prior_transform', _ptr(theta), _ptr(cube), _ptr(d['pmin']), _ptr(d['pmax']),
             _ptr(d['prior']), _ptr(d['priorlow']), _ptr(d['priorup']), self.nfree,
             cube.shape[0], _stream())
        return theta

    # ------------------------------------------------------------------ the sampler
    def draw_initial(self, n, seed=0):
        """[n, nfree]: n draws from the priors: pb_philox_uniform (sampler.uniforms_host) ->
        prior_transform, with the refusals prior_transform has."""
        self._check_transform()
        cube = torch.empty((int(n), self.nfree), dtype=torch.float64, device='cuda')
        call('pb_philox_uniform', _ptr(cube), int(seed) % 2**64, int(n), self.nfree, _stream())
        return self.prior_transform(cube)

    def sample(self, nchains, ngen, seed=0, z0=None, capacity=None, **kw):
        """A sampler.DEMC over log_posterior, started and run for ngen generations: pstep from the
        block's free lines; z0[M0, nfree], the initial history, defaults to
        draw_initial(10 nchains, seed), and its last nchains rows are the starting states (one
        outside the bounds is refused before the loop); capacity, the rows per chain of the store,
        defaults to ngen + 1; kw: fgamma, fepsilon, p_snooker, thin_z.  -> the DEMC: run(more)
        continues it, summary(it) reduces it."""
        from .sampler import DEMC
        nchains = int(nchains)
        z0 = self.draw_initial(10 * nchains, seed) if z0 is None else \
            self._theta_device('z0', dev(z0))
        if z0.shape[0] < max(nchains, 3) or nchains < 1:
            raise ValueError(f'z0 has {z0.shape[0]} rows: at least {max(nchains, 3)} for '
                             f'{nchains} chains')
        demc = DEMC(self.log_posterior, self.nfree, self.pstep[self.ifree], seed=seed, **kw)
        demc.start(z0[z0.shape[0] - nchains:], z0, int(ngen) + 1 if capacity is None else capacity)
        return demc.run(ngen)

    def nested(self, nlive=1000, seed=0, dlogz=0.5, **kw):
        """A nested.NestedSampler over log_likelihood and prior_transform (the reference's
        `sampler = multinest` with `nlive` live points), started and run until the evidence still
        to come is below dlogz (dlogz=None: started only; run(niter) or run_until() continue it).
        kw: batch, nsteps, fgamma, p_unit of the sampler, check_every and max_iter of run_until.
        A uniform parameter with an infinite bound is refused before anything is launched.
        -> the sampler: logz() is (ln Z, ln Z_err, H), summary(it) reduces its posterior."""
        from .nested import NestedSampler
        self._check_transform()
        until = {k: kw.pop(k) for k in ('check_every', 'max_iter') if k in kw}
        ns = NestedSampler(self.log_likelihood, self.prior_transform, self.nfree, nlive,
                           seed=seed, **kw).start()
        return ns if dlogz is None else ns.run_until(dlogz, **until)

    # ------------------------------------------------------------------ the optimiser
    def _check_least_squares(self):
        """Refused: a free uncertainty-scaling parameter (also one shared with a free line).  Its
        objective carries the term -0.5 sum log(2 pi uncert^2), which is no sum of squares; mc3's
        least-squares fit has the same limit."""
        free_err = [name for i, name in enumerate(self.pnames)
                    if self.destination[i][0] == 'err_pars' and self.source[i] >= 0]
        if free_err:
            raise ValueError(f'the error parameters {free_err} are free: the objective of a '
                             'retrieval with free err_scale_* / err_quad_* lines is not a sum of '
                             'squares; fix them (pstep 0) for residuals and optimize')

    @property
    def igauss(self):
        """The theta columns with a Gaussian prior, in order."""
        f = self.ifree
        return np.where((self.priorlow[f] != 0) | (self.priorup[f] != 0))[0].astype(np.int32)

    def residuals_host(self, theta, model_host):
        """theta[nw, nfree] and the model's band fluxes model_host[nw, ndata] -> R[nw, ndata +
        ngauss]: column i < ndata is (data_i + offset_i unit - model_i) / uncert_i with the
        walker's offsets and uncertainty scaling (Observation.offset_data_host /
        scale_errors_host); then one column (theta_k - prior_k) / s_k per free parameter with a
        Gaussian prior, s_k = priorlow below the prior, priorup from it upward.  So
        -0.5 sum R^2 - 0.5 sum log(2 pi uncert^2) is log_posterior of a walker inside the bounds.
        A walker outside the bounds, or with a non-finite band flux, gets a row of +inf."""
        self._check_least_squares()
        theta = self._theta_host(theta)
        model = np.asarray(model_host, dtype=np.float64)
        obs = self.observation
        nw = theta.shape[0]
        if model.shape != (nw, obs.nbands):
            raise ValueError(f'model_host must have shape ({nw}, {obs.nbands}), got '
                             f'{model.shape}')
        split = self.split_host(theta)
        f = self.ifree
        return residual_rows_host(obs, theta, self.inside_host(theta), model,
                                  split.get('offsets'), split.get('err_pars'), self.igauss,
                                  self.prior[f], self.priorlow[f], self.priorup[f])

    def residuals(self, theta):
        """theta[nw, nfree] -> R[nw, ndata + ngauss] on the device (residuals_host): arguments ->
        eval_params -> one launch of pb_lm_residuals; no torch arithmetic on the path."""
        self._check_least_squares()
        args = self.arguments(theta)
        theta = self._theta_device('theta', theta)
        obs = self.observation
        bf = self.model.eval_params(self.atmosphere, args.params, self.bands, **args.kw,
                                    **self.eval_kw)
        nw = theta.shape[0]
        if bf.dim() != 2 or tuple(bf.shape) != (nw, obs.nbands):
            raise ValueError(f'residuals: the observation has {obs.nbands} data points, the '
                             f'bands give {tuple(bf.shape)}')
        d, o = self._resident(), obs._resident()
        if 'gauss' not in d:
            d['gauss'] = dev(self.igauss, torch.int32)
        ngauss = d['gauss'].shape[0]
        noff = obs.noff if args.offsets is not None else 0
        err_pars = args.err_pars
        if obs.nerr and err_pars is None:
            err_pars = o['err_defaults'].view(1, -1).expand(nw, -1).contiguous()
        out = torch.empty((nw, obs.nbands + ngauss), dtype=torch.float64, device=theta.device)
        call('pb_lm_residuals', _ptr(out), _ptr(bf.contiguous()), _ptr(o['data']),
             _ptr(o['uncert']), _ptr(o['offset_group']) if noff else None,
             _ptr(args.offsets.contiguous()) if noff else None, obs.unit, noff,
             _ptr(o['err_group']) if obs.nerr else None,
             _ptr(o['err_mode']) if obs.nerr else None,
             _ptr(err_pars.contiguous()) if obs.nerr else None, obs.unit, obs.nerr,
             _ptr(theta), _ptr(args.inside), _ptr(d['gauss']) if ngauss else None,
             _ptr(d['prior']), _ptr(d['priorlow']), _ptr(d['priorup']), ngauss, self.nfree, nw,
             obs.nbands, _stream())
        return out

    def optimize(self, nstarts=64, seed=0, theta0=None, check_every=5, **kw):
        """The maxima of the posterior from nstarts starts at once: an
        optimize.LevenbergMarquardt over residuals, with scale = pstep of the free lines, run
        until every start has a status.  theta0[ns, nfree] defaults to draw_initial(nstarts,
        seed); a start outside the bounds is refused before the loop.  kw: the settings of
        optimize.DEFAULTS (unmeasured on a real retrieval).  The residual store takes
        8 ns (nfree + 1) m bytes: one that does not fit in free device memory is refused before
        any launch.  -> an optimize.Optimum.

        DEVIATION: a retrieval with a free err_scale_* or err_quad_* line is refused (its
        objective is no sum of squares; mc3's least-squares fit has the same limit)."""
        from .optimize import LevenbergMarquardt, Optimum
        self._check_least_squares()
        f = self.ifree
        lm = LevenbergMarquardt(self.residuals, self.nfree, self.pmin[f], self.pmax[f],
                                self.pstep[f], **kw)
        if theta0 is None:
            ns = int(nstarts)
        else:
            theta0 = np.asarray(theta0.cpu() if isinstance(theta0, torch.Tensor) else theta0,
                                dtype=np.float64)
            theta0 = self._theta_host(theta0)
            ns = theta0.shape[0]
            if not np.all(self.inside_host(theta0)):
                raise ValueError(f'theta0: rows {list(np.where(~self.inside_host(theta0))[0])} '
                                 'are outside the bounds')
        if ns < 1:
            raise ValueError('optimize: at least one start')
        m = self.observation.nbands + len(self.igauss)
        need = 8 * ns * (self.nfree + 1) * m
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            raise ValueError(f'optimize: the residual store of {ns} starts x {self.nfree + 1} '
                             f'probe points x {m} residuals needs {need} bytes, {free} bytes of '
                             'device memory are free')
        if theta0 is None:
            theta0 = self.draw_initial(ns, seed)
            if not bool((self.arguments(theta0).inside != 0).all()):
                raise ValueError('optimize: a draw from the priors is outside the bounds; give '
                                 'theta0')
        lm.start(theta0).run_until(check_every=check_every)
        cov, active, singular = lm.covariance()
        return Optimum(self, lm, self.log_posterior(lm.theta), cov, active, singular)

    def summary(self, sampler, burn=0, mode=None, **kw):
        """The posterior summary of a sampler's chain: sampler.unique(burn) -> arguments ->
        model.posterior_summary(atmosphere, params, counts, bands, ...); kw: what
        posterior_summary takes besides the per-sample tensors (quantiles, chunk,
        contribution, ...).  mode=m: the summary of one posterior mode of a nested sampler,
        sampler.unique(burn, mode=m) (NestedSampler.modes); a sampler without modes (DEMC) is
        refused."""
        if mode is None:
            theta, counts = sampler.unique(burn)
        elif not hasattr(sampler, 'modes'):
            raise ValueError(f'mode = {mode}: a {type(sampler).__name__} has no modes; only a '
                             'nested sampler separates them')
        else:
            theta, counts = sampler.unique(burn, mode=mode)
        args = self.arguments(theta)
        return self.model.posterior_summary(self.atmosphere, args.params, counts, self.bands,
                                            **args.kw, **kw)
