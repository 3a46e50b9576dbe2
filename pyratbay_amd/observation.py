"""The exit of the batched loop towards the sampler: the stellar SED grid of an eclipse retrieval
with a free stellar temperature (StellarGrid; PassBands.set_eclipse_grid uses it) and the data of
a retrieval with instrumental offsets and uncertainty scaling per walker (Observation: the
reference's tools/data.py `Data` and the likelihood of tools/retrieval_tools.py `Loglike`), both
with their NumPy statements.  Kernels: csrc/pb_observation.hip."""
import numpy as np
import torch

from ._capi import call
from ._device import _ptr, _stream, dev

# pt.u(units) of the units Data.offset_data / Data.scale_errors take (pyratbay.constants)
UNITS = {'none': 1.0, 'percent': 1.0e-2, 'ppt': 1.0e-3, 'ppm': 1.0e-6}

# Data.scale_errors' modes as the kernel takes them
SCALE, QUADRATURE = 0, 1
_ERR_PREFIXES = (('err_scale_', SCALE), ('err_quad_', QUADRATURE))
# obs.uncert_pars left as None (pyrat/observation.py:121-131): no scaling
ERR_DEFAULTS = {SCALE: 0.0, QUADRATURE: -100.0}


class StellarGrid:
    """The stellar SED grid of a retrieval with a free stellar temperature (pyrat/argum.py:93-98:
    spec.flux_interp = interp1d(atm.sed_temps, starflux, axis=0)), resident on the device:
    fluxes[nt, W] ALREADY on the model's wavenumbers wn[W] (the reference interpolates the models
    to spec.wn once, at set-up), sed_temps[nt] strictly ascending, nt >= 2."""

    def __init__(self, wn, sed_temps, fluxes):
        self.wn_host = np.ascontiguousarray(
            wn.cpu().numpy() if isinstance(wn, torch.Tensor) else wn, dtype=np.float64)
        self.sed_temps_host = np.ascontiguousarray(sed_temps, dtype=np.float64)
        self.fluxes_host = np.ascontiguousarray(fluxes, dtype=np.float64)
        if self.wn_host.ndim != 1 or self.sed_temps_host.ndim != 1:
            raise ValueError('StellarGrid: wn[W] and sed_temps[nt] must be one-dimensional')
        self.nt, self.nwave = len(self.sed_temps_host), len(self.wn_host)
        if self.nt < 2:
            raise ValueError(f'StellarGrid: at least 2 temperatures are needed, got {self.nt}')
        if self.fluxes_host.shape != (self.nt, self.nwave):
            raise ValueError(f'StellarGrid: fluxes must have shape ({self.nt}, {self.nwave}) -- '
                             f'on the model\'s grid --, got {self.fluxes_host.shape}')
        if not np.all(np.isfinite(self.sed_temps_host)) or \
                not np.all(np.diff(self.sed_temps_host) > 0):
            raise ValueError('StellarGrid: sed_temps must be finite and strictly ascending')
        self.tmin, self.tmax = float(self.sed_temps_host[0]), float(self.sed_temps_host[-1])
        self.sed_temps = dev(self.sed_temps_host)
        self.fluxes = dev(self.fluxes_host)

    def flux_host(self, tstar):
        """The NumPy statement of the device's interpolation, interp1d's linear rule as SciPy
        states it: tstar (a scalar) -> starflux[W]; tstar[n] -> [n, W].  Outside the grid's
        temperatures (where interp1d raises): ValueError."""
        t = np.asarray(tstar, float)
        x, y = self.sed_temps_host, self.fluxes_host
        if not np.all((t >= x[0]) & (t <= x[-1])):
            raise ValueError(f'StellarGrid: tstar outside the {x[0]:.1f}-{x[-1]:.1f} K range of '
                             'the SED grid')
        hi = np.clip(np.searchsorted(x, t.reshape(-1)), 1, len(x) - 1)
        lo = hi - 1
        slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[:, None]
        out = slope * (t.reshape(-1) - x[lo])[:, None] + y[lo]
        return out.reshape(t.shape + (self.nwave,))


def parse_error_param(var):
    """tools/data.py parse_error_param without the tex name: 'err_scale_NAME' / 'err_quad_NAME'
    -> (instrument, mode) with underscores of the instrument as blanks."""
    for prefix, mode in _ERR_PREFIXES:
        if var.startswith(prefix):
            return var.replace(prefix, '', 1).replace('_', ' '), mode
    raise ValueError(f"Invalid error scaling parameter '{var}'. "
                     f"Valid options begin with: {[p for p, _ in _ERR_PREFIXES]}")


class Observation:
    """tools/data.py's `Data` for the device: data[nb] and uncert[nb] with the instrumental
    offsets (offset_models, e.g. 'offset_miri') and the uncertainty scalings (err_models:
    'err_scale_NAME' multiplies the uncertainties of NAME's points by 10**value, 'err_quad_NAME'
    adds 10**value * units in quadrature) of a retrieval.  A model applies to the data points
    whose band name contains its instrument name (underscores as blanks); at most one offset and
    one scaling per point.  units ('none', 'percent', 'ppt', 'ppm') are those of the offset values
    and of the quadrature terms (the reference's obs.units).

    loglike() is the reference's Loglike.__call__ (tools/retrieval_tools.py:98-104) for a batch,
    one launch (pb_loglike_obs).  NOTE: the reference's Loglike binds obs.data / obs.uncert when
    it is constructed (retrieval_tools.py:48-52) while eval() REBINDS them with every call
    (pyrat_obj.py:362-372), so that object goes on using the arrays of its construction; the
    likelihood here uses the data and uncertainties eval() leaves in obs -- what that class's own
    docstring says it is for ("allows to dynamically modify the data and uncertainty values")."""

    def __init__(self, data, uncert, band_names=None, offset_models=(), err_models=(),
                 units='none'):
        self.data_host = np.array(data, dtype=np.float64)
        self.uncert_host = np.array(uncert, dtype=np.float64)
        if self.data_host.ndim != 1 or self.data_host.shape != self.uncert_host.shape or \
                len(self.data_host) < 1:
            raise ValueError('Observation: data[nb] and uncert[nb], nb >= 1')
        self.nbands = nb = len(self.data_host)
        if units not in UNITS:
            raise ValueError(f"Observation: units '{units}': one of {list(UNITS)}")
        self.units, self.unit = units, UNITS[units]
        offset_models = [offset_models] if isinstance(offset_models, str) else \
            list(offset_models or ())
        err_models = [err_models] if isinstance(err_models, str) else list(err_models or ())
        if (offset_models or err_models) and (band_names is None or len(band_names) != nb):
            raise ValueError(f'Observation: offset and error models need band_names[{nb}]')
        band_names = [] if band_names is None else [str(name) for name in band_names]
        self.offset_models, self.err_models = offset_models, err_models
        self.noff, self.nerr = len(offset_models), len(err_models)

        self.offset_indices = []
        for var in offset_models:
            inst = var.replace('offset_', '').replace('_', ' ')
            indices = np.array([inst in name for name in band_names], bool)
            if np.sum(indices) == 0:
                raise ValueError(f"Invalid instrumental offset parameter '{var}'. "
                                 f"There is no instrument matching the name '{inst}'")
            self.offset_indices.append(indices)
        if self.noff and np.any(np.sum(self.offset_indices, axis=0) > 1):
            raise ValueError('Multiple instrumental offsets apply to a same data point')

        self.err_indices, self.err_inst, modes = [], [], []
        for var in err_models:
            inst, mode = parse_error_param(var)
            indices = np.array([inst in name for name in band_names], bool)
            if np.sum(indices) == 0:
                raise ValueError(f"Invalid retrieval parameter '{var}'. "
                                 f"There is no instrument matching the name '{inst}'")
            self.err_indices.append(indices)
            self.err_inst.append(inst)
            modes.append(mode)
        if self.nerr and np.any(np.sum(self.err_indices, axis=0) > 1):
            raise ValueError('Multiple uncertainty scaling apply to a same data point')
        self.err_mode_host = np.array(modes, np.int32)
        self.err_defaults = np.array([ERR_DEFAULTS[m] for m in modes], float)

        def groups(index_lists):
            g = np.full(nb, -1, np.int32)
            for j, indices in enumerate(index_lists):
                g[indices] = j
            return g
        self.offset_group_host = groups(self.offset_indices)
        self.err_group_host = groups(self.err_indices)
        self._device = None

    # ---- the host statements (tools/data.py:210-270, retrieval_tools.py:98-104) ----
    def offset_data_host(self, vals=None):
        """Data.offset_data(vals, units): the data with the offsets vals[noff] applied."""
        data = np.copy(self.data_host)
        if vals is None or self.noff == 0:
            return data
        for j, val in enumerate(vals):
            data[self.offset_indices[j]] += val * self.unit
        return data

    def scale_errors_host(self, vals=None):
        """Data.scale_errors(vals, units): the uncertainties scaled by vals[nerr] (log10)."""
        uncert = np.copy(self.uncert_host)
        if vals is None or self.nerr == 0:
            return uncert
        for j, val in enumerate(vals):
            indices = self.err_indices[j]
            e_scaling = 10.0**val
            if self.err_mode_host[j] == SCALE:
                uncert[indices] *= e_scaling
            else:
                e_scaling *= self.unit
                uncert[indices] = np.sqrt(uncert[indices]**2.0 + e_scaling**2.0)
        return uncert

    def loglike_host(self, model, offsets=None, err_pars=None):
        """Loglike.__call__ on the data and uncertainties of offsets[noff] / err_pars[nerr]
        (None: the defaults -- no offset, no scaling): model[nb] -> a float, model[nw, nb] with
        offsets[nw, noff] / err_pars[nw, nerr] -> [nw]."""
        model = np.asarray(model, float)
        if model.ndim == 2:
            return np.array([self.loglike_host(
                m, None if offsets is None else offsets[w],
                None if err_pars is None else err_pars[w]) for w, m in enumerate(model)])
        data = self.offset_data_host(offsets)
        uncert = self.scale_errors_host(self.err_defaults if err_pars is None else err_pars)
        with np.errstate(all='ignore'):
            log_like = (-0.5 * np.sum(((data - model) / uncert)**2.0)
                        - 0.5 * np.sum(np.log(2.0 * np.pi * uncert**2.0)))
        return float(log_like) if np.isfinite(log_like) else -1.0e98

    # ---- the device form ----
    def _resident(self):
        if self._device is None:
            self._device = dict(
                data=dev(self.data_host), uncert=dev(self.uncert_host),
                offset_group=dev(self.offset_group_host, torch.int32),
                err_group=dev(self.err_group_host, torch.int32),
                err_mode=dev(self.err_mode_host, torch.int32),
                err_defaults=dev(self.err_defaults))
        return self._device

    def loglike(self, bandflux, offsets=None, err_pars=None):
        """bandflux[nw, nb] (a float64 device tensor; [nb]: one walker) -> loglike[nw], one launch
        and no read-back.  offsets[nw, noff] and err_pars[nw, nerr]: float64 device tensors in
        model order; None with models present: the reference's defaults (offset 0; scale 0.0,
        quadrature -100.0: pyrat/observation.py:121-131).  A non-finite value (a rejected walker's
        +inf band fluxes) becomes -1e98, the reference's reject value."""
        bf = bandflux if bandflux.dim() == 2 else bandflux.view(1, -1)
        nw = bf.shape[0]
        if not bf.is_cuda or bf.dtype != torch.float64 or bf.shape[1] != self.nbands:
            raise ValueError(f'Observation.loglike: bandflux must be a float64 device tensor '
                             f'[nw, {self.nbands}], got {bf.dtype} {tuple(bf.shape)} on '
                             f'{bf.device}')
        for name, t, n in (('offsets', offsets, self.noff), ('err_pars', err_pars, self.nerr)):
            if t is None:
                continue
            if n == 0:
                raise ValueError(f'Observation.loglike: {name} without such models')
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or \
                    tuple(t.shape) != (nw, n):
                raise ValueError(f'Observation.loglike: {name} must be a float64 device tensor '
                                 f'of shape {(nw, n)}, got {type(t).__name__} '
                                 f'{getattr(t, "dtype", "")} {tuple(getattr(t, "shape", ()))}')
        d = self._resident()
        # (the defaults: no offset is no offset model for the kernel; the error models' default
        # values are one row expanded over the walkers)
        noff = self.noff if offsets is not None else 0
        if self.nerr and err_pars is None:
            err_pars = d['err_defaults'].view(1, -1).expand(nw, -1)
        out = torch.empty(nw, dtype=torch.float64, device=bf.device)
        call('pb_loglike_obs', _ptr(out), _ptr(bf.contiguous()), _ptr(d['data']),
             _ptr(d['uncert']), _ptr(d['offset_group']) if noff else None,
             _ptr(offsets.contiguous()) if noff else None, self.unit, noff,
             _ptr(d['err_group']) if self.nerr else None,
             _ptr(d['err_mode']) if self.nerr else None,
             _ptr(err_pars.contiguous()) if self.nerr else None, self.unit, self.nerr, nw,
             self.nbands, _stream())
        return out
