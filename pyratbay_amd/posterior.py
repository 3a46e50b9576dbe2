"""Posterior summary on the device (posterior_post_processing,
pyratbay/tools/retrieval_tools.py:384-503): the median and the 1- and 2-sigma bounds of the
spectra, band fluxes, temperature and abundance profiles of a posterior, per wavenumber, band,
layer and (layer, species).

The reference evaluates every UNIQUE sample of the chain (np.unique of the posterior's first
column), expands the results with the inverse index (`models[uinv]`: each sample as often as the
chain visited it) and takes np.percentile along the samples.  Here the unique samples go through
TableSpectrum.eval_bands in chunks, their results are kept sample-minor on the device
([nwave, n], ...) and pb_weighted_quantiles (csrc/pb_quantiles.hip) selects the order statistics
of the expansion from the samples and their multiplicities, without forming it:
weighted_quantiles_host is the NumPy statement of that kernel, and both have np.percentile's
bits.  The reference's fifth product, the median of the band contribution functions
(retrieval_tools.py:474-504: np.median(cf[uinv], axis=0)), comes the same way when asked for
(contribution=True): eval_bands(contribution_out=...) per chunk into a store [L, nbands, n] and
its 0.5 quantile."""
import collections

import numpy as np

from . import _capi
from ._device import _ptr, _stream, dev, require_gpu

# the median and the bounds of the central 68.27 % and 95.45 %, in the reference's order
# (retrieval_tools.py:454)
QUANTILES = [0.5, 0.15865, 0.84135, 0.02275, 0.97725]


def unique_samples(posterior):
    """(u_index, counts, inverse) of a chain posterior[nsamples, npar], as the reference takes
    them (retrieval_tools.py:440-442): np.unique on the FIRST column only; posterior[u_index] are
    the unique samples, counts[i] how often the chain visited sample i, posterior[u_index][inverse]
    the chain."""
    posterior = np.asarray(posterior)
    if posterior.ndim != 2 or posterior.shape[0] < 1:
        raise ValueError(f'unique_samples: posterior[nsamples, npar], got shape {posterior.shape}')
    _, u_index, inverse = np.unique(posterior[:, 0], return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    return u_index, np.bincount(inverse), inverse


def quantile_ranks(total, q):
    """(rank_lo[nq], rank_hi[nq], gamma[nq]) of the quantiles q (fractions in [0, 1]) of a sorted
    array of `total` elements, as np.percentile(a, 100 * q, method='linear') forms them: the
    result is lerp(a[rank_lo], a[rank_hi], gamma)."""
    q = np.atleast_1d(np.asarray(q, float))
    total = int(total)
    if q.ndim != 1 or q.size < 1 or not np.all((q >= 0) & (q <= 1)):
        raise ValueError('quantiles: a non-empty list of fractions in [0, 1]')
    if total < 1:
        raise ValueError('quantiles of an empty sample (every count is zero)')
    v = (total - 1) * np.true_divide(100 * q, 100)
    lo = np.floor(v)
    rank_lo = lo.astype(np.int64)
    return rank_lo, np.minimum(rank_lo + 1, total - 1), v - lo


def _sort_key(values):
    """The order-preserving unsigned key of a double the kernel selects on: -0.0 before +0.0,
    NaNs of positive sign last."""
    bits = np.ascontiguousarray(values, np.float64).view(np.uint64)
    sign = np.uint64(1) << np.uint64(63)
    return np.where(bits & sign != 0, ~bits, bits | sign)


def weighted_quantiles_host(values, counts, q):
    """The NumPy statement of pb_weighted_quantiles: values[n, ...] (samples along the FIRST
    axis, as np.percentile(..., axis=0) takes them), counts[n] >= 0 -> [nq, ...], equal to
    np.percentile(values[inverse], 100 * q, axis=0) for any `inverse` that repeats sample i
    counts[i] times -- without the expansion, so the counts may be large."""
    values = np.asarray(values, float)
    counts = np.asarray(counts, np.int64).reshape(-1)
    if values.ndim < 1 or values.shape[0] != len(counts) or len(counts) < 1:
        raise ValueError(f'weighted_quantiles_host: values[n, ...] and counts[n], got '
                         f'{values.shape} and {counts.shape}')
    live = counts > 0
    rank_lo, rank_hi, gamma = quantile_ranks(counts[live].sum(), q)
    flat = values.reshape(values.shape[0], -1)[live]
    order = np.argsort(_sort_key(flat), axis=0, kind='stable')
    ordered = np.take_along_axis(flat, order, axis=0)
    ends = np.cumsum(counts[live][order], axis=0)        # ranks [ends[k-1], ends[k]) hold row k
    cols = np.arange(flat.shape[1])

    def select(ranks):
        return np.stack([ordered[np.sum(ends <= r, axis=0), cols] for r in ranks])

    a, b, t = select(rank_lo), select(rank_hi), gamma[:, None]
    with np.errstate(invalid='ignore'):
        # NumPy's _lerp (lib/_function_base_impl.py), operation by operation
        d = b - a
        out = np.where(t >= 0.5, b - d * (1 - t), a + d * t)
    return out.reshape((len(gamma),) + values.shape[1:])


def weighted_quantiles(values, counts, q, total=None):
    """Quantiles of weighted samples on the device (pb_weighted_quantiles): values[..., n], a
    float64 device tensor with the SAMPLES ALONG THE LAST AXIS (sample-minor: every leading index
    is a column), counts[n] (int64 device tensor or host array) -> [nq, ...].  A 2-D values may
    be a view with a row stride above n (columns [ncol, ld] of which n are used).  total = the
    sum of the counts when the caller knows it; None: it is read back from the device (the one
    synchronisation of this function; the ranks are formed on the host, once per call)."""
    import torch
    require_gpu()
    if not isinstance(values, torch.Tensor) or not values.is_cuda or \
            values.dtype != torch.float64 or values.dim() < 1:
        raise ValueError('weighted_quantiles: values must be a float64 device tensor [..., n]')
    n = values.shape[-1]
    lead = tuple(values.shape[:-1])
    if values.dim() == 2 and values.stride(1) == 1 and values.stride(0) >= n and n > 0:
        ld = values.stride(0) if values.shape[0] > 1 else n
    else:
        values = values.contiguous()
        ld = n
    ncol = int(np.prod(lead, dtype=np.int64))
    if not isinstance(counts, torch.Tensor):
        counts = dev(np.asarray(counts, np.int64).reshape(-1), torch.int64)
    if not counts.is_cuda or counts.dtype != torch.int64 or tuple(counts.shape) != (n,) or n < 1:
        raise ValueError(f'weighted_quantiles: counts must be int64[{n}] (n >= 1), got '
                         f'{counts.dtype} {tuple(counts.shape)}')
    counts = counts.contiguous()
    if total is None:
        total = int(torch.clamp(counts, min=0).sum())
    rank_lo, rank_hi, gamma = quantile_ranks(total, q)
    nq = len(gamma)
    out = torch.empty((nq,) + lead, dtype=torch.float64, device=values.device)
    need = _capi.lib().pb_weighted_quantiles_work_doubles(n, ncol, nq)
    work = torch.empty(need, dtype=torch.float64, device=values.device) if need else None
    lo, hi, g = dev(rank_lo, torch.int64), dev(rank_hi, torch.int64), dev(gamma)
    # (values may be a strided view: its data pointer, not _ptr's contiguous tensor)
    _capi.call('pb_weighted_quantiles', _ptr(out), values.data_ptr(), int(ld), _ptr(counts), n,
               ncol, _ptr(lo), _ptr(hi), _ptr(g), nq, _ptr(work), _stream())
    return out


PosteriorSummary = collections.namedtuple(
    'PosteriorSummary', 'spectrum bands temperature vmr n_rejected quantiles stores contribution',
    defaults=(None,))

# per-walker keywords of eval_bands: posterior_summary hands each chunk its rows
_PER_SAMPLE = ('continuum_pars', 'rv', 'deck_logp', 'f_patchy', 'f_dilution', 'tstar',
               'rplanet', 'iso_pars')


def posterior_summary(model, atmosphere, params, counts, bands, quantiles=QUANTILES, chunk=64,
                      keep_stores=False, contribution=False, **kw):
    """TableSpectrum.posterior_summary: see there."""
    import torch
    from .atmosphere import BAR, K_BOLTZ
    require_gpu()
    quantiles = [float(x) for x in np.atleast_1d(quantiles)]
    quantile_ranks(1, quantiles)                                  # (range check)
    if not isinstance(params, torch.Tensor) or params.dim() != 2 or params.shape[0] < 1:
        raise ValueError('posterior_summary: params must be a device tensor [n >= 1, npar]')
    n = params.shape[0]
    counts_host = None if isinstance(counts, torch.Tensor) else \
        np.asarray(counts, np.int64).reshape(-1)
    if tuple(counts.shape if counts_host is None else counts_host.shape) != (n,):
        raise ValueError(f'posterior_summary: counts must have shape ({n},)')
    if counts_host is not None and np.any(counts_host < 0):
        raise ValueError('posterior_summary: negative counts')
    if int(chunk) < 1:
        raise ValueError('posterior_summary: chunk >= 1')
    for name in ('temps', 'dens', 'radius', 'continuum_density', 'alkali_density', 'spectra_out',
                 'contribution_out', 'contribution_pressure'):
        if name in kw:
            raise ValueError(f'posterior_summary: {name} is not the caller\'s to give')
    from .table import free_rplanet
    kw = free_rplanet(atmosphere, params, bands, kw, 'posterior_summary')
    for name in _PER_SAMPLE:
        if kw.get(name) is not None and tuple(kw[name].shape[:1]) != (n,):
            raise ValueError(f'posterior_summary: {name} must have one row per sample ({n})')
    chunk = min(int(chunk), n)
    nwave, L, nbands = model.nwave, model.nlayers, bands.nbands
    need = 8 * nwave * n + (8 * L * nbands * n if contribution else 0)
    free = torch.cuda.mem_get_info()[0]
    if need > free:
        raise ValueError(f'posterior_summary: the spectrum store of {n} samples x {nwave} '
                         f'wavenumbers' +
                         (f' and the contribution store of {L} layers x {nbands} bands need'
                          if contribution else ' needs') +
                         f' {need} bytes, {free} bytes of device memory are free')
    device = params.device
    counts_d = counts.to(torch.int64) if counts_host is None else dev(counts_host, torch.int64)
    nspec = None
    spectra = torch.empty((chunk, nwave), dtype=torch.float64, device=device)
    stores = dict(spectrum=torch.empty((nwave, n), dtype=torch.float64, device=device),
                  bands=torch.empty((nbands, n), dtype=torch.float64, device=device),
                  temperature=torch.empty((L, n), dtype=torch.float64, device=device))
    cf = None
    if contribution:
        # (the pressure enters as diff(log p) only: the atmosphere's, in its own unit)
        kw = dict(kw, contribution_pressure=np.asarray(atmosphere.pressure, float))
        cf = torch.empty((chunk, L, nbands), dtype=torch.float64, device=device)
        stores['contribution'] = torch.empty((L, nbands, n), dtype=torch.float64, device=device)
    rejected = torch.empty(n, dtype=torch.bool, device=device)
    # (ideal gas: the total number density of a layer is p / (k T); here p / k per layer)
    pressure = dev(np.asarray(atmosphere.pressure, float) * BAR / K_BOLTZ)
    for w0 in range(0, n, chunk):
        w1 = min(w0 + chunk, n)
        m = w1 - w0
        prof = atmosphere.evaluate(params[w0:w1])
        ckw = {k: (v[w0:w1] if k in _PER_SAMPLE and v is not None else v) for k, v in kw.items()}
        if prof.continuum_density is not None:
            ckw['continuum_density'] = prof.continuum_density
        if prof.alkali_density is not None:
            ckw['alkali_density'] = prof.alkali_density
        if contribution:
            ckw['contribution_out'] = cf[:m]
        flux = model.eval_bands(prof.temps, prof.dens, bands, radius=prof.radius, chunk=m,
                                spectra_out=spectra[:m], **ckw)
        if contribution:
            stores['contribution'][:, :, w0:w1] = cf[:m].permute(1, 2, 0)
        if nspec is None:
            nspec = prof.dens.shape[2]
            stores['vmr'] = torch.empty((L, nspec, n), dtype=torch.float64, device=device)
        # the seams of the sample-minor stores: columns [w0, w1) of every row
        stores['spectrum'][:, w0:w1] = spectra[:m].t()
        stores['bands'][:, w0:w1] = flux.t()
        stores['temperature'][:, w0:w1] = prof.temps.t()
        # mole fractions of the table's species from the densities: n_s k T / p
        stores['vmr'][:, :, w0:w1] = (prof.dens * (prof.temps / pressure).unsqueeze(2)
                                      ).permute(1, 2, 0)
        rejected[w0:w1] = (prof.reject != 0) | torch.isposinf(flux).any(dim=1)
    live = torch.where(rejected, torch.zeros_like(counts_d), counts_d)
    # the one read-back: how many samples were rejected, and the length of the expansion
    n_rejected, total = (int(x) for x in torch.stack([rejected.sum(), live.sum()]).cpu())
    if total < 1:
        raise ValueError(f'posterior_summary: no sample is left ({n_rejected} of {n} rejected, '
                         'the others have count 0)')
    out = {name: weighted_quantiles(store, live, quantiles, total=total)
           for name, store in stores.items() if name != 'contribution'}
    median = None
    if contribution:
        median = weighted_quantiles(stores['contribution'], live, [0.5], total=total)[0]
    if keep_stores:
        stores['counts'] = live
    return PosteriorSummary(out['spectrum'], out['bands'], out['temperature'], out['vmr'],
                            n_rejected, quantiles, stores if keep_stores else None, median)
