"""Band contribution functions (Pyrat.band_contribution, pyrat/pyrat_obj.py:671-696 ->
spectrum/contribution_funcs.py), without clouds: the NumPy statements of the formulas that
pb_contribution.hip evaluates per walker on the device.

  transit geometry      transmittance: exp(-depth) above the layer where the column stopped, 0
                        from there on
  emission, two-stream  contribution_function: B d(exp(-tau)) / d(ln p), every column normalised
                        to a sum of 1 (Knutson et al. 2009, ApJ 690, 822, eq. 2)
  both                  band_cf: the pass bands' integrals over wavenumber, every band normalised
                        to a maximum of 1 over the layers

The device forms are batch.band_transmittance_batch and batch.band_contribution_emission_batch;
TableSpectrum.eval_bands(contribution_out=...) and TableSpectrum.band_contribution call them."""
import numpy as np

__all__ = ['transmittance_host', 'contribution_function_host', 'band_cf_host',
           'band_contribution_host']


def _trapezoid(y, x):
    """np.trapezoid(y, x, axis=1) (np.trapz before NumPy 2): d * (y[1:] + y[:-1]) / 2, summed."""
    d = np.diff(x)
    return np.sum(d * (y[:, 1:] + y[:, :-1]) / 2.0, axis=1)


def transmittance_host(depth, ideep):
    """depth[L, W] (transit optical depth per impact parameter), ideep[W] (the row at which each
    column exceeded maxdepth, or the last row evaluated) -> transmittance[L, W]: exp(-depth) in
    the rows above ideep, 0 in row ideep and below (completely opaque)."""
    depth = np.asarray(depth, float)
    out = np.exp(-depth)
    rows = np.arange(depth.shape[0])[:, None]
    out[rows >= np.asarray(ideep)[None, :]] = 0.0
    return out


def contribution_function_host(depth, pressure, planck):
    """depth[L, W] (plane-parallel optical depth: 0 in the rows up to itop and below the layer
    where the column stopped), pressure[L] (any unit), planck[L, W] -> cf[L, W].  The step of
    exp(-depth) from one layer to the next, with the steps above 0.1 -- the jump back to
    depth = 0 below the stop -- set to 0 (a smaller jump stays), times B over the step of ln p; a
    zero row for the last layer; every column divided by its sum over the layers."""
    depth = np.asarray(depth, float)
    planck = np.asarray(planck, float)
    detau = np.diff(np.exp(-depth), axis=0)
    detau[detau > 0.1] = 0.0
    dlogp = np.diff(np.log(np.asarray(pressure, float)))
    cf = planck[:-1] * detau / dlogp[:, None]
    cf = np.vstack([cf, np.zeros(planck.shape[1])])
    with np.errstate(invalid='ignore', divide='ignore'):
        return cf / np.sum(cf, axis=0)


def band_cf_host(contrib, responses, wn, indices):
    """contrib[L, W], responses / indices: per band the response curve and the samples of wn[W] it
    is given on -> [L, nbands]: the trapezoid integral over wavenumber of contrib x response per
    layer, every band divided by its maximum over the layers.  A band of one sample integrates to
    0 in every layer and comes out as 0 / 0 = NaN."""
    contrib = np.asarray(contrib, float)
    wn = np.asarray(wn, float)
    out = np.zeros((contrib.shape[0], len(responses)))
    for b, (response, idx) in enumerate(zip(responses, indices)):
        out[:, b] = _trapezoid(contrib[:, idx] * np.asarray(response, float), wn[idx])
    with np.errstate(invalid='ignore', divide='ignore'):
        out /= np.amax(out, axis=0)
    return out


def band_contribution_host(depth, ideep, responses, wn, indices, rt_path='transit',
                           pressure=None, planck=None):
    """Pyrat.band_contribution without clouds from an optical depth: rt_path 'transit' takes
    depth and ideep, any other geometry (emission, two-stream) depth, pressure[L] and
    planck[L, W] -> [L, nbands]."""
    if rt_path == 'transit':
        contrib = transmittance_host(depth, ideep)
    else:
        if pressure is None or planck is None:
            raise ValueError('band_contribution_host: emission geometry needs pressure and planck')
        contrib = contribution_function_host(depth, pressure, planck)
    return band_cf_host(contrib, responses, wn, indices)
