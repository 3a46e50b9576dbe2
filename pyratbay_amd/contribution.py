"""Band contribution functions (Pyrat.band_contribution, pyrat/pyrat_obj.py:671-696 ->
spectrum/contribution_funcs.py), clear and with clouds: the NumPy statements of the formulas that
pb_contribution.hip evaluates per walker on the device.

  transit geometry      transmittance: exp(-depth) above the layer where the column stopped, 0
                        from there on
  emission, two-stream  contribution_function: B d(exp(-tau)) / d(ln p), every column normalised
                        to a sum of 1 (Knutson et al. 2009, ApJ 690, 822, eq. 2)
  both                  band_cf: the pass bands' integrals over wavenumber, every band normalised
                        to a maximum of 1 over the layers

With clouds (an opaque deck, cloud-type opacity, a patchy fraction; pyrat_obj.py:129-164, 683-693)
the reference has a cloudy column, ec + ec_cloud down to the deck, and -- patchy -- a clear one:

  transit geometry      patchy: f transmittance(cloudy) + (1 - f) transmittance(clear), element by
                        element before band_cf; else the cloudy column's transmittance
  emission              contribution_function of the CLOUDY column only, patchy or not (the
                        reference does not mix the clear column in, and f does not enter), with
                        the deck's temperature in the deck layer's row of B

The device forms are batch.band_transmittance_batch and batch.band_contribution_emission_batch,
with clouds batch.band_transmittance_cloudy_batch and
batch.band_contribution_emission_cloudy_batch; TableSpectrum.eval_bands(contribution_out=...) and
TableSpectrum.band_contribution call them."""
import numpy as np

__all__ = ['transmittance_host', 'contribution_function_host', 'band_cf_host',
           'band_contribution_host', 'transmittance_patchy_host', 'band_contribution_cloudy_host']


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


def transmittance_patchy_host(depth, ideep, depth_clear, ideep_clear, f_patchy):
    """The transmittance of a patchy model (pyrat_obj.py:684-689): depth / ideep of the cloudy
    column (rows itop .. deck itop evaluated, 0 elsewhere; ideep at most the deck's layer),
    depth_clear / ideep_clear of the clear one, f_patchy the cloudy fraction ->
    f transmittance(cloudy) + (1 - f) transmittance(clear) [L, W], element by element.  The
    fraction is used as given: the device clamps it to [0, 1] first."""
    f = float(f_patchy)
    return f * transmittance_host(depth, ideep) + \
        (1.0 - f) * transmittance_host(depth_clear, ideep_clear)


def band_contribution_cloudy_host(depth, ideep, responses, wn, indices, rt_path='transit',
                                  depth_clear=None, ideep_clear=None, f_patchy=None,
                                  pressure=None, planck=None):
    """Pyrat.band_contribution with clouds from the optical depths of the two columns
    (opacity/optic_depth.py:91-136) -> [L, nbands].  depth / ideep: the cloudy column.
    rt_path 'transit': with f_patchy (not None) also depth_clear / ideep_clear, mixed by
    transmittance_patchy_host; without, the cloudy column alone.  Any other geometry: the
    contribution function of the CLOUDY depth only, as the reference -- depth_clear, ideep_clear
    and f_patchy are accepted and change nothing -- with pressure[L] and planck[L, W], whose row
    at the deck's layer holds the Planck function at the deck's temperature
    (spectrum/radiative_transfer.py:125-127 writes it in place)."""
    if rt_path == 'transit':
        if f_patchy is None:
            contrib = transmittance_host(depth, ideep)
        else:
            if depth_clear is None or ideep_clear is None:
                raise ValueError('band_contribution_cloudy_host: a patchy model needs depth_clear '
                                 'and ideep_clear')
            contrib = transmittance_patchy_host(depth, ideep, depth_clear, ideep_clear, f_patchy)
    else:
        if pressure is None or planck is None:
            raise ValueError('band_contribution_cloudy_host: emission geometry needs pressure and '
                             'planck')
        contrib = contribution_function_host(depth, pressure, planck)
    return band_cf_host(contrib, responses, wn, indices)
