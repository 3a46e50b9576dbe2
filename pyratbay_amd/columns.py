"""Column stages of ONE spectrum (device tensors in, device tensors out) and the host pre-computes
of their callers: ray paths, optical depth, transmission, emission and two-stream fluxes, what is
made of an emission-type flux afterwards, the quadrature of the emission geometry, loglike."""
import numpy as np
import torch

from . import _capi
from ._capi import call
from ._device import _ptr, _stream


# --------------------------------------------------------------------------
# Host pre-computes of the callers
# --------------------------------------------------------------------------
def transit_path(radius, nskip=0):
    """Chord segments between concentric shells for each impact parameter
    (pyratbay/atmosphere/atmosphere.py:737-802)."""
    rad = np.asarray(radius, float)[nskip:]
    # The reference squares SCALARS (`rad[i]**2`: libm pow), and pow(x, 2) is not always the
    # correctly rounded x*x that NumPy's array power computes (0.09 % of values differ by one
    # ulp).  Every square here is the scalar pow, like there: mixing the two forms makes
    # rad[r]**2 - rad[r]**2 non-zero, and its square root NaN, for one atmosphere in ~30.
    sq = np.array([x**2 for x in rad.tolist()], float)
    path = [np.empty(0) for _ in range(nskip)]
    for r in range(len(rad)):
        path.append(np.sqrt(sq[:r] - sq[r]) - np.sqrt(sq[1:r + 1] - sq[r]))
    return path


def pack_raypath(raypath, itop):
    """Lower triangle of transit_path(radius, itop) as one array (pbhip.h layout)."""
    rows = [np.asarray(p, float) for p in raypath[itop:]]
    for r, p in enumerate(rows):
        assert len(p) == r, 'raypath must come from transit_path(radius, itop)'
    return np.concatenate(rows) if rows else np.empty(0)


def transit_path_device(radius, itop=0):
    """atmosphere.transit_path on the device: radius[L] or [nw, L] (device) -> packed lower
    triangle [n(n-1)/2] or [nw, n(n-1)/2], n = L - itop (pb_transit_path)."""
    rad = radius if radius.dim() == 2 else radius.view(1, -1)
    nw, nlayers = rad.shape
    n = nlayers - itop
    out = torch.empty((nw, (n * (n - 1)) // 2), dtype=torch.float64, device=rad.device)
    call('pb_transit_path', _ptr(out), _ptr(rad.contiguous()), int(itop), nlayers, nw, _stream())
    return out if radius.dim() == 2 else out[0]


# --------------------------------------------------------------------------
# Column stages (device tensors in, device tensors out)
# --------------------------------------------------------------------------
def optical_depth_transit(ec, raypath_packed, itop, ibottom, maxdepth):
    """optic_depth.py:103-112.  ec[L,W] -> depth[L,W], ideep[W] (int32)."""
    nlayers, nwave = ec.shape
    depth = torch.empty_like(ec)
    ideep = torch.empty(nwave, dtype=torch.int32, device=ec.device)
    call('pb_optical_depth_transit', _ptr(depth), _ptr(ideep), _ptr(ec),
         _ptr(raypath_packed), int(itop), int(ibottom), float(maxdepth), nlayers, nwave,
         _stream())
    return depth, ideep


def transit_spectrum(ec, raypath_packed, radius, rstar, itop, ibottom, maxdepth,
                     deck_rsurf=None, deck_itop=None, out=None):
    """optic_depth.py:103-112 + radiative_transfer.py:57-71 in one call:
    ec[L,W] -> spectrum[W], depth[L,W], ideep[W].  With an opaque cloud deck pass its
    radius and the index of the layer right below it (and ibottom = deck_itop + 1).
    out: a contiguous [W] tensor to receive the spectrum (a shard's slot of a gather buffer)."""
    nlayers, nwave = ec.shape
    depth = torch.empty_like(ec)
    ideep = torch.empty(nwave, dtype=torch.int32, device=ec.device)
    if out is not None:
        assert out.shape == (nwave,) and out.dtype == torch.float64 and out.is_contiguous()
    spectrum = out if out is not None else torch.empty(nwave, dtype=torch.float64,
                                                       device=ec.device)
    call('pb_transit_spectrum_deck', _ptr(spectrum), _ptr(depth), _ptr(ideep), _ptr(ec),
         _ptr(raypath_packed), _ptr(radius), float(rstar), int(itop), int(ibottom),
         float(maxdepth), -1 if deck_rsurf is None else int(deck_itop),
         0.0 if deck_rsurf is None else float(deck_rsurf), nlayers, nwave, _stream())
    return spectrum, depth, ideep


def patchy_transit_spectrum(ec, ec_cloud, fpatchy, raypath_packed, radius, rstar, itop,
                            maxdepth, deck_rsurf=None, deck_itop=None):
    """Patchy clouds, transit geometry (opacity/optic_depth.py:94-121 +
    pyrat/spectrum.py:350-363): the cloudy atmosphere is ec + ec_cloud (from itop down) with
    the opaque deck, if any, as its bottom; the clear one is ec over all layers; the spectrum
    is their fpatchy-weighted mean.  -> (spectrum, clear, cloudy), each [W]."""
    nlayers = ec.shape[0]
    ec_cloudy = ec.clone()
    ec_cloudy[itop:] += ec_cloud[itop:]
    ibottom = nlayers if deck_rsurf is None else int(deck_itop) + 1
    cloudy, _, _ = transit_spectrum(ec_cloudy, raypath_packed, radius, rstar, itop, ibottom,
                                    maxdepth, deck_rsurf, deck_itop)
    clear, _, _ = transit_spectrum(ec, raypath_packed, radius, rstar, itop, nlayers, maxdepth)
    return fpatchy * cloudy + (1.0 - fpatchy) * clear, clear, cloudy


def patchy_emission_flux(ec, ec_cloud, fpatchy, intervals, wn, temp, mu, weights, itop,
                         maxdepth, deck_tsurf=None, deck_itop=None):
    """Patchy clouds, plane-parallel emission (opacity/optic_depth.py:123-136 +
    pyrat/spectrum.py:366-385).  -> (flux, clear, cloudy), each [W]."""
    nlayers = ec.shape[0]
    ec_cloudy = ec.clone()
    ec_cloudy[itop:] += ec_cloud[itop:]
    ibottom = nlayers if deck_tsurf is None else int(deck_itop) + 1
    depth, ideep = plane_parallel_optical_depth(ec_cloudy, intervals, itop, ibottom, maxdepth)
    cloudy = emission_flux(depth, ideep, wn, temp, mu, weights, itop,
                           cloud_tsurf=deck_tsurf, cloud_itop=deck_itop)
    depth, ideep = plane_parallel_optical_depth(ec, intervals, itop, nlayers, maxdepth)
    # The reference's cloudy pass overwrites row deck_itop of its Planck array with the
    # cloud-top emission IN PLACE (spectrum/radiative_transfer.py:125-126) and the clear pass
    # then integrates that same array (pyrat/spectrum.py:380-383): its "clear" atmosphere
    # emits at the cloud-top temperature in that one layer.  Reproduced, not corrected.
    temp_clear = temp
    if deck_tsurf is not None:
        temp_clear = temp.clone()
        temp_clear[int(deck_itop)] = float(deck_tsurf)
    clear = emission_flux(depth, ideep, wn, temp_clear, mu, weights, itop)
    return fpatchy * cloudy + (1.0 - fpatchy) * clear, clear, cloudy


def plane_parallel_optical_depth(ec, intervals, itop, ibottom, maxdepth, depth=None):
    """optic_depth.py:122-130.  Rows below the stopping layer stay zero."""
    nlayers, nwave = ec.shape
    if depth is None:
        depth = torch.zeros_like(ec)
    ideep = torch.full((nwave,), nlayers - 1, dtype=torch.int32, device=ec.device)
    call('pb_plane_parallel_optical_depth', _ptr(depth), _ptr(ideep), _ptr(ec),
         _ptr(intervals), float(maxdepth), int(itop), int(ibottom), nlayers, nwave, _stream())
    return depth, ideep


def transmission(depth, ideep, radius, itop, rstar, deck_rsurf=None, deck_itop=None):
    """radiative_transfer.py:17-71 -> spectrum[W]; deck_rsurf / deck_itop = radius of an
    opaque cloud deck and index of the layer right below it."""
    nlayers, nwave = depth.shape
    spectrum = torch.empty(nwave, dtype=torch.float64, device=depth.device)
    call('pb_transmission_deck', _ptr(spectrum), _ptr(depth), _ptr(ideep), _ptr(radius),
         int(itop), float(rstar), -1 if deck_rsurf is None else int(deck_itop),
         0.0 if deck_rsurf is None else float(deck_rsurf), nlayers, nwave, _stream())
    return spectrum


def emission_flux(depth, ideep, wn, temp, mu, weights, rtop, want_intensity=False,
                  cloud_tsurf=None, cloud_itop=None):
    """pyrat/spectrum.py:366-377: Planck + intensity per mu + quadrature sum.  With an
    opaque cloud deck (radiative_transfer.py:121-131) the layer cloud_itop radiates at
    cloud_tsurf and is the deepest one seen."""
    nlayers, nwave = depth.shape
    flux = torch.empty(nwave, dtype=torch.float64, device=depth.device)
    inten = (torch.empty((len(mu), nwave), dtype=torch.float64, device=depth.device)
             if want_intensity else None)
    itop_cloud = -1
    if cloud_tsurf is not None:
        temp = temp.clone()
        temp[int(cloud_itop)] = float(cloud_tsurf)
        itop_cloud = int(cloud_itop)
    call('pb_emission_flux_deck', _ptr(flux), _ptr(inten), _ptr(depth), _ptr(ideep), _ptr(wn),
         _ptr(temp), _ptr(mu), _ptr(weights), len(mu), int(rtop), itop_cloud, nlayers, nwave,
         _stream())
    return (flux, inten) if want_intensity else flux


# the reference's rt_path values by family (constants/code_constants.py:83-102) -> (geometry of the
# radiative transfer here, what is made of the flux afterwards)
RT_PATHS = {
    'transit': ('transit', None),
    'emission': ('emission', 'emission'),
    'eclipse': ('emission', 'eclipse'),
    'f_lambda': ('emission', 'f_lambda'),
    'two_stream': ('two_stream', 'emission'),
    'emission_two_stream': ('two_stream', 'emission'),
    'eclipse_two_stream': ('two_stream', 'eclipse'),
}


def emission_observables(flux, kind='emission', starflux=None, rplanet=None, rstar=None,
                         f_dilution=None, wn=None, distance=None, in_place=False):
    """What the reference makes of a plane-parallel flux after the radiative transfer
    (pyrat/spectrum.py:394-405, eval()'s f_lambda conversion pyrat_obj.py:323-329), one launch:
    flux[W] -> (spectrum[W], fplanet[W]).
      fplanet = flux [* f_dilution]
      kind 'emission': spectrum = fplanet (the same tensor, as in the reference)
      kind 'eclipse' : spectrum = fplanet * (1/starflux * (rplanet/rstar)**2)
      kind 'f_lambda': spectrum = 10 * fplanet * (rplanet/distance * wn * 1e-4)**2
    in_place: fplanet is written over `flux`."""
    mode = {'emission': 0, 'eclipse': 1, 'f_lambda': 2}[kind]
    n = flux.shape[0]
    scale = 0.0
    if mode == 1:
        if starflux is None or rplanet is None or rstar is None:
            raise _capi.PbError('eclipse: starflux[W], rplanet and rstar are needed '
                                '(pyrat/argum.py:37-44)')
        assert starflux.shape == flux.shape
        scale = (float(rplanet) / float(rstar))**2
    if mode == 2:
        if wn is None or rplanet is None or distance is None:
            raise _capi.PbError('f_lambda: wn[W], rplanet and distance are needed')
        assert wn.shape == flux.shape
        scale = float(rplanet) / float(distance)
    if mode == 0 and f_dilution is None:
        return flux, flux                                   # (`spec.fplanet = spec.spectrum`)
    fplanet = flux if in_place else torch.empty_like(flux)
    spectrum = fplanet if mode == 0 else torch.empty_like(flux)
    call('pb_emission_observables', _ptr(spectrum), None if mode == 0 else _ptr(fplanet),
         _ptr(flux), _ptr(starflux), _ptr(wn), n, mode, 0 if f_dilution is None else 1,
         0.0 if f_dilution is None else float(f_dilution), scale, _stream())
    return spectrum, fplanet


def loglike(bandflux, data, uncert):
    """tools/retrieval_tools.py:98-104 for a batch of walkers: bandflux[nw, nbands] (or
    [nbands]) -> loglike[nw]; a non-finite value becomes -1e98, the reference's reject value."""
    bf = bandflux if bandflux.dim() == 2 else bandflux.view(1, -1)
    out = torch.empty(bf.shape[0], dtype=torch.float64, device=bf.device)
    call('pb_loglike', _ptr(out), _ptr(bf.contiguous()), _ptr(data), _ptr(uncert), bf.shape[0],
         bf.shape[1], _stream())
    return out


def internal_flux(wn, tint):
    """f_int of pyrat/spectrum.py:475-478 (Planck at tint scaled to sigma*tint^4)."""
    out = torch.empty(wn.shape[0], dtype=torch.float64, device=wn.device)
    call('pb_internal_flux', _ptr(out), _ptr(wn), float(tint), wn.shape[0], _stream())
    return out


def two_stream(depth, wn, temp, f_int=None, flux_top=None, rtop=0):
    """pyrat/spectrum.py:454-522 -> (flux_down, flux_up) [L,W]; the emission spectrum is
    flux_up[0].  flux_top = beta_irr*(rstar/smaxis)**2*starflux (or None)."""
    nlayers, nwave = depth.shape
    down = torch.empty((nlayers, nwave), dtype=torch.float64, device=depth.device)
    up = torch.empty((nlayers, nwave), dtype=torch.float64, device=depth.device)
    call('pb_two_stream', _ptr(down), _ptr(up), _ptr(depth), _ptr(wn), _ptr(temp),
         _ptr(f_int), _ptr(flux_top), int(rtop), nlayers, nwave, _stream())
    return down, up


def blackbody_wn_2D(wn, temp, last=None):
    B = torch.zeros((temp.shape[0], wn.shape[0]), dtype=torch.float64, device=wn.device)
    call('pb_blackbody_wn_2D', _ptr(B), _ptr(wn), wn.shape[0], _ptr(temp), temp.shape[0],
         _ptr(last), _stream())
    return B


def intensity(tau, ideep, planck, mu, rtop):
    nlayers, nwave = tau.shape
    out = torch.empty((mu.shape[0], nwave), dtype=torch.float64, device=tau.device)
    call('pb_intensity', _ptr(out), _ptr(tau), _ptr(ideep), _ptr(planck), _ptr(mu),
         mu.shape[0], int(rtop), nlayers, nwave, _stream())
    return out


def interp_ec(extinction, etable, ttable, temperatures, density, lay1, lay2, per_mol=False,
              assign=False):
    """_extcoeff.interp_ec[_per_mol]: accumulates into `extinction`; assign=True writes the
    rows lay1..lay2 instead (no need to zero them first)."""
    nmol, ntemp, nlayers, nwave = etable.shape
    call('pb_interp_ec_set' if assign else 'pb_interp_ec', _ptr(extinction), _ptr(etable),
         _ptr(ttable), _ptr(temperatures),
         _ptr(density), nmol, ntemp, nlayers, nwave, int(lay1), int(lay2), int(per_mol),
         _stream())
    return extinction


def default_quadrature():
    """(mu, weights) of the reference when `quadrature` is unset: raygrid = 0, 20, 40, 60, 80
    degrees, weights = the solid angle between the mid-points (pyrat/spectrum.py:30-58)."""
    raygrid = np.radians([0.0, 20.0, 40.0, 60.0, 80.0])
    bounds = np.linspace(0, 0.5 * np.pi, len(raygrid) + 1)
    bounds[1:-1] = 0.5 * (raygrid[:-1] + raygrid[1:])
    return np.cos(raygrid), np.pi * (np.sin(bounds[1:])**2 - np.sin(bounds[:-1])**2)


def _legendre_newton(n):
    """Gauss-Legendre nodes and weights on [-1, 1] by Newton's iteration on P_n in extended
    precision, ascending nodes.  Correctly rounded to ~1 ulp -- which is NOT what the reference
    uses: SciPy's roots_legendre (Golub-Welsch eigenvalues + one Newton step) is up to 3 ulp off
    in the nodes and up to 1.5e-13 relative in the weights at n <= 16 (tests/test_host_logic.py)."""
    ld = np.longdouble
    k = np.arange(1, n + 1, dtype=ld)
    x = np.cos(np.pi * (k - ld(0.25)) / (n + ld(0.5)))

    def pn(x):
        p0, p1 = np.ones_like(x), x.copy()
        for j in range(2, n + 1):
            p0, p1 = p1, ((2 * j - 1) * x * p1 - (j - 1) * p0) / j
        return p1, n * (x * p1 - p0) / (x * x - 1)
    for _ in range(60):
        p, dp = pn(x)
        dx = p / dp
        x = x - dx
        if np.max(np.abs(dx)) < 1e-19:
            break
    _, dp = pn(x)
    w = 2 / ((1 - x * x) * dp * dp)
    return x[::-1].astype(float), w[::-1].astype(float)


def gauss_quadrature(n, use_scipy=True):
    """(mu, weights) of the reference for `quadrature = n` (pyrat/spectrum.py:41-49):
    Gauss-Legendre nodes x_i, weights w_i of order n mapped to q = (x + 1) / 2, mu = sqrt(q),
    weights = pi/2 w -- the flux integral  2 pi Int_0^1 I(mu) mu dmu = pi Int_0^1 I dq.  The
    reference takes (x, w) from scipy.special.p_roots; so does this function when SciPy is
    importable (same call of the same third-party library: bit-identical mu and weights --
    tests/golden/g18_p_roots.npz holds SciPy 1.15.3's values); without SciPy (or with
    use_scipy=False) the nodes come from _legendre_newton (within 3 ulp / 1.5e-13 of SciPy's).
    n <= 16: the emission kernels keep at most 16 running sums per column."""
    n = int(n)
    if not 1 <= n <= 16:
        raise ValueError(f'quadrature = {n}: 1 ... 16 nodes are supported')
    nodes = weights = None
    if use_scipy:
        try:
            from scipy.special import roots_legendre
            nodes, weights = roots_legendre(n)
        except ImportError:
            pass
    if nodes is None:
        nodes, weights = _legendre_newton(n)
    qnodes = 0.5 * (nodes + 1.0)
    return np.sqrt(qnodes), 0.5 * np.pi * weights
