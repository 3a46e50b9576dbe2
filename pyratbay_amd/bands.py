"""The exits of the batched loop: pass bands and high-resolution data resident on the device."""
import numpy as np
import torch

from . import hires
from ._capi import call
from ._device import _ptr, _stream, dev


class PassBands:
    """A set of pass bands resident on the device (PassBand.set_sampling/integrate,
    pyratbay/spectrum/spec_tools.py:120-233).  Each band is (start index on the global
    wavenumber grid, response sampled on wn[start:start+count], height); for photon
    counting the caller folds the wavelength factor into the response."""

    def __init__(self, wn, bands):
        self.nbands = len(bands)
        self.wn = dev(wn)
        start = np.array([b[0] for b in bands], np.int32)
        count = np.array([len(b[1]) for b in bands], np.int32)
        offset = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
        self.max_count = int(count.max()) if len(count) else 0     # (the contribution kernels' grid)
        self.start, self.count = dev(start, torch.int32), dev(count, torch.int32)
        self.offset = dev(offset, torch.int64)
        self.response = dev(np.concatenate([np.asarray(b[1], float) for b in bands]))
        self.heights = dev(np.array([b[2] for b in bands], float))
        self.partial = torch.zeros(self.nbands, dtype=torch.float64, device='cuda')
        self.scale = None               # per-band factor after the heights (set_eclipse)
        self.star_grid = None           # a StellarGrid: the factor per walker (set_eclipse_grid)

    def partial_integrate(self, spectrum_full, wbegin=0, wcount=None):
        """Un-scaled partial sums over the pairs whose left sample is in the shard."""
        if wcount is None:
            wcount = spectrum_full.shape[0] - wbegin
        call('pb_band_integrate', _ptr(self.partial), _ptr(spectrum_full), _ptr(self.wn),
             _ptr(self.start), _ptr(self.count), _ptr(self.response), _ptr(self.offset),
             self.nbands, int(wbegin), int(wcount), _stream())
        return self.partial

    def set_eclipse(self, rplanet, rstar, bandflux_star):
        """Eclipse geometry: integrate_batch() then returns band(fplanet) * rprs**2 / bandflux_star
        (Pyrat.band_integrate, pyrat_obj.py:662-665).  bandflux_star[nbands] = the band integrals
        of the stellar flux (pyrat/argum.py:86-90: `star_bandflux()` computes them here)."""
        rprs = float(rplanet) / float(rstar)
        self.scale = dev(rprs**2.0 / np.asarray(bandflux_star, float))
        return self

    def star_bandflux(self, starflux):
        """bandflux_star of pyrat/argum.py:86-90: the bands' integrals of starflux[W] -> [nbands]
        (host array)."""
        scale, self.scale = self.scale, None
        try:
            out = self.integrate_batch(dev(starflux).view(1, -1))[0]
        finally:
            self.scale = scale
        return out.cpu().numpy()

    def set_eclipse_grid(self, rstar, star, rplanet=None):
        """Eclipse geometry with a stellar temperature per walker (eval()'s tstar branch,
        pyrat_obj.py:288-294): star, an observation.StellarGrid on these bands' grid;
        integrate_batch(..., tstar=tstar[nw]) then returns band(fplanet) * rprs**2 /
        band(star.flux(tstar[w])) per walker, the stellar band fluxes re-integrated on the device
        (pb_star_band_scale_batch).  rprs = rplanet / rstar with the planet radius given here, or
        with integrate_batch's rplanet[nw] (a free rplanet changes the factor too:
        Pyrat.band_integrate, pyrat_obj.py:662-665, reads the current atm.rplanet).
        DEVIATION: a walker whose tstar is NaN or outside the grid's temperatures gets +inf in
        every band (the reference's interp1d raises): rejected like a walker outside the table's
        temperatures.  set_eclipse(), star_bandflux() and a call without tstar are unchanged."""
        if star.nwave != self.wn.shape[0] or \
                not np.array_equal(star.wn_host, self.wn.cpu().numpy()):
            raise ValueError('set_eclipse_grid: the StellarGrid is not on the wavenumbers of '
                             'these bands')
        if not float(rstar) > 0.0:
            raise ValueError(f'set_eclipse_grid: rstar must be positive, got {rstar}')
        self.star_grid = star
        self.grid_rstar = float(rstar)
        self.grid_rplanet = None if rplanet is None else float(rplanet)
        return self

    def integrate_batch(self, spectra, out=None, f_dilution=None, tstar=None, rplanet=None):
        """Band fluxes (heights applied; then the walkers' dilution factors f_dilution[nw], if
        given, and the eclipse factor, if set) of full-grid spectra[nw, W] -> [nw, nbands].
        tstar[nw] (with rplanet[nw], or the planet radius of set_eclipse_grid): the eclipse factor
        of each walker's stellar temperature, from the grid of set_eclipse_grid."""
        nw, nwave = spectra.shape
        if out is None:
            out = torch.empty((nw, self.nbands), dtype=torch.float64, device=spectra.device)
        call('pb_band_integrate_batch', _ptr(out), _ptr(spectra), _ptr(self.wn),
             _ptr(self.start), _ptr(self.count), _ptr(self.response), _ptr(self.offset),
             _ptr(self.heights), self.nbands, nwave, nw, _stream())
        if tstar is not None:
            star = self.star_grid
            if star is None:
                raise ValueError('integrate_batch: tstar needs set_eclipse_grid()')
            if rplanet is None and self.grid_rplanet is None:
                raise ValueError('integrate_batch: a planet radius is needed, here (rplanet[nw]) '
                                 'or in set_eclipse_grid()')
            assert tstar.shape == (nw,) and (rplanet is None or rplanet.shape == (nw,))
            assert f_dilution is None or f_dilution.shape == (nw,)
            assert nwave == star.nwave
            rprs2 = 0.0 if rplanet is not None else (self.grid_rplanet / self.grid_rstar)**2.0
            call('pb_star_band_scale_batch', _ptr(out), _ptr(star.fluxes), _ptr(star.sed_temps),
                 _ptr(tstar.contiguous()), rprs2,
                 None if rplanet is None else _ptr(rplanet.contiguous()), self.grid_rstar,
                 _ptr(f_dilution), _ptr(self.wn), _ptr(self.start), _ptr(self.count),
                 _ptr(self.response), _ptr(self.offset), _ptr(self.heights), star.nt, self.nbands,
                 nwave, nw, _stream())
            return out
        if rplanet is not None:
            raise ValueError('integrate_batch: rplanet[nw] belongs to tstar[nw] and '
                             'set_eclipse_grid()')
        if self.scale is not None or f_dilution is not None:
            assert f_dilution is None or f_dilution.shape == (nw,)
            call('pb_band_scale', _ptr(out), _ptr(self.scale), _ptr(f_dilution), self.nbands, nw,
                 _stream())
        return out


class HiresData:
    """High-resolution spectroscopic data as the exit of the batched loop (eval()'s second exit,
    pyrat/pyrat_obj.py:331-356): the model spectrum convolved with the instrument profile of
    resolving power inst_resolution (ps.inst_convolution), the grid Doppler-shifted by each
    walker's radial velocity (ps.rv_shift) and the result sampled at data_wn by interp1d's linear
    rule.  wn: the model's grid (ascending); sampling_res: the grid's resolving power when it is a
    constant-resolution grid (the reference's spec.resolution), None: taken from the grid's steps;
    data_wn: in any order -- sorted once here, integrate_batch() returns the caller's order.
    rv_max (km/s): walkers beyond it are rejected (+inf, like eval()'s reject path); the
    constructor refuses data that can leave the shifted grid within +-rv_max (where the
    reference's interp1d raises); check_data=False leaves that to the device, which rejects a
    walker whose data leave ITS shifted grid.

    integrate_batch() is ONE fused launch (pb_hires_observe_batch): the convolved spectra
    [nw, W] are never stored, and only the convolved samples that a data point brackets are
    computed.  `fused = False` takes the two-launch form instead (convolve() into a [nw, W]
    buffer, then the same kernel with a single unit tap): the same bits, kept for comparison."""

    def __init__(self, wn, data_wn, inst_resolution, sampling_res=None, rv_max=100.0,
                 check_data=True):
        wn_host = np.ascontiguousarray(wn.cpu().numpy() if isinstance(wn, torch.Tensor) else wn,
                                       dtype=np.float64)
        data_host = np.ascontiguousarray(data_wn, dtype=np.float64)
        hires.check_data_in_grid(wn_host, data_host, rv_max, span=check_data)
        taps = hires.inst_kernel(inst_resolution, wn=wn_host, sampling_res=sampling_res)
        if len(taps) > hires.MAX_TAPS:
            raise ValueError(f'HiresData: the instrument profile spans {len(taps)} samples of '
                             f'the grid, at most {hires.MAX_TAPS} are supported')
        self.inst_resolution, self.sampling_res = inst_resolution, sampling_res
        self.rv_max = float(rv_max)
        self.nwave = len(wn_host)
        self.nbands = self.ndata = len(data_host)
        self.taps_host = taps
        order = np.argsort(data_host, kind='stable')
        self.wn = dev(wn_host)
        self.taps = dev(taps)
        self.data_wn_sorted = dev(data_host[order])
        self.data_slot = dev(order, torch.int32)
        self.unit_tap = dev(np.ones(1))
        self.sample_scale = None        # per-sample factor before the convolution
        self.fused = True

    def set_eclipse(self, rplanet, rstar, starflux):
        """Eclipse geometry: every sample of fplanet is multiplied by 1/starflux * rprs**2 BEFORE
        the convolution (pyrat/spectrum.py:401-404 -- pb_emission_observables' mode 1)."""
        starflux = np.asarray(starflux, float)
        assert starflux.shape == (self.nwave,)
        self.sample_scale = dev(1 / starflux * (float(rplanet) / float(rstar))**2)
        return self

    def set_f_lambda(self, rplanet, distance):
        """f_lambda geometry: erg s-1 cm-2 cm to W m-2 um-1 per sample before the convolution
        (pyrat_obj.py:323-329 -- pb_emission_observables' mode 2: 10 (rplanet/distance wn um)^2,
        here as ONE factor per sample: within an ulp of the reference's two products)."""
        t = float(rplanet) / float(distance) * self.wn.cpu().numpy() * 1.0e-4
        self.sample_scale = dev(10.0 * (t * t))
        return self

    def convolve(self, spectra):
        """spectra[nw, W] (x the per-sample factor, if set) convolved with the instrument profile
        -> [nw, W], the reference's spec.spectrum_convolved."""
        nw, nwave = spectra.shape
        assert nwave == self.nwave
        out = torch.empty_like(spectra)
        call('pb_inst_convolve_batch', _ptr(out), _ptr(spectra), _ptr(self.taps),
             _ptr(self.sample_scale), len(self.taps_host), nwave, nw, _stream())
        return out

    def integrate_batch(self, spectra, out=None, f_dilution=None, rv=None):
        """Model values at the data of full-grid spectra[nw, W] -> [nw, ndata] in the order of
        data_wn.  rv[nw]: the walkers' radial velocities in km/s (None: no shift); f_dilution[nw]:
        the walkers' dilution factors, applied per sample first (pyrat/spectrum.py:395-396)."""
        nw, nwave = spectra.shape
        assert nwave == self.nwave
        assert rv is None or rv.shape == (nw,)
        assert f_dilution is None or f_dilution.shape == (nw,)
        if out is None:
            out = torch.empty((nw, self.ndata), dtype=torch.float64, device=spectra.device)
        rv = None if rv is None else rv.contiguous()
        if self.fused:
            call('pb_hires_observe_batch', _ptr(out), _ptr(spectra), _ptr(self.wn),
                 _ptr(self.taps), _ptr(self.sample_scale), _ptr(self.data_wn_sorted),
                 _ptr(self.data_slot), _ptr(rv), _ptr(f_dilution), self.rv_max,
                 len(self.taps_host), nwave, self.ndata, nw, _stream())
            return out
        if f_dilution is not None:
            spectra = spectra * f_dilution.view(-1, 1)
        call('pb_hires_observe_batch', _ptr(out), _ptr(self.convolve(spectra)), _ptr(self.wn),
             _ptr(self.unit_tap), None, _ptr(self.data_wn_sorted), _ptr(self.data_slot),
             _ptr(rv), None, self.rv_max, 1, nwave, self.ndata, nw, _stream())
        return out
