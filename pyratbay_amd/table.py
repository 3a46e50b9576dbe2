"""Retrieval inner loop on sampled cross sections: TableSpectrum, and the three steps of its
batched form eval_bands -- validate (BatchCall), plan (plan_eval_bands -> BatchPlan: which form a
chunk runs, decided once per call by a pure function) and run (_eval_chunk: one step per stage).
The batch wrappers are looked up in the module `batch` at call time."""
import contextlib
import os
from collections import namedtuple

import numpy as np
import torch

from . import _capi, batch, posterior
from ._capi import call
from ._device import StageTimer, _ptr, _stream, dev, require_gpu, side_streams
from .bands import HiresData
from .batch import _check_walker_tensor
from .columns import (RT_PATHS, default_quadrature, emission_flux, internal_flux, interp_ec,
                      pack_raypath, plane_parallel_optical_depth, transit_path,
                      transit_path_device, transit_spectrum, two_stream)
from .observation import StellarGrid
from .radeq import RadiativeEquilibrium


# What the caller of eval_bands gave, validated and filled by name (TableSpectrum._batch_call).
# radius is [1, L] when shared_radius; out[nw, nbands] receives the result; cloudy: the call takes
# the cloud form; tmin / tmax: the temperatures outside which a walker is rejected; path1: the ray
# path of a shared radius in transit geometry (set once the column order is settled);
# contribution_out[nw, L, nbands] receives the band contribution functions (None: not asked for),
# dlogp[L-1] = diff(log(contribution_pressure)) on the device (emission and two-stream geometry);
# tstar[nw] / rplanet[nw]: the walkers' stellar temperatures and planet radii for the eclipse
# factor of bands.set_eclipse_grid (None: not given).  On a model with isotope ratios temps and
# dens are the SCALED tensors (isotopes.IsotopeRatios.scale): zeros for a walker it rejects.
BatchCall = namedtuple('BatchCall', (
    'temps dens bands radius shared_radius f_dilution continuum_density continuum_pars '
    'alkali_density rv deck_logp f_patchy spectra_out out nw cloudy tmin tmax path1 '
    'contribution_out dlogp tstar rplanet'),
    defaults=(None, None, None, None, None))

# Which kernels the chunks of one eval_bands call run (plan_eval_bands).  form: 'one_pass',
# 'two_stream', 'emission', 'transit' or 'clouds'; table / wn / column name the attributes of the
# model a chunk reads (column None: grid order).
BatchPlan = namedtuple('BatchPlan', 'form ordered limited table wn column may_auto_order')

# The walkers [w0, w1) of a BatchCall: n = w1 - w0 and views, nothing launched (the ray paths and
# the layer intervals are formed by the radiative-transfer step, after the interpolation).  rad:
# the chunk's radius rows, or the shared row [1, L]; ckw: the continuum keywords of interp_ec_batch.
ChunkInputs = namedtuple('ChunkInputs',
                         'n temps dens rad ckw rv f_dilution deck_logp f_patchy tstar rplanet')


# refusals of eval_bands that the retrieval front end (retrieval.Retrieval) repeats at construction
MSG_RV_NEEDS_HIRES = ('eval_bands: rv (a radial-velocity shift) needs a HiresData, pass bands are '
                      'integrated on the unshifted grid')
MSG_STAR_HIRES = ('eval_bands: tstar / rplanet with a HiresData are not supported (its eclipse '
                  'factor is applied per sample before the convolution); they belong to a '
                  'PassBands with set_eclipse_grid()')
MSG_STAR_TRANSIT = ('eval_bands: tstar / rplanet (the eclipse factor per walker) belong to '
                    'emission and two-stream geometry, not to transit geometry')
MSG_STAR_NEEDS_GRID = ('eval_bands: tstar / rplanet need a stellar SED grid on the bands '
                       '(PassBands.set_eclipse_grid)')
MSG_GRID_NEEDS_TSTAR = ('eval_bands: the bands carry a stellar SED grid (set_eclipse_grid): '
                        'tstar[nw] is needed')
MSG_IRRADIATION_NEEDS_TSTAR = ('eval_bands: the model carries a stellar SED grid for its '
                               'irradiation (irradiation=): tstar[nw] is needed')
MSG_DECK_NEEDS_DECK = ('eval_bands: deck_logp needs a Deck among the models of the attached '
                       'Continuum')


def ordered_supported(rt_path, nlayers, itop, nwave):
    """Whether the depth-ordered kernels exist for a shape: the transit form is the matrix-core
    kernel only (pb_transit_spectrum_ordered: 2 ... 128 impact parameters, i.e.
    2 <= nlayers - itop <= 128); the emission form has no limit."""
    if rt_path != 'transit':
        return True
    return 2 <= nlayers - itop <= 128 and nwave >= 2


def plan_eval_bands(facts, call_facts):
    """The form of one eval_bands call from plain values -- no device, library or environment
    access.  facts (the model): rt_path ('transit', 'emission', 'two_stream'), nlayers, itop,
    nwave, order_set / tile_limit_set (a column order / its layer limits are set), one_pass (the
    one-pass transit is wanted and the library has it for the shape), continuum (one is
    attached).  call_facts: cloudy; contribution (default False: the band contribution functions
    are asked for -- grid order, every layer and the two passes whatever the model's column order
    is: the transit form needs the stored depth, the emission form reads the chunk's ec in grid
    order; a cloudy call takes the form 'clouds' in the same grid order: its contribution kernels
    walk the chunk's clear ec themselves).  (Two-stream with clouds is refused before planning.)"""
    rt_path = facts['rt_path']
    if call_facts.get('contribution', False):
        return BatchPlan('clouds' if call_facts['cloudy'] else rt_path, False, False,
                         table='etable', wn='wn', column=None, may_auto_order=False)
    # (the one-pass transit takes no continuum: with one attached, the two passes)
    one_pass = rt_path == 'transit' and facts['one_pass'] and not facts['continuum']
    form = 'clouds' if call_facts['cloudy'] else 'one_pass' if one_pass else rt_path
    # (an explicit order on a shape the ordered transit kernel does not take -- more than 128
    # impact parameters -- is worked in grid order: the spectra do not depend on the order;
    # two-stream geometry: always grid order -- no stop, nothing to order for)
    ordered = facts['order_set'] and form not in ('one_pass', 'two_stream') and \
        ordered_supported(rt_path, facts['nlayers'], facts['itop'], facts['nwave'])
    # (clouds: the clear column of a patchy walker may run below any limit taken from a
    # cloud-free base model)
    limited = ordered and facts['tile_limit_set'] and form != 'clouds'
    return BatchPlan(form, ordered, limited,
                     table='etable_ordered' if ordered else 'etable',
                     wn='wn_ordered' if ordered else 'wn',
                     column='column_order' if ordered else None,
                     may_auto_order=facts['nwave'] >= 64 and rt_path != 'two_stream' and
                     not one_pass)


def free_rplanet(atmosphere, params, bands, kw, who):
    """kw with rplanet = the 'rplanet' column of params[nw, npar] (cm) when the atmosphere has
    it free and the bands carry a stellar SED grid; the caller's own rplanet is then refused."""
    col = getattr(atmosphere, 'par_scalar', {}).get('rplanet', -1)
    if col < 0 or getattr(bands, 'star_grid', None) is None:
        return kw
    if kw.get('rplanet') is not None:
        raise ValueError(f"{who}: rplanet comes from the atmosphere's free 'rplanet', not from "
                         'the caller')
    return dict(kw, rplanet=params[:, col].contiguous())


class TableSpectrum:
    """Retrieval inner loop on sampled cross sections (Line_Sample path,
    pyratbay/opacity/line_sampling.py:394-463 -> _extcoeff.interp_ec): the table
    etable[nspec, ntemp, nlayers, nwave] stays resident; each eval() interpolates it to the
    layer temperatures, weights by the species densities, and runs optical depth + RT.

    column_order='auto' (default) has a ONE-TIME cost in the first eval_bands() call of a model
    with >= 64 columns: the first walker's temperatures are checked on the host (one stream
    synchronisation), its spectrum is computed to order the columns by optical depth
    (order_columns: interpolation + transit/plane-parallel depth + a sort) and a permuted SECOND
    COPY of the table is made (2 x the table's memory from then on; skipped when
    1.25 x table + 2 x the batch's ec buffer do not fit in free memory, when the ordered kernels
    do not support the shape -- transit geometry with more than 128 impact parameters -- or while
    the stream is being captured into a graph).  Every later call is launch-only.  To keep the first call
    free of both, call order_columns(temp, dens) yourself during set-up or pass
    column_order=None (grid order).  In a multi-rank run every rank orders by its own first
    walker: results do not depend on the order, memory use per rank is the same 2 x table."""

    def __init__(self, etable, ttable, wn, radius, rstar, rt_path='transit', itop=0,
                 maxdepth=10.0, quadrature_mu=None, quadrature_weights=None, continuum=None,
                 timestamps=True, column_order='auto', tint=0.0, flux_top=None,
                 irradiation=None, isotopes=None):
        require_gpu()
        # rt_path 'two_stream' / 'emission_two_stream' / 'eclipse_two_stream' (RT_PATHS, as in
        # LBLSpectrum): the geometry 'two_stream' (pyrat/spectrum.py:454-522) with the internal
        # flux of tint (K) added at the bottom and flux_top[W], the irradiation
        # beta_irr * (rstar / smaxis)**2 * starflux the caller forms (host or device; None: none),
        # at the top.  The optical depth has no maxdepth stop (opacity/optic_depth.py:124-126).
        # irradiation=(StellarGrid, factor), exclusive with flux_top: a retrieval with a free
        # stellar temperature (pyrat_obj.py:288-290 updates spec.starflux, which two_stream() puts
        # at the top, pyrat/spectrum.py:498-500): eval_bands(..., tstar=) takes every walker's top
        # boundary factor * grid(tstar[w]) from the grid (an observation.StellarGrid on wn);
        # factor = beta_irr * (rstar / smaxis)**2, formed by the caller like flux_top's.
        self.rt_path_name = rt_path
        self.observable = None
        if rt_path in ('two_stream', 'emission_two_stream', 'eclipse_two_stream'):
            rt_path, self.observable = RT_PATHS[rt_path]
            if itop != 0:
                # (layers above itop have dtau0 = 0 and the reference's own statement then gives
                # 0 * exp1(0) = NaN in every column)
                raise ValueError(f'rt_path {self.rt_path_name!r}: itop must be 0, got {itop}')
            maxdepth = float('inf')
            column_order = None               # (no early exit to order the columns for)
        elif tint != 0.0 or flux_top is not None or irradiation is not None:
            raise ValueError('tint, flux_top and irradiation belong to the two-stream geometries')
        if irradiation is not None and flux_top is not None:
            raise ValueError('irradiation (a stellar SED grid, one top boundary per walker) and '
                             'flux_top (one shared top boundary) are exclusive')
        self.irradiation = None
        self._timer = StageTimer() if timestamps else None
        # eval_bands: the order the columns are worked in (see order_columns).
        # 'auto': taken from the first walker of the first batch; None: grid order
        self.column_order = None
        self.etable_ordered = None
        # transit geometry, columns ordered by order_columns(): last row tile a block of 256
        # ordered columns can need (int32, device) -- see _eval_chunk; None: every layer
        self.tile_limit = None
        self.tile_margin = int(os.environ.get('PB_C5_MARGIN', '4'))
        if isinstance(column_order, str) and column_order == 'auto' and \
                os.environ.get('PB_COLUMN_ORDER', '1') == '0':
            column_order = None                       # (A/B switch: grid order)
        self._auto_order = isinstance(column_order, str) and column_order == 'auto'
        if isinstance(column_order, str) and not self._auto_order:
            raise ValueError("column_order: 'auto', None or a permutation of range(nwave)")
        if column_order is not None and not self._auto_order:
            self._pending_order = column_order
        else:
            self._pending_order = None
        self.continuum = continuum          # pyratbay_amd.continuum.Continuum or None
        self._alkali_checked = None         # the Continuum whose alkali models eval_bands has checked
        # the one-pass transit of eval_bands (_one_pass): True / False, None: PB_TABLE_TRANSIT
        self.one_pass = None
        self.etable = etable if isinstance(etable, torch.Tensor) else dev(etable)
        self.nspec, self.ntemp, self.nlayers, self.nwave = self.etable.shape
        # isotopes (an isotopes.IsotopeRatios: opacity_table.load_cross_sections(...,
        # isotope_ratios=) makes it; None: none): every table slot's density is multiplied by its
        # isotope ratio (line_sampling.py:451-456) before the table is interpolated -- eval() and
        # eval_bands take the walkers' log10 ratios as iso_pars, None: the block's defaults
        if isotopes is not None and isotopes.nspec != self.nspec:
            raise ValueError(f'isotopes: the model has {isotopes.nspec} slots, the table '
                             f'{self.nspec}')
        self.isotopes = isotopes
        self.ttable = dev(ttable)
        self.tmin, self.tmax = float(np.min(ttable)), float(np.max(ttable))
        self.wn = dev(wn)
        self.rt_path, self.itop, self.maxdepth = rt_path, itop, maxdepth
        self.rstar = float(rstar)
        self.set_radius(radius)
        if rt_path == 'two_stream':
            self.f_int = internal_flux(self.wn, tint)
            self.flux_top = None if flux_top is None else dev(flux_top)
            if self.flux_top is not None and self.flux_top.shape != (self.nwave,):
                raise ValueError(f'flux_top must have shape ({self.nwave},), got '
                                 f'{tuple(self.flux_top.shape)}')
            if irradiation is not None:
                grid, factor = irradiation
                if not isinstance(grid, StellarGrid) or grid.nwave != self.nwave:
                    raise ValueError('irradiation: (StellarGrid, factor) with the grid on the '
                                     f"model's {self.nwave} wavenumbers")
                self.irradiation = (grid, float(factor))
        elif rt_path != 'transit':
            if quadrature_mu is None:
                quadrature_mu, quadrature_weights = default_quadrature()
            elif quadrature_weights is None:
                raise ValueError('quadrature_mu needs quadrature_weights')
            self.mu = dev(quadrature_mu)
            self.weights = dev(quadrature_weights)
        self.ec = torch.zeros((self.nlayers, self.nwave), dtype=torch.float64, device='cuda')
        if self._pending_order is not None:
            self.set_column_order(self._pending_order)

    def set_column_order(self, order):
        """Work the columns of eval_bands' batches in the order `order` (a permutation of
        range(nwave); None: back to grid order).  A second copy of the table is kept with its
        wavenumber axis in that order, so that every stage still streams contiguous columns."""
        self.tile_limit = None
        if order is None:
            self.column_order = self.etable_ordered = None
            return
        order = torch.as_tensor(order, device='cuda').to(torch.int64).contiguous()
        if order.shape != (self.nwave,) or \
                not bool(torch.equal(torch.sort(order).values,
                                     torch.arange(self.nwave, device='cuda'))):
            raise ValueError('column order: not a permutation of range(nwave)')
        out = torch.empty_like(self.etable)
        for s in range(self.nspec):               # (species by species: a bounded temporary)
            torch.index_select(self.etable[s], -1, order, out=out[s])
        self.etable_ordered = out
        self.column_order = order.to(torch.int32)
        self.wn_ordered = self.wn[order].contiguous()

    def order_columns(self, temp, dens, radius=None):
        """Order the columns by the layer at which the model (temp[L], dens[L, nspec], radius[L])
        becomes optically thick (its ideep, _trapezoid.c:259-273).  The reference stops a column
        there; the matrix-core transit kernel can stop only when all 32 columns of a wavefront
        have -- which neighbours on the wavenumber grid never do together (a line core next to a
        window), and columns of similar depth do: at C5's shape 62 % of the products and 76 % of
        the layer reads remain.  Any model near the ones to come will do (walkers of a retrieval
        differ by per cent); the spectra do not depend on the order, only the time does."""
        temp = (temp if isinstance(temp, torch.Tensor) else dev(temp)).reshape(1, -1)
        dens = (dens if isinstance(dens, torch.Tensor) else dev(dens)).reshape(1, self.nlayers, -1)
        rad = self.radius if radius is None else \
            (radius if isinstance(radius, torch.Tensor) else dev(radius))
        rad = rad.reshape(1, -1).contiguous()
        ec = batch.interp_ec_batch(self.etable, self.ttable, temp.contiguous(), dens.contiguous())
        if self.rt_path == 'transit':
            _, _, ideep = batch.transit_spectrum_batch(
                ec, transit_path_device(rad, self.itop), rad, self.rstar, self.itop, self.nlayers,
                self.maxdepth, want_depth=True)
            ideep = ideep[0]
        else:
            # (emission: a wavefront of the fused kernel walks the layers until its last lane has
            # reached maxdepth -- lanes that stop together waste nothing)
            _, ideep = plane_parallel_optical_depth(
                ec[0], (rad[0, :-1] - rad[0, 1:]).contiguous(), self.itop, self.nlayers,
                self.maxdepth)
        order = torch.sort(ideep, stable=True).indices
        self.set_column_order(order)
        if self.tile_margin >= 0 and self._ordered_supported():
            # The layers nobody reads: walkers of a retrieval cross maxdepth within a layer or two
            # of the base model (measured at C5's shape: -1 ... +2 layers), so a block of 256
            # ordered columns needs the row tiles (transit) / layers (emission) up to the one
            # holding its deepest base crossing + tile_margin layers -- the interpolation writes
            # only those (80 % of ec at C5's shape), and a walker that does run past them is
            # flagged on the device and repaired (see _eval_chunk): the spectra never depend on
            # the limits.
            sorted_ideep = ideep[order].to(torch.int64)
            nblk = -(-self.nwave // 256)
            pad = nblk * 256 - self.nwave
            if pad:
                sorted_ideep = torch.cat([sorted_ideep, sorted_ideep[-1:].expand(pad)])
            bmax = sorted_ideep.view(nblk, 256).max(dim=1).values
            ntiles = -(-(self.nlayers - self.itop) // 16)
            tile = torch.clamp((bmax - self.itop + self.tile_margin) // 16, 0, ntiles - 1)
            # (worth its two gated repair launches only where it saves something: C5's emission
            # geometry crosses maxdepth near the bottom and keeps 97 % of the layers)
            written = torch.clamp(16 * (tile + 1), max=self.nlayers - self.itop).double().mean() / \
                (self.nlayers - self.itop)
            if float(written) <= 0.95 or self.tile_margin == 0:
                self.tile_limit = tile.to(torch.int32).contiguous()

    def set_radius(self, radius):
        self.radius = dev(radius)
        if self.rt_path == 'transit':
            self.raypath = dev(pack_raypath(transit_path(radius, self.itop), self.itop))
        else:
            self.intervals = dev(-np.diff(np.asarray(radius, float)))

    def eval(self, temp, dens, continuum_density=None, iso_pars=None):
        """temp[L] (K, inside the table's range -- the caller rejects the rest like
        line_sampling.py:426-427), dens[L, nspec] (molecules cm-3) -> spectrum[W].
        With a Continuum attached, continuum_density = {species: n[L]} feeds its terms
        (pyrat/opacity.py:206-257: every model adds to the same ec).  On a model with isotope
        ratios dens[L, nspec] holds the density of every slot's SPECIES and is multiplied by the
        slots' ratios (pb_iso_density): iso_pars[npars], a host vector of log10 ratios in
        isotopes.pnames order (None: the defaults); a negative or non-finite ratio is refused
        (ValueError), like a temperature outside the table."""
        iso = getattr(self, 'isotopes', None)
        if iso_pars is not None and iso is None:
            raise ValueError('eval: iso_pars on a model without isotope ratios')
        if iso is not None:
            if iso_pars is not None:
                iso_pars = np.asarray(iso_pars, float).reshape(1, -1)
            # (the block's defaults can be bad too: fillers that sum above 1)
            ratios = iso.iso_ratios if iso_pars is None else iso.ratios_host(iso_pars)[0]
            if not np.all(np.isfinite(ratios) & (ratios >= 0.0)):
                raise ValueError(f'eval: iso_pars give a negative or non-finite isotope ratio '
                                 f'({ratios}; the reference carries on with a negative opacity)')
        temp_host = None if isinstance(temp, torch.Tensor) else np.asarray(temp, float)
        if temp_host is not None and (np.any(temp_host < self.tmin) or
                                      np.any(temp_host > self.tmax)):
            raise ValueError(f'temperature outside the {self.tmin:.1f}-{self.tmax:.1f} '
                             'K range of the table (the reference rejects such a model, '
                             'line_sampling.py:426-427)')
        if getattr(self, 'irradiation', None) is not None:
            raise ValueError('eval: a model with irradiation= has one top boundary per walker: '
                             'use eval_bands(..., tstar=)')
        self.temp = temp if isinstance(temp, torch.Tensor) else dev(temp)
        dens = dens if isinstance(dens, torch.Tensor) else dev(dens)
        if iso is not None:
            _, dens, _, _ = iso.scale(self.temp.reshape(1, -1), dens.unsqueeze(0),
                                      None if iso_pars is None else dev(iso_pars))
            dens = dens[0]
        t = self._timer
        if t is not None:
            t.start('extinction')
        interp_ec(self.ec, self.etable, self.ttable, self.temp, dens, 0, self.nlayers,
                  assign=True)
        if self.continuum is not None:
            # the continuum's per-layer factors are prepared on the host: hand it host
            # temperatures when the caller has them (no device -> host copy in the loop)
            self.continuum.add(self.ec, temp_host if temp_host is not None
                               else self.temp.cpu().numpy(), continuum_density)
        if t is not None:
            t.mark('extinction', 'odepth')
        if self.rt_path == 'transit':
            self.spectrum, self.depth, self.ideep = transit_spectrum(
                self.ec, self.raypath, self.radius, self.rstar, self.itop, self.nlayers,
                self.maxdepth)
        else:
            self.depth, self.ideep = plane_parallel_optical_depth(
                self.ec, self.intervals, self.itop, self.nlayers, self.maxdepth)
            if t is not None:
                t.mark('odepth', 'spectrum')
            if self.rt_path == 'two_stream':
                self.flux_down, self.flux_up = two_stream(self.depth, self.wn, self.temp,
                                                          self.f_int, self.flux_top, 0)
                self.spectrum = self.flux_up[0]
            else:
                self.spectrum = emission_flux(self.depth, self.ideep, self.wn, self.temp,
                                              self.mu, self.weights, self.itop)
        if t is not None:
            t.mark('spectrum')
        return self.spectrum

    def band_contribution(self, bands, pressure=None):
        """The band contribution functions of the last eval() (Pyrat.band_contribution,
        pyrat_obj.py:671-696, without clouds) -> [L, nbands], every band divided by its maximum
        over the layers: transit geometry: the bands' transmittance per impact parameter;
        emission and two-stream geometry: the contribution function, with pressure[L] (any unit:
        only diff(log p) enters).  From the ec (and temperatures) eval() kept, through the kernels
        of eval_bands(contribution_out=...) with one walker: row 0 of such a batch, bit for bit."""
        if isinstance(bands, HiresData):
            raise ValueError('band_contribution: needs a PassBands')
        if getattr(self, 'spectrum', None) is None or getattr(self, 'depth', None) is None:
            raise ValueError('band_contribution: call eval() first')
        if self.rt_path == 'transit':
            # (eval()'s own depth comes from the one-spectrum kernel and host-made ray paths, which
            # round differently from the batch's: the depth is formed again from the ec eval()
            # kept, by the batch's pass, so that the result is row 0 of a batch, bit for bit)
            rad = self.radius.view(1, -1).contiguous()
            _, depth, ideep = batch.transit_spectrum_batch(
                self.ec.unsqueeze(0), transit_path_device(rad, self.itop), rad, self.rstar,
                self.itop, self.nlayers, self.maxdepth, want_depth=True)
            return batch.band_transmittance_batch(depth, ideep, bands, self.itop)[0]
        if pressure is None:
            raise ValueError(f'band_contribution: pressure[{self.nlayers}] is needed in emission '
                             'and two-stream geometry')
        return batch.band_contribution_emission_batch(
            self.ec.unsqueeze(0), self.intervals.view(1, -1), self.temp.reshape(1, -1), bands,
            pressure, self.itop, self.nlayers, self.maxdepth)[0]

    @property
    def timestamps(self):
        """Seconds of the last eval() by stage: 'extinction' (interpolation of the table +
        continuum terms), 'odepth', 'spectrum' -- the reference's keys (pyrat_obj.py:203-214)."""
        if self._timer is None:
            raise _capi.PbError('this model was built with timestamps=False')
        return self._timer.read()

    def eval_bands(self, temps, dens, bands, radius=None, chunk=64, streams=None,
                   f_dilution=None, continuum_density=None, continuum_pars=None, rv=None,
                   deck_logp=None, f_patchy=None, alkali_density=None, spectra_out=None,
                   contribution_out=None, contribution_pressure=None, tstar=None, rplanet=None,
                   iso_pars=None):
        """Batched-walker evaluation (the inner loop of a retrieval, pyrat_obj.py:225-385
        without the parameter mapping -- eval_params adds it): temps[nw, L], dens[nw, L, nspec] device tensors,
        optional per-walker radius[nw, L] (the hydrostatic profile changes with every model),
        bands: PassBands on this model's grid -> bandflux[nw, nbands].  Every stage is ONE
        launch per chunk of walkers -- interp_ec, transit_path, optical depth + transmission,
        band integration -- with no per-walker Python and no host synchronisation (except the
        one-time column ordering of the first call with column_order='auto': class docstring).  Walkers
        whose temperatures leave the table's range get +inf, like eval()'s reject path
        (pyrat_obj.py:302-320, 378-380).  Emission geometry: f_dilution[nw] = the walkers'
        dilution factors (pyrat_obj.py:296-297), and bands.set_eclipse(...) for the planet-to-star
        flux ratios of an eclipse retrieval (pyrat_obj.py:662-665).

        Two-stream geometry (rt_path 'two_stream' / 'emission_two_stream' / 'eclipse_two_stream',
        pyrat/spectrum.py:454-522): interpolation, then ONE launch for the optical depth without a
        stop and both sweeps (two_stream_batch), then the bands; f_dilution, set_eclipse, a
        HiresData with rv, radius[nw, L] and the Continuum's terms and alkali doublets work as in
        emission geometry.  Always grid order (there is no stop to order the columns for:
        column_order orders nothing and copies no table); deck_logp, f_patchy and a Continuum with
        cloud-type models are refused (ValueError: the reference's two-stream ignores the clear
        column and its deck leaves zero rows below it) -- eval() takes them.

        With a Continuum attached (TableSpectrum(..., continuum=cont)) its terms are added in the
        store of the interpolation (pb_interp_ec_batch_cont): continuum_density[nw, L, ncs] holds
        the number densities of cont.species, continuum_pars[nw, npars] the free parameters in
        cont.free_pars order (None: every walker uses the models' current pars).  A walker outside
        a CIA table's temperatures is rejected like one outside the table.  Alkali doublets
        (SodiumVdW, PotassiumVdW) take alkali_density[nw, L, len(cont.alkali)], the number
        densities of cont.alkali_species in model order (a float64 device tensor): their terms are
        added in the same store, the Voigt values at the detuning distance formed per walker and
        layer on the device.  At most 2 alkali models with 4 lines in all; a model whose detuning
        distance is less than 20 Gaussian widths at the table's lowest temperature (no shipped
        model: 570 and more) is outside the regime of the device's Faddeeva function.  Both are
        refused (ValueError), as are alkali models without alkali_density and a Deck without
        deck_logp; eval() takes them.

        Clouds (pb_clouds.hip; both arguments are device tensors of shape [nw]):
        deck_logp = log10 of each walker's cloud-deck pressure in bar (needs a Deck in the
        Continuum; the pressure grid is cont.pressure): the deck's layer, radius and temperature
        are found on the device (deck_state_batch: clamped at the ends of the grid) and the
        column ends there.  f_patchy = each walker's cloudy fraction: the spectrum is
        f cloudy + (1 - f) clear, combined per sample BEFORE the band integration / the
        instrument profile, where the cloudy column is ec + the terms of the Continuum's
        cloud_models down to the deck (if any) and the clear column has neither.  f_patchy is
        CLAMPED to [0, 1] on the device (no host check; NaN gives NaN).  Without f_patchy a deck
        alone gives the cloudy column; cloud_models without f_patchy likewise.  Both columns come
        from one kernel on the clear ec (no second ec buffer); it runs in the column order in use
        but without its layer limits (tile_limit), whatever column_order is: the spectra do not
        depend on it bit for bit.

        bands may be a HiresData instead (high-resolution spectroscopy, pyrat_obj.py:331-356):
        the spectra are convolved with the instrument profile, shifted by the walkers' radial
        velocities rv[nw] (km/s, a device tensor; None: no shift) and sampled at the data in one
        launch per chunk -> [nw, ndata].  rv with a PassBands is refused (ValueError).

        spectra_out (a contiguous float64 device tensor [nw, nwave]; None: nothing changes)
        receives every walker's full-resolution spectrum in GRID order, whatever column order is
        in use: the spectrum a one-walker eval() of this model returns (transit: the modulation
        spectrum; emission and two-stream: the planet's flux, before f_dilution, the eclipse ratio
        and the instrument profile, which belong to the bands) -- one copy per chunk on every
        branch: one-pass, ordered and limited transit, emission, two-stream and clouds.  The rows
        of rejected walkers hold whatever the kernels made of their inputs.

        contribution_out (a contiguous float64 device tensor [nw, L, nbands]; None: nothing
        changes) receives every walker's band contribution functions (Pyrat.band_contribution,
        pyrat_obj.py:671-696; contribution.band_contribution_host is the NumPy statement): transit
        geometry: the bands' transmittance per impact parameter, from the depth a second transit
        pass stores (transit_spectrum_batch(..., want_depth=True) + band_transmittance_batch);
        emission and two-stream geometry: the contribution function B d(exp(-tau)) / d(ln p) from
        the chunk's ec (band_contribution_emission_batch, before two_stream_batch consumes ec),
        which needs contribution_pressure[L] (any unit: only diff(log p) enters; a host array, or a
        tensor that is read back once per call).  Every band is divided by its maximum over the
        layers; a band of one sample is NaN.  Such a call runs in grid order, over every layer and
        in two passes, whatever column_order is; the band fluxes and spectra_out keep their bits.
        With clouds (deck_logp, or a Continuum with cloud-type models; with or without f_patchy)
        one more pass over the chunk's clear ec takes the deck state and the cloud factors the
        flux kernel is given (no depth and no second ec is stored for either column): transit
        geometry: f transmittance(cloudy) + (1 - f) transmittance(clear) per sample before the
        band integral, the cloudy column ending at the deck's layer (the deck's radius does not
        enter), or the cloudy column alone without f_patchy (band_transmittance_cloudy_batch);
        emission geometry: the contribution function of the cloudy column only, as the reference
        -- the clear column is not mixed in and f_patchy does not enter -- with the depth through
        the row past the deck and the deck's temperature in its layer's row of B
        (band_contribution_emission_cloudy_batch); contribution.band_contribution_cloudy_host is
        the NumPy statement.  The band fluxes and spectra_out of such a call have the bits of the
        same call without contribution_out.
        Refused (ValueError) before any launch: a HiresData as bands; f_patchy ALONE (no
        deck_logp and no cloud-type model: there is nothing cloudy to mix, the clear call gives
        the result); clouds in two-stream geometry.  Rows of rejected walkers hold whatever the
        kernels made of their inputs.

        tstar[nw] (K) and rplanet[nw] (cm), float64 device tensors: an eclipse retrieval with a
        free stellar temperature (pyrat_obj.py:288-294) on bands that carry a stellar SED grid
        (PassBands.set_eclipse_grid): each walker's eclipse factor rprs**2 / bandflux_star comes
        from the grid interpolated at ITS temperature and integrated over the bands on the device
        (pb_star_band_scale_batch in place of pb_band_scale: still two launches for the bands),
        with rprs = rplanet[w] / rstar when rplanet is given (a free rplanet enters the factor,
        pyrat_obj.py:662-665), else the planet radius of set_eclipse_grid.  A walker whose tstar
        is NaN or outside the grid's temperatures is rejected (+inf; DEVIATION: the reference's
        interp1d raises).  Refused (ValueError) before any launch: tstar on bands without a grid;
        bands with a grid and no tstar; rplanet without tstar; either in transit geometry; either
        with a HiresData (its eclipse factor is applied per sample before the convolution).

        Two-stream geometry and the star's temperature: on a model built with
        irradiation=(StellarGrid, factor) tstar also sets every walker's top boundary,
        factor * grid(tstar[w]), inside the sweep (two_stream_batch_star: one launch, as before);
        bands without a grid are then allowed (tstar moves the irradiation only), and such a model
        without tstar is refused.  On a model built with a shared flux_top the irradiation is
        FROZEN at the temperature flux_top was formed with, whatever tstar is: tstar then moves
        the eclipse factor only.

        Isotope ratios (a model built with isotopes=, an isotopes.IsotopeRatios; Line_Sample's
        isotope_ratios, line_sampling.py:282-298, 451-456): dens[nw, L, nspec] holds the density
        of every slot's SPECIES (a 12CO and a 13CO slot both CO's) and ONE launch per call
        (pb_iso_density, before the chunks) multiplies it by the walkers' ratios: iso_pars[nw,
        npars], a float64 device tensor of log10 ratios in isotopes.pnames order, None: the
        block's defaults.  Every form above then runs on the scaled densities with no change.
        DEVIATION: a walker with a negative or non-finite ratio (a fill slot whose fillers sum
        above 1, a NaN parameter) is rejected, +inf like one outside the table's temperatures;
        the reference carries on with a negative opacity.  iso_pars on a model without isotopes,
        or of another shape, is refused (ValueError) before any launch."""
        call_ = self._batch_call(temps, dens, bands, radius, f_dilution, continuum_density,
                                 continuum_pars, rv, deck_logp, f_patchy, alkali_density,
                                 spectra_out, contribution_out, contribution_pressure, tstar,
                                 rplanet, iso_pars)
        nw = call_.nw
        one_pass = self.rt_path == 'transit' and self._one_pass()
        call_facts = {'cloudy': call_.cloudy}
        if call_.contribution_out is not None:
            call_facts['contribution'] = True
        plan = plan_eval_bands(self._plan_facts(one_pass), call_facts)
        if plan.may_auto_order and self._auto_order and self.column_order is None and nw > 0:
            self._try_auto_order(call_, chunk)
            # (the ordering changes column_order and tile_limit: the plan the chunks run is made
            # after it)
            plan = plan_eval_bands(self._plan_facts(one_pass), call_facts)
        if call_.shared_radius and self.rt_path == 'transit':
            call_ = call_._replace(
                path1=transit_path_device(call_.radius[0], self.itop).view(1, -1))
        # Consecutive chunks are independent: with `streams` > 1 (PB_EVAL_STREAMS) chunk i runs on
        # side stream i % streams.  Measured at C5's shape and NOT the default: the interpolation
        # of one chunk beside the optical-depth pass of the previous one gains nothing (two chunks
        # of 32 on two streams 2.97 ms, one chunk of 64 2.73 ms per 64 walkers): both stages
        # stream every walker's ec through HBM.
        nchunks = -(-nw // chunk)
        if streams is None:
            streams = int(os.environ.get('PB_EVAL_STREAMS', '1'))
        streams = max(1, min(streams, nchunks))
        caller = torch.cuda.current_stream()
        eval_streams = side_streams(streams) if streams > 1 else []
        for st in eval_streams:
            st.wait_stream(caller)
        for ci, w0 in enumerate(range(0, nw, chunk)):
            with torch.cuda.stream(eval_streams[ci % streams]) if eval_streams else \
                    contextlib.nullcontext():
                self._eval_chunk(plan, call_, w0, min(w0 + chunk, nw))
        for st in eval_streams:
            caller.wait_stream(st)
        # (with CIA tables: the intersection of their temperature ranges and the table's; with
        # isotope ratios: the scaled call's temperatures, zeros for a walker they reject)
        call('pb_reject_walkers', _ptr(call_.out), _ptr(call_.temps.contiguous()), call_.tmin,
             call_.tmax, self.nlayers, bands.nbands, nw, _stream())
        return call_.out

    def _batch_call(self, temps, dens, bands, radius, f_dilution, continuum_density,
                    continuum_pars, rv, deck_logp, f_patchy, alkali_density, spectra_out,
                    contribution_out=None, contribution_pressure=None, tstar=None, rplanet=None,
                    iso_pars=None):
        """The arguments of eval_bands, checked and filled -> BatchCall (allocates `out`; on a
        model with isotope ratios its one launch scales temps and dens, after every check)."""
        assert self.rt_path in ('transit', 'emission', 'two_stream'), \
            'eval_bands: transit, emission or two-stream geometry on sampled cross sections'
        two_stream_rt = self.rt_path == 'two_stream'
        if rv is not None:
            if not isinstance(bands, HiresData):
                raise ValueError(MSG_RV_NEEDS_HIRES)
            if tuple(rv.shape) != (temps.shape[0],):
                raise ValueError(f'eval_bands: rv must have shape {(temps.shape[0],)}, got '
                                 f'{tuple(rv.shape)}')
        assert f_dilution is None or self.rt_path in ('emission', 'two_stream'), \
            'f_dilution: emission geometry'
        assert f_dilution is None or f_dilution.shape == (temps.shape[0],)
        nw = temps.shape[0]
        iso = getattr(self, 'isotopes', None)
        if iso is None and iso_pars is not None:
            raise ValueError('eval_bands: iso_pars on a model without isotope ratios '
                             '(TableSpectrum(..., isotopes=))')
        if iso is not None:
            iso.check_pars('eval_bands: iso_pars', iso_pars, nw)
            if not isinstance(dens, torch.Tensor) or \
                    tuple(dens.shape) != (nw, self.nlayers, self.nspec):
                raise ValueError(f'eval_bands: dens must have shape '
                                 f'{(nw, self.nlayers, self.nspec)} (slots {list(iso.species)}), '
                                 f'got {tuple(getattr(dens, "shape", ()))}')
        grid = getattr(bands, 'star_grid', None)
        irradiation = getattr(self, 'irradiation', None)
        if tstar is not None or rplanet is not None:
            if isinstance(bands, HiresData):
                raise ValueError(MSG_STAR_HIRES)
            if self.rt_path == 'transit':
                raise ValueError(MSG_STAR_TRANSIT)
            # (tstar alone on bands without a grid: the irradiation of a model that carries one)
            if grid is None and (irradiation is None or rplanet is not None):
                raise ValueError(MSG_STAR_NEEDS_GRID)
            if tstar is None:
                raise ValueError('eval_bands: rplanet needs tstar (the bands carry a stellar SED '
                                 'grid: every walker needs its stellar temperature)')
            if grid is not None and rplanet is None and bands.grid_rplanet is None:
                raise ValueError('eval_bands: a planet radius is needed, rplanet[nw] or the one '
                                 'of set_eclipse_grid()')
            _check_walker_tensor('eval_bands: tstar', tstar, nw)
            _check_walker_tensor('eval_bands: rplanet', rplanet, nw)
        elif grid is not None:
            raise ValueError(MSG_GRID_NEEDS_TSTAR)
        if irradiation is not None and tstar is None:
            raise ValueError(MSG_IRRADIATION_NEEDS_TSTAR)
        if spectra_out is not None:
            _check_walker_tensor('eval_bands: spectra_out', spectra_out, nw,
                                 shape=(nw, self.nwave))
            if not spectra_out.is_contiguous():
                raise ValueError('eval_bands: spectra_out must be contiguous')
        tmin, tmax = self.tmin, self.tmax
        cont = self.continuum
        _check_walker_tensor('eval_bands: deck_logp', deck_logp, nw)
        _check_walker_tensor('eval_bands: f_patchy', f_patchy, nw)
        if deck_logp is not None and (cont is None or not cont.deck):
            raise ValueError(MSG_DECK_NEEDS_DECK)
        if two_stream_rt:
            # (the reference's two-stream ignores the clear column of a patchy model, and its deck
            # leaves zero rows below the deck's layer)
            for name, given in (('deck_logp', deck_logp is not None),
                                ('f_patchy', f_patchy is not None),
                                ('a Continuum with cloud-type models',
                                 cont is not None and bool(cont.cloud))):
                if given:
                    raise ValueError(f'eval_bands: {name}: clouds are not supported in batched '
                                     'form in two-stream geometry; use eval()')
        # (cloud-type models alone take the cloud path too: the cloudy column is the spectrum)
        cloudy = deck_logp is not None or f_patchy is not None or \
            (cont is not None and bool(cont.cloud))
        if cloudy and radius is not None and (radius.dim() != 2 or
                                              radius.shape[1] != self.nlayers or
                                              radius.shape[0] not in (1, nw)):
            raise ValueError(f'eval_bands: radius must have shape ({nw} or 1, {self.nlayers}), '
                             f'got {tuple(radius.shape)}')
        if cont is not None:
            if alkali_density is not None:
                if not cont.alkali:
                    raise ValueError('eval_bands: alkali_density needs an alkali model '
                                     '(SodiumVdW, PotassiumVdW) among the models of the '
                                     'attached Continuum')
                if cont.batch_unsupported(deck=True, alkali=True):
                    raise ValueError(
                        f'eval_bands: {len(cont.alkali)} alkali models with '
                        f'{sum(m.nlines for m in cont.alkali)} lines: the batched form takes at '
                        'most 2 models with 4 lines in all; use eval()')
                _check_walker_tensor(f'eval_bands: alkali_density (species '
                                     f'{cont.alkali_species})', alkali_density, nw,
                                     shape=(nw, self.nlayers, len(cont.alkali)))
                if self._alkali_checked is not cont:
                    cont.check_alkali_batch(self.tmin)       # (once per model: host arithmetic)
                    self._alkali_checked = cont
            bad = cont.batch_unsupported(deck=deck_logp is not None,
                                         alkali=alkali_density is not None)
            if bad:
                raise ValueError(f'eval_bands: continuum models {bad} are not supported in '
                                 'batched form (cloud deck, alkali); use eval()')
            shape = (nw, self.nlayers, len(cont.species))
            got = None if continuum_density is None else tuple(continuum_density.shape)
            if got != shape:
                raise ValueError(f'eval_bands: continuum_density must be a device tensor of shape '
                                 f'{shape} (species {cont.species}), got {got}')
            npars = len(cont.free_pars)
            if continuum_pars is not None and tuple(continuum_pars.shape) != (nw, npars):
                raise ValueError(f'eval_bands: continuum_pars must have shape {(nw, npars)} '
                                 f'({cont.free_pars}), got {tuple(continuum_pars.shape)}')
            for m in cont.cia:
                tmin, tmax = max(tmin, float(m.tmin)), min(tmax, float(m.tmax))
        elif continuum_density is not None or continuum_pars is not None:
            raise ValueError('eval_bands: continuum arguments without a Continuum')
        elif alkali_density is not None:
            raise ValueError('eval_bands: alkali_density without a Continuum that has an alkali '
                             'model')
        dlogp = None
        if contribution_out is not None:
            if isinstance(bands, HiresData):
                raise ValueError('eval_bands: contribution_out needs a PassBands (band '
                                 'contribution functions of high-resolution data are not '
                                 'supported)')
            if cloudy and deck_logp is None and not (cont is not None and bool(cont.cloud)):
                # (f_patchy alone: nothing cloudy to mix -- the two columns are the same numbers,
                # and the clear call gives them in half the work)
                raise ValueError('eval_bands: contribution_out with clouds (deck_logp, f_patchy, '
                                 'cloud-type models) is not supported: the reference mixes a '
                                 'clear and a cloudy transmittance there')
            _check_walker_tensor('eval_bands: contribution_out', contribution_out, nw,
                                 shape=(nw, self.nlayers, bands.nbands))
            if not contribution_out.is_contiguous():
                raise ValueError('eval_bands: contribution_out must be contiguous')
            if self.rt_path != 'transit':
                if contribution_pressure is None:
                    raise ValueError('eval_bands: contribution_out needs contribution_pressure'
                                     f'[{self.nlayers}] in emission and two-stream geometry')
                if tuple(np.shape(contribution_pressure)) != (self.nlayers,):
                    raise ValueError(f'eval_bands: contribution_pressure must have shape '
                                     f'({self.nlayers},), got '
                                     f'{tuple(np.shape(contribution_pressure))}')
                dlogp = batch.contribution_dlogp(contribution_pressure, self.nlayers)
        elif contribution_pressure is not None:
            raise ValueError('eval_bands: contribution_pressure without contribution_out')
        if iso is not None:
            temps, dens, _, _ = iso.scale(temps, dens, iso_pars)
        out = torch.empty((nw, bands.nbands), dtype=torch.float64, device='cuda')
        if radius is None:
            radius = self.radius.view(1, -1)
        return BatchCall(temps, dens, bands, radius, radius.shape[0] == 1, f_dilution,
                         continuum_density, continuum_pars, alkali_density, rv, deck_logp,
                         f_patchy, spectra_out, out, nw, cloudy, tmin, tmax,
                         contribution_out=contribution_out, dlogp=dlogp, tstar=tstar,
                         rplanet=rplanet)

    def _plan_facts(self, one_pass):
        """The model's side of plan_eval_bands' inputs; one_pass: wanted and supported."""
        return dict(rt_path=self.rt_path, nlayers=self.nlayers, itop=self.itop, nwave=self.nwave,
                    order_set=self.column_order is not None,
                    tile_limit_set=self.tile_limit is not None, one_pass=one_pass,
                    continuum=self.continuum is not None)

    def _try_auto_order(self, call_, chunk):
        """ONE-TIME set-up of the first batch (class docstring): a host read-back, a sort and a
        permuted second copy of the table.  Skipped -- grid order, nothing else changes --
        where the ordered kernels do not exist for the shape, while the stream is being
        captured into a graph, and when the second copy + this batch's ec would not fit."""
        t0 = call_.temps[0]
        table_bytes = self.etable.numel() * 8
        ec_bytes = 8 * min(chunk, call_.nw) * self.nlayers * self.nwave
        if not self._ordered_supported() or torch.cuda.is_current_stream_capturing():
            self._auto_order = self._auto_order and self._ordered_supported()
        elif torch.cuda.mem_get_info()[0] < 1.25 * table_bytes + 2 * ec_bytes:
            self._auto_order = False      # no room for the second copy of the table: grid order
        # (a walker outside the table's range would order by garbage: wait for a valid one)
        elif bool(((t0 >= self.tmin) & (t0 <= self.tmax)).all()):
            self.order_columns(t0, call_.dens[0], call_.radius[0])

    def eval_params(self, atmosphere, params, bands, **kw):
        """The batched loop from the walkers' parameter vectors (pyrat_obj.py:225-385 WITH the
        parameter mapping of :258-275 and Atmosphere.calc_profiles): atmosphere, a bound
        pyratbay_amd.atmosphere.WalkerAtmosphere, turns params[nw, npar] into temps, dens, radius
        and the continuum / alkali densities in one launch (WalkerAtmosphere.evaluate), and those
        tensors go to eval_bands unchanged; kw: everything else eval_bands takes (continuum_pars,
        rv, deck_logp, f_patchy, f_dilution, chunk, streams, spectra_out, contribution_out,
        contribution_pressure, tstar, iso_pars).  Walkers the atmosphere rejects
        (non-positive temperature, trace abundances above qcap, ...: WalkerAtmosphere) come out
        as +inf like those outside the table's temperatures.  When the atmosphere has 'rplanet'
        free and the bands carry a stellar SED grid (PassBands.set_eclipse_grid), that column of
        params is the rplanet[nw] of eval_bands' eclipse factor (Pyrat.band_integrate reads the
        current atm.rplanet, pyrat_obj.py:662-665); passing rplanet as well is refused."""
        for name in ('temps', 'dens', 'radius', 'continuum_density', 'alkali_density'):
            if name in kw:
                raise ValueError(f'eval_params: {name} comes from the atmosphere, not from the '
                                 'caller')
        kw = free_rplanet(atmosphere, params, bands, kw, 'eval_params')
        prof = atmosphere.evaluate(params)
        if prof.continuum_density is not None:
            kw['continuum_density'] = prof.continuum_density
        if prof.alkali_density is not None:
            kw['alkali_density'] = prof.alkali_density
        return self.eval_bands(prof.temps, prof.dens, bands, radius=prof.radius, **kw)

    def eval_loglike(self, atmosphere, params, bands, observation, offsets=None, err_pars=None,
                     **kw):
        """The batched loop from the walkers' parameter vectors to their log-likelihoods
        (Loglike.__call__, tools/retrieval_tools.py:74-104, around eval()): eval_params, then
        observation.loglike (an observation.Observation on these bands' data) with the walkers'
        instrumental offsets offsets[nw, noff] and uncertainty-scaling parameters
        err_pars[nw, nerr] (pyrat_obj.py:362-372; None: the defaults) -> loglike[nw].  kw:
        everything eval_params takes, tstar included.  Rejected walkers (+inf band fluxes) come
        out as -1e98.  Launches only: one pb_loglike_obs after those of eval_params, no
        read-back.  The likelihood uses the data and uncertainties eval() leaves in obs (see
        Observation on what the reference's Loglike binds)."""
        if observation.nbands != bands.nbands:
            raise ValueError(f'eval_loglike: the observation has {observation.nbands} data '
                             f'points, the bands give {bands.nbands}')
        return observation.loglike(self.eval_params(atmosphere, params, bands, **kw),
                                   offsets=offsets, err_pars=err_pars)

    def posterior_summary(self, atmosphere, params, counts, bands, quantiles=None, chunk=64,
                          **kw):
        """The summary of a posterior (posterior_post_processing, tools/retrieval_tools.py:384-503):
        params[n, npar] = the chain's UNIQUE samples (device; posterior.unique_samples gives their
        rows and counts[n], how often the chain visited each) go through the eval_params path in
        chunks of `chunk`; each chunk's full-resolution spectra, band fluxes, temperatures and mole
        fractions are written transposed into sample-minor stores ([nwave, n], [nbands, n],
        [L, n], [L, nspec, n]) and one pb_weighted_quantiles call per store gives the quantiles
        (default posterior.QUANTILES: the median and the 1- and 2-sigma bounds, the reference's
        order) of the chain -- each sample counts[i] times, np.percentile's bits, the expansion
        never formed.  -> posterior.PosteriorSummary of device tensors: spectrum[nq, nwave],
        bands[nq, nbands], temperature[nq, L], vmr[nq, L, nspec] (nspec: the table's species, the
        atmosphere's dens output times k T / p -- on a model with isotope ratios the unscaled
        one, as the reference stores atm.vmr: a 12CO and a 13CO slot both show CO's), n_rejected,
        quantiles, stores (None unless keep_stores=True: the four stores and the counts used).

        DEVIATION: samples the batch rejects (+inf band fluxes: outside the table's temperatures,
        a radial velocity beyond rv_max; or a reject flag of the atmosphere) get count 0 before the
        reduction and are reported in n_rejected -- the reference would return NaN / inf
        quantiles.  Every sample rejected: ValueError.  One read-back (n_rejected and the length
        of the expansion), otherwise launches only.  The spectrum store takes 8 nwave n bytes: a
        store that does not fit in free device memory is refused (ValueError) before anything is
        allocated.  kw: what eval_bands takes per walker (continuum_pars, rv, deck_logp, f_patchy,
        f_dilution, tstar, rplanet, iso_pars) with one row per sample, and streams; a free
        'rplanet' of the atmosphere enters the eclipse factor of bands with a stellar SED grid as in eval_params.

        contribution=True adds the reference's fifth product, the median over the chain of the
        band contribution functions (eval_bands' contribution_out, with atmosphere.pressure; pass
        bands only; with deck_logp / f_patchy / cloud-type models the cloudy forms described
        there -- in emission geometry the cloudy column only, as the reference): a fifth store
        [L, nbands, n], counted in the memory check, and
        its 0.5 quantile -> PosteriorSummary.contribution[L, nbands] (None when not asked for)."""
        return posterior.posterior_summary(
            self, atmosphere, params, counts, bands,
            quantiles=posterior.QUANTILES if quantiles is None else quantiles, chunk=chunk, **kw)

    def radiative_equilibrium(self, pressure, vmr, mol_mass, **kw):
        """The radiative-equilibrium iteration (runmode = radeq, pyrat_obj.py:559-646) of a batch
        of profiles on this model's table, grid and Continuum, at fixed volume mixing ratios or
        (vmr=None, chemistry=ChemNetwork) with the equilibrium chemistry of every iteration: a
        pyratbay_amd.radeq.RadiativeEquilibrium (its docstring has the keywords); .run(temp0,
        nsamples) iterates on the device.  Two-stream geometry only; a model with isotope ratios
        is refused (ValueError)."""
        if getattr(self, 'isotopes', None) is not None:
            raise ValueError('radiative_equilibrium: a model with isotope ratios (isotopes=) is '
                             'not supported: the iteration forms its densities from vmr and '
                             'would not scale them')
        return RadiativeEquilibrium(self, pressure, vmr, mol_mass, **kw)

    def _ordered_supported(self):
        """Whether the depth-ordered kernels exist for this model's shape (ordered_supported)."""
        return ordered_supported(self.rt_path, self.nlayers, self.itop, self.nwave)

    def _one_pass(self):
        """The transit batch through pb_table_transit_batch (interpolation, optical depth and
        transmission in one pass, ec never stored): opt-in (`one_pass = True` or
        PB_TABLE_TRANSIT=1).  It saves the ec[walkers, L, W] buffer (4.1 GB per 64 walkers at
        C5's shape); at that shape it runs 2.54 ms per 64 walkers when the walkers resemble one
        another (two walkers per wavefront share their table loads; the two passes: 2.42-2.70 box
        to box), 2.86 when they do not -- which only the device knows, hence not the default."""
        want = self.one_pass
        if want is None:
            want = os.environ.get('PB_TABLE_TRANSIT', '0') == '1'
        return bool(want) and batch.table_transit_supported(
            self.nspec, self.ntemp, self.nlayers, self.itop, self.nlayers, self.nwave)

    def _eval_chunk(self, plan, call_, w0, w1):
        """One chunk of eval_bands: walkers [w0, w1) through every stage, one launch each --
        interpolation, the radiative transfer of the plan's form, the bands."""
        table, wn = getattr(self, plan.table), getattr(self, plan.wn)
        column = getattr(self, plan.column) if plan.column else None
        ci = self._chunk_inputs(plan, call_, column, w0, w1)
        keep = None
        if plan.form == 'one_pass':
            # interpolation + optical depth + transmission in one pass: ec is never stored
            rad, path = self._transit_geometry(call_, ci)
            spectra = batch.table_transit_batch(table, self.ttable, ci.temps, ci.dens, path, rad,
                                                self.rstar, self.itop, self.nlayers,
                                                self.maxdepth)
        else:
            ec, work = self._interpolate(plan, ci, table)
            if plan.form == 'clouds':
                spectra, keep = self._rt_clouds(call_, ci, ec, wn, column,
                                                None if call_.contribution_out is None else
                                                call_.contribution_out[w0:w1])
            elif call_.contribution_out is not None:
                spectra = self._rt_contribution(plan, call_, ci, ec, wn,
                                                call_.contribution_out[w0:w1])
            elif plan.form == 'transit':
                spectra = self._rt_transit(plan, call_, ci, ec, table, column, work)
            else:
                spectra = self._rt_emission(plan, ci, ec, table, wn, column, work)
        if call_.spectra_out is not None:
            call_.spectra_out[w0:w1].copy_(spectra)
        # (the walkers' radial velocities: HiresData only -- eval_bands has checked)
        okw = {} if ci.rv is None else {'rv': ci.rv}
        if ci.tstar is not None and getattr(call_.bands, 'star_grid', None) is not None:
            okw = {'tstar': ci.tstar, 'rplanet': ci.rplanet}
        call_.bands.integrate_batch(
            spectra, call_.out[w0:w1],
            None if ci.f_dilution is None else ci.f_dilution.contiguous(), **okw)
        del keep

    def _chunk_inputs(self, plan, call_, column, w0, w1):
        """The walkers [w0, w1) of the call -> ChunkInputs (views only)."""
        def rows(t):
            return None if t is None else t[w0:w1]
        temps = call_.temps[w0:w1]
        if plan.form == 'clouds':
            temps = temps.contiguous()
        # the continuum's operands in the table's column order, this chunk's walkers
        ckw = {}
        if self.continuum is not None:
            ckw = dict(continuum=self.continuum.batch_operands(column),
                       continuum_density=call_.continuum_density[w0:w1],
                       continuum_pars=rows(call_.continuum_pars),
                       alkali_density=rows(call_.alkali_density))
        return ChunkInputs(w1 - w0, temps, call_.dens[w0:w1],
                           call_.radius if call_.shared_radius else call_.radius[w0:w1], ckw,
                           rows(call_.rv), rows(call_.f_dilution), rows(call_.deck_logp),
                           rows(call_.f_patchy), rows(call_.tstar), rows(call_.rplanet))

    def _interpolate(self, plan, ci, table):
        """ec[n, L, W] of the chunk -> (ec, work).  Limited: only the layers a block of columns
        can need are written (ec keeps whatever an earlier batch left in the others: they are
        read by no one, or the walker is flagged and repaired); work = (flags, iwork, twork), the
        walkers' flags and the scratch the gated repair reuses."""
        if not plan.limited:
            return batch.interp_ec_batch(table, self.ttable, ci.temps, ci.dens, **ci.ckw), None
        n = ci.n
        flags = torch.zeros(n + 1, dtype=torch.int32, device=table.device)
        iwork = torch.empty(_capi.lib().pb_interp_ec_batch_work_doubles(self.nlayers, n)
                            if not ci.ckw else
                            ci.ckw['continuum'].work_doubles(self.nlayers, self.nwave, n),
                            dtype=torch.float64, device=table.device)
        twork = None
        if self.rt_path == 'transit':
            twork = torch.empty(_capi.lib().pb_transit_work_doubles(
                self.nlayers, int(self.itop), int(self.nlayers), self.nwave, n),
                dtype=torch.float64, device=table.device)
        ec = batch.interp_ec_batch(table, self.ttable, ci.temps, ci.dens,
                                   tile_limit=self.tile_limit, row0=self.itop, work=iwork,
                                   **ci.ckw)
        return ec, (flags, iwork, twork)

    def _limited_rt(self, rt, args, ci, table, ws, **rt_work):
        """The limited form of a radiative-transfer wrapper `rt(*args)` (args[0] is ec): first
        pass under the layer limits, then the repair, gated on the device -- the full
        interpolation if ANY walker ran past its limit, then `rt` again for the flagged walkers:
        two launches of workgroups that return at once otherwise, no host round trip."""
        flags, iwork, _ = ws
        spectra = rt(*args, tile_limit=self.tile_limit, flags=flags, **rt_work)
        batch.interp_ec_batch(table, self.ttable, ci.temps, ci.dens, out=args[0],
                              gate=flags[ci.n:ci.n + 1], work=iwork, **ci.ckw)
        rt(*args, gate=flags, out=spectra, **rt_work)
        return spectra

    def _transit_geometry(self, call_, ci):
        """(radius[n, L], raypath[n, npath]) of the chunk, contiguous."""
        if call_.shared_radius:
            return (call_.radius.expand(ci.n, -1).contiguous(),
                    call_.path1.expand(ci.n, -1).contiguous())
        rad = ci.rad.contiguous()
        return rad, transit_path_device(rad, self.itop)

    def _intervals(self, ci):
        rad = ci.rad.expand(ci.n, -1)
        return (rad[:, :-1] - rad[:, 1:]).contiguous()                     # -diff(radius)

    def _rt_transit(self, plan, call_, ci, ec, table, column, work):
        rad, path = self._transit_geometry(call_, ci)
        if not plan.ordered:
            return batch.transit_spectrum_batch(ec, path, rad, self.rstar, self.itop,
                                                self.nlayers, self.maxdepth)
        # columns in depth order: wavefronts stop at the row tile where theirs have all crossed
        args = (ec, path, rad, column, self.rstar, self.itop, self.nlayers, self.maxdepth)
        if plan.limited:
            return self._limited_rt(batch.transit_spectrum_ordered, args, ci, table, work,
                                    work=work[2])
        return batch.transit_spectrum_ordered(*args)

    def _rt_emission(self, plan, ci, ec, table, wn, column, work):
        """Emission and two-stream geometry."""
        intervals = self._intervals(ci)
        if plan.form == 'two_stream':
            # depth without a stop + both sweeps in one launch; ec is consumed
            return self._two_stream(ci, ec, intervals, wn)
        args = (ec, intervals, wn, ci.temps, self.mu, self.weights, self.itop, self.nlayers,
                self.maxdepth, column)
        if plan.limited:
            return self._limited_rt(batch.emission_flux_batch, args, ci, table, work)
        return batch.emission_flux_batch(*args)

    def _rt_contribution(self, plan, call_, ci, ec, wn, cout):
        """The radiative transfer of a chunk whose band contribution functions are asked for
        (grid order, every layer): -> spectra; cout[n, L, nbands] is filled."""
        if plan.form == 'transit':
            # The spectra come from the launch a call without contribution_out makes (the
            # matrix-core kernel stores no depth, and the kernel that does rounds its sums
            # differently: ~1e-16 relative), so that they keep their bits; a second pass stores
            # depth and ideep, and the transmittance is read from them.
            rad, path = self._transit_geometry(call_, ci)
            spectra = batch.transit_spectrum_batch(ec, path, rad, self.rstar, self.itop,
                                                   self.nlayers, self.maxdepth)
            _, depth, ideep = batch.transit_spectrum_batch(
                ec, path, rad, self.rstar, self.itop, self.nlayers, self.maxdepth, want_depth=True)
            batch.band_transmittance_batch(depth, ideep, call_.bands, self.itop, out=cout)
            return spectra
        # (before the flux: two_stream_batch consumes ec)
        intervals = self._intervals(ci)
        batch.band_contribution_emission_batch(ec, intervals, ci.temps, call_.bands, None,
                                               self.itop, self.nlayers, self.maxdepth, out=cout,
                                               dlogp=call_.dlogp)
        if plan.form == 'two_stream':
            return self._two_stream(ci, ec, intervals, wn)
        return batch.emission_flux_batch(ec, intervals, wn, ci.temps, self.mu, self.weights,
                                         self.itop, self.nlayers, self.maxdepth, None)

    def _two_stream(self, ci, ec, intervals, wn):
        """Depth without a stop + both sweeps in one launch (ec is consumed): the shared flux_top,
        or with irradiation= every walker's own top boundary from the stellar grid at its tstar."""
        if getattr(self, 'irradiation', None) is None:
            return batch.two_stream_batch(ec, intervals, wn, ci.temps, self.f_int, self.flux_top)
        grid, factor = self.irradiation
        return batch.two_stream_batch_star(ec, intervals, wn, ci.temps, self.f_int, grid, factor,
                                           ci.tstar)

    def _rt_clouds(self, call_, ci, ec, wn, column, cout=None):
        """A cloud deck and / or patchy clouds on the CLEAR ec: the deck state and the cloud-type
        models' factors are one small launch each, and one pass over ec gives
        f cloudy + (1 - f) clear.  cout[n, L, nbands] (or None): the chunk's band contribution
        functions, from the same deck state and factors in one more pass over ec (grid order:
        column is None).  -> (spectra, what must outlive the chunk's launches)."""
        cont = self.continuum
        deck = None if ci.deck_logp is None else \
            batch.deck_state_batch(cont.pressure_d, ci.deck_logp, ci.rad, ci.temps)
        terms = keep = None
        cops = None if cont is None else cont.cloud_operands(column)
        if cops is not None:
            terms, keep = cops.plan(ci.temps, ci.ckw['continuum_pars'])
        if self.rt_path == 'transit':
            path = call_.path1 if call_.shared_radius else \
                transit_path_device(ci.rad.contiguous(), self.itop)
            spectra = batch.cloudy_transit_batch(ec, path, ci.rad, self.rstar, self.itop,
                                                 self.maxdepth, deck=deck, f_patchy=ci.f_patchy,
                                                 column=column, _terms=terms)
            if cout is not None:
                batch.band_transmittance_cloudy_batch(ec, path, call_.bands, self.itop,
                                                      self.maxdepth, deck=deck,
                                                      f_patchy=ci.f_patchy, out=cout,
                                                      _terms=terms)
        else:
            if cout is not None:
                batch.band_contribution_emission_cloudy_batch(
                    ec, self._intervals(ci), ci.temps, call_.bands, None, self.itop,
                    self.nlayers, self.maxdepth, deck=deck, out=cout, dlogp=call_.dlogp,
                    _terms=terms)
            spectra = batch.cloudy_emission_batch(ec, self._intervals(ci), wn, ci.temps, self.mu,
                                                  self.weights, self.itop, self.maxdepth,
                                                  deck=deck, f_patchy=ci.f_patchy, column=column,
                                                  _terms=terms)
        return spectra, keep
