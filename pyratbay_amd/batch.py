"""The walker-batch wrappers of the retrieval loop: one launch per stage for a chunk of walkers
(interpolation of the table, transit / emission / two-stream radiative transfer, cloud deck and
patchy clouds).  TableSpectrum.eval_bands (table.py) looks them up in this module."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from . import continuum as ct
from ._capi import call
from ._device import _ptr, _stream, dev


def interp_ec_batch(etable, ttable, temps, dens, out=None, tile_limit=None, row0=0, gate=None,
                    work=None, continuum=None, continuum_density=None, continuum_pars=None,
                    alkali_density=None):
    """interp_ec for a batch of walkers (assigning): temps[nw, L], dens[nw, L, S] ->
    ec[nw, L, W]; the table is read once per chunk of walkers.  tile_limit (int32[ceil(W/256)],
    device) / row0: only the layers a block of 256 columns can need are written
    (pb_interp_ec_batch_limited); gate (int32[1], device): the launch does nothing unless the
    flag is set, and runs on the `work` buffer its first pass filled.
    continuum: a continuum.Continuum (grid order) or its batch_operands(order) (the table's column
    order): its terms are added to every sample before it is stored (pb_interp_ec_batch_cont),
    with continuum_density[nw, L, len(continuum.species)] and continuum_pars[nw, npars] (None:
    the models' current parameters) as device tensors.  alkali_density[nw, L,
    len(continuum.alkali)] (device; the densities of continuum.alkali_species): the alkali
    doublets are added too, their Voigt values at the detuning distance formed on the device
    (valid while VanderWaals.detuning_x(T) >= continuum.BATCH_MIN_X: the caller's check, see
    Continuum.check_alkali_batch); None: the alkali models add nothing."""
    nmol, ntemp, nlayers, nwave = etable.shape
    nw = temps.shape[0]
    assert temps.shape == (nw, nlayers) and dens.shape == (nw, nlayers, nmol)
    if out is None:
        out = torch.empty((nw, nlayers, nwave), dtype=torch.float64, device=etable.device)
    if continuum is not None:
        ops = continuum.batch_operands() if hasattr(continuum, 'batch_operands') else continuum
        if continuum_pars is None and ops.npars:
            continuum_pars = ops.cont.default_pars()
        cd = None if continuum_density is None else continuum_density.contiguous()
        cp = None if continuum_pars is None else continuum_pars.contiguous()
        ad = None if alkali_density is None else alkali_density.contiguous()
        if work is None:
            work = torch.empty(ops.work_doubles(nlayers, nwave, nw), dtype=torch.float64,
                               device=etable.device)
        args = ops.args(cd, cp, ad)
        if tile_limit is None and gate is None:
            call('pb_interp_ec_batch_cont', _ptr(out), _ptr(etable), _ptr(ttable),
                 _ptr(temps.contiguous()), _ptr(dens.contiguous()), _ptr(work), nmol, ntemp,
                 nlayers, nwave, nw, args, _stream())
        else:
            call('pb_interp_ec_batch_cont_limited', _ptr(out), _ptr(etable), _ptr(ttable),
                 _ptr(temps.contiguous()), _ptr(dens.contiguous()), _ptr(work), nmol, ntemp,
                 nlayers, nwave, nw, args, _ptr(tile_limit), int(row0), _ptr(gate), _stream())
        return out
    if work is None:
        work = torch.empty(_capi.lib().pb_interp_ec_batch_work_doubles(nlayers, nw),
                           dtype=torch.float64, device=etable.device)
    if tile_limit is None and gate is None:
        call('pb_interp_ec_batch', _ptr(out), _ptr(etable), _ptr(ttable),
             _ptr(temps.contiguous()), _ptr(dens.contiguous()), _ptr(work), nmol, ntemp, nlayers,
             nwave, nw, _stream())
    else:
        call('pb_interp_ec_batch_limited', _ptr(out), _ptr(etable), _ptr(ttable),
             _ptr(temps.contiguous()), _ptr(dens.contiguous()), _ptr(work), nmol, ntemp, nlayers,
             nwave, nw, _ptr(tile_limit), int(row0), _ptr(gate), _stream())
    return out


def transit_spectrum_batch(ec, raypath, radius, rstar, itop, ibottom, maxdepth,
                           want_depth=False):
    """optical depth + transmission for a batch: ec[nw, L, W], raypath[nw, npath],
    radius[nw, L] -> spectrum[nw, W] (and depth[nw, L, W], ideep[nw, W] when asked for)."""
    nw, nlayers, nwave = ec.shape
    spectrum = torch.empty((nw, nwave), dtype=torch.float64, device=ec.device)
    depth = ideep = None
    if want_depth:
        depth = torch.empty_like(ec)
        ideep = torch.empty((nw, nwave), dtype=torch.int32, device=ec.device)
    nwork = _capi.lib().pb_transit_work_doubles(nlayers, int(itop), int(ibottom), nwave, nw)
    work = torch.empty(nwork, dtype=torch.float64, device=ec.device)
    call('pb_transit_spectrum_batch', _ptr(spectrum), _ptr(depth), _ptr(ideep), _ptr(ec),
         _ptr(raypath), _ptr(radius), float(rstar), int(itop), int(ibottom), float(maxdepth),
         nlayers, nwave, nw, _ptr(work), _stream())
    return (spectrum, depth, ideep) if want_depth else spectrum


def transit_spectrum_ordered(ec, raypath, radius, column, rstar, itop, ibottom, maxdepth,
                             tile_limit=None, flags=None, gate=None, out=None, work=None):
    """transit_spectrum_batch for ec[nw, L, W] whose columns are in the order `column` (int32[W]:
    grid index of each column): spectrum[nw, W] in GRID order.  Wavefronts stop at the row tile in
    which their 32 columns have all crossed maxdepth (pb_transit_spectrum_ordered).  With
    tile_limit / flags / gate: pb_transit_spectrum_limited (see interp_ec_batch)."""
    nw, nlayers, nwave = ec.shape
    spectrum = out if out is not None else torch.empty((nw, nwave), dtype=torch.float64,
                                                       device=ec.device)
    if work is None:
        nwork = _capi.lib().pb_transit_work_doubles(nlayers, int(itop), int(ibottom), nwave, nw)
        work = torch.empty(nwork, dtype=torch.float64, device=ec.device)
    if tile_limit is None and gate is None:
        call('pb_transit_spectrum_ordered', _ptr(spectrum), _ptr(ec), _ptr(raypath), _ptr(radius),
             _ptr(column), float(rstar), int(itop), int(ibottom), float(maxdepth), nlayers, nwave,
             nw, _ptr(work), _stream())
    else:
        call('pb_transit_spectrum_limited', _ptr(spectrum), _ptr(ec), _ptr(raypath), _ptr(radius),
             _ptr(column), float(rstar), int(itop), int(ibottom), float(maxdepth), nlayers, nwave,
             nw, _ptr(work), _ptr(tile_limit), _ptr(flags), _ptr(gate), _stream())
    return spectrum


def table_transit_supported(nmol, ntemp, nlayers, itop, ibottom, nwave):
    """Whether the one-pass form (table_transit_batch) exists for this shape -- never in the
    default library (an experiment: libpbhip_exp.so)."""
    if not _capi.experiments():
        return False
    return bool(_capi.lib().pb_table_transit_supported(int(nmol), int(ntemp), int(nlayers),
                                                       int(itop), int(ibottom), int(nwave)))


def table_transit_batch(etable, ttable, temps, dens, raypath, radius, rstar, itop, ibottom,
                        maxdepth):
    """interp_ec + optical depth + transmission of a batch of walkers in ONE pass
    (pb_table_transit_batch; experiments build of the library only): etable[S, T, L, W],
    temps[nw, L], dens[nw, L, S],
    raypath[nw, npath], radius[nw, L] -> spectrum[nw, W].  The interpolated extinction is
    the operand of the matrix products and is never stored."""
    nmol, ntemp, nlayers, nwave = etable.shape
    nw = temps.shape[0]
    assert temps.shape == (nw, nlayers) and dens.shape == (nw, nlayers, nmol)
    assert radius.shape == (nw, nlayers) and raypath.shape[0] == nw
    spectrum = torch.empty((nw, nwave), dtype=torch.float64, device=etable.device)
    if not _capi.experiments():
        call('pb_table_transit_batch')                     # (raises: not in libpbhip.so)
    nwork = _capi.lib().pb_table_transit_work_doubles(nmol, nlayers, int(itop), int(ibottom), nw)
    work = torch.empty(max(nwork, 8), dtype=torch.float64, device=etable.device)
    call('pb_table_transit_batch', _ptr(spectrum), _ptr(etable), _ptr(ttable),
         _ptr(temps.contiguous()), _ptr(dens.contiguous()), _ptr(raypath.contiguous()),
         _ptr(radius.contiguous()), float(rstar), int(itop), int(ibottom), float(maxdepth),
         nmol, ntemp, nlayers, nwave, nw, _ptr(work), _stream())
    return spectrum


def emission_flux_batch(ec, intervals, wn, temps, mu, weights, itop, ibottom, maxdepth,
                        column=None, tile_limit=None, flags=None, gate=None, out=None):
    """plane-parallel optical depth + emission flux for a batch: ec[nw, L, W],
    intervals[nw, L-1], temps[nw, L] -> flux[nw, W] (no cloud deck).  With `column` (int32[W]) the
    columns of ec and wn are in that order (grid index of each) and flux comes in grid order.
    tile_limit / flags / gate (ordered columns only): pb_emission_flux_limited, see
    interp_ec_batch."""
    nw, nlayers, nwave = ec.shape
    flux = out if out is not None else torch.empty((nw, nwave), dtype=torch.float64,
                                                   device=ec.device)
    if tile_limit is not None or gate is not None:
        call('pb_emission_flux_limited', _ptr(flux), _ptr(ec), _ptr(intervals.contiguous()),
             _ptr(wn), _ptr(temps.contiguous()), _ptr(mu), _ptr(weights), _ptr(column), len(mu),
             float(maxdepth), int(itop), int(ibottom), nlayers, nwave, nw, _ptr(tile_limit),
             _ptr(flags), _ptr(gate), _stream())
        return flux
    if column is not None:
        call('pb_emission_flux_ordered', _ptr(flux), _ptr(ec), _ptr(intervals.contiguous()),
             _ptr(wn), _ptr(temps.contiguous()), _ptr(mu), _ptr(weights), _ptr(column), len(mu),
             float(maxdepth), int(itop), int(ibottom), nlayers, nwave, nw, _stream())
        return flux
    call('pb_emission_flux_batch', _ptr(flux), _ptr(ec), _ptr(intervals.contiguous()), _ptr(wn),
         _ptr(temps.contiguous()), _ptr(mu), _ptr(weights), len(mu), float(maxdepth), int(itop),
         int(ibottom), nlayers, nwave, nw, _stream())
    return flux


def two_stream_batch(ec, intervals, wn, temps, f_int=None, flux_top=None, out=None, work=None):
    """plane-parallel optical depth without a stop + two-stream fluxes for a batch, itop = 0:
    ec[nw, L, W], intervals[nw, L-1], temps[nw, L], f_int[W] / flux_top[W] (shared by the walkers;
    None: none) -> flux_up[0] of every walker, [nw, W].  ec is CONSUMED: the kernel leaves each
    interval's optical depth in it (pb_two_stream_batch).  work: at least
    pb_two_stream_batch_work_doubles(L, W, nw) doubles of scratch (None: allocated here)."""
    nw, nlayers, nwave = ec.shape
    assert ec.is_contiguous() and ec.dtype == torch.float64
    flux = out if out is not None else torch.empty((nw, nwave), dtype=torch.float64,
                                                   device=ec.device)
    need = _capi.lib().pb_two_stream_batch_work_doubles(nlayers, nwave, nw)
    if work is None:
        work = torch.empty(need, dtype=torch.float64, device=ec.device) if need else None
    elif work.numel() < need or work.dtype != torch.float64 or not work.is_contiguous():
        raise ValueError(f'two_stream_batch: work must hold {need} contiguous doubles')
    call('pb_two_stream_batch', _ptr(flux), _ptr(ec), _ptr(intervals.contiguous()), _ptr(wn),
         _ptr(temps.contiguous()), _ptr(f_int), _ptr(flux_top), _ptr(work), nlayers, nwave, nw,
         _stream())
    return flux


def two_stream_batch_star(ec, intervals, wn, temps, f_int, star_grid, factor, tstar, out=None,
                          work=None):
    """two_stream_batch with every walker's own irradiation (pb_two_stream_batch_star): the top
    boundary of walker w is factor * star_grid.flux_host(tstar[w]) -- star_grid: an
    observation.StellarGrid on wn, factor = beta_irr * (rstar / smaxis)**2, tstar[nw] a float64
    device tensor -- formed per column inside the sweep, no flux_top[nw, W] is stored.  The bits
    of two_stream_batch run one walker at a time with that flux_top.  A walker whose tstar is NaN
    or outside the grid's temperatures gets a row of +inf."""
    nw, nlayers, nwave = ec.shape
    assert ec.is_contiguous() and ec.dtype == torch.float64
    if star_grid.nwave != nwave:
        raise ValueError(f'two_stream_batch_star: the stellar grid has {star_grid.nwave} samples, '
                         f'the columns {nwave}')
    _check_walker_tensor('two_stream_batch_star: tstar', tstar, nw)
    flux = out if out is not None else torch.empty((nw, nwave), dtype=torch.float64,
                                                   device=ec.device)
    need = _capi.lib().pb_two_stream_batch_work_doubles(nlayers, nwave, nw)
    if work is None:
        work = torch.empty(need, dtype=torch.float64, device=ec.device) if need else None
    elif work.numel() < need or work.dtype != torch.float64 or not work.is_contiguous():
        raise ValueError(f'two_stream_batch_star: work must hold {need} contiguous doubles')
    call('pb_two_stream_batch_star', _ptr(flux), _ptr(ec), _ptr(intervals.contiguous()), _ptr(wn),
         _ptr(temps.contiguous()), _ptr(f_int), _ptr(star_grid.fluxes), _ptr(star_grid.sed_temps),
         _ptr(tstar.contiguous()), float(factor), star_grid.nt, _ptr(work), nlayers, nwave, nw,
         _stream())
    return flux


# --------------------------------------------------------------------------
# Band contribution functions for a batch (pb_contribution.hip)
# --------------------------------------------------------------------------
def _contribution_buffers(name, bands, nw, nlayers, nwave, device, out):
    """The output [nw, L, nbands] (checked when given), the work buffer and the band arguments of
    the two contribution entries."""
    if not hasattr(bands, 'response') or not hasattr(bands, 'offset'):
        raise ValueError(f'{name}: bands must be a PassBands (high-resolution data have no '
                         'contribution functions here)')
    if tuple(bands.wn.shape) != (nwave,):
        raise ValueError(f'{name}: the bands are on a grid of {tuple(bands.wn.shape)} samples, '
                         f'the columns on one of {nwave}')
    shape = (nw, nlayers, bands.nbands)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=device)
    else:
        _check_walker_tensor(f'{name}: out', out, nw, shape=shape)
        if not out.is_contiguous():
            raise ValueError(f'{name}: out must be contiguous')
    max_count = bands.max_count if hasattr(bands, 'max_count') else \
        int(bands.count.max()) if bands.nbands else 0
    need = _capi.lib().pb_band_contribution_work_doubles(nlayers, bands.nbands, max_count, nw)
    work = torch.empty(max(need, 1), dtype=torch.float64, device=device)
    args = (_ptr(bands.start), _ptr(bands.count), _ptr(bands.response), _ptr(bands.offset),
            max_count)
    return out, work, args


def band_transmittance_batch(depth, ideep, bands, itop, out=None):
    """Band transmittances of a batch in transit geometry (Pyrat.band_contribution:
    contribution_funcs.transmittance + band_cf; contribution.band_contribution_host is the NumPy
    statement): depth[nw, L, W] and ideep[nw, W] (int32) as transit_spectrum_batch(...,
    want_depth=True) returns them, bands: a PassBands on the same grid -> [nw, L, nbands], every
    band divided by its maximum over the layers (a band of one sample: NaN)."""
    nw, nlayers, nwave = depth.shape
    if depth.dtype != torch.float64 or not depth.is_contiguous() or \
            ideep.dtype != torch.int32 or tuple(ideep.shape) != (nw, nwave):
        raise ValueError(f'band_transmittance_batch: contiguous float64 depth[nw, L, W] and int32 '
                         f'ideep[{nw}, {nwave}] wanted, got {depth.dtype} {tuple(depth.shape)}, '
                         f'{ideep.dtype} {tuple(ideep.shape)}')
    out, work, bargs = _contribution_buffers('band_transmittance_batch', bands, nw, nlayers,
                                             nwave, depth.device, out)
    call('pb_band_transmittance_batch', _ptr(out), _ptr(depth), _ptr(ideep.contiguous()),
         _ptr(bands.wn), *bargs, int(itop), nlayers, nwave, bands.nbands, nw, _ptr(work),
         _stream())
    return out


def _emission_contribution_args(name, ec, intervals, temps, pressure, dlogp):
    """What the two emission contribution wrappers check alike: ec[nw, L, W], intervals[nw, L-1]
    and temps[nw, L]; dlogp[L-1] (formed from pressure when None) -> dlogp."""
    nw, nlayers, _ = ec.shape
    if ec.dtype != torch.float64 or not ec.is_contiguous() or \
            tuple(intervals.shape) != (nw, nlayers - 1) or tuple(temps.shape) != (nw, nlayers):
        raise ValueError(f'{name}: contiguous float64 ec[nw, L, W], intervals[{nw}, '
                         f'{nlayers - 1}] and temps[{nw}, {nlayers}] wanted, got '
                         f'{tuple(ec.shape)}, {tuple(intervals.shape)}, {tuple(temps.shape)}')
    if dlogp is None:
        return contribution_dlogp(pressure, nlayers)
    if not isinstance(dlogp, torch.Tensor) or not dlogp.is_cuda or \
            dlogp.dtype != torch.float64 or tuple(dlogp.shape) != (nlayers - 1,):
        raise ValueError(f'{name}: dlogp must be a float64 device tensor of shape '
                         f'({nlayers - 1},)')
    return dlogp


def band_contribution_emission_batch(ec, intervals, temps, bands, pressure, itop, ibottom,
                                     maxdepth, out=None, dlogp=None):
    """Band contribution functions of a batch in emission or two-stream geometry
    (contribution_funcs.contribution_function + band_cf) from ec[nw, L, W] directly:
    intervals[nw, L-1] = -diff(radius), temps[nw, L], pressure[L] in any unit (host array or
    tensor: only diff(log(pressure)), formed on the host with NumPy, enters; or None with dlogp =
    contribution_dlogp(pressure, L), formed once for several calls), maxdepth (inf in two-stream
    geometry: no stop) -> [nw, L, nbands].  Neither the depth nor B is stored; ec is
    only read."""
    name = 'band_contribution_emission_batch'
    nw, nlayers, nwave = ec.shape
    dlogp = _emission_contribution_args(name, ec, intervals, temps, pressure, dlogp)
    out, work, bargs = _contribution_buffers(name, bands, nw, nlayers, nwave, ec.device, out)
    call('pb_band_contribution_emission_batch', _ptr(out), _ptr(ec),
         _ptr(intervals.contiguous()), _ptr(dlogp.contiguous()), _ptr(bands.wn),
         _ptr(temps.contiguous()), *bargs, float(maxdepth), int(itop), int(ibottom), nlayers,
         nwave, bands.nbands, nw, _ptr(work), _stream())
    return out


def contribution_dlogp(pressure, nlayers):
    """diff(log(pressure)) [L-1] on the device, formed with NumPy (the bits of the host form) from
    pressure[L], a host array or a tensor (read back)."""
    p = pressure.cpu().numpy() if isinstance(pressure, torch.Tensor) else pressure
    p = np.asarray(p, float)
    if p.shape != (nlayers,):
        raise ValueError(f'contribution pressure must have shape ({nlayers},), got {p.shape}')
    return dev(np.diff(np.log(p)))


# --------------------------------------------------------------------------
# Cloud deck and patchy clouds for a batch (pb_clouds.hip)
# --------------------------------------------------------------------------
def alkali_voigt_det_batch(model, temps, pressure_barye=None):
    """VanderWaals.voigt_det for a batch of walkers on the device (pb_alkali_voigt_det_batch):
    temps[nw, L] (device) -> [nw, L, model.nlines].  pressure_barye[L] (device; None: the
    model's pressures).  The device's Faddeeva function needs model.detuning_x(T) >=
    continuum.BATCH_MIN_X at every temperature (it grows with T): not checked here."""
    nw, nlayers = temps.shape
    if pressure_barye is None:
        pressure_barye = dev(np.asarray(model.pressure, float) * 1e6)
    assert pressure_barye.shape == (nlayers,)
    out = torch.empty((nw, nlayers, model.nlines), dtype=torch.float64, device=temps.device)
    wn0 = np.ascontiguousarray(model.wn0, float)
    call('pb_alkali_voigt_det_batch', _ptr(out), _ptr(temps.contiguous()),
         _ptr(pressure_barye.contiguous()), float(model.detuning), float(model.mass),
         float(model.lpar), _capi.hptr(wn0), model.nlines, nlayers, nw, _stream())
    return out


def deck_state_batch(pressure, logp, radius, temps):
    """The state of an opaque cloud deck at 10**logp[w] bar for every walker
    (opacity/clouds/gray.py:129-150), on the device in one launch, nothing read back:
    pressure[L] (bar), logp[nw], radius[nw, L] or [1, L] / [L] (shared), temps[nw, L] ->
    (itop int32[nw], rsurf[nw], tsurf[nw]).  itop = the first layer with pressure >= the deck's
    (L - 1 beyond the bottom of the grid, 1 above its top); rsurf / tsurf are linear in pressure
    and CLAMPED to the end values outside the grid, as continuum.Deck does (the reference's
    interp1d raises there).  continuum.deck_state is the NumPy mirror."""
    nw, nlayers = temps.shape
    rad = radius if radius.dim() == 2 else radius.view(1, -1)
    if tuple(pressure.shape) != (nlayers,) or tuple(logp.shape) != (nw,) or \
            rad.shape[1] != nlayers or rad.shape[0] not in (1, nw):
        raise ValueError(f'deck_state_batch: pressure[{nlayers}], logp[{nw}], radius[{nw} or 1, '
                         f'{nlayers}] wanted, got {tuple(pressure.shape)}, {tuple(logp.shape)}, '
                         f'{tuple(radius.shape)}')
    itop = torch.empty(nw, dtype=torch.int32, device=temps.device)
    rsurf = torch.empty(nw, dtype=torch.float64, device=temps.device)
    tsurf = torch.empty(nw, dtype=torch.float64, device=temps.device)
    rad = rad.contiguous()
    call('pb_deck_state_batch', _ptr(itop), _ptr(rsurf), _ptr(tsurf), _ptr(pressure.contiguous()),
         _ptr(logp.contiguous()), _ptr(rad), 0 if rad.shape[0] == 1 else nlayers,
         _ptr(temps.contiguous()), nlayers, nw, _stream())
    return itop, rsurf, tsurf


def _check_walker_tensor(name, t, nw, dtype=torch.float64, shape=None):
    """A per-walker argument of eval_bands: None, or a device tensor [nw] (or of `shape`) of
    `dtype` (its data pointer goes to a kernel as that element type)."""
    if t is None:
        return
    kind = str(dtype).replace('torch.', '')
    shape = (nw,) if shape is None else tuple(shape)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or \
            tuple(t.shape) != shape:
        raise ValueError(f'{name} must be a {kind} device tensor of shape {shape}, got '
                         f'{type(t).__name__} {getattr(t, "dtype", "")} '
                         f'{tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')


def _cloud_args(prefix, nw, deck, surf, cloud_cs, cloud_f, f_patchy, terms, flux=None):
    """What the cloudy flux and contribution wrappers share: the deck's tensors (deck[0] and
    deck[surf]), the pb_cloud_terms struct, f_patchy and the tensors that must outlive the
    launch; `prefix` opens the names in the error messages.  flux = (nwave, device, want_parts,
    out): the outputs (spectrum, clear, cloudy) too, else None.
    -> (deck itop, deck surface, terms by reference or None, f_patchy, outputs, keep-alive)."""
    for name, t, dtype in (('f_patchy', f_patchy, torch.float64),) + \
            (() if deck is None else (('deck itop', deck[0], torch.int32),
                                      ('deck surface', deck[surf], torch.float64))):
        _check_walker_tensor(prefix + name, t, nw, dtype)
    keep = []
    if terms is None and cloud_cs is not None:
        if cloud_f is None or cloud_f.dim() != 3 or cloud_f.shape[0] != nw:
            raise ValueError(f'{prefix}cloud_cs needs cloud_f[nw, L, nr]')
        terms, keep = ct.cloud_terms(cloud_cs, cloud_f)
    outs = None
    if flux is not None:
        nwave, device, want_parts, out = flux
        spectrum = out if out is not None else torch.empty((nw, nwave), dtype=torch.float64,
                                                           device=device)
        outs = (spectrum, torch.empty_like(spectrum) if want_parts else None,
                torch.empty_like(spectrum) if want_parts else None)
    ditop = None if deck is None else deck[0].contiguous()
    dsurf = None if deck is None else deck[surf].contiguous()
    fp = None if f_patchy is None else f_patchy.contiguous()
    return (ditop, dsurf, None if terms is None else C.byref(terms), fp, outs,
            (keep, terms, ditop, dsurf, fp))


def _ray_path_args(raypath, nw, nrow):
    """The ray paths of the two cloudy transit wrappers: raypath[nw, npath] or [1, npath] /
    [npath] (shared), npath = nrow (nrow - 1) / 2 the packed triangle of nrow impact parameters
    -> (whether the shape fits, npath, the C arguments (pointer or None, walker stride), the
    tensor they point into)."""
    path = (raypath if raypath.dim() == 2 else raypath.view(1, -1)).contiguous()
    npath = (nrow * (nrow - 1)) // 2
    fits = path.shape[0] in (1, nw) and path.shape[1] == npath
    return fits, npath, (_ptr(path) if path.numel() else None,
                         0 if path.shape[0] == 1 else path.shape[1]), path


def cloudy_transit_batch(ec, raypath, radius, rstar, itop, maxdepth, deck=None, cloud_cs=None,
                         cloud_f=None, f_patchy=None, want_parts=False, column=None, out=None,
                         _terms=None):
    """Transit spectra of a batch with a cloud deck and / or patchy clouds, ONE pass over
    ec[nw, L, W] (opacity/optic_depth.py:94-121, spectrum/radiative_transfer.py:57-71,
    pyrat/spectrum.py:350-363):
      clear   ec over all layers from itop, no deck
      cloudy  ec + ec_cloud down to the deck: deck = deck_state_batch()'s (itop[nw], rsurf[nw],
              tsurf[nw]); None: down to the last layer
      spectrum = f_patchy[w] cloudy + (1 - f_patchy[w]) clear; f_patchy None: the cloudy column
    ec_cloud = sum_m cloud_cs[m] x cloud_f[:, :, m] is never stored: cloud_cs[nr, W] (or
    [nr, nw, W], a row per walker), cloud_f[nw, L, nr], nr <= 8; None: no cloud opacity, the two
    columns then share one optical-depth sum down to the deck.  f_patchy is CLAMPED to [0, 1] on
    the device (NaN gives NaN).  raypath[nw, npath] or [1, npath] / [npath] (shared; the packed
    triangle of transit_path_device), radius[nw, L] or [1, L] / [L].  column (int32[W]): ec's
    columns are in that order, the spectra come in grid order (same bits).
    -> spectrum[nw, W], or (spectrum, clear, cloudy) with want_parts."""
    nw, nlayers, nwave = ec.shape
    rad = radius if radius.dim() == 2 else radius.view(1, -1)
    fits, npath, pargs, path = _ray_path_args(raypath, nw, nlayers - int(itop))
    if rad.shape[1] != nlayers or rad.shape[0] not in (1, nw) or not fits:
        raise ValueError(f'cloudy_transit_batch: radius[{nw} or 1, {nlayers}] and raypath[{nw} or '
                         f'1, {npath}] wanted, got {tuple(radius.shape)}, '
                         f'{tuple(raypath.shape)}')
    ditop, dsurf, terms, fp, (spectrum, clear, cloudy), keep = _cloud_args(
        '', nw, deck, 1, cloud_cs, cloud_f, f_patchy, _terms,
        flux=(nwave, ec.device, want_parts, out))
    rad = rad.contiguous()
    call('pb_cloudy_transit_batch', _ptr(spectrum), _ptr(clear), _ptr(cloudy), _ptr(ec), *pargs,
         _ptr(rad), 0 if rad.shape[0] == 1 else nlayers, _ptr(column), float(rstar), int(itop),
         float(maxdepth), nlayers, nwave, nw, _ptr(ditop), _ptr(dsurf), terms, _ptr(fp),
         _stream())
    del keep, path
    return (spectrum, clear, cloudy) if want_parts else spectrum


def cloudy_emission_batch(ec, intervals, wn, temps, mu, weights, itop, maxdepth, deck=None,
                          cloud_cs=None, cloud_f=None, f_patchy=None, want_parts=False,
                          column=None, out=None, _terms=None):
    """The emission counterpart of cloudy_transit_batch (opacity/optic_depth.py:123-136,
    spectrum/radiative_transfer.py:74-139, pyrat/spectrum.py:366-385): intervals[nw, L-1],
    temps[nw, L], wn[W] in ec's column order.  The cloudy column's deepest layer is the deck's
    itop, which radiates at the deck's tsurf -- in the clear column too: the reference's cloudy
    pass overwrites that row of its Planck array and its clear pass reads it (reproduced, like
    patchy_emission_flux does)."""
    nw, nlayers, nwave = ec.shape
    if tuple(intervals.shape) != (nw, nlayers - 1) or tuple(temps.shape) != (nw, nlayers) or \
            tuple(wn.shape) != (nwave,):
        raise ValueError(f'cloudy_emission_batch: intervals[{nw}, {nlayers - 1}], temps[{nw}, '
                         f'{nlayers}], wn[{nwave}] wanted, got {tuple(intervals.shape)}, '
                         f'{tuple(temps.shape)}, {tuple(wn.shape)}')
    ditop, dsurf, terms, fp, (flux, clear, cloudy), keep = _cloud_args(
        '', nw, deck, 2, cloud_cs, cloud_f, f_patchy, _terms,
        flux=(nwave, ec.device, want_parts, out))
    call('pb_cloudy_emission_batch', _ptr(flux), _ptr(clear), _ptr(cloudy), _ptr(ec),
         _ptr(intervals.contiguous()), _ptr(wn), _ptr(temps.contiguous()), _ptr(mu), _ptr(weights),
         _ptr(column), len(mu), float(maxdepth), int(itop), nlayers, nwave, nw, _ptr(ditop),
         _ptr(dsurf), terms, _ptr(fp), _stream())
    del keep
    return (flux, clear, cloudy) if want_parts else flux


# --------------------------------------------------------------------------
# Band contribution functions for a batch with clouds (pb_contribution.hip)
# --------------------------------------------------------------------------
def band_transmittance_cloudy_batch(ec, raypath, bands, itop, maxdepth, deck=None, cloud_cs=None,
                                    cloud_f=None, f_patchy=None, out=None, _terms=None):
    """Band transmittances of a batch in transit geometry WITH clouds (Pyrat.band_contribution,
    pyrat_obj.py:671-696, on the two optical depths of opacity/optic_depth.py:94-121;
    contribution.band_contribution_cloudy_host is the NumPy statement), from ec[nw, L, W] in ONE
    pass -- neither column's depth is stored -- with the walk and the arguments of
    cloudy_transit_batch:
      clear   ec over the rows itop .. L-1
      cloudy  ec + ec_cloud over the rows itop .. deck itop: deck = deck_state_batch()'s (itop[nw],
              rsurf[nw], tsurf[nw]; only itop enters); None: down to the last row
      transmittance  exp(-depth) above the row where a column exceeded maxdepth, or its last row;
              0 from there on; 1 above itop
      value   f_patchy[w] cloudy + (1 - f_patchy[w]) clear per sample, before the band integral;
              f_patchy None: the cloudy column alone.  f_patchy is CLAMPED to [0, 1] on the device
              (NaN gives NaN).
    ec_cloud = sum_m cloud_cs[m] x cloud_f[:, :, m] as in cloudy_transit_batch (None: none, one
    running sum serves both columns).  raypath[nw, npath] or [1, npath] / [npath] (shared).
    -> [nw, L, nbands], every band divided by its maximum over the layers (one sample: NaN)."""
    name = 'band_transmittance_cloudy_batch'
    nw, nlayers, nwave = ec.shape
    fits, npath, pargs, path = _ray_path_args(raypath, nw, nlayers - int(itop))
    if ec.dtype != torch.float64 or not ec.is_contiguous() or not fits:
        raise ValueError(f'{name}: contiguous float64 ec[nw, L, W] and raypath[{nw} or 1, '
                         f'{npath}] wanted, got {ec.dtype} {tuple(ec.shape)}, '
                         f'{tuple(raypath.shape)}')
    ditop, _, terms, fp, _, keep = _cloud_args(f'{name}: ', nw, deck, 1, cloud_cs, cloud_f,
                                               f_patchy, _terms)
    out, work, bargs = _contribution_buffers(name, bands, nw, nlayers, nwave, ec.device, out)
    call('pb_band_transmittance_cloudy_batch', _ptr(out), _ptr(ec), *pargs, _ptr(bands.wn),
         *bargs, int(itop), float(maxdepth), nlayers, nwave, bands.nbands, nw, _ptr(ditop), terms,
         _ptr(fp), _ptr(work), _stream())
    del keep, path
    return out


def band_contribution_emission_cloudy_batch(ec, intervals, temps, bands, pressure, itop, ibottom,
                                            maxdepth, deck=None, cloud_cs=None, cloud_f=None,
                                            out=None, dlogp=None, _terms=None):
    """band_contribution_emission_batch WITH clouds: the contribution function of the CLOUDY
    column only, as the reference (pyrat_obj.py:691-693 reads od.depth and od.B: the clear column
    of a patchy model is not mixed in, and a patchy fraction does not enter).  The column is
    ec + ec_cloud (cloud_cs / cloud_f as in cloudy_emission_batch; None: none); with deck =
    deck_state_batch()'s (itop[nw], rsurf[nw], tsurf[nw]) the depth runs through the row past
    the deck's layer and is 0 below (ibottom = deck itop + 1 per walker; else `ibottom`), and
    that layer radiates at the deck's tsurf.  -> [nw, L, nbands]."""
    name = 'band_contribution_emission_cloudy_batch'
    nw, nlayers, nwave = ec.shape
    dlogp = _emission_contribution_args(name, ec, intervals, temps, pressure, dlogp)
    ditop, dsurf, terms, _, _, keep = _cloud_args(f'{name}: ', nw, deck, 2, cloud_cs, cloud_f,
                                                  None, _terms)
    out, work, bargs = _contribution_buffers(name, bands, nw, nlayers, nwave, ec.device, out)
    call('pb_band_contribution_emission_cloudy_batch', _ptr(out), _ptr(ec),
         _ptr(intervals.contiguous()), _ptr(dlogp.contiguous()), _ptr(bands.wn),
         _ptr(temps.contiguous()), *bargs, float(maxdepth), int(itop), int(ibottom), nlayers,
         nwave, bands.nbands, nw, _ptr(ditop), _ptr(dsurf), terms, _ptr(work), _stream())
    del keep
    return out
