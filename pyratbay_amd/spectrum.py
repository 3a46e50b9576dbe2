"""Whole-path line-by-line model: the three timed stages of Pyrat.run() (pyrat_obj.py:203-214)
for one wavenumber shard, and consecutive spectra kept in flight on several streams."""
import os

import numpy as np
import torch

from . import _capi
from ._capi import call
from ._device import StageTimer, _ptr, _stream, dev, require_gpu, side_streams
from .batch import transit_spectrum_batch
from .columns import (RT_PATHS, default_quadrature, emission_flux, emission_observables,
                      internal_flux, optical_depth_transit, pack_raypath,
                      plane_parallel_optical_depth, transit_path, transit_spectrum,
                      transmission, two_stream)
from .lbl import LBL, LineList, PartitionTable, VoigtTable


class LBLSpectrum:
    """extinction -> optical depth -> spectrum for one wavenumber shard, all on device.

    `case` is a dict as produced by pyratbay_amd.synth.lbl_case (or assembled by a caller
    from a real Pyrat object: the same arrays the reference hands to its C extensions).
    """

    def __init__(self, case, rt_path='transit', wbegin=0, wcount=None, itop=0,
                 quadrature_mu=None, quadrature_weights=None, keep_flat=False,
                 voigt=None, lines=None, tint=0.0, flux_top=None, continuum=None,
                 continuum_density=None, timestamps=True, materialize_depth=True,
                 predict_runs=False, starflux=None, rplanet=None, f_dilution=None,
                 distance=None):
        require_gpu()
        # rt_path: any of the reference's (constants/code_constants.py:83-102) or 'two_stream'
        # (= emission_two_stream).  self.rt_path is the GEOMETRY of the radiative transfer
        # ('transit', 'emission', 'two_stream'); self.observable what is made of an emission-type
        # flux afterwards ('emission', 'eclipse', 'f_lambda'; pyrat/spectrum.py:394-405) from
        # starflux[nwave], rplanet (with atm['rstar']), f_dilution, distance.
        if rt_path not in RT_PATHS:
            raise _capi.PbError(f'rt_path {rt_path!r}: select from {sorted(RT_PATHS)}')
        self.rt_path_name = rt_path
        rt_path, self.observable = RT_PATHS[rt_path]
        # per-stage HIP-event timers behind the `timestamps` property (the reference's
        # pyrat.timestamps keys); timestamps=False: run() records no events
        self._timer = StageTimer() if timestamps else None
        # materialize_depth=False (transit geometry): run() computes the optical depths, applies
        # the reference's exit rule and integrates the spectrum in ONE pass on the matrix cores
        # (pb_transit_spectrum_batch with one "walker": tau = Q . ec) without
        # writing depth[L, W] / ideep[W] -- `self.depth` and `self.ideep` then stay None.  The
        # default keeps the reference's outputs (pyrat.od.depth, pyrat.od.ideep).
        self.materialize_depth = bool(materialize_depth)
        g, atm, ln, iso, vg = (case['grid'], case['atm'], case['lines'], case['iso'],
                               case['voigt'])
        self.case = case
        self.rt_path = rt_path
        # optional continuum terms (pyratbay_amd.continuum.Continuum on this shard's grid)
        # and the host-side number densities {species: n[L]} they use
        self.continuum, self.continuum_density = continuum, continuum_density
        self.nwave = g['nwave']
        self.nlayers = atm['nlayers']
        self.wbegin = wbegin
        self.wcount = self.nwave - wbegin if wcount is None else wcount
        self.itop = itop
        self.maxdepth = case['maxdepth']
        # (resolution mode reads the reference layout only: keep_flat = 2 keeps no second copy)
        interpolate = g.get('resolution') is not None or bool(g.get('interpolate'))
        if interpolate and not keep_flat:
            keep_flat = 2
        self.voigt = voigt or VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'],
                                               g['ownstep'], g['wnosamp'], keep_flat)
        self.lines = lines or LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'],
                                       len(iso['isomass']), g['own'])
        # a constant-resolving-power (or constant-wavelength-step) output grid: the kept samples
        # are interpolated from the dynamic grid (_extcoeff.c:320-326) and ACCUMULATED into ec
        self.resolution = interpolate
        self.lbl = LBL(self.voigt, self.lines, g['wn'], g['divisors'], atm['mol_radius'],
                       atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                       iso['isoiext'], vg['cutoff'], case['ethresh'],
                       resolution=self.resolution, max_layers=self.nlayers)
        if self.resolution:
            # an object made for many spectra: the one-time constant-step sub-plans of the layers'
            # dynamic grids pay off from the second spectrum on (a bare LBL plan keeps the direct gather)
            self.lbl.set_gather_mode('dynamic')
            # predict_runs: plan every call from the last read-back of the layers' oversampling
            # factors instead of synchronising the stream in every call (LBL.set_dyn_predict;
            # results to 1e-12 of the default, bit for bit for a steady atmosphere; capturable)
            if predict_runs:
                self.lbl.set_dyn_predict(True)
        self.predict_runs = bool(predict_runs) and self.resolution
        # atmosphere state, resident (+ the host copy of the temperatures that the continuum
        # terms take their per-layer factors from)
        self.temp_host = np.array(atm['temp'], float)
        self.temp = dev(atm['temp'])
        self.dens = dev(atm['dens'])
        self.isoz = dev(iso['isoz'])
        self.radius = dev(atm['radius'])
        self.rstar = float(atm['rstar'])
        self.wn = dev(g['wn'][wbegin:wbegin + self.wcount])
        if rt_path == 'transit':
            self.raypath = dev(pack_raypath(transit_path(atm['radius'], itop), itop))
        else:
            self.intervals = dev(-np.diff(atm['radius']))
            if quadrature_mu is None:
                quadrature_mu, quadrature_weights = default_quadrature()
            self.mu = dev(quadrature_mu)
            self.weights = dev(quadrature_weights)
        if rt_path == 'two_stream':
            # rt_path emission_two_stream: depth without the maxdepth stop
            # (opacity/optic_depth.py:124-125), internal flux, optional irradiation
            self.maxdepth = np.inf
            self.f_int = internal_flux(self.wn, tint)
            self.flux_top = None if flux_top is None else dev(
                np.asarray(flux_top)[wbegin:wbegin + self.wcount])
            self.flux_down = self.flux_up = None
        self.ec = torch.empty((self.nlayers, 1, self.wcount), dtype=torch.float64,
                              device='cuda')
        self.depth = self.ideep = self.spectrum = None
        # emission-type paths: the planet's flux (after f_dilution) beside `spectrum`, as the
        # reference's spec.fplanet; eclipse: spectrum = fplanet / starflux * (rplanet/rstar)^2
        self.fplanet = None
        self.f_dilution = f_dilution
        self.rplanet = rplanet if rplanet is not None else atm.get('rplanet')
        self.distance = distance
        self.starflux = None
        if self.observable == 'eclipse':
            if starflux is None or self.rplanet is None:
                raise _capi.PbError(f'rt_path {self.rt_path_name!r} needs starflux[nwave] and '
                                    'rplanet (pyrat/argum.py:37-44)')
            self.starflux = dev(np.asarray(starflux, float)[wbegin:wbegin + self.wcount])
        # the TLI file's partition-function tables (from_tli): set_atmosphere() without `isoz`
        # evaluates them at the new temperatures on the device
        self.partition = None
        # a [wcount] tensor the transit spectrum is written to instead of a fresh one (the shard's
        # slot of a gather buffer: dist.SpectrumGather(uniform=True))
        self.spectrum_out = None
        # set to a function(tensor) that all-reduces (MAX) over the ranks to switch the
        # extinction of a wavenumber shard to its two-phase form (dist.kmax_allreduce)
        self.kmax_exchange = None

    @classmethod
    def from_tli(cls, tlifiles, atm, grid, *, nlor=100, ndop=50, extent=300.0, cutoff=25.0,
                 dlratio=0.1, lorentz=None, doppler=None, tmin=100.0, tmax=3000.0,
                 ethresh=1e-30, maxdepth=10.0, skip_species=(), iso_numbering='file', **kw):
        """TLI file(s) + atmosphere + spectral grid -> a model ready to run(): what
        Line_By_Line.__init__ / Voigt.__init__ assemble before the reference's first extinction
        call (pyratbay/pyrat/line_by_line.py:120-200, pyrat/voigt.py:20-149), with nothing taken
        from a fixture -- lines and isotope data from the file(s) (tli.read_tli on the grid's
        range, databases concatenated in file order), isotope -> species indices by molecule
        name, Z_i(T_layer) by tli's restatement of the reference's interp1d, Voigt width grids
        from the atmosphere (or given: the reference's voigt_dmin/dmax/lmin/lmax keys).

        iso_numbering: how the lines of a file with SEVERAL databases find their isotope.  The
        file stores each line's isotope index relative to its own database (lread.py:181-209,
        309).  'file' (default): numbered over the file's databases, i.e. every line gets its own
        isotope.  'reference': as Line_By_Line does (line_by_line.py:114-119: the stored index +
        the isotope count of the previous FILES) -- in a multi-database file the lines of the
        second database then use the first database's isotope data, and the list steps back in
        wavenumber within an isotope id, which pb_lines_create refuses (the reference's result
        on such a list depends on its one-way Doppler-index search; fixture G16, run `onefile`,
        is pinned by the CPU-side checker only).  One database per file, the layout of the reference's
        own configurations, is the same either way.

        atm: dict with temp[L], dens[L, nspecies] (cm-3), radius[L], press[L] (bar; for the width
        grids), species (names), mol_mass, mol_radius (cm), rstar.  grid: synth.spectral_grid /
        resolution_grid / wlstep_grid (wn, own, ownstep, onwave, wnosamp, divisors, wnlow,
        wnhigh)."""
        from . import synth, tli
        paths = [tlifiles] if isinstance(tlifiles, (str, bytes, os.PathLike)) else list(tlifiles)
        species = list(atm['species'])
        dbs, lwn, gf, elow, lid = [], [], [], [], []
        niso = 0
        # the reference selects the lines of [spec.wnlow, spec.wnhigh] (pyrat/opacity.py:46-47,
        # 105): the CONFIGURED boundaries -- wnhigh can lie up to one step above wn[-1], and a line
        # in between still throws its wing onto the grid
        wn_lo = float(grid.get('wnlow', grid['wn'][0]))
        wn_hi = float(grid.get('wnhigh', grid['wn'][-1]))
        for path in paths:
            d, wn_, gf_, el_, stored, meta = tli.read_tli(path, wn_lo, wn_hi)
            dbs += d
            lwn.append(wn_); gf.append(gf_); elow.append(el_)
            if iso_numbering == 'reference':
                lid.append(stored.astype(np.int32) + niso)
            elif iso_numbering == 'file':
                lid.append(meta['iso_global'].astype(np.int32) + niso)
            else:
                raise ValueError("iso_numbering: 'file' or 'reference'")
            niso += sum(len(db['isotopes']) for db in d)
        isoimol, isomass, isoratio = [], [], []
        for db in dbs:
            if db['molecule'] not in species:
                raise ValueError(f"The species '{db['molecule']}' is not present in the "
                                 'atmosphere, required for LBL calculation')
            isoimol += [species.index(db['molecule'])] * len(db['isotopes'])
            isomass += list(db['iso_mass'])
            isoratio += list(db['iso_ratio'])
        isoimol = np.asarray(isoimol, np.int32)
        # rows of the un-added extinction: one per line-carrying species, in np.unique's order
        # (line_by_line.py:177-188); skip_species flags their isotopes -1 (extinction.py:165-168)
        carriers = sorted({species[i] for i in isoimol})
        isoiext = np.asarray([carriers.index(species[i]) for i in isoimol], np.int32)
        for name in skip_species:
            if name in carriers:
                isoiext[isoiext == carriers.index(name)] = -1
        iso = dict(isoimol=isoimol, isomass=np.asarray(isomass, float),
                   isoratio=np.asarray(isoratio, float), isoiext=isoiext,
                   isoz=tli.iso_partition(dbs, atm['temp']))
        if lorentz is None or doppler is None:
            used = np.unique(isoimol)
            lor, dop = synth.voigt_widths(grid['wn'], atm['press'],
                                          np.asarray(atm['mol_mass'])[used],
                                          np.asarray(atm['mol_radius'])[used], nlor, ndop,
                                          tmin, tmax)
            lorentz = lor if lorentz is None else lorentz
            doppler = dop if doppler is None else doppler
        lorentz, doppler = np.asarray(lorentz, float), np.asarray(doppler, float)
        size = synth.voigt_sizes(lorentz, doppler, extent, cutoff, grid['ownstep'],
                                 grid['onwave'], dlratio)
        atm = dict(atm)
        atm['nlayers'] = len(atm['temp'])
        case = dict(grid=grid, atm=atm, iso=iso,
                    lines=dict(lwn=np.concatenate(lwn), elow=np.concatenate(elow),
                               gf=np.concatenate(gf), lid=np.concatenate(lid)),
                    voigt=dict(lorentz=lorentz, doppler=doppler, size=size, extent=extent,
                               cutoff=cutoff, dlratio=dlratio),
                    ethresh=ethresh, maxdepth=maxdepth)
        model = cls(case, **kw)
        model.partition = PartitionTable(dbs)
        model.databases = dbs
        return model

    def set_atmosphere(self, temp, dens, isoz=None, radius=None, continuum_density=None):
        """New temperature / number-density / partition-function (and radius) profiles for the
        next run().  isoz=None (models made by from_tli): Z_i(T) is interpolated from the file's
        tables at the new temperatures on the device, as the reference does on every extinction
        call (line_by_line.py:219-222); a temperature outside a table raises ValueError.  With a
        Continuum attached pass its number densities {species: n[L]} too: every opacity term of
        the next run then sees the SAME atmosphere."""
        self.temp_host = np.array(temp.cpu().numpy() if isinstance(temp, torch.Tensor) else temp,
                                  float)
        self.temp.copy_(dev(temp))
        self.dens.copy_(dev(dens))
        if isoz is not None:
            self.isoz.copy_(dev(isoz))
        elif self.partition is not None:
            self.partition.evaluate(self.temp, out=self.isoz)
        else:
            raise _capi.PbError('set_atmosphere: pass isoz[niso, L] (this model has no '
                                'partition-function tables: it was not made by from_tli)')
        if continuum_density is not None:
            self.continuum_density = continuum_density
        elif self.continuum is not None:
            raise _capi.PbError('set_atmosphere: this model has continuum terms, pass their '
                                'number densities (continuum_density) with the new atmosphere')
        if radius is not None:
            self.radius.copy_(dev(radius))
            if self.rt_path == 'transit':
                self.raypath.copy_(dev(pack_raypath(transit_path(radius, self.itop),
                                                    self.itop)))
            else:
                self.intervals.copy_(dev(-np.diff(radius)))

    def extinction(self):
        if self.resolution:
            self.ec.zero_()              # the interpolating kernel adds to what it finds
        if self.kmax_exchange is not None and not self.resolution:
            # (`resolution` mode: the dynamic-grid path takes the maxima over every line itself
            # and a shard equals the slice of the whole call bit for bit -- no exchange)
            # wavenumber shard of a multi-GPU run: every rank derives the records (and the
            # strengths, the exp() work) of its own groups only; the per-row maxima that set
            # the ethresh threshold are made global by ONE small all-reduce(MAX)
            self.lbl.extinction_begin(self.temp, self.dens, self.isoz, add=True, out=self.ec,
                                      wbegin=self.wbegin, wcount=self.wcount)
            self.kmax_exchange(self.lbl.kmax_tensor())
            self.lbl.extinction_end()
        else:
            self.lbl.extinction(self.temp, self.dens, self.isoz, add=True, out=self.ec,
                                wbegin=self.wbegin, wcount=self.wcount)
        if self.continuum is not None:
            self.continuum.add(self.ec.view(self.nlayers, self.wcount), self.temp_host,
                               self.continuum_density)
        return self.ec

    def optical_depth(self):
        ec = self.ec.view(self.nlayers, self.wcount)
        if self.rt_path == 'transit':
            self.depth, self.ideep = optical_depth_transit(
                ec, self.raypath, self.itop, self.nlayers, self.maxdepth)
        else:
            self.depth, self.ideep = plane_parallel_optical_depth(
                ec, self.intervals, self.itop, self.nlayers, self.maxdepth)
        return self.depth, self.ideep

    def rt(self):
        if self.rt_path == 'transit':
            self.spectrum = transmission(self.depth, self.ideep, self.radius, self.itop,
                                         self.rstar)
        elif self.rt_path == 'two_stream':
            self.flux_down, self.flux_up = two_stream(self.depth, self.wn, self.temp,
                                                      self.f_int, self.flux_top, self.itop)
            self.spectrum = self.flux_up[0]
        else:
            self.spectrum = emission_flux(self.depth, self.ideep, self.wn, self.temp,
                                          self.mu, self.weights, self.itop)
        if self.rt_path != 'transit':
            # f_dilution, eclipse ratio (pyrat/spectrum.py:394-405); 'f_lambda' stays in
            # erg s-1 cm-2 cm here as in the reference's run(): observed() converts
            kind = 'eclipse' if self.observable == 'eclipse' else 'emission'
            self.spectrum, self.fplanet = emission_observables(
                self.spectrum, kind, self.starflux, self.rplanet, self.rstar, self.f_dilution,
                in_place=self.rt_path != 'two_stream')    # (flux_up[0] stays what two_stream made)
        return self.spectrum

    def get_ec(self, layer):
        """Pyrat.get_ec(layer) for the line-by-line model (pyrat_obj.py:700-719 ->
        line_by_line.py:224-230): the cross sections of ONE layer per species (`add = 0`,
        extinction.py:155-158) times that species' number density -> (ec[nspec, wcount] in cm-1 on
        the device, labels).  A species is a row of `isoiext`; its label is atm['species'] of the
        molecule its isotopes belong to (the row index when the case names none).  (The reference
        multiplies every row by `density[layer]` of ALL the model's species at once, which only
        broadcasts for a single-species model; here each row takes its own species' density.)"""
        atm, iso = self.case['atm'], self.case['iso']
        layer = int(layer)
        if not 0 <= layer < self.nlayers:
            raise _capi.PbError(f'get_ec: layer {layer} outside 0 ... {self.nlayers - 1}')
        sl = slice(layer, layer + 1)
        ec = self.lbl.extinction(self.temp[sl], self.dens[sl].contiguous(),
                                 self.isoz[:, sl].contiguous(), add=False, wbegin=self.wbegin,
                                 wcount=self.wcount)[0]
        isoiext = np.asarray(iso['isoiext'])
        isoimol = np.asarray(iso['isoimol'])
        imol = [int(isoimol[np.flatnonzero(isoiext == r)[0]]) if np.any(isoiext == r) else -1
                for r in range(ec.shape[0])]
        dens = self.dens[layer]
        scale = torch.stack([dens[m] if m >= 0 else torch.zeros_like(dens[0]) for m in imol])
        names = atm.get('species')
        labels = [str(names[m]) if names is not None and m >= 0 else str(r)
                  for r, m in enumerate(imol)]
        # ec[r, :] *= scale[r] (pb_band_scale with the rows as its 'walkers')
        call('pb_band_scale', _ptr(ec), None, _ptr(scale.contiguous()), ec.shape[1], ec.shape[0],
             _stream())
        return ec, labels

    def observed(self):
        """The last spectrum as eval() returns it (pyrat_obj.py:323-329): rt_path 'f_lambda'
        converts the planet's flux to W m-2 um-1 at `distance`; every other path: `spectrum`."""
        if self.observable != 'f_lambda':
            return self.spectrum
        return emission_observables(self.fplanet, 'f_lambda', rplanet=self.rplanet, wn=self.wn,
                                    distance=self.distance)[0]

    def capture(self):
        """Capture one run() into a HIP graph (torch.cuda.CUDAGraph on a side stream) and
        return a replay function: the whole step -- layer state, records, gather, optical
        depth, spectrum -- is then ONE graph launch, with inputs read from and outputs
        written to the same device buffers (update the atmosphere with set_atmosphere()).
        The first call allocates workspaces, so it runs once eagerly before the capture.
        The `resolution` mode's dynamic-grid path needs predict_runs=True: its launches depend on
        the layers' oversampling factors, which the default form reads back in every call; the
        captured plan is the one of the atmosphere at capture time, and layers of a later
        atmosphere that it does not fit are computed by the direct gather inside the graph."""
        if self.resolution and self.lbl.gather_mode == 'dynamic' and not self.predict_runs:
            raise RuntimeError("capture(): the dynamic-grid path of the `resolution` mode reads "
                               "the layers' factors back on every call and cannot be captured; "
                               "LBLSpectrum(..., predict_runs=True) plans its calls from the last "
                               "read-back instead, lbl.set_gather_mode('auto') selects the direct "
                               "gather")
        self.run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.run()                         # warm-up on the capture stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                out = self.run()
        torch.cuda.current_stream().wait_stream(side)
        self._graph = graph

        def replay():
            graph.replay()
            return out
        return replay

    def run(self):
        """One spectrum: the 'extinction', 'odepth' and 'spectrum' stages (the last two
        in one library call for the transit geometry, which marks their boundary itself)."""
        t = self._timer
        if t is not None:
            t.start('extinction')
        self.extinction()
        if t is not None:
            t.mark('extinction', 'odepth')
        if self.rt_path == 'transit' and not self.materialize_depth:
            if t is not None:
                t.mark('odepth', 'spectrum')        # (no separate stage: counted under 'spectrum')
            self.depth = self.ideep = None
            self.spectrum = transit_spectrum_batch(
                self.ec.view(1, self.nlayers, self.wcount), self.raypath.view(1, -1),
                self.radius.view(1, -1), self.rstar, self.itop, self.nlayers, self.maxdepth)[0]
            if t is not None:
                t.mark('spectrum')
            return self.spectrum
        if self.rt_path == 'transit':
            self.spectrum, self.depth, self.ideep = transit_spectrum(
                self.ec.view(self.nlayers, self.wcount), self.raypath, self.radius,
                self.rstar, self.itop, self.nlayers, self.maxdepth, out=self.spectrum_out)
            if t is not None:
                t.mark('spectrum')
            return self.spectrum
        self.optical_depth()
        if t is not None:
            t.mark('odepth', 'spectrum')
        out = self.rt()
        if t is not None:
            t.mark('spectrum')
        return out

    @property
    def timestamps(self):
        """Seconds of the last run() by stage, with the reference's keys 'extinction',
        'odepth', 'spectrum' (pyrat_obj.py:203-214).  Waits for that run to finish."""
        if self._timer is None:
            raise _capi.PbError('this model was built with timestamps=False')
        return self._timer.read()


class SpectrumPipeline:
    """Consecutive, independent spectra of one line-by-line model kept in flight on `depth` HIP
    streams (default 2): spectrum i+1 starts while spectrum i is still finishing.

    Why: one spectrum of C2 is a chain of launches whose dominant one, the extinction gather,
    runs ~2000 workgroups of 0.3-0.7 ms on 1024 slots -- its last fifth is a tail in which most
    of the chip idles (measured: 79 % of the slot-time busy), and the small launches around it
    (layer state, records, ray paths, depth, spectrum) cannot fill a chip either.  A second
    spectrum on another stream fills those holes: +19 % spectra/s at C2 on one MI355X.  The
    callers this serves compute many independent spectra anyway: the temperature loop of
    `compute_opacity` (pyrat/extinction.py:100-122), the walkers of a retrieval.

    Every context has its own plan (records, per-layer state, ec, depth) and shares the Voigt
    table and the line list, which a run only reads.  A context's output buffers are reused by
    its next submit(): consume (or copy) a result before submitting `depth` more spectra.
    Results are bit-identical to LBLSpectrum.run() of the same atmosphere
    (tests/test_gpu_pipeline.py::test_spectrum_pipeline_equals_serial_runs)."""

    def __init__(self, case, depth=2, **kw):
        require_gpu()
        first = LBLSpectrum(case, **kw)
        kw = dict(kw, voigt=first.voigt, lines=first.lines)
        self.models = [first] + [LBLSpectrum(case, **kw) for _ in range(depth - 1)]
        for m in self.models:
            m.lbl.set_concurrency(depth)
        self.streams = side_streams(depth)
        self.done = [None] * depth          # completion event of each context's last spectrum
        self.count = 0

    @property
    def depth(self):
        return len(self.models)

    def submit(self, atmosphere=None):
        """Enqueue one spectrum (optionally of a new atmosphere: the arguments of
        LBLSpectrum.set_atmosphere as a tuple or dict) and return (spectrum, event): the
        device tensor is complete once `event` has fired (flush() waits for all of them)."""
        j = self.count % len(self.models)
        self.count += 1
        model, stream = self.models[j], self.streams[j]
        caller = torch.cuda.current_stream()
        if not caller.query():                              # (an idle stream has nothing to wait for)
            stream.wait_stream(caller)                      # inputs made on the caller's stream
        with torch.cuda.stream(stream):
            if isinstance(atmosphere, dict):
                model.set_atmosphere(**atmosphere)
            elif atmosphere is not None:
                model.set_atmosphere(*atmosphere)
            out = model.run()
            event = torch.cuda.Event()
            event.record(stream)
        # the result was allocated on the side stream and will be read on the caller's: keep the
        # caching allocator from handing its memory out again before the caller's reads are done
        out.record_stream(caller)
        self.done[j] = event
        return out, event

    def flush(self):
        """Make the caller's stream wait for every spectrum submitted so far."""
        cur = torch.cuda.current_stream()
        for event in self.done:
            if event is not None:
                cur.wait_event(event)
